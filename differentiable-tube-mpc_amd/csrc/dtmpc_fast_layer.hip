// dtmpc_fast_layer.hip — the backward of the differentiable iLQR solve (dtmpc_solve_backward): the reference's
// ddp_sensitivity (core/ddp.py:317-427) for ARBITRARY upper gradients gX / gU and both cost kinds, fused with the
// accumulation of ift_gradient (core/ift.py:35-92) restricted to the PLAIN cost weights and the references.  None of
// those terms involves delta_lambda (only the DBaS parameters alpha, gamma and the tightening enter f_hat), so the
// kernel keeps neither V_xx nor tilde V_x per step and no sensitivity tape (dX, dU, dlam) touches HBM:
//   backward k = N-1 .. 0: K_k, k_ff,k from sensitivity<M>'s recursion (dtmpc_fast.hip) with tilde Q_x = gX_k + A^T
//     tilde V_x, tilde Q_u = gU_k + B^T tilde V_x; stored with the nine off-identity A / B entries and the active mask
//     (20 values, 80 B per step and trajectory);
//   forward k = 0 .. N: delta x_k, delta u_k formed in registers and contracted at once into
//     g_Q  += 2 (x_k - r_k) dx_k     g_R += 2 (u_k - ubar_k) du_k     g_qb += 2 b_k db_k      (k < N)
//     g_Qf  = 2 (x_N - r_N) dx_N     g_qb += 2 b_N db_N
//     g_xref[k] = -2 Q dx_k (Qf at k = N), g_uref[k] = -2 R du_k;   g_target = sum_k g_xref[k]
//   (oracle/oracle_general.h ift1's lines without the softplus factors).
// One lane per trajectory, compile-time obstacle count M (1..8) and cost kind.  The ABI arrays are SoA [row][field][B]:
// a wave's loads of one field are one 256 B line, so they are read in place, and the workspace has the same form
// ([N][20][B]); every access is a 32-bit load / store.  Bytes per trajectory and step by construction: backward 44 read
// (X 12, U 8, gX 16, gU 8) + 80 written, forward 80 + 24 read (target cost: 228 B), a tracking cost 20 more read
// (Xref 12, Uref 8) and up to 20 written (g_xref, g_uref): 268 B.  Storing the linearisation is sensitivity<M>'s
// choice; recomputing it in the forward sweep (sin / cos, h_grad, B': ~120 instructions against 80 B) is unmeasured.
// The device functions are dtmpc_fast.hip's (h_grad, dbarrier, jac, vsincos, scene_p, scene_tg, pin_p) and
// dtmpc_device.hpp / dtmpc_solver.hpp's (sens_qblocks, lu2, solve_reduced); nothing is restated here.
#define DTMPC_FAST_LAYER_TU 1
#include "dtmpc_fast.hip"

namespace dtmpc {
namespace fk {

constexpr int kLayerRec = 20;  // workspace values per step: K (8), k_ff (2), a02 a12 a30 a31 a32 b00 b10 b30 b31, mask

struct LArgs {
  int B;
  const real* X;     // [N+1][4][B]
  const real* U;     // [N][2][B]
  const real* Xr;    // [N+1][3][B] (tracking cost)
  const real* Ur;    // [N][2][B]
  const real* sc;    // [3M+3][B] or NULL
  const real* gX;    // [N+1][4][B]
  const real* gU;    // [N][2][B]
  real* gw;          // [9][B]
  real* gt;          // [3][B] or NULL (target cost)
  real* gxr;         // [N+1][3][B] or NULL (tracking cost)
  real* gur;         // [N][2][B] or NULL
  real* work;        // [N][kLayerRec][B]
  int* status;       // [B]
};
struct LK {
  FP p;  // first, as in every fused kernel's argument block
  FCost c;
  LArgs a;
};

// one step's inputs of the backward pass / of the forward sweep, loaded one step ahead of their use
struct LBwdIn {
  real x0, x1, x2, u0, u1, g0, g1, g2, g3, h0, h1;
};
struct LFwdIn {
  real K[8], kf[2], A[9], act, x[4], u[2], r[3], q[2];
};

template <int M, bool TRACK>
__global__ void __launch_bounds__(kBlock) solve_backward_kernel(LK kk) {
  const LArgs& a = kk.a;
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= a.B) return;
  const size_t nb = (size_t)a.B;
  FP p = kk.p;
  FCost c = kk.c;
  if (a.sc) {  // per-trajectory scene: this trajectory's obstacles and, for the target cost, its target
    p = scene_p<M>(p, a.sc, nb, i);
    if (!TRACK) c.tg = scene_tg<M>(a.sc, nb, i);
  }
  p = pin_p<M>(p);
  const int N = p.N;
  const real* X = a.X + i;
  const real* U = a.U + i;
  const real* GX = a.gX + i;
  const real* GU = a.gU + i;
  real* W = a.work + i;
  const real lxx[4] = {2.f * c.Q0, 2.f * c.Q1, 2.f * c.Q2, 2.f * c.qb};
  const real luu[2] = {2.f * c.R0, 2.f * c.R1};
  const real pxx[4] = {2.f * c.Qf0, 2.f * c.Qf1, 2.f * c.Qf2, 2.f * c.qb};
  const real reg = 1e-9f;
  Riccati<real> R;  // R.Vx holds tilde V_x
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int j = 0; j < 4; ++j) R.Vxx[r][j] = r == j ? pxx[r] : 0.f;
    R.Vx[r] = GX[(size_t)(4 * N + r) * nb];
  }
  real gxn, gyn, dBn;
  dBn = dbarrier(p, h_grad<M>(p, X[(size_t)(4 * N) * nb], X[(size_t)(4 * N + 1) * nb], gxn, gyn));
  auto bload = [&](LBwdIn& L, int k) {
    L.x0 = X[(size_t)(4 * k) * nb];
    L.x1 = X[(size_t)(4 * k + 1) * nb];
    L.x2 = X[(size_t)(4 * k + 2) * nb];
    L.u0 = U[(size_t)(2 * k) * nb];
    L.u1 = U[(size_t)(2 * k + 1) * nb];
    L.g0 = GX[(size_t)(4 * k) * nb];
    L.g1 = GX[(size_t)(4 * k + 1) * nb];
    L.g2 = GX[(size_t)(4 * k + 2) * nb];
    L.g3 = GX[(size_t)(4 * k + 3) * nb];
    L.h0 = GU[(size_t)(2 * k) * nb];
    L.h1 = GU[(size_t)(2 * k + 1) * nb];
  };
  LBwdIn Bn;
  bload(Bn, N - 1);
  for (int k = N - 1; k >= 0; --k) {
    const LBwdIn L = Bn;
    if (k > 0) bload(Bn, k - 1);
    real sn, cs;
    vsincos(L.x2, sn, cs);
    real gxk, gyk;
    const real dBk = dbarrier(p, h_grad<M>(p, L.x0, L.x1, gxk, gyk));
    const Jac<real> J = jac(p, sn, cs, L.u0, gxk, gyk, dBk, gxn, gyn, dBn);
    gxn = gxk;
    gyn = gyk;
    dBn = dBk;
    real Qxx[4][4], Qxu[4][2], Qux[2][4], Quu[2][2];
    sens_qblocks(J, R.Vxx, lxx, luu, Qxx, Qxu, Qux, Quu);
    const real* tv = R.Vx;
    // tilde Q_u = g_u + B^T tilde V_x ; tilde Q_x = g_x + A^T tilde V_x   (:383-384)
    const real tQu0 = L.h0 + (J.b00 * tv[0] + J.b10 * tv[1] + J.b30 * tv[3]);
    const real tQu1 = L.h1 + (J.b21 * tv[2] + J.b31 * tv[3]);
    real tQx[4];
    tQx[0] = L.g0 + (tv[0] + J.a30 * tv[3]);
    tQx[1] = L.g1 + (tv[1] + J.a31 * tv[3]);
    tQx[2] = L.g2 + (J.a02 * tv[0] + J.a12 * tv[1] + tv[2] + J.a32 * tv[3]);
    tQx[3] = L.g3 + J.g * tv[3];
    const bool act0 = (L.u0 <= p.umin0 + p.active_tol) || (L.u0 >= p.umax0 - p.active_tol);
    const bool act1 = (L.u1 <= p.umin1 + p.active_tol) || (L.u1 >= p.umax1 - p.active_tol);
    const real m00 = Quu[0][0] + reg, m11 = Quu[1][1] + reg;
    const LU2<real> f = lu2(m00, Quu[0][1], Quu[1][0], m11);
    real Kk[8], kf[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      real y0, y1;
      solve_reduced(f, m00, m11, act0, act1, Qux[0][j], Qux[1][j], y0, y1);
      Kk[j] = -y0;
      Kk[4 + j] = -y1;
    }
    {
      real y0, y1;
      solve_reduced(f, m00, m11, act0, act1, tQu0, tQu1, y0, y1);
      kf[0] = -y0;
      kf[1] = -y1;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      R.Vx[r] = tQx[r] + (Qxu[r][0] * kf[0] + Qxu[r][1] * kf[1]);
#pragma unroll
      for (int j = 0; j < 4; ++j) R.Vxx[r][j] = Qxx[r][j] + (Qxu[r][0] * Kk[j] + Qxu[r][1] * Kk[4 + j]);
    }
    real* w = W + (size_t)(kLayerRec * k) * nb;
#pragma unroll
    for (int j = 0; j < 8; ++j) w[(size_t)j * nb] = Kk[j];
    w[(size_t)8 * nb] = kf[0];
    w[(size_t)9 * nb] = kf[1];
    w[(size_t)10 * nb] = J.a02;
    w[(size_t)11 * nb] = J.a12;
    w[(size_t)12 * nb] = J.a30;
    w[(size_t)13 * nb] = J.a31;
    w[(size_t)14 * nb] = J.a32;
    w[(size_t)15 * nb] = J.b00;
    w[(size_t)16 * nb] = J.b10;
    w[(size_t)17 * nb] = J.b30;
    w[(size_t)18 * nb] = J.b31;
    w[(size_t)19 * nb] = real((act0 ? 1 : 0) + (act1 ? 2 : 0));
  }
  // forward (:413-425) fused with the accumulation
  const real* XR = TRACK ? a.Xr + i : nullptr;
  const real* UR = TRACK ? a.Ur + i : nullptr;
  real* GXR = TRACK && a.gxr ? a.gxr + i : nullptr;
  real* GUR = TRACK && a.gur ? a.gur + i : nullptr;
  auto fload = [&](LFwdIn& F, int k) {
    const real* w = W + (size_t)(kLayerRec * k) * nb;
#pragma unroll
    for (int j = 0; j < 8; ++j) F.K[j] = w[(size_t)j * nb];
    F.kf[0] = w[(size_t)8 * nb];
    F.kf[1] = w[(size_t)9 * nb];
#pragma unroll
    for (int j = 0; j < 9; ++j) F.A[j] = w[(size_t)(10 + j) * nb];
    F.act = w[(size_t)19 * nb];
#pragma unroll
    for (int j = 0; j < 4; ++j) F.x[j] = X[(size_t)(4 * k + j) * nb];
    F.u[0] = U[(size_t)(2 * k) * nb];
    F.u[1] = U[(size_t)(2 * k + 1) * nb];
    if (TRACK) {
#pragma unroll
      for (int j = 0; j < 3; ++j) F.r[j] = XR[(size_t)(3 * k + j) * nb];
      F.q[0] = UR[(size_t)(2 * k) * nb];
      F.q[1] = UR[(size_t)(2 * k + 1) * nb];
    } else {
      F.r[0] = c.tg.x;
      F.r[1] = c.tg.y;
      F.r[2] = c.tg.z;
      F.q[0] = F.q[1] = 0.f;
    }
  };
  real d[4] = {0.f, 0.f, 0.f, 0.f};
  real gQ[3] = {0.f, 0.f, 0.f}, gR[2] = {0.f, 0.f}, gqb = 0.f, gT[3] = {0.f, 0.f, 0.f};
  const real Qw[3] = {c.Q0, c.Q1, c.Q2}, Rw[2] = {c.R0, c.R1}, Qfw[3] = {c.Qf0, c.Qf1, c.Qf2};
  const real g = p.gamma, dt = p.dt;
  bool ok = true;
  LFwdIn Fn;
  fload(Fn, 0);
  for (int k = 0; k < N; ++k) {
    const LFwdIn F = Fn;
    if (k + 1 < N) fload(Fn, k + 1);
    const int act = (int)F.act;
    const real v0 = (act & 1) ? 0.f : F.kf[0] + (F.K[0] * d[0] + F.K[1] * d[1] + F.K[2] * d[2] + F.K[3] * d[3]);
    const real v1 = (act & 2) ? 0.f : F.kf[1] + (F.K[4] * d[0] + F.K[5] * d[1] + F.K[6] * d[2] + F.K[7] * d[3]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      gQ[j] += 2.f * (F.x[j] - F.r[j]) * d[j];
      const real gr = -(2.f * Qw[j]) * d[j];
      if (TRACK) {
        if (GXR) GXR[(size_t)(3 * k + j) * nb] = gr;
        ok = ok && finite(gr);
      } else {
        gT[j] += gr;
      }
    }
    gR[0] += 2.f * (F.u[0] - F.q[0]) * v0;
    gR[1] += 2.f * (F.u[1] - F.q[1]) * v1;
    gqb += 2.f * F.x[3] * d[3];
    if (TRACK) {
      const real h0 = -(2.f * Rw[0]) * v0, h1 = -(2.f * Rw[1]) * v1;
      if (GUR) {
        GUR[(size_t)(2 * k) * nb] = h0;
        GUR[(size_t)(2 * k + 1) * nb] = h1;
      }
      ok = ok && finite(h0) && finite(h1);
    }
    // delta x_{k+1} = A delta x_k + B delta u_k
    const real a02 = F.A[0], a12 = F.A[1], a30 = F.A[2], a31 = F.A[3], a32 = F.A[4], b00 = F.A[5], b10 = F.A[6],
               b30 = F.A[7], b31 = F.A[8];
    const real n0 = (d[0] + a02 * d[2]) + b00 * v0;
    const real n1 = (d[1] + a12 * d[2]) + b10 * v0;
    const real n2 = d[2] + dt * v1;
    const real n3 = (a30 * d[0] + a31 * d[1] + a32 * d[2] + g * d[3]) + (b30 * v0 + b31 * v1);
    d[0] = n0;
    d[1] = n1;
    d[2] = n2;
    d[3] = n3;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) ok = ok && finite(d[j]);
  real gQf[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const real xn = X[(size_t)(4 * N + j) * nb];
    const real rn = TRACK ? XR[(size_t)(3 * N + j) * nb] : (j == 0 ? c.tg.x : j == 1 ? c.tg.y : c.tg.z);
    gQf[j] = 2.f * (xn - rn) * d[j];
    const real gr = -(2.f * Qfw[j]) * d[j];
    if (TRACK) {
      if (GXR) GXR[(size_t)(3 * N + j) * nb] = gr;
      ok = ok && finite(gr);
    } else {
      gT[j] += gr;
    }
  }
  gqb += 2.f * X[(size_t)(4 * N + 3) * nb] * d[3];
  real* GW = a.gw + i;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    GW[(size_t)j * nb] = gQ[j];
    GW[(size_t)(5 + j) * nb] = gQf[j];
    ok = ok && finite(gQ[j]) && finite(gQf[j]);
  }
  GW[(size_t)3 * nb] = gR[0];
  GW[(size_t)4 * nb] = gR[1];
  GW[(size_t)8 * nb] = gqb;
  ok = ok && finite(gR[0]) && finite(gR[1]) && finite(gqb);
  if (!TRACK) {
    if (a.gt) {
#pragma unroll
      for (int j = 0; j < 3; ++j) a.gt[(size_t)j * nb + i] = gT[j];
    }
    ok = ok && finite(gT[0]) && finite(gT[1]) && finite(gT[2]);
  }
  if (!ok) a.status[i] |= DTMPC_ST_NONFINITE;
}

}  // namespace fk

// ---------------------------------------------------------------------------------------------
// host side
static const char* layer_unsupported(int dtype, const dtmpc_spec* sp, const dtmpc_cost* c) {
  if (!sp || !c) return "solve backward: NULL spec or cost";
  if (dtype != DTMPC_F32) return "solve backward: f32 only";
  if (sp->obs_aggregation != DTMPC_OBS_SMOOTHMIN) return "solve backward: smooth-min obstacle aggregation only";
  if (sp->n_obstacles < 1 || sp->n_obstacles > 8) return "solve backward: 1 to 8 obstacles";
  if (sp->barrier_type != DTMPC_BARRIER_INVERSE) return "solve backward: relaxed inverse barrier only";
  if (sp->h_offset != 0.0) return "solve backward: h_offset must be 0";
  if (c->wrap_angle) return "solve backward: no wrapped heading error";
  return nullptr;
}

static size_t layer_workspace_bytes(int32_t N, int64_t B) {
  return (size_t)N * fk::kLayerRec * sizeof(real) * (size_t)B;
}

static int launch_solve_backward(const dtmpc_spec* sp, const dtmpc_cost* cp, int64_t B, const fk::LArgs& a,
                                 hipStream_t st) {
  fk::LK kk;
  std::memset(&kk, 0, sizeof(kk));
  fast_p(sp, kk.p);
  const DCost<real> c = make_cost<real>(*cp);
  const bool track = cp->kind == DTMPC_COST_TRACK;
  kk.c = fk::FCost{c.Q0, c.Q1, c.Q2, c.R0, c.R1, c.Qf0, c.Qf1, c.Qf2, c.qb,
                   track ? fk::f4{0.f, 0.f, 0.f, 0.f} : fk::f4{c.t0, c.t1, c.t2, 0.f}};
  kk.a = a;
  const int bs = tube_block(B, 1);
  const dim3 grid((unsigned)((B + bs - 1) / bs));
#define LY_LAUNCH(m, t) hipLaunchKernelGGL((fk::solve_backward_kernel<m, t>), grid, dim3(bs), 0, st, kk)
#define LY_CASE(m) \
  case m:          \
    if (track) LY_LAUNCH(m, true); else LY_LAUNCH(m, false); \
    break;
  switch (sp->n_obstacles) {
#ifdef DTMPC_FAST_M_ONLY
    LY_CASE(DTMPC_FAST_M_ONLY)
#else
    LY_CASE(1) LY_CASE(2) LY_CASE(3) LY_CASE(4) LY_CASE(5) LY_CASE(6) LY_CASE(7) LY_CASE(8)
#endif
    default: return set_err(DTMPC_ERR_BAD_ARG, "solve backward: obstacle count not instantiated");
  }
#undef LY_CASE
#undef LY_LAUNCH
  return check_launch("solve_backward_kernel");
}

}  // namespace dtmpc

extern "C" {

int32_t dtmpc_solve_backward_supported(int dtype, const dtmpc_spec* spec, const dtmpc_cost* cost) {
  return dtmpc::layer_unsupported(dtype, spec, cost) ? 0 : 1;
}

size_t dtmpc_solve_backward_workspace_bytes(int dtype, int32_t horizon, int64_t B) {
  if (dtype != DTMPC_F32 || horizon < 1 || B < 1) return 0;
  return dtmpc::layer_workspace_bytes(horizon, B);
}

int dtmpc_solve_backward(int dtype, const dtmpc_spec* spec, const dtmpc_cost* cost, int64_t B, const void* X,
                         const void* U, const void* Xref, const void* Uref, const void* scenes, const void* gX,
                         const void* gU, void* g_w, void* g_target, void* g_xref, void* g_uref, void* work,
                         size_t work_bytes, int32_t* status, void* stream) {
  using namespace dtmpc;
  if (!spec || !cost) return set_err(DTMPC_ERR_BAD_ARG, "solve backward: NULL spec or cost");
  if (B < 1) return set_err(DTMPC_ERR_BAD_ARG, "solve backward: batch must be >= 1");
  if (spec->horizon < 1) return set_err(DTMPC_ERR_BAD_ARG, "solve backward: horizon must be >= 1");
  if (int r = check_spec(spec, B)) return r;
  if (cost->kind != DTMPC_COST_TARGET && cost->kind != DTMPC_COST_TRACK)
    return set_err(DTMPC_ERR_BAD_ARG, "solve backward: bad cost kind");
  if (const char* why = layer_unsupported(dtype, spec, cost)) return set_err(DTMPC_ERR_BAD_ARG, why);
  if (!X || !U || !gX || !gU || !g_w || !status)
    return set_err(DTMPC_ERR_BAD_ARG, "solve backward: NULL X, U, gX, gU, g_w or status");
  if (cost->kind == DTMPC_COST_TRACK) {
    if (!Xref || !Uref) return set_err(DTMPC_ERR_BAD_ARG, "solve backward: the tracking cost needs Xref and Uref");
    if (g_target) return set_err(DTMPC_ERR_BAD_ARG, "solve backward: g_target goes with the target cost");
  } else if (Xref || Uref || g_xref || g_uref) {
    return set_err(DTMPC_ERR_BAD_ARG, "solve backward: Xref, Uref, g_xref and g_uref go with the tracking cost");
  }
  if (!work || work_bytes < layer_workspace_bytes(spec->horizon, B))
    return set_err(DTMPC_ERR_BAD_ARG, "solve backward: work_bytes < dtmpc_solve_backward_workspace_bytes(...)");
  fk::LArgs a;
  a.B = (int)B;
  a.X = (const real*)X;
  a.U = (const real*)U;
  a.Xr = (const real*)Xref;
  a.Ur = (const real*)Uref;
  a.sc = (const real*)scenes;
  a.gX = (const real*)gX;
  a.gU = (const real*)gU;
  a.gw = (real*)g_w;
  a.gt = (real*)g_target;
  a.gxr = (real*)g_xref;
  a.gur = (real*)g_uref;
  a.work = (real*)work;
  a.status = status;
  return launch_solve_backward(spec, cost, B, a, (hipStream_t)stream);
}

}  // extern "C"
