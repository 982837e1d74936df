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
// GEOM variant (dtmpc_solve_backward_geom, solve_backward_geom_kernel): the two terms that DO involve delta_lambda, the
// rows w.r.t. the start state (g_x0 = tilde V_x[0]) and the obstacle circles.  It keeps the barrier row of V_xx and of
// tilde V_x per step as well (25 values, 100 B), forms lam_k in the forward sweep and accumulates 3M sums (geom_row).
// WTS variant (dtmpc_solve_backward_weights, solve_backward_weights_kernel<M, TRACK, GEOM>): the nine cost weights per
// trajectory, from a weights array [9][B] (36 B more read per trajectory); one kernel family for both record forms.
// DBAS variant (dtmpc_solve_backward_dbas, solve_backward_dbas_kernel<M, TRACK, W>): the rows w.r.t. the barrier-state
// parameters alpha_eff = max(alpha, eps) and gamma, the last of ift_gradient's terms that involve delta_lambda and
// h_offset == 0 admits.  Only the barrier row b' = B(h(x')) - gamma (B(h(x)) - b) of f_hat depends on them:
//   g_alpha_eff = sum_{m=0..N} co_m dBa(h(x_m)),  co_m = [m >= 1] lam_m - gamma [m <= N-1] lam_{m+1},
//                 dBa(z) = dB/da = 0 for z >= a, -3 (z - a)^2 / a^4 below
//   g_gamma     = -sum_{k<N} lam_{k+1} (B(h(x_k)) - b_k)
// (oracle/oracle_general.h ift1's ga / gg without the softplus / tanh chain, evaluated at the tape rows).  The family
// always has the GEOM record (25 values, no new workspace); W is the per-trajectory-weights flag.  The forward sweep
// already holds co_k, lam_{k+1}, b_k and, inside geom_row, h(x_k): B and dBa are formed from that one evaluation and
// two more per-lane sums are kept.  On a tape whose b_0 is the barrier of its own position B(h(x_k)) - b_k = 0 for
// every k, whatever gamma is: the gamma row is then zero in exact arithmetic (rounding noise in f32); it is non-zero
// only when the solve starts from a barrier state that is not the barrier of its position (a disturbed plant state,
// the second of two chained solves).  The family is a translation unit of its own, csrc/dtmpc_fast_layer_dbas.hip
// (this file included with DTMPC_FAST_LAYER_DBAS_TU: its 32 kernels compile beside this unit's 64, not after them).
// TIGHT variant (dtmpc_solve_backward_tight, solve_backward_tight_kernel<M, TRACK, W>): the backward of a solve whose
// barrier saw the tightened h(x) - s_i, s_i the lane's own element of a tight array [B], and the row w.r.t. s_i, the
// eleventh of ift_gradient's terms:
//   g_tight = -sum_{m=0..N} co_m B'(h(x_m) - s_i)
// (oracle/oracle_general.h ift1's gs without the softplus chain).  The reference linearises with B'(h) of the PLAIN h
// (core/tube_mpc.py:315-320 against :273-276; h_grad above), so the backward sweep is unchanged and delta_lambda of a
// given tape does not depend on s; only geom_row's factors move to z = h - s: B'(z) in the obstacle rows, dBa(z) in
// the alpha row, B(z) - b_k in the gamma row.  The family is the DBAS family with one more load and one more sum, a
// translation unit of its own, csrc/dtmpc_fast_layer_tight.hip (this file included with DTMPC_FAST_LAYER_TIGHT_TU).
// All kernels include one body text, dtmpc_fast_layer_body.hpp.
#define DTMPC_FAST_LAYER_TU 1
#include "dtmpc_fast.hip"

namespace dtmpc {
namespace fk {

constexpr int kLayerRec = 20;  // workspace values per step: K (8), k_ff (2), a02 a12 a30 a31 a32 b00 b10 b30 b31, mask
constexpr int kGeomRec = 25;   // GEOM: and the barrier row of V_xx (4) and of tilde V_x (1), what lam_k is formed from

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
struct LFwdInG : LFwdIn {  // GEOM
  real L[5];  // V_xx[k][3][0..3], tilde V_x[k][3]
};
// GEOM (dtmpc_solve_backward_geom): the kernel's block and two more outputs
struct LKG {
  LK k;       // p first
  real* gx0;  // [4][B] or NULL
  real* gob;  // [3M][B] or NULL: rows cx[0..M), cy[0..M), r2[0..M)
};

// One tape row's part of the obstacle rows: acc[j], acc[M + j], acc[2M + j] += co * B'(h(x)) * w_j(x) * (-2 (px - cx_j),
// -2 (py - cy_j), -1), w_j = softmax_j(-beta h_j).  The weights and h are h_grad<M>'s (dtmpc_fast.hip) operation for
// operation -- the same differences, exp2 arguments, sum order and reciprocal, so B' is evaluated at bitwise the h that
// jac's linearisation saw -- with the terms kept apart instead of summed into grad h.
// Returns h(x), the smooth-min the row was evaluated at (the DBAS variant forms B and dB/da from it).
// T (the TIGHT variant): B' is evaluated at z = h(x) - p.tight instead, z is what is returned, and *cb receives
// co * B'(z), the row's term of the tightening's sum.
template <int M, bool T = false>
__device__ __forceinline__ real geom_row(const FP& p, real px, real py, real co, real (&acc)[3 * M], real* cb = nullptr) {
#pragma clang fp contract(off)
  real hh[M], dxs[M], dys[M], zmax = 0.f;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const real dx = px - ocx<M>(p, i);
    const real dy = py - ocy<M>(p, i);
    const real h = dx * dx + dy * dy - or2<M>(p, i);
    const real zi = p.neg_beta * h;
    dxs[i] = dx;
    dys[i] = dy;
    hh[i] = h;
    zmax = (i == 0 || zi > zmax) ? zi : zmax;
  }
  const real zl = zmax * real(1.44269504088896341);
  real e[M], se = 0.f;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    e[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(hh[i], p.nbl2e, -zl));
    se += e[i];
  }
  const real inv = frcp(se);
  real hv = p.neg_inv_beta * (zmax + m_log(se));
  if constexpr (T) hv = hv - p.tight;
  const real cd = co * dbarrier(p, hv);
  if constexpr (T) *cb = cd;
  const real s = cd * inv;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const real cw = s * e[i];
    acc[i] += cw * (-2.f * dxs[i]);
    acc[M + i] += cw * (-2.f * dys[i]);
    acc[2 * M + i] -= cw;
  }
  return hv;
}

template <int M, bool TRACK>
__global__ void __launch_bounds__(kBlock) solve_backward_kernel(LK kk) {
  constexpr bool GEOM = false;
  constexpr bool WTS = false;
  constexpr bool DBAS = false;
  constexpr bool TIGHT = false;
  real* const gx0 = nullptr;
  real* const gob = nullptr;
  const real* const wts = nullptr;
  real* const gdb = nullptr;
  const real* const tgt = nullptr;
  real* const gtg = nullptr;
  (void)tgt;
  (void)gtg;
  (void)wts;
  (void)gdb;
#include "dtmpc_fast_layer_body.hpp"
}
// ... and with the rows w.r.t. the start state and the obstacle circles (dtmpc_solve_backward_geom)
template <int M, bool TRACK>
__global__ void __launch_bounds__(kBlock) solve_backward_geom_kernel(LKG kg) {
  constexpr bool GEOM = true;
  constexpr bool WTS = false;
  constexpr bool DBAS = false;
  constexpr bool TIGHT = false;
  const LK& kk = kg.k;
  real* const gx0 = kg.gx0;
  real* const gob = kg.gob;
  const real* const wts = nullptr;
  real* const gdb = nullptr;
  const real* const tgt = nullptr;
  real* const gtg = nullptr;
  (void)tgt;
  (void)gtg;
  (void)wts;
  (void)gdb;
#include "dtmpc_fast_layer_body.hpp"
}
// ... and with per-trajectory cost weights (dtmpc_solve_backward_weights): both record forms, G the GEOM one
struct LKW {
  LKG g;            // p first
  const real* wts;  // [9][B]: rows Q0 Q1 Q2 R0 R1 Qf0 Qf1 Qf2 qb (g_w's row order)
};
template <int M, bool TRACK, bool G>
__global__ void __launch_bounds__(kBlock) solve_backward_weights_kernel(LKW kw) {
  constexpr bool GEOM = G;
  constexpr bool WTS = true;
  constexpr bool DBAS = false;
  constexpr bool TIGHT = false;
  const LK& kk = kw.g.k;
  real* const gx0 = kw.g.gx0;
  real* const gob = kw.g.gob;
  const real* const wts = kw.wts;
  real* const gdb = nullptr;
  const real* const tgt = nullptr;
  real* const gtg = nullptr;
  (void)tgt;
  (void)gtg;
  (void)gdb;
#include "dtmpc_fast_layer_body.hpp"
}
// ... and with the rows w.r.t. the DBaS parameters (dtmpc_solve_backward_dbas): always the GEOM record, W the
// per-trajectory-weights flag (kd.w.wts is NULL without it); g_x0 / g_obs stay optional
struct LKD {
  LKW w;      // p first
  real* gdb;  // [2][B]: rows alpha_eff, gamma
};
template <int M, bool TRACK, bool PW>  // PW: per-trajectory weights (the body text names the workspace W)
__global__ void __launch_bounds__(kBlock) solve_backward_dbas_kernel(LKD kd) {
  constexpr bool GEOM = true;
  constexpr bool WTS = PW;
  constexpr bool DBAS = true;
  constexpr bool TIGHT = false;
  const LK& kk = kd.w.g.k;
  real* const gx0 = kd.w.g.gx0;
  real* const gob = kd.w.g.gob;
  const real* const wts = kd.w.wts;
  real* const gdb = kd.gdb;
  const real* const tgt = nullptr;
  real* const gtg = nullptr;
  (void)wts;
  (void)tgt;
  (void)gtg;
#include "dtmpc_fast_layer_body.hpp"
}
// ... and of a solve with a per-trajectory tightening, with the row w.r.t. it (dtmpc_solve_backward_tight): the DBAS
// family's record and sums, g_dbas optional as g_x0 / g_obs are
struct LKT {
  LKD d;            // p first
  const real* tgt;  // [B]: s_i
  real* gtg;        // [B]
};
template <int M, bool TRACK, bool PW>
__global__ void __launch_bounds__(kBlock) solve_backward_tight_kernel(LKT kt) {
  constexpr bool GEOM = true;
  constexpr bool WTS = PW;
  constexpr bool DBAS = true;
  constexpr bool TIGHT = true;
  const LK& kk = kt.d.w.g.k;
  real* const gx0 = kt.d.w.g.gx0;
  real* const gob = kt.d.w.g.gob;
  const real* const wts = kt.d.w.wts;
  real* const gdb = kt.d.gdb;
  const real* const tgt = kt.tgt;
  real* const gtg = kt.gtg;
  (void)wts;
#include "dtmpc_fast_layer_body.hpp"
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

static size_t layer_workspace_bytes(int32_t N, int64_t B, bool geom = false) {
  return (size_t)N * (geom ? fk::kGeomRec : fk::kLayerRec) * sizeof(real) * (size_t)B;
}

// geom: solve_backward_geom_kernel with the two further outputs (either may be NULL), else solve_backward_kernel;
// gdb (the DBAS unit only): solve_backward_dbas_kernel, wts may then be NULL;
// tgt / gtg (the TIGHT unit only): solve_backward_tight_kernel, wts and gdb may then be NULL
static int launch_solve_backward(const dtmpc_spec* sp, const dtmpc_cost* cp, int64_t B, const fk::LArgs& a,
                                 hipStream_t st, bool geom = false, real* gx0 = nullptr, real* gob = nullptr,
                                 const real* wts = nullptr, real* gdb = nullptr, const real* tgt = nullptr,
                                 real* gtg = nullptr) {
  fk::LKT kt;
  std::memset(&kt, 0, sizeof(kt));
  fk::LKD& kd = kt.d;
  kt.tgt = tgt;
  kt.gtg = gtg;
  fk::LKW& kw = kd.w;
  kd.gdb = gdb;
  fk::LKG& kg = kw.g;
  fk::LK& kk = kg.k;
  kw.wts = wts;
  fast_p(sp, kk.p);
  const DCost<real> c = make_cost<real>(*cp);
  const bool track = cp->kind == DTMPC_COST_TRACK;
  kk.c = fk::FCost{c.Q0, c.Q1, c.Q2, c.R0, c.R1, c.Qf0, c.Qf1, c.Qf2, c.qb,
                   track ? fk::f4{0.f, 0.f, 0.f, 0.f} : fk::f4{c.t0, c.t1, c.t2, 0.f}};
  kk.a = a;
  kg.gx0 = gx0;
  kg.gob = gob;
  const int bs = tube_block(B, 1);
  const dim3 grid((unsigned)((B + bs - 1) / bs));
#define LY_CASE(m) \
  case m:          \
    if (track) LY_LAUNCH(m, true); else LY_LAUNCH(m, false); \
    break;
#ifdef DTMPC_FAST_M_ONLY
#define LY_CASES LY_CASE(DTMPC_FAST_M_ONLY)
#else
#define LY_CASES LY_CASE(1) LY_CASE(2) LY_CASE(3) LY_CASE(4) LY_CASE(5) LY_CASE(6) LY_CASE(7) LY_CASE(8)
#endif
#if defined(DTMPC_FAST_LAYER_TIGHT_TU)  // this unit holds the TIGHT family alone
  if (!geom || !tgt || !gtg)
    return set_err(DTMPC_ERR_BAD_ARG, "solve backward tight: the GEOM record, tight and g_tight are required");
#define LY_LAUNCH(m, t)                                                                                    \
  do {                                                                                                     \
    if (wts) hipLaunchKernelGGL((fk::solve_backward_tight_kernel<m, t, true>), grid, dim3(bs), 0, st, kt); \
    else hipLaunchKernelGGL((fk::solve_backward_tight_kernel<m, t, false>), grid, dim3(bs), 0, st, kt);    \
  } while (0)
  switch (sp->n_obstacles) {
    LY_CASES
    default: return set_err(DTMPC_ERR_BAD_ARG, "solve backward: obstacle count not instantiated");
  }
#undef LY_LAUNCH
#elif defined(DTMPC_FAST_LAYER_DBAS_TU)  // this unit holds the DBAS family alone
  (void)kt;
  if (!geom || !gdb) return set_err(DTMPC_ERR_BAD_ARG, "solve backward dbas: the GEOM record and g_dbas are required");
#define LY_LAUNCH(m, t)                                                                               \
  do {                                                                                                \
    if (wts) hipLaunchKernelGGL((fk::solve_backward_dbas_kernel<m, t, true>), grid, dim3(bs), 0, st, kd); \
    else hipLaunchKernelGGL((fk::solve_backward_dbas_kernel<m, t, false>), grid, dim3(bs), 0, st, kd);    \
  } while (0)
  switch (sp->n_obstacles) {
    LY_CASES
    default: return set_err(DTMPC_ERR_BAD_ARG, "solve backward: obstacle count not instantiated");
  }
#undef LY_LAUNCH
#else
  (void)kt;
  if (wts) {  // per-trajectory weights: one family for both record forms
#define LY_LAUNCH(m, t)                                                                                       \
  do {                                                                                                        \
    if (geom) hipLaunchKernelGGL((fk::solve_backward_weights_kernel<m, t, true>), grid, dim3(bs), 0, st, kw); \
    else hipLaunchKernelGGL((fk::solve_backward_weights_kernel<m, t, false>), grid, dim3(bs), 0, st, kw);     \
  } while (0)
    switch (sp->n_obstacles) {
      LY_CASES
      default: return set_err(DTMPC_ERR_BAD_ARG, "solve backward: obstacle count not instantiated");
    }
#undef LY_LAUNCH
  } else if (!geom) {
#define LY_LAUNCH(m, t) hipLaunchKernelGGL((fk::solve_backward_kernel<m, t>), grid, dim3(bs), 0, st, kk)
    switch (sp->n_obstacles) {
      LY_CASES
      default: return set_err(DTMPC_ERR_BAD_ARG, "solve backward: obstacle count not instantiated");
    }
#undef LY_LAUNCH
  } else {
#define LY_LAUNCH(m, t) hipLaunchKernelGGL((fk::solve_backward_geom_kernel<m, t>), grid, dim3(bs), 0, st, kg)
    switch (sp->n_obstacles) {
      LY_CASES
      default: return set_err(DTMPC_ERR_BAD_ARG, "solve backward: obstacle count not instantiated");
    }
#undef LY_LAUNCH
  }
#endif
#undef LY_CASES
#undef LY_CASE
  return check_launch(gtg ? "solve_backward_tight_kernel" : gdb ? "solve_backward_dbas_kernel" : wts ? "solve_backward_weights_kernel"
                      : geom ? "solve_backward_geom_kernel" : "solve_backward_kernel");
}

// dtmpc_solve_backward and dtmpc_solve_backward_geom: the argument rules of include/dtmpc.h, then the launch
// (dbas: dtmpc_solve_backward_dbas -- the GEOM record, g_dbas required, g_x0 / g_obs / weights each optional)
static int solve_backward_entry(bool geom, int dtype, const dtmpc_spec* spec, const dtmpc_cost* cost, int64_t B,
                                const void* X, const void* U, const void* Xref, const void* Uref, const void* scenes,
                                const void* gX, const void* gU, void* g_w, void* g_target, void* g_xref, void* g_uref,
                                void* g_x0, void* g_obs, void* work, size_t work_bytes, int32_t* status,
                                void* stream, bool wts = false, const void* weights = nullptr, bool dbas = false,
                                void* g_dbas = nullptr, bool tightf = false, const void* tight = nullptr,
                                void* g_tight = nullptr) {
  if (!spec || !cost) return set_err(DTMPC_ERR_BAD_ARG, "solve backward: NULL spec or cost");
  if (B < 1) return set_err(DTMPC_ERR_BAD_ARG, "solve backward: batch must be >= 1");
  if (spec->horizon < 1) return set_err(DTMPC_ERR_BAD_ARG, "solve backward: horizon must be >= 1");
  if (int r = check_spec(spec, B)) return r;
  if (cost->kind != DTMPC_COST_TARGET && cost->kind != DTMPC_COST_TRACK)
    return set_err(DTMPC_ERR_BAD_ARG, "solve backward: bad cost kind");
  if (const char* why = layer_unsupported(dtype, spec, cost)) return set_err(DTMPC_ERR_BAD_ARG, why);
  if (!X || !U || !gX || !gU || !g_w || !status)
    return set_err(DTMPC_ERR_BAD_ARG, "solve backward: NULL X, U, gX, gU, g_w or status");
  if (wts && !weights) return set_err(DTMPC_ERR_BAD_ARG, "solve backward weights: NULL weights");
  if (dbas && !g_dbas) return set_err(DTMPC_ERR_BAD_ARG, "solve backward dbas: NULL g_dbas");
  if (tightf && (!tight || !g_tight)) return set_err(DTMPC_ERR_BAD_ARG, "solve backward tight: NULL tight or g_tight");
  if (geom && !wts && !dbas && !tightf && !g_x0 && !g_obs)
    return set_err(DTMPC_ERR_BAD_ARG, "solve backward geom: g_x0 and g_obs both NULL (that is dtmpc_solve_backward)");
  if (cost->kind == DTMPC_COST_TRACK) {
    if (!Xref || !Uref) return set_err(DTMPC_ERR_BAD_ARG, "solve backward: the tracking cost needs Xref and Uref");
    if (g_target) return set_err(DTMPC_ERR_BAD_ARG, "solve backward: g_target goes with the target cost");
  } else if (Xref || Uref || g_xref || g_uref) {
    return set_err(DTMPC_ERR_BAD_ARG, "solve backward: Xref, Uref, g_xref and g_uref go with the tracking cost");
  }
  if (!work || work_bytes < layer_workspace_bytes(spec->horizon, B, geom))
    return set_err(DTMPC_ERR_BAD_ARG, tightf ? "solve backward tight: work_bytes < "
                                               "dtmpc_solve_backward_tight_workspace_bytes(...)"
                                      : dbas ? "solve backward dbas: work_bytes < "
                                             "dtmpc_solve_backward_dbas_workspace_bytes(...)"
                                      : wts  ? "solve backward weights: work_bytes < "
                                             "dtmpc_solve_backward_weights_workspace_bytes(...)"
                                      : geom ? "solve backward geom: work_bytes < "
                                             "dtmpc_solve_backward_geom_workspace_bytes(...)"
                                           : "solve backward: work_bytes < dtmpc_solve_backward_workspace_bytes(...)");
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
  return launch_solve_backward(spec, cost, B, a, (hipStream_t)stream, geom, (real*)g_x0, (real*)g_obs,
                               (const real*)weights, (real*)g_dbas, (const real*)tight, (real*)g_tight);
}

}  // namespace dtmpc

extern "C" {

#if defined(DTMPC_FAST_LAYER_TIGHT_TU)

size_t dtmpc_solve_backward_tight_workspace_bytes(int dtype, int32_t horizon, int64_t B) {
  if (dtype != DTMPC_F32 || horizon < 1 || B < 1) return 0;
  return dtmpc::layer_workspace_bytes(horizon, B, true);
}

int dtmpc_solve_backward_tight(int dtype, const dtmpc_spec* spec, const dtmpc_cost* cost, int64_t B, const void* X,
                               const void* U, const void* Xref, const void* Uref, const void* scenes,
                               const void* weights, const void* tight, const void* gX, const void* gU, void* g_w,
                               void* g_target, void* g_xref, void* g_uref, void* g_x0, void* g_obs, void* g_dbas,
                               void* g_tight, void* work, size_t work_bytes, int32_t* status, void* stream) {
  // always the GEOM record; weights == NULL is the shared cost, g_dbas == NULL leaves the DBaS sums unwritten
  return dtmpc::solve_backward_entry(true, dtype, spec, cost, B, X, U, Xref, Uref, scenes, gX, gU, g_w, g_target, g_xref,
                                     g_uref, g_x0, g_obs, work, work_bytes, status, stream, weights != nullptr, weights,
                                     false, g_dbas, true, tight, g_tight);
}

#elif defined(DTMPC_FAST_LAYER_DBAS_TU)

size_t dtmpc_solve_backward_dbas_workspace_bytes(int dtype, int32_t horizon, int64_t B) {
  if (dtype != DTMPC_F32 || horizon < 1 || B < 1) return 0;
  return dtmpc::layer_workspace_bytes(horizon, B, true);
}

int dtmpc_solve_backward_dbas(int dtype, const dtmpc_spec* spec, const dtmpc_cost* cost, int64_t B, const void* X,
                              const void* U, const void* Xref, const void* Uref, const void* scenes,
                              const void* weights, const void* gX, const void* gU, void* g_w, void* g_target,
                              void* g_xref, void* g_uref, void* g_x0, void* g_obs, void* g_dbas, void* work,
                              size_t work_bytes, int32_t* status, void* stream) {
  // always the GEOM record; weights == NULL is the shared cost
  return dtmpc::solve_backward_entry(true, dtype, spec, cost, B, X, U, Xref, Uref, scenes, gX, gU, g_w, g_target, g_xref,
                                     g_uref, g_x0, g_obs, work, work_bytes, status, stream, weights != nullptr, weights,
                                     true, g_dbas);
}

#else

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
  return dtmpc::solve_backward_entry(false, dtype, spec, cost, B, X, U, Xref, Uref, scenes, gX, gU, g_w, g_target, g_xref,
                                     g_uref, nullptr, nullptr, work, work_bytes, status, stream);
}

size_t dtmpc_solve_backward_geom_workspace_bytes(int dtype, int32_t horizon, int64_t B) {
  if (dtype != DTMPC_F32 || horizon < 1 || B < 1) return 0;
  return dtmpc::layer_workspace_bytes(horizon, B, true);
}

int dtmpc_solve_backward_geom(int dtype, const dtmpc_spec* spec, const dtmpc_cost* cost, int64_t B, const void* X,
                              const void* U, const void* Xref, const void* Uref, const void* scenes, const void* gX,
                              const void* gU, void* g_w, void* g_target, void* g_xref, void* g_uref, void* g_x0,
                              void* g_obs, void* work, size_t work_bytes, int32_t* status, void* stream) {
  return dtmpc::solve_backward_entry(true, dtype, spec, cost, B, X, U, Xref, Uref, scenes, gX, gU, g_w, g_target, g_xref,
                                     g_uref, g_x0, g_obs, work, work_bytes, status, stream);
}

size_t dtmpc_solve_backward_weights_workspace_bytes(int dtype, int32_t horizon, int64_t B, int32_t geom) {
  if (dtype != DTMPC_F32 || horizon < 1 || B < 1) return 0;
  return dtmpc::layer_workspace_bytes(horizon, B, geom != 0);
}

int dtmpc_solve_backward_weights(int dtype, const dtmpc_spec* spec, const dtmpc_cost* cost, int64_t B, const void* X,
                                 const void* U, const void* Xref, const void* Uref, const void* scenes,
                                 const void* weights, const void* gX, const void* gU, void* g_w, void* g_target,
                                 void* g_xref, void* g_uref, void* g_x0, void* g_obs, void* work, size_t work_bytes,
                                 int32_t* status, void* stream) {
  // the GEOM record (25 values) when either of its outputs is asked for, else the plain one (20)
  return dtmpc::solve_backward_entry(g_x0 || g_obs, dtype, spec, cost, B, X, U, Xref, Uref, scenes, gX, gU, g_w, g_target,
                                     g_xref, g_uref, g_x0, g_obs, work, work_bytes, status, stream, true, weights);
}

#endif  // DTMPC_FAST_LAYER_DBAS_TU

}  // extern "C"
