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
// GEOM variant (dtmpc_solve_backward_geom, solve_backward_kernel<LKG, M, TRACK>): the two terms that DO involve
// delta_lambda, the rows w.r.t. the start state (g_x0 = tilde V_x[0]) and the obstacle circles.  It keeps the barrier
// row of V_xx and of tilde V_x per step as well (25 values, 100 B), forms lam_k in the forward sweep and accumulates 3M
// sums (geom_row).
// WTS variant (dtmpc_solve_backward_weights, solve_backward_kernel<LKW, M, TRACK, GEOM>): the nine cost weights per
// trajectory, from a weights array [9][B] (36 B more read per trajectory); one kernel family for both record forms.
// DBAS variant (dtmpc_solve_backward_dbas, solve_backward_kernel<LKD, M, TRACK, W>): the rows w.r.t. the barrier-state
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
// TIGHT variant (dtmpc_solve_backward_tight, solve_backward_kernel<LKT, M, TRACK, W>): the backward of a solve whose
// barrier saw the tightened h(x) - s_i, s_i the lane's own element of a tight array [B], and the row w.r.t. s_i, the
// eleventh of ift_gradient's terms:
//   g_tight = -sum_{m=0..N} co_m B'(h(x_m) - s_i)
// (oracle/oracle_general.h ift1's gs without the softplus chain).  The reference linearises with B'(h) of the PLAIN h
// (core/tube_mpc.py:315-320 against :273-276; h_grad above), so the backward sweep is unchanged and delta_lambda of a
// given tape does not depend on s; only geom_row's factors move to z = h - s: B'(z) in the obstacle rows, dBa(z) in
// the alpha row, B(z) - b_k in the gamma row.  The family is the DBAS family with one more load and one more sum, a
// translation unit of its own, csrc/dtmpc_fast_layer_tight.hip (this file included with DTMPC_FAST_LAYER_TIGHT_TU).
// One kernel template over the variants' argument blocks includes the body text, dtmpc_fast_layer_body.hpp.
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

// The kernels' argument blocks, one per entry point of include/dtmpc.h: each holds the one before it (`in`) with its
// own pointers behind, so a kernel's argument offsets are those of every smaller block and the host fills the largest.
// A block says which of GEOM / WTS / DBAS / TIGHT its kernels compile in, f being the kernel's flag FL where it has one.
enum LVariant { kLPlain, kLGeom, kLWeights, kLDbas, kLTight };
struct LK {
  FP p;  // first, as in every fused kernel's argument block
  FCost c;
  LArgs a;
  static constexpr int kVariant = kLPlain;
  static constexpr bool kFlag = false, kHasDbas = false, kHasTight = false;
  static constexpr bool has_geom(bool) { return false; }
  static constexpr bool has_wts(bool) { return false; }
};
// GEOM (dtmpc_solve_backward_geom): the rows w.r.t. the start state and the obstacle circles
struct LKG {
  LK in;
  real* gx0;  // [4][B] or NULL
  real* gob;  // [3M][B] or NULL: rows cx[0..M), cy[0..M), r2[0..M)
  static constexpr int kVariant = kLGeom;
  static constexpr bool kFlag = false, kHasDbas = false, kHasTight = false;
  static constexpr bool has_geom(bool) { return true; }
  static constexpr bool has_wts(bool) { return false; }
};
// WTS (dtmpc_solve_backward_weights): per-trajectory cost weights, both record forms -- FL the GEOM one
struct LKW {
  LKG in;
  const real* wts;  // [9][B]: rows Q0 Q1 Q2 R0 R1 Qf0 Qf1 Qf2 qb (g_w's row order)
  static constexpr int kVariant = kLWeights;
  static constexpr bool kFlag = true, kHasDbas = false, kHasTight = false;
  static constexpr bool has_geom(bool f) { return f; }
  static constexpr bool has_wts(bool) { return true; }
};
// DBAS (dtmpc_solve_backward_dbas): the rows w.r.t. the DBaS parameters; always the GEOM record, FL the
// per-trajectory-weights flag (wts is NULL without it); g_x0 / g_obs stay optional
struct LKD {
  LKW in;
  real* gdb;  // [2][B]: rows alpha_eff, gamma
  static constexpr int kVariant = kLDbas;
  static constexpr bool kFlag = true, kHasDbas = true, kHasTight = false;
  static constexpr bool has_geom(bool) { return true; }
  static constexpr bool has_wts(bool f) { return f; }
};
// TIGHT (dtmpc_solve_backward_tight): a solve with a per-trajectory tightening and the row w.r.t. it; the DBAS family's
// record and sums, g_dbas optional as g_x0 / g_obs are
struct LKT {
  LKD in;
  const real* tgt;  // [B]: s_i
  real* gtg;        // [B]
  static constexpr int kVariant = kLTight;
  static constexpr bool kFlag = true, kHasDbas = true, kHasTight = true;
  static constexpr bool has_geom(bool) { return true; }
  static constexpr bool has_wts(bool f) { return f; }
};
// The member m of block B where the kernel's block K holds a B, else NULL.  (The block goes by value: an accessor that
// takes the kernel's argument by reference compiles to other code, as dtmpc_fast_layer_body.hpp notes.)
template <class K, class B, class P>
__device__ __forceinline__ P opt(const K k, P B::*m) {
  if constexpr (std::is_same_v<K, B>) {
    return k.*m;
  } else if constexpr (K::kVariant > B::kVariant) {
    return opt(k.in, m);
  } else {
    return nullptr;
  }
}

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

// One kernel over the blocks: solve_backward_kernel<LK, M, TRACK>, <LKG, M, TRACK>, <LKW, M, TRACK, G>,
// <LKD, M, TRACK, W> and <LKT, M, TRACK, W>.
template <class K, int M, bool TRACK, bool FL = false>
__global__ void __launch_bounds__(kBlock) solve_backward_kernel(K kb) {
  constexpr bool GEOM = K::has_geom(FL), WTS = K::has_wts(FL), DBAS = K::kHasDbas, TIGHT = K::kHasTight;
  static_assert(std::is_standard_layout_v<K>, "a block's address is that of the LK it begins with");
  const LK& kk = reinterpret_cast<const LK&>(kb);
  [[maybe_unused]] real* const gx0 = opt(kb, &LKG::gx0);
  [[maybe_unused]] real* const gob = opt(kb, &LKG::gob);
  [[maybe_unused]] const real* const wts = opt(kb, &LKW::wts);
  [[maybe_unused]] real* const gdb = opt(kb, &LKD::gdb);
  [[maybe_unused]] const real* const tgt = opt(kb, &LKT::tgt);
  [[maybe_unused]] real* const gtg = opt(kb, &LKT::gtg);
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

// What a variant adds to dtmpc_solve_backward's arguments; a pointer the variant does not have stays NULL.
struct LayerOpt {
  fk::LVariant variant = fk::kLPlain;
  bool geom = false;              // the GEOM record (kGeomRec values per step) is in use
  void* gx0 = nullptr;            // g_x0 [4][B]
  void* gob = nullptr;            // g_obs [3M][B]
  const void* weights = nullptr;  // [9][B]
  void* gdb = nullptr;            // g_dbas [2][B]
  const void* tight = nullptr;    // [B]
  void* gtg = nullptr;            // g_tight [B]
};
// per variant: the kernel as check_launch names it, and the message of a workspace that is too small
static const char* const kLayerKernel[] = {"solve_backward_kernel<LK>", "solve_backward_kernel<LKG>",
                                           "solve_backward_kernel<LKW>", "solve_backward_kernel<LKD>",
                                           "solve_backward_kernel<LKT>"};
static const char* const kLayerWorkMsg[] = {
    "solve backward: work_bytes < dtmpc_solve_backward_workspace_bytes(...)",
    "solve backward geom: work_bytes < dtmpc_solve_backward_geom_workspace_bytes(...)",
    "solve backward weights: work_bytes < dtmpc_solve_backward_weights_workspace_bytes(...)",
    "solve backward dbas: work_bytes < dtmpc_solve_backward_dbas_workspace_bytes(...)",
    "solve backward tight: work_bytes < dtmpc_solve_backward_tight_workspace_bytes(...)"};

// The blocks whose kernels this unit instantiates: the DBAS and the TIGHT family (32 kernels each) are units of their
// own, so that they compile beside this unit's 64 kernels, not after them.
template <class... K>
struct Blocks {};
#if defined(DTMPC_FAST_LAYER_TIGHT_TU)
using UnitBlocks = Blocks<fk::LKT>;
#elif defined(DTMPC_FAST_LAYER_DBAS_TU)
using UnitBlocks = Blocks<fk::LKD>;
#else
using UnitBlocks = Blocks<fk::LK, fk::LKG, fk::LKW>;
#endif

// solve_backward_kernel<K, M, track[, FL]> on the K that kt begins with
template <class K>
static int launch_block(const fk::LKT& kt, int M, bool track, const LayerOpt& o, dim3 grid, int bs, hipStream_t st) {
  if constexpr (K::kHasTight) {
    if (!o.geom || !o.tight || !o.gtg)
      return set_err(DTMPC_ERR_BAD_ARG, "solve backward tight: the GEOM record, tight and g_tight are required");
  } else if constexpr (K::kHasDbas) {
    if (!o.geom || !o.gdb)
      return set_err(DTMPC_ERR_BAD_ARG, "solve backward dbas: the GEOM record and g_dbas are required");
  }
  static_assert(std::is_standard_layout_v<fk::LKT>, "kt's address is that of the K it begins with");
  const K& kb = reinterpret_cast<const K&>(kt);
  const bool f = K::has_geom(false) ? o.weights != nullptr : o.geom;  // FL is W where the record is always GEOM, else G
  const bool hit = pick_obstacles(M, [&](auto m) {
    return pick_flag(track, [&](auto t) {
      constexpr int Mc = decltype(m)::value;
      constexpr bool T = decltype(t)::value;
      if constexpr (K::kFlag) {
        pick_flag(f, [&](auto ff) {
          hipLaunchKernelGGL((fk::solve_backward_kernel<K, Mc, T, decltype(ff)::value>), grid, dim3(bs), 0, st, kb);
        });
      } else {
        hipLaunchKernelGGL((fk::solve_backward_kernel<K, Mc, T>), grid, dim3(bs), 0, st, kb);
      }
    });
  });
  if (!hit) return not_instantiated("solve backward");
  return check_launch(kLayerKernel[K::kVariant]);
}
template <class... K>
static int launch_unit(Blocks<K...>, const fk::LKT& kt, int M, bool track, const LayerOpt& o, dim3 grid, int bs,
                       hipStream_t st) {
  int r = DTMPC_OK;
  if (((K::kVariant == o.variant && ((r = launch_block<K>(kt, M, track, o, grid, bs, st)), true)) || ...)) return r;
  return set_err(DTMPC_ERR_BAD_ARG, "solve backward: variant not in this unit");
}

static int launch_solve_backward(const dtmpc_spec* sp, const dtmpc_cost* cp, int64_t B, const fk::LArgs& a,
                                 hipStream_t st, const LayerOpt& o) {
  fk::LK kk;
  std::memset(&kk, 0, sizeof(kk));
  fast_p(sp, kk.p);
  const bool track = cp->kind == DTMPC_COST_TRACK;
  kk.c = fast_cost(*cp, track);
  kk.a = a;
  // the largest block: every variant's is what it begins with
  const fk::LKG kg = {kk, (real*)o.gx0, (real*)o.gob};
  const fk::LKW kw = {kg, (const real*)o.weights};
  const fk::LKD kd = {kw, (real*)o.gdb};
  const fk::LKT kt = {kd, (const real*)o.tight, (real*)o.gtg};
  const int bs = tube_block(B, 1);
  const dim3 grid((unsigned)((B + bs - 1) / bs));
  return launch_unit(UnitBlocks{}, kt, sp->n_obstacles, track, o, grid, bs, st);
}

// the argument rules of include/dtmpc.h for every variant, then the launch
static int solve_backward_entry(const LayerOpt& o, int dtype, const dtmpc_spec* spec, const dtmpc_cost* cost, int64_t B,
                                const void* X, const void* U, const void* Xref, const void* Uref, const void* scenes,
                                const void* gX, const void* gU, void* g_w, void* g_target, void* g_xref, void* g_uref,
                                void* work, size_t work_bytes, int32_t* status, void* stream) {
  if (!spec || !cost) return set_err(DTMPC_ERR_BAD_ARG, "solve backward: NULL spec or cost");
  if (B < 1) return set_err(DTMPC_ERR_BAD_ARG, "solve backward: batch must be >= 1");
  if (spec->horizon < 1) return set_err(DTMPC_ERR_BAD_ARG, "solve backward: horizon must be >= 1");
  if (int r = check_spec(spec, B)) return r;
  if (cost->kind != DTMPC_COST_TARGET && cost->kind != DTMPC_COST_TRACK)
    return set_err(DTMPC_ERR_BAD_ARG, "solve backward: bad cost kind");
  if (const char* why = layer_unsupported(dtype, spec, cost)) return set_err(DTMPC_ERR_BAD_ARG, why);
  if (!X || !U || !gX || !gU || !g_w || !status)
    return set_err(DTMPC_ERR_BAD_ARG, "solve backward: NULL X, U, gX, gU, g_w or status");
  if (o.variant == fk::kLWeights && !o.weights) return set_err(DTMPC_ERR_BAD_ARG, "solve backward weights: NULL weights");
  if (o.variant == fk::kLDbas && !o.gdb) return set_err(DTMPC_ERR_BAD_ARG, "solve backward dbas: NULL g_dbas");
  if (o.variant == fk::kLTight && (!o.tight || !o.gtg))
    return set_err(DTMPC_ERR_BAD_ARG, "solve backward tight: NULL tight or g_tight");
  if (o.variant == fk::kLGeom && !o.gx0 && !o.gob)
    return set_err(DTMPC_ERR_BAD_ARG, "solve backward geom: g_x0 and g_obs both NULL (that is dtmpc_solve_backward)");
  if (cost->kind == DTMPC_COST_TRACK) {
    if (!Xref || !Uref) return set_err(DTMPC_ERR_BAD_ARG, "solve backward: the tracking cost needs Xref and Uref");
    if (g_target) return set_err(DTMPC_ERR_BAD_ARG, "solve backward: g_target goes with the target cost");
  } else if (Xref || Uref || g_xref || g_uref) {
    return set_err(DTMPC_ERR_BAD_ARG, "solve backward: Xref, Uref, g_xref and g_uref go with the tracking cost");
  }
  if (!work || work_bytes < layer_workspace_bytes(spec->horizon, B, o.geom))
    return set_err(DTMPC_ERR_BAD_ARG, kLayerWorkMsg[o.variant]);
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
  return launch_solve_backward(spec, cost, B, a, (hipStream_t)stream, o);
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
  const dtmpc::LayerOpt o = {.variant = dtmpc::fk::kLTight, .geom = true, .gx0 = g_x0, .gob = g_obs, .weights = weights,
                             .gdb = g_dbas, .tight = tight, .gtg = g_tight};
  return dtmpc::solve_backward_entry(o, dtype, spec, cost, B, X, U, Xref, Uref, scenes, gX, gU, g_w, g_target, g_xref,
                                     g_uref, work, work_bytes, status, stream);
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
  const dtmpc::LayerOpt o = {.variant = dtmpc::fk::kLDbas, .geom = true, .gx0 = g_x0, .gob = g_obs, .weights = weights,
                             .gdb = g_dbas};
  return dtmpc::solve_backward_entry(o, dtype, spec, cost, B, X, U, Xref, Uref, scenes, gX, gU, g_w, g_target, g_xref,
                                     g_uref, work, work_bytes, status, stream);
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
  const dtmpc::LayerOpt o = {.variant = dtmpc::fk::kLPlain};
  return dtmpc::solve_backward_entry(o, dtype, spec, cost, B, X, U, Xref, Uref, scenes, gX, gU, g_w, g_target, g_xref,
                                     g_uref, work, work_bytes, status, stream);
}

size_t dtmpc_solve_backward_geom_workspace_bytes(int dtype, int32_t horizon, int64_t B) {
  if (dtype != DTMPC_F32 || horizon < 1 || B < 1) return 0;
  return dtmpc::layer_workspace_bytes(horizon, B, true);
}

int dtmpc_solve_backward_geom(int dtype, const dtmpc_spec* spec, const dtmpc_cost* cost, int64_t B, const void* X,
                              const void* U, const void* Xref, const void* Uref, const void* scenes, const void* gX,
                              const void* gU, void* g_w, void* g_target, void* g_xref, void* g_uref, void* g_x0,
                              void* g_obs, void* work, size_t work_bytes, int32_t* status, void* stream) {
  const dtmpc::LayerOpt o = {.variant = dtmpc::fk::kLGeom, .geom = true, .gx0 = g_x0, .gob = g_obs};
  return dtmpc::solve_backward_entry(o, dtype, spec, cost, B, X, U, Xref, Uref, scenes, gX, gU, g_w, g_target, g_xref,
                                     g_uref, work, work_bytes, status, stream);
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
  const dtmpc::LayerOpt o = {.variant = dtmpc::fk::kLWeights, .geom = g_x0 || g_obs, .gx0 = g_x0, .gob = g_obs,
                             .weights = weights};
  return dtmpc::solve_backward_entry(o, dtype, spec, cost, B, X, U, Xref, Uref, scenes, gX, gU, g_w, g_target, g_xref,
                                     g_uref, work, work_bytes, status, stream);
}

#endif  // DTMPC_FAST_LAYER_DBAS_TU

}  // extern "C"
