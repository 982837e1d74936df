// dtmpc_fast_layer_body.hpp -- the body of solve_backward_kernel (csrc/dtmpc_fast_layer.hip), included textually into
// the kernel template: it sees `const LK& kk` (the LK its argument block begins with), the constexpr bools GEOM, WTS,
// DBAS and TIGHT that the block type stands for, and the pointers gx0 / gob / wts / gdb / tgt / gtg, NULL where the
// block has none.  Text, not a shared device function: with GEOM false every `if constexpr
// (GEOM)` statement is discarded in the front end and the kernel's code is what it was before the variant existed
// (a body shared through a reference to the kernel's argument compiled to other code, ten VGPRs more; so did accessors
// that take the argument block by reference, which is why the kernel's take it by value).
// WTS (solve_backward_kernel<LKW, ...>, dtmpc_solve_backward_weights): a third constexpr bool beside GEOM, with the
// pointer `wts` -- the nine cost weights come from the lane's own column of the weights array [9][B] (wts_c) instead of
// kk.c, so g_xref = -2 Q_i dx and g_target use trajectory i's own Q / Qf; with WTS false the statement is discarded.
// DBAS (solve_backward_kernel<LKD, ...>, dtmpc_solve_backward_dbas): a fourth constexpr bool, valid with GEOM only, with the
// pointer `gdb` [2][B] -- the rows w.r.t. alpha_eff = max(alpha, eps) and gamma: from geom_row's one evaluation of
// h(x_m) the forward sweep also forms dBa(h) = -3 (h - a)^2 / a^4 below a (0 at and above it) and B(h) (vbarrier) and
// keeps the sums g_alpha_eff += co_m dBa, g_gamma -= lam_{k+1} (B(h(x_k)) - b_k); row N adds its alpha term only.
// With b_0 = B(h(x_0)) every B(h(x_k)) - b_k is zero on a rolled-out tape and the gamma row is rounding noise.  With
// DBAS false every `if constexpr (DBAS)` statement is discarded.
// TIGHT (solve_backward_kernel<LKT, ...>, dtmpc_solve_backward_tight): a fifth constexpr bool, valid with GEOM and DBAS
// only, with the pointers `tgt` [B] and `gtg` [B] -- the lane's own tightening s_i goes into p.tight before the table is
// pinned; geom_row<M, true> evaluates B' at z = h(x_m) - s_i, returns z (so dBa and B of the DBAS sums are taken at z as
// well) and hands out co_m B'(z), which the forward sweep sums into g_tight = -sum_m co_m B'(z_m).  The backward sweep
// k = N-1..0 is untouched: the reference linearises with B'(h) of the plain h (h_grad), so delta_lambda of a given tape
// does not depend on s.  gdb may be NULL here.  With TIGHT false every `if constexpr (TIGHT)` statement is discarded.
// No include guard: it is a function body, included once, inside the kernel template.
  static_assert(GEOM || !DBAS, "DBAS needs the GEOM record");
  static_assert(DBAS || !TIGHT, "TIGHT needs the GEOM record and the DBAS sums");
  constexpr int REC = GEOM ? kGeomRec : kLayerRec;
  using LFwd = typename std::conditional<GEOM && (M > 0), LFwdInG, LFwdIn>::type;  // (M > 0: a dependent type)
  const LArgs& a = kk.a;
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= a.B) return;
  const size_t nb = (size_t)a.B;
  FP p = kk.p;
  FCost c = kk.c;
  if constexpr (WTS) c = wts_c(c, wts, nb, i);  // this trajectory's own weights
  if (a.sc) {  // per-trajectory scene: this trajectory's obstacles and, for the target cost, its target
    p = scene_p<M>(p, a.sc, nb, i);
    if (!TRACK) c.tg = scene_tg<M>(a.sc, nb, i);
  }
  if constexpr (TIGHT) p.tight = tgt[i];  // this trajectory's own tightening
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
    real* w = W + (size_t)(REC * k) * nb;
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
    if constexpr (GEOM) {
#pragma unroll
      for (int j = 0; j < 4; ++j) w[(size_t)(20 + j) * nb] = R.Vxx[3][j];
      w[(size_t)24 * nb] = R.Vx[3];
    }
  }
  bool ok0 = true;
  if constexpr (GEOM) {  // g_x0 = dlam_0 = tilde V_x[0] (delta x_0 = 0)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (gx0) gx0[(size_t)j * nb + i] = R.Vx[j];
      ok0 = ok0 && finite(R.Vx[j]);
    }
  }
  // forward (:413-425) fused with the accumulation
  const real* XR = TRACK ? a.Xr + i : nullptr;
  const real* UR = TRACK ? a.Ur + i : nullptr;
  real* GXR = TRACK && a.gxr ? a.gxr + i : nullptr;
  real* GUR = TRACK && a.gur ? a.gur + i : nullptr;
  auto fload = [&](LFwd& F, int k) {
    const real* w = W + (size_t)(REC * k) * nb;
#pragma unroll
    for (int j = 0; j < 8; ++j) F.K[j] = w[(size_t)j * nb];
    F.kf[0] = w[(size_t)8 * nb];
    F.kf[1] = w[(size_t)9 * nb];
#pragma unroll
    for (int j = 0; j < 9; ++j) F.A[j] = w[(size_t)(10 + j) * nb];
    F.act = w[(size_t)19 * nb];
    if constexpr (GEOM) {
#pragma unroll
      for (int j = 0; j < 5; ++j) F.L[j] = w[(size_t)(20 + j) * nb];
    }
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
  // GEOM: the obstacle rows' 3M sums; lam = lam_k on entry to trip k (row 0 takes no lam_0 term); lamN = gX_N[3]
  real go[GEOM ? 3 * M : 1];
  real lam = 0.f, lamN = 0.f;
  if constexpr (GEOM) {
#pragma unroll
    for (int j = 0; j < 3 * M; ++j) go[j] = 0.f;
    lamN = GX[(size_t)(4 * N + 3) * nb];
  }
  (void)go;
  (void)lam;
  (void)lamN;
  // DBAS: the two sums g_alpha_eff, g_gamma; dBa(z) = dba_c (z - a)^2 below a, dba_c = -3 / a^4
  real ga = 0.f, gg = 0.f, dba_c = 0.f;
  if constexpr (DBAS) dba_c = -3.f / (p.a2 * p.a2);
  (void)ga;
  (void)gg;
  (void)dba_c;
  real gs = 0.f;  // TIGHT: sum_m co_m B'(h(x_m) - s)
  (void)gs;
  bool ok = true;
  if constexpr (GEOM) ok = ok0;
  LFwd Fn;
  fload(Fn, 0);
  for (int k = 0; k < N; ++k) {
    const LFwd F = Fn;
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
    if constexpr (GEOM) {
      // lam_{k+1} = tilde V_x[k+1][3] + V_xx[k+1][3] . dx_{k+1} (Fn holds step k + 1's record; V_xx[N] = diag pxx),
      // then tape row k's coefficient c_k / B'(h(x_k)) = [k >= 1] lam_k - gamma lam_{k+1}
      const real ln = k + 1 < N ? Fn.L[4] + (Fn.L[0] * n0 + Fn.L[1] * n1 + Fn.L[2] * n2 + Fn.L[3] * n3)
                                : lamN + pxx[3] * n3;
      if constexpr (DBAS) {
        // the same evaluation of h(x_k): co_k dBa(h) into the alpha sum, -lam_{k+1} (B(h) - b_k) into the gamma sum
        const real co = lam - g * ln;
        real hv;
        if constexpr (TIGHT) {  // hv is h(x_k) - s, and the row's term of the tightening's sum comes with it
          real cb;
          hv = geom_row<M, true>(p, F.x[0], F.x[1], co, go, &cb);
          gs += cb;
        } else {
          hv = geom_row<M>(p, F.x[0], F.x[1], co, go);
        }
        const real df = hv - p.a;
        const real ta = co * (dba_c * (df * df));
        ga += hv >= p.a ? 0.f : ta;
        gg -= ln * (vbarrier(p, hv) - F.x[3]);
      } else {
        geom_row<M>(p, F.x[0], F.x[1], lam - g * ln, go);
      }
      lam = ln;
    }
    d[0] = n0;
    d[1] = n1;
    d[2] = n2;
    d[3] = n3;
  }
  if constexpr (GEOM) {  // row N: c_N = B'(h(x_N)) lam_N
    if constexpr (DBAS) {  // row N adds its alpha term only (co_N = lam_N; no step leaves x_N)
      real hv;
      if constexpr (TIGHT) {
        real cb;
        hv = geom_row<M, true>(p, X[(size_t)(4 * N) * nb], X[(size_t)(4 * N + 1) * nb], lam, go, &cb);
        gs += cb;
      } else {
        hv = geom_row<M>(p, X[(size_t)(4 * N) * nb], X[(size_t)(4 * N + 1) * nb], lam, go);
      }
      const real df = hv - p.a;
      const real ta = lam * (dba_c * (df * df));
      ga += hv >= p.a ? 0.f : ta;
      if constexpr (TIGHT) {
        if (gdb) {
          gdb[i] = ga;
          gdb[nb + i] = gg;
        }
        gtg[i] = -gs;
        ok = ok && finite(gs);
      } else {
        gdb[i] = ga;
        gdb[nb + i] = gg;
      }
      ok = ok && finite(ga) && finite(gg);
    } else {
      geom_row<M>(p, X[(size_t)(4 * N) * nb], X[(size_t)(4 * N + 1) * nb], lam, go);
    }
    real* GO = gob ? gob + i : nullptr;
#pragma unroll
    for (int j = 0; j < 3 * M; ++j) {
      if (GO) GO[(size_t)j * nb] = go[j];
      ok = ok && finite(go[j]);
    }
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
