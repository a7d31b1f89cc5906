// C ABI, measurement update (include/xivo_hip.h): the route table, the hand-over of measurements, the update pipelines, the
// L D L^T fallback, the one-filter plumbing call and the update's getters. Host-side orchestration only (capi_internal.h).
#include <algorithm>

#include "capi_internal.h"

using namespace xivo_hip;
using namespace xivo_hip::capi;

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Route selection of Estimator::UpdateJosephForm (src/estimator.cpp:1257-1288), in ONE place. Every pass of the update
// (update_joseph_range) asks plan_update() once; the pipelines below only execute what the plan says, and
// tests/test_update_gpu.py::test_every_route_of_the_plan enumerates the routes of this table against the oracle,
// tests/test_update_edges_gpu.py runs shapes on both sides of each of its limits.
//
//   route              | rows of H                   | gain + covariance                                   | when
//   -------------------+-----------------------------+-----------------------------------------------------+--------------------------
//   FUSED              | row-pair compressed         | one kernel per filter (fused_update.hip)            | M <= 64 / N <= 256 or M <= 112 / N <= 192, and M <= N (rounded to 16), default form
//   SPARSE_IN_SOLVE    | compressed (+ OOS / lead)   | whitened Joseph form inside the solve kernel        | N <= 256, M <= 176, > 64 filters
//   SPARSE_WHITENED    | compressed (+ OOS / lead)   | whitened outputs V^T, Y^T + tiled P - V^T Y         | wider shapes; <= 64 filters (latency route)
//   SPARSE_SYMMETRIC   | compressed                  | P - W^T W, forward substitution only                | XIVO_HIP_FLAG_SYMMETRIC_FORM
//   SPARSE_TAIL        | compressed                  | T = K(HP) - P, G = T H^T + K R, P+ = G K^T - T      | XIVO_HIP_FLAG_STANDALONE_TAIL
//   DENSE_ASCODED      | dense                       | A = KH - I, T = A P, P+ = T A^T + K R K^T           | XIVO_HIP_FLAG_DENSE_H
//   DENSE_WHITENED     | dense (H does not compress) | dense H P and S, then as SPARSE_IN_SOLVE / _WHITENED | an H without XIVO's row structure
//   DENSE_SYMMETRIC    | dense                       | as SPARSE_SYMMETRIC                                 | SYMMETRIC_FORM on dense rows
enum UpdateRoute : int { ROUTE_FUSED = 0, ROUTE_SPARSE_IN_SOLVE, ROUTE_SPARSE_WHITENED, ROUTE_SPARSE_SYMMETRIC, ROUTE_SPARSE_TAIL,
                         ROUTE_DENSE_ASCODED, ROUTE_DENSE_WHITENED, ROUTE_DENSE_SYMMETRIC, ROUTE_COUNT };
static const char* kRouteNames[ROUTE_COUNT] = {"fused", "sparse_in_solve", "sparse_whitened", "sparse_symmetric", "sparse_tail",
                                               "dense_ascoded", "dense_whitened", "dense_symmetric"};
struct UpdatePlan {
  int route;
  bool sparse;        // the rows are used in their compressed form
  bool in_solve;      // the covariance update runs inside the solve kernel (one workgroup per filter)
  bool latency;       // few filters: streamed solve on four-wave workgroups + the product on 64 x 64 tiles
  bool stream8;       // N > 256 with a short factor: the streamed solve on eight-wave workgroups
  bool f32_whitened;  // XIVO_HIP_FLAG_FP32_WHITENED applies (the product runs outside the solve kernel because of the SHAPE)
};

// (B = the filters of this pass; with the batch walked in chunks - XIVO_HIP_CHUNK - the few-filter decision is made on the
//  WHOLE call's batch, c->call_batch: chunks of <= 64 filters of a large batch must not take the few-filter kernels)
static UpdatePlan plan_update(const xivo_hip_ctx* c, int b0, int B, bool gate) {
  const StagedRows& r = c->rows;
  const int Np = c->Np, Mp = r.rows_padded();
  const unsigned f = c->flags;
  UpdatePlan p{};
  bool sparse = !(f & XIVO_HIP_FLAG_DENSE_H) && !r.any_over(b0, B);
  const auto [nc_max, pw_max] = r.max_slots(b0, B);
  const bool extra_rows = r.mixed_row0() >= 0 || r.has_lead();     // dense OOS rows / the leading calibration block next to the compressed rows
  // the stand-alone tail's G = T H^T walks compressed rows of ALL of H, and the compact gate of a calibration stacking reads whole rows
  if (sparse && extra_rows && ((f & XIVO_HIP_FLAG_STANDALONE_TAIL) || (r.has_lead() && gate))) sparse = false;
  if (sparse && r.has_lead() && (f & XIVO_HIP_FLAG_SYMMETRIC_FORM)) sparse = false;
  p.sparse = sparse;
  const bool holds = trsm_forms_T(Mp, Np);                          // one workgroup per filter holds the factor and every column of the state
  const int Ball = c->call_batch > B ? c->call_batch : B;
  p.latency = !(f & (XIVO_HIP_FLAG_THROUGHPUT_ROUTE | XIVO_HIP_FLAG_STANDALONE_TAIL | XIVO_HIP_FLAG_SYMMETRIC_FORM)) &&
              trsm_latency_route(Mp, Ball) && (sparse || !(f & XIVO_HIP_FLAG_DENSE_H));
  p.stream8 = !p.latency && Np > 256 && Mp / 16 <= 8;               // (N = 276, M = 120: 2.01 -> 1.39 ms per 4096 filters)
  if (f & XIVO_HIP_FLAG_SYMMETRIC_FORM) { p.route = sparse ? ROUTE_SPARSE_SYMMETRIC : ROUTE_DENSE_SYMMETRIC; p.in_solve = holds; return p; }
  if (!sparse && (f & XIVO_HIP_FLAG_DENSE_H)) { p.route = ROUTE_DENSE_ASCODED; return p; }
  if (sparse && (f & XIVO_HIP_FLAG_STANDALONE_TAIL)) { p.route = ROUTE_SPARSE_TAIL; return p; }
  if (sparse && !extra_rows && !(f & XIVO_HIP_FLAG_MULTI_KERNEL) && nc_max <= 12 && pw_max <= 9 && fused_update_supported(Mp, Np)) {
    p.route = ROUTE_FUSED; p.latency = false; return p;
  }
  p.in_solve = holds && !p.latency;
  p.f32_whitened = (f & XIVO_HIP_FLAG_FP32_WHITENED) && !holds;
  p.route = sparse ? (p.in_solve ? ROUTE_SPARSE_IN_SOLVE : ROUTE_SPARSE_WHITENED) : ROUTE_DENSE_WHITENED;
  return p;
}

// One pass of the update pipeline over filters [b0, b0 + B); `gate` (or null): MH gating of its F features per filter first
struct UpdateGate { int F; GateParams gp; };

// The row-pair compressed rows of filters [b0, ...)
EllBuffers ell_range(const EllBuffers& ell, int b0) {
  EllBuffers e = ell;
  e.idx += (long)b0 * e.stride_idx(); e.val += (long)b0 * e.stride_val(); e.nc += b0; e.pw += b0; e.over += b0;
  return e;
}

// The context's per-filter buffers from filter b0 on: the views of the context (capi_internal.h), each moved to b0.
struct UpdateViews {
  BatchMat P, H, HT, HP, PHT, S, K, G, KHI, T, lead;
  BatchVec invD, inn, diagR, err, y;
  int *status, *ldlt_used;
  EllBuffers ell;
};

UpdateViews views_from(xivo_hip_ctx* c, int b0) {
  return {c->P.from(b0), c->H.from(b0), c->HT.from(b0), c->HP.from(b0), c->PHT.from(b0), c->S.from(b0), c->K.from(b0),
          c->G.from(b0), c->KHI.from(b0), c->T.from(b0), c->Hlead.from(b0),
          c->invD.from(b0), c->inn.from(b0), c->diagR.from(b0), c->err.from(b0), c->yvec.from(b0),
          c->status + b0, c->ldlt_used + b0, ell_range(c->ell, b0)};
}

// S = L L^T (chol_f64.hip) over B filters, the gate folded into its prologue when `cg` is given. `flops`: what the calling
// pipeline counts for the stage.
int factor_S(xivo_hip_ctx* c, const UpdateViews& v, int B, int latency, const CholGateArgs* cg, double flops) {
  const int Mp = c->rows.rows_padded();
  CholArgs a{}; v.S.to(a.S, a.strideS, a.lds); a.Mp = Mp; v.invD.to(a.invD, a.strideInvD);
  a.status = v.status; a.batch = B; a.latency = latency;
  char clabel[64]; chol_kernel_label(Mp, B, clabel, sizeof(clabel));
  if (cg) { const size_t n = strlen(clabel); snprintf(clabel + n, sizeof(clabel) - n, "+gate"); }
  StageTimer st(c, ST_CHOL, flops, clabel, 8.0 * B * ((double)Mp * (Mp + 1) + Mp / 16 * 512.0));
  HIP_TRY((hipError_t)launch_chol_f64(a, c->stream, cg));
  return XIVO_HIP_OK;
}

// The arguments every launch of the substitution kernels shares: the factor, P H^T in, the gain and dx out. The caller adds
// what its form needs (the mode, T / Pm / Yout, joseph, fwd_only / y, latency / stream8 / out_f32).
TrsmArgs trsm_args(const xivo_hip_ctx* c, const UpdateViews& v, int B) {
  TrsmArgs a{}; v.S.to(a.LU, a.strideLU, a.ldlu); v.invD.to(a.invD, a.strideInvD);
  v.PHT.to(a.PHT, a.stridePHT, a.ldpht); v.K.to(a.K, a.strideK, a.ldk);
  v.inn.to(a.inn, a.strideInn); v.err.to(a.err, a.strideErr); a.Mp = c->rows.rows_padded(); a.Np = c->Np; a.batch = B;
  return a;
}
// XIVO_HIP_FLAG_SYMMETRIC_FORM: gain and covariance in the symmetric "square-root" form. With S = L L^T and
// W = L^-1 (H P) (forward substitution only):  K (H P) = W^T W,  dx = K inn = W^T (L^-1 inn),  P+ = P - W^T W.
// This is the covariance the Joseph form of src/estimator.cpp:1276-1287 evaluates to for the optimal gain (the Joseph
// correction term vanishes identically), computed without the backward substitution, the residual G and the second
// N x N x M product; its rounding error grows with cond(L) = sqrt(cond(S)), not cond(S). Opt-in: the reference codes
// the Joseph form, which stays the default.
static int finish_symmetric(xivo_hip_ctx* c, const UpdatePlan& plan, const UpdateViews& v, int B) {
  const int Np = c->Np, Mp = c->rows.rows_padded();
  {
    StageTimer st(c, ST_OTHER, 0.0, "fwd_vec_kernel");
    HIP_TRY((hipError_t)launch_fwd_vec(v.S.p, v.S.stride, v.S.ld, v.invD.p, v.invD.stride, v.inn.p, v.inn.stride, v.y.p, v.y.stride, Mp, B, c->stream));
  }
  {
    TrsmArgs a = trsm_args(c, v, B);
    a.fwd_only = 1; v.y.to(a.y, a.strideY);
    // the solve kernel goes on to P+ = P - W^T W in place, W^T still in its registers (blocks exchanged through LDS)
    const bool p_here = plan.in_solve;
    if (p_here) { v.P.to(a.T, a.strideT, a.ldt); a.skip_status = v.status; }
    char label[64]; trsm_kernel_label(Mp, label, sizeof(label), p_here ? 2 : 0);
    const double outs = 0.5 * Np * (Np + 1.0), Nf = c->N, Mf = c->rows.rows();
    StageTimer st(c, ST_TRSM, (1.0 * Mf * Mf * Nf + (p_here ? Nf * (Nf + 1.0) * Mf : 0.0)) * B, label,
                  8.0 * B * (0.5 * Mp * (Mp + 1) + Mp / 16 * 512.0 + (p_here ? 1.0 : 2.0) * Np * Mp + (p_here ? outs + (double)Np * Np : 0.0)));
    HIP_TRY((hipError_t)launch_trsm_f64(a, c->stream));
    if (p_here) return XIVO_HIP_OK;
  }
  // P+ = P - W^T W in place: the accumulators start at -P (every tile reads its part of P before it stores anything)
  // and the result is negated on the way out
  GemmExtra x; x.epi = EPI_RSUB_MAT; x.msub = v.P; x.lower_only = 1;
  x.skip = v.status;
  return gemm(c, ST_PNEW, B, Np, Np, {v.K, v.K, Mp}, v.P, x);
}

// XIVO_HIP_FLAG_FP32_WHITENED: both whitened outputs left the solve as FLOAT in the G buffer - Y^T at float 0, V^T at float
// Np Mp (TrsmArgs::out_f32). As operands of a product that reads floats (GemmExtra::a_f32 / b_f32: leading dimension and
// stride count ELEMENTS): the same leading dimension, twice the stride of the buffer of doubles.
struct WhitenedF32 { BatchMat V, Y; };
static WhitenedF32 whitened_f32(const BatchMat& G, int Np, int Mp) {
  double* V = reinterpret_cast<double*>(reinterpret_cast<float*>(G.p) + (long)Np * Mp);
  return {BatchMat{V, 2 * G.stride, G.ld}, BatchMat{G.p, 2 * G.stride, G.ld}};
}

// The factorisation, the gain, dx and the covariance update once P H^T and S are formed - shared by the sparse and the dense
// whitened pipelines (they differ in how H P and S are built, not behind them):
//   S = L L^T (gate folded into its prologue when `cg` is given)                 estimator.cpp:1266
//   in_solve : W = L^-1 (HP), K^T = L^-T W, dx, P+ = P - (W - D)^T (W + D) inside the solve kernel  estimator.cpp:1265-1287
//   else     : V^T, Y^T leave the (chunked / streamed) solve, P+ = P - V^T Y as one tiled symmetric product
static int finish_whitened(xivo_hip_ctx* c, const UpdatePlan& plan, const UpdateViews& v, int B, const CholGateArgs* cg) {
  const int Np = c->Np, Mp = c->rows.rows_padded();
  const double Nf = c->N, Mf = c->rows.rows();
  // (the streamed solve reads the mirrored upper triangle)
  int rc = factor_S(c, v, B, plan.latency || plan.stream8, cg, Mf * Mf * Mf / 3.0 * B);
  if (rc) return rc;
  {
    TrsmArgs a = trsm_args(c, v, B);
    if (plan.in_solve) { v.P.to(a.T, a.strideT, a.ldt); a.joseph = 2; a.skip_status = v.status; }
    else { v.G.to(a.Yout, a.strideY2, a.ldy2); a.latency = plan.latency; a.stream8 = plan.stream8 ? 1 : 0; a.out_f32 = plan.f32_whitened ? 1 : 0; }
    char label[64]; trsm_kernel_label(Mp, label, sizeof(label), plan.in_solve ? 4 : 5, plan.latency, plan.stream8);
    // seven block rows on a narrow state: the ten- / twelve-wave instantiation with W in registers (solve_fused.hip)
    const bool narrow = plan.in_solve && trsm_narrow_supported(Mp, Np);
    if (narrow) trsm_narrow_label(Mp, Np, label, sizeof(label));
    const double t_outs = 0.5 * Np * (Np + 1.0), t_outs_f = 0.5 * Nf * (Nf + 1.0);
    // algorithmic flops (true N, M): the two triangular solves (M^2 N each), the residual blocks of the whitened form
    // (2 * 16 * M * N) and, in the solve kernel, the symmetric N x N x M product (lower triangle). Algorithmic bytes: the
    // factor, P H^T once, P's lower triangle in, P out (the gain is not stored)
    StageTimer st(c, ST_TRSM, (2.0 * Mf * Mf * Nf + 32.0 * Mf * Nf + (plan.in_solve ? 2.0 * t_outs_f * Mf : 0.0)) * B, label,
                  8.0 * B * (0.5 * Mp * (Mp + 1) + Mp / 16 * 512.0 + (plan.in_solve ? 1.0 : 3.0) * Np * Mp + (plan.in_solve ? t_outs + (double)Np * Np : 0.0)));
    HIP_TRY((hipError_t)(narrow ? launch_trsm_narrow(a, c->stream) : launch_trsm_f64(a, c->stream)));
    if (plan.in_solve) return XIVO_HIP_OK;
  }
  // P+ = P - V^T Y in place (V^T in the K buffer, Y^T in the G buffer), lower triangle + mirror
  GemmExtra x; x.epi = EPI_RSUB_MAT; x.msub = v.P; x.lower_only = 1; x.skip = v.status;
  x.small_tiles = plan.latency;
  if (plan.f32_whitened) {
    x.fp32 = 1; x.a_f32 = 1; x.b_f32 = 1;
    const WhitenedF32 w = whitened_f32(v.G, Np, Mp);
    return gemm(c, ST_PNEW, B, Np, Np, {w.V, w.Y, Mp}, v.P, x);
  }
  return gemm(c, ST_PNEW, B, Np, Np, {v.K, v.G, Mp}, v.P, x);
}

// Sparse-H pipelines (ell.h): H P, S and T H^T skip the structural zeros of H; the factorisation, the gain and the
// N x N x M covariance products stay on the MFMA kernels.
//   FUSED            everything in one kernel per filter                                     fused_update.hip
//   otherwise        HP = H P (+ P H^T)            ell_mul<HP>                               estimator.cpp:1259
//                    S = (HP) H^T + R              ell_mul<S>                                estimator.cpp:1259-1263
//                    [MH gating]                   in the prologue of the factorisation / gate_ell    update.cpp:60-96
//                    then finish_whitened / finish_symmetric, or (SPARSE_TAIL)
//                    T = K (HP) - P, G = T H^T + K R, P+ = G K^T - T                          estimator.cpp:1276-1287 re-associated
static int update_sparse_range(xivo_hip_ctx* c, const UpdatePlan& plan, const UpdateViews& v, int b0, int B, const UpdateGate* gate) {
  const int Np = c->Np, Mp = c->rows.rows_padded();
  const BatchMat &P = v.P, &HP = v.HP, &PHT = v.PHT, &S = v.S, &K = v.K, &G = v.G, &T = v.T;
  const BatchVec &inn = v.inn, &diagR = v.diagR;
  const EllBuffers& e = v.ell;
  const auto [nc_max, pw_max] = c->rows.max_slots(b0, B);
  // algorithmic flops are counted on the TRUE sizes N, M (the padded Np, Mp only size the launches and the bytes)
  const double Nf = c->N, Mf = c->rows.rows();
  const double nnz_flops = 2.0 * Mf * 21.0;   // per contiguous-index value: 21 structural non-zeros per row
  int rc;
  if (plan.route == ROUTE_FUSED) {
    // Round 6: the shapes a CU holds (TUM-VI 203 / 60, BASELINE config 2 150 / 100) take ONE kernel for the whole update -
    // P H^T, S, the gate, the factor, both substitutions and the covariance product stay in the registers and the LDS of the
    // workgroup that owns the filter; nothing but P, P+ and the compressed rows crosses HBM.
    FusedArgs a{};
    P.to(a.P, a.strideP, a.ldp); a.ell = e; inn.to(a.inn, a.strideInn); diagR.to(a.diagR, a.strideR);
    v.err.to(a.err, a.strideErr); PHT.to(a.PHT, a.stridePHT, a.ldpht); a.status = v.status;
    a.Np = Np; a.Mp = Mp; a.batch = B; a.pw = pw_max;
    if (gate) {
      a.gate = 1; a.F = gate->F; a.gp = gate->gp;
      a.mask = c->mask + (long)b0 * gate->F; a.dist = c->dist + (long)b0 * gate->F;
      if (c->rows.dense_alive()) { v.H.to(a.H, a.strideH, a.ldh); v.HT.to(a.HT, a.strideHT, a.ldht); }
    }
    char label[64]; fused_update_label(Mp, Np, pw_max, label, sizeof(label));
    const double t_outs_f = 0.5 * Nf * (Nf + 1.0);
    StageTimer st(c, ST_TRSM, (nnz_flops * (Nf + Mf) + Mf * Mf * Mf / 3.0 + 2.0 * Mf * Mf * Nf + 32.0 * Mf * Nf + 2.0 * t_outs_f * Mf) * B, label,
                  B * (16.0 * Np * Np + (Mp / 2) * ELL_W * 20.0));
    HIP_TRY((hipError_t)launch_fused_update(a, c->stream));
    return XIVO_HIP_OK;
  }
  // mixed stacking: rows [0, mr0) of H are the compressed in-state rows, rows [mr0, M) the dense OOS rows appended by
  // xivo_hip_oos_project (non-zero over the extrinsics + group columns only: src/oos.cpp:74-88). The in-state rows keep the
  // sparse walk below; the OOS block goes through two small MFMA products (rows padded to 16 from mr0 on).
  const int mr0 = c->rows.mixed_row0();
  const int Mp_ell = mr0 >= 0 ? round_up16(mr0) : Mp;
  const int oos_pad = mr0 >= 0 ? round_up16(Mp - mr0) : 0;
  // the OOS rows are zero beyond the extrinsics and group columns (the mode clears and writes nothing else there): the two
  // products of the OOS block contract over the leading oos_k state columns only
  bool walk_tiled = false;
  const int oos_k = (mr0 >= 0 && c->have_layout) ? std::min(Np, round_up16(c->lay.group_begin + 6 * c->lay.n_groups)) : Np;
  {
    EllMulArgs a{}; a.ell = e; P.to(a.Src, a.strideSrc, a.ldsrc); PHT.to(a.out, a.strideOut, a.ldo);
    HP.to(a.out2, a.strideOut2, a.ldo2); a.X = Np; a.Mp = Mp_ell; a.batch = B; a.nc_max = nc_max; a.pw_max = pw_max; a.cols = Np;
    char label[64]; ell_kernel_label(ELL_HP, a, label, sizeof(label));
    walk_tiled = ell_uses_slab_form(a);   // (the same decision for ell<S> below: it depends on the shape and slot counts only)
    StageTimer st(c, ST_HP, nnz_flops * Nf * B, label, 8.0 * B * ((double)Np * Np + (double)Np * Mp));
    HIP_TRY((hipError_t)launch_ell_mul(ELL_HP, a, c->stream));
  }
  if (mr0 >= 0) {   // (H P)_oos = H_oos P, with its transpose into the P H^T columns behind the in-state ones
    GemmExtra x; x.C2 = PHT.at(0, mr0);
    rc = gemm(c, ST_HP, B, oos_pad, Np, {v.H.at(mr0, 0), P, oos_k}, HP.at(mr0, 0), x);
    if (rc) return rc;
  }
  // online-calibration stacking on the sparse pipeline: the calibration columns of H live in the leading dense block
  // L [Mp x LEAD_K] (stack_kernel, laid out on the allocated row count): P H^T += P[:, 0:LEAD_K] L^T on the MFMA product
  const bool lead = c->rows.has_lead() && mr0 < 0;
  if (lead) {
    // (the tiled walk writes P H^T only: this product completes it in place and leaves H P as its transposed copy - the
    //  leading LEAD_K columns the S product below reads, or all of it where ell<S> takes the gather form, which reads H P)
    GemmExtra x; x.epi = EPI_ADD_MAT; x.msub = PHT; x.C2 = HP;
    x.c2_rows = walk_tiled ? LEAD_K : 0;
    rc = gemm(c, ST_HP, B, Np, Mp, {P, v.lead, LEAD_K}, PHT, x);
    if (rc) return rc;
  }
  GateEllArgs ga{};
  if (gate) {
    ga.ell = e;
    v.H.to(ga.H, ga.strideH, ga.ldh); v.HT.to(ga.HT, ga.strideHT, ga.ldht);
    if (!c->rows.dense_alive()) { ga.H = nullptr; ga.HT = nullptr; }
    ga.PHT = PHT.p;   // (H P [Mp x Np] has no reader behind this point: S is formed already, the solve reads P H^T)
    inn.to(ga.inn, ga.strideInn); diagR.to(ga.diagR, ga.strideR);
    ga.mask = c->mask + (long)b0 * gate->F; ga.dist = c->dist + (long)b0 * gate->F;
    ga.F = gate->F; ga.Np = Np; ga.batch = B;
    S.to(ga.S, ga.strideS, ga.lds); ga.Mp = Mp; ga.gp = gate->gp;   // distances from the diagonal blocks of S
  }
  // the compact copy of the 2 x 2 diagonal blocks of S lives in the T buffer (free until the solve): 2 Mp doubles per filter
  const BatchVec Sdiag{T.p, T.stride};
  int diag_done = 0;
  {
    EllMulArgs a{}; a.ell = e; PHT.to(a.Src, a.strideSrc, a.ldsrc); HP.to(a.SrcAlt, a.strideSrcAlt, a.ldsrcAlt);
    S.to(a.out, a.strideOut, a.ldo); a.cols = Np;
    diagR.to(a.diagR, a.strideR); a.X = Mp; a.Mp = Mp_ell; a.batch = B; a.nc_max = nc_max; a.pw_max = pw_max;
    // the lead product below starts its accumulators from S and, on 96 x 96 tiles, runs its diagonal tiles in full: it reads
    // the 16 x 16 blocks above the diagonal inside them (and drops what it made of them) - S keeps them for it
    a.keep_upper = lead ? 1 : 0;
    // the 2 x 2 diagonal blocks of S once more, compact: what the gate reads
    if (gate && mr0 < 0 && !lead && (long)2 * Mp <= Sdiag.stride) { Sdiag.to(a.diag_out, a.strideDiag); a.diag_done = &diag_done; }
    char label[64]; ell_kernel_label(ELL_S, a, label, sizeof(label));
    StageTimer st(c, ST_S, nnz_flops * Mf * B, label, B * (8.0 * Np * Mp + ell_s_bytes_written(a)));
    HIP_TRY((hipError_t)launch_ell_mul(ELL_S, a, c->stream));
  }
  if (mr0 >= 0) {   // the OOS x OOS block of S (the OOS x in-state block came out of the walk above: rows of S run over all M)
    GemmExtra x; x.epi = EPI_ADD_DIAG; x.diag = BatchVec{diagR.p + mr0, diagR.stride}; x.lower_only = 1;
    rc = gemm(c, ST_S, B, oos_pad, oos_pad, {HP.at(mr0, 0), v.H.at(mr0, 0), oos_k}, S.at(mr0, mr0), x);
    if (rc) return rc;
  }
  if (lead) {
    // S += (H P)[:, 0:LEAD_K] L^T. The walk above left, in the lower triangle, S[i, j] = sum over the COMPRESSED columns k of
    // row j of (H P)[i, k] H[j, k] with the complete H P: what is missing is the same sum over row j's calibration columns
    // (the order of the operands matters - L (H P)^T is the transpose, and neither term is symmetric on its own)
    GemmExtra x; x.epi = EPI_ADD_MAT; x.msub = S; x.lower_only = 1;
    rc = gemm(c, ST_S, B, Mp, Mp, {HP, v.lead, LEAD_K}, S, x);
    if (rc) return rc;
  }
  // With thousands of factors the gate rides in the prologue of the factorisation (chol_f64.hip, GATE): the distances come
  // from the compact diagonal blocks ell<S> just left, the rejected pairs are decoupled where the factor loads S - no gate
  // launch, no extra pass over S. (Few filters, dense copies of H alive, mixed stacking: the gate kernel.)
  CholGateArgs cg{};
  bool gate_folded = false;
  if (gate) {
    if (diag_done) Sdiag.to(ga.Sdiag, ga.strideSdiag);
    gate_folded = diag_done && !c->rows.dense_alive() && mr0 < 0 && !plan.latency && chol_gate_supported(Mp, B);
    if (gate_folded) {
      Sdiag.to(cg.Sdiag, cg.strideSdiag); inn.to(cg.inn, cg.strideInn); diagR.to(cg.diagR, cg.strideR);
      cg.ellval = e.val; cg.strideVal = e.stride_val(); cg.ell_w = ELL_W; PHT.to(cg.PHT, cg.stridePHT, cg.ldpht); cg.Np = Np;
      cg.mask = ga.mask; cg.dist = ga.dist; cg.F = gate->F; cg.gp = gate->gp;
    } else {
      StageTimer st(c, ST_GATE, 0.0, "gate_ell_kernel");
      HIP_TRY((hipError_t)launch_gate_ell(ga, c->stream));
    }
  }
  if (plan.route != ROUTE_SPARSE_TAIL && plan.route != ROUTE_SPARSE_SYMMETRIC)
    return finish_whitened(c, plan, v, B, gate_folded ? &cg : nullptr);
  rc = factor_S(c, v, B, 0, gate_folded ? &cg : nullptr, Mf * Mf * Mf / 3.0 * B);
  if (rc) return rc;
  if (plan.route == ROUTE_SPARSE_SYMMETRIC) return finish_symmetric(c, plan, v, B);
  // ---- SPARSE_TAIL (XIVO_HIP_FLAG_STANDALONE_TAIL): K^T = S^-1 (HP), dx; T = K (HP) - P; G = T H^T + K R; P+ = G K^T - T
  const bool t_here = trsm_forms_T(Mp, Np);      // the solve forms T on the gain still in its registers
  {
    TrsmArgs a = trsm_args(c, v, B);
    if (t_here) { T.to(a.T, a.strideT, a.ldt); P.to(a.Pm, a.stridePm, a.ldpm); }
    char label[64]; trsm_kernel_label(Mp, label, sizeof(label), t_here ? 1 : 0);
    const double t_outs = 0.5 * Np * (Np + 1.0), t_outs_f = 0.5 * Nf * (Nf + 1.0);
    StageTimer st(c, ST_TRSM, (2.0 * Mf * Mf * Nf + (t_here ? 2.0 * t_outs_f * Mf : 0.0)) * B, label,
                  8.0 * B * (0.5 * Mp * (Mp + 1) + Mp / 16 * 512.0 + 2.0 * Np * Mp + (t_here ? t_outs + (double)Np * Np : 0.0)));
    HIP_TRY((hipError_t)launch_trsm_f64(a, c->stream));
  }
  if (!t_here) {  // T = K (HP) - P = (HP)^T S^-1 (HP) - P: symmetric up to the rounding of the solve, so the lower
                  // triangle is computed and mirrored
    GemmExtra x; x.epi = EPI_SUB_MAT; x.msub = P; x.lower_only = 1;
    rc = gemm(c, ST_AP, B, Np, Np, {K, PHT, Mp}, T, x);
    if (rc) return rc;
  }
  {  // G = T H^T + K diag(R)   [Np x Mp, in the A buffer]
    EllMulArgs a{}; a.ell = e; T.to(a.Src, a.strideSrc, a.ldsrc); G.to(a.out, a.strideOut, a.ldo);
    diagR.to(a.diagR, a.strideR); K.to(a.K, a.strideK, a.ldk); a.X = Np; a.Mp = Mp; a.batch = B; a.nc_max = nc_max; a.pw_max = pw_max; a.cols = Np;
    char label[64]; ell_kernel_label(ELL_G, a, label, sizeof(label));
    StageTimer st(c, ST_KH, nnz_flops * Np * B, label, 8.0 * B * ((double)Np * Np + 2.0 * Np * Mp));
    HIP_TRY((hipError_t)launch_ell_mul(ELL_G, a, c->stream));
  }
  if (pnew_reg_supported(Mp, Np)) {
    // P+ = G K^T - T, all fp64: rows of G in registers, blocks of K through LDS, one workgroup per filter
    PnewRegArgs a{}; G.to(a.G, a.strideG, a.ldg); K.to(a.K, a.strideK, a.ldk);
    T.to(a.T, a.strideT, a.ldt); P.to(a.P, a.strideP, a.ldp);
    a.skip_status = v.status; a.Mp = Mp; a.Np = Np; a.batch = B;
    char label[64]; pnew_reg_kernel_label(Mp, label, sizeof(label));
    const double outs = 0.5 * Np * (Np + 1.0);
    StageTimer st(c, ST_PNEW, 2.0 * outs * Mp * B, label, 8.0 * B * (2.0 * Np * Mp + outs + (double)Np * Np));
    HIP_TRY((hipError_t)launch_pnew_reg_f64(a, c->stream));
    return XIVO_HIP_OK;
  }
  // P+ = G K^T - T   (lower triangle + mirror)
  GemmExtra x; x.epi = EPI_SUB_MAT; x.msub = T; x.lower_only = 1;
  x.skip = v.status;   // S not positive definite: P of that filter stays the prior (reported through xivo_hip_get_status)
  return gemm(c, ST_PNEW, B, Np, Np, {G, K, Mp}, P, x);
}

static int update_dense_range(xivo_hip_ctx* c, const UpdatePlan& plan, const UpdateViews& v, int b0, int B, const UpdateGate* gate) {
  const int Np = c->Np, Mp = c->rows.rows_padded();
  const BatchMat &H = v.H, &HT = v.HT, &P = v.P, &HP = v.HP, &PHT = v.PHT, &S = v.S, &K = v.K, &A = v.KHI, &T = v.T;
  int rc = ensure_dense(c);   // (mixed stacking / a leading block: the in-state rows are rebuilt densely next to the rows already in place)
  if (rc) return rc;
  {  // HP = H * P and its transpose PH^T (estimator.cpp:1259 first product; P symmetric => B operand = P rows)
    GemmExtra x; x.C2 = PHT;
    rc = gemm(c, ST_HP, B, Mp, Np, {H, P, Np}, HP, x);
    if (rc) return rc;
  }
  if (gate) {  // Estimator::MHGating on the rows just multiplied (update.cpp:60-96): S_f = (HP)_f H_f^T + R
    rc = ensure_HT(c);   // the gate reads (and neutralises) the transposed rows
    if (rc) return rc;
    GateDenseArgs a{};
    H.to(a.Hw, a.strideH, a.ldh); HT.to(a.HTw, a.strideHT, a.ldht);
    HP.to(a.HPw, a.strideHP, a.ldhp); a.PHTw = PHT.p; a.PHTr = PHT.p;
    v.inn.to(a.inn, a.strideInn); v.diagR.to(a.diagR, a.strideR);
    a.mask = c->mask + (long)b0 * gate->F; a.dist = c->dist + (long)b0 * gate->F;
    a.F = gate->F; a.Np = Np; a.batch = B;
    a.gp = gate->gp;
    a.ell = c->ell; a.have_ell = 0;
    StageTimer st(c, ST_GATE, 0.0, "gate_dense_kernel");
    HIP_TRY((hipError_t)launch_gate_dense(a, c->stream));
  }
  {  // S = HP * H^T + diag(R)  (estimator.cpp:1259-1263); lower triangle + mirror
    GemmExtra x; x.epi = EPI_ADD_DIAG; x.diag = v.diagR; x.lower_only = 1;
    rc = gemm(c, ST_S, B, Mp, Mp, {HP, H, Np}, S, x);
    if (rc) return rc;
  }
  if (plan.route == ROUTE_DENSE_WHITENED)      // an H without XIVO's row structure: everything behind S as on the sparse pipeline
    return finish_whitened(c, plan, v, B, nullptr);
  rc = factor_S(c, v, B, 0, nullptr, (double)Mp * Mp * Mp / 3.0 * B);   // S = L L^T (flops counted on the padded size)
  if (rc) return rc;
  if (plan.route == ROUTE_DENSE_SYMMETRIC) return finish_symmetric(c, plan, v, B);
  // ---- DENSE_ASCODED (XIVO_HIP_FLAG_DENSE_H): the products of estimator.cpp:1265-1287 as they are written
  {  // K^T = S^-1 HP ; dx = K inn  (estimator.cpp:1265-1267)
    TrsmArgs a = trsm_args(c, v, B);
    char label[64]; trsm_kernel_label(Mp, label, sizeof(label), 0);
    StageTimer st(c, ST_TRSM, 2.0 * Mp * Mp * Np * B, label, 8.0 * B * (0.5 * Mp * (Mp + 1) + Mp / 16 * 512.0 + 2.0 * Np * Mp));
    HIP_TRY((hipError_t)launch_trsm_f64(a, c->stream));
  }
  rc = ensure_HT(c);
  if (rc) return rc;
  {  // A = K * H - I  (estimator.cpp:1276-1279)
    GemmExtra x; x.epi = EPI_SUB_IDENT;
    rc = gemm(c, ST_KH, B, Np, Np, {K, HT, Mp}, A, x);
    if (rc) return rc;
  }
  {  // T = A * P = K * (HP) - P  (estimator.cpp:1280, left product; distributes over the already
     // formed HP, 2MN^2 instead of 2N^3 flops, same value up to rounding)
    GemmExtra x; x.epi = EPI_SUB_MAT; x.msub = P;
    rc = gemm(c, ST_AP, B, Np, Np, {K, PHT, Mp}, T, x);
    if (rc) return rc;
  }
  {  // P = T * A^T + K diag(R) K^T  (estimator.cpp:1280-1287, fused; lower triangle + mirror)
    GemmExtra x; x.lower_only = 1;
    x.skip = v.status;
    x.seg1 = {K, K, Mp}; x.scale1 = v.diagR;
    rc = gemm(c, ST_PNEW, B, Np, Np, {T, A, Np}, P, x);
  }
  return rc;
}

// One pass of the update over filters [b0, b0 + B), then the device answer to a filter whose S the un-pivoted Cholesky
// could not factor: Eigen's diagonally pivoted L D L^T (what src/estimator.cpp:1266 runs for EVERY filter) and the
// as-coded Joseph update, on exactly those filters (ldlt_fallback.hip). Every pipeline leaves the covariance of such a
// filter untouched and its status set, so the fallback starts from the prior.
static int update_joseph_range(xivo_hip_ctx* c, int b0, int B, const UpdateGate* gate = nullptr) {
  const UpdateViews v = views_from(c, b0);
  const UpdatePlan plan = plan_update(c, b0, B, gate != nullptr);
  c->last_path = plan.sparse ? 1 : 0;
  c->last_route = plan.route;
  if (gate) c->rows.gate_wrote(GateLayout::packed);   // every route's gate writes mask / dist [B][F]
  int rc = plan.sparse ? update_sparse_range(c, plan, v, b0, B, gate) : update_dense_range(c, plan, v, b0, B, gate);
  if (rc || (c->flags & XIVO_HIP_FLAG_NO_LDLT_FALLBACK)) {   // no fallback launch: clear the flags of this call here
    HIP_TRY(hipMemsetAsync(v.ldlt_used, 0, (size_t)B * sizeof(int), c->stream));
    return rc;
  }
  // (the fallback kernel writes ldlt_used of EVERY filter of the range: 0 where the Cholesky succeeded, 1 where it stepped in)
  LdltFallbackArgs a{};
  a.status = v.status; a.used = v.ldlt_used; a.ell = v.ell;
  v.H.to(a.H, a.strideH, a.ldh); a.use_dense = c->last_path == 0 ? 1 : 0;
  a.mixed_row0 = c->last_path == 1 ? c->rows.mixed_row0() : -1;
  if (c->last_path == 1 && c->rows.has_lead()) { v.lead.to(a.lead, a.strideLead, a.ldlead); a.lead_k = LEAD_K; }
  v.PHT.to(a.PHT, a.stridePHT, a.ldpht); v.S.to(a.S, a.strideS, a.lds); v.K.to(a.K, a.strideK, a.ldk);
  v.G.to(a.A, a.strideA, a.lda); v.T.to(a.T, a.strideT, a.ldt); v.P.to(a.P, a.strideP, a.ldp);
  v.inn.to(a.inn, a.strideInn); v.diagR.to(a.diagR, a.strideR); v.err.to(a.err, a.strideErr);
  a.N = c->N; a.M = c->rows.rows(); a.batch = B;
  StageTimer st(c, ST_OTHER, 0.0, "ldlt_fallback_kernel");
  HIP_TRY((hipError_t)launch_ldlt_fallback(a, c->stream));
  return XIVO_HIP_OK;
}

// Filters are independent, so the batch is walked in chunks (XIVO_HIP_CHUNK) whose intermediates (HP, PH^T, S, K, A, T:
// ~2.7 MB per filter at N=250/M=160) stay resident in the 256 MiB Infinity Cache between consecutive kernels instead of
// round-tripping HBM.
static int update_chunks(xivo_hip_ctx* c, int B, const UpdateGate* gate) {
  const int chunk = c->chunk > 0 ? c->chunk : B;
  c->call_batch = chunk < B ? B : 0;
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int nb = B - b0 < chunk ? B - b0 : chunk;
    int rc = update_joseph_range(c, b0, nb, gate);
    if (rc) { c->call_batch = 0; c->dx_clear(); return rc; }
  }
  c->call_batch = 0;
  c->dx_set(0, B, true);   // err holds the dx of the staged rows until something absorbs it or stages new rows (innovation log)
  return XIVO_HIP_OK;
}

// ------------------------------------------------------------------ one-filter plumbing call
// Estimator::UpdateJosephForm() as the reference calls it (src/update.cpp:141, :332): members in host memory in, members in
// host memory out, ONE call, ONE host synchronisation. See include/xivo_hip.h.
// Row-pair compression of ONE dense H_ on the host: the arithmetic-free format conversion meas_compress_kernel does for a
// batch (ell_kernels.hip - same lists, same common-column rule, same slot order, so the rows are those the device would have
// built, bit for bit), done while the matrix is staged: the host has to touch every byte of H_ once anyway, and the
// compressed rows are 1/7 of it. Returns over (1: the rows do not fit the compressed form).
static int host_compress(xivo_hip_ctx::HostCompressScratch& sc, const double* H, int ldh, int M, int N, int pairs_clear, int* idx,
                         double* val, int* nc_out, int* pw_out) {
  const int pairs = (M + 1) / 2;
  sc.cnt.assign(pairs_clear, 0); sc.occ.assign(N, 0); sc.cslot.assign(N, 0);
  sc.n.resize((size_t)pairs_clear * ELL_W); sc.v.resize((size_t)pairs_clear * ELL_W * 2);
  int* cnt = sc.cnt.data(); int* occ = sc.occ.data(); int* cslot = sc.cslot.data();
  int* ln = sc.n.data(); double* lv = sc.v.data();
  const int Me = M & ~1;                            // rows covered by complete pairs
  for (int n = 0; n < N; ++n) {
    const double* col = H + (size_t)n * ldh;
    const uint64_t* cb = reinterpret_cast<const uint64_t*>(col);
    int m = 0;
    for (; m + 8 <= Me; m += 8) {                   // four pairs at a time: all-zero runs (most of H_) cost one test
      const uint64_t any = cb[m] | cb[m + 1] | cb[m + 2] | cb[m + 3] | cb[m + 4] | cb[m + 5] | cb[m + 6] | cb[m + 7];
      if ((any << 1) == 0) continue;                // +0.0 / -0.0 only
      for (int q = m; q < m + 8; q += 2) {
        const double v0 = col[q], v1 = col[q + 1];
        if (v0 != 0.0 || v1 != 0.0) {
          const int p = q >> 1;
          if (cnt[p] < ELL_W) { ln[p * ELL_W + cnt[p]] = n; lv[2 * (p * ELL_W + cnt[p])] = v0; lv[2 * (p * ELL_W + cnt[p]) + 1] = v1; }
          ++cnt[p]; ++occ[n];
        }
      }
    }
    for (; m < M; m += 2) {
      const double v0 = col[m], v1 = m + 1 < M ? col[m + 1] : 0.0;
      if (v0 != 0.0 || v1 != 0.0) {
        const int p = m >> 1;
        if (cnt[p] < ELL_W) { ln[p * ELL_W + cnt[p]] = n; lv[2 * (p * ELL_W + cnt[p])] = v0; lv[2 * (p * ELL_W + cnt[p]) + 1] = v1; }
        ++cnt[p]; ++occ[n];
      }
    }
  }
  int ne = 0;
  for (int p = 0; p < pairs; ++p) ne += cnt[p] > 0;
  int ccols[ELL_CW] = {0};
  int flagged = 0;
  for (int n = 0; n < N; ++n) {                     // columns used by more than half of the non-empty pairs, ascending
    if (ne > 0 && 2 * occ[n] > ne) {
      if (flagged < ELL_CW) { cslot[n] = flagged + 1; ccols[flagged] = n; }
      ++flagged;
    }
  }
  const int nc = flagged < ELL_CW ? flagged : ELL_CW;
  int pw = 0, over = 0;
  for (int p = 0; p < pairs_clear; ++p) {
    int* pi = idx + (size_t)p * ELL_W;
    double* pv = val + (size_t)p * ELL_W * 2;
    for (int t = 0; t < ELL_W; ++t) { pi[t] = t < nc ? ccols[t] : 0; pv[2 * t] = 0.0; pv[2 * t + 1] = 0.0; }
    int pos = 0;
    const int walk = cnt[p] < ELL_W ? cnt[p] : ELL_W;
    for (int k = 0; k < walk; ++k) {
      const int n = ln[p * ELL_W + k];
      const double v0 = lv[2 * (p * ELL_W + k)], v1 = lv[2 * (p * ELL_W + k) + 1];
      const int cs = cslot[n];
      if (cs) { pv[2 * (cs - 1)] = v0; pv[2 * (cs - 1) + 1] = v1; }
      else {
        if (pos < ELL_PW) { pi[ELL_CW + pos] = n; pv[2 * (ELL_CW + pos)] = v0; pv[2 * (ELL_CW + pos) + 1] = v1; }
        ++pos;
      }
    }
    if (cnt[p] > ELL_W) pos = ELL_PW + 1;           // more than 28 non-zero columns cannot fit
    if (pos > ELL_PW) over = 1;
    if (pos > pw) pw = pos;
  }
  *nc_out = nc; *pw_out = pw;
  return over;
}

}  // namespace

namespace xivo_hip::capi {

// Hand-over of dense measurements that already live in device memory (dH: M x N column-major per filter): ONE
// launch builds the row-pair compressed rows of the whole range; the padded dense copies are written only for
// the filters that do not fit it (they take the dense pipeline) and otherwise rebuilt from the compressed rows
// on demand (ensure_dense).
int stage_measurements(xivo_hip_ctx* c, int b0, int nb, int M, const double* dH, long strideH, int ldh,
                       const double* dInn, long strideInn, const double* dR, long strideR) {
  const int N = c->N;
  const MeasBuffers mb = meas_buffers(c, b0);
  const EllBuffers e = ell_range(c->ell, b0);
  // (XIVO_HIP_NO_COMPRESS: test hook for the branch very wide states take - the shape limit itself is N > ~2800 at M = 384)
  static const bool no_compress = getenv("XIVO_HIP_NO_COMPRESS") != nullptr;
  const bool compressed = meas_compress_fits(c->Mpmax, c->Np) && !no_compress;
  c->rows.handed_over(b0, nb, M, compressed);
  c->dx_set(b0, nb, false);   // (a hand-over in pieces leaves the other filters' rows alone)
  if (!compressed) {
    // the compression kernel's LDS lists do not fit this shape: every filter keeps its dense rows and takes the dense pipeline
    StageTimer st(c, ST_STACK, 0.0, "unpack_meas_kernel", 8.0 * nb * (3.0 * M * N + 4.0 * M));
    HIP_TRY((hipError_t)launch_meas_vectors(dInn, strideInn, dR, strideR, M, c->Mpmax, e, mb.inn, mb.strideInn, mb.diagR, mb.strideR, nb, c->stream));
    HIP_TRY((hipError_t)launch_unpack_meas(dH, strideH, ldh, nullptr, mb, M, c->Mpmax, N, c->Np, nb, c->stream));
    return XIVO_HIP_OK;
  }
  {
    StageTimer st(c, ST_STACK, 0.0, "meas_compress_kernel", 8.0 * nb * ((double)M * N + 4.0 * M) + (double)nb * c->ell.pairs_max * ELL_W * 20.0);
    // clear up to the allocated row count so stale rows of a previous, larger M vanish
    HIP_TRY((hipError_t)launch_meas_compress(dH, strideH, ldh, dInn, strideInn, dR, strideR, M, N, c->Np, c->Mpmax, e, mb.inn,
                                             mb.strideInn, mb.diagR, mb.strideR, nb, c->stream,
                                             c->ell_flags_d ? c->ell_flags_d + 3 * (long)b0 : nullptr));
  }
  if (c->ell_flags_h) {
    HIP_TRY(hipStreamSynchronize(c->stream));     // kernel end = system-scope release: the mirrored flags are in host memory
    const int* f = c->ell_flags_h + 3 * (long)b0;
    for (int b = 0; b < nb; ++b) c->rows.fit_reported(b0 + b, f[3 * b], f[3 * b + 1], f[3 * b + 2]);
  } else {
    std::vector<int> f(3 * (size_t)nb);   // over | nc | pw
    const int* src[3] = {e.over, e.nc, e.pw};
    for (int k = 0; k < 3; ++k) HIP_TRY(hipMemcpyAsync(f.data() + (size_t)k * nb, src[k], (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int b = 0; b < nb; ++b) c->rows.fit_reported(b0 + b, f[b], f[nb + b], f[2 * nb + b]);
  }
  const bool any_over = c->rows.any_over(b0, nb);
  if (debug_on()) fprintf(stderr, "xivo_hip: hand-over b0=%d nb=%d M=%d any_over=%d nc0=%d pw0=%d\n", b0, nb, M, (int)any_over, c->rows.nc(b0), c->rows.pw(b0));
  if (any_over) HIP_TRY((hipError_t)launch_unpack_meas(dH, strideH, ldh, e.over, mb, M, c->Mpmax, N, c->Np, nb, c->stream));
  return XIVO_HIP_OK;
}

}  // namespace xivo_hip::capi

extern "C" {

int xivo_hip_set_measurements(xivo_hip_ctx* c, int b0, int nb, int M, const double* H, long strideH, int ldh,
                              const double* inn, long strideInn, const double* diagR, long strideR) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !H || !inn || !diagR || M <= 0 || M > c->Mmax || ldh < M) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  const int N = c->N;
  const size_t per = (size_t)M * N + 2 * (size_t)M;
  int rc = ensure_staging(c, (size_t)nb * per);
  if (rc) return rc;
  double* sH = c->staging;
  double* sInn = sH + (size_t)nb * M * N;
  double* sR = sInn + (size_t)nb * M;
  rc = h2d_packed(c, sH, H, nb, M, N, strideH, ldh);
  if (rc) return rc;
  rc = h2d_packed(c, sInn, inn, nb, M, 1, strideInn, M);
  if (rc) return rc;
  rc = h2d_packed(c, sR, diagR, nb, M, 1, strideR, M);
  if (rc) return rc;
  rc = stage_measurements(c, b0, nb, M, sH, (long)M * N, M, sInn, M, sR, M);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));   // host buffers are only borrowed for the call
  return XIVO_HIP_OK;
}

int xivo_hip_set_measurements_device(xivo_hip_ctx* c, int b0, int nb, int M, const double* dH, long strideH, int ldh,
                                     const double* dInn, long strideInn, const double* dR, long strideR) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !dH || !dInn || !dR || M <= 0 || M > c->Mmax || ldh < M || strideH < 0) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  return stage_measurements(c, b0, nb, M, dH, strideH, ldh, dInn, strideInn, dR, strideR);
}

int xivo_hip_update_joseph(xivo_hip_ctx* c, int B) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || B <= 0 || B > c->Bmax || c->rows.rows_padded() <= 0) return XIVO_HIP_ERR_INVALID;
  return update_chunks(c, B, nullptr);
}

int xivo_hip_update_dense_gated(xivo_hip_ctx* c, int B, int F, double R, double mh_thresh, double mh_mult,
                                int min_inliers) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || B <= 0 || B > c->Bmax || c->rows.rows_padded() <= 0 || F <= 0 || 2 * F > c->rows.rows()) return XIVO_HIP_ERR_INVALID;
  const UpdateGate gate{F, {R, mh_thresh, mh_mult, min_inliers}};
  if (bad_gate_params(gate.gp)) return XIVO_HIP_ERR_INVALID;
  if (c->tune.configured()) return XIVO_HIP_ERR_UNSUPPORTED;   // tuning table: one parameter set for all filters is not applied silently
  int rc = ensure_gate_buffers(c, F);
  if (rc) return rc;
  // Estimator::OutlierRejection only gates when F > min_required_inliers_ (src/manager.cpp:635)
  return update_chunks(c, B, F > min_inliers ? &gate : nullptr);
}

int xivo_hip_last_path(xivo_hip_ctx* c) { return c ? c->last_path : -1; }
int xivo_hip_last_route(xivo_hip_ctx* c) { return c ? c->last_route : -1; }
const char* xivo_hip_route_name(int route) { return route >= 0 && route < ROUTE_COUNT ? kRouteNames[route] : ""; }

double xivo_hip_stage_bytes(xivo_hip_ctx* c, int stage) {
  return (c && stage >= 0 && stage < ST_COUNT) ? c->prof.bytes[stage] : 0.0;
}

const char* xivo_hip_stage_kernel(xivo_hip_ctx* c, int stage) {
  return (c && stage >= 0 && stage < ST_COUNT) ? c->prof.kernel[stage] : "";
}

int xivo_hip_get_gate(xivo_hip_ctx* c, int B, int F, unsigned char* mask_out, double* dist_out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || B <= 0 || B > c->Bmax || F <= 0 || !c->mask) return XIVO_HIP_ERR_INVALID;
  // the dense gate packs [B][F]; the layout-faithful gate (xivo_hip_mh_gate / filter_update) strides by Fmax
  const bool strided = c->rows.gate_layout() == GateLayout::strided;
  const size_t ld = strided ? (size_t)c->Fmax : (size_t)F;
  if (strided && F != c->F) return XIVO_HIP_ERR_INVALID;
  if (mask_out) { int rc = d2h_rows(c, mask_out, F, c->mask, ld, F, B); if (rc) return rc; }
  if (dist_out) {
    int rc = d2h_rows(c, dist_out, F * sizeof(double), c->dist, ld * sizeof(double), F * sizeof(double), B);
    if (rc) return rc;
  }
  return XIVO_HIP_OK;
}

int xivo_hip_get_err(xivo_hip_ctx* c, int b0, int nb, double* err, long stride) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !err || stride < c->N) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  return d2h_rows(c, err, (size_t)stride * sizeof(double), c->err.from(b0).p, (size_t)c->err.stride * sizeof(double),
                  (size_t)c->N * sizeof(double), nb);
}

int xivo_hip_get_ldlt_used(xivo_hip_ctx* c, int b0, int nb, int* used) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !used) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  HIP_TRY(hipMemcpyAsync(used, c->ldlt_used + b0, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return XIVO_HIP_OK;
}

int xivo_hip_get_status(xivo_hip_ctx* c, int b0, int nb, int* status) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (bad_range(c, b0, nb) || !status) return XIVO_HIP_ERR_INVALID;
  if (nb == 0) return XIVO_HIP_OK;
  HIP_TRY(hipMemcpyAsync(status, c->status + b0, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int i = 0; i < nb; ++i) if (status[i]) return XIVO_HIP_ERR_NOT_SPD;
  return XIVO_HIP_OK;
}

int xivo_hip_selftest_fused_tiles(int column_blocks, int* per_simd) { return fused_tiles_selftest(column_blocks, per_simd); }
// test hook (no device): the one-kernel update's admission of a padded shape and the invariants of what it would launch
int xivo_hip_selftest_fused_shape(int Mp, int Np, int pw, char* label, int n) {
  return fused_shape_selftest(Mp, Np, pw, label, n > 0 ? (size_t)n : 0);
}

// test hook (no device, no context): the host-side row compression on its own, for the CPU test that pins it to the format
// of ell.h / meas_compress_kernel. idx [pairs_clear][28], val [pairs_clear][28][2]; returns over.
int xivo_hip_selftest_host_compress(const double* H, int ldh, int M, int N, int pairs_clear, int* idx, double* val, int* nc, int* pw) {
  if (!H || !idx || !val || !nc || !pw || M <= 0 || N <= 0 || ldh < M || 2 * pairs_clear < M) return XIVO_HIP_ERR_INVALID;
  xivo_hip_ctx::HostCompressScratch sc;
  return host_compress(sc, H, ldh, M, N, pairs_clear, idx, val, nc, pw);
}

int xivo_hip_update_joseph_host(xivo_hip_ctx* c, int b, int M, const double* H, int ldh, const double* inn,
                                const double* diagR, double* P, int ldp, double* err_out, unsigned mode) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  const bool p_up = !(mode & XIVO_HIP_HOST_P_RESIDENT), p_down = !(mode & XIVO_HIP_HOST_KEEP_P);
  if (bad_range(c, b, 1) || !H || !inn || !diagR || !err_out || M <= 0 || M > c->Mmax || ldh < M ||
      ((p_up || p_down) && (!P || ldp < c->N)))
    return XIVO_HIP_ERR_INVALID;
  const int N = c->N, Np = c->Np, pairs_clear = c->Mpmax / 2;
  // the staged block: compressed rows | inn | diagR | flags | P in | P out | err | status
  auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };
  const size_t o_idx = 0, o_val = al(o_idx + (size_t)pairs_clear * ELL_W * sizeof(int)),
               o_inn = al(o_val + (size_t)pairs_clear * ELL_W * 2 * sizeof(double)), o_R = al(o_inn + (size_t)c->Mpmax * sizeof(double)),
               o_flags = al(o_R + (size_t)c->Mpmax * sizeof(double)), o_Pin = al(o_flags + 4 * sizeof(int)),
               o_Pout = al(o_Pin + (size_t)N * N * sizeof(double)), o_err = al(o_Pout + (size_t)N * N * sizeof(double)),
               o_st = al(o_err + (size_t)N * sizeof(double)), total = al(o_st + 4 * sizeof(int));
  if (!c->pin_h) {
    if (hipHostMalloc(reinterpret_cast<void**>(&c->pin_h), total, hipHostMallocMapped) != hipSuccess) { c->pin_h = nullptr; (void)hipGetLastError(); return XIVO_HIP_ERR_NOMEM; }
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&c->pin_d), c->pin_h, 0) != hipSuccess || !c->pin_d) {
      hipHostFree(c->pin_h); c->pin_h = nullptr; c->pin_d = nullptr; (void)hipGetLastError(); return XIVO_HIP_ERR_HIP;
    }
  }
  // the row-pair compressed rows, built while H_ is staged; an H_ that does not fit them (dense rows, stacked OOS rows) or a
  // context pinned to the dense / fp32 pipelines takes the general entry points - same results, more crossings
  int nc = 0, pw = 0, over = 1;
  const bool want_ell = !(c->flags & XIVO_HIP_FLAG_DENSE_H) && meas_compress_fits(c->Mpmax, Np);
  if (want_ell)
    over = host_compress(c->hc, H, ldh, M, N, pairs_clear, reinterpret_cast<int*>(c->pin_h + o_idx),
                         reinterpret_cast<double*>(c->pin_h + o_val), &nc, &pw);
  if (over) {
    int rc = XIVO_HIP_OK;
    if (p_up) rc = xivo_hip_upload_P(c, b, 1, P, (long)ldp * N, ldp);
    if (!rc) rc = xivo_hip_set_measurements(c, b, 1, M, H, (long)ldh * N, ldh, inn, M, diagR, M);
    if (!rc) rc = update_joseph_range(c, b, 1);
    if (rc) return rc;
    c->dx_set(b, 1, true);
    int st = 0;
    rc = xivo_hip_get_status(c, b, 1, &st);
    if (rc) return rc;
    rc = xivo_hip_get_err(c, b, 1, err_out, N);
    if (!rc && p_down) rc = xivo_hip_download_P(c, b, 1, P, (long)ldp * N, ldp);
    return rc;
  }
  double* s_inn = reinterpret_cast<double*>(c->pin_h + o_inn);
  double* s_R = reinterpret_cast<double*>(c->pin_h + o_R);
  for (int m = 0; m < c->Mpmax; ++m) { s_inn[m] = m < M ? inn[m] : 0.0; s_R[m] = m < M ? diagR[m] : 1.0; }
  int* s_flags = reinterpret_cast<int*>(c->pin_h + o_flags);
  s_flags[0] = nc; s_flags[1] = pw; s_flags[2] = 0;
  // P_ crosses through the context's page-locked block: one host copy each way (~9 us per 500 KB), the boundary kernels
  // read / write the block over PCIe. (Page-locking the caller's own P_ in place - hipHostRegister - saved 18 us per call
  // and was dropped: with large pageable copies elsewhere in the process the runtime's own pinning of recycled heap
  // addresses left the device faulting on the registered pages, scripts/register_stress.py)
  DropinInArgs ia{};
  if (p_up) {
    double* sp = reinterpret_cast<double*>(c->pin_h + o_Pin);   // (the lower triangle is all the device reads: p_unpack_device.h)
    for (int j = 0; j < N; ++j) memcpy(sp + (size_t)j * N + j, P + (size_t)j * ldp + j, (size_t)(N - j) * sizeof(double));
    ia.Psrc = reinterpret_cast<const double*>(c->pin_d + o_Pin); ia.ldps = N;
  }
  const UpdateViews v = views_from(c, b);
  ia.P = v.P.p; ia.N = N; ia.Np = Np; ia.ldp = v.P.ld;
  ia.block = c->pin_d; ia.off_idx = (int)o_idx; ia.off_val = (int)o_val; ia.off_inn = (int)o_inn; ia.off_R = (int)o_R; ia.off_flags = (int)o_flags;
  ia.pairs_clear = pairs_clear; ia.Mpmax = c->Mpmax;
  ia.idx = v.ell.idx; ia.val = v.ell.val; ia.inn = v.inn.p; ia.diagR = v.diagR.p;
  ia.nc = v.ell.nc; ia.pw = v.ell.pw; ia.over = v.ell.over;
  {
    StageTimer st(c, ST_STACK, 0.0, "dropin_in_kernel", (p_up ? 8.0 * N * N : 0.0) + (double)pairs_clear * ELL_W * 20.0 + 16.0 * c->Mpmax);
    HIP_TRY((hipError_t)launch_dropin_in(ia, c->stream));
  }
  // what stage_measurements leaves behind for the pipeline
  c->rows.handed_over(b, 1, M, true); c->rows.fit_reported(b, 0, nc, pw);
  c->dx_set(b, 1, false);
  // (from here on kernels that read the context's pinned block may be in flight: an early return drains the stream first,
  //  the next call overwrites that block)
  int rc = update_joseph_range(c, b, 1);
  if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
  c->dx_set(b, 1, true);
  DropinOutArgs oa{};
  oa.P = v.P.p; oa.N = N; oa.ldp = v.P.ld;
  if (p_down) { oa.Pdst = reinterpret_cast<double*>(c->pin_d + o_Pout); oa.ldpd = N; }
  oa.err = v.err.p; oa.err_dst = reinterpret_cast<double*>(c->pin_d + o_err);
  oa.status = v.status; oa.ldlt_used = v.ldlt_used; oa.flags_dst = reinterpret_cast<int*>(c->pin_d + o_st);
  {
    StageTimer st(c, ST_OTHER, 0.0, "dropin_out_kernel", (p_down ? 8.0 * N * N : 0.0) + 8.0 * N);
    if (launch_dropin_out(oa, c->stream) != 0) { (void)hipStreamSynchronize(c->stream); return XIVO_HIP_ERR_HIP; }
  }
  HIP_TRY(hipStreamSynchronize(c->stream));        // the one synchronisation of the call: kernel end = system-scope release
  const int* s_st = reinterpret_cast<const int*>(c->pin_h + o_st);
  memcpy(err_out, c->pin_h + o_err, (size_t)N * sizeof(double));
  if (p_down) {
    const double* sp = reinterpret_cast<const double*>(c->pin_h + o_Pout);
    if (ldp == N) memcpy(P, sp, (size_t)N * N * sizeof(double));
    else for (int j = 0; j < N; ++j) memcpy(P + (size_t)j * ldp, sp + (size_t)j * N, (size_t)N * sizeof(double));
  }
  return s_st[0] ? XIVO_HIP_ERR_NOT_SPD : XIVO_HIP_OK;
}

int xivo_hip_mh_gate_dense(xivo_hip_ctx* c, int B, int F, double R, double mh_thresh, double mh_mult,
                           int min_inliers, unsigned char* mask_out, double* dist_out) {
  if (c && hipSetDevice(c->device) != hipSuccess) return XIVO_HIP_ERR_HIP;
  if (!c || B <= 0 || B > c->Bmax || F <= 0 || 2 * F > c->rows.rows()) return XIVO_HIP_ERR_INVALID;
  GateDenseArgs a{};
  a.gp = {R, mh_thresh, mh_mult, min_inliers};
  if (bad_gate_params(a.gp)) return XIVO_HIP_ERR_INVALID;
  if (c->tune.configured()) return XIVO_HIP_ERR_UNSUPPORTED;   // tuning table: one parameter set for all filters is not applied silently
  int rc = ensure_gate_buffers(c, F);
  if (rc) return rc;
  rc = ensure_dense(c);
  if (rc) return rc;
  a.mask = c->mask; a.dist = c->dist; a.F = F; a.have_ell = 1;
  rc = gate_dense_rows(c, B, a);
  if (rc) return rc;
  c->rows.gate_wrote(GateLayout::packed);
  return xivo_hip_get_gate(c, B, F, mask_out, dist_out);
}

}  // extern "C"
