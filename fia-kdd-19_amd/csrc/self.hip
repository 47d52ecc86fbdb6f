// fia_self_influence: every listed train row's effect on its OWN prediction (include/fia.h), the
// leverage scan.  For train row j = (a, b, y) the query is (a, b): n = |R_a| + |C_b| related
// ratings, theta_t, v = d r-hat(a, b) / d theta_t and the assembled H of fia_query_batch,
// e = r-hat(a, b) - y, and, row j occurring twice in its own related list (m_j = 2),
//
//   b_j = (2/n) (2 e v + wd M theta_t)
//   H_j = (2/n) (2 v v^T + 2 e C + wd M)
//   first_order = (H^-1 v) . b_j,   newton = v . (H - H_j)^-1 b_j,   error = e
//
// which is fia_group_influence for query (a, b) with the single group {j} (group.hip: a member
// with on_u && on_i), fused: one prologue serves the query and the member (they are the same
// pair, g_j = v), no index arrays, no binary search, and H^-1 v stays in LDS.
//
// Kernels:
//   k_self<M, COPY>  persistent one-wave workgroups, a grid-stride loop over positions: the 16-B
//                    row record (group.hip's table), prologue, H from the two Gram caches, LDL^T on
//                    v, the dot with b_j; then H again -- COPY: a second packed triangle kept in
//                    LDS; else assembled again from the caches -- downdated by the member's three
//                    terms, LDL^T on b_j, the dot with v
//   k_self_tile      with top-K: the K best |newton| of every tile of kSelfTile positions
//   k_topk_merge     (kern.h) the tiles' slots, level by level
//   k_self_rows      the winners' train rows
// No floating-point atomics; a position's values depend on its row alone, so the same row gives
// the same bits wherever it sits in `rows` and whatever else is in the batch.
#include "solve.h"

namespace fia {
namespace {

constexpr int kSelfTile = 256;          // positions per top-K tile workgroup, one per thread
constexpr int kSelfFan = 16;            // slots merged by one workgroup of a merge level (as total.hip)

struct SelfArgs {
  int64_t n;                 // positions
  const int32_t* rows;       // [n] train rows; null: position p is row p
  const int4* rowrec;        // [N] train row -> {user, item, rating bits, user-major list position}
  double* first;             // [n], nullable
  double* newton;            // [n], nullable (the caller's array, or scratch for the top-K)
  double* error;             // [n], nullable
};

// Whether k_self keeps a second packed triangle in LDS (else H is assembled twice).  Measured on
// MI355X, the first 200,000 train rows of ml-1m-ex, all three outputs, ms per call copy / twice
// (two runs each, spread under 1 %):
//   MF k=8 2.07 / 2.17    MF k=16 6.22 / 5.40    MF k=32 53.2 / 34.6    MF k=64 880 / 475
//   NCF k=8 9.70 / 5.09   NCF k=16 63.1 / 38.2   NCF k=32 850 / 1017
// The copy loses at every size where it leaves fewer workgroups resident (at NCF k=8, 13 against
// 16 per CU, by more than that alone explains: not looked into); at NCF k=32 one workgroup fits
// per CU either way, and at MF k=8 sixteen do.
#ifndef FIA_SELF_COPY
#define FIA_SELF_COPY -1                // -1: per size (self_copy); 0 / 1: every size (measurement builds)
#endif
template <class M>
constexpr bool self_copy() {
  if (FIA_SELF_COPY >= 0) return FIA_SELF_COPY != 0;
  return (M::ncf && M::K == 32) || (!M::ncf && M::K == 8);
}

// LDS of one k_self workgroup
template <class M, bool COPY>
constexpr int64_t self_lds_bytes() {
  constexpr int64_t K = M::K, D = M::D, T = D * (D + 1) / 2;
  return 8 * (T + (COPY ? T : 1) + 6 * D + 4 * K + 8 + (M::ncf ? 2 * K * K + K + K * (K / 2) + 2 * K : 8));
}

template <class M, bool COPY>
__global__ __launch_bounds__(kSolveThreads) void k_self(QueryArgs A, SelfArgs S) {
  constexpr int K = M::K, D = M::D, T = D * (D + 1) / 2;
  __shared__ double H[T];
  __shared__ double H2[COPY ? T : 1];
  __shared__ double g[D], th[D], dd[D], ww[D];
  __shared__ double x[D], bj[D];
  __shared__ double sh[4 * K + 8];
  __shared__ NCFWeights<M::ncf ? K : 2> w;
  __shared__ double sW1[M::ncf ? 2 * K * K : 1];
  __shared__ double sb1[M::ncf ? K : 1];
  stage_ncf<M>(A, w, sW1, sb1);
  const int lane = threadIdx.x;
  const bool want_first = S.first != nullptr, want_newton = S.newton != nullptr;
  for (int64_t p = blockIdx.x; p < S.n; p += gridDim.x) {
    __syncthreads();
    const int32_t row = S.rows ? S.rows[p] : (int32_t)p;
    if (row < 0 || row >= A.N) {                      // never used as an index
      if (lane == 0) {
        if (S.first) S.first[p] = NAN;
        if (S.newton) S.newton[p] = NAN;
        if (S.error) S.error[p] = NAN;
      }
      continue;
    }
    const int4 rr = S.rowrec[row];
    const int32_t a = rr.x, b = rr.y;
    const int64_t n = related_count(A, a, b);         // >= 2: the row is in both lists
    const double rhat = solve_prologue<M, kSolveThreads>(A, a, b, th, g, sh, w, sW1, sb1);
    const double e = rhat - (double)__int_as_float(rr.z);
    if (lane == 0 && S.error) S.error[p] = e;
    if (!want_first && !want_newton) continue;
    const double mn = 2.0 / (double)n;                // m_j / n
    for (int c = lane; c < D; c += kSolveThreads) bj[c] = member_rhs<M>(c, g, th, e, mn, A.wd);
    // two passes through one solve: 0 = H x = v and the dot with b_j; 1 = H again, downdated,
    // solved for b_j in place, and the dot with v
#pragma nounroll
    for (int pass = want_first ? 0 : 1; pass <= (want_newton ? 1 : 0); ++pass) {
      const bool down = pass == 1;
      double* Hs = H;
      if (COPY && down && want_first) {
        Hs = H2;                                      // the copy pass 0 left
      } else {
        if (down) __syncthreads();                    // the first solve's reads of H
        assemble_hessian<M>(A, a, b, n, rhat, g, H);
      }
      if (!down)
        for (int c = lane; c < D; c += kSolveThreads) x[c] = g[c];
      __syncthreads();
      if (COPY && !down && want_newton) {
        for (int t = lane; t < T; t += kSolveThreads) H2[t] = H[t];
        __syncthreads();
      }
      if (down) {
        // H - H_j: a member on both sides (g_j = v, m_j = 2)
        remove_member<M>(Hs, g, e, mn, 0, D, true, w, A.wd);
        __syncthreads();
      }
      double* rhs = down ? bj : x;
      const double* other = down ? g : bj;
      ldlt_solve<D>(Hs, rhs, dd, ww, 0, D);
      __syncthreads();
      double part = 0.0;
      for (int c = lane; c < D; c += kSolveThreads) part += rhs[c] * other[c];
      part = wave_sum(part);
      if (lane == 0) (down ? S.newton : S.first)[p] = part;
    }
  }
}

// The K best |newton| of positions [tile * kSelfTile, ...) into the tile's slot; a NaN (a row
// out of range among them) is a candidate that ranks last.
__global__ __launch_bounds__(kSelfTile) void k_self_tile(int64_t n, const double* __restrict__ newton, int K,
                                                         int32_t* __restrict__ cand_pos,
                                                         double* __restrict__ cand_val) {
  __shared__ double s_a[kSelfTile / 64], s_v[kSelfTile / 64];
  __shared__ int s_p[kSelfTile / 64];
  const int64_t p = (int64_t)blockIdx.x * kSelfTile + threadIdx.x;
  const bool active = p < n;
  const double v = active ? newton[p] : 0.0;
  const double ca[1] = {active ? topk_key(v) : -2.0};
  const int cp[1] = {active ? (int)p : -1};
  const double cv[1] = {v};
  const int64_t out = (int64_t)blockIdx.x * K;
  block_topk<1, kSelfTile>(ca, cp, cv, K, cand_pos + out, cand_val + out, s_a, s_p, s_v);
}

// topk_idx[t] = the train row at position topk_pos[t] (the entry of `rows` as given), -1 for none
__global__ void k_self_rows(int K, const int32_t* __restrict__ rows, const int64_t* __restrict__ topk_pos,
                            int64_t* __restrict__ topk_idx) {
  const int t = threadIdx.x;
  if (t >= K) return;
  const int64_t p = topk_pos[t];
  topk_idx[t] = p < 0 ? -1 : (rows ? (int64_t)rows[p] : p);
}

template <class M>
hipError_t self_impl(fia_ctx* c, const QueryArgs& A, SelfArgs S, hipStream_t s) {
  constexpr bool COPY = self_copy<M>();
  FIA_HIP_TRY(ensure_rowrec(c, s));
  S.rowrec = c->rowrec.as<int4>();
  // persistent workgroups (NCF weights staged once each), as many as their LDS lets be resident
  const int64_t cap = solve_grid_cap(c, self_lds_bytes<M, COPY>());
  hipLaunchKernelGGL((k_self<M, COPY>), dim3((unsigned)(S.n < cap ? S.n : cap)), dim3(kSolveThreads), 0, s, A, S);
  return hipGetLastError();
}

}  // namespace

hipError_t self_influence(fia_ctx* c, int64_t n, const int32_t* rows, double* first_order, double* newton,
                          double* error, int K, int64_t* topk_pos, int64_t* topk_idx, double* topk_val,
                          hipStream_t s) {
  static_assert(FIA_MAX_TOPK <= 64, "k_self_rows is one wave");
  const int64_t tiles = (n + kSelfTile - 1) / kSelfTile;
  if (n > 0) {
    if (K > 0) {
      const size_t slots = topk_merge_slots<kSelfFan>(tiles);
      FIA_HIP_TRY(c->cand_pos.reserve(sizeof(int32_t) * slots * (size_t)K, s));
      FIA_HIP_TRY(c->cand_val.reserve(sizeof(double) * slots * (size_t)K, s));
      if (!newton) {
        FIA_HIP_TRY(c->gxq.reserve(sizeof(double) * (size_t)n, s));
        newton = c->gxq.as<double>();
      }
    }
    if (big_supported(c->p.model, c->p.k)) {
      // the large-k models: the systems in device memory, in chunks of rows (group_big.hip); the
      // top-K stage below reads the newton values either way
      FIA_HIP_TRY(self_influence_big(c, n, rows, first_order, newton, error, s));
    } else {
      const QueryArgs A = make_args(c, nullptr, nullptr);
      SelfArgs S{};
      S.n = n;
      S.rows = rows;
      S.first = first_order;
      S.newton = newton;
      S.error = error;
      hipError_t e = hipErrorInvalidValue;            // (the sizes are checked by the caller)
      dispatch_small(c->p.model, c->p.k, [&](auto m) { e = self_impl<decltype(m)>(c, A, S, s); });
      FIA_HIP_TRY(e);
    }
  }
  if (K <= 0) return hipSuccess;
  if (n > 0) {
    hipLaunchKernelGGL(k_self_tile, dim3((unsigned)tiles), dim3(kSelfTile), 0, s, n, (const double*)newton, K,
                       c->cand_pos.as<int32_t>(), c->cand_val.as<double>());
    FIA_HIP_TRY(hipGetLastError());
  }
  // the winners' positions, then their rows (n == 0: -1 / -1 / NaN)
  FIA_HIP_TRY(topk_merge_levels<kSelfFan>(n > 0 ? tiles : 0, K, c->cand_pos.as<int32_t>(), c->cand_val.as<double>(),
                                          topk_pos, topk_val, s));
  hipLaunchKernelGGL(k_self_rows, dim3(1), dim3(64), 0, s, K, rows, (const int64_t*)topk_pos, topk_idx);
  return hipGetLastError();
}

}  // namespace fia
