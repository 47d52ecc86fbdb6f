// fia_score_candidates: influence of hypothetical ratings ("phantom points",
// matrix_factorization.py:228-235 and the NCF.py branch alike) on a query's prediction.
//
// A candidate c = (a, b, y) of query q = (u, i) has no position in the CSR/CSC index, so
// none of the per-list-position caches of the run kernels apply: everything is computed
// from the parameter tables (and, NCF, the dense per-entity layer-1 rows l1, which every
// prepare -- fia_prepare and fia_prepare_for, small and large k -- writes for ALL entities,
// so the result cannot depend on the cover):
//
//   infl_c = c_q + 2 (r-hat(a, b) - y) (x_q . g_c) / n_q,   c_q = x_q . (wd M theta_t) / n_q
//
// with g_c's user-side blocks zero unless a == u and its item-side blocks zero unless b == i.
//
// Three kernels, all reading x from global memory in the reference theta order:
//   k_cand_rec    per query, once: the tiles that start inside its list (below), 1 / n_q and c_q; NCF also y_side = W1_side^T x_mlp (the
//                 k_ncf_rec_y identity x_mlp . (W1_side d1) = y_side . d1) and W3g * x_gmf
//   k_cand_score  one candidate per thread over tiles of kCandTile consecutive candidates of
//                 the WHOLE batch (a tile may span several queries; a long list spans many
//                 tiles): perfect balance whatever the list lengths.  With top-K each
//                 (tile, query) segment selects its best min(K, length) candidates into
//                 slot tile + q (unique: along the batch either the tile or the query
//                 advances from one segment to the next)
//   k_cand_merge  per query: K-round selection over the slots of its tiles
// Every round takes the best candidate strictly worse than the previous winner under the
// total order (|v| descending, position ascending, NaN last), so the result does not depend
// on where the tiles cut a list.
// The per-query record and the per-pair pieces (coop_dots, stage_z1, cand_core_ncf) live in
// cand.h, shared with fia_total_influence (total.hip).
#include "cand.h"

namespace fia {
namespace {

constexpr int kCandRecGrid = 1 << 20; // most workgroups of the per-query kernels (grid-stride)

struct CandArgs : ModelArgs {
  int64_t Q, total;
  const int32_t* qu;
  const int32_t* qi;
  const double* x;        // [Q * D], reference theta order
  const int64_t* off;     // [Q + 1]
  const int32_t* cu;
  const int32_t* ci;
  const float* cy;
  int64_t tiles;         // ceil(total / kCandTile)
  int32_t* tile_q;        // [tiles]: the query of each tile's first candidate (k_cand_rec)
};

template <class M>
__global__ __launch_bounds__(64) void k_cand_rec(CandArgs A, double* __restrict__ rec) {
  constexpr int D = M::D, R = cand_rec_size<M>();
  const int lane = threadIdx.x;
  for (int64_t q = blockIdx.x; q < A.Q; q += gridDim.x) {
    const int32_t u = A.qu[q], i = A.qi[q];
    double* __restrict__ Rq = rec + q * R;
    {
      // the tiles whose first candidate is one of this query's: each tile is named by exactly
      // one (non-empty) query, so the scoring workgroups start without a search
      const int64_t cb = A.off[q] > 0 ? A.off[q] : 0, ce = A.off[q + 1];
      for (int64_t t = (cb + kCandTile - 1) / kCandTile + lane; t < A.tiles && t * kCandTile < ce; t += 64)
        A.tile_q[t] = (int32_t)q;
    }
    if (!(u >= 0 && u < A.U && i >= 0 && i < A.I)) {   // never dereferenced: NaN scores
      for (int a = lane; a < R; a += 64) Rq[a] = NAN;
      continue;
    }
    query_record<M>(A, u, i, A.x + q * D, Rq, lane);
  }
}

// MF: one dot for r-hat, one per matching side with x (d r-hat / d p_u = q_b, d r-hat / d q_i = p_a).
// Called by the whole wave.
template <int K>
__device__ __forceinline__ double cand_value_mf(const CandArgs& A, const double* __restrict__ rec, bool valid,
                                                int64_t q, int32_t a, int32_t b, float y) {
  constexpr int D = 2 * K + 2;
  bool on_u = false, on_i = false;
  if (valid) {
    on_u = a == A.qu[q];
    on_i = b == A.qi[q];
  }
  double r, su, si;
  coop_dots<K, false, D, 0, K>(valid, a, b, (int)q, on_u, on_i, A.t[0], A.t[1], A.x, nullptr, r, su, si);
  if (!valid) return NAN;
  constexpr int R = CandHead::head;   // MF: the header is the record
  const double inv_n = rec[q * R + CandHead::inv_n], cq = rec[q * R + CandHead::c_q];
  const double* __restrict__ xq = A.x + q * D;
  r += (double)A.t[2][a] + (double)A.t[3][b] + (double)A.t[4][0];
  if (on_u) su += xq[2 * K];
  if (on_i) si += xq[2 * K + 1];
  const double e = r - (double)y;
  return cq + 2.0 * e * (su + si) * inv_n;
}

// NCF: the MLP's share of r-hat and of x . g_c from cand_core_ncf with the query's y_side
// vectors; GMF (coop_dots, by the caller): rg = W3g . (Pg_a * Qg_b),
// sg = x_Pg . (W3g * Qg_b) + x_Qg . (W3g * Pg_a)
template <int K>
__device__ __forceinline__ double cand_value_ncf(const CandArgs& A, const double* __restrict__ rec,
                                                 const NCFWeights<(K <= 64 ? K : 2)>& w, int64_t q, int32_t a,
                                                 int32_t b, float y, bool on_u, bool on_i, double rg, double sg,
                                                 const double* __restrict__ z1col) {
  using L = CandRecNCF<K>;
  const double* __restrict__ Rq = rec + q * L::size;
  const double inv_n = Rq[L::inv_n], cq = Rq[L::c_q];
  double r, s;
  cand_core_ncf<K>(A, w, a, b, on_u, on_i, Rq + L::y_user, Rq + L::y_item, z1col, r, s);
  s += sg;
  r += rg + (double)A.t[9][0];
  const double e = r - (double)y;
  return cq + 2.0 * e * s * inv_n;
}

template <class M>
__global__ __launch_bounds__(kCandTile) void k_cand_score(CandArgs A, const double* __restrict__ rec,
                                                          double* __restrict__ influence, int K,
                                                          int32_t* __restrict__ cand_pos,
                                                          double* __restrict__ cand_val) {
  constexpr int KK = M::K;
  __shared__ NCFWeights<(M::ncf && KK <= 64 ? KK : 2)> w;
  __shared__ int32_t s_qid[kCandTile];
  __shared__ double s_a[kCandTile / 64], s_v[kCandTile / 64];
  __shared__ int s_p[kCandTile / 64];
  if constexpr (M::ncf && KK <= 64) {
    load_ncf_weights<KK>(w, A.t[6], A.t[7], A.t[8]);
    __syncthreads();
  }
  const int tid = threadIdx.x;
  const int64_t g0 = (int64_t)blockIdx.x * kCandTile;     // < total: the grid is ceil(total / tile)
  const int64_t tile_end = g0 + kCandTile < A.total ? g0 + kCandTile : A.total;
  const int64_t g = g0 + tid;
  const bool active = g < tile_end;
  // the tile's first query and the next tile's (k_cand_rec wrote them; clamped, so offsets that
  // break the contract still index inside the arrays), then the thread's own between them
  int64_t qlo = A.tile_q[blockIdx.x];
  qlo = qlo < 0 ? 0 : (qlo > A.Q - 1 ? A.Q - 1 : qlo);
  int64_t qhi = (int64_t)blockIdx.x + 1 < A.tiles ? A.tile_q[blockIdx.x + 1] : A.Q - 1;
  qhi = qhi < qlo ? qlo : (qhi > A.Q - 1 ? A.Q - 1 : qhi);
  double v = NAN;
  int pos = -1;
  int64_t q = qlo;
  int32_t a = 0, b = 0;
  float y = 0.f;
  bool valid = false;
  if (active) {
    if (qhi != qlo) q = last_at_most(A.off, qlo, qhi, g);
    pos = (int)(g - A.off[q]);
    a = A.cu[g];
    b = A.ci[g];
    y = A.cy[g];
    // an id outside [0, U) x [0, I) is never used as an index: the candidate scores NaN
    valid = a >= 0 && a < A.U && b >= 0 && b < A.I;
  }
  // (whole waves from here: the row gathers are cooperative)
  if constexpr (M::ncf) {
    // (written out: the layout's names as template arguments reorder this kernel's instructions)
    constexpr int R = 2 + 4 * KK;
    static_assert(R == CandRecNCF<KK>::size && 2 + 2 * KK == CandRecNCF<KK>::w3g_x_pg &&
                      2 + 3 * KK == CandRecNCF<KK>::w3g_x_qg, "the record of cand.h");
    bool on_u = false, on_i = false;
    if (valid) {
      on_u = a == A.qu[q];
      on_i = b == A.qi[q];
    }
    __shared__ double z1s[cand_stage_z1<KK>() ? KK * kCandZ1Stride : 1];
    if constexpr (cand_stage_z1<KK>()) {
      stage_z1<KK>(A, valid, a, b, z1s);
      __syncthreads();
    }
    double rg, sgu, sgi;
    coop_dots<KK, true, R, 2 + 2 * KK, 2 + 3 * KK>(valid, a, b, (int)q, on_u, on_i, A.t[2], A.t[3], rec,
                                                    A.t[8] + KK / 2, rg, sgu, sgi);
    if (valid) v = cand_value_ncf<KK>(A, rec, w, q, a, b, y, on_u, on_i, rg, sgu + sgi, z1s + tid);
  } else {
    v = cand_value_mf<KK>(A, rec, valid, q, a, b, y);
  }
  if (active && influence) influence[g] = v;
  if (K <= 0) return;
  s_qid[tid] = active ? (int32_t)q : -1;
  __syncthreads();
  const int nact = (int)(tile_end - g0);
  int cur = 0;
  while (cur < nact) {                       // every (tile, query) segment, in batch order
    const int32_t sq = s_qid[cur];
    const int64_t qe = A.off[sq + 1];
    int end = (int)((qe < tile_end ? qe : tile_end) - g0);
    if (end <= cur) end = cur + 1;           // (offsets that are not monotone: still terminates)
    const int rounds = K < end - cur ? K : end - cur;
    const bool mine = active && tid >= cur && tid < end;
    const double ca[1] = {mine ? topk_key(v) : -2.0};
    const int cp[1] = {mine ? pos : -1};
    const double cv[1] = {v};
    const int64_t slot = ((int64_t)blockIdx.x + sq) * K;
    block_topk<1, kCandTile>(ca, cp, cv, rounds, cand_pos + slot, cand_val + slot, s_a, s_p, s_v);
    if (tid >= rounds && tid < K) {          // K <= FIA_MAX_TOPK < kCandTile
      cand_pos[slot + tid] = -1;
      cand_val[slot + tid] = NAN;
    }
    cur = end;
  }
}

// Per query: the K best of the slots its tiles wrote (slots t + q of consecutive tiles t are
// consecutive).  One workgroup per query walks all of them K times; a list of L candidates has
// ceil(L / kCandTile) + 1 slots at most, each already reduced to K entries.
__global__ __launch_bounds__(256) void k_cand_merge(int64_t Q, int64_t total, const int64_t* __restrict__ off, int K,
                                                    const int32_t* __restrict__ cand_pos,
                                                    const double* __restrict__ cand_val,
                                                    int64_t* __restrict__ topk_pos, double* __restrict__ topk_val) {
  for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
    // (clamped to the scored range: offsets that break cand_offsets[Q] == total_cand still
    // read inside the reserved slots)
    const int64_t e = off[q + 1] < total ? off[q + 1] : total;
    const int64_t b = off[q] < e ? (off[q] > 0 ? off[q] : 0) : e;
    const int64_t t0 = b / kCandTile;
    const int64_t nt = e > b ? (e - 1) / kCandTile - t0 + 1 : 0;
    block_topk_slots(nt * K, cand_pos + (t0 + q) * K, cand_val + (t0 + q) * K, K, [&](int t, bool ok, int bp, double bv) {
      topk_pos[q * K + t] = ok ? (int64_t)bp : -1;
      topk_val[q * K + t] = ok ? bv : NAN;
    });
  }
}

template <class M>
hipError_t score_impl(fia_ctx* c, const CandArgs& A0, double* influence, int K, int64_t* topk_pos, double* topk_val,
                      hipStream_t s) {
  constexpr int R = cand_rec_size<M>();
  const int64_t Q = A0.Q;
  const int64_t tiles = (A0.total + kCandTile - 1) / kCandTile;
  FIA_HIP_TRY(c->rec.reserve(sizeof(double) * (size_t)(Q * R), s));
  if (K > 0) {
    FIA_HIP_TRY(c->cand_pos.reserve(sizeof(int32_t) * (size_t)((tiles + Q) * K), s));
    FIA_HIP_TRY(c->cand_val.reserve(sizeof(double) * (size_t)((tiles + Q) * K), s));
  }
  // (zeroed: a tile no query names -- offsets that break the contract -- reads query 0)
  FIA_HIP_TRY(c->coff.reserve(sizeof(int32_t) * (size_t)(tiles + 1), s));
  FIA_HIP_TRY(hipMemsetAsync(c->coff.ptr, 0, sizeof(int32_t) * (size_t)(tiles + 1), s));
  CandArgs A = A0;
  A.tiles = tiles;
  A.tile_q = c->coff.as<int32_t>();
  double* rec = c->rec.as<double>();
  const unsigned qgrid = (unsigned)(Q < kCandRecGrid ? Q : kCandRecGrid);
  phase_begin(c, 2, s);
  hipLaunchKernelGGL(k_cand_rec<M>, dim3(qgrid), dim3(64), 0, s, A, rec);
  FIA_HIP_TRY(hipGetLastError());
  if (tiles > 0) {
    hipLaunchKernelGGL(k_cand_score<M>, dim3((unsigned)tiles), dim3(kCandTile), 0, s, A, rec, influence, K,
                       c->cand_pos.as<int32_t>(), c->cand_val.as<double>());
    FIA_HIP_TRY(hipGetLastError());
  }
  phase_end(c, 2, s);
  if (K > 0) {
    phase_begin(c, 3, s);
    hipLaunchKernelGGL(k_cand_merge, dim3(qgrid), dim3(256), 0, s, Q, A.total, A.off, K, c->cand_pos.as<int32_t>(),
                       c->cand_val.as<double>(), topk_pos, topk_val);
    FIA_HIP_TRY(hipGetLastError());
    phase_end(c, 3, s);
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_cand_merge(fia_ctx* c, int64_t Q, int64_t total, const int64_t* cand_offsets, int K,
                             int64_t* topk_pos, double* topk_val, hipStream_t s) {
  hipLaunchKernelGGL(k_cand_merge, dim3((unsigned)(Q < kCandRecGrid ? Q : kCandRecGrid)), dim3(256), 0, s, Q, total,
                     cand_offsets, K, c->cand_pos.as<int32_t>(), c->cand_val.as<double>(), topk_pos, topk_val);
  return hipGetLastError();
}

hipError_t score_candidates(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const double* x,
                            const int64_t* cand_offsets, int64_t total_cand, const int32_t* cand_user,
                            const int32_t* cand_item, const float* cand_rating, double* influence, int K,
                            int64_t* topk_pos, double* topk_val, hipStream_t s) {
  CandArgs A{};
  fill_model_args(c, A);
  A.Q = Q;
  A.total = total_cand;
  A.qu = qu;
  A.qi = qi;
  A.x = x;
  A.off = cand_offsets;
  A.cu = cand_user;
  A.ci = cand_item;
  A.cy = cand_rating;
  hipError_t e = hipErrorInvalidValue;      // (model_supported is checked by the caller)
  dispatch_any(c->p.model, c->p.k,
               [&](auto m) { e = score_impl<decltype(m)>(c, A, influence, K, topk_pos, topk_val, s); });
  return e;
}

}  // namespace fia
