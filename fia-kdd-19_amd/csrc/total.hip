// fia_total_influence: for every TRAIN row the sum of its influence on a batch of predictions,
//
//   total[j] = sum_q m_q(j) I_q(j),   I_q(j) = x_q . (2 e_j g_j + wd M theta_t(q)) / n_q,
//   m_q(j)   = [a == u_q] + [b == i_q]            for train row j = (a, b, y)
//
// i.e. the scatter-add of fia_query_batch_x's influence by rel_idx, without walking the
// related lists (the reference has no counterpart: get_influence_on_test_loss asserts
// len(test_indices) == 1, matrix_factorization.py:179).  I_q(j) is linear in x_q, and what
// multiplies x_q's user-side blocks -- d r-hat(a, b) / d (user blocks) -- depends on the train
// row only, so the queries of one user add up BEFORE any train row is touched:
//
//   total[j] = C_a + C_b + 2 e_j (A_a . gU_j + B_b . gI_j) + 2 e_j sum_{q: (u_q, i_q) == (a, b)} d_q
//   A_u = sum_{q: u_q == u} x_q[user blocks] / n_q,   C_u = sum_{q: u_q == u} c_q   (items alike)
//   d_q = (x_q[U] . gU + x_q[I] . gI) / n_q at the query's own pair
//
// The last term: a query whose pair is train row j's pair holds j twice, both times with the
// full gradient, while the two aggregates give each side once.  Cost O(Q D) + O(N D) instead of
// O(total_rel D).
//
// Kernels (x read from global memory in the reference theta order):
//   k_total_rec    per query: the record of cand.h (1 / n_q, c_q, NCF y_side and W3g * x_gmf), the
//                  two sort keys (user, U + item; U + I for a query that contributes nothing:
//                  ids out of range or n_q = 0) and whether its pair is a train row
//   (rocprim)      one stable radix sort of the 2Q (key, query) pairs: every entity's queries
//                  contiguous, in ascending query position
//   k_total_rows<false>   d_q of the queries whose pair is a train row
//   k_total_agg    one wave per group: the aggregate, summed serially in ascending query position
//                  (same bits on every call), the group's size, and entity -> group
//   k_total_rows<true>    one thread per position of the user-major lists (every train row once,
//                  a single writer per row), tiles of kTotalTile positions: e_j and the dots as
//                  fia_score_candidates computes them (coop_dots / cand_core_ncf), the per-query
//                  vectors replaced by the two entities' aggregates; with top-K the tile's K best
//   k_topk_merge   (kern.h) K-round selection over groups of kTotalFan slots, level by level
// No floating-point atomics anywhere.
#include <rocprim/device/device_radix_sort.hpp>

#include "cand.h"

namespace fia {
namespace {

constexpr int kTotalTile = kCandTile;   // list positions per train-row workgroup, one per thread
constexpr int kTotalFan = 16;           // slots merged by one workgroup of a top-K merge level
                                        // (ml-1m, K = 64: fan 64 0.67 ms for the merge; see profiles/total_influence.md)
constexpr int kTotalGrid = 1 << 20;     // most workgroups of the grid-stride kernels

struct TotalArgs : ModelArgs {
  int64_t Q, N;
  const int32_t* qu;
  const int32_t* qi;
  const double* x;          // [Q * D], reference theta order
  const int32_t* row;      // user-major lists: train row, item, rating by list position
  const int32_t* other;
  const float* rating;
  PairTable pairs;
  double* rec;              // [Q * cand_rec_size]
  uint32_t* keys;           // [2Q] sorted group keys
  int32_t* vals;            // [2Q] the queries in group order
  double* agg;              // [2Q * AS] aggregate of the group starting at sorted position p
  int32_t* gcnt;            // [2Q] its size
  int32_t* gcpl;            // [2Q] != 0: it holds a query whose pair is a train row
  int32_t* slot;            // [U + I] entity -> sorted position of its group, -1 = no query
  int32_t* cpl;             // [Q] != 0: the query's pair is a train row
  double* pd;               // [Q] d_q of those queries
};

template <class M>
constexpr int agg_size() {
  // MF: sum x_side / n [K], sum x_bias / n, sum c_q;  NCF: sum y_side / n [K], sum W3g * x_gmf / n [K], sum c_q
  return M::ncf ? 2 * M::K + 1 : M::K + 2;
}

template <class M>
__global__ __launch_bounds__(64) void k_total_rec(TotalArgs A, uint32_t* __restrict__ keys_in,
                                                  int32_t* __restrict__ vals_in) {
  constexpr int D = M::D, R = cand_rec_size<M>();
  const int lane = threadIdx.x;
  const uint32_t none = (uint32_t)(A.U + A.I);
  for (int64_t q = blockIdx.x; q < A.Q; q += gridDim.x) {
    const int32_t u = A.qu[q], i = A.qi[q];
    bool ok = u >= 0 && u < A.U && i >= 0 && i < A.I;     // else never used as an index
    bool train_pair = false;
    if (ok) {
      const int64_t n = (A.ptr[0][u + 1] - A.ptr[0][u]) + (A.ptr[1][i + 1] - A.ptr[1][i]);
      ok = n > 0;                                         // n_q = 0: its NaN x reaches no row
    }
    if (ok) {
      query_record<M>(A, u, i, A.x + q * D, A.rec + q * R, lane);
      if (lane == 0) {
        double cdup, rsum;
        A.pairs.lookup((unsigned long long)u * (unsigned long long)A.I + (unsigned long long)i, cdup, rsum);
        train_pair = cdup > 0.0;
      }
    }
    if (lane == 0) {
      keys_in[q] = ok ? (uint32_t)u : none;
      keys_in[A.Q + q] = ok ? (uint32_t)(A.U + i) : none;
      vals_in[q] = vals_in[A.Q + q] = (int32_t)q;
      A.cpl[q] = train_pair ? 1 : 0;
    }
  }
}

// One wave per sorted position; the wave of a group's first position sums the group.
template <class M>
__global__ __launch_bounds__(64) void k_total_agg(TotalArgs A) {
  constexpr int K = M::K, D = M::D, R = cand_rec_size<M>(), AS = agg_size<M>(), NA = (AS + 63) / 64;
  const int lane = threadIdx.x;
  const uint32_t none = (uint32_t)(A.U + A.I);
  const int64_t n2 = 2 * A.Q;
  for (int64_t p = blockIdx.x; p < n2; p += gridDim.x) {
    const uint32_t key = A.keys[p];
    if (key >= none || (p > 0 && A.keys[p - 1] == key)) continue;
    const int sd = key >= (uint32_t)A.U ? 1 : 0;
    double acc[NA];
#pragma unroll
    for (int t = 0; t < NA; ++t) acc[t] = 0.0;
    int cnt = 0, any_pair = 0;
    for (int64_t pp = p; pp < n2 && A.keys[pp] == key; ++pp) {     // ascending query position
      const int64_t q = A.vals[pp];
      const double* __restrict__ Rq = A.rec + q * R;
      const double inv_n = Rq[CandHead::inv_n];
#pragma unroll
      for (int t = 0; t < NA; ++t) {
        const int a = t * 64 + lane;
        if (a >= AS) continue;
        double v;
        if (a == AS - 1) {
          v = Rq[CandHead::c_q];
        } else if constexpr (!M::ncf) {
          v = inv_n * A.x[q * D + (a < K ? sd * K + a : 2 * K + sd)];
        } else {
          // y_user | y_item, w3g_x_pg | w3g_x_qg: the side's half of each pair
          v = inv_n * Rq[CandHead::head + (a < K ? sd * K + a : 2 * K + sd * K + (a - K))];
        }
        acc[t] += v;
      }
      any_pair |= A.cpl[q];
      ++cnt;
    }
    double* __restrict__ out = A.agg + p * AS;
#pragma unroll
    for (int t = 0; t < NA; ++t) {
      const int a = t * 64 + lane;
      if (a < AS) out[a] = acc[t];
    }
    if (lane == 0) {
      A.gcnt[p] = cnt;
      A.gcpl[p] = any_pair;
      A.slot[key] = (int32_t)p;
    }
  }
}

// AGG: one thread per position of the user-major lists, scored against the two entities'
// aggregates -> total / count / the tile's top-K.  !AGG: one thread per query, scored against
// the query's own vectors at its own pair -> d_q (only where the pair is a train row).
template <class M, bool AGG>
__global__ __launch_bounds__(kTotalTile) void k_total_rows(TotalArgs A, double* __restrict__ total,
                                                           int32_t* __restrict__ count, int K,
                                                           int32_t* __restrict__ cand_pos,
                                                           double* __restrict__ cand_val) {
  constexpr int KK = M::K, D = M::D, R = cand_rec_size<M>(), AS = agg_size<M>();
  __shared__ NCFWeights<(M::ncf && KK <= 64 ? KK : 2)> w;
  __shared__ double s_a[kTotalTile / 64], s_v[kTotalTile / 64];
  __shared__ int s_p[kTotalTile / 64];
  __shared__ int64_t s_own[2];
  if constexpr (M::ncf && KK <= 64) {
    load_ncf_weights<KK>(w, A.t[6], A.t[7], A.t[8]);
    __syncthreads();
  }
  const int tid = threadIdx.x;
  const int64_t n_items = AGG ? A.N : A.Q;
  const int64_t g0 = (int64_t)blockIdx.x * kTotalTile;     // < n_items: the grid is ceil(n_items / tile)
  const int64_t g = g0 + tid;
  const bool active = g < n_items;
  int32_t a = 0, b = 0, row = -1;
  int sa = 0, sb = 0;          // AGG: the groups of a and b; else the query, twice
  float y = 0.f;
  bool valid = false, on_u = false, on_i = false;
  if constexpr (AGG) {
    // the owners of the tile's first and last positions, then the thread's own between them
    if (tid == 0) s_own[0] = last_at_most(A.ptr[0], (int64_t)0, A.U - 1, g0);
    if (tid == 64) {
      const int64_t last = g0 + kTotalTile < A.N ? g0 + kTotalTile - 1 : A.N - 1;
      s_own[1] = last_at_most(A.ptr[0], (int64_t)0, A.U - 1, last);
    }
    __syncthreads();
    if (active) {
      a = (int32_t)last_at_most(A.ptr[0], s_own[0], s_own[1], g);
      b = A.other[g];
      row = A.row[g];
      sa = A.slot[a];
      sb = A.slot[A.U + b];
      on_u = sa >= 0;
      on_i = sb >= 0;
      valid = on_u || on_i;      // else: no query touches the row, nothing is computed
      if (valid) y = A.rating[g];
      if (!on_u) sa = 0;
      if (!on_i) sb = 0;
    }
  } else {
    if (active && A.cpl[g]) {    // (ids in range: k_total_rec looked the pair up)
      a = A.qu[g];
      b = A.qi[g];
      sa = sb = (int)g;
      valid = on_u = on_i = true;
    }
  }
  // (whole waves from here: the row gathers are cooperative)
  double r = 0.0, s = 0.0;
  if constexpr (M::ncf) {
    __shared__ double z1s[cand_stage_z1<KK>() ? KK * kCandZ1Stride : 1];
    if constexpr (cand_stage_z1<KK>()) {
      stage_z1<KK>(A, valid, a, b, z1s);
      __syncthreads();
    }
    double rg, sgu, sgi;
    const double *yu, *yi;
    if constexpr (AGG) {
      coop_dots<KK, true, AS, KK, KK, true>(valid, a, b, sa, on_u, on_i, A.t[2], A.t[3], A.agg, A.t[8] + KK / 2, rg,
                                            sgu, sgi, sb);
      yu = A.agg + (int64_t)sa * AS;
      yi = A.agg + (int64_t)sb * AS;
    } else {
      using L = CandRecNCF<KK>;
      coop_dots<KK, true, R, L::w3g_x_pg, L::w3g_x_qg>(valid, a, b, sa, on_u, on_i, A.t[2], A.t[3], A.rec,
                                                        A.t[8] + KK / 2, rg, sgu, sgi);
      yu = A.rec + (int64_t)sa * R + L::y_user;
      yi = A.rec + (int64_t)sa * R + L::y_item;
    }
    if (valid) {
      cand_core_ncf<KK>(A, w, a, b, on_u, on_i, yu, yi, z1s + tid, r, s);
      s += sgu + sgi;
      r += rg + (double)A.t[9][0];
    }
  } else {
    double su, si;
    if constexpr (AGG) {
      coop_dots<KK, false, AS, 0, 0, true>(valid, a, b, sa, on_u, on_i, A.t[0], A.t[1], A.agg, nullptr, r, su, si, sb);
      if (on_u) su += A.agg[(int64_t)sa * AS + KK];
      if (on_i) si += A.agg[(int64_t)sb * AS + KK];
    } else {
      coop_dots<KK, false, D, 0, KK>(valid, a, b, sa, on_u, on_i, A.t[0], A.t[1], A.x, nullptr, r, su, si);
      if (valid) {
        su += A.x[(int64_t)sa * D + 2 * KK];
        si += A.x[(int64_t)sa * D + 2 * KK + 1];
      }
    }
    if (valid) {
      s = su + si;
      r += (double)A.t[2][a] + (double)A.t[3][b] + (double)A.t[4][0];
    }
  }
  if constexpr (!AGG) {
    if (valid) A.pd[g] = s * A.rec[g * R + CandHead::inv_n];
    return;
  } else {
    double v = 0.0;
    int cnt = 0;
    if (valid) {
      const double e = r - (double)y;
      if (on_u && A.gcpl[sa]) {
        // the queries at this row's own pair hold it twice with the full gradient (ascending q)
        const int nu = A.gcnt[sa];
        double extra = 0.0;
        for (int t = 0; t < nu; ++t) {
          const int32_t q = A.vals[(int64_t)sa + t];
          if (A.cpl[q] && A.qi[q] == b) extra += A.pd[q];
        }
        s += extra;
      }
      v = 2.0 * e * s;
      if (on_u) {
        v += A.agg[(int64_t)sa * AS + AS - 1];
        cnt += A.gcnt[sa];
      }
      if (on_i) {
        v += A.agg[(int64_t)sb * AS + AS - 1];
        cnt += A.gcnt[sb];
      }
    }
    if (active) {
      if (total) total[row] = v;
      if (count) count[row] = cnt;
    }
    if (K <= 0) return;
    const double ca[1] = {valid ? topk_key(v) : -2.0};
    const int cp[1] = {valid ? row : -1};
    const double cv[1] = {v};
    const int64_t out = (int64_t)blockIdx.x * K;
    block_topk<1, kTotalTile>(ca, cp, cv, K, cand_pos + out, cand_val + out, s_a, s_p, s_v);
  }
}

inline unsigned key_bits(int64_t n) {       // bits holding every key in [0, n]
  unsigned b = 1;
  while (b < 32 && ((int64_t)1 << b) <= n) ++b;
  return b;
}

template <class M>
hipError_t total_impl(fia_ctx* c, TotalArgs A, double* total, int32_t* count, int K, int64_t* topk_idx,
                      double* topk_val, hipStream_t s) {
  constexpr int R = cand_rec_size<M>(), AS = agg_size<M>();
  const int64_t Q = A.Q, N = A.N, nE = A.U + A.I, n2 = 2 * Q;
  const int64_t tiles = (N + kTotalTile - 1) / kTotalTile;
  phase_begin(c, 2, s);
  if (Q == 0 || N == 0) {
    // no query (or no train row): every row is untouched
    if (total && N > 0) FIA_HIP_TRY(hipMemsetAsync(total, 0, sizeof(double) * (size_t)N, s));
    if (count && N > 0) FIA_HIP_TRY(hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)N, s));
    if (K > 0) {
      FIA_HIP_TRY(topk_merge_levels<kTotalFan>(0, K, nullptr, nullptr, topk_idx, topk_val, s));
    }
    phase_end(c, 2, s);
    return hipSuccess;
  }
  // sort keys and queries, in and out: [4Q] each
  FIA_HIP_TRY(c->rec.reserve(sizeof(double) * (size_t)(Q * R), s));
  FIA_HIP_TRY(c->tkeys.reserve(sizeof(uint32_t) * (size_t)(2 * n2), s));
  FIA_HIP_TRY(c->tvals.reserve(sizeof(int32_t) * (size_t)(2 * n2), s));
  FIA_HIP_TRY(c->tagg.reserve(sizeof(double) * (size_t)(n2 * AS), s));
  FIA_HIP_TRY(c->tslot.reserve(sizeof(int32_t) * (size_t)(nE + 1), s));
  // per-group size and flag [2Q] each, per-query flag [Q], then d_q [Q] (8-B aligned: 5Q + pad words)
  const int64_t words = (5 * Q + 1) & ~(int64_t)1;
  FIA_HIP_TRY(c->tword.reserve(sizeof(int32_t) * (size_t)words + sizeof(double) * (size_t)Q, s));
  uint32_t* keys_in = c->tkeys.as<uint32_t>() + n2;
  int32_t* vals_in = c->tvals.as<int32_t>() + n2;
  A.rec = c->rec.as<double>();
  A.keys = c->tkeys.as<uint32_t>();
  A.vals = c->tvals.as<int32_t>();
  A.agg = c->tagg.as<double>();
  A.slot = c->tslot.as<int32_t>();
  A.gcnt = c->tword.as<int32_t>();
  A.gcpl = A.gcnt + n2;
  A.cpl = A.gcpl + n2;
  A.pd = reinterpret_cast<double*>(c->tword.as<int32_t>() + words);
  const unsigned bits = key_bits(nE);
  size_t tb = 0;
  FIA_HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, keys_in, A.keys, vals_in, A.vals, (size_t)n2, 0u, bits, s));
  FIA_HIP_TRY(c->tsort.reserve(tb + 16, s));
  tb = c->tsort.bytes;
  if (K > 0) {
    // every level of the merge behind the tiles' slots: tiles + tiles / 64 + tiles / 64^2 + ...
    const size_t slots = topk_merge_slots<kTotalFan>(tiles);
    FIA_HIP_TRY(c->cand_pos.reserve(sizeof(int32_t) * slots * (size_t)K, s));
    FIA_HIP_TRY(c->cand_val.reserve(sizeof(double) * slots * (size_t)K, s));
  }
  FIA_HIP_TRY(hipMemsetAsync(A.slot, 0xff, sizeof(int32_t) * (size_t)(nE + 1), s));
  const unsigned qgrid = (unsigned)(Q < kTotalGrid ? Q : kTotalGrid);
  hipLaunchKernelGGL(k_total_rec<M>, dim3(qgrid), dim3(64), 0, s, A, keys_in, vals_in);
  FIA_HIP_TRY(hipGetLastError());
  FIA_HIP_TRY(rocprim::radix_sort_pairs(c->tsort.ptr, tb, keys_in, A.keys, vals_in, A.vals, (size_t)n2, 0u, bits, s));
  hipLaunchKernelGGL((k_total_rows<M, false>), dim3((unsigned)((Q + kTotalTile - 1) / kTotalTile)), dim3(kTotalTile), 0,
                     s, A, nullptr, nullptr, 0, nullptr, nullptr);
  FIA_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_total_agg<M>, dim3((unsigned)(n2 < kTotalGrid ? n2 : kTotalGrid)), dim3(64), 0, s, A);
  FIA_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL((k_total_rows<M, true>), dim3((unsigned)tiles), dim3(kTotalTile), 0, s, A, total, count, K,
                     c->cand_pos.as<int32_t>(), c->cand_val.as<double>());
  FIA_HIP_TRY(hipGetLastError());
  phase_end(c, 2, s);
  if (K > 0) {
    phase_begin(c, 3, s);
    FIA_HIP_TRY(topk_merge_levels<kTotalFan>(tiles, K, c->cand_pos.as<int32_t>(), c->cand_val.as<double>(), topk_idx,
                                             topk_val, s));
    phase_end(c, 3, s);
  }
  return hipSuccess;
}

}  // namespace

hipError_t total_influence(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const double* x,
                           double* total, int32_t* count, int K, int64_t* topk_idx, double* topk_val,
                           hipStream_t s) {
  TotalArgs A{};
  fill_model_args(c, A);
  A.Q = Q;
  A.N = c->idx.N;
  A.qu = qu;
  A.qi = qi;
  A.x = x;
  A.row = c->idx.side[0].row.as<int32_t>();
  A.other = c->idx.side[0].other.as<int32_t>();
  A.rating = c->idx.side[0].rating.as<float>();
  A.pairs = pair_table(c->idx);
  hipError_t e = hipErrorInvalidValue;      // (model_supported is checked by the caller)
  dispatch_any(c->p.model, c->p.k,
               [&](auto m) { e = total_impl<decltype(m)>(c, A, total, count, K, topk_idx, topk_val, s); });
  return e;
}

}  // namespace fia
