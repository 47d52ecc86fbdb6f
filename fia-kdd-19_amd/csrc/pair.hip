// fia_count_related_pair / fia_pair_batch: which ratings put item i above item j for a user
// (include/fia.h).  The explained number is the gap d = r-hat(u, i) - r-hat(u, j); its FIA system
// is not the difference of two fia_query_batch systems: the restricted parameters are
// theta_t = (theta_u, theta_i, theta_j), the related list is R_u ++ C_i ++ C_j with
// n = |R_u| + |C_i| + |C_j|, and there is ONE Hessian over that list and one solve:
//
//   H_uu = (2/n) (A_u + cd_i v^i_u v^i_u^T + cd_j v^j_u v^j_u^T)
//   H_ii = (2/n) (B_i + cd_i v^i_i v^i_i^T)          H_jj likewise
//   H_iu = (2/n) 2 (cd_i v^i_i v^i_u^T + es_i C)     H_ju likewise          H_ij = 0
//   + wd diag(M) + damping I,     v = (v^i_u - v^j_u, v^i_i, -v^j_j),     x = H^-1 v
//   influence_p = x . (2 e_p g_p + wd M theta_t) / n
//
// with A_u, B_i, B_j the entity Gram caches, (cd, es) the train-pair lookups of assemble_hessian
// (solve.h) and v^i, v^j the prediction gradients of the two pairs.  Block order in LDS: user, item
// i, item j (Ds coordinates each, D3 = 3 Ds).
//
// Kernels:
//   k_pair_scan    n per query and its exclusive prefix, one launch (scan.h's look-back)
//   k_pair_rel     rel_idx from the CSR / CSC lists, a workgroup per query
//   k_pair_solve   persistent one-wave workgroups: the prologue of (u, i) and of (u, j), the packed
//                  3-block triangle, one full-range LDL^T when either pair is a train row and three
//                  block-range ones when neither is; x_out, diff, the scoring record and the tiles
//                  that start inside the query's list
//   k_pair_score   k_cand_score's decomposition: tiles of kCandTile consecutive positions of the
//                  whole batch's flat related array, a position per thread -- its query by a search
//                  of offsets, then its list (user, i, j) and its entry, which is a candidate
//                  (a, b, y) read from the index and scored with the pieces of cand.h; with top-K
//                  every (tile, query) segment selects into slot tile + q
//   k_cand_merge (score_cand.hip), k_pair_topk_idx   the per-query merge, then topk_idx from the position
// No floating-point atomics; a query's values depend on (u, i, j) alone.
#include "pair.h"
#include "scan.h"

namespace fia {
namespace {

constexpr int kPairRecGrid = 1 << 20;   // most workgroups of the per-query kernels (grid-stride)

struct PairArgs : ModelArgs {
  int64_t Q, total;
  const int32_t* qu;
  const int32_t* qi;
  const int32_t* qj;
  const int64_t* off;       // [Q + 1]
  const int32_t* row[2];    // the lists of both sides (train row, other endpoint, rating)
  const int32_t* other[2];
  const float* rating[2];
  int64_t tiles;            // ceil(total / kCandTile)
  int32_t* tile_q;          // [tiles]: the query of each tile's first position (k_pair_solve)
  double* rec;              // [Q * 2 * pair_half]
};

// Position `pos` of the related list of (u, i, j) (ids in range, i != j): its list (0 user, 1 item
// i, 2 item j; -1 past the list's end) and its index into that side's list arrays
__device__ __forceinline__ int pair_locate(const int64_t* __restrict__ uptr, const int64_t* __restrict__ iptr,
                                           int32_t u, int32_t i, int32_t j, int64_t pos, int64_t& entry) {
  const int64_t ub = uptr[u], du = uptr[u + 1] - ub;
  if (pos < du) {
    entry = ub + pos;
    return 0;
  }
  pos -= du;
  const int64_t ib = iptr[i], di = iptr[i + 1] - ib;
  if (pos < di) {
    entry = ib + pos;
    return 1;
  }
  pos -= di;
  const int64_t jb = iptr[j], dj = iptr[j + 1] - jb;
  entry = jb + pos;
  return pos < dj ? 2 : -1;
}

// n = |R_u| + |C_i| + |C_j| per query (0: an id out of range, flag[1] set; or i == j) and its
// exclusive prefix, the total at [Q]: k_group_scan's single pass over one array
__global__ __launch_bounds__(kScanThreads) void k_pair_scan(
    const int32_t* __restrict__ qu, const int32_t* __restrict__ qi, const int32_t* __restrict__ qj, int64_t Q,
    const int64_t* __restrict__ uptr, const int64_t* __restrict__ iptr, int64_t U, int64_t I,
    int64_t* __restrict__ out, unsigned long long* __restrict__ tstate, unsigned int* __restrict__ tctr,
    int32_t* __restrict__ flag) {
  __shared__ int s_tile;
  __shared__ int64_t s_wave[kScanThreads / 64];
  __shared__ int64_t s_prefix;
  const unsigned ntiles = (unsigned)((Q + 1 + kScanTile - 1) / kScanTile);
  if (threadIdx.x == 0) s_tile = (int)atomicAdd(&tctr[0], 1u);
  __syncthreads();
  const int64_t tile = s_tile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q = tile * kScanTile + threadIdx.x;
  int64_t x = 0;
  if (q < Q) {
    const int32_t u = qu[q], i = qi[q], j = qj[q];
    if (!pair_ids_ok(u, i, j, U, I)) atomicOr(flag + 1, 1);
    else if (i != j) x = (uptr[u + 1] - uptr[u]) + (iptr[i + 1] - iptr[i]) + (iptr[j + 1] - iptr[j]);
  }
  int64_t inc = x;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int64_t y = __shfl_up(inc, off);
    if (lane >= off) inc += y;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  int64_t wbase = 0, agg = 0;
#pragma unroll
  for (int w = 0; w < kScanThreads / 64; ++w) {
    if (w < wave) wbase += s_wave[w];
    agg += s_wave[w];
  }
  if (wave == 0) {
    const int64_t excl = scan_lookback(tstate, tile, agg);
    if (lane == 0) s_prefix = excl;
  }
  __syncthreads();
  if (q <= Q) out[q] = s_prefix + wbase + inc - x;
  __syncthreads();
  if (threadIdx.x == 0) {
    // the block's tile-word stores performed before it counts itself done (see query_scan_body)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned done = atomicAdd(&tctr[1], 1u);
    if (done == ntiles - 1) {
      for (unsigned t = 0; t < ntiles; ++t)
        __hip_atomic_store(&tstate[t], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&tctr[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&tctr[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// one workgroup per query: rel[offsets[q] + p] = R_u[p], then C_i, then C_j
__global__ void k_pair_rel(PairArgs A, int32_t* __restrict__ rel) {
  const int64_t q = blockIdx.x;
  const int32_t u = A.qu[q], i = A.qi[q], j = A.qj[q];
  if (!pair_ids_ok(u, i, j, A.U, A.I) || i == j) return;
  int64_t base = A.off[q];
  const int64_t end = A.off[q + 1] < A.total ? A.off[q + 1] : A.total;   // (never past the array)
  if (base < 0) return;
  const int64_t lb[3] = {A.ptr[0][u], A.ptr[1][i], A.ptr[1][j]};
  const int64_t ln[3] = {A.ptr[0][u + 1] - lb[0], A.ptr[1][i + 1] - lb[1], A.ptr[1][j + 1] - lb[2]};
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const int32_t* __restrict__ src = A.row[l ? 1 : 0] + lb[l];
    for (int64_t p = threadIdx.x; p < ln[l] && base + p < end; p += blockDim.x) rel[base + p] = src[p];
    base += ln[l];
  }
}

template <class M>
__global__ __launch_bounds__(kSolveThreads) void k_pair_solve(QueryArgs A, PairArgs P, double* __restrict__ x_out,
                                                              double* __restrict__ diff) {
  constexpr int K = M::K, Ds = M::Ds, D = M::D, D3 = 3 * Ds, GS = Ds * (Ds + 1) / 2, HS = pair_half<M>();
  __shared__ double H[D3 * (D3 + 1) / 2];
  __shared__ double gi[D], gj[D], thi[D], thj[D];     // v^i, v^j and theta of (u, i), (u, j): [user | item]
  __shared__ double v[D3], dd[D3], ww[D3];
  __shared__ double sh[4 * K + 8];
  __shared__ NCFWeights<M::ncf ? K : 2> w;
  __shared__ double sW1[M::ncf ? 2 * K * K : 1];
  __shared__ double sb1[M::ncf ? K : 1];
  stage_ncf<M>(A, w, sW1, sb1);
  const int lane = threadIdx.x;
  for (int64_t q = blockIdx.x; q < P.Q; q += gridDim.x) {
    __syncthreads();
    const int32_t u = P.qu[q], i = P.qi[q], j = P.qj[q];
    double* __restrict__ Rq = P.rec + q * (2 * HS);
    double* __restrict__ xo = x_out ? x_out + q * D3 : nullptr;
    if (P.tile_q) {
      // the tiles whose first position is one of this query's: each tile is named by exactly one
      // (non-empty) query, so the scoring workgroups start without a search
      const int64_t cb = P.off[q] > 0 ? P.off[q] : 0, ce = P.off[q + 1];
      for (int64_t t = (cb + kCandTile - 1) / kCandTile + lane; t < P.tiles && t * kCandTile < ce; t += 64)
        P.tile_q[t] = (int32_t)q;
    }
    const bool in_range = pair_ids_ok(u, i, j, A.U, A.I);
    double rhat_i = 0.0, rhat_j = 0.0;
    int64_t n = 0;
    if (in_range && i != j) {
      n = (A.ptr[0][u + 1] - A.ptr[0][u]) + (A.ptr[1][i + 1] - A.ptr[1][i]) + (A.ptr[1][j + 1] - A.ptr[1][j]);
      rhat_i = solve_prologue<M, kSolveThreads>(A, u, i, thi, gi, sh, w, sW1, sb1);
      rhat_j = solve_prologue<M, kSolveThreads>(A, u, j, thj, gj, sh, w, sW1, sb1);
    }
    // an id out of range (never an index): NaN; i == j: +0.0; else the gap, whatever n is
    if (lane == 0 && diff) diff[q] = in_range ? rhat_i - rhat_j : NAN;
    if (n == 0) {
      if (xo)
        for (int a = lane; a < D3; a += kSolveThreads) xo[a] = NAN;
      for (int a = lane; a < 2 * HS; a += kSolveThreads) Rq[a] = NAN;
      continue;
    }
    // ---- the packed 3-block triangle from the three Gram reads and the two pair lookups ----
    const double s2n = 2.0 / (double)n;
    double cd_i, rs_i, cd_j, rs_j;
    A.pairs.lookup((unsigned long long)u * (unsigned long long)A.I + (unsigned long long)i, cd_i, rs_i);
    A.pairs.lookup((unsigned long long)u * (unsigned long long)A.I + (unsigned long long)j, cd_j, rs_j);
    const double es_i = cd_i * rhat_i - rs_i, es_j = cd_j * rhat_j - rs_j;
    const bool coupled = cd_i > 0.0 || cd_j > 0.0;
    const double* __restrict__ Gu = A.gram[0] + (int64_t)u * ((GS + 1) & ~1);
    const double* __restrict__ Gi = A.gram[1] + (int64_t)i * ((GS + 1) & ~1);
    const double* __restrict__ Gj = A.gram[1] + (int64_t)j * ((GS + 1) & ~1);
    for (int t = lane; t < D3 * (D3 + 1) / 2; t += kSolveThreads) {
      int r = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
      while (tri(r + 1, 0) <= t) ++r;
      while (tri(r, 0) > t) --r;
      const int c = t - tri(r, 0);
      const int br = r / Ds, bc = c / Ds, rr = r - br * Ds, cc = c - bc * Ds;
      double h = 0.0;
      if (br == 0) {
        h = s2n * (Gu[gidx<M>(rr, cc)] + cd_i * gi[rr] * gi[cc] + cd_j * gj[rr] * gj[cc]);
      } else if (br == bc) {
        const double* __restrict__ g = br == 1 ? gi : gj;
        h = s2n * ((br == 1 ? Gi : Gj)[gidx<M>(rr, cc)] + (br == 1 ? cd_i : cd_j) * g[Ds + rr] * g[Ds + cc]);
      } else if (bc == 0) {
        // cross block: item row rr, user col cc: 2 (cd g_item g_user^T + es * d2r/dtheta_item dtheta_u)
        const double* __restrict__ g = br == 1 ? gi : gj;
        const double cd = br == 1 ? cd_i : cd_j, es = br == 1 ? es_i : es_j;
        if (cd > 0.0) {
          h = s2n * 2.0 * cd * g[Ds + rr] * g[cc];
          if constexpr (!M::ncf) {
            if (rr == cc && cc < K) h += s2n * 2.0 * es;                               // I on (p_u, q)
          } else {
            if (rr == cc && cc >= K) h += s2n * 2.0 * es * w.W3[K / 2 + (cc - K)];     // diag(W3g) on (Pg_u, Qg)
          }
        }
      }                                                   // (item i against item j: zero)
      if (r == c) h += (M::decayed(rr) ? A.wd : 0.0) + A.damping;
      H[t] = h;
    }
    // v = d (r-hat(u, i) - r-hat(u, j)) / d theta_t
    for (int a = lane; a < Ds; a += kSolveThreads) {
      v[a] = gi[a] - gj[a];
      v[Ds + a] = gi[Ds + a];
      v[2 * Ds + a] = -gj[Ds + a];
    }
    __syncthreads();
    if (coupled) {
      ldlt_solve<D3>(H, v, dd, ww, 0, D3);
    } else {
      // block diagonal: three side systems, nine times fewer flops (the common case for a test pair)
      ldlt_solve<D3>(H, v, dd, ww, 0, Ds);
      ldlt_solve<D3>(H, v, dd, ww, Ds, 2 * Ds);
      ldlt_solve<D3>(H, v, dd, ww, 2 * Ds, D3);
    }
    __syncthreads();
    if (xo)
      for (int a = lane; a < D3; a += kSolveThreads) xo[pair_ref_index<M>(a)] = v[a];
    // ---- the scoring record ----
    const double inv_n = 1.0 / (double)n;
    double part = 0.0;
    for (int a = lane; a < Ds; a += kSolveThreads)
      if (M::decayed(a)) part += v[a] * thi[a] + v[Ds + a] * thi[Ds + a] + v[2 * Ds + a] * thj[Ds + a];
    part = wave_sum(part);
    if (lane == 0) {
      Rq[CandHead::inv_n] = inv_n;
      Rq[CandHead::c_q] = A.wd * part * inv_n;
    }
    if constexpr (!M::ncf) {
      using L = PairRecMF<K>;
      for (int a = lane; a < K; a += kSolveThreads) {
        Rq[L::x_user + a] = v[a];
        Rq[L::x_item + a] = v[Ds + a];
        Rq[HS + L::x_item + a] = v[2 * Ds + a];
      }
      if (lane == 0) {
        Rq[L::x_bias_user] = v[K];
        Rq[L::x_bias_item] = v[Ds + K];
        Rq[HS + L::x_bias_item] = v[2 * Ds + K];
      }
    } else {
      // y_side = W1_side^T x_mlp (x_mlp . (W1_side d1) = y_side . d1) and W3g * x_gmf, as query_record
      using L = CandRecNCF<K>;
      for (int c = lane; c < K; c += kSolveThreads) {
        double yu = 0.0, yi = 0.0, yj = 0.0;
        for (int a = 0; a < K; ++a) {
          yu = fma(sW1[a * K + c], v[a], yu);
          yi = fma(sW1[(K + a) * K + c], v[Ds + a], yi);
          yj = fma(sW1[(K + a) * K + c], v[2 * Ds + a], yj);
        }
        const double w3g = w.W3[K / 2 + c];
        Rq[L::y_user + c] = yu;
        Rq[L::y_item + c] = yi;
        Rq[HS + L::y_item + c] = yj;
        Rq[L::w3g_x_pg + c] = w3g * v[K + c];
        Rq[L::w3g_x_qg + c] = w3g * v[Ds + K + c];
        Rq[HS + L::w3g_x_qg + c] = w3g * v[2 * Ds + K + c];
      }
    }
  }
}

template <class M>
__global__ __launch_bounds__(kCandTile) void k_pair_score(PairArgs A, double* __restrict__ influence, int K,
                                                          int32_t* __restrict__ cand_pos,
                                                          double* __restrict__ cand_val) {
  constexpr int KK = M::K, HS = pair_half<M>();
  __shared__ NCFWeights<(M::ncf ? KK : 2)> w;
  __shared__ int32_t s_qid[kCandTile];
  __shared__ double s_a[kCandTile / 64], s_v[kCandTile / 64];
  __shared__ int s_p[kCandTile / 64];
  if constexpr (M::ncf) {
    load_ncf_weights<KK>(w, A.t[6], A.t[7], A.t[8]);
    __syncthreads();
  }
  const int tid = threadIdx.x;
  const int64_t g0 = (int64_t)blockIdx.x * kCandTile;     // < total: the grid is ceil(total / tile)
  const int64_t tile_end = g0 + kCandTile < A.total ? g0 + kCandTile : A.total;
  const int64_t g = g0 + tid;
  const bool active = g < tile_end;
  // the tile's first query and the next tile's (k_pair_solve wrote them; clamped, so offsets that
  // break the contract still index inside the arrays), then the thread's own between them
  int64_t qlo = A.tile_q[blockIdx.x];
  qlo = qlo < 0 ? 0 : (qlo > A.Q - 1 ? A.Q - 1 : qlo);
  int64_t qhi = (int64_t)blockIdx.x + 1 < A.tiles ? A.tile_q[blockIdx.x + 1] : A.Q - 1;
  qhi = qhi < qlo ? qlo : (qhi > A.Q - 1 ? A.Q - 1 : qhi);
  double val = NAN;
  int pos = -1;
  int64_t q = qlo;
  int32_t a = 0, b = 0;
  float y = 0.f;
  bool valid = false, on_u = false, on_it = false;
  int sel = 0;                                // the item block of the position: 0 item i, 1 item j
  if (active) {
    if (qhi != qlo) q = last_at_most(A.off, qlo, qhi, g);
    const int64_t p = g - A.off[q];
    pos = (int)p;
    const int32_t u = A.qu[q], i = A.qi[q], j = A.qj[q];
    // an id outside [0, U) x [0, I) is never used as an index; a position no list holds scores NaN
    if (p >= 0 && pair_ids_ok(u, i, j, A.U, A.I) && i != j) {
      int64_t entry;
      const int list = pair_locate(A.ptr[0], A.ptr[1], u, i, j, p, entry);
      if (list >= 0) {
        valid = true;
        const int sd = list ? 1 : 0;
        const int32_t o = A.other[sd][entry];
        y = A.rating[sd][entry];
        a = sd ? o : u;
        b = sd ? (list == 1 ? i : j) : o;
        // an entry of the user's list whose item is i or j also takes that item block's term, an
        // entry of an item list whose user is u the user block's
        on_u = a == u;
        on_it = b == i || b == j;
        sel = b == j ? 1 : 0;
      }
    }
  }
  // (whole waves from here: the row gathers are cooperative).  Half 2 q holds the head, the user
  // entries and item i's, half 2 q + 1 item j's at the same offsets
  const int h0 = (int)(2 * q), hit = h0 + sel;
  const double* __restrict__ R0 = A.rec + (2 * q) * HS;
  if constexpr (M::ncf) {
    using L = CandRecNCF<KK>;
    __shared__ double z1s[KK * kCandZ1Stride];
    stage_z1<KK>(A, valid, a, b, z1s);
    __syncthreads();
    double rg, sgu, sgi;
    coop_dots<KK, true, HS, L::w3g_x_pg, L::w3g_x_qg, true>(valid, a, b, h0, on_u, on_it, A.t[2], A.t[3], A.rec,
                                                            A.t[8] + KK / 2, rg, sgu, sgi, hit);
    if (valid) {
      double r, s;
      cand_core_ncf<KK>(A, w, a, b, on_u, on_it, R0 + L::y_user, R0 + sel * HS + L::y_item, z1s + tid, r, s);
      s += sgu + sgi;
      r += rg + (double)A.t[9][0];
      val = R0[L::c_q] + 2.0 * (r - (double)y) * s * R0[L::inv_n];
    }
  } else {
    using L = PairRecMF<KK>;
    double r, su, si;
    coop_dots<KK, false, HS, L::x_user, L::x_item, true>(valid, a, b, h0, on_u, on_it, A.t[0], A.t[1], A.rec, nullptr,
                                                         r, su, si, hit);
    if (valid) {
      r += (double)A.t[2][a] + (double)A.t[3][b] + (double)A.t[4][0];
      if (on_u) su += R0[L::x_bias_user];
      if (on_it) si += R0[sel * HS + L::x_bias_item];
      val = R0[L::c_q] + 2.0 * (r - (double)y) * (su + si) * R0[L::inv_n];
    }
  }
  if (active && influence) influence[g] = val;
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
    const double ca[1] = {mine ? topk_key(val) : -2.0};
    const int cp[1] = {mine ? pos : -1};
    const double cv[1] = {val};
    const int64_t slot = ((int64_t)blockIdx.x + sq) * K;
    block_topk<1, kCandTile>(ca, cp, cv, rounds, cand_pos + slot, cand_val + slot, s_a, s_p, s_v);
    if (tid >= rounds && tid < K) {          // K <= FIA_MAX_TOPK < kCandTile
      cand_pos[slot + tid] = -1;
      cand_val[slot + tid] = NAN;
    }
    cur = end;
  }
}

// topk_idx from topk_pos: the train row at that position of the query's own related list
__global__ void k_pair_topk_idx(PairArgs A, int K, const int64_t* __restrict__ topk_pos,
                                int64_t* __restrict__ topk_idx) {
  const int64_t n = A.Q * K;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = s / K, p = topk_pos[s];
    int64_t idx = -1;
    const int32_t u = A.qu[q], i = A.qi[q], j = A.qj[q];
    if (p >= 0 && pair_ids_ok(u, i, j, A.U, A.I) && i != j) {
      int64_t entry;
      const int list = pair_locate(A.ptr[0], A.ptr[1], u, i, j, p, entry);
      if (list >= 0) idx = A.row[list ? 1 : 0][entry];
    }
    topk_idx[s] = idx;
  }
}

PairArgs pair_args(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int32_t* qj,
                   const int64_t* off, int64_t total) {
  PairArgs A{};
  fill_model_args(c, A);
  A.Q = Q;
  A.total = total;
  A.qu = qu;
  A.qi = qi;
  A.qj = qj;
  A.off = off;
  for (int s = 0; s < 2; ++s) {
    A.row[s] = c->idx.side[s].row.as<int32_t>();
    A.other[s] = c->idx.side[s].other.as<int32_t>();
    A.rating[s] = c->idx.side[s].rating.as<float>();
  }
  return A;
}

template <class M>
hipError_t pair_impl(fia_ctx* c, const QueryArgs& QA, PairArgs A, double* influence, double* x_out, double* diff,
                     int K, int64_t* topk_pos, int64_t* topk_idx, double* topk_val, hipStream_t s) {
  if constexpr (pair_built<M>()) {
    constexpr int HS = pair_half<M>();
    const int64_t Q = A.Q;
    const bool score = influence || K > 0;
    const int64_t tiles = score ? (A.total + kCandTile - 1) / kCandTile : 0;
    FIA_HIP_TRY(c->rec.reserve(sizeof(double) * (size_t)(Q * 2 * HS), s));
    if (K > 0) {
      FIA_HIP_TRY(c->cand_pos.reserve(sizeof(int32_t) * (size_t)((tiles + Q) * K), s));
      FIA_HIP_TRY(c->cand_val.reserve(sizeof(double) * (size_t)((tiles + Q) * K), s));
    }
    if (score) {
      // (zeroed: a tile no query names -- offsets that break the contract -- reads query 0)
      FIA_HIP_TRY(c->coff.reserve(sizeof(int32_t) * (size_t)(tiles + 1), s));
      FIA_HIP_TRY(hipMemsetAsync(c->coff.ptr, 0, sizeof(int32_t) * (size_t)(tiles + 1), s));
      A.tile_q = c->coff.as<int32_t>();
    }
    A.tiles = tiles;
    A.rec = c->rec.as<double>();
    phase_begin(c, 1, s);
    // persistent workgroups (NCF weights staged once each), as many as their LDS lets be resident
    const int64_t cap = solve_grid_cap(c, pair_lds_bytes<M>());
    hipLaunchKernelGGL(k_pair_solve<M>, dim3((unsigned)(Q < cap ? Q : cap)), dim3(kSolveThreads), 0, s, QA, A, x_out,
                       diff);
    FIA_HIP_TRY(hipGetLastError());
    phase_end(c, 1, s);
    if (tiles > 0) {
      phase_begin(c, 2, s);
      hipLaunchKernelGGL(k_pair_score<M>, dim3((unsigned)tiles), dim3(kCandTile), 0, s, A, influence, K,
                         c->cand_pos.as<int32_t>(), c->cand_val.as<double>());
      FIA_HIP_TRY(hipGetLastError());
      phase_end(c, 2, s);
    }
    if (K > 0) {
      phase_begin(c, 3, s);
      FIA_HIP_TRY(launch_cand_merge(c, Q, A.total, A.off, K, topk_pos, topk_val, s));
      const int64_t nb = (Q * K + 255) / 256;
      hipLaunchKernelGGL(k_pair_topk_idx, dim3((unsigned)(nb < kPairRecGrid ? nb : kPairRecGrid)), dim3(256), 0, s, A,
                         K, topk_pos, topk_idx);
      FIA_HIP_TRY(hipGetLastError());
      phase_end(c, 3, s);
    }
    return hipSuccess;
  } else {
    return hipErrorInvalidValue;            // (pair_supported is checked by the caller)
  }
}

}  // namespace

bool pair_supported(int model, int k) {
  bool built = false;
  dispatch_small(model, k, [&](auto m) { built = pair_built<decltype(m)>(); });
  return built;
}

hipError_t count_related_pair(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int32_t* qj,
                              int64_t* offsets, hipStream_t s) {
  // the tile words + two counters of the query scans (index.hip): zero when (re)allocated, left
  // zero by every launch
  const int64_t ntiles = scan_tiles(Q);
  const size_t need = sizeof(unsigned long long) * (size_t)(2 * ntiles) + 16;
  if (c->qscan.bytes < need || !c->qscan.ptr) {
    FIA_HIP_TRY(c->qscan.reserve(need < 4096 ? 4096 : need, s));
    FIA_HIP_TRY(hipMemsetAsync(c->qscan.ptr, 0, c->qscan.bytes, s));
  }
  FIA_HIP_TRY(c->flag.reserve(64, s));
  unsigned int* ctr = reinterpret_cast<unsigned int*>(c->qscan.as<char>() + c->qscan.bytes - 16);
  phase_begin(c, 4, s);
  hipLaunchKernelGGL(k_pair_scan, dim3((unsigned)ntiles), dim3(kScanThreads), 0, s, qu, qi, qj, Q,
                     c->idx.side[0].ptr.as<int64_t>(), c->idx.side[1].ptr.as<int64_t>(), c->idx.U, c->idx.I, offsets,
                     c->qscan.as<unsigned long long>(), ctr, c->flag.as<int32_t>());
  FIA_HIP_TRY(hipGetLastError());
  phase_end(c, 4, s);
  return hipSuccess;
}

hipError_t pair_batch(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int32_t* qj,
                      const int64_t* offsets, int64_t total_rel, int32_t* rel_idx, double* influence, double* x_out,
                      double* diff, int K, int64_t* topk_pos, int64_t* topk_idx, double* topk_val, hipStream_t s) {
  PairArgs A = pair_args(c, Q, qu, qi, qj, offsets, total_rel);
  if (rel_idx && total_rel > 0) {
    phase_begin(c, 4, s);
    hipLaunchKernelGGL(k_pair_rel, dim3((unsigned)Q), dim3(256), 0, s, A, rel_idx);
    FIA_HIP_TRY(hipGetLastError());
    phase_end(c, 4, s);
  }
  if (!influence && !x_out && !diff && K <= 0) return hipSuccess;
  const QueryArgs QA = make_args(c, qu, qi);
  hipError_t e = hipErrorInvalidValue;
  dispatch_small(c->p.model, c->p.k, [&](auto m) {
    e = pair_impl<decltype(m)>(c, QA, A, influence, x_out, diff, K, topk_pos, topk_idx, topk_val, s);
  });
  return e;
}

}  // namespace fia
