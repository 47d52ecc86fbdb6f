// fia_count_related_slate / fia_slate_batch: which ratings shape a user's top-N list
// (include/fia.h).  The explained number is f = sum_l w_l r-hat(u, i_l) over a slate of m distinct
// items, 1 <= m <= FIA_SLATE_MAX_ITEMS.  Its FIA system is pair.hip's with m item blocks in place
// of two: theta_t = (theta_u, theta_i1 .. theta_im), the related list R_u ++ C_i1 ++ .. ++ C_im
// with n its length, one Hessian over that list and one solve:
//
//   H_uu = (2/n) (A_u + sum_l cd_l v^l_u v^l_u^T)        H_ll = (2/n) (B_il + cd_l v^l_l v^l_l^T)
//   H_lu = (2/n) 2 (cd_l v^l_l v^l_u^T + es_l diag(E))   H_lm = 0 (l != m)
//   + wd diag(M) + damping I,   v = (sum_l w_l v^l_u, w_1 v^1_1, .., w_m v^m_m),   x = H^-1 v
//   influence_p = x . (2 e_p g_p + wd M theta_t) / n
//
// H is an arrowhead, and the solve uses it: the (m + 1) Ds triangle is never formed.  With
// alpha = 4 / n, S = H_uu and r = v_u, the items are walked in slate order; each item block is
// assembled into LDS, factored (LDL^T of solve.h) and solved for pv = H_ll^-1 v^l_l.  An item the
// user has not rated (cd_l = 0) is done: x_l = w_l pv.  A rated item takes its Schur complement
// out of S and r:
//   S -= alpha^2 (cd^2 (v_l . pv) v_u v_u^T + cd es (v_u (E o pv)^T + (E o pv) v_u^T) + es^2 E H_ll^-1 E)
//   r -= alpha w_l (cd (v_l . pv) v_u + es E o pv)
// the last term of S column by column from the substitutions on the factor (ldlt_resolve of
// newton.h), no Ds x Ds block stored.  Then S x_u = r, and a second pass over the rated items alone
// assembles and factors H_ll again for
//   x_l = w_l pv - alpha cd (v_u . x_u) pv - alpha es H_ll^-1 (E o x_u).
// LDS: two packed Ds triangles, a handful of Ds vectors and (NCF) the staged weights.
//
// Kernels:
//   k_slate_scan      per query the checks (slate length, id ranges, repeated items, the
//                     prepare_for cover), n and its exclusive prefix, one launch (scan.h's look-back)
//   k_slate_rel       rel_idx from the CSR / CSC lists, a workgroup per query
//   k_slate_solve     persistent one-wave workgroups: the route above; x_out, value, the scoring
//                     record (one HALF per (query, item)), the query's list starts, its items sorted
//                     and the scoring tiles that start inside its list
//   k_slate_score     k_pair_score's decomposition: tiles of kCandTile consecutive positions of the
//                     batch's flat related array, a position per thread -- its query by a search of
//                     offsets, its list by a search of the query's list starts, its entry scored with
//                     the pieces of cand.h; with top-K every (tile, query) segment selects into slot
//                     tile + q
//   k_cand_merge (score_cand.hip), k_slate_topk_idx   the per-query merge, then topk_idx
// No floating-point atomics, every sum in slate order: a query's bits depend on (u, the items in
// their order, the weights) alone.
#include "cand.h"
#include "newton.h"
#include "scan.h"
#include "solve.h"

namespace fia {
namespace {

constexpr int kSlateMax = FIA_SLATE_MAX_ITEMS;
constexpr int kSlateRecGrid = 1 << 20;   // most workgroups of the per-query kernels (grid-stride)
static_assert(kSlateMax <= kSolveThreads, "a lane per slate item");

// The scoring record k_slate_solve writes and k_slate_score reads: one HALF per (query, item), half
// slate_offsets[q] + l for item l, so that coop_dots (cand.h) picks the item block of a position by
// the half's index.  MF: the layout below (pair.hip's); NCF: CandRecNCF of cand.h.  The head
// (1 / n, c_q) and the user entries are those of the query's first half.  Offsets in doubles.
template <int K>
struct SlateRecMF : CandHead {
  static constexpr int x_user = head;               // [K] x at p_u
  static constexpr int x_item = head + K;           // [K] x at q_il (half l)
  static constexpr int x_bias_user = head + 2 * K;
  static constexpr int x_bias_item = head + 2 * K + 1;
  static constexpr int size = head + 2 * K + 2;
};
template <class M>
constexpr int slate_half() {
  return M::ncf ? CandRecNCF<M::K>::size : SlateRecMF<M::K>::size;
}

struct SlateArgs : ModelArgs {
  int64_t Q, total, total_items;
  const int32_t* qu;
  const int64_t* soff;      // [Q + 1] slate offsets
  const int32_t* item;      // [total_items]
  const double* weight;     // [total_items]
  const int64_t* off;       // [Q + 1]
  const int32_t* row[2];    // the lists of both sides (train row, other endpoint, rating)
  const int32_t* other[2];
  const float* rating[2];
  int64_t tiles;            // ceil(total / kCandTile)
  int32_t* tile_q;          // [tiles]: the query of each tile's first position (k_slate_solve)
  double* rec;              // [total_items * slate_half]
  // written by k_slate_solve for the scoring pass, per query: whether it is scored at all, the
  // starts of its m + 1 lists inside its related list (at slate_offsets[q] + q) and its items
  // sorted with their slate index (at slate_offsets[q])
  int32_t* qok;             // [Q]
  int64_t* lbeg;            // [total_items + Q]
  int32_t* sitem;           // [total_items]
  int32_t* sidx;            // [total_items]
};

// slate [sb, se) of a batch with `total_items` items: inside the arrays and of a legal length
__device__ __forceinline__ bool slate_shape_ok(int64_t sb, int64_t se, int64_t total_items) {
  return sb >= 0 && se <= total_items && se - sb >= 1 && se - sb <= kSlateMax;
}

// One wave, lane l holding item l of an m-item slate (it; lanes >= m idle): every id in range and
// no item twice.  sit: the wave's LDS copy of the items, written here.
__device__ __forceinline__ bool slate_items_ok(int32_t it, int m, int lane, int64_t I, int32_t* sit) {
  if (lane < m) sit[lane] = it;
  __syncthreads();
  bool bad = false;
  if (lane < m) {
    bad = it < 0 || it >= I;
    for (int l2 = 0; l2 < lane; ++l2) bad |= sit[l2] == it;
  }
  return !__any(bad);
}

// Position p of the related list of a scored query (qok): its list (0 the user's, 1 + l item l's;
// -1 past the list's end) and its index into that side's list arrays
__device__ __forceinline__ int slate_locate(const SlateArgs& A, int64_t q, int32_t u, int64_t sb, int m, int64_t p,
                                            int64_t& entry) {
  const int64_t* __restrict__ lb = A.lbeg + sb + q;
  const int list = last_at_most(lb, 0, m, p);
  const int64_t rp = p - lb[list];
  int64_t b0, len;
  if (list == 0) {
    b0 = A.ptr[0][u];
    len = A.ptr[0][u + 1] - b0;
  } else {
    const int32_t it = A.item[sb + list - 1];
    b0 = A.ptr[1][it];
    len = A.ptr[1][it + 1] - b0;
  }
  entry = b0 + rp;
  return rp >= 0 && rp < len ? list : -1;
}

// n = |R_u| + sum_l |C_il| per query (0 and flag[1]: a bad slate length, an id out of range or a
// repeated item) and its exclusive prefix, the total at [Q]: k_pair_scan's single pass.  mark
// (small k) / slot0, slot1 (large k), each nullable: the cover of the last fia_prepare_for, flag[2]
// when an entity of a good query is outside it.
__global__ __launch_bounds__(kScanThreads) void k_slate_scan(
    const int32_t* __restrict__ qu, const int64_t* __restrict__ soff, int64_t total_items,
    const int32_t* __restrict__ item, int64_t Q, const int64_t* __restrict__ uptr, const int64_t* __restrict__ iptr,
    int64_t U, int64_t I, const uint8_t* __restrict__ mark, const int32_t* __restrict__ slot0,
    const int32_t* __restrict__ slot1, int64_t* __restrict__ out, unsigned long long* __restrict__ tstate,
    unsigned int* __restrict__ tctr, int32_t* __restrict__ flag) {
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
    const int32_t u = qu[q];
    const int64_t sb = soff[q], se = soff[q + 1];
    bool ok = slate_shape_ok(sb, se, total_items) && u >= 0 && u < U;
    if (ok) {
      const int m = (int)(se - sb);
      int64_t n = uptr[u + 1] - uptr[u];
      bool out_of_cover = (mark && !mark[u]) || (slot0 && slot0[u] < 0);
      for (int l = 0; l < m && ok; ++l) {
        const int32_t it = item[sb + l];
        ok = it >= 0 && it < I;
        for (int l2 = 0; l2 < l && ok; ++l2) ok = item[sb + l2] != it;
        if (ok) {
          n += iptr[it + 1] - iptr[it];
          out_of_cover |= (mark && !mark[U + it]) || (slot1 && slot1[it] < 0);
        }
      }
      if (ok) {
        x = n;
        if (out_of_cover) atomicOr(flag + 2, 1);
      }
    }
    if (!ok) atomicOr(flag + 1, 1);
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

// one workgroup per query: rel[offsets[q] + p] = R_u[p], then C_i1 .. C_im
__global__ __launch_bounds__(256) void k_slate_rel(SlateArgs A, int32_t* __restrict__ rel) {
  __shared__ int32_t sit[kSlateMax];
  __shared__ int s_ok;
  const int64_t q = blockIdx.x;
  const int32_t u = A.qu[q];
  const int64_t sb = A.soff[q], se = A.soff[q + 1];
  if (!slate_shape_ok(sb, se, A.total_items) || u < 0 || u >= A.U) return;   // (uniform)
  const int m = (int)(se - sb);
  const int tid = threadIdx.x;
  if (tid < m) sit[tid] = A.item[sb + tid];
  __syncthreads();
  if (tid < 64) {
    bool bad = false;
    if (tid < m) {
      const int32_t it = sit[tid];
      bad = it < 0 || it >= A.I;
      for (int l2 = 0; l2 < tid; ++l2) bad |= sit[l2] == it;
    }
    const bool any_bad = __any(bad);
    if (tid == 0) s_ok = !any_bad;
  }
  __syncthreads();
  if (!s_ok) return;
  int64_t base = A.off[q];
  const int64_t end = A.off[q + 1] < A.total ? A.off[q + 1] : A.total;   // (never past the array)
  if (base < 0) return;
  for (int l = 0; l <= m; ++l) {
    const int sd = l ? 1 : 0;
    const int64_t e = l ? sit[l - 1] : u;
    const int64_t lb = A.ptr[sd][e], ln = A.ptr[sd][e + 1] - lb;
    const int32_t* __restrict__ src = A.row[sd] + lb;
    for (int64_t p = tid; p < ln && base + p < end; p += blockDim.x) rel[base + p] = src[p];
    base += ln;
  }
}

// coordinate c of block b (0 the user's, 1 + l item l's) of an m-item slate -> the reference theta
// order, extended: MF [p_u, q_1 .. q_m, b_u, b_1 .. b_m], NCF [Pm_u, Qm_1 .., Pg_u, Qg_1 ..]
template <class M>
__device__ __forceinline__ int64_t slate_ref_index(int b, int c, int m) {
  constexpr int K = M::K;
  if constexpr (!M::ncf) return c < K ? (int64_t)b * K + c : (int64_t)(m + 1) * K + b;
  else return c < K ? (int64_t)b * K + c : (int64_t)(m + 1) * K + (int64_t)b * K + (c - K);
}

template <class M>
constexpr int64_t slate_lds_bytes() {
  constexpr int64_t K = M::K, D = M::D, Ds = M::Ds;
  // S and Hl; g and th; five Ds vectors; the slate's items and weights; NCF: the prologue's scratch,
  // W1, b1 and the staged weights
  return 8 * (Ds * (Ds + 1) + 2 * D + 5 * Ds + kSlateMax / 2 + kSlateMax +
              (M::ncf ? 4 * K + 8 + 2 * K * K + K + K * (K / 2) + 2 * K : 8));
}

// row and column (c <= r) of element t of a packed lower triangle
__device__ __forceinline__ void tri_rc(int t, int& r, int& c) {
  r = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while (tri(r + 1, 0) <= t) ++r;
  while (tri(r, 0) > t) --r;
  c = t - tri(r, 0);
}

template <class M>
__global__ __launch_bounds__(kSolveThreads) void k_slate_solve(QueryArgs A, SlateArgs P, double* __restrict__ x_out,
                                                               double* __restrict__ value) {
  constexpr int K = M::K, Ds = M::Ds, D = M::D, GS = Ds * (Ds + 1) / 2, HS = slate_half<M>();
  __shared__ double S[GS], Hl[GS];                  // the user block's Schur complement; the item block
  __shared__ double g[D], th[D];                    // v^l and theta of (u, i_l): [user | item]
  __shared__ double rr[Ds], pv[Ds], tv[Ds], dd[Ds], ww[Ds];
  __shared__ double sh[4 * K + 8];
  __shared__ int32_t sit[kSlateMax];
  __shared__ double swt[kSlateMax];
  __shared__ NCFWeights<M::ncf ? K : 2> w;
  __shared__ double sW1[M::ncf ? 2 * K * K : 1];
  __shared__ double sb1[M::ncf ? K : 1];
  stage_ncf<M>(A, w, sW1, sb1);
  const int lane = threadIdx.x;
  // E: the diagonal of the own pair's d2 r-hat / d theta_i d theta_u
  auto E = [&](int a) -> double {
    if constexpr (!M::ncf) return a < K ? 1.0 : 0.0;
    else return a >= K ? w.W3[K / 2 + (a - K)] : 0.0;
  };
  constexpr int e_lo = M::ncf ? K : 0, e_hi = M::ncf ? 2 * K : K;      // the coordinates where E != 0
  for (int64_t q = blockIdx.x; q < P.Q; q += gridDim.x) {
    __syncthreads();
    const int32_t u = P.qu[q];
    const int64_t sb = P.soff[q], se = P.soff[q + 1];
    if (P.tile_q) {
      // the tiles whose first position is one of this query's: each tile is named by exactly one
      // (non-empty) query, so the scoring workgroups start without a search
      const int64_t cb = P.off[q] > 0 ? P.off[q] : 0, ce = P.off[q + 1];
      for (int64_t t = (cb + kCandTile - 1) / kCandTile + lane; t < P.tiles && t * kCandTile < ce; t += 64)
        P.tile_q[t] = (int32_t)q;
    }
    // the slate's own range of the per-item arrays: nothing outside it is touched
    const bool in_arrays = sb >= 0 && se >= sb && se <= P.total_items;
    const int64_t mm = in_arrays ? se - sb : 0;
    double* __restrict__ xo = x_out && in_arrays ? x_out + (int64_t)Ds * (sb + q) : nullptr;
    double* __restrict__ Rq = P.rec + sb * HS;
    bool ok = in_arrays && mm >= 1 && mm <= kSlateMax && u >= 0 && u < A.U;
    const int m = ok ? (int)mm : 0;
    if (ok) {
      const int32_t it = lane < m ? P.item[sb + lane] : 0;
      if (lane < m) swt[lane] = P.weight[sb + lane];
      ok = slate_items_ok(it, m, lane, A.I, sit);
    }
    if (lane == 0) P.qok[q] = ok ? 1 : 0;
    int64_t n = 0;
    if (ok) {
      // the list starts, the sorted items and n
      const int64_t du = A.ptr[0][u + 1] - A.ptr[0][u];
      const int32_t it = lane < m ? sit[lane] : 0;
      const int64_t len = lane < m ? A.ptr[1][it + 1] - A.ptr[1][it] : 0;
      int64_t inc = len;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int64_t y = __shfl_up(inc, off);
        if (lane >= off) inc += y;
      }
      n = du + __shfl(inc, 63);
      if (lane == 0) P.lbeg[sb + q] = 0;
      if (lane < m) {
        P.lbeg[sb + q + 1 + lane] = du + inc - len;
        int rank = 0;
        for (int l2 = 0; l2 < m; ++l2) rank += sit[l2] < it;
        P.sitem[sb + rank] = it;
        P.sidx[sb + rank] = lane;
      }
    }
    if (!ok || n == 0) {
      // a bad slate: NaN everywhere (an id out of range is never an index); a good one with no
      // related rating: a NaN x and the finite value
      double f = NAN;
      if (ok) {
        f = 0.0;
        for (int l = 0; l < m; ++l) {
          __syncthreads();
          f += swt[l] * solve_prologue<M, kSolveThreads>(A, u, sit[l], th, g, sh, w, sW1, sb1);
        }
      }
      if (lane == 0 && value) value[q] = f;
      if (xo)
        for (int64_t a = lane; a < (int64_t)Ds * (mm + 1); a += kSolveThreads) xo[a] = NAN;
      if (in_arrays)
        for (int64_t a = lane; a < mm * HS; a += kSolveThreads) Rq[a] = NAN;
      continue;
    }
    const double s2n = 2.0 / (double)n, alpha = 2.0 * s2n, inv_n = 1.0 / (double)n;
    // ---- S = H_uu without the own pairs' terms, r = 0 ----
    {
      const double* __restrict__ Gu = A.gram[0] + (int64_t)u * ((GS + 1) & ~1);
      for (int t = lane; t < GS; t += kSolveThreads) {
        int r, c;
        tri_rc(t, r, c);
        double h = s2n * Gu[gidx<M>(r, c)];
        if (r == c) h += (M::decayed(r) ? A.wd : 0.0) + A.damping;
        S[t] = h;
      }
      for (int a = lane; a < Ds; a += kSolveThreads) rr[a] = 0.0;
    }
    double f = 0.0, part = 0.0;                       // the value; this lane's share of x . M theta_t
    // x_l (in tv) of item l: x_out, the record's half l and the decay sum
    auto emit_item = [&](int l) {
      double* __restrict__ Rl = Rq + (int64_t)l * HS;
      for (int a = lane; a < Ds; a += kSolveThreads) {
        if (xo) xo[slate_ref_index<M>(1 + l, a, m)] = tv[a];
        if (M::decayed(a)) part += tv[a] * th[Ds + a];
      }
      if constexpr (!M::ncf) {
        using L = SlateRecMF<K>;
        for (int a = lane; a < K; a += kSolveThreads) Rl[L::x_item + a] = tv[a];
        if (lane == 0) Rl[L::x_bias_item] = tv[K];
      } else {
        // y_item = W1[k:]^T x_Qm (x_mlp . (W1_side d1) = y_side . d1) and W3g * x_Qg, as query_record
        using L = CandRecNCF<K>;
        for (int c = lane; c < K; c += kSolveThreads) {
          double yi = 0.0;
          for (int a = 0; a < K; ++a) yi = fma(sW1[(K + a) * K + c], tv[a], yi);
          Rl[L::y_item + c] = yi;
          Rl[L::w3g_x_qg + c] = w.W3[K / 2 + c] * tv[K + c];
        }
      }
    };
    // (u, i_l): the prologue, the pair lookup, H_ll into Hl (with `first` the own pair's term into S
    // too) and pv = v^l_l; factors Hl and solves pv = H_ll^-1 v^l_l.  Returns r-hat(u, i_l).
    auto item_block = [&](int l, bool first, double& cd, double& es) -> double {
      __syncthreads();
      const int32_t il = sit[l];
      const double rhat = solve_prologue<M, kSolveThreads>(A, u, il, th, g, sh, w, sW1, sb1);
      double rs;
      A.pairs.lookup((unsigned long long)u * (unsigned long long)A.I + (unsigned long long)il, cd, rs);
      es = cd * rhat - rs;
      const double* __restrict__ Gi = A.gram[1] + (int64_t)il * ((GS + 1) & ~1);
      for (int t = lane; t < GS; t += kSolveThreads) {
        int r, c;
        tri_rc(t, r, c);
        double h = s2n * (Gi[gidx<M>(r, c)] + cd * g[Ds + r] * g[Ds + c]);
        if (r == c) h += (M::decayed(r) ? A.wd : 0.0) + A.damping;
        Hl[t] = h;
        if (first && cd > 0.0) S[t] += s2n * cd * g[r] * g[c];
      }
      for (int a = lane; a < Ds; a += kSolveThreads) pv[a] = g[Ds + a];
      __syncthreads();
      ldlt_solve<Ds>(Hl, pv, dd, ww, 0, Ds);
      return rhat;
    };
    // ---- pass 1, slate order: every item block; the rated items' Schur complements ----
    for (int l = 0; l < m; ++l) {
      double cd, es;
      const double wl = swt[l];
      f += wl * item_block(l, true, cd, es);
      for (int a = lane; a < Ds; a += kSolveThreads) rr[a] += wl * g[a];
      if (!(cd > 0.0)) {
        for (int a = lane; a < Ds; a += kSolveThreads) tv[a] = wl * pv[a];
        __syncthreads();
        emit_item(l);
        continue;
      }
      double dot = 0.0;
      for (int a = lane; a < Ds; a += kSolveThreads) dot += g[Ds + a] * pv[a];
      dot = wave_sum(dot);                            // v_l . H_ll^-1 v_l
      const double a2 = alpha * alpha;
      for (int t = lane; t < GS; t += kSolveThreads) {
        int r, c;
        tri_rc(t, r, c);
        S[t] -= a2 * (cd * cd * dot * g[r] * g[c] + cd * es * (g[r] * (E(c) * pv[c]) + (E(r) * pv[r]) * g[c]));
      }
      for (int a = lane; a < Ds; a += kSolveThreads) rr[a] -= alpha * wl * (cd * dot * g[a] + es * (E(a) * pv[a]));
      // es^2 E H_ll^-1 E, a column per coordinate where E != 0: the substitutions alone
      for (int c = e_lo; c < e_hi; ++c) {
        __syncthreads();
        for (int a = lane; a < Ds; a += kSolveThreads) tv[a] = a == c ? 1.0 : 0.0;
        __syncthreads();
        ldlt_resolve<Ds>(Hl, tv, dd);
        const double ec = a2 * es * es * E(c);
        for (int r = c + lane; r < Ds; r += kSolveThreads) S[tri(r, c)] -= ec * E(r) * tv[r];
      }
    }
    // ---- S x_u = r ----
    __syncthreads();
    ldlt_solve<Ds>(S, rr, dd, ww, 0, Ds);
    __syncthreads();
    for (int a = lane; a < Ds; a += kSolveThreads) {
      if (xo) xo[slate_ref_index<M>(0, a, m)] = rr[a];
      if (M::decayed(a)) part += rr[a] * th[a];
    }
    if constexpr (!M::ncf) {
      using L = SlateRecMF<K>;
      for (int a = lane; a < K; a += kSolveThreads) Rq[L::x_user + a] = rr[a];
      if (lane == 0) Rq[L::x_bias_user] = rr[K];
    } else {
      using L = CandRecNCF<K>;
      for (int c = lane; c < K; c += kSolveThreads) {
        double yu = 0.0;
        for (int a = 0; a < K; ++a) yu = fma(sW1[a * K + c], rr[a], yu);
        Rq[L::y_user + c] = yu;
        Rq[L::w3g_x_pg + c] = w.W3[K / 2 + c] * rr[K + c];
      }
    }
    // ---- pass 2, the rated items alone: x_l from x_u ----
    for (int l = 0; l < m; ++l) {
      double cd, rs;
      A.pairs.lookup((unsigned long long)u * (unsigned long long)A.I + (unsigned long long)sit[l], cd, rs);
      if (!(cd > 0.0)) continue;
      double es;
      const double wl = swt[l];
      item_block(l, false, cd, es);
      for (int a = lane; a < Ds; a += kSolveThreads) tv[a] = E(a) * rr[a];
      __syncthreads();
      ldlt_resolve<Ds>(Hl, tv, dd);
      double dot = 0.0;
      for (int a = lane; a < Ds; a += kSolveThreads) dot += g[a] * rr[a];
      dot = wave_sum(dot);                            // v_u . x_u
      for (int a = lane; a < Ds; a += kSolveThreads) tv[a] = wl * pv[a] - alpha * cd * dot * pv[a] - alpha * es * tv[a];
      __syncthreads();
      emit_item(l);
    }
    part = wave_sum(part);
    if (lane == 0) {
      Rq[CandHead::inv_n] = inv_n;
      Rq[CandHead::c_q] = A.wd * part * inv_n;
      if (value) value[q] = f;
    }
  }
}

template <class M>
__global__ __launch_bounds__(kCandTile) void k_slate_score(SlateArgs A, double* __restrict__ influence, int K,
                                                           int32_t* __restrict__ cand_pos,
                                                           double* __restrict__ cand_val) {
  constexpr int KK = M::K, HS = slate_half<M>();
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
  // the tile's first query and the next tile's (k_slate_solve wrote them; clamped, so offsets that
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
  int sel = 0;                                // the item block of the position: its slate index
  int h0 = 0;                                 // the query's first half
  if (active) {
    if (qhi != qlo) q = last_at_most(A.off, qlo, qhi, g);
    const int64_t p = g - A.off[q];
    pos = (int)p;
    // a query k_slate_solve refused (a bad slate, an id out of range) is never used as an index; a
    // position no list holds scores NaN
    if (p >= 0 && A.qok[q]) {
      const int32_t u = A.qu[q];
      const int64_t sb = A.soff[q];
      const int m = (int)(A.soff[q + 1] - sb);
      h0 = (int)sb;
      int64_t entry;
      const int list = slate_locate(A, q, u, sb, m, p, entry);
      if (list >= 0) {
        valid = true;
        const int sd = list ? 1 : 0;
        const int32_t o = A.other[sd][entry];
        y = A.rating[sd][entry];
        // an entry of the user's list whose item is in the slate also takes that item block's term
        // (a search of the query's sorted items), an entry of an item list whose user is u the
        // user block's
        if (list) {
          a = o;
          b = A.item[sb + list - 1];
          on_u = a == u;
          on_it = true;
          sel = list - 1;
        } else {
          a = u;
          b = o;
          on_u = true;
          const int32_t* __restrict__ si = A.sitem + sb;
          int lo = 0, hi = m - 1;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (si[mid] < b) lo = mid + 1; else hi = mid;
          }
          on_it = si[lo] == b;
          sel = on_it ? A.sidx[sb + lo] : 0;
        }
      }
    }
  }
  // (whole waves from here: the row gathers are cooperative).  The query's first half holds the
  // head and the user entries, half h0 + sel item sel's at the same offsets
  const int hit = h0 + sel;
  const double* __restrict__ R0 = A.rec + (int64_t)h0 * HS;
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
      cand_core_ncf<KK>(A, w, a, b, on_u, on_it, R0 + L::y_user, R0 + (int64_t)sel * HS + L::y_item, z1s + tid, r, s);
      s += sgu + sgi;
      r += rg + (double)A.t[9][0];
      val = R0[L::c_q] + 2.0 * (r - (double)y) * s * R0[L::inv_n];
    }
  } else {
    using L = SlateRecMF<KK>;
    double r, su, si;
    coop_dots<KK, false, HS, L::x_user, L::x_item, true>(valid, a, b, h0, on_u, on_it, A.t[0], A.t[1], A.rec, nullptr,
                                                         r, su, si, hit);
    if (valid) {
      r += (double)A.t[2][a] + (double)A.t[3][b] + (double)A.t[4][0];
      if (on_u) su += R0[L::x_bias_user];
      if (on_it) si += R0[(int64_t)sel * HS + L::x_bias_item];
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
__global__ void k_slate_topk_idx(SlateArgs A, int K, const int64_t* __restrict__ topk_pos,
                                 int64_t* __restrict__ topk_idx) {
  const int64_t n = A.Q * K;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = s / K, p = topk_pos[s];
    int64_t idx = -1;
    if (p >= 0 && A.qok[q]) {
      const int64_t sb = A.soff[q];
      int64_t entry;
      const int list = slate_locate(A, q, A.qu[q], sb, (int)(A.soff[q + 1] - sb), p, entry);
      if (list >= 0) idx = A.row[list ? 1 : 0][entry];
    }
    topk_idx[s] = idx;
  }
}

SlateArgs slate_args(fia_ctx* c, int64_t Q, const int32_t* qu, const int64_t* soff, int64_t total_items,
                     const int32_t* item, const double* weight, const int64_t* off, int64_t total) {
  SlateArgs A{};
  fill_model_args(c, A);
  A.Q = Q;
  A.total = total;
  A.total_items = total_items;
  A.qu = qu;
  A.soff = soff;
  A.item = item;
  A.weight = weight;
  A.off = off;
  for (int s = 0; s < 2; ++s) {
    A.row[s] = c->idx.side[s].row.as<int32_t>();
    A.other[s] = c->idx.side[s].other.as<int32_t>();
    A.rating[s] = c->idx.side[s].rating.as<float>();
  }
  return A;
}

template <class M>
hipError_t slate_impl(fia_ctx* c, const QueryArgs& QA, SlateArgs A, double* influence, double* x_out, double* value,
                      int K, int64_t* topk_pos, int64_t* topk_idx, double* topk_val, hipStream_t s) {
  constexpr int HS = slate_half<M>();
  const int64_t Q = A.Q, TI = A.total_items;
  const bool score = influence || K > 0;
  const int64_t tiles = score ? (A.total + kCandTile - 1) / kCandTile : 0;
  FIA_HIP_TRY(c->rec.reserve(sizeof(double) * (size_t)(TI * HS), s));
  FIA_HIP_TRY(c->nch.reserve(sizeof(int64_t) * (size_t)(TI + Q), s));
  FIA_HIP_TRY(c->tkeys.reserve(sizeof(int32_t) * (size_t)(2 * TI + Q), s));
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
  A.lbeg = c->nch.as<int64_t>();
  A.sitem = c->tkeys.as<int32_t>();
  A.sidx = A.sitem + TI;
  A.qok = A.sidx + TI;
  phase_begin(c, 1, s);
  // persistent workgroups (NCF weights staged once each), as many as their LDS lets be resident
  const int64_t cap = solve_grid_cap(c, slate_lds_bytes<M>());
  hipLaunchKernelGGL(k_slate_solve<M>, dim3((unsigned)(Q < cap ? Q : cap)), dim3(kSolveThreads), 0, s, QA, A, x_out,
                     value);
  FIA_HIP_TRY(hipGetLastError());
  phase_end(c, 1, s);
  if (tiles > 0) {
    phase_begin(c, 2, s);
    hipLaunchKernelGGL(k_slate_score<M>, dim3((unsigned)tiles), dim3(kCandTile), 0, s, A, influence, K,
                       c->cand_pos.as<int32_t>(), c->cand_val.as<double>());
    FIA_HIP_TRY(hipGetLastError());
    phase_end(c, 2, s);
  }
  if (K > 0) {
    phase_begin(c, 3, s);
    FIA_HIP_TRY(launch_cand_merge(c, Q, A.total, A.off, K, topk_pos, topk_val, s));
    const int64_t nb = (Q * K + 255) / 256;
    hipLaunchKernelGGL(k_slate_topk_idx, dim3((unsigned)(nb < kSlateRecGrid ? nb : kSlateRecGrid)), dim3(256), 0, s, A,
                       K, topk_pos, topk_idx);
    FIA_HIP_TRY(hipGetLastError());
    phase_end(c, 3, s);
  }
  return hipSuccess;
}

}  // namespace

bool slate_supported(int model, int k) {
  return dispatch_small(model, k, [](auto) {});
}

hipError_t count_related_slate(fia_ctx* c, int64_t Q, const int32_t* qu, const int64_t* slate_offsets,
                               int64_t total_items, const int32_t* slate_item, int64_t* offsets, bool cover,
                               hipStream_t s) {
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
  // the cover of the last fia_prepare_for: the marks (small k) or the cache slots (large k)
  const uint8_t* mark = cover && c->small_subset ? c->mark.as<uint8_t>() : nullptr;
  const int32_t* slot0 = cover && c->subset ? c->slot[0].as<int32_t>() : nullptr;
  const int32_t* slot1 = cover && c->subset ? c->slot[1].as<int32_t>() : nullptr;
  phase_begin(c, 4, s);
  hipLaunchKernelGGL(k_slate_scan, dim3((unsigned)ntiles), dim3(kScanThreads), 0, s, qu, slate_offsets, total_items,
                     slate_item, Q, c->idx.side[0].ptr.as<int64_t>(), c->idx.side[1].ptr.as<int64_t>(), c->idx.U,
                     c->idx.I, mark, slot0, slot1, offsets, c->qscan.as<unsigned long long>(), ctr,
                     c->flag.as<int32_t>());
  FIA_HIP_TRY(hipGetLastError());
  phase_end(c, 4, s);
  return hipSuccess;
}

hipError_t slate_batch(fia_ctx* c, int64_t Q, const int32_t* qu, const int64_t* slate_offsets, int64_t total_items,
                       const int32_t* slate_item, const double* slate_weight, const int64_t* offsets,
                       int64_t total_rel, int32_t* rel_idx, double* influence, double* x_out, double* value, int K,
                       int64_t* topk_pos, int64_t* topk_idx, double* topk_val, hipStream_t s) {
  SlateArgs A = slate_args(c, Q, qu, slate_offsets, total_items, slate_item, slate_weight, offsets, total_rel);
  if (rel_idx && total_rel > 0) {
    phase_begin(c, 4, s);
    hipLaunchKernelGGL(k_slate_rel, dim3((unsigned)Q), dim3(256), 0, s, A, rel_idx);
    FIA_HIP_TRY(hipGetLastError());
    phase_end(c, 4, s);
  }
  if (!influence && !x_out && !value && K <= 0) return hipSuccess;
  const QueryArgs QA = make_args(c, qu, nullptr);
  hipError_t e = hipErrorInvalidValue;
  dispatch_small(c->p.model, c->p.k, [&](auto m) {
    e = slate_impl<decltype(m)>(c, QA, A, influence, x_out, value, K, topk_pos, topk_idx, topk_val, s);
  });
  return e;
}

}  // namespace fia
