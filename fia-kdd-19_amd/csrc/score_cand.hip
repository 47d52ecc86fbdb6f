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
#include "kern.h"

namespace fia {
namespace {

constexpr int kCandTile = 256;        // candidates per scoring workgroup, one per thread
constexpr int kCandRecGrid = 1 << 20; // most workgroups of the per-query kernels (grid-stride)

struct CandArgs {
  int64_t Q, total;
  const int32_t* qu;
  const int32_t* qi;
  const double* x;        // [Q * D], reference theta order
  const int64_t* off;     // [Q + 1]
  const int32_t* cu;
  const int32_t* ci;
  const float* cy;
  int64_t U, I;
  const int64_t* ptr[2];
  const float* t[10];
  const double* l1[2];
  double wd;
  int64_t tiles;          // ceil(total / kCandTile)
  int32_t* tile_q;        // [tiles]: the query of each tile's first candidate (k_cand_rec)
};

template <class M>
constexpr int cand_rec_size() {
  // {1 / n_q, c_q}; NCF: + y_user[K], y_item[K], W3g * x_Pg [K], W3g * x_Qg [K]
  return M::ncf ? 2 + 4 * M::K : 2;
}

__device__ __forceinline__ double cand_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <class M>
__global__ __launch_bounds__(64) void k_cand_rec(CandArgs A, double* __restrict__ rec) {
  constexpr int K = M::K, D = M::D, R = cand_rec_size<M>();
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
    const double* __restrict__ xq = A.x + q * D;
    const int64_t n = (A.ptr[0][u + 1] - A.ptr[0][u]) + (A.ptr[1][i + 1] - A.ptr[1][i]);
    double part = 0.0;
    if constexpr (!M::ncf) {
      // M = [1] * 2k + [0, 0]: the biases are not decayed
      const float* __restrict__ P = A.t[0] + (int64_t)u * K;
      const float* __restrict__ Qt = A.t[1] + (int64_t)i * K;
      for (int a = lane; a < K; a += 64) part += xq[a] * (double)P[a] + xq[K + a] * (double)Qt[a];
    } else {
      const float* __restrict__ Pm = A.t[0] + (int64_t)u * K;
      const float* __restrict__ Qm = A.t[1] + (int64_t)i * K;
      const float* __restrict__ Pg = A.t[2] + (int64_t)u * K;
      const float* __restrict__ Qg = A.t[3] + (int64_t)i * K;
      for (int a = lane; a < K; a += 64)
        part += xq[a] * (double)Pm[a] + xq[K + a] * (double)Qm[a] + xq[2 * K + a] * (double)Pg[a] +
                xq[3 * K + a] * (double)Qg[a];
    }
    part = cand_wave_sum(part);
    const double inv_n = 1.0 / (double)n;     // n_q = 0: inf, and x is NaN
    if (lane == 0) {
      Rq[0] = inv_n;
      Rq[1] = A.wd * part * inv_n;
    }
    if constexpr (M::ncf) {
      const float* __restrict__ W1 = A.t[4];
      const float* __restrict__ W3g = A.t[8] + K / 2;
      for (int c = lane; c < K; c += 64) {
        double yu = 0.0, yi = 0.0;
        for (int j = 0; j < K; ++j) {
          yu = fma((double)W1[(int64_t)j * K + c], xq[j], yu);
          yi = fma((double)W1[(int64_t)(K + j) * K + c], xq[K + j], yi);
        }
        Rq[2 + c] = yu;
        Rq[2 + K + c] = yi;
        Rq[2 + 2 * K + c] = (double)W3g[c] * xq[2 * K + c];
        Rq[2 + 3 * K + c] = (double)W3g[c] * xq[3 * K + c];
      }
    }
  }
}

// largest q in [lo, hi] with off[q] <= g (off[lo] <= g given)
__device__ __forceinline__ int64_t cand_query(const int64_t* __restrict__ off, int64_t lo, int64_t hi, int64_t g) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (off[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Three dot products over a row pair gathered by candidate ids -- r = sum_c [g_c] TA[a][c] TB[b][c],
// su = sum_c xu[c] TB[b][c] (user side on), si = sum_c xi[c] TA[a][c] (item side on) -- for the 64
// candidates of a wave, one per lane, with the rows fetched COOPERATIVELY: a lane reading its
// own two rows touches 64 cache lines per load instruction; here LPC = min(k / 4, 16) lanes
// share a candidate, each loading 16-B pieces of its rows (a load instruction covers 64 / LPC
// whole rows), in LPC rounds of 64 / LPC candidates.  The partial sums are added across the LPC
// lanes by an xor butterfly (the same bits in every lane, the same order wherever the candidate
// sits) and handed to the candidate's own lane.  The whole wave must call this (shuffles);
// lanes without a valid candidate load nothing.  xu / xi = xbase + q * XS + XU / XI.
template <int K, bool WEIGHTED, int XS, int XU, int XI>
__device__ __forceinline__ void coop_dots(bool valid, int32_t a, int32_t b, int q, bool on_u, bool on_i,
                                          const float* __restrict__ TA, const float* __restrict__ TB,
                                          const double* __restrict__ xbase, const float* __restrict__ wgt,
                                          double& r_out, double& su_out, double& si_out) {
  constexpr int P = K / 4;                  // 16-B pieces per row
  constexpr int LPC = P < 16 ? P : 16;      // lanes per candidate
  constexpr int CPR = 64 / LPC;             // candidates per round
  constexpr int PPL = P / LPC;              // pieces per lane
  const int lane = threadIdx.x & 63, sub = lane % LPC, grp = lane / LPC;
  const int flags = (valid ? 1 : 0) | (on_u ? 2 : 0) | (on_i ? 4 : 0);
  r_out = su_out = si_out = 0.0;
#pragma unroll
  for (int j = 0; j < LPC; ++j) {
    const int src = j * CPR + grp;          // this round's candidate of the lane's group
    const int fj = __shfl(flags, src);
    const int32_t aj = __shfl(a, src), bj = __shfl(b, src);
    const int qj = __shfl(q, src);
    double r = 0.0, su = 0.0, si = 0.0;
    if (fj & 1) {
      const float4* __restrict__ PA = reinterpret_cast<const float4*>(TA + (int64_t)aj * K);
      const float4* __restrict__ PB = reinterpret_cast<const float4*>(TB + (int64_t)bj * K);
      const double* __restrict__ xu = xbase + (int64_t)qj * XS + XU;
      const double* __restrict__ xi = xbase + (int64_t)qj * XS + XI;
#pragma unroll
      for (int t = 0; t < PPL; ++t) {
        const int pc = sub + t * LPC;
        const float4 p = PA[pc], w = PB[pc];
        const double pv[4] = {p.x, p.y, p.z, p.w}, wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 4 * pc + e;
          if constexpr (WEIGHTED) r = fma((double)wgt[c] * pv[e], wv[e], r);
          else r = fma(pv[e], wv[e], r);
          if (fj & 2) su = fma(xu[c], wv[e], su);
          if (fj & 4) si = fma(xi[c], pv[e], si);
        }
      }
    }
#pragma unroll
    for (int o = 1; o < LPC; o <<= 1) {
      r += __shfl_xor(r, o);
      su += __shfl_xor(su, o);
      si += __shfl_xor(si, o);
    }
    const int from = (lane % CPR) * LPC;    // the group that had lane's candidate, if this was its round
    const double gr = __shfl(r, from), gu = __shfl(su, from), gi = __shfl(si, from);
    if (lane / CPR == j) {
      r_out = gr;
      su_out = gu;
      si_out = gi;
    }
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
  const double inv_n = rec[q * 2], cq = rec[q * 2 + 1];
  const double* __restrict__ xq = A.x + q * D;
  r += (double)A.t[2][a] + (double)A.t[3][b] + (double)A.t[4][0];
  if (on_u) su += xq[2 * K];
  if (on_i) si += xq[2 * K + 1];
  const double e = r - (double)y;
  return cq + 2.0 * e * (su + si) * inv_n;
}

// NCF k <= 32: z1 = l1_user[a] + l1_item[b] + b1 of the tile's candidates staged in LDS,
// unit-major ([c][thread], rows padded by 2), the rows gathered cooperatively as in coop_dots:
// a row is k / 2 16-B pieces, a wave's load instruction covers 128 / k whole rows.  Above
// k = 32 the tile's z1 would not fit beside a second workgroup; each lane reads its own rows.
constexpr int kCandZ1Stride = kCandTile + 2;
template <int K>
constexpr bool cand_stage_z1() { return K <= 32; }

template <int K>
__device__ __forceinline__ void stage_z1(const CandArgs& A, bool valid, int32_t a, int32_t b, double* __restrict__ z1s) {
  constexpr int PZ = K / 2;                 // 16-B pieces per layer-1 row
  const int lane = threadIdx.x & 63, wbase = threadIdx.x & ~63;
#pragma unroll
  for (int it = 0; it < PZ; ++it) {
    const int e = it * 64 + lane, row = e / PZ, pc = e % PZ;
    const int vr = __shfl((int)valid, row);
    const int32_t ar = __shfl(a, row), br = __shfl(b, row);
    if (vr) {
      const double2 lu = reinterpret_cast<const double2*>(A.l1[0] + (int64_t)ar * K)[pc];
      const double2 li = reinterpret_cast<const double2*>(A.l1[1] + (int64_t)br * K)[pc];
      z1s[(2 * pc) * kCandZ1Stride + wbase + row] = lu.x + li.x + (double)A.t[5][2 * pc];
      z1s[(2 * pc + 1) * kCandZ1Stride + wbase + row] = lu.y + li.y + (double)A.t[5][2 * pc + 1];
    }
  }
}

// NCF: z1 from the per-entity layer-1 rows; the MLP's share of x . g_c is y_side . d1 with
// d1 = 1[z1 > 0] (W2 (1[z2 > 0] W3m)) -- W1 is never touched per candidate.
// W2 / b2 / W3 come from LDS (fp64) up to k = 64 and from wave-uniform global loads above.
template <int K>
__device__ __forceinline__ double cand_value_ncf(const CandArgs& A, const double* __restrict__ rec,
                                                 const NCFWeights<(K <= 64 ? K : 2)>& w, int64_t q, int32_t a,
                                                 int32_t b, float y, bool on_u, bool on_i, double rg, double sg,
                                                 const double* __restrict__ z1col) {
  constexpr int H = K / 2, R = 2 + 4 * K;
  constexpr bool lds = K <= 64;
  const double* __restrict__ Rq = rec + q * R;
  const double inv_n = Rq[0], cq = Rq[1];
  const double* __restrict__ l1u = A.l1[0] + (int64_t)a * K;
  const double* __restrict__ l1i = A.l1[1] + (int64_t)b * K;
  const float* __restrict__ b1 = A.t[5];
  const float* __restrict__ gW2 = A.t[6];
  const float* __restrict__ gb2 = A.t[7];
  const float* __restrict__ gW3 = A.t[8];
  auto W2 = [&](int c, int h) -> double {
    if constexpr (lds) return w.W2[c * H + h]; else return (double)gW2[c * H + h];
  };
  auto W3 = [&](int j) -> double {
    if constexpr (lds) return w.W3[j]; else return (double)gW3[j];
  };
  // One pass over the k first-layer units per block of HC second-layer units, with two
  // accumulators per unit h: z2[h] = b2[h] + sum_c W2[c][h] relu(z1[c]) and
  // wy[h] = sum_c W2[c][h] 1[z1[c] > 0] y[c] (y = the matching sides' y_side), because
  //   y . d1 = sum_c y[c] 1[z1[c] > 0] sum_h W2[c][h] d2[h] = sum_h d2[h] wy[h],  d2[h] = 1[z2[h] > 0] W3m[h]
  // -- no d1 / d2 vector is kept, and the registers are 2 HC doubles at every k.
  constexpr int HC = H < 16 ? H : 16;
  const double* __restrict__ yu = Rq + 2;
  const double* __restrict__ yi = Rq + 2 + K;
  const bool on_any = on_u || on_i;
  double r = 0.0, s = 0.0;
#pragma unroll 1
  for (int h0 = 0; h0 < H; h0 += HC) {
    double z2[HC], wy[HC];
#pragma unroll
    for (int h = 0; h < HC; ++h) {
      if constexpr (lds) z2[h] = w.b2[h0 + h]; else z2[h] = (double)gb2[h0 + h];
      wy[h] = 0.0;
    }
#pragma unroll 1
    for (int c = 0; c < K; ++c) {
      double z1;
      if constexpr (cand_stage_z1<K>()) z1 = z1col[c * kCandZ1Stride];
      else z1 = l1u[c] + l1i[c] + (double)b1[c];
      const bool pos1 = z1 > 0.0;
      const double h1 = pos1 ? z1 : 0.0;
      double yv = 0.0;
      if (pos1 && on_u) yv += yu[c];
      if (pos1 && on_i) yv += yi[c];
#pragma unroll
      for (int h = 0; h < HC; ++h) {
        const double w2 = W2(c, h0 + h);
        z2[h] = fma(w2, h1, z2[h]);
        if (on_any) wy[h] = fma(w2, yv, wy[h]);
      }
    }
#pragma unroll
    for (int h = 0; h < HC; ++h) {
      const double w3 = W3(h0 + h);
      if (z2[h] > 0.0) {
        r = fma(w3, z2[h], r);
        s = fma(w3, wy[h], s);
      }
    }
  }
  // GMF (coop_dots, by the caller): rg = W3g . (Pg_a * Qg_b), sg = x_Pg . (W3g * Qg_b) + x_Qg . (W3g * Pg_a)
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
    if (qhi != qlo) q = cand_query(A.off, qlo, qhi, g);
    pos = (int)(g - A.off[q]);
    a = A.cu[g];
    b = A.ci[g];
    y = A.cy[g];
    // an id outside [0, U) x [0, I) is never used as an index: the candidate scores NaN
    valid = a >= 0 && a < A.U && b >= 0 && b < A.I;
  }
  // (whole waves from here: the row gathers are cooperative)
  if constexpr (M::ncf) {
    constexpr int R = 2 + 4 * KK;
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
  __shared__ double s_a[4], s_v[4];
  __shared__ int s_p[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
    // (clamped to the scored range: offsets that break cand_offsets[Q] == total_cand still
    // read inside the reserved slots)
    const int64_t e = off[q + 1] < total ? off[q + 1] : total;
    const int64_t b = off[q] < e ? (off[q] > 0 ? off[q] : 0) : e;
    const int64_t t0 = b / kCandTile;
    const int64_t nt = e > b ? (e - 1) / kCandTile - t0 + 1 : 0;
    const int64_t ncand = nt * K;
    const int32_t* __restrict__ cp = cand_pos + (t0 + q) * K;
    const double* __restrict__ cv = cand_val + (t0 + q) * K;
    double pa = INFINITY;
    int pp = -1;
    for (int t = 0; t < K; ++t) {
      double ba = -2.0, bv = 0.0;
      int bp = 0x7fffffff;
      for (int64_t j = tid; j < ncand; j += 256) {
        const int p = cp[j];
        if (p < 0) continue;
        const double val = cv[j];
        const double a = topk_key(val);
        if (better(pa, pp, a, p) && better(a, p, ba, bp)) { ba = a; bp = p; bv = val; }
      }
      wave_best(ba, bp, bv);
      if (lane == 0) { s_a[wave] = ba; s_p[wave] = bp; s_v[wave] = bv; }
      __syncthreads();
      ba = s_a[0]; bp = s_p[0]; bv = s_v[0];
#pragma unroll
      for (int w = 1; w < 4; ++w)
        if (better(s_a[w], s_p[w], ba, bp)) { ba = s_a[w]; bp = s_p[w]; bv = s_v[w]; }
      __syncthreads();
      if (tid == 0) {
        const bool ok = ba > -1.5;
        topk_pos[q * K + t] = ok ? (int64_t)bp : -1;
        topk_val[q * K + t] = ok ? bv : NAN;
      }
      pa = ba;
      pp = bp;
    }
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

hipError_t score_candidates(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const double* x,
                            const int64_t* cand_offsets, int64_t total_cand, const int32_t* cand_user,
                            const int32_t* cand_item, const float* cand_rating, double* influence, int K,
                            int64_t* topk_pos, double* topk_val, hipStream_t s, bool& unsupported) {
  CandArgs A{};
  A.Q = Q;
  A.total = total_cand;
  A.qu = qu;
  A.qi = qi;
  A.x = x;
  A.off = cand_offsets;
  A.cu = cand_user;
  A.ci = cand_item;
  A.cy = cand_rating;
  A.U = c->p.U;
  A.I = c->p.I;
  for (int sd = 0; sd < 2; ++sd) {
    A.ptr[sd] = c->idx.side[sd].ptr.as<int64_t>();
    A.l1[sd] = c->l1[sd].as<double>();
  }
  for (int t = 0; t < 10; ++t) A.t[t] = c->p.t[t];
  A.wd = c->p.wd;
  unsupported = false;
#define FIA_CAND_CASE(MODEL, KV, T)                                              \
  if (c->p.model == MODEL && c->p.k == KV) return score_impl<T<KV>>(c, A, influence, K, topk_pos, topk_val, s);
  FIA_CAND_CASE(FIA_MODEL_MF, 8, MFm)
  FIA_CAND_CASE(FIA_MODEL_MF, 16, MFm)
  FIA_CAND_CASE(FIA_MODEL_MF, 32, MFm)
  FIA_CAND_CASE(FIA_MODEL_MF, 64, MFm)
  FIA_CAND_CASE(FIA_MODEL_MF, 128, MFm)
  FIA_CAND_CASE(FIA_MODEL_MF, 256, MFm)
  FIA_CAND_CASE(FIA_MODEL_NCF, 8, NCFm)
  FIA_CAND_CASE(FIA_MODEL_NCF, 16, NCFm)
  FIA_CAND_CASE(FIA_MODEL_NCF, 32, NCFm)
  FIA_CAND_CASE(FIA_MODEL_NCF, 64, NCFm)
  FIA_CAND_CASE(FIA_MODEL_NCF, 128, NCFm)
  FIA_CAND_CASE(FIA_MODEL_NCF, 256, NCFm)
#undef FIA_CAND_CASE
  unsupported = true;
  return hipSuccess;
}

}  // namespace fia
