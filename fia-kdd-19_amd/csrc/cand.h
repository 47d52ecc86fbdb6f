// Pair scoring from the parameter tables, shared by score_cand.hip (fia_score_candidates) and
// total.hip (fia_total_influence): r-hat(a, b) and x . d r-hat(a, b) / d theta for an arbitrary
// pair (a, b), with no use of the per-list-position caches -- the parameter tables and, NCF,
// the dense per-entity layer-1 rows l1 (which every prepare writes for ALL entities).
//
//   query_record  per query, once: 1 / n_q and c_q = x_q . (wd M theta_t) / n_q; NCF also
//                 y_side = W1_side^T x_mlp (the k_ncf_rec_y identity
//                 x_mlp . (W1_side d1) = y_side . d1) and W3g * x_gmf
//   coop_dots     the three k-long dots of a pair, rows gathered cooperatively
//   stage_z1 / cand_core_ncf   the NCF MLP forward and y . d1
// `Args` is any struct with the members of ModelArgs (common.h): the tables t[10], the list
// pointers ptr[2], l1[2] and wd.
#pragma once

#include "kern.h"

namespace fia {

constexpr int kCandTile = 256;        // pairs per scoring workgroup, one per thread

// The record query_record writes per query and the pair-scoring kernels of score_cand.hip and
// total.hip read (in c->rec, but not the scoring record of kern.h).  Offsets in doubles.
struct CandHead {
  static constexpr int inv_n = 0;                 // 1 / n_q
  static constexpr int c_q = 1;                   // wd * x . theta / n_q
  static constexpr int head = 2;                  // MF: the whole record
};
template <int K>
struct CandRecNCF : CandHead {
  static constexpr int y_user = head;             // [K] W1[:k]^T x_Pm
  static constexpr int y_item = head + K;         // [K] W1[k:]^T x_Qm
  static constexpr int w3g_x_pg = head + 2 * K;   // [K] W3g * x_Pg
  static constexpr int w3g_x_qg = head + 3 * K;   // [K] W3g * x_Qg
  static constexpr int size = head + 4 * K;
};
template <class M>
constexpr int cand_rec_size() {
  return M::ncf ? CandRecNCF<M::K>::size : CandHead::head;
}

// The record of query (u, i) (ids in range) with inverse HVP xq (reference theta order), by
// one wave (lane = its lane): Rq[cand_rec_size<M>()].
template <class M, class Args>
__device__ __forceinline__ void query_record(const Args& A, int32_t u, int32_t i, const double* __restrict__ xq,
                                             double* __restrict__ Rq, int lane) {
  constexpr int K = M::K;
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
  part = wave_sum(part);
  const double inv_n = 1.0 / (double)n;     // n_q = 0: inf, and x is NaN
  if (lane == 0) {
    Rq[CandHead::inv_n] = inv_n;
    Rq[CandHead::c_q] = A.wd * part * inv_n;
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
      using L = CandRecNCF<K>;
      Rq[L::y_user + c] = yu;
      Rq[L::y_item + c] = yi;
      Rq[L::w3g_x_pg + c] = (double)W3g[c] * xq[2 * K + c];
      Rq[L::w3g_x_qg + c] = (double)W3g[c] * xq[3 * K + c];
    }
  }
}

// Three dot products over a row pair gathered by pair ids -- r = sum_c [g_c] TA[a][c] TB[b][c],
// su = sum_c xu[c] TB[b][c] (user side on), si = sum_c xi[c] TA[a][c] (item side on) -- for the 64
// pairs of a wave, one per lane, with the rows fetched COOPERATIVELY: a lane reading its
// own two rows touches 64 cache lines per load instruction; here LPC = min(k / 4, 16) lanes
// share a pair, each loading 16-B pieces of its rows (a load instruction covers 64 / LPC
// whole rows), in LPC rounds of 64 / LPC pairs.  The partial sums are added across the LPC
// lanes by an xor butterfly (the same bits in every lane, the same order wherever the pair
// sits) and handed to the pair's own lane.  The whole wave must call this (shuffles);
// lanes without a valid pair load nothing.  xu = xbase + q * XS + XU, xi = xbase + q2 * XS + XI
// (TWO; else q serves both).
template <int K, bool WEIGHTED, int XS, int XU, int XI, bool TWO = false>
__device__ __forceinline__ void coop_dots(bool valid, int32_t a, int32_t b, int q, bool on_u, bool on_i,
                                          const float* __restrict__ TA, const float* __restrict__ TB,
                                          const double* __restrict__ xbase, const float* __restrict__ wgt,
                                          double& r_out, double& su_out, double& si_out, int q2 = 0) {
  constexpr int P = K / 4;                  // 16-B pieces per row
  constexpr int LPC = P < 16 ? P : 16;      // lanes per pair
  constexpr int CPR = 64 / LPC;             // pairs per round
  constexpr int PPL = P / LPC;              // pieces per lane
  const int lane = threadIdx.x & 63, sub = lane % LPC, grp = lane / LPC;
  const int flags = (valid ? 1 : 0) | (on_u ? 2 : 0) | (on_i ? 4 : 0);
  r_out = su_out = si_out = 0.0;
#pragma unroll
  for (int j = 0; j < LPC; ++j) {
    const int src = j * CPR + grp;          // this round's pair of the lane's group
    const int fj = __shfl(flags, src);
    const int32_t aj = __shfl(a, src), bj = __shfl(b, src);
    const int qj = __shfl(q, src);
    int q2j = qj;
    if constexpr (TWO) q2j = __shfl(q2, src);
    double r = 0.0, su = 0.0, si = 0.0;
    if (fj & 1) {
      const float4* __restrict__ PA = reinterpret_cast<const float4*>(TA + (int64_t)aj * K);
      const float4* __restrict__ PB = reinterpret_cast<const float4*>(TB + (int64_t)bj * K);
      const double* __restrict__ xu = xbase + (int64_t)qj * XS + XU;
      const double* __restrict__ xi = xbase + (int64_t)q2j * XS + XI;
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
    const int from = (lane % CPR) * LPC;    // the group that had lane's pair, if this was its round
    const double gr = __shfl(r, from), gu = __shfl(su, from), gi = __shfl(si, from);
    if (lane / CPR == j) {
      r_out = gr;
      su_out = gu;
      si_out = gi;
    }
  }
}

// NCF k <= 32: z1 = l1_user[a] + l1_item[b] + b1 of the tile's pairs staged in LDS,
// unit-major ([c][thread], rows padded by 2), the rows gathered cooperatively as in coop_dots:
// a row is k / 2 16-B pieces, a wave's load instruction covers 128 / k whole rows.  Above
// k = 32 the tile's z1 would not fit beside a second workgroup; each lane reads its own rows.
constexpr int kCandZ1Stride = kCandTile + 2;
template <int K>
constexpr bool cand_stage_z1() { return K <= 32; }

template <int K, class Args>
__device__ __forceinline__ void stage_z1(const Args& A, bool valid, int32_t a, int32_t b, double* __restrict__ z1s) {
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

// NCF MLP of pair (a, b): z1 from the per-entity layer-1 rows; r = W3m . relu(z2) and, with
// y = the matching sides' vectors yu / yi, s = y . d1 with d1 = 1[z1 > 0] (W2 (1[z2 > 0] W3m))
// -- W1 is never touched per pair.  W2 / b2 / W3 come from LDS (fp64) up to k = 64 and from
// wave-uniform global loads above.
template <int K, class Args>
__device__ __forceinline__ void cand_core_ncf(const Args& A, const NCFWeights<(K <= 64 ? K : 2)>& w, int32_t a,
                                              int32_t b, bool on_u, bool on_i, const double* __restrict__ yu,
                                              const double* __restrict__ yi, const double* __restrict__ z1col,
                                              double& r_out, double& s_out) {
  constexpr int H = K / 2;
  constexpr bool lds = K <= 64;
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
  r_out = r;
  s_out = s;
}

}  // namespace fia
