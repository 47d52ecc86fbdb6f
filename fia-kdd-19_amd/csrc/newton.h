// What the two Newton calls share (newton.hip: fia_query_batch_newton, a rating REMOVED;
// cand_newton.hip: fia_score_candidates_newton, a rating ADDED): the per-query record, the kernel
// kernel that writes it -- one factorisation of H -/+ (wd/n) diag(M), the sign a template parameter --
// the second substitution on a factor, the d1 table of the NCF k <= 16 masks and the launch knob.
// Kernel-internal, so in an unnamed namespace like the units that include it (a kernel keeps the
// name it had in newton.hip).
#pragma once

#include <cstdlib>

#include "solve.h"

namespace fia {
namespace {

// doubles of one (query, side) block and of one query's record
template <class M>
constexpr int newton_side() { return M::Ds * M::Ds + 2 * M::Ds; }
// a query's record (in c->rec, private to the two units): these words, then the two side blocks
constexpr int kNwInvN = 0, kNwCp = 1, kNwCoupled = 2, kNwPad = 3, kNwHead = 4;
template <class M>
constexpr int newton_rec() { return kNwHead + 2 * newton_side<M>(); }

struct NewtonArgs {
  int64_t Q;
  const int64_t* offsets;    // [Q + 1] of this launch's queries (absolute output positions)
  const ChunkDesc* cdesc;    // plain chunks of this launch's queries
  const int64_t* coff;       // [Q + 1] chunk offsets; coff[Q] = chunks
  double* rec;               // [Q * newton_rec]
  double* own;               // own-pair values by output position: `newton`, or scratch without it
  int32_t* rel_idx;          // nullable
  double* newton;            // nullable
  int K;
  int32_t* cand_pos;
  double* cand_val;
};

// L D L^T x = v with the factor ldlt_solve left in H / d (its substitutions alone)
template <int D>
__device__ void ldlt_resolve(const double* H, double* v, const double* d) {
  const int lane = threadIdx.x;
  for (int j = 0; j < D; ++j) {
    const double yj = v[j];
    for (int r = j + 1 + lane; r < D; r += kSolveThreads) v[r] = fma(-H[tri(r, j)], yj, v[r]);
    __syncthreads();
  }
  for (int j = lane; j < D; j += kSolveThreads) v[j] /= d[j];
  __syncthreads();
  for (int j = D - 1; j >= 0; --j) {
    const double xj = v[j];
    const double* Lj = H + tri(j, 0);
    for (int c = lane; c < j; c += kSolveThreads) v[c] = fma(-Lj[c], xj, v[c]);
    __syncthreads();
  }
}

// NCF k <= 16: the d1 table of the stored ReLU masks (as fia_query_batch builds it per call)
template <class M>
__global__ __launch_bounds__(256) void k_newton_d1_table(const float* __restrict__ W2, const float* __restrict__ W3,
                                                         double* __restrict__ tab) {
  constexpr int K = M::K, H = K / 2;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= (1 << H) * K) return;
  const int m2 = t / K, c = t - m2 * K;
  double v = 0.0;
#pragma unroll
  for (int e = 0; e < H; ++e) v = fma((double)W2[c * H + e], (m2 >> e) & 1 ? (double)W3[e] : 0.0, v);
  tab[t] = v;
}

template <class M>
constexpr int64_t newton_lds_bytes() {
  constexpr int64_t K = M::K, D = M::D;
  return 8 * (D * (D + 1) / 2 + 6 * D + 4 * K + 8 + (M::ncf ? 2 * K * K + K + K * (K / 2) + 2 * K : 8));
}

// The sign of the shift rides in the model type: NewtonAdd<M> is M with `adds` set, so the kernel
// of the plain M is the very function it was before the sign existed.
template <class M>
struct NewtonAdd : M {
  static constexpr bool adds = true;
};
template <class M, class = void>
struct newton_adds { static constexpr bool value = false; };
template <class M>
struct newton_adds<M, decltype((void)M::adds)> { static constexpr bool value = true; };

// The per-query kernel: persistent one-wave workgroups, one query each.  M a model
// (fia_query_batch_newton): the record of H' = H - (wd/n) diag(M), then the own train rows of a
// coupled query.  M = NewtonAdd<model> (fia_score_candidates_newton): the record of
// H" = H + (wd/n) diag(M) alone, and in d1 coordinates at every NCF size (a candidate has no stored
// g_mlp, only its masks).
template <class M>
__global__ __launch_bounds__(kSolveThreads) void k_newton_query(QueryArgs A, NewtonArgs Nw) {
  constexpr bool ADD = newton_adds<M>::value;
  constexpr int K = M::K, Ds = M::Ds, D = M::D, T = D * (D + 1) / 2, PS = newton_side<M>(), R = newton_rec<M>();
  __shared__ double H[T];
  __shared__ double g[D], th[D], dd[D], ww[D];
  __shared__ double x[D], wv[D];
  __shared__ double sh[4 * K + 8];
  __shared__ NCFWeights<M::ncf ? K : 2> w;
  __shared__ double sW1[M::ncf ? 2 * K * K : 1];
  __shared__ double sb1[M::ncf ? K : 1];
  stage_ncf<M>(A, w, sW1, sb1);
  const int lane = threadIdx.x;
  for (int64_t q = blockIdx.x; q < Nw.Q; q += gridDim.x) {
    __syncthreads();
    const int32_t u = A.qu[q], i = A.qi[q];
    const int64_t n = related_count(A, u, i);
    if (n == 0) continue;                             // no chunk reads its record
    const double rhat = solve_prologue<M, kSolveThreads>(A, u, i, th, g, sh, w, sW1, sb1);
    const bool coupled = assemble_hessian<M>(A, u, i, n, rhat, g, H);
    const double inv_n = 1.0 / (double)n;
    for (int a = lane; a < D; a += kSolveThreads) {
      x[a] = g[a];
      wv[a] = (M::decayed(a < Ds ? a : a - Ds) ? A.wd : 0.0) * th[a] * inv_n;
    }
    __syncthreads();
    // H' = H - (wd/n) diag(M): the decay share that leaves with any one rating (ADD: that comes
    // with one)
    for (int a = lane; a < D; a += kSolveThreads) {
      if constexpr (ADD) H[tri(a, a)] += (M::decayed(a < Ds ? a : a - Ds) ? A.wd : 0.0) * inv_n;
      else H[tri(a, a)] -= (M::decayed(a < Ds ? a : a - Ds) ? A.wd : 0.0) * inv_n;
    }
    double part = 0.0;
    __syncthreads();
    ldlt_solve<D>(H, x, dd, ww, 0, D);
    __syncthreads();
    for (int a = lane; a < D; a += kSolveThreads) part += x[a] * wv[a];      // (wv: still the right-hand side)
    const double cp = wave_sum(part);
    __syncthreads();
    ldlt_resolve<D>(H, wv, dd);
    // Z = L^-1 in place, column by column from the right: Z[r][j] = -(L[r][j] + sum_{j<c<r} Z[r][c] L[c][j])
    for (int j = D - 2; j >= 0; --j) {
      for (int r = j + 1 + lane; r < D; r += kSolveThreads) ww[r] = H[tri(r, j)];
      __syncthreads();
      for (int r = j + 1 + lane; r < D; r += kSolveThreads) {
        const double* Zr = H + tri(r, 0);
        double t = ww[r];
        for (int c = j + 1; c < r; ++c) t = fma(Zr[c], ww[c], t);
        H[tri(r, j)] = -t;
      }
      __syncthreads();
    }
    for (int a = lane; a < D; a += kSolveThreads) ww[a] = 1.0 / dd[a];
    __syncthreads();
    // the record: header, then per side P_ss = (Z^T D^-1 Z)_ss, x'_s, w'_s
    double* __restrict__ Rq = Nw.rec + q * R;
    if (lane == 0) {
      Rq[kNwInvN] = inv_n;
      Rq[kNwCp] = cp;
      Rq[kNwCoupled] = coupled ? 1.0 : 0.0;
      Rq[kNwPad] = 0.0;
    }
    for (int sd = 0; sd < 2; ++sd) {
      double* __restrict__ Ps = Rq + kNwHead + sd * PS;
      const int o = sd * Ds;
      for (int t = lane; t < Ds * (Ds + 1) / 2; t += kSolveThreads) {
        int a = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
        while (tri(a + 1, 0) <= t) ++a;
        while (tri(a, 0) > t) --a;
        const int b = t - tri(a, 0);                  // b <= a
        const int ra = o + a, rb = o + b;
        // rows r >= ra of columns ra and rb of Z (Z[ra][ra] = 1)
        double p = (ra == rb ? 1.0 : H[tri(ra, rb)]) * ww[ra];
        for (int r = ra + 1; r < D; ++r) p = fma(H[tri(r, ra)] * H[tri(r, rb)], ww[r], p);
        Ps[a * Ds + b] = p;
        Ps[b * Ds + a] = p;
      }
      for (int a = lane; a < Ds; a += kSolveThreads) {
        Ps[Ds * Ds + a] = x[o + a];
        Ps[Ds * Ds + Ds + a] = wv[o + a];
      }
    }
    if constexpr (mask_path<M>() || (ADD && M::ncf)) {
      // NCF k <= 16: the record in the coordinates the scoring pass has per rating.  With
      // T = diag(W1_side, I), g_j = T [d1_j ; W3g * gmf_o], so P~ = T^T P T, x~ = T^T x', w~ = T^T w'
      // serve d1_j as it comes from the stored masks (k_ncf_rec_y's identity on both sides of P).
      // Z is done with: P_ss and Y = P_ss W1_side go through the factor's LDS.
      static_assert(!M::ncf || Ds * Ds + Ds * K <= T, "P_ss and Y fit the packed triangle");
      double* __restrict__ Pl = H;                    // [Ds][Ds]
      double* __restrict__ Yl = H + Ds * Ds;          // [Ds][K]
      for (int sd = 0; sd < 2; ++sd) {
        double* __restrict__ Ps = Rq + kNwHead + sd * PS;
        const double* __restrict__ W = sW1 + sd * K * K;        // W[a][c] = T[a][c], a, c < K
        const int o = sd * Ds;
        __threadfence_block();                        // P_ss as the lanes above stored it
        __syncthreads();
        for (int t = lane; t < Ds * Ds; t += kSolveThreads) Pl[t] = Ps[t];
        __syncthreads();
        for (int t = lane; t < Ds * K; t += kSolveThreads) {
          const int a = t / K, c = t - a * K;
          double y = 0.0;
          for (int a2 = 0; a2 < K; ++a2) y = fma(Pl[a * Ds + a2], W[a2 * K + c], y);
          Yl[t] = y;
        }
        __syncthreads();
        for (int t = lane; t < K * Ds; t += kSolveThreads) {     // rows c < K
          const int c = t / Ds, b = t - c * Ds;
          double p = 0.0;
          for (int a = 0; a < K; ++a) p = fma(W[a * K + c], b < K ? Yl[a * K + b] : Pl[a * Ds + b], p);
          Ps[c * Ds + b] = p;
        }
        for (int t = lane; t < K * K; t += kSolveThreads) {      // rows c >= K, columns b < K
          const int c = K + t / K, b = t % K;
          Ps[c * Ds + b] = Yl[c * K + b];
        }
        for (int c = lane; c < K; c += kSolveThreads) {
          double xt = 0.0, wt = 0.0;
          for (int a = 0; a < K; ++a) {
            xt = fma(W[a * K + c], x[o + a], xt);
            wt = fma(W[a * K + c], wv[o + a], wt);
          }
          Ps[Ds * Ds + c] = xt;
          Ps[Ds * Ds + Ds + c] = wt;
        }
      }
    }
    if (ADD || !coupled) continue;                    // (ADD: a `both` candidate is cand_newton.hip's k_cand_newton_both)
    // ---- the query's own train rows (m_j = 2), k_self's pass 1 per row ----
    const int64_t ub = A.ptr[0][u], du = A.ptr[0][u + 1] - ub;
    const int64_t ib = A.ptr[1][i], di = A.ptr[1][i + 1] - ib;
    const int64_t ob = Nw.offsets[q];
    const double mn = 2.0 * inv_n;                    // m_j / n
    for (int64_t p0 = 0; p0 < du; p0 += kSolveThreads) {
      const int64_t p = p0 + lane;
      unsigned long long hits = __ballot(p < du && A.other[0][ub + (p < du ? p : 0)] == i);
      while (hits) {                                  // (wave-uniform)
        const int64_t pu = p0 + __builtin_ctzll(hits);
        hits &= hits - 1;
        const int32_t row = A.row[0][ub + pu];
        const double e = rhat - (double)A.rating[0][ub + pu];
        // the row's place in i's list: train rows ascend there
        int64_t lo = 0, hi = di - 1;
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (A.row[1][ib + mid] < row) lo = mid + 1; else hi = mid;
        }
        __syncthreads();                              // the previous solve's reads of H and x
        assemble_hessian<M>(A, u, i, n, rhat, g, H);
        for (int c = lane; c < D; c += kSolveThreads) x[c] = member_rhs<M>(c, g, th, e, mn, A.wd);
        __syncthreads();
        remove_member<M>(H, g, e, mn, 0, D, true, w, A.wd);
        __syncthreads();
        ldlt_solve<D>(H, x, dd, ww, 0, D);
        __syncthreads();
        double pt = 0.0;
        for (int c = lane; c < D; c += kSolveThreads) pt += x[c] * g[c];
        pt = wave_sum(pt);
        if (lane == 0) {
          Nw.own[ob + pu] = pt;
          Nw.own[ob + du + lo] = pt;
        }
      }
    }
  }
}

// the sum over the four lanes that hold one rating's coordinates (l, l ^ 16, l ^ 32, l ^ 48): the
// same bits in all four
__device__ __forceinline__ double sum4(double v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// FIA_NEWTON_CHUNK (a positive integer): at most that many queries per launch -- a testing knob (a
// small value makes a short batch run in several chunks).  It can only lower the scratch-derived
// bound `dflt`; results do not depend on it
inline int64_t newton_chunk_knob(int64_t dflt) {
  if (const char* e = std::getenv("FIA_NEWTON_CHUNK")) {
    const long long v = std::atoll(e);
    if (v > 0 && v < dflt) return (int64_t)v;
  }
  return dflt;
}

}  // namespace
}  // namespace fia
