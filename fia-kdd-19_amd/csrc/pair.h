// Device code of the three-block pair system (theta_u, theta_i, theta_j), shared by pair.hip
// (fia_pair_batch) and flip.hip (fia_pair_flip): which sizes are built, the two half records per
// query that k_pair_solve hands to the scoring kernels, the coordinate order of the outputs and the
// LDS of one solve workgroup (pair.hip's header has the formulas).  pair_assemble and
// pair_gap_gradient are k_pair_solve's assembly of the packed D3 triangle and of v as device
// functions, for k_flip_newton; k_pair_solve keeps the loops in its own body, because calling the
// functions there renumbered registers in all five of its instantiations.
#pragma once

#include "cand.h"
#include "solve.h"

namespace fia {

// The sizes whose packed D3 triangle, vectors and (NCF) staged W1 fit one workgroup's LDS
template <class M>
constexpr bool pair_built() {
  return M::ncf ? M::K <= 16 : M::K <= 32;
}

// The scoring record k_pair_solve writes and k_pair_score reads: two HALVES per query, 2 q for
// (user, item i) and 2 q + 1 for item j, so that coop_dots (cand.h) picks the item block of a
// position by the half's index.  MF: the layout below; NCF: CandRecNCF of cand.h.  The head
// (1 / n, c_q) and the user entries are those of half 0.  Offsets in doubles.
template <int K>
struct PairRecMF : CandHead {
  static constexpr int x_user = head;               // [K] x at p_u
  static constexpr int x_item = head + K;           // [K] x at q_i (half 0) / q_j (half 1)
  static constexpr int x_bias_user = head + 2 * K;
  static constexpr int x_bias_item = head + 2 * K + 1;
  static constexpr int size = head + 2 * K + 2;
};
template <class M>
constexpr int pair_half() {
  return M::ncf ? CandRecNCF<M::K>::size : PairRecMF<M::K>::size;
}

__device__ __forceinline__ bool pair_ids_ok(int32_t u, int32_t i, int32_t j, int64_t U, int64_t I) {
  return u >= 0 && u < U && i >= 0 && i < I && j >= 0 && j < I;
}

// coordinate a of the 3-block order -> the reference theta order, extended:
// MF [p_u, q_i, q_j, b_u, b_i, b_j], NCF [Pm_u, Qm_i, Qm_j, Pg_u, Qg_i, Qg_j]
template <class M>
__device__ __forceinline__ int pair_ref_index(int a) {
  constexpr int K = M::K, Ds = M::Ds;
  const int b = a / Ds, c = a - b * Ds;
  if constexpr (!M::ncf) return c < K ? b * K + c : 3 * K + b;
  else return c < K ? b * K + c : 3 * K + b * K + (c - K);
}

template <class M>
constexpr int64_t pair_lds_bytes() {
  constexpr int64_t K = M::K, D = M::D, D3 = 3 * M::Ds;
  return 8 * (D3 * (D3 + 1) / 2 + 4 * D + 3 * D3 + 4 * K + 8 + (M::ncf ? 2 * K * K + K + K * (K / 2) + 2 * K : 8));
}

// The packed 3-block triangle H of query (u, i, j) (ids in range, i != j, n > 0 related ratings) from
// the three Gram reads and the two pair lookups; gi / gj hold v^i / v^j ([user | item],
// solve_prologue's), rhat_i / rhat_j the two predictions.  One wave (lane = its lane); the caller
// synchronises before reading H.  Returns whether either pair is a train row (then the blocks are
// coupled).
template <class M>
__device__ __forceinline__ bool pair_assemble(const QueryArgs& A, int32_t u, int32_t i, int32_t j, int64_t n,
                                              double rhat_i, double rhat_j, const double* gi, const double* gj,
                                              const NCFWeights<M::ncf ? M::K : 2>& w, double* H, int lane) {
  constexpr int K = M::K, Ds = M::Ds, D3 = 3 * Ds, GS = Ds * (Ds + 1) / 2;
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
  return coupled;
}

// v = d (r-hat(u, i) - r-hat(u, j)) / d theta_t from v^i and v^j
template <class M>
__device__ __forceinline__ void pair_gap_gradient(const double* gi, const double* gj, double* v, int lane) {
  constexpr int Ds = M::Ds;
  for (int a = lane; a < Ds; a += kSolveThreads) {
    v[a] = gi[a] - gj[a];
    v[Ds + a] = gi[Ds + a];
    v[2 * Ds + a] = -gj[Ds + a];
  }
}

}  // namespace fia
