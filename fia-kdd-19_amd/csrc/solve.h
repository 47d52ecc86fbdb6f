// Device code of the full-D per-query system, shared by small_solve.hip (k_solve, k_record_x and
// the side-system solves' prologue), group.hip (fia_group_influence), self.hip
// (fia_self_influence) and edit.hip (fia_edit_influence): the LDS LDL^T, the
// query prologue (theta_t, v = d r-hat / d theta_t, r-hat of one pair), the assembly of the
// packed coupled Hessian from the two entity Gram caches and the removal of one train row from
// it.  One wave (kSolveThreads) per system unless a function says otherwise.
#pragma once

#include "kern.h"

namespace fia {

// WV = false: the system's wave is a 64-thread workgroup (lane = threadIdx.x, workgroup barriers).
// WV = true: one wave of a larger workgroup on LDS arrays of its own (lane = threadIdx.x & 63,
// wave_lds_sync: a wave's LDS accesses complete in order, the fence keeps the compiler from
// moving them across) -- the same arithmetic in the same order, so the same bits.
template <bool WV>
__device__ __forceinline__ int solve_lane() {
  return WV ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
}
template <bool WV>
__device__ __forceinline__ void solve_sync() {
  if constexpr (WV) wave_lds_sync(); else __syncthreads();
}

// In-place LDL^T of the packed lower block [lo, hi) followed by L D L^T x = v.
template <int D, bool WV = false>
__device__ void ldlt_solve(double* H, double* v, double* d, double* w, int lo, int hi) {
  const int lane = solve_lane<WV>();
  for (int j = lo; j < hi; ++j) {
    for (int c = lo + lane; c < j; c += kSolveThreads) w[c] = H[tri(j, c)] * d[c];
    solve_sync<WV>();
    for (int r = j + lane; r < hi; r += kSolveThreads) {
      const double* Lr = H + tri(r, 0);
      double t = Lr[j];
      for (int c = lo; c < j; ++c) t = fma(-Lr[c], w[c], t);
      if (r == j) d[j] = t; else H[tri(r, j)] = t;
    }
    solve_sync<WV>();
    const double dj = d[j];
    for (int r = j + 1 + lane; r < hi; r += kSolveThreads) H[tri(r, j)] /= dj;
    solve_sync<WV>();
  }
  for (int j = lo; j < hi; ++j) {
    const double yj = v[j];
    for (int r = j + 1 + lane; r < hi; r += kSolveThreads) v[r] = fma(-H[tri(r, j)], yj, v[r]);
    solve_sync<WV>();
  }
  for (int j = lo + lane; j < hi; j += kSolveThreads) v[j] /= d[j];
  solve_sync<WV>();
  for (int j = hi - 1; j >= lo; --j) {
    const double xj = v[j];
    const double* Lj = H + tri(j, 0);
    for (int c = lo + lane; c < j; c += kSolveThreads) v[c] = fma(-Lj[c], xj, v[c]);
    solve_sync<WV>();
  }
}


// theta_t, v = d r(u,i)/d theta_t (gnn:155, mf:194,201 / ncf:222,229) and r-hat(u,i) of one
// query into the workgroup's LDS arrays th[D] / g[D] (NTH threads cooperate; r-hat is
// valid in the first wave)
template <class M, int NTH, bool WV = false>
__device__ double solve_prologue(const QueryArgs& A, int32_t u, int32_t i, double* __restrict__ th,
                                 double* __restrict__ g, double* __restrict__ sh, const NCFWeights<M::ncf ? M::K : 2>& w,
                                 const double* __restrict__ sW1, const double* __restrict__ sb1) {
  constexpr int K = M::K, Ds = M::Ds;
  static_assert(!WV || NTH == 64, "one wave");
  const int lane = solve_lane<WV>();
  double rhat_ui = 0.0;
  if constexpr (!M::ncf) {
    const float* P = A.t[0];
    const float* Qt = A.t[1];
    for (int a = lane; a < K; a += NTH) {
      th[a] = P[(int64_t)u * K + a];
      th[Ds + a] = Qt[(int64_t)i * K + a];
      g[a] = Qt[(int64_t)i * K + a];           // user block of v: q_i
      g[Ds + a] = P[(int64_t)u * K + a];       // item block of v: p_u
    }
    if (lane == 0) {
      th[K] = A.t[2][u];
      th[Ds + K] = A.t[3][i];
      g[K] = 1.0;
      g[Ds + K] = 1.0;
    }
    solve_sync<WV>();
    double part = 0.0;
    for (int a = lane; a < K; a += NTH) part += th[a] * th[Ds + a];
    rhat_ui = wave_sum(part) + th[K] + th[Ds + K] + (double)A.t[4][0];
  } else {
    constexpr int H2 = K / 2;
    const float* Pm = A.t[0];
    const float* Qm = A.t[1];
    const float* Pg = A.t[2];
    const float* Qg = A.t[3];
    double* z1 = sh;            // K
    double* d2 = sh + K;        // K/2
    double* d1 = sh + 2 * K;    // K
    for (int a = lane; a < K; a += NTH) {
      th[a] = Pm[(int64_t)u * K + a];
      th[K + a] = Pg[(int64_t)u * K + a];
      th[Ds + a] = Qm[(int64_t)i * K + a];
      th[Ds + K + a] = Qg[(int64_t)i * K + a];
      z1[a] = A.l1[0][(int64_t)u * K + a] + A.l1[1][(int64_t)i * K + a] + sb1[a];
    }
    solve_sync<WV>();
    double mlp_part = 0.0;
    for (int dd2 = lane; dd2 < H2; dd2 += NTH) {
      double z2 = w.b2[dd2];
      for (int c = 0; c < K; ++c) z2 = fma(w.W2[c * H2 + dd2], z1[c] > 0.0 ? z1[c] : 0.0, z2);
      const bool on = z2 > 0.0;
      d2[dd2] = on ? w.W3[dd2] : 0.0;
      mlp_part += on ? w.W3[dd2] * z2 : 0.0;
    }
    double gmf_part = 0.0;
    for (int a = lane; a < K; a += NTH) gmf_part += w.W3[H2 + a] * th[K + a] * th[Ds + K + a];
    rhat_ui = wave_sum(mlp_part + gmf_part) + (double)A.t[9][0];
    solve_sync<WV>();
    for (int c = lane; c < K; c += NTH) {
      double t = 0.0;
      for (int dd2 = 0; dd2 < H2; ++dd2) t = fma(w.W2[c * H2 + dd2], d2[dd2], t);
      d1[c] = z1[c] > 0.0 ? t : 0.0;
    }
    solve_sync<WV>();
    for (int a = lane; a < 2 * K; a += NTH) {
      // rows a < K: W1[:k] (Pm part, user block); rows a >= K: W1[k:] (Qm part, item block)
      double s = 0.0;
      for (int c = 0; c < K; ++c) s = fma(sW1[a * K + c], d1[c], s);
      if (a < K) g[a] = s; else g[Ds + (a - K)] = s;
    }
    for (int a = lane; a < K; a += NTH) {
      g[K + a] = w.W3[H2 + a] * th[Ds + K + a];        // d r/d Pg_u = W3g * Qg_i
      g[Ds + K + a] = w.W3[H2 + a] * th[K + a];        // d r/d Qg_i = W3g * Pg_u
    }
  }
  solve_sync<WV>();
  return rhat_ui;
}

// The packed lower triangle of the full D x D Hessian of query (u, i) (n related ratings,
// v in g[D], r-hat(u, i) given) from the two entity Gram caches:
//   H = (2/n) (A_u (+) B_i) + the (u, i) train rows' second copies and coupling + wd M + damping I
// One wave; the caller synchronises before reading H.  Returns whether (u, i) is a train
// row (then the user and item blocks are coupled).
template <class M, bool WV = false>
__device__ __forceinline__ bool assemble_hessian(const QueryArgs& A, int32_t u, int32_t i, int64_t n, double rhat_ui,
                                                 const double* __restrict__ g, double* __restrict__ H) {
  constexpr int K = M::K, Ds = M::Ds, D = M::D, GS = Ds * (Ds + 1) / 2;
  const int lane = solve_lane<WV>();
  const double s2n = 2.0 / (double)n;
  // ---- the (u,i) pair among the train rows (pair set built with the index) ----
  double cdup, rsum;
  A.pairs.lookup((unsigned long long)u * (unsigned long long)A.I + (unsigned long long)i, cdup, rsum);
  const bool coupled = cdup > 0.0;
  const double esum = cdup * rhat_ui - rsum;
  const double* Gu = A.gram[0] + (int64_t)u * ((GS + 1) & ~1);
  const double* Gi = A.gram[1] + (int64_t)i * ((GS + 1) & ~1);
  for (int t = lane; t < D * (D + 1) / 2; t += kSolveThreads) {
    int r = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while (tri(r + 1, 0) <= t) ++r;
    while (tri(r, 0) > t) --r;
    const int c = t - tri(r, 0);
    double h = 0.0;
    if (r < Ds) {
      h = s2n * (Gu[gidx<M>(r, c)] + cdup * g[r] * g[c]);
    } else if (c >= Ds) {
      const int rr = r - Ds, cc = c - Ds;
      h = s2n * (Gi[gidx<M>(rr, cc)] + cdup * g[r] * g[c]);
    } else if (coupled) {
      // cross block: item row rr, user col c: 2 (c g_i g_u^T + esum * d2r/dtheta_i dtheta_u)
      const int rr = r - Ds;
      h = s2n * 2.0 * cdup * g[r] * g[c];
      if constexpr (!M::ncf) {
        if (rr == c && c < K) h += s2n * 2.0 * esum;                     // d2 r / dp_u dq_i = I
      } else {
        if (rr == c && c >= K) h += s2n * 2.0 * esum * (double)A.t[8][K / 2 + (c - K)];   // diag(W3g)
      }
    }
    if (r == c) h += (M::decayed(r < Ds ? r : r - Ds) ? A.wd : 0.0) + A.damping;
    H[t] = h;
  }
  return coupled;
}

// Removing train row j = (a, b, y) from the system of a query it is related to (group.hip's
// header): g_j = d r-hat(a, b) / d theta_t with the blocks of a side that does not match the
// query zeroed, e = r-hat(a, b) - y, mn = m_j / n.
//
// H -= the member's three terms on the packed triangle: (2 m_j / n) g_j g_j^T over rows and
// columns [r0, r1) (the blocks where g_j is nonzero); own -- the member is the query's own pair
// -- (2 m_j / n) e_j C_j, the coupling of the user and item blocks; and (m_j / n) wd M.  One
// wave; the caller synchronises before H is read.
template <class M>
__device__ __forceinline__ void remove_member(double* H, const double* gj, double e, double mn, int r0, int r1,
                                              bool own, const NCFWeights<M::ncf ? M::K : 2>& w, double wd) {
  constexpr int K = M::K, Ds = M::Ds, D = M::D;
  const int lane = threadIdx.x;
  const double s2 = 2.0 * mn;
#pragma nounroll
  for (int r = r0; r < r1; ++r) {
    const double gr = s2 * gj[r];
    double* __restrict__ Hr = H + tri(r, 0);
    for (int c = r0 + lane; c <= r; c += kSolveThreads) Hr[c] = fma(-gr, gj[c], Hr[c]);
  }
  // the entries below were other lanes' above: NCF's coupling entry (Ds + K + c, K + c) lane
  // (K + c) % 64's, a diagonal entry (c, c) lane (c - r0) % 64's
  __syncthreads();
  if (own) {
    for (int c = lane; c < K; c += kSolveThreads) {
      if constexpr (!M::ncf) H[tri(Ds + c, c)] -= s2 * e;                         // I on (p_u, q_i)
      else H[tri(Ds + K + c, K + c)] -= s2 * e * w.W3[K / 2 + c];                 // diag(W3g) on (Pg_u, Qg_i)
    }
  }
  for (int c = lane; c < D; c += kSolveThreads) {
    const double dec = M::decayed(c < Ds ? c : c - Ds) ? wd : 0.0;
    H[tri(c, c)] -= mn * dec;
  }
}

// ... and element c of its right-hand-side term (m_j / n) (2 e_j g_j + wd M theta_t)
template <class M>
__device__ __forceinline__ double member_rhs(int c, const double* gj, const double* th, double e, double mn,
                                             double wd) {
  const double dec = M::decayed(c < M::Ds ? c : c - M::Ds) ? wd : 0.0;
  return mn * (2.0 * e * gj[c] + dec * th[c]);
}

// ids in range and related count of query (u, i); 0 for an id out of range (never an index)
__device__ __forceinline__ int64_t related_count(const QueryArgs& A, int32_t u, int32_t i) {
  if (!(u >= 0 && u < A.U && i >= 0 && i < A.I)) return 0;
  return (A.ptr[0][u + 1] - A.ptr[0][u]) + (A.ptr[1][i + 1] - A.ptr[1][i]);
}

// the NCF weights solve_prologue reads, into the workgroup's LDS (once per persistent workgroup)
template <class M>
__device__ __forceinline__ void stage_ncf(const QueryArgs& A, NCFWeights<M::ncf ? M::K : 2>& w, double* sW1,
                                          double* sb1) {
  if constexpr (M::ncf) {
    constexpr int K = M::K;
    load_ncf_weights<K>(w, A.t[6], A.t[7], A.t[8]);
    for (int t = threadIdx.x; t < 2 * K * K; t += blockDim.x) sW1[t] = (double)A.t[4][t];
    for (int t = threadIdx.x; t < K; t += blockDim.x) sb1[t] = (double)A.t[5][t];
  }
}

// ---- host side, shared by group.hip and self.hip ----
// c->rowrec: train row -> {user, item, rating bits, user-major list position}, built once per
// index (group.hip)
hipError_t ensure_rowrec(fia_ctx* c, hipStream_t s);
// group.hip's k_group_x for a caller in another unit (edit.hip): x_q = H^-1 v of the Q queries of
// A with n_q > 0 into xq [Q * D], block order
hipError_t launch_group_x(fia_ctx* c, const QueryArgs& A, int64_t Q, double* xq, hipStream_t s);
// one-wave workgroups of `lds` bytes that the device keeps resident (160 KB of LDS per CU, at most
// 16 per CU: 4 waves per SIMD at <= 128 VGPRs): the grid of a persistent full-D kernel
inline int64_t solve_grid_cap(const fia_ctx* c, int64_t lds) {
  const int64_t fit = 160 * 1024 / lds;
  const int64_t per_cu = fit < 1 ? 1 : (fit > 16 ? 16 : fit);
  return (int64_t)(c->num_cus > 0 ? c->num_cus : 256) * per_cu;
}

}  // namespace fia
