// fia_query_batch_newton: the Newton-corrected influence of EVERY related rating of a test
// prediction (include/fia.h) -- fia_group_influence's `group` for the singleton group {j} of every
// related position, without a solve per rating.  For query q = (u, i) with n related ratings and a
// related row j = (a, b, y) that is not the query's own pair (m_j = 1) the downdate is rank one
// plus a shift that is the same for every rating of the query:
//
//   H' = H - (wd/n) diag(M),  c = 2/n,  x' = H'^-1 v,  w' = H'^-1 (wd M theta_t)/n,  c' = x' . (wd M theta_t)/n
//   s_j = x' . g_j,  t_j = w' . g_j,  h_j = g_j^T H'^-1 g_j
//   newton_j = 2 e_j s_j / n + c' + c s_j (2 e_j h_j / n + t_j) / (1 - c h_j)        (Sherman-Morrison)
//
// g_j is nonzero in one side's block only, so h_j needs that side's diagonal block P_ss of the FULL
// inverse H'^-1 (the blocks are coupled when the pair is a train row) and s_j, t_j that side's part
// of x' and w'.  The denominator may be negative (H is indefinite through the 2 e C term of a
// coupled query): nothing takes its root or assumes its sign.  The query's own train rows
// (m_j = 2: coupling block, twice the decay share -- not rank one) get the downdated solve of
// self.hip's pass 1.
//
// Kernels:
//   k_newton_query  persistent one-wave workgroups, one query each (as k_group): prologue, H from
//                   the Gram caches, H' = H - (wd/n) diag(M), LDL^T for x', substitution for w',
//                   L^-1 in place, the two diagonal blocks of Z^T D^-1 Z (Z = L^-1) -- the record
//                   {1/n, c', coupled, -, then per side P_ss [Ds x Ds] full symmetric, x'_s, w'_s}
//                   into context scratch (NCF k <= 16: transformed, below); for a coupled query then every own train row (a
//                   wave-parallel walk of u's list for other == i; its place in i's list by the
//                   ascending train rows): H again, remove_member(own), ldlt_solve on b_j, the dot
//                   with v, written to both of the row's output positions
//   k_newton_score  one wave per chunk of <= kChunk ratings of one side of one query (the plain
//                   chunk descriptors of build_chunks), tiles of 16 ratings: Y^T = P_ss G^T on
//                   v_mfma_f64_16x16x4_f64 (A: 16 rows of P_ss, held in registers for the chunk;
//                   B: the 16 ratings' coordinates) -- lane l's B value of k-step s is coordinate
//                   (l >> 4) + 4 s of rating l & 15 and its C register v row (l >> 4) + 4 v of the
//                   same rating, the same coordinates, so h_j is sum_v C[v] B[v] per lane summed
//                   over the four lanes l, l ^ 16, l ^ 32, l ^ 48: no LDS round trip, no transpose.
//                   MF: the bias coordinate apart (h = q^T P_ee q + 2 q . p_eb + p_bb), e_j from
//                   the tables; NCF: e_j and the MLP gradient from what the Gram pass stored per
//                   list position (k <= 16: d1_j from the ReLU masks, the record in d1 coordinates
//                   -- P~ = T^T P T, x~ = T^T x', w~ = T^T w', T = diag(W1_side, I), formed once per
//                   query by k_newton_query -- so never W1_side d1_j; k = 32: g_mlp as stored,
//                   T = I).  Own-pair positions read k_newton_query's value.
//                   The chunk's values go through LDS to coalesced stores and the chunk top-K, in
//                   the slots k_topk_merge* read.
// No floating-point atomics; a position's value depends on its query and list position alone, so
// the same inputs give the same bits wherever the query sits in the batch and however the batch is
// cut into launches.
#include <cstdlib>

#include "solve.h"

namespace fia {
namespace {

// doubles of one (query, side) block and of one query's record
template <class M>
constexpr int newton_side() { return M::Ds * M::Ds + 2 * M::Ds; }
// a query's record (in c->rec, private to this file): these words, then the two side blocks
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

template <class M>
__global__ __launch_bounds__(kSolveThreads) void k_newton_query(QueryArgs A, NewtonArgs Nw) {
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
    // H' = H - (wd/n) diag(M): the decay share that leaves with any one rating
    for (int a = lane; a < D; a += kSolveThreads)
      H[tri(a, a)] -= (M::decayed(a < Ds ? a : a - Ds) ? A.wd : 0.0) * inv_n;
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
    if constexpr (mask_path<M>()) {
      // NCF k <= 16: the record in the coordinates the scoring pass has per rating.  With
      // T = diag(W1_side, I), g_j = T [d1_j ; W3g * gmf_o], so P~ = T^T P T, x~ = T^T x', w~ = T^T w'
      // serve d1_j as it comes from the stored masks (k_ncf_rec_y's identity on both sides of P).
      // Z is done with: P_ss and Y = P_ss W1_side go through the factor's LDS.
      static_assert(!mask_path<M>() || Ds * Ds + Ds * K <= T, "P_ss and Y fit the packed triangle");
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
    if (!coupled) continue;
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

template <class M>
__global__ __launch_bounds__(64) void k_newton_score(QueryArgs A, NewtonArgs Nw) {
  constexpr int K = M::K, Ds = M::Ds, PS = newton_side<M>(), R = newton_rec<M>();
  constexpr int Dm = M::ncf ? 2 * K : K;              // coordinates on the matrix cores (MF: the bias apart)
  constexpr int KS = Dm / 4, RB = (Dm + 15) / 16;     // k-steps; 16-row blocks of P
  constexpr bool MASK = mask_path<M>();
  static_assert(Dm % 4 == 0, "whole k-steps");
  __shared__ double vals[kChunk];
  __shared__ int32_t rows[kChunk];
  const int lane = threadIdx.x, kk = lane >> 4, cn = lane & 15;
  const int64_t nch = Nw.coff[Nw.Q];
  for (int64_t c = blockIdx.x; c < nch; c += gridDim.x) {
    __syncthreads();                                  // the previous chunk's reads of vals / rows
    const ChunkDesc d = Nw.cdesc[c];
    const int sd = d.side, len = d.len;
    const int64_t q = d.q;
    const int32_t u = A.qu[q], i = A.qi[q];
    const double* __restrict__ Rq = Nw.rec + q * R;
    const double* __restrict__ Ps = Rq + kNwHead + sd * PS;
    const double inv_n = Rq[kNwInvN], cp = Rq[kNwCp], c2 = 2.0 * inv_n;
    const int32_t dup = Rq[kNwCoupled] > 0.0 ? (sd == 0 ? i : u) : -1;
    // A operand: lane (row cn of block rb, k-group kk) holds P[16 rb + cn][kk + 4 s]; and the
    // lane's coordinates kk + 4 s of x'_s and w'_s
    double pa[RB][KS], xs[KS], ws[KS];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int s = 0; s < KS; ++s) pa[rb][s] = 16 * rb + cn < Dm ? Ps[(16 * rb + cn) * Ds + kk + 4 * s] : 0.0;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      xs[s] = Ps[Ds * Ds + kk + 4 * s];
      ws[s] = Ps[Ds * Ds + Ds + kk + 4 * s];
    }
    // MF: the bias row of P, the bias entries of x' and w', this side's entity (for e_j)
    double pb[M::ncf ? 1 : KS], se[M::ncf ? 1 : KS];
    double pbb = 0.0, xb = 0.0, wb = 0.0, ebase = 0.0;
    const float* __restrict__ Eo = nullptr;           // MF: the other side's embeddings / biases
    const float* __restrict__ Bo = nullptr;
    if constexpr (!M::ncf) {
      const float* __restrict__ Es = (sd == 0 ? A.t[0] : A.t[1]) + (int64_t)(sd == 0 ? u : i) * K;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        pb[s] = Ps[K * Ds + kk + 4 * s];
        se[s] = (double)Es[kk + 4 * s];
      }
      pbb = Ps[K * Ds + K];
      xb = Ps[Ds * Ds + K];
      wb = Ps[Ds * Ds + Ds + K];
      ebase = (double)(sd == 0 ? A.t[2][u] : A.t[3][i]) + (double)A.t[4][0];
      Eo = sd == 0 ? A.t[1] : A.t[0];
      Bo = sd == 0 ? A.t[3] : A.t[2];
    }
    const int ntl = (len + 15) / 16;
    for (int t = 0; t < ntl; ++t) {
      const int idx = 16 * t + cn;
      const bool pv = idx < len;
      const int64_t lp = d.list_base + (pv ? idx : 0);
      const int32_t o = A.other[sd][lp];
      // B operand: coordinates kk + 4 s of rating cn's g_j
      double b[KS];
      double e;
      if constexpr (!M::ncf) {
        const float* __restrict__ Er = Eo + (int64_t)o * K;
        double ep = 0.0;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          b[s] = (double)Er[kk + 4 * s];
          ep = fma(b[s], se[s], ep);
        }
        e = sum4(ep) + ebase + (double)Bo[o] - (double)A.rating[sd][lp];
      } else {
        e = A.lres[(int64_t)sd * A.N + lp];
        const float* __restrict__ Gr = (sd == 0 ? A.t[3] : A.t[2]) + (int64_t)o * K;
        if constexpr (MASK) {
          const int32_t mk = reinterpret_cast<const int32_t*>(A.lgm[sd])[lp];
          const double* __restrict__ tr = A.d1tab + (int64_t)((mk >> K) & ((1 << (K / 2)) - 1)) * K;
          // (the record is in d1 coordinates: P~ = T^T P T of k_newton_query, never W1 d1_j)
#pragma unroll
          for (int s = 0; s < K / 4; ++s) b[s] = (mk >> (kk + 4 * s)) & 1 ? tr[kk + 4 * s] : 0.0;
        } else {
#pragma unroll
          for (int s = 0; s < K / 4; ++s) b[s] = A.lgm[sd][(int64_t)(kk + 4 * s) * A.N + lp];
        }
#pragma unroll
        for (int s = 0; s < K / 4; ++s)
          b[K / 4 + s] = (double)A.t[8][K / 2 + kk + 4 * s] * (double)Gr[kk + 4 * s];
      }
      double hp = 0.0, sp = 0.0, tp = 0.0;
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        d4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[rb][s], b[s], acc, 0, 0, 0);
#pragma unroll
        for (int v = 0; v < 4; ++v)
          if (4 * rb + v < KS) hp = fma(acc[v], b[4 * rb + v], hp);
      }
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        if constexpr (!M::ncf) hp = fma(2.0 * pb[s], b[s], hp);
        sp = fma(xs[s], b[s], sp);
        tp = fma(ws[s], b[s], tp);
      }
      const double h = sum4(hp) + pbb, sj = sum4(sp) + xb, tj = sum4(tp) + wb;
      double val = 2.0 * e * sj * inv_n + cp + c2 * sj * (2.0 * e * h * inv_n + tj) / (1.0 - c2 * h);
      if (pv && o == dup) val = Nw.own[d.out_base + idx];       // the query's own train row
      if (pv && kk == 0) {
        vals[idx] = val;
        rows[idx] = A.row[sd][lp];
      }
    }
    __syncthreads();
    double ca[kScoreRows], cv[kScoreRows];
    int cpz[kScoreRows];
#pragma unroll
    for (int r = 0; r < kScoreRows; ++r) {
      const int idx = 64 * r + lane;
      const bool ok = idx < len;
      const double v = ok ? vals[idx] : 0.0;
      if (ok && Nw.newton) Nw.newton[d.out_base + idx] = v;
      if (ok && Nw.rel_idx) Nw.rel_idx[d.out_base + idx] = rows[idx];
      ca[r] = ok ? topk_key(v) : -2.0;
      cpz[r] = ok ? d.pos0 + idx : -1;
      cv[r] = v;
    }
    if (Nw.K > 0)
      block_topk<kScoreRows, 64>(ca, cpz, cv, Nw.K, Nw.cand_pos + c * Nw.K, Nw.cand_val + c * Nw.K, nullptr, nullptr,
                                 nullptr);
  }
}

// FIA_NEWTON_CHUNK (a positive integer): at most that many queries per launch -- a testing knob (a
// small value makes a short batch run in several chunks).  It can only lower the scratch-derived
// bound `dflt`; results do not depend on it
int64_t newton_chunk_knob(int64_t dflt) {
  if (const char* e = std::getenv("FIA_NEWTON_CHUNK")) {
    const long long v = std::atoll(e);
    if (v > 0 && v < dflt) return (int64_t)v;
  }
  return dflt;
}

template <class M>
hipError_t newton_impl(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                       int64_t total_rel, int32_t* rel_idx, double* newton, int K, int64_t* topk_pos,
                       int64_t* topk_idx, double* topk_val, hipStream_t s) {
  constexpr int64_t R = newton_rec<M>();
  // the records of a launch: at most 1 GiB of context scratch
  int64_t qc = ((int64_t)1 << 30) / (8 * R);
  qc = newton_chunk_knob(qc < 1 ? 1 : qc);
  if (qc > Q) qc = Q;
  const int64_t max_chunks = 2 * qc + total_rel / kChunk + 1;
  FIA_HIP_TRY(c->rec.reserve(sizeof(double) * (size_t)(qc * R), s));
  if (K > 0) {
    FIA_HIP_TRY(c->cand_pos.reserve(sizeof(int32_t) * (size_t)((max_chunks + 1) * K), s));
    FIA_HIP_TRY(c->cand_val.reserve(sizeof(double) * (size_t)((max_chunks + 1) * K), s));
  }
  double* own = newton;
  if (!own) {                                         // the own-pair values of a top-K-only call
    FIA_HIP_TRY(c->gxq.reserve(sizeof(double) * (size_t)(total_rel > 0 ? total_rel : 1), s));
    own = c->gxq.as<double>();
  }
  const double* d1tab = nullptr;
  if constexpr (mask_path<M>()) {
    constexpr int NT = (1 << (M::K / 2)) * M::K;
    FIA_HIP_TRY(c->d1tab.reserve(sizeof(double) * NT, s));
    hipLaunchKernelGGL(k_newton_d1_table<M>, dim3((unsigned)((NT + 255) / 256)), dim3(256), 0, s, c->p.t[6], c->p.t[8],
                       c->d1tab.as<double>());
    FIA_HIP_TRY(hipGetLastError());
    d1tab = c->d1tab.as<double>();
  }
  const int64_t cap = solve_grid_cap(c, newton_lds_bytes<M>());
  const int64_t scap = (int64_t)(c->num_cus > 0 ? c->num_cus : 256) * 16;
  for (int64_t q0 = 0; q0 < Q; q0 += qc) {
    const int64_t Qn = Q - q0 < qc ? Q - q0 : qc;
    phase_begin(c, 4, s);
    FIA_HIP_TRY(build_chunks(c, Qn, qu + q0, qi + q0, offsets + q0, max_chunks, false, s));
    phase_end(c, 4, s);
    QueryArgs A = make_args(c, qu + q0, qi + q0);
    A.d1tab = d1tab;
    NewtonArgs Nw{};
    Nw.Q = Qn;
    Nw.offsets = offsets + q0;
    Nw.cdesc = c->cdesc.as<ChunkDesc>();
    Nw.coff = c->coff.as<int64_t>();
    Nw.rec = c->rec.as<double>();
    Nw.own = own;
    Nw.rel_idx = rel_idx;
    Nw.newton = newton;
    Nw.K = K;
    Nw.cand_pos = c->cand_pos.as<int32_t>();
    Nw.cand_val = c->cand_val.as<double>();
    phase_begin(c, 1, s);
    hipLaunchKernelGGL(k_newton_query<M>, dim3((unsigned)(Qn < cap ? Qn : cap)), dim3(kSolveThreads), 0, s, A, Nw);
    FIA_HIP_TRY(hipGetLastError());
    phase_end(c, 1, s);
    phase_begin(c, 2, s);
    hipLaunchKernelGGL(k_newton_score<M>, dim3((unsigned)(max_chunks < scap ? max_chunks : scap)), dim3(64), 0, s, A,
                       Nw);
    FIA_HIP_TRY(hipGetLastError());
    phase_end(c, 2, s);
    if (K > 0) {
      phase_begin(c, 3, s);
      FIA_HIP_TRY(launch_topk_merge(c, Qn, qu + q0, qi + q0, K, 1, topk_pos + q0 * K, topk_idx + q0 * K,
                                    topk_val + q0 * K, s, max_chunks));
      phase_end(c, 3, s);
    }
  }
  return hipSuccess;
}

}  // namespace

bool newton_supported(int model, int k) {
  return dispatch_small(model, k, [](auto) {});
}

hipError_t query_newton(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                        int64_t total_rel, int32_t* rel_idx, double* newton, int K, int64_t* topk_pos,
                        int64_t* topk_idx, double* topk_val, hipStream_t s) {
  hipError_t e = hipErrorInvalidValue;                // (newton_supported is checked by the caller)
  dispatch_small(c->p.model, c->p.k, [&](auto m) {
    e = newton_impl<decltype(m)>(c, Q, qu, qi, offsets, total_rel, rel_idx, newton, K, topk_pos, topk_idx, topk_val,
                                 s);
  });
  return e;
}

}  // namespace fia
