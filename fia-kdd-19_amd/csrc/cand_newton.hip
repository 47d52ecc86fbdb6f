// fia_score_candidates_newton: the Newton-corrected influence of HYPOTHETICAL ratings
// (include/fia.h) -- fia_score_candidates with the candidate's own curvature in the system.  For
// query q = (u, i) with n related ratings and a candidate c = (a, b, y)
//
//   newton_add[c] = v . (H + H_c)^-1 b_c,   H_c = (1/n) (2 g_c g_c^T + 2 e_c C [both] + wd diag(M)),
//                                           b_c = (1/n) (2 e_c g_c + wd M theta_t)
//
// and for every candidate that is not the query's own pair the update is rank one plus a shift that
// is the same for every candidate of the query (fia_query_batch_newton's closed form with the signs
// of an ADDED rating):
//
//   H" = H + (wd/n) diag(M),  c = 2/n,  x" = H"^-1 v,  w" = H"^-1 (wd M theta_t)/n,  c" = x" . (wd M theta_t)/n
//   s = x" . g_c,  t = w" . g_c,  h = g_c^T H"^-1 g_c
//   newton_add = 2 e_c s / n + c" - c s (2 e_c h / n + t) / (1 + c h)                (Sherman-Morrison)
//
// 1 + c h may be negative (H is indefinite through the 2 e C term of a coupled query): nothing takes
// its root or assumes its sign.  A candidate has no list position, so e_c and g_c come from the
// parameter tables and the dense NCF layer-1 rows, as in fia_score_candidates.
//
// Kernels (newton.h: the record, k_newton_query):
//   k_cand_newton_classify  a candidate per thread, the whole batch: its query (a search of the
//                   offsets), its class and sort key -- 2 q + side for a candidate on one side of
//                   its query, then `neither`, `both`, `NaN` (a bad id, a query with n_q = 0 or ids
//                   out of range: NaN stored here) -- and the `both` list (an integer atomic; its
//                   order decides nothing)
//   (rocprim)       one stable radix sort of the (key, candidate) pairs: the candidates of a
//                   (query, side) become consecutive, so a tile of 16 shares one P_ss
//   k_cand_newton_segments  the first sorted position of every key
//   k_newton_query<NewtonAdd<M>>  per launch of a chunk of queries: the record of H" (NCF: in d1
//                   coordinates at every size, P~ = T^T P T -- so W1_side d1_c is never formed)
//   k_cand_newton_score  one wave per 256 sorted positions of the launch's queries, walking the
//                   (query, side) segments inside them in tiles of 16: Y^T = P_ss G^T on
//                   v_mfma_f64_16x16x4_f64 and h, s, t from the C / B registers exactly as
//                   k_newton_score forms them.  MF: B is the candidate's other-side row, the bias
//                   coordinate apart, e_c from the tables.  NCF: the four lanes of a candidate
//                   share its MLP forward -- z1 from the layer-1 rows, z2, the two ReLU masks,
//                   r-hat -- and d1_c at the lane's coordinates (k <= 16: the d1 table row of the
//                   z2 mask; k = 32: W2 d2 from LDS).  The value goes to the candidate's own position
//   k_cand_newton_neither  per launch: c" of the record to the candidates sharing neither side
//   k_cand_newton_both  one wave per `both` candidate: H again, + (2/n) v v^T + (2 e_c / n) C +
//                   (wd/n) diag(M) (remove_member with the member's weight negated), ldlt_solve on
//                   b_c, the dot with v
//   k_cand_newton_topk + k_cand_merge  one wave per tile of 256 positions of the whole batch selects
//                   per (tile, query) segment, four values per lane as k_newton_score's chunks do;
//                   then the per-query merge of fia_score_candidates
// No floating-point atomics.  A candidate's value depends on (query, a, b, y) alone: a column of
// the MFMA tile is computed from its own B column, whatever the other fifteen hold, so the bits are
// the same wherever the candidate sits in its list, wherever the query sits in the batch, whatever
// else is listed and however the batch is cut into launches.
#include <rocprim/device/device_radix_sort.hpp>

#include "cand.h"
#include "newton.h"

namespace fia {
namespace {

constexpr int kCnTile = 256;          // sorted positions per scoring wave

struct CnArgs {
  int64_t Q, total;                   // the whole batch
  const int64_t* off;                 // [Q + 1]
  const int32_t* cu;
  const int32_t* ci;
  const float* cy;
  uint32_t* key_in;                   // [total] by candidate (kept: k_cand_newton_neither reads it)
  uint32_t* key;                      // [total] sorted
  int32_t* idx_in;                    // [total] candidate
  int32_t* idx;                       // [total] candidate by sorted position
  int32_t* seg;                       // [2Q + 2] first sorted position of key k; seg[2Q]: side candidates
  int32_t* both;                      // {count, -, candidate ...}
  double* val;                        // [total]
};

// keys past the (query, side) pairs 2 q + side
__host__ __device__ inline uint32_t cn_neither(int64_t Q) { return (uint32_t)(2 * Q); }
__host__ __device__ inline uint32_t cn_both(int64_t Q) { return (uint32_t)(2 * Q + 1); }
__host__ __device__ inline uint32_t cn_nan(int64_t Q) { return (uint32_t)(2 * Q + 2); }

__global__ __launch_bounds__(256) void k_cand_newton_classify(QueryArgs A, CnArgs C) {
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < C.total; g += (int64_t)gridDim.x * 256) {
    const int64_t q = last_at_most(C.off, (int64_t)0, C.Q - 1, g);
    const int32_t u = A.qu[q], i = A.qi[q];
    const int32_t a = C.cu[g], b = C.ci[g];
    // an id outside [0, U) x [0, I) is never used as an index
    const bool valid = a >= 0 && a < A.U && b >= 0 && b < A.I;
    uint32_t key;
    if (!valid || related_count(A, u, i) == 0) {
      key = cn_nan(C.Q);
      C.val[g] = NAN;
    } else if (a == u && b == i) {
      key = cn_both(C.Q);
      C.both[2 + atomicAdd(C.both, 1)] = (int32_t)g;
    } else if (a == u) {
      key = (uint32_t)(2 * q);
    } else if (b == i) {
      key = (uint32_t)(2 * q + 1);
    } else {
      key = cn_neither(C.Q);
    }
    C.key_in[g] = key;
    C.idx_in[g] = (int32_t)g;
  }
}

__global__ __launch_bounds__(256) void k_cand_newton_segments(CnArgs C) {
  const int64_t nk = 2 * C.Q + 2;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < nk; k += (int64_t)gridDim.x * 256) {
    int64_t lo = 0, hi = C.total;                     // the first position whose key is >= k
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)C.key[mid] < k) lo = mid + 1; else hi = mid;
    }
    C.seg[k] = (int32_t)lo;
  }
}

// `rec` holds the records of queries [q0, q0 + Qn) (k_newton_query<NewtonAdd<M>>); A.qu / A.qi are
// the whole batch's
template <class M>
__global__ __launch_bounds__(64) void k_cand_newton_score(QueryArgs A, CnArgs C, int64_t q0, int64_t Qn,
                                                          const double* __restrict__ rec) {
  constexpr int K = M::K, Ds = M::Ds, PS = newton_side<M>(), R = newton_rec<M>();
  constexpr int Dm = M::ncf ? 2 * K : K;              // coordinates on the matrix cores (MF: the bias apart)
  constexpr int KS = Dm / 4, RB = (Dm + 15) / 16;     // k-steps; 16-row blocks of P
  constexpr int KQ = K / 4, H2 = K / 2;               // NCF: a lane's MLP coordinates; second-layer units
  static_assert(Dm % 4 == 0, "whole k-steps");
  __shared__ NCFWeights<M::ncf ? K : 2> w;            // NCF: W2, b2, W3 (fp64)
  if constexpr (M::ncf) {
    load_ncf_weights<K>(w, A.t[6], A.t[7], A.t[8]);
    __syncthreads();
  }
  __shared__ double d1s[M::ncf && !mask_path<M>() ? KQ * 64 : 1];   // NCF k = 32: d1 by [coordinate][lane]
  (void)w;
  (void)d1s;
  const int lane = threadIdx.x, kk = lane >> 4, cn = lane & 15;
  const int64_t sb = C.seg[2 * q0], se = C.seg[2 * (q0 + Qn)];
  const int64_t ntile = (se - sb + kCnTile - 1) / kCnTile;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    int64_t p = sb + tile * kCnTile;
    const int64_t tend = p + kCnTile < se ? p + kCnTile : se;
    while (p < tend) {                                // every (query, side) segment of the tile (wave-uniform)
      const uint32_t key = C.key[p];
      const int64_t q = key >> 1;
      const int sd = (int)(key & 1u);
      int64_t send = C.seg[key + 1] < tend ? C.seg[key + 1] : tend;
      if (send <= p) send = p + 1;                    // (never with the sorted keys: still terminates)
      const int32_t u = A.qu[q], i = A.qi[q];
      const double* __restrict__ Rq = rec + (q - q0) * R;
      const double* __restrict__ Ps = Rq + kNwHead + sd * PS;
      const double inv_n = Rq[kNwInvN], cp = Rq[kNwCp], c2 = 2.0 * inv_n;
      // A operand: lane (row cn of block rb, k-group kk) holds P[16 rb + cn][kk + 4 s]; and the
      // lane's coordinates kk + 4 s of x"_s and w"_s
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
      // MF: the bias row of P, the bias entries of x" and w", this side's entity (for e_c)
      double pb[M::ncf ? 1 : KS], es[M::ncf ? 1 : KS];
      double pbb = 0.0, xb = 0.0, wb = 0.0, ebase = 0.0;
      const float* __restrict__ Eo = nullptr;         // MF: the other side's embeddings / biases
      const float* __restrict__ Bo = nullptr;
      if constexpr (!M::ncf) {
        const float* __restrict__ Es = (sd == 0 ? A.t[0] : A.t[1]) + (int64_t)(sd == 0 ? u : i) * K;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          pb[s] = Ps[K * Ds + kk + 4 * s];
          es[s] = (double)Es[kk + 4 * s];
        }
        pbb = Ps[K * Ds + K];
        xb = Ps[Ds * Ds + K];
        wb = Ps[Ds * Ds + Ds + K];
        ebase = (double)(sd == 0 ? A.t[2][u] : A.t[3][i]) + (double)A.t[4][0];
        Eo = sd == 0 ? A.t[1] : A.t[0];
        Bo = sd == 0 ? A.t[3] : A.t[2];
      }
      for (int64_t t0 = p; t0 < send; t0 += 16) {
        const bool pv = t0 + cn < send;               // (the tail tile: columns of zeros)
        const int64_t gi = C.idx[pv ? t0 + cn : p];
        const int32_t a = C.cu[gi], b_id = C.ci[gi];
        const double y = (double)C.cy[gi];
        const int32_t o = sd == 0 ? b_id : a;         // in range: the candidate was classified valid
        // B operand: coordinates kk + 4 s of candidate cn's g_c
        double b[KS];
        double e;
        if constexpr (!M::ncf) {
          const float* __restrict__ Er = Eo + (int64_t)o * K;
          double ep = 0.0;
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            b[s] = (double)Er[kk + 4 * s];
            ep = fma(b[s], es[s], ep);
          }
          e = sum4(ep) + ebase + (double)Bo[o] - y;
        } else {
          // the MLP forward of (a, b), the candidate's four lanes each at coordinates kk + 4 s
          const double* __restrict__ l1u = A.l1[0] + (int64_t)a * K;
          const double* __restrict__ l1i = A.l1[1] + (int64_t)b_id * K;
          // (one coordinate at a time: unrolled, the W2 rows of all of them are in flight at once)
          double z2[H2];
          int m1 = 0;                                 // bit s: z1 > 0 at coordinate kk + 4 s
#pragma unroll
          for (int h = 0; h < H2; ++h) z2[h] = 0.0;
#pragma unroll 1
          for (int s = 0; s < KQ; ++s) {
            const int c = kk + 4 * s;
            const double z1 = l1u[c] + l1i[c] + (double)A.t[5][c];
            const double h1 = z1 > 0.0 ? z1 : 0.0;
            m1 |= z1 > 0.0 ? 1 << s : 0;
#pragma unroll
            for (int h = 0; h < H2; ++h) z2[h] = fma(w.W2[c * H2 + h], h1, z2[h]);
          }
          double rm = 0.0;
          int m2 = 0;
#pragma unroll
          for (int h = 0; h < H2; ++h) {
            z2[h] = sum4(z2[h]) + w.b2[h];
            const bool on = z2[h] > 0.0;
            m2 |= on ? 1 << h : 0;
            rm = fma(on ? w.W3[h] : 0.0, z2[h], rm);
            z2[h] = on ? w.W3[h] : 0.0;               // d2
          }
          const float* __restrict__ Pg = A.t[2] + (int64_t)a * K;
          const float* __restrict__ Qg = A.t[3] + (int64_t)b_id * K;
          // d1 = 1[z1 > 0] (W2 d2) at the lane's coordinates: the record is in d1 coordinates, never
          // W1_side d1.  k = 32: a coordinate at a time through the lane's own LDS words (unrolled,
          // the W2 rows of all eight coordinates are in flight at once and the kernel spills)
          if constexpr (!mask_path<M>()) {
#pragma unroll 1
            for (int s = 0; s < KQ; ++s) {
              const int c = kk + 4 * s;
              double d1 = 0.0;
#pragma unroll
              for (int h = 0; h < H2; ++h) d1 = fma(w.W2[c * H2 + h], z2[h], d1);
              d1s[s * 64 + lane] = (m1 >> s) & 1 ? d1 : 0.0;
            }
          }
          double rg = 0.0;
#pragma unroll
          for (int s = 0; s < KQ; ++s) {
            const int c = kk + 4 * s;
            if constexpr (mask_path<M>()) b[s] = (m1 >> s) & 1 ? A.d1tab[(int64_t)m2 * K + c] : 0.0;
            else b[s] = d1s[s * 64 + lane];
            const double pg = (double)Pg[c], qg = (double)Qg[c], w3g = w.W3[H2 + c];
            rg = fma(w3g * pg, qg, rg);
            b[KQ + s] = w3g * (sd == 0 ? qg : pg);
          }
          e = rm + sum4(rg) + (double)A.t[9][0] - y;
        }
        if (!pv) {
#pragma unroll
          for (int s = 0; s < KS; ++s) b[s] = 0.0;
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
        const double val = 2.0 * e * sj * inv_n + cp - c2 * sj * (2.0 * e * h * inv_n + tj) / (1.0 + c2 * h);
        if (pv && kk == 0) C.val[gi] = val;
      }
      p = send;
    }
  }
}

// the candidates of queries [q0, q0 + Qn) that share neither side: the record's c"
template <class M>
__global__ __launch_bounds__(256) void k_cand_newton_neither(CnArgs C, int64_t q0, int64_t Qn,
                                                             const double* __restrict__ rec) {
  constexpr int R = newton_rec<M>();
  const int64_t cb = C.off[q0] > 0 ? C.off[q0] : 0, ce = C.off[q0 + Qn] < C.total ? C.off[q0 + Qn] : C.total;
  const uint32_t kn = cn_neither(C.Q);
  for (int64_t g = cb + (int64_t)blockIdx.x * 256 + threadIdx.x; g < ce; g += (int64_t)gridDim.x * 256) {
    if (C.key_in[g] != kn) continue;
    const int64_t q = last_at_most(C.off, q0, q0 + Qn - 1, g);
    C.val[g] = rec[(q - q0) * R + kNwCp];
  }
}

template <class M>
__global__ __launch_bounds__(kSolveThreads) void k_cand_newton_both(QueryArgs A, CnArgs C) {
  constexpr int K = M::K, D = M::D, T = D * (D + 1) / 2;
  __shared__ double H[T];
  __shared__ double g[D], th[D], dd[D], ww[D];
  __shared__ double x[D];
  __shared__ double sh[4 * K + 8];
  __shared__ NCFWeights<M::ncf ? K : 2> w;
  __shared__ double sW1[M::ncf ? 2 * K * K : 1];
  __shared__ double sb1[M::ncf ? K : 1];
  const int nb = C.both[0];
  if ((int)blockIdx.x >= nb) return;
  stage_ncf<M>(A, w, sW1, sb1);
  const int lane = threadIdx.x;
  for (int t = blockIdx.x; t < nb; t += gridDim.x) {
    __syncthreads();                                  // the previous solve's reads of H, x and g
    const int64_t gi = C.both[2 + t];
    const int64_t q = last_at_most(C.off, (int64_t)0, C.Q - 1, gi);
    const int32_t u = A.qu[q], i = A.qi[q];
    const int64_t n = related_count(A, u, i);         // > 0: the candidate was classified `both`
    const double rhat = solve_prologue<M, kSolveThreads>(A, u, i, th, g, sh, w, sW1, sb1);
    assemble_hessian<M>(A, u, i, n, rhat, g, H);
    const double e = rhat - (double)C.cy[gi];
    const double mn = 1.0 / (double)n;
    for (int c = lane; c < D; c += kSolveThreads) x[c] = member_rhs<M>(c, g, th, e, mn, A.wd);
    __syncthreads();
    // a member of weight -1: H + (2/n) v v^T + (2 e/n) C + (wd/n) diag(M)
    remove_member<M>(H, g, e, -mn, 0, D, true, w, A.wd);
    __syncthreads();
    ldlt_solve<D>(H, x, dd, ww, 0, D);
    __syncthreads();
    double pt = 0.0;
    for (int c = lane; c < D; c += kSolveThreads) pt += x[c] * g[c];
    pt = wave_sum(pt);
    if (lane == 0) C.val[gi] = pt;
  }
}

// Per tile of kCandTile consecutive candidates of the whole batch, one wave, kScoreRows values per
// lane (k_newton_score's chunk selection: no LDS, no barrier): every (tile, query) segment selects
// its best min(K, length) values into slot tile + q, the slots k_cand_merge reads
__global__ __launch_bounds__(64) void k_cand_newton_topk(int64_t Q, int64_t total, const int64_t* __restrict__ off,
                                                         const double* __restrict__ val, int K,
                                                         int32_t* __restrict__ cand_pos,
                                                         double* __restrict__ cand_val) {
  static_assert(kCandTile == 64 * kScoreRows, "a tile is one wave's chunk");
  const int lane = threadIdx.x;
  const int64_t g0 = (int64_t)blockIdx.x * kCandTile;     // < total: the grid is ceil(total / tile)
  const int64_t tile_end = g0 + kCandTile < total ? g0 + kCandTile : total;
  const int nact = (int)(tile_end - g0);
  double v[kScoreRows];
#pragma unroll
  for (int r = 0; r < kScoreRows; ++r) v[r] = 64 * r + lane < nact ? val[g0 + 64 * r + lane] : NAN;
  int64_t q = 0;
  int cur = 0;
  while (cur < nact) {                       // every (tile, query) segment, in batch order (wave-uniform)
    q = last_at_most(off, q, Q - 1, g0 + cur);
    const int64_t qb = off[q], qe = off[q + 1];
    int end = (int)((qe < tile_end ? qe : tile_end) - g0);
    if (end <= cur) end = cur + 1;           // (offsets that are not monotone: still terminates)
    const int rounds = K < end - cur ? K : end - cur;
    double ca[kScoreRows];
    int cp[kScoreRows];
#pragma unroll
    for (int r = 0; r < kScoreRows; ++r) {
      const int idx = 64 * r + lane;
      const bool mine = idx >= cur && idx < end;
      ca[r] = mine ? topk_key(v[r]) : -2.0;
      cp[r] = mine ? (int)(g0 + idx - qb) : -1;
    }
    const int64_t slot = ((int64_t)blockIdx.x + q) * K;
    block_topk<kScoreRows, 64>(ca, cp, v, rounds, cand_pos + slot, cand_val + slot, nullptr, nullptr, nullptr);
    for (int t = rounds + lane; t < K; t += 64) {
      cand_pos[slot + t] = -1;
      cand_val[slot + t] = NAN;
    }
    cur = end;
  }
}

unsigned cn_key_bits(int64_t Q) {
  unsigned bits = 1;
  while (bits < 32 && ((uint64_t)1 << bits) <= (uint64_t)(2 * Q + 2)) ++bits;
  return bits;
}

template <class M>
hipError_t cand_newton_impl(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* off,
                            int64_t total, const int32_t* cu, const int32_t* ci, const float* cy, double* newton_add,
                            int K, int64_t* topk_pos, double* topk_val, hipStream_t s) {
  constexpr int64_t R = newton_rec<M>();
  const int64_t tiles = (total + kCandTile - 1) / kCandTile;
  if (K > 0) {
    FIA_HIP_TRY(c->cand_pos.reserve(sizeof(int32_t) * (size_t)((tiles + Q) * K), s));
    FIA_HIP_TRY(c->cand_val.reserve(sizeof(double) * (size_t)((tiles + Q) * K), s));
  }
  double* val = newton_add;
  if (!val && total > 0) {                            // the values of a top-K-only call
    FIA_HIP_TRY(c->gxq.reserve(sizeof(double) * (size_t)total, s));
    val = c->gxq.as<double>();
  }
  if (total > 0) {
    // the records of a launch: at most 1 GiB of context scratch
    int64_t qc = ((int64_t)1 << 30) / (8 * R);
    qc = newton_chunk_knob(qc < 1 ? 1 : qc);
    if (qc > Q) qc = Q;
    FIA_HIP_TRY(c->rec.reserve(sizeof(double) * (size_t)(qc * R), s));
    FIA_HIP_TRY(c->tkeys.reserve(sizeof(uint32_t) * (size_t)(2 * total), s));
    FIA_HIP_TRY(c->tvals.reserve(sizeof(int32_t) * (size_t)(2 * total), s));
    FIA_HIP_TRY(c->tslot.reserve(sizeof(int32_t) * (size_t)(2 * Q + 2), s));
    FIA_HIP_TRY(c->tword.reserve(sizeof(int32_t) * (size_t)(total + 2), s));
    CnArgs C{};
    C.Q = Q;
    C.total = total;
    C.off = off;
    C.cu = cu;
    C.ci = ci;
    C.cy = cy;
    C.key = c->tkeys.as<uint32_t>();
    C.key_in = C.key + total;
    C.idx = c->tvals.as<int32_t>();
    C.idx_in = C.idx + total;
    C.seg = c->tslot.as<int32_t>();
    C.both = c->tword.as<int32_t>();
    C.val = val;
    const unsigned bits = cn_key_bits(Q);
    size_t tb = 0;
    FIA_HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, C.key_in, C.key, C.idx_in, C.idx, (size_t)total, 0u, bits, s));
    FIA_HIP_TRY(c->tsort.reserve(tb + 16, s));
    tb = c->tsort.bytes;
    const double* d1tab = nullptr;
    if constexpr (mask_path<M>()) {
      constexpr int NT = (1 << (M::K / 2)) * M::K;
      FIA_HIP_TRY(c->d1tab.reserve(sizeof(double) * NT, s));
      hipLaunchKernelGGL(k_newton_d1_table<M>, dim3((unsigned)((NT + 255) / 256)), dim3(256), 0, s, c->p.t[6],
                         c->p.t[8], c->d1tab.as<double>());
      FIA_HIP_TRY(hipGetLastError());
      d1tab = c->d1tab.as<double>();
    }
    const int64_t cus = c->num_cus > 0 ? c->num_cus : 256;
    const int64_t cap = solve_grid_cap(c, newton_lds_bytes<M>());
    auto grid = [](int64_t items, int64_t per, int64_t most) {
      const int64_t g = (items + per - 1) / per;
      return dim3((unsigned)(g < 1 ? 1 : (g < most ? g : most)));
    };
    QueryArgs A = make_args(c, qu, qi);               // the whole batch's queries
    A.d1tab = d1tab;
    // ---- the partition (phase 4) ----
    phase_begin(c, 4, s);
    FIA_HIP_TRY(hipMemsetAsync(C.both, 0, 2 * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_cand_newton_classify, grid(total, 256, cus * 32), dim3(256), 0, s, A, C);
    FIA_HIP_TRY(hipGetLastError());
    FIA_HIP_TRY(rocprim::radix_sort_pairs(c->tsort.ptr, tb, C.key_in, C.key, C.idx_in, C.idx, (size_t)total, 0u, bits, s));
    hipLaunchKernelGGL(k_cand_newton_segments, grid(2 * Q + 2, 256, cus * 32), dim3(256), 0, s, C);
    FIA_HIP_TRY(hipGetLastError());
    phase_end(c, 4, s);
    // ---- the `both` candidates, a full solve each (phase 0) ----
    phase_begin(c, 0, s);
    hipLaunchKernelGGL(k_cand_newton_both<M>, grid(total, 1, cap), dim3(kSolveThreads), 0, s, A, C);
    FIA_HIP_TRY(hipGetLastError());
    phase_end(c, 0, s);
    for (int64_t q0 = 0; q0 < Q; q0 += qc) {
      const int64_t Qn = Q - q0 < qc ? Q - q0 : qc;
      QueryArgs Aq = make_args(c, qu + q0, qi + q0);
      NewtonArgs Nw{};
      Nw.Q = Qn;
      Nw.rec = c->rec.as<double>();
      phase_begin(c, 1, s);
      hipLaunchKernelGGL(k_newton_query<NewtonAdd<M>>, dim3((unsigned)(Qn < cap ? Qn : cap)), dim3(kSolveThreads), 0, s,
                         Aq, Nw);
      FIA_HIP_TRY(hipGetLastError());
      phase_end(c, 1, s);
      phase_begin(c, 2, s);
      hipLaunchKernelGGL(k_cand_newton_score<M>, grid(total, kCnTile, cus * 16), dim3(64), 0, s, A, C, q0, Qn,
                         Nw.rec);
      FIA_HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_cand_newton_neither<M>, grid(total, 256, cus * 32), dim3(256), 0, s, C, q0, Qn, Nw.rec);
      FIA_HIP_TRY(hipGetLastError());
      phase_end(c, 2, s);
    }
  }
  if (K > 0) {
    phase_begin(c, 3, s);
    if (total > 0) {
      hipLaunchKernelGGL(k_cand_newton_topk, dim3((unsigned)tiles), dim3(64), 0, s, Q, total, off, val, K,
                         c->cand_pos.as<int32_t>(), c->cand_val.as<double>());
      FIA_HIP_TRY(hipGetLastError());
    }
    FIA_HIP_TRY(launch_cand_merge(c, Q, total, off, K, topk_pos, topk_val, s));
    phase_end(c, 3, s);
  }
  return hipSuccess;
}

}  // namespace

hipError_t score_candidates_newton(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi,
                                   const int64_t* cand_offsets, int64_t total_cand, const int32_t* cand_user,
                                   const int32_t* cand_item, const float* cand_rating, double* newton_add, int K,
                                   int64_t* topk_pos, double* topk_val, hipStream_t s) {
  hipError_t e = hipErrorInvalidValue;                // (newton_supported is checked by the caller)
  dispatch_small(c->p.model, c->p.k, [&](auto m) {
    e = cand_newton_impl<decltype(m)>(c, Q, qu, qi, cand_offsets, total_cand, cand_user, cand_item, cand_rating,
                                      newton_add, K, topk_pos, topk_val, s);
  });
  return e;
}

}  // namespace fia
