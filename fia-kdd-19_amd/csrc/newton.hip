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
// Kernels (k_newton_query, the record layout and ldlt_resolve are in newton.h, shared with
// cand_newton.hip's added ratings):
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
#include "newton.h"

namespace fia {
namespace {

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
