// fia_group_influence and fia_self_influence for the large-k models (MF k in {128, 256},
// NCF k in {64, 128, 256}), whose systems live in device memory (bigk.hip).  For query
// q = (u, i) -- n related ratings, the cached Grams A_u and B_i, cdup train rows equal to
// (u, i) with residual sum esum, v = (v_u, v_i) -- and a group S of train rows, H - H_S is the
// base coupled system of k_big_solve with
//
//   A_u  -> A_u - dA_u,  dA_u = sum_{j in S on u's side} g_ju g_ju^T   (an own-pair listing counts once)
//   B_i  -> B_i - dB_i   likewise
//   cdup -> cdup - c_S   c_S own-pair listings in S (same-side rank-1 terms and the cross block)
//   esum -> esum - e_S   e_S the sum of their residuals (the cross block's C term)
//   wd   -> wd (1 - m_S / n),  m_S = sum_{j in S} m_j;  the damping stays
//
// and, block by block, b_S = (2/n) (sum_{j on the side} e_j g_j + e_S v) + (m_S / n) wd M theta_t
// (tests/test_group_bigk_cpu.py checks both against the definition).  So a group costs two
// Gram-shaped downdates in the cache's own tile layout, four scalars and a right-hand side.
//
// Kernels:
//   k_group_down   one workgroup per group: the members in list order (a row out of range makes
//                  the group bad; m_j = 0 rows are dropped before anything of theirs is read),
//                  compacted per side into a queue; every 16 queued members are staged in LDS as
//                  a slab of gradient rows (MF: the other side's embedding row and the bias 1;
//                  NCF: g_mlp of the row and W3g * the other side's GMF row -- k_big_gram's
//                  operands) and added to dA_u / dB_i on v_mfma_f64_16x16x4_f64, the tail slab
//                  zero-padded; e_j g_j, c_S, e_S and m_S ride along
//   k_self_pairs   fia_self_influence: the implicit query (a, b) of every listed row
//   k_big_down     one workgroup per system, persistent: the downdated coupled system through the
//                  blocked LDL^T of bigk.h, right-hand side b_S; group = v . x, dtheta in the
//                  reference order, first_order = (H^-1 v) . b_S from the per-query solves of
//                  bigk.hip.  A row's own system (fia_self_influence) needs no slab: dA_u = v_u
//                  v_u^T, dB_i = v_i v_i^T, c_S = 1, e_S = e, m_S = 2.
// No floating-point atomics; slab order, k-step order and the member order inside a slab are
// fixed by the compacted list alone, so the same group gives the same bits wherever it sits and
// whatever unrelated rows are listed with it.
#include <cstdlib>

#include "bigk.h"

namespace fia {
namespace {

constexpr int kGdThreads = 512, kGdWaves = kGdThreads / 64;
constexpr int64_t kDownScratch = (int64_t)1 << 30;   // bytes of downdate slabs per launch (group chunks)
constexpr int64_t kSelfChunk = 4096;                 // rows per fia_self_influence chunk (QW words of qwork each)

// per-system words: [status, c_S, e_S, m_S, slab of side 0 written, of side 1, -, -, sum e_j g_ju, sum e_j g_ji]
// status 0: nothing removed (+0.0); 1: solve; 2: NaN (a bad member, n_q = 0, a query id out of range)
template <class M>
constexpr int down_words() { return 8 + 2 * M::NPs; }

template <class M>
constexpr int slab_ld() { return M::NPs % 32 == 0 ? M::NPs + 16 : M::NPs; }

struct DownArgs {
  int64_t n;                 // systems of this launch
  int64_t first;             // group mode: its first group; self mode: its first position
  int64_t Q, TM, N;
  const int64_t* grp_off;    // [Q + 1]; null: self mode (system w is query w of the chunk)
  const int64_t* mem_off;    // [G + 1]
  const int32_t* mem_row;    // [TM]
  const int32_t* rows;       // self mode: [num_rows] or null (position = row)
  const int4* rowrec;        // [N] train row -> {user, item, rating bits, user-major list position}
  const double* qwork;
  const double* xb;          // H^-1 v per query (null: no first_order)
  double* dwork;             // [n * down_words]
  double* slab;              // [n * 2 * gram_words]
  double* lscr;
  double* group;             // self mode: newton
  double* first_order;
  double* dtheta;
  double* error;             // self mode
  int solve;                 // group / dtheta (newton) asked for
};

template <class M>
__global__ __launch_bounds__(kGdThreads) void k_group_down(BigArgs A, DownArgs Dn) {
  constexpr int K = M::K, NPs = M::NPs, T = M::T, NTL = T * (T + 1) / 2, LDG = slab_ld<M>();
  constexpr int64_t GW = gram_words<M>();
  static_assert(NPs <= kGdThreads, "one coordinate per thread");
  __shared__ double Gs[16 * LDG];
  __shared__ double e16[16];
  __shared__ int own16[16];
  __shared__ int32_t qrow[2][kGdThreads + 16];
  __shared__ int wcnt[2][kGdWaves];
  __shared__ int sbad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ml = lane & 15, kl = lane >> 4;
  for (int64_t w = blockIdx.x; w < Dn.n; w += gridDim.x) {
    const int64_t gi = Dn.first + w;
    const int64_t q = last_at_most(Dn.grp_off, (int64_t)0, Dn.Q - 1, gi);
    double* __restrict__ dw = Dn.dwork + w * down_words<M>();
    double* __restrict__ dA[2] = {Dn.slab + w * 2 * GW, Dn.slab + w * 2 * GW + GW};
    const double nq = Dn.qwork[q * M::QW + M::Work::n];
    if (nq == 0.0) {                                  // (the prologue's verdict: ids out of range, no cache, n = 0)
      if (tid == 0) dw[0] = 2.0;
      continue;
    }
    const int32_t u = A.qu[q], i = A.qi[q];
    int64_t m0 = Dn.mem_off[gi], m1 = Dn.mem_off[gi + 1];
    m0 = m0 < 0 ? 0 : m0;                             // (never past the member array)
    m1 = m1 > Dn.TM ? Dn.TM : m1;
    // every value below but `bacc` is the same in all threads
    int cnt[2] = {0, 0}, nslab[2] = {0, 0};
    int64_t mem[2] = {0, 0};
    double cS = 0.0, eS = 0.0;
    double bacc[2] = {0.0, 0.0};                      // coordinate tid of sum e_j g_j, per side
    bool bad = false;
    // one slab: members qrow[sd][off .. off + len), len <= 16, the rest of the slab zero
    auto slab = [&](int sd, int off, int len) {
      {
        const int r = tid >> 5, pp = tid & 31;        // 32 threads per member row
        const bool valid = r < len;
        const int32_t j = valid ? qrow[sd][off + r] : 0;
        int4 rr = make_int4(0, 0, 0, 0);
        if (valid) rr = Dn.rowrec[j];
        const int32_t o = sd == 0 ? rr.y : rr.x;
        if (pp == 0) {
          e16[r] = valid ? A.resid[j] : 0.0;
          own16[r] = valid && sd == 0 && rr.y == i;   // an own-pair listing (counted on the user side)
        }
        double* __restrict__ row = Gs + r * LDG;
        if constexpr (!M::ncf) {
          const float* __restrict__ emb = (sd == 0 ? A.t[1] : A.t[0]) + (int64_t)o * K;
          for (int c = pp; c < NPs; c += 32) row[c] = !valid ? 0.0 : (c < K ? (double)emb[c] : (c == K ? 1.0 : 0.0));
        } else {
          const double* __restrict__ gm = A.gm[sd] + (int64_t)j * K;
          const float* __restrict__ gmf = (sd == 0 ? A.t[3] : A.t[2]) + (int64_t)o * K;
          const float* __restrict__ W3g = A.t[8] + M::H;
          for (int c = pp; c < K; c += 32) {
            row[c] = valid ? gm[c] : 0.0;
            row[K + c] = valid ? (double)W3g[c] * (double)gmf[c] : 0.0;
          }
        }
      }
      __syncthreads();
      if (sd == 0)
        for (int r = 0; r < 16; ++r)
          if (own16[r]) {
            cS += 1.0;
            eS += e16[r];
          }
      if (tid < NPs) {
        double b = bacc[sd];
        for (int r = 0; r < 16; ++r) b = fma(e16[r], Gs[r * LDG + tid], b);
        bacc[sd] = b;
      }
      // rank-16 update of this wave's tiles (idx = tr (tr + 1) / 2 + tc), the running sums in the
      // group's slab: a tile is read and written by the same lanes of the same wave only
      const bool first = nslab[sd] == 0;
      int tr = 0;
      for (int idx = wave; idx < NTL; idx += kGdWaves) {
        while ((tr + 1) * (tr + 2) / 2 <= idx) ++tr;
        const int tc = idx - tr * (tr + 1) / 2;
        double* __restrict__ tb = dA[sd] + (int64_t)tile_off(T, tr, tc) * 256 + 16 * ml + kl;
        d4_t acc = {0.0, 0.0, 0.0, 0.0};
        if (!first) {
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[r] = tb[4 * r];
        }
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          const double* gr = Gs + (4 * s4 + kl) * LDG + ml;
          acc = mfma4(gr[16 * tr], gr[16 * tc], acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) tb[4 * r] = acc[r];
      }
      ++nslab[sd];
      __syncthreads();                                // the next slab rewrites Gs / e16 / own16
    };
    for (int64_t base = m0; base < m1; base += kGdThreads) {
      const int64_t m = base + tid;
      const bool have = m < m1;
      const int32_t row = have ? Dn.mem_row[m] : 0;
      const bool inr = have && row >= 0 && row < Dn.N;    // (a bad row is never used as an index)
      if (tid == 0) sbad = 0;
      __syncthreads();
      if (have && !inr) sbad = 1;
      int4 rr = make_int4(-1, -1, 0, 0);
      if (inr) rr = Dn.rowrec[row];
      const bool on[2] = {inr && rr.x == u, inr && rr.y == i};
      int pre[2];
#pragma unroll
      for (int sd = 0; sd < 2; ++sd) {
        const unsigned long long mask = __ballot(on[sd]);
        pre[sd] = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[sd][wave] = __popcll(mask);
      }
      __syncthreads();
      if (sbad) {
        bad = true;
        break;
      }
#pragma unroll
      for (int sd = 0; sd < 2; ++sd) {
        int before = 0, total = 0;
#pragma unroll
        for (int ww = 0; ww < kGdWaves; ++ww) {
          before += ww < wave ? wcnt[sd][ww] : 0;
          total += wcnt[sd][ww];
        }
        if (on[sd]) qrow[sd][cnt[sd] + before + pre[sd]] = row;
        cnt[sd] += total;
        mem[sd] += total;
      }
      __syncthreads();
      // full slabs now; what is left (< 16 per side) moves to the front of its queue
#pragma unroll 1
      for (int sd = 0; sd < 2; ++sd) {
        int off = 0;
        for (; off + 16 <= cnt[sd]; off += 16) slab(sd, off, 16);
        const int left = cnt[sd] - off;
        if (off > 0) {
          const int32_t keep = tid < left ? qrow[sd][off + tid] : 0;
          __syncthreads();
          if (tid < left) qrow[sd][tid] = keep;
        }
        cnt[sd] = left;
      }
      __syncthreads();
    }
    if (!bad) {
#pragma unroll 1
      for (int sd = 0; sd < 2; ++sd)
        if (cnt[sd] > 0) slab(sd, 0, cnt[sd]);
    }
    __syncthreads();
    const bool none = mem[0] + mem[1] == 0;
    if (tid == 0) {
      dw[0] = bad ? 2.0 : (none ? 0.0 : 1.0);
      dw[1] = cS;
      dw[2] = eS;
      dw[3] = (double)(mem[0] + mem[1]);
      dw[4] = nslab[0] > 0 ? 1.0 : 0.0;
      dw[5] = nslab[1] > 0 ? 1.0 : 0.0;
    }
    if (tid < NPs) {
      dw[8 + tid] = bacc[0];
      dw[8 + NPs + tid] = bacc[1];
    }
  }
}

// the implicit queries of fia_self_influence's positions [p0, p0 + n): (a, b) of the row, (-1, -1)
// for a row outside [0, N) (never used as an index; the prologue then reports n = 0)
__global__ void k_self_pairs(int64_t n, int64_t p0, int64_t N, const int32_t* __restrict__ rows,
                             const int4* __restrict__ rowrec, int32_t* __restrict__ qu, int32_t* __restrict__ qi) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int64_t row = rows ? (int64_t)rows[p0 + t] : p0 + t;
  const bool ok = row >= 0 && row < N;
  int4 rr = make_int4(-1, -1, 0, 0);
  if (ok) rr = rowrec[row];
  qu[t] = rr.x;
  qi[t] = rr.y;
}

template <class M>
__global__ __launch_bounds__(solve_threads<2 * M::NPs>()) void k_big_down(BigArgs A, DownArgs Dn) {
  constexpr int K = M::K, NPs = M::NPs, Ds = M::Ds, NP = 2 * NPs, D = 2 * Ds;
  constexpr int NB = solve_nb<NP>(), LDR = NP + 16, LDP = NB + 1;
  constexpr int64_t GW = gram_words<M>();
  constexpr int kST = solve_threads<NP>(), kSW = kST / 64;
  __shared__ double P[LDR * LDP];
  // dd starts as the right-hand side b_S (block order, pads zero): column c of the augmented row
  // is read in the update of the panel that holds c, before that panel's factorisation puts d_c
  // there (a barrier apart)
  __shared__ double dd[NP];
  __shared__ double W11[NB * NB];
  __shared__ double red[64];
  double* __restrict__ Ls = Dn.lscr + (int64_t)blockIdx.x * LDR * NP;
  const int tid = threadIdx.x;
  const bool self = Dn.grp_off == nullptr;
  for (int64_t w = blockIdx.x; w < Dn.n; w += gridDim.x) {
    const int64_t o = Dn.first + w;            // the output slot: group, or position in rows
    const int64_t q = self ? w : last_at_most(Dn.grp_off, (int64_t)0, Dn.Q - 1, o);
    const double* __restrict__ qw = Dn.qwork + q * M::QW;
    const double n = qw[M::Work::n];
    const double* __restrict__ dw = Dn.dwork + w * down_words<M>();
    int status;
    double cS = 1.0, eS = 0.0, mS = 2.0;
    const double* __restrict__ dA0 = nullptr;
    const double* __restrict__ dA1 = nullptr;
    if (self) {
      status = n == 0.0 ? 2 : 1;
      if (status == 1) {
        const int64_t row = Dn.rows ? (int64_t)Dn.rows[o] : o;
        eS = A.resid[row];
      }
    } else {
      status = n == 0.0 ? 2 : (int)dw[0];
      if (status == 1) {
        cS = dw[1];
        eS = dw[2];
        mS = dw[3];
        if (dw[4] != 0.0) dA0 = Dn.slab + w * 2 * GW;
        if (dw[5] != 0.0) dA1 = Dn.slab + w * 2 * GW + GW;
      }
    }
    if (self && tid == 0 && Dn.error) Dn.error[o] = status == 1 ? eS : NAN;
    if (status != 1) {
      const double fill = status == 2 ? NAN : 0.0;
      if (Dn.dtheta)
        for (int a = tid; a < D; a += kST) Dn.dtheta[o * D + a] = fill;
      if (tid == 0) {
        if (Dn.group) Dn.group[o] = fill;
        if (Dn.first_order) Dn.first_order[o] = fill;
      }
      continue;
    }
    const double s2n = 2.0 / n, cdup = qw[M::Work::cdup], esum = qw[M::Work::esum];
    const double* __restrict__ vv = M::Work::v(qw, 0);         // both sides, 2 NPs
    const double* __restrict__ th = M::Work::theta(qw, 0);
    // b_S; a row's own system: sum e_j g_j is e v
    const double wdm = A.wd * (mS / n);
    for (int r = tid; r < NP; r += kST) {
      const int a = r >= NPs ? r - NPs : r;
      const double eg = self ? eS * vv[r] : dw[8 + r];
      dd[r] = a < Ds ? s2n * (eg + eS * vv[r]) + (M::decayed(a) ? wdm * th[r] : 0.0) : 0.0;
    }
    __syncthreads();
    if (Dn.first_order) {
      const double* __restrict__ xq = Dn.xb + q * NP;
      double part = 0.0;
      for (int r = tid; r < NP; r += kST) part = fma(xq[r], dd[r], part);
      part = bsum<kSW>(part, red);
      if (tid == 0) Dn.first_order[o] = part;
    }
    if (!Dn.solve) {
      __syncthreads();
      continue;
    }
    const int32_t u = A.qu[q], i = A.qi[q];
    const double* __restrict__ G0 = A.gram[0] + (int64_t)(A.slot[0] ? A.slot[0][u] : u) * GW;
    const double* __restrict__ G1 = A.gram[1] + (int64_t)(A.slot[1] ? A.slot[1][i] : i) * GW;
    // a row's own downdate takes v v^T out of each side's Gram: one more from the rank-1 factor
    const double cd_same = self ? cdup - 2.0 : cdup - cS, cd_cross = cdup - cS, es = esum - eS;
    const double wdd = A.wd * (1.0 - mS / n);
    auto aorig = [&](int r, int c) -> double {
      if (r >= NP) return (r == NP && c < NP) ? dd[c] : 0.0;
      const int sr = r >= NPs, sc = c >= NPs, rr = r - sr * NPs, cc = c - sc * NPs;
      if (rr >= Ds || cc >= Ds) return r == c ? 1.0 : 0.0;
      double h;
      if (sr == sc) {
        double g = gram_at<M>(sr ? G1 : G0, rr, cc);
        const double* __restrict__ dA = sr ? dA1 : dA0;
        if (dA) g -= gram_at<M>(dA, rr, cc);
        h = s2n * (g + cd_same * vv[r] * vv[c]);
        if (r == c) h += (M::decayed(rr) ? wdd : 0.0) + A.damping;
      } else {
        // item row / user column, as k_big_solve, with the group's share of the pair terms removed
        const int iu = sr ? cc : rr, ii = sr ? rr : cc;
        h = s2n * 2.0 * cd_cross * vv[NPs + ii] * vv[iu];
        if (ii == iu) {
          if constexpr (!M::ncf) {
            if (iu < K) h += s2n * 2.0 * es;
          } else {
            if (iu >= K) h += s2n * 2.0 * es * (double)A.t[8][M::H + (iu - K)];
          }
        }
      }
      return h;
    };
    big_ldlt_solve<NP>(aorig, Ls, P, dd, W11);
    const double* __restrict__ xs = P;
    double part = 0.0;
    for (int r = tid; r < NP; r += kST) {
      const int side = r >= NPs, a = r - side * NPs;
      if (a < Ds) {
        part = fma(vv[r], xs[r], part);
        if (Dn.dtheta) Dn.dtheta[o * D + M::ref_index(side, a)] = xs[r];
      }
    }
    part = bsum<kSW>(part, red);
    if (tid == 0 && Dn.group) Dn.group[o] = part;
    __syncthreads();   // P / dd are rewritten by the next system
  }
}

// FIA_BIGK_CHUNK (a positive integer): at most that many systems per launch of the large-k group
// and self paths -- a testing knob (a small value makes a short batch run in several chunks).  It
// can only lower the scratch-derived bound `dflt`; results do not depend on it
int64_t chunk_knob(int64_t dflt) {
  if (const char* e = std::getenv("FIA_BIGK_CHUNK")) {
    const long long v = std::atoll(e);
    if (v > 0 && v < dflt) return (int64_t)v;
  }
  return dflt;
}

template <class M>
hipError_t launch_down(fia_ctx* c, const BigArgs& A, DownArgs& Dn, hipStream_t s) {
  constexpr int NP = 2 * M::NPs;
  constexpr size_t lds = solve_lds<NP>();
  const int per_cu = (int)((160 * 1024) / lds);
  const int64_t resident = (int64_t)cu_count(c) * (per_cu > 0 ? per_cu : 1);
  const int64_t grid = Dn.n < resident ? Dn.n : resident;
  Dn.lscr = c->lscr.as<double>();
  hipLaunchKernelGGL(k_big_down<M>, dim3((unsigned)grid), dim3(solve_threads<NP>()), 0, s, A, Dn);
  return hipGetLastError();
}

template <class M>
hipError_t reserve_down(fia_ctx* c, int64_t chunk, bool slabs, hipStream_t s) {
  constexpr int NP = 2 * M::NPs;
  constexpr size_t lds = solve_lds<NP>();
  const int per_cu = (int)((160 * 1024) / lds);
  const int64_t resident = (int64_t)cu_count(c) * (per_cu > 0 ? per_cu : 1);
  const int64_t grid = chunk < resident ? chunk : resident;
  FIA_HIP_TRY(c->lscr.reserve(sizeof(double) * (size_t)(grid * (int64_t)(NP + 16) * NP), s));
  if (slabs) {
    FIA_HIP_TRY(c->dwork.reserve(sizeof(double) * (size_t)(chunk * down_words<M>()), s));
    FIA_HIP_TRY(c->dslab.reserve(sizeof(double) * (size_t)(chunk * 2 * gram_words<M>()), s));
  }
  return hipSuccess;
}

template <class M>
hipError_t group_big_impl(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* grp_offsets,
                          int64_t G, const int64_t* mem_offsets, int64_t TM, const int32_t* mem_row, double* group,
                          double* first_order, double* dtheta, hipStream_t s) {
  FIA_HIP_TRY(ensure_rowrec(c, s));
  // n, the pair terms, v and theta_t of every query, and H^-1 v when first_order is asked for
  FIA_HIP_TRY(big_systems(c, Q, qu, qi, first_order != nullptr, true, s));
  int64_t chunk = kDownScratch / (int64_t)(sizeof(double) * 2 * gram_words<M>());
  chunk = chunk_knob(chunk < 1 ? 1 : chunk);
  chunk = chunk > G ? G : chunk;
  FIA_HIP_TRY(reserve_down<M>(c, chunk, true, s));
  const BigArgs A = make_big_args(c, qu, qi);
  DownArgs Dn{};
  Dn.Q = Q;
  Dn.TM = TM;
  Dn.N = c->idx.N;
  Dn.grp_off = grp_offsets;
  Dn.mem_off = mem_offsets;
  Dn.mem_row = mem_row;
  Dn.rowrec = c->rowrec.as<int4>();
  Dn.qwork = c->qwork.as<double>();
  Dn.xb = c->xb.as<double>();
  Dn.dwork = c->dwork.as<double>();
  Dn.slab = c->dslab.as<double>();
  Dn.group = group;
  Dn.first_order = first_order;
  Dn.dtheta = dtheta;
  Dn.solve = group || dtheta;
  for (int64_t g0 = 0; g0 < G; g0 += chunk) {
    Dn.first = g0;
    Dn.n = G - g0 < chunk ? G - g0 : chunk;
    hipLaunchKernelGGL(k_group_down<M>, dim3(grid_cap(Dn.n, 1 << 20)), dim3(kGdThreads), 0, s, A, Dn);
    FIA_HIP_TRY(hipGetLastError());
    FIA_HIP_TRY(launch_down<M>(c, A, Dn, s));
  }
  return hipSuccess;
}

template <class M>
hipError_t self_big_impl(fia_ctx* c, int64_t n, const int32_t* rows, double* first_order, double* newton,
                         double* error, hipStream_t s) {
  FIA_HIP_TRY(ensure_rowrec(c, s));
  int64_t chunk = chunk_knob(kSelfChunk);
  chunk = chunk > n ? n : chunk;
  FIA_HIP_TRY(c->dpairs.reserve(sizeof(int32_t) * (size_t)(2 * chunk), s));
  int32_t* qu = c->dpairs.as<int32_t>();
  int32_t* qi = qu + chunk;
  DownArgs Dn{};
  Dn.N = c->idx.N;
  Dn.rows = rows;
  Dn.rowrec = c->rowrec.as<int4>();
  Dn.group = newton;
  Dn.first_order = first_order;
  Dn.error = error;
  Dn.solve = newton != nullptr;
  for (int64_t p0 = 0; p0 < n; p0 += chunk) {
    const int64_t len = n - p0 < chunk ? n - p0 : chunk;
    hipLaunchKernelGGL(k_self_pairs, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s, len, p0, Dn.N, rows,
                       Dn.rowrec, qu, qi);
    FIA_HIP_TRY(hipGetLastError());
    // every train row's pair is a train row: all of these are coupled systems
    FIA_HIP_TRY(big_systems(c, len, qu, qi, first_order != nullptr, false, s));
    if (p0 == 0) FIA_HIP_TRY(reserve_down<M>(c, chunk, false, s));
    const BigArgs A = make_big_args(c, qu, qi);
    Dn.first = p0;
    Dn.n = len;
    Dn.qwork = c->qwork.as<double>();
    Dn.xb = c->xb.as<double>();
    FIA_HIP_TRY(launch_down<M>(c, A, Dn, s));
  }
  return hipSuccess;
}

}  // namespace

hipError_t group_influence_big(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi,
                               const int64_t* grp_offsets, int64_t num_groups, const int64_t* mem_offsets,
                               int64_t total_members, const int32_t* mem_row, double* group, double* first_order,
                               double* dtheta, hipStream_t s) {
  hipError_t e = hipErrorInvalidValue;      // (big_supported is checked by the caller)
  for_big_size<BMF, BNCF>(c->p.model, c->p.k, [&](auto m) {
    e = group_big_impl<decltype(m)>(c, Q, qu, qi, grp_offsets, num_groups, mem_offsets, total_members, mem_row,
                                    group, first_order, dtheta, s);
  });
  return e;
}

hipError_t self_influence_big(fia_ctx* c, int64_t n, const int32_t* rows, double* first_order, double* newton,
                              double* error, hipStream_t s) {
  hipError_t e = hipErrorInvalidValue;
  for_big_size<BMF, BNCF>(c->p.model, c->p.k, [&](auto m) {
    e = self_big_impl<decltype(m)>(c, n, rows, first_order, newton, error, s);
  });
  return e;
}

}  // namespace fia
