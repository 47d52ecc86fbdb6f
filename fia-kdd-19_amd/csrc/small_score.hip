// Small-k entity-shared scoring (k_score_grouped_mf: MF k in {32, 64} with top-K > 1;
// k_score_ncf: NCF k = 32), the two per-batch NCF k <= 16 helpers of the item-run scorers
// (k_ncf_d1_table, k_ncf_rec_y) and the per-query merge of the chunk candidates
// (k_topk_merge*), which every scoring path ends with.  The other scorers: score_mf.hip (item
// runs, k <= 16), score_mfma.hip (MF k in {32, 64}, top-K <= 1).  gfx950 only.
#include <cmath>
#include <type_traits>

#include "kern.h"

namespace fia {
namespace {

// ------------------------------------------------------------------------------------
// Scoring (the dominant, HBM-streaming kernel).  Per related rating j of a query:
//   influence_j = (2 e_j s_j + c_q) / n,  s_j = x . g_j,  e_j = r-hat_j - y_j
// (mf:240-246: x . grad L_j / n with grad L_j = 2 e_j g_j + wd * M * theta_t); the K best
// of every chunk (|influence| desc, position asc) go to its candidate slots.
// ------------------------------------------------------------------------------------

// ------------------------------------------------------------------------------------
// Entity-shared scoring (MF k >= 32, NCF).  A work item is one chunk (<= kChunk ratings) of
// ONE entity's list (user list R_u or item list C_i) together with a block of the batch's
// queries that have that entity.  The list entries, the gathered other-side embedding rows
// and the per-rating residual e_j = r-hat_j - y_j depend on the train rating only, so they
// are loaded / computed once per work item and reused for every query in the block; per
// query only s_jq = x_q . g_j is new.  influence_jq = (2 e_j s_jq + c_q) / n_q
// (mf:240-246).  The test pair's own train row takes e and s from the query record
// (bit-identical copies, see k_solve).

// ------------------------------------------------------------------------------------
// MF k >= 32 entity-shared scoring with the query vectors read through the scalar cache.
// The work item (<= 256 ratings of one entity's list x <= 8 queries sharing the entity)
// needs, per query, x (k doubles) and a few header words -- the same for every lane.  In
// LDS every use is a broadcast read that still costs the LDS a full 64-lane transfer
// (with 4 rows per lane: one 16-B read per 8 FMAs, ~the LDS bandwidth of a CU); here they
// are s_load'ed into SGPRs and consumed as the SGPR operand of v_fma_f64, leaving LDS
// idle (20M MF k=64: 5.04 -> 4.74 ms per batch).  One candidate slot set per work item
// (spc = 1).
// ------------------------------------------------------------------------------------
template <class M>
__global__ __launch_bounds__(kScoreThreads) void k_score_grouped_mf(
    QueryArgs A, int64_t nE, const int64_t* __restrict__ wstart, const int32_t* __restrict__ witems,
    const int64_t* __restrict__ gstart, const int32_t* __restrict__ gq, const int64_t* __restrict__ qbase,
    const double* __restrict__ rec, int32_t* __restrict__ rel_idx, double* __restrict__ influence, int K_top,
    int32_t* __restrict__ cand_pos, double* __restrict__ cand_val) {
  static_assert(!M::ncf && M::K % 4 == 0, "MF, k a multiple of 4");
  constexpr int K = M::K, RT = kScoreRows, QB = query_block<M>(), CK = 4;
  using L = typename M::Rec;
  constexpr int NSV = (K + 1 + 63) / 64;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_items = wstart[nE];
  const int64_t stride = (int64_t)gridDim.x * (kScoreThreads / 64);
  for (int64_t wi = (int64_t)blockIdx.x * (kScoreThreads / 64) + wave; wi < n_items; wi += stride) {
    const int32_t g = witems[3 * wi], cidx = witems[3 * wi + 1], qblk = witems[3 * wi + 2];
    const int sd = g >= A.U ? 1 : 0;
    const int32_t e = sd ? (int32_t)(g - A.U) : g;
    const int64_t lb = A.ptr[sd][e] + (int64_t)cidx * kChunk;
    const int64_t rem = A.ptr[sd][e + 1] - lb;
    const int len = rem < kChunk ? (int)rem : kChunk;
    const int64_t gb = gstart[g] + (int64_t)qblk * QB;
    const int64_t gn = gstart[g + 1] - gb;
    const int nq = gn < QB ? (int)gn : QB;
    const int32_t* __restrict__ oth = A.other[sd] + lb;
    const float* __restrict__ rat = A.rating[sd] + lb;
    const int32_t* __restrict__ rw = A.row[sd] + lb;
    double selfv[NSV];
#pragma unroll
    for (int v = 0; v < NSV; ++v) {
      const int c = v * 64 + lane;
      const float* Es = sd == 0 ? A.t[0] : A.t[1];
      const float* Bs = sd == 0 ? A.t[2] : A.t[3];
      selfv[v] = c < K ? (double)Es[(int64_t)e * K + c] : (double)Bs[e];
    }
#define SV(c) readlane_d(selfv[(c) / 64], (c) % 64)
    int32_t o_[RT], row_[RT];
    float y_[RT], gb_[RT];
    bool ok_[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      const int idx = r * 64 + lane;
      ok_[r] = idx < len;
      const int li = ok_[r] ? idx : 0;
      o_[r] = oth[li];
      y_[r] = rat[li];
      row_[r] = rw[li];
    }
    const float* __restrict__ T = sd == 0 ? A.t[1] : A.t[0];
    const float* __restrict__ bt = sd == 0 ? A.t[3] : A.t[2];
#pragma unroll
    for (int r = 0; r < RT; ++r) gb_[r] = bt[o_[r]];
    // NQ = nq rounded up to a power of two: a static query count per path keeps the
    // accumulators in registers (padding columns repeat the last query, never written out)
    auto run = [&](auto nq_c) {
      constexpr int NQ = decltype(nq_c)::value;
      const double* __restrict__ xq[NQ];        // uniform: this side's x of each query
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        const int32_t q = gq[gb + (j < nq ? j : nq - 1)];
        xq[j] = L::side(rec + (int64_t)q * M::R, sd);
      }
      double ea[RT], acc[NQ][RT];
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        ea[r] = 0.0;
#pragma unroll
        for (int j = 0; j < NQ; ++j) acc[j][r] = 0.0;
      }
      float4 ga[RT];
#pragma unroll
      for (int r = 0; r < RT; ++r) ga[r] = *reinterpret_cast<const float4*>(T + (int64_t)o_[r] * K);
#pragma unroll 1
      for (int c0 = 0; c0 < K; c0 += CK) {
        float4 gn[RT];
        const int cn = c0 + CK < K ? c0 + CK : c0;
#pragma unroll
        for (int r = 0; r < RT; ++r) gn[r] = *reinterpret_cast<const float4*>(T + (int64_t)o_[r] * K + cn);
        double gd[RT][CK];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          gd[r][0] = ga[r].x; gd[r][1] = ga[r].y; gd[r][2] = ga[r].z; gd[r][3] = ga[r].w;
        }
#pragma unroll
        for (int cc = 0; cc < CK; ++cc) {
          const double sc = SV(c0 + cc);
#pragma unroll
          for (int r = 0; r < RT; ++r) ea[r] = fma(sc, gd[r][cc], ea[r]);
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
#pragma unroll
          for (int cc = 0; cc < CK; ++cc) {
            const double xc = xq[j][L::x + c0 + cc];  // scalar load, SGPR operand
#pragma unroll
            for (int r = 0; r < RT; ++r) acc[j][r] = fma(xc, gd[r][cc], acc[j][r]);
          }
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) ga[r] = gn[r];
      }
      {
        const double gbias = (double)A.t[4][0];
        const double bself = SV(K);
#pragma unroll
        for (int r = 0; r < RT; ++r) ea[r] = ea[r] + bself + (double)gb_[r] + gbias - (double)y_[r];
      }
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        if (j >= nq) continue;
        const int32_t q = gq[gb + j];
        const double* __restrict__ R = rec + (int64_t)q * M::R;
        const double inv_n = R[L::inv_n], cq = R[L::c_q], xv = R[L::x_v], rhat_ui = R[L::rhat];
        const double xsb = xq[j][L::x_bias], dup_o = xq[j][L::dup_other];
        const int64_t* __restrict__ qb = qbase + 4 * (int64_t)q;
        const int64_t obj = qb[sd] + (int64_t)cidx * kChunk, cbj = qb[2 + sd] + cidx;
        const int64_t poj = sd ? qb[1] - qb[0] : 0;   // |R_u| precedes item-side positions
        double la[RT], lv[RT];
        int lp[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
          double ee = ea[r], ss = acc[j][r] + xsb;
          if ((double)o_[r] == dup_o) { ee = rhat_ui - (double)y_[r]; ss = xv; }
          const double infl = (2.0 * ee * ss + cq) * inv_n;
          const int idx = r * 64 + lane;
          if (ok_[r]) {
            if (influence) __builtin_nontemporal_store(infl, influence + obj + idx);
            if (rel_idx) __builtin_nontemporal_store(row_[r], rel_idx + obj + idx);
          }
          lp[r] = ok_[r] ? cidx * kChunk + idx : -1;
          la[r] = ok_[r] ? topk_key(infl) : -2.0;
          lv[r] = infl;
        }
        if (K_top > 0) {
          double pa = INFINITY;
          int pp = -1;
          for (int t = 0; t < K_top; ++t) {
            double ba = -2.0, bv = 0.0;
            int bp = 0x7fffffff;
#pragma unroll
            for (int r = 0; r < RT; ++r)
              if (lp[r] >= 0 && better(pa, pp, la[r], lp[r]) && better(la[r], lp[r], ba, bp)) {
                ba = la[r]; bp = lp[r]; bv = lv[r];
              }
            wave_best(ba, bp, bv);
            if (lane == 0) {
              const bool okk = ba > -1.5;
              const int64_t slot = cbj * K_top + t;
              cand_pos[slot] = okk ? (int32_t)(bp + poj) : -1;
              cand_val[slot] = okk ? bv : NAN;
            }
            pa = ba;
            pp = bp;
          }
        }
      }
    };
    if (nq <= 1) run(std::integral_constant<int, 1>{});
    else if (nq <= 2) run(std::integral_constant<int, 2>{});
    else if (nq <= 4) run(std::integral_constant<int, 4>{});
    else if (QB == 8 || nq <= 8) run(std::integral_constant<int, 8>{});
    else run(std::integral_constant<int, QB>{});
#undef SV
  }
}

// MF k in {32, 64}, K_top <= 1: k_score_mf_mfma (score_mfma.hip)

// NCF k <= 16 (mask path): T[m][c] = sum_e W2[c][e] W3m[e] [bit e of m], the d1 of a train
// row whose z2 ReLU mask is m (before its z1 mask), one thread per entry
template <class M>
__global__ __launch_bounds__(256) void k_ncf_d1_table(const float* __restrict__ W2, const float* __restrict__ W3,
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

// NCF k <= 16 (mask path): the record's MLP block x_mlp -> y = W1_side^T x_mlp, one thread
// per (query, side), after every solve of the batch (k_score_ncf_runs dots y with d1; the
// candidates call and the Newton call take y from x by the same identity)
template <class M>
__global__ __launch_bounds__(256) void k_ncf_rec_y(int64_t Q, const float* __restrict__ W1, double* __restrict__ rec) {
  constexpr int K = M::K;
  using L = typename M::Rec;
  // W1 as fp64 in LDS: read per use as a broadcast (the per-use scalar loads of the fp32
  // table exposed one memory latency per weight: 20 us at yelp-ex)
  __shared__ double w1[2 * K * K];
  for (int e = threadIdx.x; e < 2 * K * K; e += 256) w1[e] = (double)W1[e];
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * Q) return;
  const int64_t q = t >> 1;
  const int sd = (int)(t & 1);
  double* __restrict__ S = L::side(rec + q * M::R, sd) + L::x_mlp;   // x_mlp in, y out
  double x[K];
#pragma unroll
  for (int a = 0; a < K; ++a) x[a] = S[a];
  const double* __restrict__ ws = w1 + sd * K * K;
#pragma unroll
  for (int c = 0; c < K; ++c) {
    double y = 0.0;
#pragma unroll
    for (int a = 0; a < K; ++a) y = fma(ws[a * K + c], x[a], y);
    S[c] = y;
  }
}

// ------------------------------------------------------------------------------------
// NCF k = 32 entity-shared scoring.  Same work items, query blocks and outputs as
// k_score_grouped_mf, but nothing of the MLP is recomputed here: per list position the
// Gram pass stored e_j and g_mlp,j = W1_side . d1_j (coordinate-major, every load a coalesced
// 512-B wave row), and the solve stored x_mlp and W3g * x_gmf, so
//   s_jq = x_mlp,q . g_mlp,j + (W3g * x_gmf,q) . gmf_other(j)   (ncf:193-280)
// is 2k FMAs per (rating, query) over the work item's 256 ratings (4 rows per lane).
// One candidate slot set per work item (spc = 1).  (k <= 16, which stores the ReLU masks
// instead of g_mlp, is scored by item runs: k_score_ncf_runs, score_mf.hip.)
// ------------------------------------------------------------------------------------
template <class M>
__global__ __launch_bounds__(kScoreThreads) void k_score_ncf(
    QueryArgs A, int64_t nE, const int64_t* __restrict__ wstart, const int32_t* __restrict__ witems,
    const int64_t* __restrict__ gstart, const int32_t* __restrict__ gq, const int64_t* __restrict__ qbase,
    const double* __restrict__ rec, int32_t* __restrict__ rel_idx, double* __restrict__ influence, int K_top,
    int32_t* __restrict__ cand_pos, double* __restrict__ cand_val) {
  static_assert(M::ncf && M::K == 32, "the NCF k = 32 kernel: g_mlp stored per list position (no mask path)");
  constexpr int K = M::K, RT = kScoreRows, QB = kQueryBlock, CK = 4;
  using L = typename M::Rec;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_items = wstart[nE];
  const int64_t stride = (int64_t)gridDim.x * (kScoreThreads / 64);
  const int64_t N = A.N;
  // work-item headers two stages ahead (scalar loads): the {entity, chunk, block} words of item
  // i + 2 and the list / group bounds of item i + 1 are in flight while item i is scored (most
  // yelp-ex items are short lists: the header chain was two of an item's ~four latencies)
  struct Words { int32_t g, cidx, qblk; };
  struct Bounds { int64_t p0, p1, s0, s1; };
  auto words = [&](int64_t w) {
    const int64_t wc = w < n_items ? w : n_items - 1;
    return Words{witems[3 * wc], witems[3 * wc + 1], witems[3 * wc + 2]};
  };
  auto bounds = [&](const Words& w) {
    const int sd = w.g >= A.U ? 1 : 0;
    const int32_t e = sd ? (int32_t)(w.g - A.U) : w.g;
    return Bounds{A.ptr[sd][e], A.ptr[sd][e + 1], gstart[w.g], gstart[w.g + 1]};
  };
  int64_t wi = (int64_t)blockIdx.x * (kScoreThreads / 64) + wave;
  if (wi >= n_items) return;
  Words w_cur = words(wi);
  Bounds b_cur = bounds(w_cur);
  Words w_nxt = words(wi + stride);
  for (; wi < n_items; wi += stride) {
    const Words w_n = w_nxt;
    const Bounds b_n = bounds(w_n);
    w_nxt = words(wi + 2 * stride);
    const int32_t g = w_cur.g, cidx = w_cur.cidx, qblk = w_cur.qblk;
    const int sd = g >= A.U ? 1 : 0;
    const int64_t lb = b_cur.p0 + (int64_t)cidx * kChunk;
    const int64_t rem = b_cur.p1 - lb;
    const int len = rem < kChunk ? (int)rem : kChunk;
    const int64_t gb = b_cur.s0 + (int64_t)qblk * QB;
    const int64_t gn = b_cur.s1 - gb;
    const int nq = gn < QB ? (int)gn : QB;
    w_cur = w_n;
    b_cur = b_n;

    const int32_t* __restrict__ oth = A.other[sd] + lb;
    const float* __restrict__ rat = A.rating[sd] + lb;
    const int32_t* __restrict__ rw = A.row[sd] + lb;
    const double* __restrict__ gml = A.lgm[sd] + lb;
    const double* __restrict__ res = A.lres + (int64_t)sd * N + lb;
    int32_t o_[RT], row_[RT], li_[RT];
    float y_[RT];
    double ej[RT];
    bool ok_[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      const int idx = r * 64 + lane;
      ok_[r] = idx < len;
      li_[r] = ok_[r] ? idx : 0;
      o_[r] = oth[li_[r]];
      y_[r] = rat[li_[r]];
      row_[r] = rw[li_[r]];
      ej[r] = res[li_[r]];
    }
    const float* __restrict__ T = sd == 0 ? A.t[3] : A.t[2];    // other side's gmf table
    // NQ = nq rounded up to a power of two: a static query count per path, so the
    // accumulators stay in registers without per-query exits (the padding columns
    // score copies of the last query and are never written out)
    // RTE = rows per lane actually scored: a chunk of <= 64 ratings (most lists at yelp-ex, ~24
    // ratings per user or item) runs one row per lane instead of four
    auto run = [&](auto nq_c, auto rt_c) {
      constexpr int NQ = decltype(nq_c)::value;
      constexpr int RTE = decltype(rt_c)::value;
      const double* __restrict__ xq[NQ];        // uniform: this side's record block of each query
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        const int32_t q = gq[gb + (j < nq ? j : nq - 1)];
        xq[j] = L::side(rec + (int64_t)q * M::R, sd);
      }
      double acc[NQ][RTE];
#pragma unroll
      for (int j = 0; j < NQ; ++j)
#pragma unroll
        for (int r = 0; r < RTE; ++r) acc[j][r] = 0.0;
#pragma unroll 1
      for (int c0 = 0; c0 < K; c0 += CK) {
        double gm_[RTE][CK];
        float go_[RTE][CK];
        // scalar base per coordinate + 32-bit lane offsets (kept opaque so the compiler
        // does not strength-reduce them into 2 VGPRs per (row, coordinate) pointer)
        const double* gbase = gml + (int64_t)c0 * N;
        asm volatile("" : "+s"(gbase));
#pragma unroll
        for (int r = 0; r < RTE; ++r) {
#pragma unroll
          for (int cc = 0; cc < CK; ++cc) gm_[r][cc] = gbase[(int64_t)cc * N + li_[r]];
          const float4 t = *reinterpret_cast<const float4*>(T + (int64_t)o_[r] * K + c0);
          go_[r][0] = t.x; go_[r][1] = t.y; go_[r][2] = t.z; go_[r][3] = t.w;
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
#pragma unroll
          for (int c2 = 0; c2 < CK / 2; ++c2) {
            // scalar loads: x_mlp and W3g * x_gmf as SGPR operands (no LDS)
            const double ax = xq[j][L::x_mlp + c0 + 2 * c2], ay = xq[j][L::x_mlp + c0 + 2 * c2 + 1];
            const double bx = xq[j][L::w3g_x_gmf + c0 + 2 * c2], by = xq[j][L::w3g_x_gmf + c0 + 2 * c2 + 1];
#pragma unroll
            for (int r = 0; r < RTE; ++r) {
              acc[j][r] = fma(ax, gm_[r][2 * c2], acc[j][r]);
              acc[j][r] = fma(ay, gm_[r][2 * c2 + 1], acc[j][r]);
              acc[j][r] = fma(bx, (double)go_[r][2 * c2], acc[j][r]);
              acc[j][r] = fma(by, (double)go_[r][2 * c2 + 1], acc[j][r]);
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        if (j >= nq) continue;   // padding columns (copies of the last query)
        const int32_t q = gq[gb + j];
        const double* __restrict__ Rj = rec + (int64_t)q * M::R;
        const double inv_n = Rj[L::inv_n], cq = Rj[L::c_q], xv = Rj[L::x_v], rhat_ui = Rj[L::rhat];
        const double dup_o = xq[j][L::dup_other];
        const int64_t* __restrict__ qb = qbase + 4 * (int64_t)q;
        const int64_t obj = qb[sd] + (int64_t)cidx * kChunk, cbj = qb[2 + sd] + cidx;
        const int64_t poj = sd ? qb[1] - qb[0] : 0;   // |R_u| precedes item-side positions
        double la[RTE], lv[RTE];
        int lp[RTE];
#pragma unroll
        for (int r = 0; r < RTE; ++r) {
          double ee = ej[r], ss = acc[j][r];
          if ((double)o_[r] == dup_o) { ee = rhat_ui - (double)y_[r]; ss = xv; }
          const double infl = (2.0 * ee * ss + cq) * inv_n;
          const int idx = r * 64 + lane;
          if (ok_[r]) {
            if (influence) __builtin_nontemporal_store(infl, influence + obj + idx);
            if (rel_idx) __builtin_nontemporal_store(row_[r], rel_idx + obj + idx);
          }
          lp[r] = ok_[r] ? cidx * kChunk + idx : -1;
          la[r] = ok_[r] ? topk_key(infl) : -2.0;
          lv[r] = infl;
        }
        if (K_top > 0) {
          double pa = INFINITY;
          int pp = -1;
          for (int t = 0; t < K_top; ++t) {
            double ba = -2.0, bv = 0.0;
            int bp = 0x7fffffff;
#pragma unroll
            for (int r = 0; r < RTE; ++r)
              if (lp[r] >= 0 && better(pa, pp, la[r], lp[r]) && better(la[r], lp[r], ba, bp)) {
                ba = la[r]; bp = lp[r]; bv = lv[r];
              }
            wave_best(ba, bp, bv);
            if (lane == 0) {
              const bool okk = ba > -1.5;
              const int64_t slot = cbj * K_top + t;
              cand_pos[slot] = okk ? (int32_t)(bp + poj) : -1;
              cand_val[slot] = okk ? bv : NAN;
            }
            pa = ba;
            pp = bp;
          }
        }
      }
    };
    auto run_q = [&](auto rt_c) {
      if (nq <= 1) run(std::integral_constant<int, 1>{}, rt_c);
      else if (nq <= 2) run(std::integral_constant<int, 2>{}, rt_c);
      else if (nq <= 4) run(std::integral_constant<int, 4>{}, rt_c);
      else run(std::integral_constant<int, QB>{}, rt_c);
    };
    if (len <= 64) run_q(std::integral_constant<int, 1>{});
    else run_q(std::integral_constant<int, RT>{});
    __builtin_amdgcn_wave_barrier();
  }
}

// Merge the chunk candidates of every query (one wave per query).
__global__ __launch_bounds__(64) void k_topk_merge(const int32_t* __restrict__ qu, const int32_t* __restrict__ qi,
                                                   int64_t Q, const int64_t* __restrict__ coff, int K, int spc,
                                                   const int32_t* __restrict__ cand_pos,
                                                   const double* __restrict__ cand_val,
                                                   const int64_t* __restrict__ uptr, const int32_t* __restrict__ urow,
                                                   const int64_t* __restrict__ iptr, const int32_t* __restrict__ irow,
                                                   int64_t U, int64_t I, int64_t* __restrict__ topk_pos,
                                                   int64_t* __restrict__ topk_idx, double* __restrict__ topk_val) {
  const int64_t q = blockIdx.x;
  if (q >= Q) return;
  const int lane = threadIdx.x;
  const int64_t cb = coff[q] * spc * K, ce = coff[q + 1] * spc * K;
  const int32_t u = qu[q], i = qi[q];
  const bool ok_id = (u >= 0 && u < U && i >= 0 && i < I);
  const int64_t ub = ok_id ? uptr[u] : 0, du = ok_id ? uptr[u + 1] - ub : 0, ib = ok_id ? iptr[i] : 0;
  double pa = INFINITY;
  int pp = -1;
  for (int t = 0; t < K; ++t) {
    double ba = -2.0, bv = 0.0;
    int bp = 0x7fffffff;
    for (int64_t c = cb + lane; c < ce; c += 64) {
      const int p = cand_pos[c];
      if (p < 0) continue;
      const double vv = cand_val[c];
      const double a = topk_key(vv);
      if (better(pa, pp, a, p) && better(a, p, ba, bp)) { ba = a; bp = p; bv = vv; }
    }
    wave_best(ba, bp, bv);
    if (lane == 0) {
      const bool ok = ba > -1.5;
      topk_pos[q * K + t] = ok ? bp : -1;
      topk_idx[q * K + t] = ok ? (int64_t)(bp < du ? urow[ub + bp] : irow[ib + (bp - du)]) : -1;
      topk_val[q * K + t] = ok ? bv : NAN;
    }
    pa = ba;
    pp = bp;
  }
}

// Small K: one THREAD per query walks its chunks' candidates K times (a query has a few to a
// few hundred candidate slots; a wave per query mostly idles at K = 1).  Same order and
// output as k_topk_merge.
__global__ __launch_bounds__(256) void k_topk_merge_thread(
    const int32_t* __restrict__ qu, const int32_t* __restrict__ qi, int64_t Q, const int64_t* __restrict__ coff,
    int K, int spc, const int32_t* __restrict__ cand_pos, const double* __restrict__ cand_val,
    const int64_t* __restrict__ uptr, const int32_t* __restrict__ urow, const int64_t* __restrict__ iptr,
    const int32_t* __restrict__ irow, int64_t U, int64_t I, int64_t* __restrict__ topk_pos,
    int64_t* __restrict__ topk_idx, double* __restrict__ topk_val) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Q) return;
  const int64_t cb = coff[q] * spc * K, ce = coff[q + 1] * spc * K;
  const int32_t u = qu[q], i = qi[q];
  const bool ok_id = (u >= 0 && u < U && i >= 0 && i < I);
  const int64_t ub = ok_id ? uptr[u] : 0, du = ok_id ? uptr[u + 1] - ub : 0, ib = ok_id ? iptr[i] : 0;
  double pa = INFINITY;
  int pp = -1;
  for (int t = 0; t < K; ++t) {
    double ba = -2.0, bv = 0.0;
    int bp = 0x7fffffff;
    // both words of a slot loaded unconditionally (empty slots hold -1 / NaN) and 4 slots
    // per round, so the candidate reads are one round trip per 4 slots, not two per slot
    int64_t c = cb;
    for (; c + 4 <= ce; c += 4) {
      int p4[4];
      double v4[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { p4[j] = cand_pos[c + j]; v4[j] = cand_val[c + j]; }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double a = topk_key(v4[j]);
        if (p4[j] >= 0 && better(pa, pp, a, p4[j]) && better(a, p4[j], ba, bp)) { ba = a; bp = p4[j]; bv = v4[j]; }
      }
    }
    for (; c < ce; ++c) {
      const int p = cand_pos[c];
      const double vv = cand_val[c];
      const double a = topk_key(vv);
      if (p >= 0 && better(pa, pp, a, p) && better(a, p, ba, bp)) { ba = a; bp = p; bv = vv; }
    }
    const bool ok = ba > -1.5;
    topk_pos[q * K + t] = ok ? bp : -1;
    topk_idx[q * K + t] = ok ? (int64_t)(bp < du ? urow[ub + bp] : irow[ib + (bp - du)]) : -1;
    topk_val[q * K + t] = ok ? bv : NAN;
    pa = ba;
    pp = bp;
  }
}

// K = 1 of the above on a 16-lane ROW per query (a wave takes four): the thread-per-query walk
// is a chain of about six dependent round trips (coff -> uptr -> ~9 slots 4 at a time ->
// urow/irow), here it is three: {coff, qu, qi}, then {uptr, iptr, every slot of the row: lane l
// takes slots cb + l, cb + l + 16, ...} together, then the row lookup.  Both words of a slot are
// loaded unconditionally (a slot past the query's end reads slot 0, always reserved, and
// counts as empty), kMergeRowRounds rounds issued before any use.  The lanes' bests meet in the
// row rotations of wave_best: `better` is a strict total order on (key, position), so the
// winner is the one the serial walk finds.  No lane leaves before the rotations.
// Taken up to kMergeRowMaxQ queries (a quarter of a wave per query: 4,096 waves there, half of
// what the chip holds): ml-1m-ex, 12,074 queries, 8.04 -> 4.42 us.  Beyond it the rows fill every
// wave slot for the length of the kernel -- yelp-ex, 51,153 queries = 12.8 k waves: 8.24 -> 7.41 us
// alone, but the step with two batches in flight did not gain (0.4868 -> 0.4887 ms, medians of 5
// and 4 alternating runs, inside the parent's spread): the other batch's kernels wait for the
// slots -- so larger batches keep the thread per query (profiles/step_tail.md).
constexpr int kMergeRowRounds = 2;
constexpr int64_t kMergeRowMaxQ = 16384;
__global__ __launch_bounds__(256) void k_topk_merge_row(
    const int32_t* __restrict__ qu, const int32_t* __restrict__ qi, int64_t Q, const int64_t* __restrict__ coff,
    int spc, const int32_t* __restrict__ cand_pos, const double* __restrict__ cand_val,
    const int64_t* __restrict__ uptr, const int32_t* __restrict__ urow, const int64_t* __restrict__ iptr,
    const int32_t* __restrict__ irow, int64_t U, int64_t I, int64_t* __restrict__ topk_pos,
    int64_t* __restrict__ topk_idx, double* __restrict__ topk_val) {
  const int l = threadIdx.x & 15;
  const int64_t q0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const bool act = q0 < Q;
  const int64_t q = act ? q0 : Q - 1;
  const int64_t cb = coff[q] * spc, ce = coff[q + 1] * spc;
  const int32_t u = qu[q], i = qi[q];
  int p2[kMergeRowRounds];
  double v2[kMergeRowRounds];
#pragma unroll
  for (int r = 0; r < kMergeRowRounds; ++r) {
    const int64_t c = cb + l + 16 * r;
    const int64_t cc = c < ce ? c : 0;
    p2[r] = cand_pos[cc];
    v2[r] = cand_val[cc];
    if (c >= ce) p2[r] = -1;
  }
  const bool ok_id = (u >= 0 && u < U && i >= 0 && i < I);
  const int64_t ub = ok_id ? uptr[u] : 0, du = ok_id ? uptr[u + 1] - ub : 0, ib = ok_id ? iptr[i] : 0;
  double ba = -2.0, bv = 0.0;
  int bp = 0x7fffffff;
#pragma unroll
  for (int r = 0; r < kMergeRowRounds; ++r) {
    const double a = topk_key(v2[r]);
    if (p2[r] >= 0 && better(a, p2[r], ba, bp)) { ba = a; bp = p2[r]; bv = v2[r]; }
  }
  for (int64_t c = cb + l + 16 * kMergeRowRounds; c < ce; c += 16) {
    const int p = cand_pos[c];
    const double vv = cand_val[c];
    const double a = topk_key(vv);
    if (p >= 0 && better(a, p, ba, bp)) { ba = a; bp = p; bv = vv; }
  }
  best_dpp_step<0x128>(ba, bp, bv);   // row_ror:8
  best_dpp_step<0x124>(ba, bp, bv);   // row_ror:4
  best_dpp_step<0x122>(ba, bp, bv);   // row_ror:2
  best_dpp_step<0x121>(ba, bp, bv);   // row_ror:1 -- every lane of the row holds the query's best
  if (act && l == 0) {
    const bool ok = ba > -1.5;
    topk_pos[q] = ok ? bp : -1;
    topk_idx[q] = ok ? (int64_t)(bp < du ? urow[ub + bp] : irow[ib + (bp - du)]) : -1;
    topk_val[q] = ok ? bv : NAN;
  }
}

}  // namespace

hipError_t launch_score_grouped(int model, int k, int64_t grid, hipStream_t s, PhaseSpan ps, const QueryArgs& A,
                                int64_t nE, const int64_t* wstart, const int32_t* witems, const int64_t* gstart,
                                const int32_t* gq, const int64_t* qbase, const double* rec, int32_t* rel_idx,
                                double* influence, int K, int32_t* cand_pos, double* cand_val) {
  bool ok = false;
  dispatch_small(model, k, [&](auto m) {
    using M = decltype(m);
    if constexpr (M::K >= 32) {
      if constexpr (M::ncf)
        hipExtLaunchKernelGGL(k_score_ncf<M>, dim3((unsigned)grid), dim3(kScoreThreads), 0, s, ps.a, ps.b, 0, A, nE,
                              wstart, witems, gstart, gq, qbase, rec, rel_idx, influence, K, cand_pos, cand_val);
      else
        hipExtLaunchKernelGGL(k_score_grouped_mf<M>, dim3((unsigned)grid), dim3(kScoreThreads), 0, s, ps.a, ps.b, 0,
                              A, nE, wstart, witems, gstart, gq, qbase, rec, rel_idx, influence, K, cand_pos,
                              cand_val);
      ok = true;
    }
  });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_ncf_d1_table(int k, const float* W2, const float* W3, double* tab, hipStream_t s) {
  bool ok = false;
  dispatch_small(FIA_MODEL_NCF, k, [&](auto m) {
    using M = decltype(m);
    if constexpr (mask_path<M>()) {
      constexpr int NT = (1 << (M::K / 2)) * M::K;
      hipLaunchKernelGGL(k_ncf_d1_table<M>, dim3((unsigned)((NT + 255) / 256)), dim3(256), 0, s, W2, W3, tab);
      ok = true;
    }
  });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_ncf_rec_y(int k, int64_t Q, const float* W1, double* rec, hipStream_t s) {
  bool ok = false;
  dispatch_small(FIA_MODEL_NCF, k, [&](auto m) {
    using M = decltype(m);
    if constexpr (mask_path<M>()) {
      hipLaunchKernelGGL(k_ncf_rec_y<M>, dim3((unsigned)((2 * Q + 255) / 256)), dim3(256), 0, s, Q, W1, rec);
      ok = true;
    }
  });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_topk_merge(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, int K, int spc,
                             int64_t* topk_pos, int64_t* topk_idx, double* topk_val, hipStream_t s,
                             int64_t max_chunks) {
  if (K <= 0 || Q <= 0) return hipSuccess;
  // a thread per query while the queries have few chunks (<= 16 on average: ml-1m-ex,
  // yelp-ex); a wave per query over long candidate lists (20M: ~170 chunks per query)
  if (K == 1 && max_chunks <= 16 * Q && Q <= kMergeRowMaxQ) {
    // a 16-lane row per query: three dependent round trips where the thread's walk has ~six
    hipLaunchKernelGGL(k_topk_merge_row, dim3((unsigned)((Q * 16 + 255) / 256)), dim3(256), 0, s, qu, qi, Q,
                       c->coff.as<int64_t>(), spc, c->cand_pos.as<int32_t>(), c->cand_val.as<double>(),
                       c->idx.side[0].ptr.as<int64_t>(), c->idx.side[0].row.as<int32_t>(),
                       c->idx.side[1].ptr.as<int64_t>(), c->idx.side[1].row.as<int32_t>(), c->p.U, c->p.I, topk_pos,
                       topk_idx, topk_val);
    return hipGetLastError();
  }
  if (K <= 4 && max_chunks <= 16 * Q) {
    hipLaunchKernelGGL(k_topk_merge_thread, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, qu, qi, Q,
                       c->coff.as<int64_t>(), K, spc, c->cand_pos.as<int32_t>(), c->cand_val.as<double>(),
                       c->idx.side[0].ptr.as<int64_t>(), c->idx.side[0].row.as<int32_t>(),
                       c->idx.side[1].ptr.as<int64_t>(), c->idx.side[1].row.as<int32_t>(), c->p.U, c->p.I, topk_pos,
                       topk_idx, topk_val);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)Q), dim3(64), 0, s, qu, qi, Q, c->coff.as<int64_t>(), K, spc,
                     c->cand_pos.as<int32_t>(), c->cand_val.as<double>(), c->idx.side[0].ptr.as<int64_t>(),
                     c->idx.side[0].row.as<int32_t>(), c->idx.side[1].ptr.as<int64_t>(),
                     c->idx.side[1].row.as<int32_t>(), c->p.U, c->p.I, topk_pos, topk_idx, topk_val);
  return hipGetLastError();
}

}  // namespace fia
