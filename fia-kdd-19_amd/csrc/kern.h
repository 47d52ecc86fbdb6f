// Definitions shared by the small-k translation units: the model traits and the dispatch from
// (model, k) to them, the top-K selections and the per-batch kernel arguments.  The lane
// helpers they build on (wave reductions, the top-K order) are in lane.h, which the large-k
// units share.  gfx950 only.
#pragma once

#include <cmath>
#include <cstdint>

#include "common.h"
#include "lane.h"

namespace fia {

// ------------------------------------------------------------------------------------
// The per-query scoring record (c->rec) that the solve kernels write and the scoring kernels
// read: RecHead (common.h), then the block of the user side (sd = 0) and of the item side
// (sd = 1).  Offsets in doubles; a kernel reads them through its traits, M::Rec.
// ------------------------------------------------------------------------------------
template <int K>
struct RecMF : RecHead {
  static constexpr int head = 4;
  // side block, from side(R, sd)
  static constexpr int theta = 0;               // [K] the side's embedding
  static constexpr int x = K;                   // [K] x at the embedding coordinates
  static constexpr int bias = 2 * K;            // b_s + the global bias
  static constexpr int x_bias = 2 * K + 1;      // x at the bias coordinate
  static constexpr int dup_other = 2 * K + 2;   // the test pair's other endpoint (an id, as a double)
  static constexpr int SB = 2 * K + 4;          // (one word of padding)
  static constexpr int size = head + 2 * SB;
  template <class T>
  static constexpr T* side(T* R, int sd) { return R + head + sd * SB; }   // of the record at R
  // k_score_mf_mfma loads x of either side as double2
  static_assert((head + x) % 2 == 0 && SB % 2 == 0 && size % 2 == 0, "x of a side starts 16-B aligned");
};
template <int K>
struct RecNCF : RecHead {
  static constexpr int head = 4;
  // side block, from side(R, sd)
  static constexpr int x_mlp = 0;               // [K] x at the MLP embedding (on the k <= 16 mask path
                                                // k_ncf_rec_y overwrites it with y = W1_side^T x_mlp)
  static constexpr int w3g_x_gmf = K;           // [K] W3g * x at the GMF embedding
  static constexpr int dup_other = 2 * K;       // the test pair's other endpoint (an id, as a double)
  static constexpr int SB = 2 * K + 1;
  static constexpr int size = head + 2 * SB;
  static_assert(x_mlp == 0 && w3g_x_gmf == K, "k_solve_col: a side's block coordinate is its offset here");
  template <class T>
  static constexpr T* side(T* R, int sd) { return R + head + sd * SB; }   // of the record at R
};

// ------------------------------------------------------------------------------------
// model traits
// ------------------------------------------------------------------------------------
template <int K_>
struct MFm {
  static constexpr int K = K_;
  static constexpr int Ds = K + 1;
  static constexpr int D = 2 * Ds;
  using Rec = RecMF<K>;
  static constexpr int SB = Rec::SB, R = Rec::size;   // doubles per side block, per query
  static constexpr bool ncf = false;
  __device__ static bool decayed(int a) { return a < K; }
  // reference theta order [p_u, q_i, b_u, b_i]
  __device__ static int ref_index(int a) {
    int side = a >= Ds, j = side ? a - Ds : a;
    return j < K ? side * K + j : 2 * K + side;
  }
};

template <int K_>
struct NCFm {
  static constexpr int K = K_;
  static constexpr int H2 = K / 2;
  static constexpr int Ds = 2 * K;
  static constexpr int D = 2 * Ds;
  using Rec = RecNCF<K>;
  static constexpr int SB = Rec::SB, R = Rec::size;   // doubles per side block, per query
  static constexpr bool ncf = true;
  __device__ static bool decayed(int) { return true; }
  // reference theta order [Pm_u, Qm_i, Pg_u, Qg_i]
  __device__ static int ref_index(int a) {
    int side = a >= Ds, j = side ? a - Ds : a;
    return j < K ? side * K + j : 2 * K + side * K + (j - K);
  }
};

// f(M{}) with M the traits of (model, k): the small sizes; every size (the kernels that read only
// the parameter tables are built for the large k too).  False, f not called: not such a size.
template <class F>
bool dispatch_small(int model, int k, F&& f) {
  return for_small_size<MFm, NCFm>(model, k, f);
}
template <class F>
bool dispatch_any(int model, int k, F&& f) {
  return for_small_size<MFm, NCFm>(model, k, f) || for_big_size<MFm, NCFm>(model, k, f);
}

__device__ __forceinline__ int tri(int r, int c) { return (r * (r + 1)) / 2 + c; }

// Gram cache element (R >= C) of one side block.  Packed lower triangle, except NCF k = 16
// (Ds = 32), kept in the row-pair layout of k_solve_rows: lane t of a side system owns rows t
// and 31 - t, slot C of row t and slot 32 - C of row 31 - t (33 slots per lane), element
// slot * 16 + t -- one slot of the system's 16 lanes is one 128-B line.
template <class M>
__device__ __forceinline__ int gidx(int R, int C) {
  if constexpr (M::ncf && M::Ds == 32) return R < 16 ? C * 16 + R : (32 - C) * 16 + (31 - R);
  else return tri(R, C);
}
template <class M>
constexpr bool pair_layout() { return M::ncf && M::Ds == 32; }
// NCF k <= 16: per list position the Gram pass stores the two ReLU masks of the MLP (bits
// [0, k) z1 > 0, [k, 3k/2) z2 > 0: 4 B) instead of g_mlp (8k B); scoring rebuilds
// d1 = 1[z1 > 0] (W2 (1[z2 > 0] W3m)) from a 2^(k/2)-row LDS table and dots it with
// y = W1_side^T x_mlp (the record's MLP block after k_ncf_rec_y), since
// x_mlp . g_mlp = x_mlp . (W1_side d1) = (W1_side^T x_mlp) . d1
template <class M>
constexpr bool mask_path() { return M::ncf && M::K <= 16; }

// ---- which side-system solve a model takes (kernels in small_solve.hip) ----
// MF k = 16: a quad of lanes per side system (k_solve_quad); MF k = 8: a thread per system
template <class M>
constexpr bool use_quad_solve() {
  return !M::ncf && M::K == 16;
}
template <class M>
constexpr bool use_tps() {
  return !M::ncf && M::Ds <= 17 && !use_quad_solve<M>();
}

// side systems on 16x16 tiles: NCF (Ds = 2k) and MF k >= 32 (k coordinates + the bias)
template <class M>
constexpr bool use_tile_solve() {
  return !use_tps<M>() && !use_quad_solve<M>() && (M::ncf ? M::Ds : M::K) % 16 == 0 &&
         (M::ncf ? M::Ds : M::K) <= 64;
}

// NCF k <= 16: both side blocks in one wave, a column per lane (k_solve_col)
template <class M>
constexpr bool use_col_solve() {
  return M::ncf && 2 * M::Ds <= 64;
}

// one side-system solve per model: MF k = 16 k_solve_quad, MF k = 8 k_solve_tps, NCF k = 16
// k_solve_rows, NCF k = 8 k_solve_col, MF k in {32, 64} and NCF k = 32 k_solve_tile
template <class M>
constexpr bool solve_covered() {
  return use_quad_solve<M>() || use_tps<M>() || pair_layout<M>() || use_col_solve<M>() || use_tile_solve<M>();
}

// what k_ncf_query_pro hands to k_solve_rows per query (NCF k = 16; in c->qwork), in doubles
template <class M>
struct QPro {
  static constexpr int v = 0;                   // [D] d r-hat / d theta_t, block order
  static constexpr int rhat = M::D;             // r-hat(u, i)
  static constexpr int n = M::D + 1;            // related ratings
  static constexpr int cdup = M::D + 2;         // > 0: the test pair is a train row
  static constexpr int pad = M::D + 3;
  static constexpr int stride = M::D + 4;
};

// queries per entity-shared work item: 16 for MF k >= 64, where a work item's gathered
// rows (256 B each) are the dominant traffic and two query blocks would load them twice
template <class M>
constexpr int query_block() {
  return (!M::ncf && M::K >= 64) ? 16 : kQueryBlock;
}

template <int N>
__device__ __forceinline__ void load_row_f32(const float* __restrict__ src, double* dst) {
  if constexpr (N % 4 == 0) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
    for (int c = 0; c < N / 4; ++c) {
      float4 t = s4[c];
      dst[4 * c + 0] = t.x;
      dst[4 * c + 1] = t.y;
      dst[4 * c + 2] = t.z;
      dst[4 * c + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int c = 0; c < N; ++c) dst[c] = src[c];
  }
}

// Block-wide K-round selection over per-thread candidate lists (NC each).  Round t
// takes the best candidate strictly worse than round t-1's winner, so no
// "taken" marks are needed (positions are unique).  Writes K (pos, val) pairs.
template <int NC, int NT>
__device__ void block_topk(const double (&ca)[NC], const int (&cp)[NC], const double (&cv)[NC], int K,
                           int32_t* __restrict__ out_pos, double* __restrict__ out_val, double* s_a, int* s_p,
                           double* s_v) {
  double pa = INFINITY;
  int pp = -1;
  for (int t = 0; t < K; ++t) {
    double ba = -2.0, bv = 0.0;
    int bp = 0x7fffffff;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (cp[c] >= 0 && better(pa, pp, ca[c], cp[c]) && better(ca[c], cp[c], ba, bp)) {
        ba = ca[c]; bp = cp[c]; bv = cv[c];
      }
    }
    block_best<NT / 64>(ba, bp, bv, s_a, s_p, s_v);
    if (threadIdx.x == 0) {
      bool ok = ba > -1.5;
      out_pos[t] = ok ? bp : -1;
      out_val[t] = ok ? bv : NAN;
    }
    pa = ba; pp = bp;
  }
}

// The same K rounds by a workgroup of 256 over `ncand` (position, value) candidates in memory
// (position < 0 = none): thread 0 calls emit(t, ok, position, value) with round t's winner
// (!ok: fewer than t + 1 candidates).  Selection only: no value is changed on the way.
template <class Emit>
__device__ __forceinline__ void block_topk_slots(int64_t ncand, const int32_t* __restrict__ cp,
                                                 const double* __restrict__ cv, int K, Emit emit) {
  __shared__ double s_a[4], s_v[4];
  __shared__ int s_p[4];
  const int tid = threadIdx.x;
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
    block_best<4>(ba, bp, bv, s_a, s_p, s_v);
    if (tid == 0) emit(t, ba > -1.5, bp, bv);
    pa = ba;
    pp = bp;
  }
}

// One level of a batch-wide top-K merge (fia_total_influence, fia_self_influence): workgroup g
// selects the K best of slots [g * FAN, (g + 1) * FAN) of `n_slots` (K entries each, position
// -1 = none) into slot g of the next level, or, on the last level (one workgroup), into the
// call's outputs.
template <int FAN>
__global__ __launch_bounds__(256) void k_topk_merge(int64_t n_slots, int K, const int32_t* __restrict__ in_pos,
                                                    const double* __restrict__ in_val,
                                                    int32_t* __restrict__ out_pos, double* __restrict__ out_val,
                                                    int64_t* __restrict__ topk_idx, double* __restrict__ topk_val) {
  const int64_t s0 = (int64_t)blockIdx.x * FAN;
  const int64_t s1 = s0 + FAN < n_slots ? s0 + FAN : n_slots;
  const int64_t ncand = (s1 > s0 ? s1 - s0 : 0) * K;
  block_topk_slots(ncand, in_pos + s0 * K, in_val + s0 * K, K, [&](int t, bool ok, int bp, double bv) {
    if (topk_idx) {
      topk_idx[t] = ok ? (int64_t)bp : -1;
      topk_val[t] = ok ? bv : NAN;
    } else {
      out_pos[(int64_t)blockIdx.x * K + t] = ok ? bp : -1;
      out_val[(int64_t)blockIdx.x * K + t] = ok ? bv : NAN;
    }
  });
}

// Slots (of K entries) that the levels of a merge of `first` slots need, the first level included:
// first + first / FAN + first / FAN^2 + ...
template <int FAN>
inline size_t topk_merge_slots(int64_t first) {
  return (size_t)(first + first / (FAN - 1) + 8);
}

// Every level of the merge: `n` slots at the start of pos / val (topk_merge_slots<FAN>(n) slots
// reserved), level by level behind them, down to the call's outputs [K]; n == 0 fills them with
// -1 / NaN.
template <int FAN>
inline hipError_t topk_merge_levels(int64_t n, int K, int32_t* pos, double* val, int64_t* topk_idx, double* topk_val,
                                    hipStream_t s) {
  int64_t base = 0;
  for (;;) {
    const int64_t ng = n > 0 ? (n + FAN - 1) / FAN : 1;
    const bool last = ng == 1;
    hipLaunchKernelGGL(k_topk_merge<FAN>, dim3((unsigned)ng), dim3(256), 0, s, n, K, pos + base * K, val + base * K,
                       pos + (base + n) * K, val + (base + n) * K, last ? topk_idx : nullptr,
                       last ? topk_val : nullptr);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (last) return hipSuccess;
    base += n;
    n = ng;
  }
}

// ------------------------------------------------------------------------------------
// NCF helpers (NCF.py:85-145): z1 = L1_self + L1_other + b1 given; returns r-hat
// pieces via the per-row MLP with the ReLU derivative 1[z > 0] (TF ReluGrad).
// ------------------------------------------------------------------------------------
template <int K>
struct NCFWeights {   // LDS copies (fp64)
  double W2[K * (K / 2)];   // [k][k/2]
  double b2[K / 2];
  double W3[3 * (K / 2)];   // [W3m (k/2) ; W3g (k)]
};

template <int K>
__device__ void load_ncf_weights(NCFWeights<K>& w, const float* W2, const float* b2, const float* W3) {
  constexpr int H = K / 2;
  for (int t = threadIdx.x; t < K * H; t += blockDim.x) w.W2[t] = W2[t];
  for (int t = threadIdx.x; t < H; t += blockDim.x) w.b2[t] = b2[t];
  for (int t = threadIdx.x; t < 3 * H; t += blockDim.x) w.W3[t] = W3[t];
}

struct QueryArgs {
  const int32_t* qu;
  const int32_t* qi;
  int64_t U, I;
  const int64_t* ptr[2];
  const int32_t* row[2];
  const int32_t* other[2];
  const float* rating[2];
  const double* gram[2];
  const double* l1[2];
  const float* t[10];
  double wd, damping;
  PairTable pairs;
  // NCF, per list position of each side (written by k_gram_ncf_mfma):
  // g_mlp,j = W1_side . d1_j coordinate-major [k][N], and e_j = r-hat_j - y_j [side][N]
  const double* lgm[2];
  const double* lres;
  int64_t N;
  const double* d1tab;   // NCF k <= 16: d1 table [2^(k/2)][k] (k_ncf_d1_table)
};
// the context's index, caches and parameters as the small-k kernels read them (d1tab is set by
// the queries that read it)
QueryArgs make_args(fia_ctx* c, const int32_t* qu, const int32_t* qi);

// ---- the small-k kernels behind prepare_impl / query_impl (models.hip) ----
struct ScanArgs;   // scan.h
// small_gram.hip: NCF layer-1 rows of side sd; the per-slice Gram pass of both sides (MF
// k_gram_mf_mfma, NCF k_ncf_gram_rows, which picks its waves per CU); the split lists' sums
hipError_t launch_ncf_l1(int k, const float* emb, const float* W1, int sd, int64_t n_ent, double* out, hipStream_t s);
hipError_t launch_gram_slices(int model, int k, fia_ctx* c, const uint8_t* mark, hipStream_t s);
hipError_t launch_gram_combine(fia_ctx* c, int64_t nc0, const int32_t* comb0, int64_t nc1, const int32_t* comb1,
                               int GS, int GSP, const uint8_t* mark, hipStream_t s);
// small_solve.hip: the model's side-system solve with its grid rule (MF k = 16: the launch that
// also runs the scan S and the coupled solves, stamping ps; the others append to `coupled` for
// launch_coupled_solve, whose dispatch stamps `end`); NCF k = 16's per-query prologue into
// qpro [Q * QPro::stride]; the records of a given x
hipError_t launch_side_solve(int model, int k, fia_ctx* c, const ScanArgs& S, const QueryArgs& A, int64_t Q,
                             double* x_out, int32_t* coupled, hipStream_t s, PhaseSpan ps);
hipError_t launch_coupled_solve(int model, int k, const QueryArgs& A, int64_t Q, double* rec, double* x_out,
                                int32_t* coupled, hipStream_t s, hipEvent_t end);
hipError_t launch_ncf_query_pro(int k, const QueryArgs& A, int64_t Q, double* qpro, hipStream_t s);
hipError_t launch_record_x(int model, int k, const QueryArgs& A, int64_t Q, const double* x_in, double* rec,
                           double* x_out, hipStream_t s);
// small_score.hip: entity-shared scoring, MF k in {32, 64} (k_score_grouped_mf) and NCF k = 32
// (k_score_ncf); NCF k <= 16, per batch: the d1 table [2^(k/2)][k] and the records' y
hipError_t launch_score_grouped(int model, int k, int64_t grid, hipStream_t s, PhaseSpan ps, const QueryArgs& A,
                                int64_t nE, const int64_t* wstart, const int32_t* witems, const int64_t* gstart,
                                const int32_t* gq, const int64_t* qbase, const double* rec, int32_t* rel_idx,
                                double* influence, int K, int32_t* cand_pos, double* cand_val);
hipError_t launch_ncf_d1_table(int k, const float* W2, const float* W3, double* tab, hipStream_t s);
hipError_t launch_ncf_rec_y(int k, int64_t Q, const float* W1, double* rec, hipStream_t s);

}  // namespace fia
