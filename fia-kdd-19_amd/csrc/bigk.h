// Large-k FIA path, the pieces shared by its translation units (bigk.hip: the host side;
// bigk_prepare.hip, bigk_solve.hip, bigk_solve_batched.hip, bigk_score.hip: the kernels of each
// phase behind their launchers; group_big.hip: the downdated solves of fia_group_influence and
// fia_self_influence): model traits, the Gram tile layout, the kernels' argument struct, the
// solve constants, the blocked LDL^T of one system in a workgroup's scratch slab, and the
// launchers' declarations.
#pragma once

#include "common.h"
#include "lane.h"

namespace fia {
namespace {

// C += A B on the f64 matrix cores; lane l supplies A[l&15][l>>4] and B[l>>4][l&15],
// and holds C[(l>>4) + 4r][l&15] in register r.
__device__ __forceinline__ d4_t mfma4(double a, double b, d4_t c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

constexpr int kBigSlice = 2048;     // ratings per Gram work item (big_work_lists, k_big_gram)
constexpr int kBigMfmaQB = 32;      // queries per scoring work item (build_groups, k_big_score_mfma)

// ------------------------------------------------------------------------------------
// The per-query blocks that the kernels of one phase leave for the next (offsets in doubles; a
// kernel reads them through its traits, M::Rec and M::Work).
// The scoring record (c->rec), written by the solves, headed by k_big_finish, read by
// k_big_score_mfma: RecHead (common.h), the side solves' partial sums, then the block of the user
// side (sd = 0) and of the item side (sd = 1).
// ------------------------------------------------------------------------------------
struct BigRecHead : RecHead {
  // c_q and x . v of each side system; k_big_finish sums them into RecHead's c_q and x_v
  static constexpr int cq_u = 4, xv_u = 5, cq_i = 6, xv_i = 7;
  static constexpr int cq_of(int sd) { return cq_u + 2 * sd; }
  static constexpr int xv_of(int sd) { return xv_u + 2 * sd; }
  static constexpr int head = 8;
};
template <int K>
struct BigRecMF : BigRecHead {
  // side block, from side(R, sd)
  static constexpr int x = 0;                   // [K] x at the embedding coordinates
  static constexpr int x_bias = K;              // x at the bias coordinate
  static constexpr int dup_other = K + 1;       // the test pair's other endpoint (an id, as a double)
  static constexpr int SB = K + 2;
  static constexpr int size = head + 2 * SB;
  static_assert(x_bias == x + K, "the solves write x and x_bias as one run");
  template <class T>
  static constexpr T* side(T* R, int sd) { return R + head + sd * SB; }   // of the record at R
};
template <int K>
struct BigRecNCF : BigRecHead {
  // side block, from side(R, sd)
  static constexpr int x_mlp = 0;               // [K] x at the MLP embedding
  static constexpr int w3g_x_gmf = K;           // [K] W3g * x at the GMF embedding
  static constexpr int dup_other = 2 * K;       // the test pair's other endpoint (an id, as a double)
  static constexpr int SB = 2 * K + 1;
  static constexpr int size = head + 2 * SB;
  template <class T>
  static constexpr T* side(T* R, int sd) { return R + head + sd * SB; }   // of the record at R
};
// The work words (c->qwork), written by k_big_prologue, read by the solves, k_big_finish and the
// downdated solves of group_big.hip
template <int NPs>
struct BigWork {
  static constexpr int n = 0;                   // related ratings; 0: none, ids out of range or not cached
  static constexpr int cdup = 1;                // copies of the test pair among the train rows
  static constexpr int esum = 2;                // cdup * r-hat - the sum of their ratings
  static constexpr int rhat = 3;                // r-hat(u, i)
  static constexpr int coupled = 4;             // 1: cdup > 0, the query is one full system
  static constexpr int head = 8;
  // v = d r-hat(u,i) / d theta_t and theta_t of side sd, NPs each (pads zero).  The two sides lie
  // back to back: a coupled system reads v(qw, 0) and theta(qw, 0) as vectors of 2 NPs
  template <class T>
  static constexpr T* v(T* qw, int sd) { return qw + head + sd * NPs; }
  template <class T>
  static constexpr T* theta(T* qw, int sd) { return qw + head + 2 * NPs + sd * NPs; }
  static constexpr int size = head + 4 * NPs;
};

// ------------------------------------------------------------------------------------
// model traits.  A side block has Ds coordinates padded to NPs = 16 T.
//   MF  side [emb (k), bias, 0 pad]  (mf:43-65)
//   NCF side [mlp emb (k), gmf emb (k)] (ncf:49-64)
// ------------------------------------------------------------------------------------
template <int K_>
struct BMF {
  static constexpr int K = K_, H = 1, Ds = K + 1, NPs = K + 16, T = NPs / 16;
  static constexpr bool ncf = false;
  using Rec = BigRecMF<K>;
  using Work = BigWork<NPs>;
  static constexpr int SB = Rec::SB, R = Rec::size, QW = Work::size;
  __host__ __device__ static constexpr bool decayed(int a) { return a < K; }
  // reference theta order [p_u, q_i, b_u, b_i]
  __device__ static int ref_index(int side, int a) { return a < K ? side * K + a : 2 * K + side; }
};

template <int K_>
struct BNCF {
  static constexpr int K = K_, H = K / 2, Ds = 2 * K, NPs = 2 * K, T = NPs / 16;
  static constexpr bool ncf = true;
  using Rec = BigRecNCF<K>;
  using Work = BigWork<NPs>;
  static constexpr int SB = Rec::SB, R = Rec::size, QW = Work::size;
  __host__ __device__ static constexpr bool decayed(int) { return true; }
  // reference theta order [Pm_u, Qm_i, Pg_u, Qg_i]
  __device__ static int ref_index(int side, int a) { return a < K ? side * K + a : 2 * K + side * K + (a - K); }
};

// f(M{}) for the traits M of (model, k), its result returned; hipErrorInvalidValue for a size
// that is not built
template <class F>
hipError_t big_dispatch(int model, int k, F&& f) {
  hipError_t e = hipErrorInvalidValue;
  for_big_size<BMF, BNCF>(model, k, [&](auto m) { e = f(m); });
  return e;
}

// Gram tile storage: tile (tr, tc), tc <= tr, in column-major tile order; inside a tile
// element (row m, col n) at m + 16 n.
__host__ __device__ constexpr int tile_off(int T, int tr, int tc) { return tc * T - (tc * (tc - 1)) / 2 + (tr - tc); }
template <class M>
constexpr int64_t gram_words() { return (int64_t)M::T * (M::T + 1) / 2 * 256; }

template <class M>
__device__ __forceinline__ double gram_at(const double* __restrict__ G, int r, int c) {
  const int hi = r > c ? r : c, lo = r > c ? c : r;
  return G[tile_off(M::T, hi >> 4, lo >> 4) * 256 + (hi & 15) + 16 * (lo & 15)];
}

struct BigArgs {
  const int32_t* qu;
  const int32_t* qi;
  int64_t U, I;
  const int64_t* ptr[2];
  const int32_t* row[2];
  const int32_t* other[2];
  const float* rating[2];
  const double* gram[2];
  const double* l1[2];
  const double* resid;
  const double* gm[2];     // NCF g_mlp per side, by train row
  const int32_t* slot[2];  // Gram cache slot per entity (nullptr = identity)
  const float* t[10];
  double wd, damping;
  PairTable pairs;
};

inline BigArgs make_big_args(fia_ctx* c, const int32_t* qu, const int32_t* qi) {
  BigArgs A;
  fill_list_args(c, A);
  A.qu = qu;
  A.qi = qi;
  for (int s = 0; s < 2; ++s) {
    A.gm[s] = c->gm[s].as<double>();
    A.slot[s] = c->subset ? c->slot[s].as<int32_t>() : nullptr;
  }
  A.resid = c->resid.as<double>();
  return A;
}

inline unsigned grid_cap(int64_t n, int64_t cap) {
  if (n < 1) n = 1;
  return (unsigned)(n < cap ? n : cap);
}

inline int cu_count(fia_ctx* c) {
  if (c->num_cus <= 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || n <= 0) n = 256;
    c->num_cus = n;
  }
  return c->num_cus;
}

// ------------------------------------------------------------------------------------
// Blocked left-looking LDL^T + solve of one system by one 512-thread workgroup.  The
// augmented matrix comes from the caller's `aorig(r, c)`: rows [0, NP) the symmetric system,
// row NP the right-hand side b^T, rows NP+1..NP+15 zero, so row NP of L is y = D^-1 L^-1 b.
// L (column-major, LDR = NP + 16 rows) lives in the workgroup's scratch slab Ls.  Per
// panel of NB columns:
//   (a) MFMA update of the panel rows from the factored columns (L streamed, D L^T of
//       the panel rows on the fly), result in LDS;
//   (b) one wave factors the NB x NB diagonal block in registers (readlane broadcasts);
//   (c) every row below solves against it in registers (barrier-free TRSM) and writes
//       its L row segment.
// Then L^T x = y in 32-column blocks from the end: a one-wave triangle per block and a
// GEMV update of the earlier entries, whose L operands are loaded behind the triangle.
// The solution is left in P[0, NP) (LDS), every thread past the last barrier.
// ------------------------------------------------------------------------------------
constexpr int kSolveMG = 2;     // row tiles per wave per MFMA pass
constexpr int PD = 8;           // k-steps in flight in the panel update
// solve workgroup (8 waves: 2 per SIMD, 256 VGPRs each -- the 32-wide register rows of
// the diagonal block / TRSM and the prefetch ring fit without spills)
template <int NP>
constexpr int solve_threads() { return 512; }

template <int NP>
constexpr int solve_nb() {   // 32-column panels when NP allows and LDS fits, else 16
  return NP % 32 == 0 && ((NP + 16) * 33 + NP + 32 * 32 + 64) * 8 <= 160 * 1024 ? 32 : 16;
}
template <int NP>
constexpr size_t solve_lds() {
  return (size_t)((NP + 16) * (solve_nb<NP>() + 1) + NP + solve_nb<NP>() * solve_nb<NP>() + 64) * 8;
}

// block-wide sum for workgroups of NW waves (every thread gets the result; red: NW doubles)
template <int NW>
__device__ __forceinline__ double bsum(double x, double* red) {
  x = wave_sum(x);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t += red[w];
  return t;
}

// P: LDR * (NB + 1) doubles, dd: NP, W11: NB * NB (all LDS).  k_big_solve (bigk_solve.hip) keeps
// this loop in its own body (see there: through this function its MF k = 256 instantiation
// spilled twice the registers); a change to one belongs in the other.
template <int NP, class AOrig>
__device__ __forceinline__ void big_ldlt_solve(const AOrig& aorig, double* Ls, double* P, double* dd, double* W11) {
  constexpr int NB = solve_nb<NP>(), LDR = NP + 16, LDP = NB + 1;
  constexpr int NRT = LDR / 16, NCT = NB / 16, MG = kSolveMG;
  constexpr int kST = solve_threads<NP>(), kSW = kST / 64;
  constexpr int CPT = (NP + kST - 1) / kST;    // backward-solve columns per thread
  constexpr int BW = CPT == 1 && NB == 32 ? 32 : 16;   // backward-solve block (<= NB: staged in W11)
  static_assert(BW <= NB, "backward blocks are staged in W11");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ml = lane & 15, kl = lane >> 4;
  for (int c0 = 0; c0 < NP; c0 += NB) {
    const int rt0 = c0 >> 4, nrt = NRT - rt0;
    const int nbe = NP - c0 < NB ? NP - c0 : NB;   // last panel of NP = 16 (2m+1): one tile column
    // (a) panel rows [c0, LDR) x cols [c0, c0 + NB): A - L[:, :c0] D L[c0:c0+NB, :c0]^T
    for (int gb = wave * MG; gb < nrt; gb += kSW * MG) {
      d4_t acc[MG][NCT];
#pragma unroll
      for (int m = 0; m < MG; ++m)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            acc[m][ct][r] = gb + m < nrt ? aorig(16 * (rt0 + gb + m) + kl + 4 * r, c0 + 16 * ct + ml) : 0.0;
      // k-steps (4 factored columns each) stream through a ring of PD register slots:
      // step s + PD is loaded while step s is multiplied (L comes from MALL/HBM)
      const int nst = c0 >> 2;
      double ra[PD][MG], rb[PD][NCT];
      auto ld = [&](int st, double (&a)[MG], double (&b)[NCT]) {
        const int kc = 4 * st + kl;
        const double* __restrict__ Lc = Ls + (int64_t)kc * LDR;
        const double dk = dd[kc];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) b[ct] = Lc[c0 + 16 * ct + ml] * dk;
#pragma unroll
        for (int m = 0; m < MG; ++m) a[m] = gb + m < nrt ? -Lc[16 * (rt0 + gb + m) + ml] : 0.0;
      };
#pragma unroll
      for (int d = 0; d < PD; ++d)
        if (d < nst) ld(d, ra[d], rb[d]);
      for (int s0 = 0; s0 < nst; s0 += PD) {
#pragma unroll
        for (int d = 0; d < PD; ++d) {
          if (s0 + d < nst) {
#pragma unroll
            for (int m = 0; m < MG; ++m)
              if (gb + m < nrt)
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) acc[m][ct] = mfma4(ra[d][m], rb[d][ct], acc[m][ct]);
            if (s0 + d + PD < nst) ld(s0 + d + PD, ra[d], rb[d]);
          }
        }
      }
#pragma unroll
      for (int m = 0; m < MG; ++m)
        if (gb + m < nrt)
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) P[(16 * (gb + m) + kl + 4 * r) * LDP + 16 * ct + ml] = acc[m][ct][r];
    }
    __syncthreads();
    // (b) diagonal block: lane r owns row r; right-looking LDL^T with readlane broadcasts
    if (wave == 0) {
      double a[NB];
#pragma unroll
      for (int t = 0; t < NB; ++t) a[t] = lane < nbe ? P[lane * LDP + t] : (lane == t ? 1.0 : 0.0);
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        // entries right of a lane's diagonal become garbage and are never read
        const double dj = readlane_d(a[j], j);
        const double f = lane > j ? a[j] / dj : 0.0;   // lane r > j: L[r][j]
#pragma unroll
        for (int t = j + 1; t < NB; ++t) a[t] = fma(-f, readlane_d(a[j], t), a[t]);
      }
      double dl = a[0];
#pragma unroll
      for (int t = 1; t < NB; ++t) dl = t == lane ? a[t] : dl;   // static indices only (no scratch)
      if (lane < nbe) {
        double* __restrict__ Wr = W11 + lane * NB;
#pragma unroll
        for (int t = 0; t < NB; ++t)
          if (t < lane) Wr[t] = a[t];
        dd[c0 + lane] = dl;
      }
      // L of the block (rows c0 + r > c0 + t): a[t] / d_t
#pragma unroll
      for (int t = 0; t < NB; ++t) {
        const double dt = readlane_d(dl, t);
        if (lane < nbe && t < lane) Ls[(int64_t)(c0 + t) * LDR + c0 + lane] = a[t] / dt;
      }
    }
    __syncthreads();
    // (c) rows below the block: u_j = A[r][j] - sum_{jj<j} L[r][jj] W11[j][jj],  L[r][j] = u_j / d_j
    for (int r = c0 + nbe + tid; r < LDR; r += kST) {
      double p[NB];
      const double* __restrict__ Pr = P + (r - c0) * LDP;
#pragma unroll
      for (int t = 0; t < NB; ++t) p[t] = Pr[t];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        double s = p[j];
        const double* __restrict__ Wj = W11 + j * NB;
#pragma unroll
        for (int jj = 0; jj < j; ++jj) s = fma(-p[jj], Wj[jj], s);
        p[j] = j < nbe ? s / dd[c0 + (j < nbe ? j : 0)] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < NB; ++j)
        if (j < nbe) Ls[(int64_t)(c0 + j) * LDR + r] = p[j];
    }
    __syncthreads();
  }
  // backward solve L^T x = y, y_c = L[NP][c]; BW-column blocks from the end.  Per block
  // one global round trip: the GEMV operands of the earlier columns and the block's
  // triangle (staged into W11) are loaded together, then the triangle (one wave, LDS)
  // and the GEMV update.
  double* __restrict__ xs = P;
  for (int c = tid; c < NP; c += kST) xs[c] = Ls[(int64_t)c * LDR + NP];
  for (int b0 = ((NP - 1) / BW) * BW; b0 >= 0; b0 -= BW) {
    const int bw = NP - b0 < BW ? NP - b0 : BW;
    double lv[CPT][BW];
#pragma unroll
    for (int cc = 0; cc < CPT; ++cc) {
      const int c = tid + cc * kST;
#pragma unroll
      for (int t = 0; t < BW; ++t) lv[cc][t] = (c < b0 && t < bw) ? Ls[(int64_t)c * LDR + b0 + t] : 0.0;
    }
    for (int e = tid; e < BW * BW; e += kST) {     // W11[c][t] = L[b0 + t][b0 + c], t > c
      const int cc = e / BW, t = e - cc * BW;
      W11[e] = (cc < bw && t < bw && t > cc) ? Ls[(int64_t)(b0 + cc) * LDR + b0 + t] : 0.0;
    }
    __syncthreads();
    if (wave == 0) {
      double val = lane < bw ? xs[b0 + lane] : 0.0;
      const double* __restrict__ Wc = W11 + (lane < BW ? lane : 0) * BW;
      for (int t = bw - 1; t >= 0; --t) {
        const double xt = readlane_d(val, t);
        if (lane < t) val = fma(-Wc[t], xt, val);
      }
      if (lane < bw) xs[b0 + lane] = val;
    }
    __syncthreads();
#pragma unroll
    for (int cc = 0; cc < CPT; ++cc) {
      const int c = tid + cc * kST;
      if (c < b0) {
        double s = xs[c];
#pragma unroll
        for (int t = 0; t < BW; ++t) s = fma(-lv[cc][t], xs[b0 + t], s);
        xs[c] = s;
      }
    }
    __syncthreads();
  }
}

}  // namespace

// ---- launchers of the kernel units, for the host side (bigk.hip).  (model, k) is a size of
// FIA_BIG_SIZES (else hipErrorInvalidValue); the buffers of the context are reserved by the
// caller; the batch's BigArgs are made from (c, qu, qi) ----
// bigk_prepare.hip
hipError_t launch_self(int64_t N, int64_t n_ent, const int64_t* ptr, int32_t* self, hipStream_t s);
hipError_t launch_check_cover(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, int32_t* flag,
                              hipStream_t s);
// per train row: the residual and (NCF) the layer-1 rows, weight fragments and g_mlp of both
// sides; marked: only the rows that the entities of c->mark read
hipError_t launch_big_rows(int model, int k, fia_ctx* c, bool marked, hipStream_t s);
// the Gram caches of side sd from its work lists (big_work_lists), split lists summed
hipError_t launch_big_gram(int model, int k, fia_ctx* c, int sd, hipStream_t s);
// bigk_solve.hip: the per-query work words and solve lists; the coupled systems of c->cpllist,
// one workgroup each; the records from a given x; the record headers and x_out
hipError_t launch_big_prologue(int model, int k, fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi,
                               hipStream_t s);
hipError_t launch_solve(int model, int k, fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, hipStream_t s);
hipError_t launch_big_record_x(int model, int k, fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi,
                               const double* x_in, hipStream_t s);
hipError_t launch_big_finish(int model, int k, fia_ctx* c, int64_t Q, double* x_out, hipStream_t s);
// bigk_solve_batched.hip: the side systems of c->syslist through the batched panel kernels
hipError_t launch_solve_batched(int model, int k, fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi,
                                hipStream_t s);
// bigk_score.hip: the work items of build_groups, timed by the dispatch itself (ps)
hipError_t launch_big_score(int model, int k, fia_ctx* c, const int32_t* qu, const int32_t* qi, int64_t max_chunks,
                            int32_t* rel_idx, double* influence, int K, PhaseSpan ps, hipStream_t s);

}  // namespace fia
