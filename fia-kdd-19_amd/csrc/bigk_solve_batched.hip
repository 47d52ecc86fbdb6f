// Large-k FIA path, the side systems of a batch factored together (the math and the
// structures: bigk.hip; the one-workgroup-per-system solve of the coupled queries:
// bigk_solve.hip).
#include "bigk.h"

namespace fia {
namespace {

typedef __attribute__((address_space(3))) void* lds_vp;         // LDS-DMA destination
typedef const __attribute__((address_space(1))) void* glb_vp;   // ... and its global source

// ------------------------------------------------------------------------------------
// Batched blocked LDL^T of the side systems (CPL = false).  The systems of a chunk are
// factored together, three launches per 64-column panel (NP % 64 != 0 ends in a
// narrower one), so thousands of independent workgroups keep every CU's memory
// pipeline busy -- the persistent one-workgroup-per-system kernel above spends most of
// its time waiting on its own panel chain.  Per system slab: L (column-major,
// LDR = NP + 16 rows, row NP the right-hand side v^T), d (NP), the current panel's
// diagonal block (64 x 64) and L11^-1 of every panel (64 x 64 each).
//   k_bs_dupd : the panel's diagonal block A - L D L^T (MFMA, k-steps split over four
//               waves);
//   k_bs_dfac : its LDL^T in one wave (readlane broadcasts), L11^-1 by forward
//               substitution (lane j: column j);
//   k_bs_trail: per 16-row tile below the block, the panel update (MFMA, L streamed)
//               and the triangular solve as one more MFMA product, P L11^-T D^-1;
//   k_bs_back : L^T x = y (y = row NP of L) by 64-column blocks from the end, each block's
//               triangle as a product with its stored L11^-1, and the scoring record.
// ------------------------------------------------------------------------------------
constexpr int kBsNB = 64;                          // panel width
constexpr int kBsMG = 2;                           // row tiles per k_bs_trail wave
constexpr int64_t kBsScratch = (int64_t)8 << 30;   // bytes of factor slabs per chunk

template <int NP>
__host__ __device__ constexpr int64_t bs_slab() {   // L, d, W, then L11^-1 of every panel
  return (int64_t)(NP + 16) * NP + NP + kBsNB * kBsNB + (int64_t)((NP + kBsNB - 1) / kBsNB) * kBsNB * kBsNB;
}

// Panel layout: when NP is not a multiple of 64 the NARROW panel comes first (columns
// [0, NP % 64)), then 64-column panels -- the narrow panel then has no update k-steps (no
// factored columns left of it), where as the last panel its k_bs_dupd / k_bs_trail were
// long single-wave chains over every earlier column for 16 columns of work (MF k = 256:
// 1.7 of 14 ms per batch).  Panel starting at column c0 keeps its L11^-1 in slot
// ceil(c0 / 64), so the first panel is slot 0 in both layouts.
__host__ __device__ constexpr int bs_first_panel(int NP) { return NP % kBsNB == 0 ? kBsNB : NP % kBsNB; }
__host__ __device__ constexpr int bs_panel_slot(int c0) { return (c0 + kBsNB - 1) / kBsNB; }


// one side system (mf:164-251 / ncf:193-280 restricted to one side): rows/cols [0, Ds)
// (2/n) A_e + wd M + damping I, identity padding to NP, row NP the right-hand side v
template <class M, int NP>
struct SideSys {
  const double* G;
  const double* vv;
  double s2n, wd, damping;
  // branch-free (every lane loads from a valid address, then selects), so the loads of
  // a tile's elements issue back to back instead of one exec-masked round trip each
  __device__ double at(int r, int c) const {
    const bool in = r < M::Ds && c < M::Ds;
    const int rr = in ? r : 0, cc = in ? c : 0;
    const int hi = rr > cc ? rr : cc, lo = rr > cc ? cc : rr;
    const double g = G[tile_off(M::T, hi >> 4, lo >> 4) * 256 + (hi & 15) + 16 * (lo & 15)];
    const double v = vv[c < NP ? c : NP - 1];
    const double h = s2n * g + (r == c ? (M::decayed(r) ? wd : 0.0) + damping : 0.0);
    // 0/1 weights rather than selects of the loaded values (a select lets the compiler
    // sink each load into its own exec-masked branch and wait on it there)
    const double fv = (r == NP && c < NP) ? 1.0 : 0.0, fh = (r < NP && in) ? 1.0 : 0.0;
    const double fp = (r < NP && !in && r == c) ? 1.0 : 0.0;
    return fma(fv, v, fma(fh, h, fp));
  }
};

template <class M, int NP>
__device__ __forceinline__ SideSys<M, NP> side_sys(const BigArgs& A, int code, const double* __restrict__ qwork) {
  constexpr int64_t GW = gram_words<M>();
  const int64_t q = code >> 1;
  const int sd = code & 1;
  const double* __restrict__ qw = qwork + q * M::QW;
  SideSys<M, NP> S;
  S.s2n = 2.0 / qw[M::Work::n];
  S.vv = M::Work::v(qw, sd);
  if (sd == 0) {
    const int32_t u = A.qu[q];
    S.G = A.gram[0] + (int64_t)(A.slot[0] ? A.slot[0][u] : u) * GW;
  } else {
    const int32_t i = A.qi[q];
    S.G = A.gram[1] + (int64_t)(A.slot[1] ? A.slot[1][i] : i) * GW;
  }
  S.wd = A.wd;
  S.damping = A.damping;
  return S;
}

// diagonal block of panel c0 (NBE = 64 columns, or NP's remainder for the last panel,
// identity-padded to 64): A - L[c0:c0+NBE, :c0] D L[c0:c0+NBE, :c0]^T (lower tiles
// (rt, ct <= rt); wave w takes k-steps w, w + 4, ... through a register ring), stored
// into the slab's W area for k_bs_dfac
template <class M, int NP, int NBE>
__global__ __launch_bounds__(256) void k_bs_dupd(BigArgs A, const int32_t* __restrict__ list, int w0, int c0,
                                                 const double* __restrict__ qwork, double* __restrict__ lscr) {
  constexpr int LDR = NP + 16, NB = kBsNB, LT = NB + 1, PD = 4, NT = NBE / 16;
  __shared__ double T[NB * LT];
  const int w = w0 + (int)blockIdx.x;
  if (w >= list[0]) return;
  const SideSys<M, NP> H = side_sys<M, NP>(A, list[1 + w], qwork);
  double* __restrict__ Ls = lscr + (int64_t)blockIdx.x * bs_slab<NP>();
  const double* __restrict__ dd = Ls + (int64_t)LDR * NP;
  double* __restrict__ Dg = Ls + (int64_t)LDR * NP + NP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ml = lane & 15, kl = lane >> 4;
#pragma unroll
  for (int i = 0; i < NB * NB / 256; ++i) {
    const int e = tid + 256 * i, r = e >> 6, cc = e & 63;
    T[r * LT + cc] = (r < NBE && cc < NBE) ? (cc <= r ? H.at(c0 + r, c0 + cc) : 0.0) : (r == cc ? 1.0 : 0.0);
  }
  d4_t acc[10];
#pragma unroll
  for (int t = 0; t < 10; ++t) acc[t] = d4_t{0.0, 0.0, 0.0, 0.0};
  const int nst = c0 >> 2;
  const int nmy = nst > wave ? (nst - wave + 3) >> 2 : 0;
  double ra[PD][NT], rd[PD];
  auto ld = [&](int m, double (&a)[NT], double& d) {
    const int k = 4 * (wave + 4 * m) + kl;
    const double* __restrict__ Lc = Ls + (int64_t)k * LDR + c0;
    d = dd[k];
#pragma unroll
    for (int rt = 0; rt < NT; ++rt) a[rt] = Lc[16 * rt + ml];
  };
#pragma unroll
  for (int d = 0; d < PD; ++d)
    if (d < nmy) ld(d, ra[d], rd[d]);
  for (int m0 = 0; m0 < nmy; m0 += PD) {
#pragma unroll
    for (int d = 0; d < PD; ++d) {
      if (m0 + d < nmy) {
        int t = 0;
#pragma unroll
        for (int rt = 0; rt < NT; ++rt) {
          const double a = -ra[d][rt] * rd[d];
#pragma unroll
          for (int ct = 0; ct <= rt; ++ct, ++t) acc[t] = mfma4(a, ra[d][ct], acc[t]);
        }
        if (m0 + d + PD < nmy) ld(m0 + d + PD, ra[d], rd[d]);
      }
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int wv = 0; wv < 4; ++wv) {
    if (wave == wv) {
      int t = 0;
#pragma unroll
      for (int rt = 0; rt < NT; ++rt)
#pragma unroll
        for (int ct = 0; ct <= rt; ++ct, ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) T[(16 * rt + kl + 4 * r) * LT + 16 * ct + ml] += acc[t][r];
    }
    __syncthreads();
  }
  for (int e = tid; e < NB * NB; e += 256) Dg[e] = T[(e & 63) * LT + (e >> 6)];   // column-major
}

// LDL^T of the updated diagonal block (one wave per system; lane r owns row r, readlane
// broadcasts, no LDS), L11 and d into the slab, then L11^-1 (lane j: column j by forward
// substitution) into the panel's X slot, XOR-swizzled: Xp[n][j ^ 4 (n & 7)] = (L11^-1)[n][j],
// so k_bs_trail's B-operand reads from its linear LDS copy are two-way at most.  The
// triangular solve needs W = L11^-T D^-1, i.e. W[j][n] = Xp[n][j] / d_n: k_bs_trail scales
// its product's columns; k_bs_back uses L11^-T itself.
template <class M, int NP, int NBE>
__global__ __launch_bounds__(64) void k_bs_dfac(const int32_t* __restrict__ list, int w0, int c0,
                                                double* __restrict__ lscr) {
  constexpr int LDR = NP + 16, NB = kBsNB;
  const int w = w0 + (int)blockIdx.x;
  if (w >= list[0]) return;
  double* __restrict__ Ls = lscr + (int64_t)blockIdx.x * bs_slab<NP>();
  double* __restrict__ dd = Ls + (int64_t)LDR * NP;
  double* __restrict__ W = dd + NP;
  const int lane = threadIdx.x;
  // only the NBE x NBE block is factored (a narrow panel: the chains are NBE long); the
  // inverse is identity-padded to 64 x 64 below.  Entries right of a lane's diagonal
  // become garbage and are never read
  double a[NBE];
#pragma unroll
  for (int t = 0; t < NBE; ++t) a[t] = W[t * NB + lane];     // block stored column-major
#pragma unroll
  for (int j = 0; j < NBE; ++j) {
    const double dj = readlane_d(a[j], j);
    const double f = lane > j ? a[j] / dj : 0.0;
#pragma unroll
    for (int t = j + 1; t < NBE; ++t) a[t] = fma(-f, readlane_d(a[j], t), a[t]);
  }
  double dl = a[0];
#pragma unroll
  for (int t = 1; t < NBE; ++t) dl = t == lane ? a[t] : dl;
  if (lane < NBE) dd[c0 + lane] = dl;
  const double rdl = 1.0 / dl;
#pragma unroll
  for (int t = 0; t < NBE; ++t) {                           // a[t] becomes L11[lane][t], t < lane
    a[t] = t < lane ? a[t] * readlane_d(rdl, t) : 0.0;
    if (t < lane && lane < NBE) Ls[(int64_t)(c0 + t) * LDR + c0 + lane] = a[t];
  }
  // lane j: column j of L11^-1 (x_m = 0 for m < j); lanes j >= NBE: identity columns
  double x[NBE];
#pragma unroll
  for (int i = 0; i < NBE; ++i) {
    double s = i == lane ? 1.0 : 0.0;
#pragma unroll
    for (int m = 0; m < i; ++m) s = fma(-readlane_d(a[m], i), x[m], s);
    x[i] = s;
  }
  double* __restrict__ Xp = W + NB * NB + (int64_t)bs_panel_slot(c0) * NB * NB;
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    double xn = n == lane ? 1.0 : 0.0;
    if constexpr (NBE < NB) {
#pragma unroll
      for (int i = 0; i < NBE; ++i) xn = n == i ? x[i] : xn;
    } else {
      xn = x[n < NBE ? n : 0];
    }
    Xp[n * NB + (lane ^ (4 * (n & 7)))] = xn;
  }
}

template <class M, int NP, int NBE>
__global__ __launch_bounds__(256) void k_bs_trail(BigArgs A, const int32_t* __restrict__ list, int w0, int c0,
                                                  int tpb, int nsys, const double* __restrict__ qwork,
                                                  double* __restrict__ lscr) {
  constexpr int LDR = NP + 16, NB = kBsNB, LT = NB + 1, MG = kBsMG, PDT = 5, NT = NBE / 16;
  __shared__ double Pw[4][16 * LT];
  __shared__ double Ws[NB * NB];
  // XCD-aware order: workgroups are dealt round-robin over the 8 XCDs, so physical block b
  // runs on XCD b % 8 (up to which XCD block 0 gets); all groups of system sys share the
  // XCD of block sys % 8, so the panel rows every group of a system reads (the B operand)
  // are one XCD's L2 lines instead of up to eight copies fetched by eight L2s
  const int xcd = (int)blockIdx.x & 7, jx = (int)blockIdx.x >> 3;
  const int sys = xcd + 8 * (jx / tpb), grp = jx % tpb;
  if (sys >= nsys) return;
  const int w = w0 + sys;
  if (w >= list[0]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ml = lane & 15, kl = lane >> 4;
  double* __restrict__ Ls = lscr + (int64_t)sys * bs_slab<NP>();
  const double* __restrict__ dd = Ls + (int64_t)LDR * NP;
  const double* __restrict__ W = dd + NP + NB * NB + (int64_t)bs_panel_slot(c0) * NB * NB;   // this panel's L11^-1
  // L11^-1 of this panel (k_bs_dfac) into LDS by DMA, landing while the panel update runs
#pragma unroll
  for (int i = 0; i < NB * NB / 512; ++i)
    __builtin_amdgcn_global_load_lds((glb_vp)(W + 2 * (i * 256 + tid)), (lds_vp)(Ws + 2 * (i * 256 + wave * 64)), 16,
                                     0, 0);
  const int R0 = c0 + NBE + 16 * MG * (4 * grp + wave);    // first row of this wave's tiles
  const bool active = R0 < LDR;
  const int ng = (LDR - R0) / 16 < MG ? (LDR - R0) / 16 : MG;
  const SideSys<M, NP> H = side_sys<M, NP>(A, list[1 + w], qwork);
  d4_t acc[MG][NT];
#pragma unroll
  for (int m = 0; m < MG; ++m)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[m][ct][r] = H.at(R0 + 16 * m + kl + 4 * r, c0 + NT * ml + ct);
  // panel update: k-steps (4 factored columns each) through a ring of PDT register slots.
  // Column j of product tile ct is panel column NT j + ct, so a lane's NT B values of a
  // k-step are consecutive doubles (two 16-B loads instead of four 8-B ones)
  const int nst = active ? c0 >> 2 : 0;
  double ra[PDT][MG], rb[PDT][NT], rd[PDT];
  auto ld = [&](int st, double (&a)[MG], double (&b)[NT], double& d) {
    const int k = 4 * st + kl;
    const double* __restrict__ Lc = Ls + (int64_t)k * LDR;
    d = dd[k];
#pragma unroll
    for (int m = 0; m < MG; ++m) a[m] = Lc[R0 + 16 * m + ml];     // rows past LDR: never used (m >= ng)
    if constexpr (NT % 2 == 0) {
#pragma unroll
      for (int ct = 0; ct < NT; ct += 2) {
        const double2 v = *reinterpret_cast<const double2*>(Lc + c0 + NT * ml + ct);
        b[ct] = v.x;
        b[ct + 1] = v.y;
      }
    } else {
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) b[ct] = Lc[c0 + NT * ml + ct];
    }
  };
#pragma unroll
  for (int d = 0; d < PDT; ++d)
    if (d < nst) ld(d, ra[d], rb[d], rd[d]);
  for (int s0 = 0; s0 < nst; s0 += PDT) {
#pragma unroll
    for (int d = 0; d < PDT; ++d) {
      if (s0 + d < nst) {
#pragma unroll
        for (int m = 0; m < MG; ++m) {
          const double a = -ra[d][m] * rd[d];
#pragma unroll
          for (int ct = 0; ct < NT; ++ct) acc[m][ct] = mfma4(a, rb[d][ct], acc[m][ct]);
        }
        if (s0 + d + PDT < nst) ld(s0 + d + PDT, ra[d], rb[d], rd[d]);
      }
    }
  }
  __syncthreads();   // W landed
  if (!active) return;
  // triangular solve: L[rows][panel] = P L11^-T D^-1 (upper triangular), through this
  // wave's LDS tile; column n of the product scaled by 1 / d_n
  double rdn[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) rdn[ct] = 1.0 / dd[c0 + 16 * ct + ml];
  double* __restrict__ P = Pw[wave];
#pragma unroll
  for (int m = 0; m < MG; ++m) {
    if (m >= ng) continue;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) P[(kl + 4 * r) * LT + NT * ml + ct] = acc[m][ct][r];
    wave_lds_sync();
    double pa[4 * NT];
#pragma unroll
    for (int s = 0; s < 4 * NT; ++s) pa[s] = P[ml * LT + 4 * s + kl];
    d4_t o[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
      o[ct] = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4 * ct + 4; ++s) o[ct] = mfma4(pa[s], Ws[(16 * ct + ml) * NB + ((4 * s + kl) ^ (4 * (ml & 7)))], o[ct]);
    }
    wave_lds_sync();
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) P[(kl + 4 * r) * LT + 16 * ct + ml] = o[ct][r] * rdn[ct];
    wave_lds_sync();
    const int Rm = R0 + 16 * m;
#pragma unroll
    for (int i = 0; i < NBE / 4; ++i) Ls[(int64_t)(c0 + kl + 4 * i) * LDR + Rm + ml] = P[ml * LT + kl + 4 * i];
    wave_lds_sync();
  }
}

template <class M, int NP>
__global__ __launch_bounds__(512) void k_bs_back(BigArgs A, const int32_t* __restrict__ list, int w0,
                                                 const double* __restrict__ qwork, double* __restrict__ lscr,
                                                 double* __restrict__ xb, double* __restrict__ rec) {
  constexpr int K = M::K, NPs = M::NPs, Ds = M::Ds, LDR = NP + 16, kST = 512, kSW = kST / 64, NB = kBsNB;
  __shared__ double xs[NP + NB];       // zero past NP: a partial last block reads it unguarded
  __shared__ double red[64];
  const int w = w0 + (int)blockIdx.x;
  if (w >= list[0]) return;
  const int code = list[1 + w];
  const int64_t q = code >> 1;
  const int sd = code & 1;
  const double* __restrict__ qw = qwork + q * M::QW;
  const double* __restrict__ Ls = lscr + (int64_t)blockIdx.x * bs_slab<NP>();
  const double* __restrict__ X = Ls + (int64_t)LDR * NP + NP + NB * NB;
  const int tid = threadIdx.x;
  // L^T x = y, y_c = L[NP][c].  Per panel b from the end (64 columns; a narrow first
  // panel, bs_first_panel): x_b = L_bb^-T z_b with the panel's stored inverse (z_b: y_b after
  // the later blocks' updates), then z_c -= sum_t L[b0 + t][c] x_b[t] for every earlier c.
  // One global round trip per block.
  for (int c = tid; c < NP + NB; c += kST) xs[c] = c < NP ? Ls[(int64_t)c * LDR + NP] : 0.0;
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  for (int b0 = NP - NB, bend = NP; bend > 0; bend = b0, b0 -= NB) {
    const int bw = b0 < 0 ? bend : NB;
    b0 = b0 < 0 ? 0 : b0;
    if (tid < bw) {
      // (L^-T)[c][n] = (L^-1)[n][c], zero for n < c and (identity padding) for n >= bw
      // (the padding's off-diagonal blocks are zero, so z entries past the block drop out)
      const double* __restrict__ Xb = X + (int64_t)bs_panel_slot(b0) * NB * NB;
      double xc = 0.0;
#pragma unroll 8
      for (int n = 0; n < NB; ++n) xc = fma(Xb[n * NB + (tid ^ (4 * (n & 7)))], xs[b0 + n], xc);
      __builtin_amdgcn_wave_barrier();   // (wave 0 only) every lane has read the block's z
      xs[b0 + tid] = xc;
    }
    __syncthreads();
    // z_c -= L[b0:b0+bw][c] . x_b: a column per wave step, lane t on row b0 + t (one
    // coalesced 512-B read per column), eight columns in flight
    const double xt = lane < bw ? xs[b0 + lane] : 0.0;
    for (int c0 = 8 * wave; c0 < b0; c0 += 8 * kSW) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int c = c0 + u;
        v[u] = (c < b0 && lane < bw) ? Ls[(int64_t)c * LDR + b0 + lane] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const double sum = wave_sum(v[u] * xt);
        if (lane == 0 && c0 + u < b0) xs[c0 + u] -= sum;
      }
    }
    __syncthreads();
  }
  // padded solution, this side's partial sums and scoring record (as k_big_solve)
  const int32_t u = A.qu[q], i = A.qi[q];
  const double* __restrict__ vsd = M::Work::v(qw, sd);
  const double* __restrict__ th = M::Work::theta(qw, sd);
  double* __restrict__ xo = xb + q * 2 * NPs + sd * NPs;
  double cq = 0.0, xv = 0.0;
  for (int a = tid; a < NPs; a += kST) {
    const double xa = xs[a];
    xo[a] = xa;
    if (a < Ds) {
      if (M::decayed(a)) cq = fma(xa, th[a], cq);
      xv = fma(xa, vsd[a], xv);
    }
  }
  cq = bsum<kSW>(cq, red);
  xv = bsum<kSW>(xv, red);
  double* __restrict__ R = rec + q * M::R;
  using L = typename M::Rec;
  double* __restrict__ S = L::side(R, sd);
  if (tid == 0) {
    R[L::cq_of(sd)] = A.wd * cq;
    R[L::xv_of(sd)] = xv;
  }
  if constexpr (!M::ncf) {
    for (int a = tid; a <= K; a += kST) S[L::x + a] = xs[a];
  } else {
    for (int c = tid; c < K; c += kST) {
      S[L::x_mlp + c] = xs[c];
      S[L::w3g_x_gmf + c] = (double)A.t[8][M::H + c] * xs[K + c];
    }
  }
  if (tid == 0) S[L::dup_other] = (double)(sd ? u : i);
}

// the three launches of the panel at column c0 for systems [w0, w0 + n) of the list
template <class M, int NP, int NBE>
hipError_t launch_bs_panel(fia_ctx* c, const BigArgs& A, int64_t w0, int64_t n, int c0, const int32_t* list,
                           hipStream_t s) {
  hipLaunchKernelGGL((k_bs_dupd<M, NP, NBE>), dim3((unsigned)n), dim3(256), 0, s, A, list, (int)w0, c0,
                     c->qwork.as<double>(), c->lscr.as<double>());
  FIA_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL((k_bs_dfac<M, NP, NBE>), dim3((unsigned)n), dim3(64), 0, s, list, (int)w0, c0,
                     c->lscr.as<double>());
  FIA_HIP_TRY(hipGetLastError());
  const int tiles = (NP + 16 - c0 - NBE) / 16;
  const int tpb = (tiles + 4 * kBsMG - 1) / (4 * kBsMG);
  hipLaunchKernelGGL((k_bs_trail<M, NP, NBE>), dim3((unsigned)(8 * ((n + 7) / 8) * tpb)), dim3(256), 0, s, A, list,
                     (int)w0, c0, tpb, (int)n, c->qwork.as<double>(), c->lscr.as<double>());
  return hipGetLastError();
}

// chunks of <= kBsScratch bytes of slabs; list[0] (the device-side count) bounds every launch,
// max_sys only sizes them
template <class M, int NP>
hipError_t solve_batched(fia_ctx* c, const BigArgs& A, int64_t max_sys, const int32_t* list, hipStream_t s) {
  static_assert(NP % 16 == 0, "side blocks are whole 16-column tiles");
  constexpr int kFirst = bs_first_panel(NP);   // first panel's width
  constexpr int64_t slab = bs_slab<NP>();
  int64_t S = kBsScratch / (int64_t)(sizeof(double) * slab);
  S = S < 1 ? 1 : (S > max_sys ? max_sys : S);
  FIA_HIP_TRY(c->lscr.reserve(sizeof(double) * (size_t)(S * slab), s));
  for (int64_t w0 = 0; w0 < max_sys; w0 += S) {
    const int64_t n = max_sys - w0 < S ? max_sys - w0 : S;
    // the narrow panel (if any) first, then 64-column panels (bs_first_panel)
    FIA_HIP_TRY((launch_bs_panel<M, NP, kFirst>(c, A, w0, n, 0, list, s)));
    for (int c0 = kFirst; c0 < NP; c0 += kBsNB) FIA_HIP_TRY((launch_bs_panel<M, NP, kBsNB>(c, A, w0, n, c0, list, s)));
    hipLaunchKernelGGL((k_bs_back<M, NP>), dim3((unsigned)n), dim3(512), 0, s, A, list, (int)w0,
                       c->qwork.as<double>(), c->lscr.as<double>(), c->xb.as<double>(), c->rec.as<double>());
    FIA_HIP_TRY(hipGetLastError());
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_solve_batched(int model, int k, fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi,
                                hipStream_t s) {
  if (Q <= 0) return hipSuccess;
  const BigArgs A = make_big_args(c, qu, qi);
  return big_dispatch(model, k, [&](auto m) {
    using M = decltype(m);
    return solve_batched<M, M::NPs>(c, A, 2 * Q, c->syslist.as<int32_t>(), s);
  });
}

}  // namespace fia
