// Large-k FIA path, the prepare phase (the math and the structures: bigk.hip): per list
// position its entity (k_self), per train row the residual and (NCF) the restricted MLP
// gradient of both sides (k_resid_mf / k_l1_big, k_ncf_wfrag, k_ncf_rows), per entity the
// tile-packed Gram cache on the f64 matrix cores (k_big_gram, k_big_combine), and the cover
// check of a query set after fia_prepare_for (k_check_cover).
#include "bigk.h"

namespace fia {
namespace {

__global__ void k_check_cover(int64_t Q, const int32_t* __restrict__ qu, const int32_t* __restrict__ qi, int64_t U,
                              int64_t I, const int32_t* __restrict__ slot0, const int32_t* __restrict__ slot1,
                              int32_t* __restrict__ flag) {
  int bad = 0;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < Q; q += (int64_t)gridDim.x * blockDim.x) {
    const int32_t u = qu[q], i = qi[q];
    if (u >= 0 && u < U && i >= 0 && i < I) bad |= slot0[u] < 0 || slot1[i] < 0;
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// per-position entity of a side's lists: self[p] = e with ptr[e] <= p < ptr[e+1]
// ------------------------------------------------------------------------------------
__global__ void k_self(int64_t N, int64_t n_ent, const int64_t* __restrict__ ptr, int32_t* __restrict__ self) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (int64_t)gridDim.x * blockDim.x) {
    self[p] = (int32_t)last_at_most(ptr, (int64_t)0, n_ent, p);
  }
}

// MF residual by train row (user-major pass): e_j = p_u.q_i + b_u + b_i + g - y_j (mf:89-116).
// fia_prepare_for (mark != nullptr): only the rows the shard's scoring reads -- those in a
// cached user's or a cached item's list (a query (u, i) scores exactly the lists of u and i)
template <int K>
__global__ void k_resid_mf(int64_t N, const int32_t* __restrict__ self0, const int32_t* __restrict__ other0,
                           const int32_t* __restrict__ row0, const float* __restrict__ rat0,
                           const float* __restrict__ P, const float* __restrict__ Qt, const float* __restrict__ bu,
                           const float* __restrict__ bi, const float* __restrict__ gb, double* __restrict__ resid,
                           const uint8_t* __restrict__ mark, int64_t U) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (int64_t)gridDim.x * blockDim.x) {
    const int32_t u = self0[p], i = other0[p];
    if (mark && !mark[u] && !mark[U + i]) continue;
    const float4* a = reinterpret_cast<const float4*>(P + (int64_t)u * K);
    const float4* b = reinterpret_cast<const float4*>(Qt + (int64_t)i * K);
    double acc = 0.0;
#pragma unroll 8
    for (int c = 0; c < K / 4; ++c) {
      const float4 x = a[c], y = b[c];
      acc = fma((double)x.x, (double)y.x, acc);
      acc = fma((double)x.y, (double)y.y, acc);
      acc = fma((double)x.z, (double)y.z, acc);
      acc = fma((double)x.w, (double)y.w, acc);
    }
    resid[row0[p]] = acc + (double)bu[u] + (double)bi[i] + (double)gb[0] - (double)rat0[p];
  }
}

// NCF layer-1 halves L1[e] = emb_e . W1[row_off : row_off + k]  (fp64)
template <int K>
__global__ void k_l1_big(const float* __restrict__ emb, const float* __restrict__ W1, int row_off, int64_t n_ent,
                         double* __restrict__ out) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_ent * K;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = t / K;
    const int c = (int)(t % K);
    const float* x = emb + e * K;
    double acc = 0.0;
    for (int a = 0; a < K; ++a) acc = fma((double)x[a], (double)W1[(int64_t)(row_off + a) * K + c], acc);
    out[t] = acc;
  }
}

// NCF per train row (one 4-wave workgroup per 16 list positions of side `pass`; the
// waves split each product's output tiles), all products on the f64 matrix cores
// (ncf:102-145, TF ReluGrad masks):
//   z1 = L1u + L1i + b1,  z2 = relu(z1) W2 + b2,  d2 = 1[z2>0] W3m,
//   d1 = 1[z1>0] (W2 d2),  r-hat = W3m.relu(z2) + W3g.(Pg_u*Qg_i) + b3
// pass < 0 (full prepare): user-major positions, g_mlp of both sides for every row.
// pass = sd (fia_prepare_for): side sd's positions, tiles without a cached entity's row
// skipped, g_mlp of side sd only -- a cached entity's list is one contiguous run of its
// side's positions, so the work is dense.  A row in both kinds of list gets its
// residual from both passes: the same arithmetic, the same bits.
constexpr int kRowWaves = 4;

// The MLP weights as f64 MFMA B-operand fragments, built once per prepare (3 k^2 doubles,
// L2-resident): fragment (t, p) of a product is 64 lanes x 2 doubles, lane (ml, kl)
// holding the weights of output column 16t + ml at reduction indices 8p + 2kl + {0, 1}
// (the A operand reads the same two indices as one 16-B LDS word), so every B load of
// k_ncf_rows is one contiguous 1-KB dwordx4 wave load covering two MFMAs instead of
// sixteen scattered 16-B row pieces and a convert per MFMA.
//   [0, HK)        z2 = relu(z1) W2:  W2[kidx][col]      t < H/16, p < K/8
//   [HK, 2HK)      W2 d2:             W2[col][kidx]      t < K/16, p < H/8
//   [2HK, 2HK+2K^2) g_mlp, side sd:   W1[sd K + col][kidx] t < K/16, p < K/8
template <int K>
__global__ void k_ncf_wfrag(const float* __restrict__ W1, const float* __restrict__ W2, double* __restrict__ wf) {
  constexpr int H = K / 2;
  constexpr int64_t n = (int64_t)3 * K * K;
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n; f += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(f & 1), lane = (int)((f >> 1) & 63);
    const int64_t tp = f >> 7;   // fragment index (t, p) within its product
    const int ml = lane & 15, kl = lane >> 4;
    double x;
    if (f < (int64_t)H * K) {
      const int t = (int)(tp / (K / 8)), p = (int)(tp % (K / 8));
      x = W2[(8 * p + 2 * kl + i) * H + 16 * t + ml];
    } else if (f < (int64_t)2 * H * K) {
      const int64_t q = tp - (int64_t)H * K / 128;
      const int t = (int)(q / (H / 8)), p = (int)(q % (H / 8));
      x = W2[(16 * t + ml) * H + 8 * p + 2 * kl + i];
    } else {
      const int64_t q = tp - (int64_t)2 * H * K / 128;
      const int sd = (int)(q / (K / 16 * (K / 8)));
      const int64_t r = q % (K / 16 * (K / 8));
      const int t = (int)(r / (K / 8)), p = (int)(r % (K / 8));
      x = W1[(int64_t)(sd * K + 16 * t + ml) * K + 8 * p + 2 * kl + i];
    }
    wf[f] = x;
  }
}

template <int K>
__global__ __launch_bounds__(64 * kRowWaves) void k_ncf_rows(
    int64_t N, int pass, const int32_t* __restrict__ self0, const int32_t* __restrict__ other0,
    const int32_t* __restrict__ row0, const float* __restrict__ rat0, const double* __restrict__ l1u,
    const double* __restrict__ l1i, const float* __restrict__ b1, const float* __restrict__ W2,
    const float* __restrict__ b2, const float* __restrict__ W3, const float* __restrict__ b3,
    const float* __restrict__ Pg, const float* __restrict__ Qg, const double2* __restrict__ wf,
    double* __restrict__ gm0, double* __restrict__ gm1, double* __restrict__ resid,
    const uint8_t* __restrict__ mark, int64_t U) {
  constexpr int H = K / 2, LZ = K + 4, LD2 = H + 4, NW = kRowWaves;
  __shared__ __attribute__((aligned(16))) double Z1[16 * LZ];
  __shared__ __attribute__((aligned(16))) double D2[16 * LD2];
  const double2* __restrict__ Fz2 = wf;
  const double2* __restrict__ Fd1 = wf + H * K / 2;
  const double2* __restrict__ Fg = wf + H * K;
  __shared__ double part_mlp[NW][16];
  __shared__ double part_gmf[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ml = lane & 15, kl = lane >> 4;
  for (int64_t tile = blockIdx.x; tile * 16 < N; tile += gridDim.x) {
    const int64_t p0 = tile * 16;
    const int64_t my = p0 + ml;
    const bool v = my < N;
    const int32_t s_l = v ? self0[my] : 0, o_l = v ? other0[my] : 0, j_l = v ? row0[my] : 0;
    const int32_t u_l = pass == 1 ? o_l : s_l, i_l = pass == 1 ? s_l : o_l;
    // fia_prepare_for: g_mlp of a side is needed only for rows in a cached entity's list
    const bool need_u = v && pass != 1 && (!mark || mark[u_l]);
    const bool need_i = v && pass != 0 && (!mark || mark[U + i_l]);
    const bool any_u = __any(need_u), any_i = __any(need_i);
    if (pass >= 0 && !(any_u || any_i)) continue;   // uniform over the workgroup (same tile)
    __syncthreads();
    for (int e = tid; e < 16 * K; e += 64 * NW) {
      const int r = e / K, c = e % K;
      const int32_t u = __shfl(u_l, r), i = __shfl(i_l, r);
      Z1[r * LZ + c] = l1u[(int64_t)u * K + c] + l1i[(int64_t)i * K + c] + (double)b1[c];
    }
    __syncthreads();
    double mlp[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = w; t < H / 16; t += NW) {
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
      const double2* __restrict__ fb = Fz2 + t * (K / 8) * 64 + lane;
#pragma unroll 4
      for (int p = 0; p < K / 8; ++p) {
        const double2 z = *reinterpret_cast<const double2*>(Z1 + ml * LZ + 8 * p + 2 * kl);
        const double2 b = fb[64 * p];
        acc = mfma4(z.x > 0.0 ? z.x : 0.0, b.x, acc);
        acc = mfma4(z.y > 0.0 ? z.y : 0.0, b.y, acc);
      }
      const int d = 16 * t + ml;
      const double w3m = (double)W3[d], bb = (double)b2[d];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double z2 = acc[r] + bb;
        const bool on = z2 > 0.0;
        mlp[r] += on ? w3m * z2 : 0.0;
        D2[(kl + 4 * r) * LD2 + d] = on ? w3m : 0.0;
      }
    }
    // this wave's MLP partial of row kl + 4r sits in lane 16 kl after the reduction
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double m = mlp[r];
      m += __shfl_xor(m, 1);
      m += __shfl_xor(m, 2);
      m += __shfl_xor(m, 4);
      m += __shfl_xor(m, 8);
      if (ml == 0) part_mlp[w][kl + 4 * r] = m;
    }
    // gmf dot of rows w, w + NW, ... (wave-wide over the k coordinates)
    for (int r = w; r < 16; r += NW) {
      const int32_t u = __shfl(u_l, r), i = __shfl(i_l, r);
      double part = 0.0;
      for (int c = lane; c < K; c += 64)
        part = fma((double)W3[H + c] * (double)Pg[(int64_t)u * K + c], (double)Qg[(int64_t)i * K + c], part);
      part = wave_sum(part);
      if (lane == 0) part_gmf[r] = part;
    }
    __syncthreads();
    for (int t = w; t < K / 16; t += NW) {
      d4_t acc = {0.0, 0.0, 0.0, 0.0};
      const double2* __restrict__ fb = Fd1 + t * (H / 8) * 64 + lane;
#pragma unroll 4
      for (int p = 0; p < H / 8; ++p) {
        const double2 a = *reinterpret_cast<const double2*>(D2 + ml * LD2 + 8 * p + 2 * kl);
        const double2 b = fb[64 * p];
        acc = mfma4(a.x, b.x, acc);
        acc = mfma4(a.y, b.y, acc);
      }
      const int c = 16 * t + ml;
#pragma unroll
      for (int r = 0; r < 4; ++r) {           // Z1 becomes D1 (each lane rewrites what it read)
        double* z = Z1 + (kl + 4 * r) * LZ + c;
        *z = *z > 0.0 ? acc[r] : 0.0;
      }
    }
    __syncthreads();
    // g_mlp of both sides: D1 . W1_side^T (W1 rows [0, k) act on Pm, rows [k, 2k) on Qm)
#pragma unroll 1
    for (int sd = 0; sd < 2; ++sd) {
      if (!(sd ? any_i : any_u)) continue;
      double* __restrict__ gm = sd ? gm1 : gm0;
      for (int t = w; t < K / 16; t += NW) {
        d4_t acc = {0.0, 0.0, 0.0, 0.0};
        const double2* __restrict__ fb = Fg + (sd * (K / 16) + t) * (K / 8) * 64 + lane;
#pragma unroll 4
        for (int p = 0; p < K / 8; ++p) {
          const double2 a = *reinterpret_cast<const double2*>(Z1 + ml * LZ + 8 * p + 2 * kl);
          const double2 b = fb[64 * p];
          acc = mfma4(a.x, b.x, acc);
          acc = mfma4(a.y, b.y, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = kl + 4 * r;
          const int32_t j = __shfl(j_l, row);
          if (p0 + row < N) gm[(int64_t)j * K + 16 * t + ml] = acc[r];
        }
      }
    }
    if (w == 0 && lane < 16 && v) {
      double m = 0.0;
#pragma unroll
      for (int q = 0; q < NW; ++q) m += part_mlp[q][lane];
      resid[j_l] = m + part_gmf[lane] + (double)b3[0] - (double)rat0[my];
    }
  }
}

// ------------------------------------------------------------------------------------
// Entity Gram caches on the f64 matrix cores.  A workgroup (8 waves) takes one slice
// (<= kBigSlice ratings) of one entity's list and one group of output tiles; per
// 16 ratings it stages the g rows in LDS (MF: the gathered other-side embedding + 1;
// NCF: W1_side . d1_j by MFMA + W3g * gmf_other) and every wave adds the rank-16
// update of its tiles (4 MFMAs per tile).
// ------------------------------------------------------------------------------------
constexpr int kGW = 8;              // waves per Gram workgroup

template <class M>
struct GramCfg {
  static constexpr int NTL = M::T * (M::T + 1) / 2;
  // accumulator tiles per wave (NCF: fewer, for the prefetched slab registers)
  static constexpr int MAXPER = M::ncf ? 14 : 18;
  static constexpr int NG = (NTL + kGW * MAXPER - 1) / (kGW * MAXPER);  // tile groups (workgroups per slice)
  static constexpr int TPG = (NTL + NG - 1) / NG;
  static constexpr int PER = (TPG + kGW - 1) / kGW;
  static constexpr int LDT = 18;            // NCF slab: coordinate-major, 16 ratings + 2 pad
  static constexpr int LDG = M::NPs + 16;   // MF slab: rating-major row stride (doubles)
  static constexpr int SLAB = M::ncf ? M::NPs * LDT : 16 * LDG;
};

// One staging thread's share of a 16-rating slab, loaded into registers one slab ahead and
// written to LDS as f64.  MF: the gathered other-side embedding, then the constant 1 of
// the bias coordinate, rating-major; NCF: g_mlp,j of the side (precomputed by k_ncf_rows),
// then W3g * gmf_other, coordinate-major (slab[coord * LDT + rating]: a lane's two ratings
// of an MFMA pair are one 16-B read, and the 16 lanes of a coordinate write 32 consecutive
// dwords; config-5 NCF prepare 114.7 -> 107.1 ms, same-box A/B; at MF k = 256 it measured
// 20.1 vs 19.4 ms and MF keeps the rating-major slab)
template <class M, bool NCF = M::ncf>
struct GramStage;

template <class M>
struct GramStage<M, false> {   // rating-major: row r of the slab, coordinates pp * PERT + [0, PERT)
  static constexpr int K = M::K, PERT = K / 32, LDG = GramCfg<M>::LDG;
  float4 x[PERT / 4];
  bool valid;
  __device__ void fetch(const int32_t* __restrict__ other, const int32_t*, const float* __restrict__ emb,
                        const double*, int64_t pos, int r, int rem, int pp) {
    valid = r < rem;
    const int32_t o = valid ? other[pos + r] : 0;
    const float4* src = reinterpret_cast<const float4*>(emb + (int64_t)o * K + pp * PERT);
#pragma unroll
    for (int c = 0; c < PERT / 4; ++c) x[c] = src[c];
  }
  __device__ void put(double* __restrict__ G, const double*, int r, int pp) const {
    double* row = G + r * LDG;
#pragma unroll
    for (int c = 0; c < PERT / 4; ++c) {
      double* d = row + pp * PERT + 4 * c;
      d[0] = valid ? (double)x[c].x : 0.0;
      d[1] = valid ? (double)x[c].y : 0.0;
      d[2] = valid ? (double)x[c].z : 0.0;
      d[3] = valid ? (double)x[c].w : 0.0;
    }
    if (pp < 16) row[K + pp] = (pp == 0 && valid) ? 1.0 : 0.0;
  }
};

template <class M>
struct GramStage<M, true> {
  static constexpr int K = M::K, PERT = K / 32, LDT = GramCfg<M>::LDT;
  double m[PERT];
  float g[PERT];
  bool valid;
  __device__ void fetch(const int32_t* __restrict__ other, const int32_t* __restrict__ rowid,
                        const float* __restrict__ emb, const double* __restrict__ gms, int64_t pos, int r, int rem,
                        int q) {
    valid = r < rem;
    const int32_t o = valid ? other[pos + r] : 0;
    const int32_t j = valid ? rowid[pos + r] : 0;
    const double* msrc = gms + (int64_t)j * K + q * PERT;
    const float* gsrc = emb + (int64_t)o * K + q * PERT;
#pragma unroll
    for (int c = 0; c < PERT; ++c) {
      m[c] = msrc[c];
      g[c] = gsrc[c];
    }
  }
  __device__ void put(double* __restrict__ G, const double* __restrict__ w3g, int r, int q) const {
    double* d = G + q * PERT * LDT + r;
#pragma unroll
    for (int c = 0; c < PERT; ++c) {
      d[c * LDT] = valid ? m[c] : 0.0;
      d[(K + c) * LDT] = valid ? w3g[q * PERT + c] * (double)g[c] : 0.0;
    }
  }
};

template <class M>
__global__ __launch_bounds__(64 * kGW) void k_big_gram(int sd, int64_t n_items, const int32_t* __restrict__ items,
                                                       const int64_t* __restrict__ ptr,
                                                       const int32_t* __restrict__ other,
                                                       const int32_t* __restrict__ rowid,
                                                       const float* __restrict__ emb_other,
                                                       const double* __restrict__ gms, const float* __restrict__ W3,
                                                       double* __restrict__ gram, double* __restrict__ part) {
  using C = GramCfg<M>;
  constexpr int T = M::T, LDT = C::LDT, LDG = C::LDG, PER = C::PER;
  constexpr int64_t GW = gram_words<M>();
  // two slab buffers: slab n is written to Gs[n & 1] while the waves may still read slab
  // n - 1 from the other one, so one barrier per slab, and the next slab's global loads
  // are issued before this slab's MFMAs (they land while the matrix cores run)
  __shared__ __attribute__((aligned(16))) double Gs[2][C::SLAB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ml = lane & 15, kl = lane >> 4;
  // NG > 2 (NCF k = 256): XCD-aware order -- block b runs on XCD b % 8 and the NG tile
  // groups of one slice are blocks 8 apart (same XCD, dispatched together), so a slab's
  // gathered rows come from HBM once per slice instead of once per group; gridDim.x is a
  // multiple of 8 NG, so a block keeps its group (config-5 NCF prepare 117.0 -> 115.3 ms;
  // at NG = 2, MF k = 256, the plain 2-D grid measured faster: 19.5 vs 20.4 ms)
  constexpr bool XG = C::NG > 2;
  const int grp = XG ? (int)((blockIdx.x >> 3) % C::NG) : (int)blockIdx.y;
  const int64_t n_vb = XG ? ((n_items + 7) / 8) * 8 * C::NG : n_items;
  // staging thread: rating r, coordinate chunk q (NCF: 16 lanes per coordinate; MF: 32
  // threads per rating row)
  const int r = M::ncf ? tid & 15 : tid >> 5, q = M::ncf ? tid >> 4 : tid & 31;
  __shared__ double w3g[M::ncf ? M::K : 1];   // NCF: W3's GMF weights (f64) for the staging
  if constexpr (M::ncf)
    for (int c = tid; c < M::K; c += 64 * kGW) w3g[c] = (double)W3[M::H + c];
  __syncthreads();
  GramStage<M> stage;
  const int tend = (grp + 1) * C::TPG < C::NTL ? (grp + 1) * C::TPG : C::NTL;
  int tr_[PER], tc_[PER];
  bool on_[PER];
#pragma unroll
  for (int p = 0; p < PER; ++p) {
    const int idx = grp * C::TPG + wave * PER + p;
    on_[p] = idx < tend;
    int tr = 0;
    while ((tr + 1) * (tr + 2) / 2 <= idx) ++tr;
    tr_[p] = on_[p] ? tr : 0;
    tc_[p] = on_[p] ? idx - tr * (tr + 1) / 2 : 0;
  }
  // a slot past the group's last tile (on_ false) computes tile (0, 0) and is not stored:
  // a few % more MFMAs instead of a scalar branch in front of every one
  int buf = 0;
  for (int64_t vb = blockIdx.x; vb < n_vb; vb += gridDim.x) {
    const int64_t it = XG ? 8 * (vb / (8 * C::NG)) + (vb & 7) : vb;
    if (it >= n_items) continue;   // uniform over the block
    const int32_t e = items[4 * it], start = items[4 * it + 1], len = items[4 * it + 2], dst = items[4 * it + 3];
    const int64_t lb = ptr[e] + start;
    d4_t acc[PER];
#pragma unroll
    for (int p = 0; p < PER; ++p) acc[p] = d4_t{0.0, 0.0, 0.0, 0.0};
    stage.fetch(other, rowid, emb_other, gms, lb, r, len, q);
    for (int t0 = 0; t0 < len; t0 += 16, buf ^= 1) {
      double* __restrict__ G = Gs[buf];
      stage.put(G, w3g, r, q);
      __syncthreads();
      if (t0 + 16 < len) stage.fetch(other, rowid, emb_other, gms, lb + t0 + 16, r, len - t0 - 16, q);
      // MFMA pair h: lane (m, g) supplies ratings 8h + 2g and 8h + 2g + 1 of coordinate
      // 16 tr + m (A) / 16 tc + m (B), one 16-B read each
      if constexpr (M::ncf) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const double* gc = G + ml * LDT + 8 * h + 2 * kl;
#pragma unroll
          for (int p = 0; p < PER; ++p) {
            const double2 a = *reinterpret_cast<const double2*>(gc + 16 * LDT * tr_[p]);
            const double2 b = *reinterpret_cast<const double2*>(gc + 16 * LDT * tc_[p]);
            acc[p] = mfma4(a.x, b.x, acc[p]);
            acc[p] = mfma4(a.y, b.y, acc[p]);
          }
        }
      } else {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          const double* gr = G + (4 * s4 + kl) * LDG + ml;
#pragma unroll
          for (int p = 0; p < PER; ++p) acc[p] = mfma4(gr[16 * tr_[p]], gr[16 * tc_[p]], acc[p]);
        }
      }
    }
    double* out = dst >= 0 ? gram + (int64_t)dst * GW : part + (int64_t)(-dst - 1) * GW;
#pragma unroll
    for (int p = 0; p < PER; ++p) {
      if (!on_[p]) continue;
      double* tb = out + (int64_t)tile_off(T, tr_[p], tc_[p]) * 256 + 16 * ml;
#pragma unroll
      for (int r = 0; r < 4; ++r) tb[kl + 4 * r] = acc[p][r];
    }
  }
}

// partial Grams of a long list summed in slot order; blockIdx.y splits the GW words so a
// handful of long lists still spreads over every CU
constexpr int kCombSplit = 64;
__global__ void k_big_combine(int64_t n_comb, const int32_t* __restrict__ comb, int64_t GW,
                              const double* __restrict__ part, double* __restrict__ gram) {
  const int64_t per = (GW + kCombSplit - 1) / kCombSplit;
  const int64_t t0 = (int64_t)blockIdx.y * per, t1 = t0 + per < GW ? t0 + per : GW;
  for (int64_t w = blockIdx.x; w < n_comb; w += gridDim.x) {
    const int32_t gs = comb[4 * w], first = comb[4 * w + 1], ns = comb[4 * w + 2];
    const double* __restrict__ src = part + (int64_t)first * GW;
    for (int64_t t = t0 + threadIdx.x; t < t1; t += blockDim.x) {
      double s = 0.0;
      for (int k = 0; k < ns; ++k) s += src[(int64_t)k * GW + t];
      gram[(int64_t)gs * GW + t] = s;
    }
  }
}

template <class M>
hipError_t big_rows(fia_ctx* c, bool marked, hipStream_t s) {
  constexpr int K = M::K;
  const Index& X = c->idx;
  const int64_t N = X.N, n_ent[2] = {c->p.U, c->p.I};
  const uint8_t* mark = marked ? c->mark.as<uint8_t>() : nullptr;
  if constexpr (!M::ncf) {
    if (N > 0) {
      hipLaunchKernelGGL(k_resid_mf<K>, dim3(grid_cap((N + 255) / 256, 16384)), dim3(256), 0, s, N,
                         c->self[0].as<int32_t>(), X.side[0].other.as<int32_t>(), X.side[0].row.as<int32_t>(),
                         X.side[0].rating.as<float>(), c->p.t[0], c->p.t[1], c->p.t[2], c->p.t[3], c->p.t[4],
                         c->resid.as<double>(), mark, n_ent[0]);
      FIA_HIP_TRY(hipGetLastError());
    }
  } else {
    for (int sd = 0; sd < 2; ++sd) {
      hipLaunchKernelGGL(k_l1_big<K>, dim3(grid_cap((n_ent[sd] * K + 255) / 256, 16384)), dim3(256), 0, s,
                         c->p.t[sd], c->p.t[4], sd * K, n_ent[sd], c->l1[sd].as<double>());
      FIA_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ncf_wfrag<K>, dim3(3 * K * K / 256), dim3(256), 0, s, c->p.t[4], c->p.t[6],
                       c->wfrag.as<double>());
    FIA_HIP_TRY(hipGetLastError());
    for (int pass = marked ? 0 : -1; N > 0 && pass < (marked ? 2 : 0); ++pass) {
      const int sd = pass < 0 ? 0 : pass;
      hipLaunchKernelGGL(k_ncf_rows<K>, dim3(grid_cap((N + 15) / 16, 65536)), dim3(64 * kRowWaves), 0, s, N, pass,
                         c->self[sd].as<int32_t>(), X.side[sd].other.as<int32_t>(), X.side[sd].row.as<int32_t>(),
                         X.side[sd].rating.as<float>(), c->l1[0].as<double>(), c->l1[1].as<double>(), c->p.t[5],
                         c->p.t[6], c->p.t[7], c->p.t[8], c->p.t[9], c->p.t[2], c->p.t[3],
                         c->wfrag.as<const double2>(), c->gm[0].as<double>(), c->gm[1].as<double>(), c->resid.as<double>(),
                         mark, n_ent[0]);
      FIA_HIP_TRY(hipGetLastError());
    }
  }
  return hipSuccess;
}

template <class M>
hipError_t big_gram(fia_ctx* c, int sd, hipStream_t s) {
  constexpr int64_t GW = gram_words<M>();
  const Index& X = c->idx;
  const float* emb_other = M::ncf ? c->p.t[sd == 0 ? 3 : 2] : c->p.t[sd == 0 ? 1 : 0];
  if (c->n_bitems[sd] > 0) {
    constexpr int64_t NG = GramCfg<M>::NG, unit = 8 * NG;
    const int64_t n_vb = (c->n_bitems[sd] + 7) / 8 * unit;
    const dim3 g_gram = NG > 2 ? dim3((unsigned)(n_vb < (1 << 20) / unit * unit ? n_vb : (1 << 20) / unit * unit))
                               : dim3(grid_cap(c->n_bitems[sd], 1 << 20), (unsigned)NG);
    hipLaunchKernelGGL(k_big_gram<M>, g_gram, dim3(64 * kGW), 0, s,
                       sd, c->n_bitems[sd], c->bitems[sd].as<int32_t>(), X.side[sd].ptr.as<int64_t>(),
                       X.side[sd].other.as<int32_t>(), X.side[sd].row.as<int32_t>(), emb_other,
                       c->gm[sd].as<double>(), c->p.t[8], c->gram[sd].as<double>(), c->gpart[sd].as<double>());
    FIA_HIP_TRY(hipGetLastError());
  }
  if (c->n_bcomb[sd] > 0) {
    hipLaunchKernelGGL(k_big_combine, dim3(grid_cap(c->n_bcomb[sd], 1024), kCombSplit), dim3(256), 0, s, c->n_bcomb[sd],
                       c->bcomb[sd].as<int32_t>(), GW, c->gpart[sd].as<double>(), c->gram[sd].as<double>());
    FIA_HIP_TRY(hipGetLastError());
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_self(int64_t N, int64_t n_ent, const int64_t* ptr, int32_t* self, hipStream_t s) {
  hipLaunchKernelGGL(k_self, dim3(grid_cap((N + 255) / 256, 65536)), dim3(256), 0, s, N, n_ent, ptr, self);
  return hipGetLastError();
}

hipError_t launch_check_cover(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, int32_t* flag,
                              hipStream_t s) {
  hipLaunchKernelGGL(k_check_cover, dim3(grid_cap((Q + 255) / 256, 4096)), dim3(256), 0, s, Q, qu, qi, c->p.U,
                     c->p.I, c->slot[0].as<int32_t>(), c->slot[1].as<int32_t>(), flag);
  return hipGetLastError();
}

hipError_t launch_big_rows(int model, int k, fia_ctx* c, bool marked, hipStream_t s) {
  return big_dispatch(model, k, [&](auto m) { return big_rows<decltype(m)>(c, marked, s); });
}

hipError_t launch_big_gram(int model, int k, fia_ctx* c, int sd, hipStream_t s) {
  return big_dispatch(model, k, [&](auto m) { return big_gram<decltype(m)>(c, sd, s); });
}

}  // namespace fia
