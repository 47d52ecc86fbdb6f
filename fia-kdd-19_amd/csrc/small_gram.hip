// Small-k prepare kernels: the per-entity Gram caches A_u, B_i (math: models.hip) by slices of
// the entities' lists -- k_gram_mf_mfma (MF k in {32, 64}; k <= 16 when the Gram stream of
// gram_mf.hip cannot number the entities), k_ncf_gram_rows (NCF, with the per-position rows
// scoring reads), k_gram_combine for split lists -- and the dense NCF layer-1 rows k_ncf_l1.
// gfx950 only.
#include <cmath>

#include "kern.h"

namespace fia {
namespace {

// ------------------------------------------------------------------------------------
// NCF layer-1 halves: L1[0][u] = Pm_u W1[:k], L1[1][i] = Qm_i W1[k:]  (fp64)
// ------------------------------------------------------------------------------------
template <int K>
__global__ void k_ncf_l1(const float* __restrict__ emb, const float* __restrict__ W1, int row_off, int64_t n_ent,
                         double* __restrict__ out) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_ent * K) return;
  int64_t e = t / K;
  int c = (int)(t % K);
  const float* x = emb + e * K;
  double acc = 0.0;
#pragma unroll
  for (int a = 0; a < K; ++a) acc = fma((double)x[a], (double)W1[(row_off + a) * K + c], acc);
  out[t] = acc;
}

// ------------------------------------------------------------------------------------
// MF Gram on the f64 matrix cores: one wave per entity, 4 list rows per
// v_mfma_f64_16x16x4_f64.  Lane l holds G[t0 + l/16][16 c + l%16] of the gathered
// other-side embeddings, which is both the A (= G^T) and the B operand of
// C += G^T G; the bias row (sums) and count come from VALU adds.
// C/D map (f64 16x16x4): col = l & 15, row = (l >> 4) + 4 r.
// ------------------------------------------------------------------------------------
// both sides' Gram work in one launch: blocks [0, n_items[0]) users, the rest items
struct GramSides {
  int64_t n_items[2];
  const int32_t* items[2];
  const int64_t* ptr[2];
  const int32_t* other[2];
  const float* emb_other[2];
  double* gram[2];
  double* part[2];
  // NCF (k_ncf_gram_rows): stored g_mlp rows per side, W3, list length N
  const double* lgm[2];
  const float* W3;
  int64_t N;
  // fia_prepare_for (small k): only the entities marked here (users [0, U), items [U, U+I))
  // get their Gram caches / per-position rows; nullptr = every entity
  const uint8_t* mark;
  int64_t moff[2];
  __device__ bool skip(int sd, int32_t e) const { return mark && !mark[moff[sd] + e]; }
  // MF k in {32, 64} (k_gram_mf_mfma): the residual e_p = r-hat_p - y_p of every list
  // position of a cached entity into lres[sd * N + p] for k_score_mf_mfma (nullptr: none)
  const float* emb_self[2];
  const float* rating[2];
  const float* bias[2];       // user, item bias tables
  const float* gb;
  double* lres;
};


template <class M>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void k_gram_mf_mfma(GramSides GSd) {
  constexpr int K = M::K, Ds = M::Ds, GS = Ds * (Ds + 1) / 2, GSP = (GS + 1) & ~1;
  constexpr int NT = (K + 15) / 16;               // 16-wide column tiles
  constexpr int NP = NT * (NT + 1) / 2;           // upper tile pairs
  // MFMA row-quads gathered ahead per batch (k = 64: 6, so the double-buffered rows, the
  // residual pass and the 10 accumulator tiles fit two waves per SIMD)
  constexpr int SUB = NT <= 2 ? 16 : NT == 3 ? 8 : 6;
  const int sd = (int64_t)blockIdx.x >= GSd.n_items[0] ? 1 : 0;
  const int64_t w = (int64_t)blockIdx.x - (sd ? GSd.n_items[0] : 0);
  if (w >= GSd.n_items[sd]) return;
  const int32_t* __restrict__ items = GSd.items[sd];
  const int64_t* __restrict__ ptr = GSd.ptr[sd];
  const int32_t* __restrict__ other = GSd.other[sd];
  const float* __restrict__ emb_other = GSd.emb_other[sd];
  double* __restrict__ gram = GSd.gram[sd];
  double* __restrict__ part = GSd.part[sd];
  const int32_t e = items[4 * w], start = items[4 * w + 1], len = items[4 * w + 2], slot = items[4 * w + 3];
  if (GSd.skip(sd, e)) return;
  const int lane = threadIdx.x;
  const int col = lane & 15, grp = lane >> 4;
  const int32_t* ids = other + ptr[e] + start;
  d4_t acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = d4_t{0.0, 0.0, 0.0, 0.0};
  double sum[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) sum[t] = 0.0;
  // one coalesced load of 4*SUB row ids per batch, every row-quad's gather in flight at
  // once.  k >= 32: software-pipelined (ids two batches ahead, gathers one batch ahead;
  // 20M MF k=64 prepare 8.0 -> 6.7 ms); k <= 16 lists are mostly one or two batches and
  // the look-ahead costs more than it hides (ml-1m-ex 57 -> 65 us)
  auto ids_at = [&](int t0) -> int32_t { return (lane < 4 * SUB && t0 + lane < len) ? ids[t0 + lane] : -1; };
  auto gather = [&](int32_t id, double (&val)[SUB][NT]) {
#pragma unroll
    for (int sb = 0; sb < SUB; ++sb) {
      const int32_t o = __shfl(id, 4 * sb + grp);
      const float* src = emb_other + (int64_t)(o < 0 ? 0 : o) * K;
#pragma unroll
      for (int t = 0; t < NT; ++t) val[sb][t] = (o >= 0 && 16 * t + col < K) ? (double)src[16 * t + col] : 0.0;
    }
  };
  auto accumulate = [&](const double (&val)[SUB][NT]) {
#pragma unroll
    for (int sb = 0; sb < SUB; ++sb) {
      int p = 0;
#pragma unroll
      for (int ta = 0; ta < NT; ++ta) {
        sum[ta] += val[sb][ta];
#pragma unroll
        for (int tb = ta; tb < NT; ++tb, ++p)
          acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(val[sb][ta], val[sb][tb], acc[p], 0, 0, 0);
      }
    }
  };
  if constexpr (K >= 32) {
    // the residual of each gathered row (mf:89-116): the entity's own row dotted with it --
    // lane (grp, col) holds coordinates 16 t + col of row 4 sb + grp, so a row's dot is a
    // 16-lane DPP sum; lane l < 4 SUB then owns batch row l (its list entry, rating and the
    // other side's bias, loaded with the row's gather one batch ahead).  The products and the
    // sum order are the same from either side's list, so both copies have the same bits.
    const bool want_res = GSd.lres != nullptr;
    const float* __restrict__ es = GSd.emb_self[sd] + (int64_t)e * K;
    double eself[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) eself[t] = 16 * t + col < K ? (double)es[16 * t + col] : 0.0;
    const double bself = want_res ? (double)GSd.bias[sd][e] : 0.0, gbias = want_res ? (double)GSd.gb[0] : 0.0;
    const float* __restrict__ bother = GSd.bias[1 - sd];
    const int64_t lp0 = ptr[e] + start;
    const float* __restrict__ ratp = GSd.rating[sd] + lp0;
    auto row_loads = [&](int32_t id, int t0, float& y, float& bo) {
      const bool ok = want_res && lane < 4 * SUB && t0 + lane < len;
      y = ok ? ratp[t0 + lane] : 0.0f;
      bo = ok && id >= 0 ? bother[id] : 0.0f;
    };
    auto residuals = [&](const double (&val)[SUB][NT], float y, float bo, int t0) {
      double r = 0.0;
#pragma unroll
      for (int sb = 0; sb < SUB; ++sb) {
        double part = 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) part = fma(eself[t], val[sb][t], part);
        const double v = __shfl(row_sum16(part), 16 * (lane & 3));
        r = (lane >> 2) == sb ? v : r;
      }
      if (lane < 4 * SUB && t0 + lane < len) {
        const double bu = sd == 0 ? bself : (double)bo, bi = sd == 0 ? (double)bo : bself;
        GSd.lres[sd * GSd.N + lp0 + t0 + lane] = ((r + bu) + bi) + gbias - (double)y;
      }
    };
    double val[SUB][NT];
    int32_t id_c = ids_at(0);
    gather(id_c, val);
    float y_c, bo_c;
    row_loads(id_c, 0, y_c, bo_c);
    int32_t id_n = ids_at(4 * SUB);
    for (int t0 = 0; t0 < len; t0 += 4 * SUB) {
      const int32_t id_nn = ids_at(t0 + 8 * SUB);
      double vn[SUB][NT];
      gather(id_n, vn);                          // next batch (ids -1 past the end)
      float y_n, bo_n;
      row_loads(id_n, t0 + 4 * SUB, y_n, bo_n);
      if (want_res) residuals(val, y_c, bo_c, t0);
      accumulate(val);
#pragma unroll
      for (int sb = 0; sb < SUB; ++sb)
#pragma unroll
        for (int t = 0; t < NT; ++t) val[sb][t] = vn[sb][t];
      y_c = y_n;
      bo_c = bo_n;
      id_n = id_nn;
    }
  } else {
    // k <= 16 (a work item is <= 256 rows = 4 batches): every batch's row ids loaded up front
    // (one latency instead of one per batch), the gathers batch by batch
    constexpr int NB = 4;
    int32_t idb[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) idb[b] = ids_at(4 * SUB * b);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (4 * SUB * b >= len) break;
      double val[SUB][NT];
      gather(idb[b], val);
      accumulate(val);
    }
    for (int t0 = 4 * SUB * NB; t0 < len; t0 += 4 * SUB) {      // (longer work items)
      double val[SUB][NT];
      gather(ids_at(t0), val);
      accumulate(val);
    }
  }
  double* out = slot < 0 ? gram + (int64_t)e * GSP : part + (int64_t)slot * GSP;
  int p = 0;
#pragma unroll
  for (int ta = 0; ta < NT; ++ta) {
#pragma unroll
    for (int tb = ta; tb < NT; ++tb, ++p) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int ci = 16 * ta + grp + 4 * rr;    // C row -> Gram column index (tile ta)
        const int rj = 16 * tb + col;             // C col -> Gram row index (tile tb)
        if (ci < K && rj < K && rj >= ci) out[tri(rj, ci)] = acc[p][rr];
      }
    }
  }
  // bias row: Gram[K][c] = sum over rows of G[.][c]; Gram[K][K] = row count
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    double s = sum[t];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (grp == 0 && 16 * t + col < K) out[tri(K, 16 * t + col)] = s;
  }
  if (lane == 0) out[tri(K, K)] = (double)len;
}

// ------------------------------------------------------------------------------------
// NCF per list position + entity Gram, one pass (ncf:102-145, TF ReluGrad masks).  A wave
// takes one work item (<= gchunk positions of one entity's list, both sides in one
// launch) in slabs of 16 positions p, e = the entity, o = other(p):
//   z1 = (L1_self[e] + b1) + L1_other[o],  z2 = relu(z1) W2 + b2,  d2 = 1[z2 > 0] W3m,
//   d1 = 1[z1 > 0] (W2 d2),  g_mlp = W1_side d1,  e_p = W3m.relu(z2) + W3g.(Gs_e*Go_o) + b3 - y,
//   Gram_e += g g^T over g = [g_mlp ; W3g * Go_o]
// and stores g_mlp to lgm[a * N + p] (coordinate-major) and e_p to lres[p] for scoring.
// All products run on v_mfma_f64_16x16x4_f64.  The MLP runs transposed -- out^T = W . in^T
// with the 16 positions along n -- so the weights are per-lane A operands loaded once
// per wave and each product's C registers are the next product's B operand as they stand
// (C register r = rows (l>>4) + 4r = the next k-slice r).  The last product runs the
// other way round, g_mlp = d1 . W1_side^T (the same per-lane W1 values as B operand), so
// its C register r holds positions 4r + (l>>4) x coordinates l&15 -- exactly the Gram
// MFMA's operand for row-quad r.  No LDS, no transposes.
// Map: lane l supplies A[l&15][l>>4] and B[l>>4][l&15]; C register r = out[(l>>4)+4r][l&15].
// ------------------------------------------------------------------------------------
template <class M>
__global__ __launch_bounds__(64) void k_ncf_gram_rows(GramSides GSd, const float* __restrict__ W1,
                                                      const float* __restrict__ b1, const float* __restrict__ W2,
                                                      const float* __restrict__ b2, const float* __restrict__ b3,
                                                      const double* __restrict__ l1u, const double* __restrict__ l1i,
                                                      const float* __restrict__ rat0, const float* __restrict__ rat1,
                                                      double* __restrict__ lres) {
  constexpr int K = M::K, H = K / 2, KK = K / 4, HK = (H + 3) / 4, KT = (K + 15) / 16;
  constexpr int Ds = M::Ds, GS = Ds * (Ds + 1) / 2, GSP = (GS + 1) & ~1;
  constexpr int NT = Ds / 16, NP = NT * (NT + 1) / 2;
  static_assert(M::ncf && K % 8 == 0 && H <= 16 && Ds % 16 == 0, "NCF k in {8, 16, 32}");
  const float* __restrict__ W3 = GSd.W3;
  const int64_t N = GSd.N;
  const int lane = threadIdx.x, m = lane & 15, kq = lane >> 4;
  const int64_t n_all = GSd.n_items[0] + GSd.n_items[1];
  // side-independent weight operands (per lane, once per wave)
  double aW2t[KK], aW2[KT][HK], cb2[4], cw3[4], w3gk[KK], b1v[KK], w3gt[NT];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    const int c = kq + 4 * kk;
    aW2t[kk] = m < H ? (double)W2[c * H + m] : 0.0;           // A[h][c] = W2[c][h]
    w3gk[kk] = (double)W3[H + c];
    b1v[kk] = (double)b1[c];
  }
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    const int row = m + 16 * t;
#pragma unroll
    for (int kk = 0; kk < HK; ++kk) {
      const int h = kq + 4 * kk;
      aW2[t][kk] = row < K && h < H ? (double)W2[row * H + h] : 0.0;          // A[c][h] = W2[c][h]
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int h = kq + 4 * r;
    cb2[r] = h < H ? (double)b2[h] : 0.0;
    cw3[r] = h < H ? (double)W3[h] : 0.0;
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int co = 16 * t + m;
    w3gt[t] = co >= K ? (double)W3[H + co - K] : 0.0;
  }
  const double bias3 = (double)b3[0];
  int cur_side = -1;
  double aW1[KT][KK];          // W1_side[a = m + 16t][c = kq + 4kk]: A of nothing, B of g_mlp = d1 W1^T
  for (int64_t w = blockIdx.x; w < n_all; w += gridDim.x) {
    const int sd = w >= GSd.n_items[0] ? 1 : 0;
    const int64_t wi = w - (sd ? GSd.n_items[0] : 0);
    if (sd != cur_side) {
      cur_side = sd;
#pragma unroll
      for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
          const int a = m + 16 * t;
          aW1[t][kk] = a < K ? (double)W1[(int64_t)(sd * K + a) * K + kq + 4 * kk] : 0.0;
        }
    }
    const int32_t* __restrict__ it = GSd.items[sd] + 4 * wi;
    const int32_t e = it[0], start = it[1], len = it[2], slot = it[3];
    if (GSd.skip(sd, e)) continue;
    const int64_t lb = GSd.ptr[sd][e] + start;
    const int32_t* __restrict__ ids = GSd.other[sd] + lb;
    const float* __restrict__ rat = (sd ? rat1 : rat0) + lb;
    const float* __restrict__ Go = GSd.emb_other[sd];
    const float* __restrict__ Gs = GSd.emb_other[1 - sd] + (int64_t)e * K;     // own gmf row
    const double* __restrict__ Ls = (sd ? l1i : l1u) + (int64_t)e * K;
    const double* __restrict__ L1o = sd ? l1u : l1i;
    double* __restrict__ lgp = const_cast<double*>(GSd.lgm[sd]) + lb;
    int32_t* __restrict__ lmk = reinterpret_cast<int32_t*>(const_cast<double*>(GSd.lgm[sd])) + lb;   // mask path
    double* __restrict__ lrp = lres + (int64_t)sd * N + lb;
    double zs[KK], gsk[KK];     // own-entity terms for this lane's coordinates
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      zs[kk] = Ls[kq + 4 * kk] + b1v[kk];
      gsk[kk] = w3gk[kk] * (double)Gs[kq + 4 * kk];
    }
    d4_t acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = d4_t{0.0, 0.0, 0.0, 0.0};
    // Software pipeline over the slabs: the list ids run two slabs ahead and the gathers
    // one slab ahead (they only depend on the ids), so a slab waits on no memory round trip.
    // Per slab and lane: lo = L1_other[o_m][kq + 4kk], gf = Go[o_m][kq + 4kk] (residual),
    // gg[r][t] = Go[o_(4r+kq)][16t + m - k] (Gram operand of the gmf coordinates).
    const int lastp = len - 1;
    int32_t o = ids[m < lastp ? m : lastp];
    int32_t o_n = ids[16 + m < lastp ? 16 + m : lastp];
    double lo[KK];
    float gf[KK], gg[4][NT];
    auto gather = [&](int32_t oo, double (&lo_)[KK], float (&gf_)[KK], float (&gg_)[4][NT]) {
      const double* __restrict__ Lo = L1o + (int64_t)oo * K;
      const float* __restrict__ Gom = Go + (int64_t)oo * K;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        lo_[kk] = Lo[kq + 4 * kk];
        gf_[kk] = Gom[kq + 4 * kk];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int32_t orow = __shfl(oo, 4 * r + kq);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int co = 16 * t + m;
          gg_[r][t] = 0.f;
          if (16 * t + 15 >= K && co >= K) gg_[r][t] = Go[(int64_t)orow * K + co - K];
        }
      }
    };
    gather(o, lo, gf, gg);
    for (int s0 = 0; s0 < len; s0 += 16) {
      const bool ok = s0 + m < len;
      const int32_t o_nn = ids[s0 + 32 + m < lastp ? s0 + 32 + m : lastp];
      double lo_n[KK];
      float gf_n[KK], gg_n[4][NT];
      gather(o_n, lo_n, gf_n, gg_n);       // next slab (a harmless repeat past the end)
      double z1[KK];
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) z1[kk] = ok ? zs[kk] + lo[kk] : 0.0;
      d4_t z2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
        z2 = __builtin_amdgcn_mfma_f64_16x16x4f64(aW2t[kk], z1[kk] > 0.0 ? z1[kk] : 0.0, z2, 0, 0, 0);
      double mlp = 0.0, d2[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double z = z2[r] + cb2[r];
        const bool on = z > 0.0;
        mlp = fma(cw3[r], on ? z : 0.0, mlp);
        d2[r] = on ? cw3[r] : 0.0;
      }
      double d1[KK];
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        d4_t t1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < HK; ++kk) t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(aW2[t][kk], d2[kk], t1, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * t + r < KK) d1[4 * t + r] = z1[4 * t + r] > 0.0 ? t1[r] : 0.0;
      }
      // g_mlp = d1 W1_side^T: C register r = positions 4r + kq, coordinates m + 16t
      d4_t gm[KT];
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        gm[t] = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) gm[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(d1[kk], aW1[t][kk], gm[t], 0, 0, 0);
      }
      if constexpr (mask_path<M>()) {
        // ReLU masks of position m: lane (m, kq) holds z1 at c = kq + 4kk and z2 at h = kq + 4r
        int mk = 0;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) mk |= z1[kk] > 0.0 ? 1 << (kq + 4 * kk) : 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (kq + 4 * r < H) mk |= z2[r] + cb2[r] > 0.0 ? 1 << (K + kq + 4 * r) : 0;   // d2's `on`
        mk |= __shfl_xor(mk, 16);
        mk |= __shfl_xor(mk, 32);
        if (kq == 0 && ok) lmk[s0 + m] = mk;
      }
      // residual of position m (mlp and the gmf dot are split over the 4 lane groups)
      double gmf = 0.0;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) gmf = fma(gsk[kk], (double)gf[kk], gmf);
      double re = mlp + gmf;
      re += __shfl_xor(re, 16);
      re += __shfl_xor(re, 32);
      if (kq == 0 && ok) lrp[s0 + m] = re + bias3 - (double)rat[s0 + m];
      // Gram row-quads r: positions 4r + kq
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pr = s0 + 4 * r + kq;
        const bool okr = pr < len;
        double val[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int co = 16 * t + m;
          const double gv = gm[t < KT ? t : KT - 1][r];
          double x;
          if (co < K) {
            x = gv;
            if constexpr (!mask_path<M>())
              if (okr) lgp[(int64_t)co * N + pr] = gv;
          } else {
            x = w3gt[t] * (double)gg[r][t];
          }
          val[t] = okr ? x : 0.0;
        }
        int p = 0;
#pragma unroll
        for (int ta = 0; ta < NT; ++ta)
#pragma unroll
          for (int tb = ta; tb < NT; ++tb, ++p)
            acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(val[ta], val[tb], acc[p], 0, 0, 0);
      }
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        lo[kk] = lo_n[kk];
        gf[kk] = gf_n[kk];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int t = 0; t < NT; ++t) gg[r][t] = gg_n[r][t];
      o_n = o_nn;
    }
    double* out = slot < 0 ? GSd.gram[sd] + (int64_t)e * GSP : GSd.part[sd] + (int64_t)slot * GSP;
    int p = 0;
#pragma unroll
    for (int ta = 0; ta < NT; ++ta)
#pragma unroll
      for (int tb = ta; tb < NT; ++tb, ++p)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int ci = 16 * ta + kq + 4 * rr;    // C row -> Gram column index (tile ta)
          const int rj = 16 * tb + m;              // C col -> Gram row index (tile tb)
          if (rj >= ci) out[gidx<M>(rj, ci)] = acc[p][rr];
        }
  }
}

// Sum the partial Grams of split lists in slot order (deterministic); both sides in one
// launch (blocks [0, n_comb0) the user side).
__global__ __launch_bounds__(256) void k_gram_combine(int64_t n_comb0, const int32_t* __restrict__ comb0,
                                                     const double* __restrict__ part0, double* __restrict__ gram0,
                                                     int64_t n_comb1, const int32_t* __restrict__ comb1,
                                                     const double* __restrict__ part1, double* __restrict__ gram1,
                                                     int GS, int GSP, const uint8_t* __restrict__ mark, int64_t moff1) {
  const int sd = (int64_t)blockIdx.x >= n_comb0 ? 1 : 0;
  const int64_t w = (int64_t)blockIdx.x - (sd ? n_comb0 : 0);
  if (w >= (sd ? n_comb1 : n_comb0)) return;
  const int32_t* __restrict__ comb = sd ? comb1 : comb0;
  const double* __restrict__ part = sd ? part1 : part0;
  double* __restrict__ gram = sd ? gram1 : gram0;
  const int32_t e = comb[4 * w], first = comb[4 * w + 1], ns = comb[4 * w + 2];
  if (mark && !mark[(sd ? moff1 : 0) + e]) return;
  // partials summed in slot order (deterministic), their loads issued 8 slots at a time
  // rather than one dependent round trip per slot; the last group's missing slots load slot
  // `first` and are weighted 0 (branch-free: a partial group is not a chain of round trips)
  for (int t = threadIdx.x; t < GS; t += blockDim.x) {
    const double* __restrict__ pt = part + (int64_t)first * GSP + t;
    double s = 0.0;
    for (int k = 0; k < ns; k += 8) {
      double v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = pt[(int64_t)(k + j < ns ? k + j : 0) * GSP];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += k + j < ns ? v[j] : 0.0;
    }
    gram[(int64_t)e * GSP + t] = s;
  }
}

}  // namespace

hipError_t launch_ncf_l1(int k, const float* emb, const float* W1, int sd, int64_t n_ent, double* out, hipStream_t s) {
  bool ok = false;
  dispatch_small(FIA_MODEL_NCF, k, [&](auto m) {
    if constexpr (decltype(m)::ncf) {
      constexpr int K = decltype(m)::K;
      hipLaunchKernelGGL(k_ncf_l1<K>, dim3((unsigned)((n_ent * K + 255) / 256)), dim3(256), 0, s, emb, W1, sd * K,
                         n_ent, out);
      ok = true;
    }
  });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

// The per-slice Gram pass over the slice lists of build_gram_lists (c->idx.gitems), both sides in
// one launch, into the caches and partial slots (and the per-position buffers) prepare_impl
// reserved; mark: fia_prepare_for's entities, or null for all
hipError_t launch_gram_slices(int model, int k, fia_ctx* c, const uint8_t* mark, hipStream_t s) {
  const Index& X = c->idx;
  const int64_t n_ent[2] = {c->p.U, c->p.I};
  const bool ncf = model == FIA_MODEL_NCF;
  GramSides G{};
  for (int sd = 0; sd < 2; ++sd) {
    G.n_items[sd] = n_ent[sd] > 0 ? X.n_gitems[sd] : 0;
    G.items[sd] = X.gitems[sd].as<int32_t>();
    G.ptr[sd] = X.side[sd].ptr.as<int64_t>();
    G.other[sd] = X.side[sd].other.as<int32_t>();
    G.emb_other[sd] = ncf ? c->p.t[sd == 0 ? 3 : 2] : c->p.t[sd == 0 ? 1 : 0];   // NCF: gmf tables
    G.gram[sd] = c->gram[sd].as<double>();
    G.part[sd] = c->gpart[sd].as<double>();
    // NCF, per list position of each side: g_mlp coordinate-major [k][N], or (mask path) the
    // ReLU masks int32 [N]
    G.lgm[sd] = c->gm[sd].as<double>();
  }
  G.W3 = c->p.t[8];
  G.N = X.N;
  G.mark = mark;
  G.moff[0] = 0;
  G.moff[1] = n_ent[0];
  const int64_t n_all = G.n_items[0] + G.n_items[1];
  if (n_all <= 0) return hipSuccess;
  const bool ok = dispatch_small(model, k, [&](auto m) {
    using M = decltype(m);
    if constexpr (M::ncf) {
      // persistent: the per-lane weight operands are loaded once per wave.  8 waves per CU fill
      // every CU (2 per SIMD at its registers); when other contexts share the GPU (batches in
      // flight) 6, so their kernels run beside the pass instead of after it (yelp-ex, 2 in
      // flight, same box: 102.1 -> 106.0-106.4 M q/s; one context alone: 92.5 at 8, 85.9 at 6)
      const int per_cu = live_contexts(c->device) > 1 ? 6 : 8;
      const int64_t cap = (int64_t)(c->num_cus > 0 ? c->num_cus : 256) * per_cu;
      const int64_t grid = n_all < cap ? n_all : cap;
      hipLaunchKernelGGL(k_ncf_gram_rows<M>, dim3((unsigned)grid), dim3(64), 0, s, G, c->p.t[4], c->p.t[5],
                         c->p.t[6], c->p.t[7], c->p.t[9], c->l1[0].as<double>(), c->l1[1].as<double>(),
                         X.side[0].rating.as<float>(), X.side[1].rating.as<float>(), c->resid.as<double>());
    } else {
      if constexpr (M::K == 32 || M::K == 64) {
        // list-ordered residuals of both sides for k_score_mf_mfma ([0, N) users, [N, 2N) items),
        // written by the Gram pass for every list position of a cached entity
        for (int sd = 0; sd < 2; ++sd) {
          G.emb_self[sd] = c->p.t[sd];
          G.rating[sd] = X.side[sd].rating.as<float>();
          G.bias[sd] = c->p.t[2 + sd];
        }
        G.gb = c->p.t[4];
        G.lres = c->resid.as<double>();
      }
      hipLaunchKernelGGL(k_gram_mf_mfma<M>, dim3((unsigned)n_all), dim3(64), 0, s, G);
    }
  });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

// the partial Grams (c->gpart) of the split lists comb0 / comb1 {entity, first slot, slots, 0}
// summed into the caches
hipError_t launch_gram_combine(fia_ctx* c, int64_t nc0, const int32_t* comb0, int64_t nc1, const int32_t* comb1,
                               int GS, int GSP, const uint8_t* mark, hipStream_t s) {
  if (nc0 + nc1 <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_gram_combine, dim3((unsigned)(nc0 + nc1)), dim3(256), 0, s, nc0, comb0,
                     c->gpart[0].as<double>(), c->gram[0].as<double>(), nc1, comb1, c->gpart[1].as<double>(),
                     c->gram[1].as<double>(), GS, GSP, mark, c->p.U);
  return hipGetLastError();
}

}  // namespace fia
