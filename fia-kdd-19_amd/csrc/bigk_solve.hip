// Large-k FIA path, the per-query systems (the math and the structures: bigk.hip): the
// prologue that writes a query's work words and appends its systems to the solve lists
// (k_big_prologue), the blocked LDL^T solve of one system per workgroup (k_big_solve: the
// coupled queries; the side systems go through bigk_solve_batched.hip), the records from a
// given x instead of a solve (k_big_record_x), and the record headers (k_big_finish).
#include "bigk.h"

namespace fia {
namespace {

// ------------------------------------------------------------------------------------
// Per-query prologue (one 256-thread block per query): n, the pair terms, r-hat(u,i),
// theta_t and v = d r-hat(u,i) / d theta_t (gnn:155, mf:194,201 / ncf:222,229); append
// the query's systems to the solve lists.
// ------------------------------------------------------------------------------------
template <class M>
__global__ __launch_bounds__(256) void k_big_prologue(BigArgs A, int64_t Q, double* __restrict__ qwork,
                                                      int32_t* __restrict__ syslist, int32_t* __restrict__ cpllist) {
  constexpr int K = M::K, NPs = M::NPs;
  using W = typename M::Work;
  __shared__ double red[4];
  __shared__ double z1[M::ncf ? K : 1], d2[M::ncf ? M::H : 1], d1[M::ncf ? K : 1];
  const int tid = threadIdx.x;
  for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
    const int32_t u = A.qu[q], i = A.qi[q];
    double* qw = qwork + q * M::QW;
    bool ok = u >= 0 && u < A.U && i >= 0 && i < A.I;
    if (ok && A.slot[0]) ok = A.slot[0][u] >= 0 && A.slot[1][i] >= 0;   // not cached: NaN (checked by the ABI)
    const int64_t n = ok ? (A.ptr[0][u + 1] - A.ptr[0][u]) + (A.ptr[1][i + 1] - A.ptr[1][i]) : 0;
    if (n == 0) {
      if (tid == 0) qw[W::n] = 0.0;
      continue;
    }
    double* vu = W::v(qw, 0);
    double* vi = W::v(qw, 1);
    double* thu = W::theta(qw, 0);
    double* thi = W::theta(qw, 1);
    double rhat;
    if constexpr (!M::ncf) {
      const float* P = A.t[0] + (int64_t)u * K;
      const float* Qt = A.t[1] + (int64_t)i * K;
      double part = 0.0;
      for (int a = tid; a < NPs; a += 256) {
        const double pu = a < K ? (double)P[a] : 0.0, qi = a < K ? (double)Qt[a] : 0.0;
        part = fma(pu, qi, part);
        vu[a] = a < K ? qi : (a == K ? 1.0 : 0.0);
        vi[a] = a < K ? pu : (a == K ? 1.0 : 0.0);
        thu[a] = a < K ? pu : (a == K ? (double)A.t[2][u] : 0.0);
        thi[a] = a < K ? qi : (a == K ? (double)A.t[3][i] : 0.0);
      }
      rhat = bsum<4>(part, red) + (double)A.t[2][u] + (double)A.t[3][i] + (double)A.t[4][0];
    } else {
      constexpr int H = M::H;
      const float* W1 = A.t[4];
      const float* W2 = A.t[6];
      const float* W3 = A.t[8];
      __syncthreads();
      for (int c = tid; c < K; c += 256)
        z1[c] = A.l1[0][(int64_t)u * K + c] + A.l1[1][(int64_t)i * K + c] + (double)A.t[5][c];
      __syncthreads();
      double mlp = 0.0;
      for (int d = tid; d < H; d += 256) {
        double z2 = (double)A.t[7][d];
        for (int c = 0; c < K; ++c) z2 = fma((double)W2[c * H + d], z1[c] > 0.0 ? z1[c] : 0.0, z2);
        const bool on = z2 > 0.0;
        mlp += on ? (double)W3[d] * z2 : 0.0;
        d2[d] = on ? (double)W3[d] : 0.0;
      }
      __syncthreads();
      for (int c = tid; c < K; c += 256) {
        double t = 0.0;
        for (int d = 0; d < H; ++d) t = fma((double)W2[c * H + d], d2[d], t);
        d1[c] = z1[c] > 0.0 ? t : 0.0;
      }
      __syncthreads();
      double gmf = 0.0;
      for (int a = tid; a < K; a += 256) {
        double su = 0.0, si = 0.0;
        for (int c = 0; c < K; ++c) {
          su = fma((double)W1[(int64_t)a * K + c], d1[c], su);
          si = fma((double)W1[(int64_t)(K + a) * K + c], d1[c], si);
        }
        const double pm = A.t[0][(int64_t)u * K + a], qm = A.t[1][(int64_t)i * K + a];
        const double pg = A.t[2][(int64_t)u * K + a], qg = A.t[3][(int64_t)i * K + a];
        const double w3g = (double)W3[H + a];
        vu[a] = su;
        vi[a] = si;
        vu[K + a] = w3g * qg;        // d r / d Pg_u = W3g * Qg_i
        vi[K + a] = w3g * pg;        // d r / d Qg_i = W3g * Pg_u
        thu[a] = pm;
        thu[K + a] = pg;
        thi[a] = qm;
        thi[K + a] = qg;
        gmf = fma(w3g * pg, qg, gmf);
      }
      rhat = bsum<4>(mlp + gmf, red) + (double)A.t[9][0];
    }
    if (tid == 0) {
      double cdup, rsum;
      A.pairs.lookup((unsigned long long)u * (unsigned long long)A.I + (unsigned long long)i, cdup, rsum);
      qw[W::n] = (double)n;
      qw[W::cdup] = cdup;
      qw[W::esum] = cdup * rhat - rsum;
      qw[W::rhat] = rhat;
      qw[W::coupled] = cdup > 0.0 ? 1.0 : 0.0;
      if (cdup > 0.0) {
        const int s = atomicAdd(cpllist, 1);
        cpllist[1 + s] = (int32_t)q;
      } else {
        const int s = atomicAdd(syslist, 2);
        syslist[1 + s] = (int32_t)(2 * q);
        syslist[2 + s] = (int32_t)(2 * q + 1);
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// Per-query solve, one 512-thread workgroup per system (persistent over the list).
// System = one side block (CPL = false, NP = NPs) or a full coupled query (CPL = true,
// NP = 2 NPs); the matrix source is `aorig` (the Hessian from the Gram caches, row NP the
// right-hand side v^T), the epilogue writes the padded solution and the scoring record.
// The blocked LDL^T between them is the algorithm of big_ldlt_solve (bigk.h, where it is
// described), kept in place here: calling the shared function instead compiled this kernel
// at MF k = 256 with 1070 spilled VGPRs instead of 575 and its solve of 1,024 coupled
// queries measured 18.2 ms instead of 12.1 ms (same MI355X, interleaved), whatever the
// function's signature (references, by value, LDS-typed pointers, thread indices passed in).
// ------------------------------------------------------------------------------------
template <class M, int NP, bool CPL>
__global__ __launch_bounds__(solve_threads<NP>()) void k_big_solve(BigArgs A, const int32_t* __restrict__ list,
                                                   const double* __restrict__ qwork, double* __restrict__ lscr,
                                                   double* __restrict__ xb, double* __restrict__ rec) {
  constexpr int K = M::K, NPs = M::NPs, Ds = M::Ds, NB = solve_nb<NP>(), LDR = NP + 16, LDP = NB + 1;
  constexpr int NRT = LDR / 16, NCT = NB / 16, MG = kSolveMG;
  constexpr int64_t GW = gram_words<M>();
  constexpr int kST = solve_threads<NP>(), kSW = kST / 64;
  constexpr int CPT = (NP + kST - 1) / kST;    // backward-solve columns per thread
  constexpr int BW = CPT == 1 && NB == 32 ? 32 : 16;   // backward-solve block (<= NB: staged in W11)
  static_assert(BW <= NB, "backward blocks are staged in W11");
  using L = typename M::Rec;
  using W = typename M::Work;
  __shared__ double P[LDR * LDP];
  __shared__ double dd[NP];
  __shared__ double W11[NB * NB];              // W11[j][jj] = L[c0+j][c0+jj] d[c0+jj], jj < j
  __shared__ double red[64];
  double* __restrict__ Ls = lscr + (int64_t)blockIdx.x * LDR * NP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ml = lane & 15, kl = lane >> 4;
  const int nsys = list[0];
  for (int w = blockIdx.x; w < nsys; w += gridDim.x) {
    const int code = list[1 + w];
    const int64_t q = CPL ? code : (code >> 1);
    const int sd = CPL ? 0 : (code & 1);
    const double* __restrict__ qw = qwork + q * M::QW;
    const double s2n = 2.0 / qw[W::n], cdup = qw[W::cdup], esum = qw[W::esum];
    const double* __restrict__ vv = W::v(qw, sd);   // v of this system (coupled: sd = 0, both sides)
    const int32_t u = A.qu[q], i = A.qi[q];
    const double* __restrict__ G0 = A.gram[0] + (int64_t)(A.slot[0] ? A.slot[0][u] : u) * GW;
    const double* __restrict__ G1 = A.gram[1] + (int64_t)(A.slot[1] ? A.slot[1][i] : i) * GW;
    auto aorig = [&](int r, int c) -> double {
      if (r >= NP) return (r == NP && c < NP) ? vv[c] : 0.0;
      if constexpr (!CPL) {
        if (r >= Ds || c >= Ds) return r == c ? 1.0 : 0.0;
        double h = s2n * gram_at<M>(sd ? G1 : G0, r, c);
        if (r == c) h += (M::decayed(r) ? A.wd : 0.0) + A.damping;
        return h;
      } else {
        const int sr = r >= NPs, sc = c >= NPs, rr = r - sr * NPs, cc = c - sc * NPs;
        if (rr >= Ds || cc >= Ds) return r == c ? 1.0 : 0.0;
        double h;
        if (sr == sc) {
          h = s2n * (gram_at<M>(sr ? G1 : G0, rr, cc) + cdup * vv[r] * vv[c]);
          if (r == c) h += (M::decayed(rr) ? A.wd : 0.0) + A.damping;
        } else {
          // item row / user column: 2 (cdup g_i g_u^T + esum d2r / dtheta_i dtheta_u)
          const int iu = sr ? cc : rr, ii = sr ? rr : cc;
          h = s2n * 2.0 * cdup * vv[NPs + ii] * vv[iu];
          if (ii == iu) {
            if constexpr (!M::ncf) {
              if (iu < K) h += s2n * 2.0 * esum;                                     // d2 r / dp_u dq_i = I
            } else {
              if (iu >= K) h += s2n * 2.0 * esum * (double)A.t[8][M::H + (iu - K)];    // diag(W3g)
            }
          }
        }
        return h;
      }
    };
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
    // epilogue: padded solution, per-side partial sums and the scoring record
    double* __restrict__ R = rec + q * M::R;
    for (int s = 0; s < (CPL ? 2 : 1); ++s) {
      const int side = CPL ? s : sd;
      const double* __restrict__ xsd = xs + (CPL ? s * NPs : 0);
      const double* __restrict__ vsd = W::v(qw, side);
      const double* __restrict__ th = W::theta(qw, side);
      double* __restrict__ xo = xb + q * 2 * NPs + side * NPs;
      double cq = 0.0, xv = 0.0;
      for (int a = tid; a < NPs; a += kST) {
        const double xa = xsd[a];
        xo[a] = xa;
        if (a < Ds) {
          if (M::decayed(a)) cq = fma(xa, th[a], cq);
          xv = fma(xa, vsd[a], xv);
        }
      }
      cq = bsum<kSW>(cq, red);
      xv = bsum<kSW>(xv, red);
      double* __restrict__ S = L::side(R, side);
      if (tid == 0) {
        R[L::cq_of(side)] = A.wd * cq;
        R[L::xv_of(side)] = xv;
      }
      if constexpr (!M::ncf) {
        for (int a = tid; a <= K; a += kST) S[L::x + a] = xsd[a];
      } else {
        for (int c = tid; c < K; c += kST) {
          S[L::x_mlp + c] = xsd[c];
          S[L::w3g_x_gmf + c] = (double)A.t[8][M::H + c] * xsd[K + c];
        }
      }
      if (tid == 0) S[L::dup_other] = (double)(side ? u : i);
    }
    __syncthreads();   // xs / dd / P are rewritten by the next system
  }
}

// fia_query_batch_x (a given inverse HVP, mf:210-214): the padded solution and this side's
// record words from x_in (reference theta order) instead of the k_bs_* solve -- the same
// words k_bs_back / k_big_solve write, from the prologue's theta and v.  One wave per (query, side).
template <class M>
__global__ __launch_bounds__(64) void k_big_record_x(BigArgs A, int64_t Q, const double* __restrict__ x_in,
                                                     const double* __restrict__ qwork, double* __restrict__ xb,
                                                     double* __restrict__ rec) {
  constexpr int K = M::K, NPs = M::NPs, Ds = M::Ds, D = 2 * Ds;
  using L = typename M::Rec;
  using W = typename M::Work;
  const int tid = threadIdx.x;
  for (int64_t w = blockIdx.x; w < 2 * Q; w += gridDim.x) {
    const int64_t q = w >> 1;
    const int sd = (int)(w & 1);
    const double* __restrict__ qw = qwork + q * M::QW;
    const double* __restrict__ vsd = W::v(qw, sd);
    const double* __restrict__ th = W::theta(qw, sd);
    const double* __restrict__ xq = x_in + q * D;
    double* __restrict__ xo = xb + q * 2 * NPs + sd * NPs;
    double* __restrict__ R = rec + q * M::R;
    double* __restrict__ S = L::side(R, sd);
    double cq = 0.0, xv = 0.0;
    for (int a = tid; a < NPs; a += 64) {
      const double xa = a < Ds ? xq[M::ref_index(sd, a)] : 0.0;
      xo[a] = xa;
      if (a < Ds) {
        if (M::decayed(a)) cq = fma(xa, th[a], cq);
        xv = fma(xa, vsd[a], xv);
      }
      if constexpr (!M::ncf) {
        if (a <= K) S[L::x + a] = xa;
      } else {
        if (a < K) S[L::x_mlp + a] = xa;
        else if (a < Ds) S[L::w3g_x_gmf + (a - K)] = (double)A.t[8][M::H + (a - K)] * xa;
      }
    }
    cq = wave_sum(cq);
    xv = wave_sum(xv);
    if (tid == 0) {
      R[L::cq_of(sd)] = A.wd * cq;
      R[L::xv_of(sd)] = xv;
      const int32_t u = A.qu[q], i = A.qi[q];
      S[L::dup_other] = (double)(sd ? u : i);
    }
  }
}

// per-query record header and x in the reference theta order
template <class M>
__global__ __launch_bounds__(64) void k_big_finish(int64_t Q, const double* __restrict__ qwork,
                                                   const double* __restrict__ xb, double* __restrict__ rec,
                                                   double* __restrict__ x_out) {
  constexpr int Ds = M::Ds, NPs = M::NPs, D = 2 * Ds;
  using L = typename M::Rec;
  using W = typename M::Work;
  for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
    const double n = qwork[q * M::QW + W::n];
    double* R = rec + q * M::R;
    if (threadIdx.x == 0) {
      R[L::inv_n] = n > 0.0 ? 1.0 / n : NAN;
      if (n > 0.0) {
        R[L::c_q] = R[L::cq_u] + R[L::cq_i];
        R[L::x_v] = R[L::xv_u] + R[L::xv_i];
        R[L::rhat] = qwork[q * M::QW + W::rhat];
      }
    }
    if (x_out)
      for (int a = threadIdx.x; a < D; a += 64) {
        const int side = a >= Ds, aa = a - side * Ds;
        x_out[q * D + M::ref_index(side, aa)] = n > 0.0 ? xb[q * 2 * NPs + side * NPs + aa] : NAN;
      }
  }
}

}  // namespace

hipError_t launch_big_prologue(int model, int k, fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi,
                               hipStream_t s) {
  const BigArgs A = make_big_args(c, qu, qi);
  return big_dispatch(model, k, [&](auto m) {
    hipLaunchKernelGGL(k_big_prologue<decltype(m)>, dim3(grid_cap(Q, 1 << 20)), dim3(256), 0, s, A, Q,
                       c->qwork.as<double>(), c->syslist.as<int32_t>(), c->cpllist.as<int32_t>());
    return hipGetLastError();
  });
}

// one workgroup per coupled query of c->cpllist, persistent over the list: the grid is what is
// resident; the list's first word (the device-side count) bounds the work, Q only sizes it
hipError_t launch_solve(int model, int k, fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, hipStream_t s) {
  if (Q <= 0) return hipSuccess;
  const BigArgs A = make_big_args(c, qu, qi);
  return big_dispatch(model, k, [&](auto m) {
    using M = decltype(m);
    constexpr int NP = 2 * M::NPs;
    constexpr size_t lds = solve_lds<NP>();
    const int per_cu = (int)((160 * 1024) / lds);
    const int64_t resident = (int64_t)cu_count(c) * (per_cu > 0 ? per_cu : 1);
    const int64_t grid = Q < resident ? Q : resident;
    constexpr int64_t slab = (int64_t)(NP + 16) * NP;
    FIA_HIP_TRY(c->lscr.reserve(sizeof(double) * (size_t)(grid * slab), s));
    hipLaunchKernelGGL((k_big_solve<M, NP, true>), dim3((unsigned)grid), dim3(solve_threads<NP>()), 0, s, A,
                       c->cpllist.as<int32_t>(), c->qwork.as<double>(), c->lscr.as<double>(), c->xb.as<double>(),
                       c->rec.as<double>());
    return hipGetLastError();
  });
}

hipError_t launch_big_record_x(int model, int k, fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi,
                               const double* x_in, hipStream_t s) {
  if (Q <= 0) return hipSuccess;
  const BigArgs A = make_big_args(c, qu, qi);
  return big_dispatch(model, k, [&](auto m) {
    hipLaunchKernelGGL(k_big_record_x<decltype(m)>, dim3(grid_cap(2 * Q, 1 << 20)), dim3(64), 0, s, A, Q, x_in,
                       (const double*)c->qwork.as<double>(), c->xb.as<double>(), c->rec.as<double>());
    return hipGetLastError();
  });
}

hipError_t launch_big_finish(int model, int k, fia_ctx* c, int64_t Q, double* x_out, hipStream_t s) {
  return big_dispatch(model, k, [&](auto m) {
    hipLaunchKernelGGL(k_big_finish<decltype(m)>, dim3(grid_cap(Q, 1 << 20)), dim3(64), 0, s, Q,
                       c->qwork.as<double>(), c->xb.as<double>(), c->rec.as<double>(), x_out);
    return hipGetLastError();
  });
}

}  // namespace fia
