// Small-k solve kernels: x = H_t^-1 v per query by an exact fp64 LDL^T (math: models.hip).  One
// side-system solve per model (the predicates of kern.h) -- k_solve_quad (MF k = 16, with the
// chunk scan and the coupled solves as roles), k_solve_tps (MF k = 8), k_solve_tile (MF k in
// {32, 64}, NCF k = 32), k_solve_rows after k_ncf_query_pro (NCF k = 16), k_solve_col (NCF
// k = 8) -- the full-D k_solve for the queries whose test pair is a train row, and k_record_x
// for a given x.  gfx950 only.
#include <cmath>
#include <type_traits>

#include "kern.h"
#include "scan.h"    // query_scan_body: the scan role of k_solve_quad
#include "solve.h"   // ldlt_solve, solve_prologue, assemble_hessian

namespace fia {
namespace {

// 1 / d: v_rcp_f64 and two Newton steps, instead of an IEEE division sequence on a solve's
// critical path
__device__ __forceinline__ double rcp_nr2(double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = fma(r, fma(-d, r, 1.0), r);
  r = fma(r, fma(-d, r, 1.0), r);
  return r;
}

// query q joins the coupled list {count, q_0, q_1, ...}: its test pair is a train row, the
// full-D k_solve finishes it
__device__ __forceinline__ void coupled_append(int32_t* __restrict__ list, int64_t q) {
  const int slot = atomicAdd(list, 1);
  list[1 + slot] = (int32_t)q;
}

// Record + x_out of one solved query (first wave only, 64 lanes): v = the solution in
// block order [user block (Ds) | item block (Ds)]
template <class M>
__device__ void solve_epilogue(const QueryArgs& A, int64_t q, int32_t u, int32_t i, int64_t n, double rhat_ui,
                               const double* __restrict__ th, const double* __restrict__ g,
                               const double* __restrict__ v, const NCFWeights<M::ncf ? M::K : 2>& w,
                               double* __restrict__ R, double* __restrict__ x_out) {
  constexpr int K = M::K, Ds = M::Ds, D = M::D;
  using L = typename M::Rec;
  const int lane = threadIdx.x & 63;
  if (x_out)
    for (int a = lane; a < D; a += kSolveThreads) x_out[q * D + M::ref_index(a)] = v[a];
  double cq = 0.0, xg_user = 0.0, xg_item = 0.0;
  for (int a = lane; a < D; a += kSolveThreads) {
    const int j = a < Ds ? a : a - Ds;
    if (M::decayed(j)) cq += v[a] * th[a];
    if (a < Ds) xg_user += v[a] * g[a]; else xg_item += v[a] * g[a];
  }
  cq = wave_sum(cq) * A.wd;
  xg_user = wave_sum(xg_user);
  xg_item = wave_sum(xg_item);
  // The (u,i) train row itself has g = v, so x.g = x.v and e = r-hat(u,i) - y: both of
  // its copies in rel (user side and item side) get bit-identical influence, as the
  // reference's per-row sess.run gives them (mf:240-246).
  if (lane == 0) {
    R[L::inv_n] = 1.0 / (double)n;
    R[L::c_q] = cq;
    R[L::x_v] = xg_user + xg_item;
    R[L::rhat] = rhat_ui;
  }
  double* S0 = L::side(R, 0);
  double* S1 = L::side(R, 1);
  if constexpr (!M::ncf) {
    const double gb = (double)A.t[4][0];
    for (int a = lane; a < K; a += kSolveThreads) {
      S0[L::theta + a] = th[a];         // p_u
      S0[L::x + a] = v[a];              // x_pu
      S1[L::theta + a] = th[Ds + a];    // q_i
      S1[L::x + a] = v[Ds + a];         // x_qi
    }
    if (lane == 0) {
      S0[L::bias] = th[K] + gb;         S1[L::bias] = th[Ds + K] + gb;
      S0[L::x_bias] = v[K];             S1[L::x_bias] = v[Ds + K];
      S0[L::dup_other] = (double)i;     S1[L::dup_other] = (double)u;
    }
  } else {
    // x . g_j = x_mlp . g_mlp,j + (W3g * x_gmf) . gmf_other(j)  (k_score_ncf)
    constexpr int H2 = K / 2;
    for (int c = lane; c < K; c += kSolveThreads) {
      S0[L::x_mlp + c] = v[c];
      S1[L::x_mlp + c] = v[Ds + c];
      const double w3g = w.W3[H2 + c];
      S0[L::w3g_x_gmf + c] = w3g * v[K + c];
      S1[L::w3g_x_gmf + c] = w3g * v[Ds + K + c];
    }
    if (lane == 0) {
      S0[L::dup_other] = (double)i;  S1[L::dup_other] = (double)u;
    }
  }
}

// The full D x D system of one query on ONE WAVE: prologue, packed Hessian, LDL^T, record.  The
// wave may be a 64-thread workgroup (k_solve) or one wave of a larger one (the coupled role of
// k_solve_quad): its LDS is the caller's slab of kFullSlab<M> doubles, its synchronisation is
// wave-level (solve.h, WV = true), and it reads nothing another wave writes.  w / sW1 / sb1:
// the NCF weights the caller staged (dummies for MF).
template <class M>
constexpr int kFullSlab = M::D * (M::D + 1) / 2 + 5 * M::D + 4 * M::K + 8;
template <class M>
__device__ __forceinline__ void solve_full_wave(const QueryArgs& A, int64_t q, double* __restrict__ rec,
                                                double* __restrict__ x_out, double* __restrict__ slab,
                                                const NCFWeights<M::ncf ? M::K : 2>& w,
                                                const double* __restrict__ sW1, const double* __restrict__ sb1) {
  constexpr int Ds = M::Ds, D = M::D;
  double* const H = slab;
  double* const v = H + D * (D + 1) / 2;
  double* const g = v + D;
  double* const th = g + D;
  double* const dd = th + D;
  double* const ww = dd + D;
  double* const sh = ww + D;
  wave_lds_sync();               // the slab's previous query is read out
  const int lane = threadIdx.x & 63;
  const int32_t u = A.qu[q], i = A.qi[q];
  double* R = rec + q * M::R;
  const bool ok_id = (u >= 0 && u < A.U && i >= 0 && i < A.I);
  const int64_t ub = ok_id ? A.ptr[0][u] : 0, du = ok_id ? A.ptr[0][u + 1] - ub : 0;
  const int64_t ib = ok_id ? A.ptr[1][i] : 0, di = ok_id ? A.ptr[1][i + 1] - ib : 0;
  const int64_t n = du + di;
  if (n == 0) {
    if (x_out)
      for (int a = lane; a < D; a += kSolveThreads) x_out[q * D + a] = NAN;
    if (lane == 0) R[M::Rec::inv_n] = NAN;
    return;
  }

  const double rhat_ui = solve_prologue<M, kSolveThreads, true>(A, u, i, th, g, sh, w, sW1, sb1);

  // ---- assemble H (solve.h) and solve ----
  {
    const bool coupled = assemble_hessian<M, true>(A, u, i, n, rhat_ui, g, H);
    for (int a = lane; a < D; a += kSolveThreads) v[a] = g[a];
    wave_lds_sync();

    if (coupled) {
      ldlt_solve<D, true>(H, v, dd, ww, 0, D);
    } else {
      ldlt_solve<D, true>(H, v, dd, ww, 0, Ds);
      ldlt_solve<D, true>(H, v, dd, ww, Ds, D);
    }
    wave_lds_sync();
  }

  solve_epilogue<M>(A, q, u, i, n, rhat_ui, th, g, v, w, R, x_out);
}

// One wave per query, the full D x D packed LDL^T: the queries whose test pair is a train row
// (its Hessian couples the user and item blocks; the side-system solves list them in qlist
// {count, q_0, q_1, ...}).  The word before the count counts this kernel's workgroups as they
// read it: one 64-bit atomic on {readers, count} returns the count and the number of earlier
// readers, and the last reader zeroes both words -- the list is empty again for the next call's
// side-system solve, with no memset and no launch (and the same under a replayed graph).
// (MF k = 16 never lists one: its coupled queries are a role of k_solve_quad.)
template <class M>
__global__ __launch_bounds__(kSolveThreads, (M::Ds <= 33 ? 2 : 1)) void k_solve(QueryArgs A, int64_t Q, double* __restrict__ rec,
                                                         double* __restrict__ x_out, int32_t* __restrict__ qlist) {
  constexpr int K = M::K;
  static_assert(kSolveThreads == 64, "one wave: lane 0's atomic is broadcast by a shuffle");
  unsigned long long rw = 0;
  {
    unsigned long long* word = reinterpret_cast<unsigned long long*>(qlist - 1);
    if (threadIdx.x == 0) {
      rw = atomicAdd(word, 1ull);
      if ((unsigned)(rw & 0xffffffffull) == gridDim.x - 1)
        __hip_atomic_store(word, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    rw = __shfl(rw, 0);
  }
  __shared__ double slab[kFullSlab<M>];
  // NCF weights staged once per block (fp64), read by every query the block solves
  __shared__ NCFWeights<M::ncf ? K : 2> w;
  __shared__ double sW1[M::ncf ? 2 * K * K : 1];
  __shared__ double sb1[M::ncf ? K : 1];
  if constexpr (M::ncf) {
    load_ncf_weights<K>(w, A.t[6], A.t[7], A.t[8]);
    for (int t = threadIdx.x; t < 2 * K * K; t += blockDim.x) sW1[t] = (double)A.t[4][t];
    for (int t = threadIdx.x; t < K; t += blockDim.x) sb1[t] = (double)A.t[5][t];
  }
  const int64_t nwork = (int64_t)(rw >> 32);
  for (int64_t wk = blockIdx.x; wk < nwork; wk += gridDim.x)
    solve_full_wave<M>(A, (int64_t)qlist[1 + wk], rec, x_out, slab, w, sW1, sb1);
}

// Scoring records from a GIVEN inverse HVP (fia_query_batch_x: the reference's cached
// <model>-cg-normal_loss-test-[t].npz when force_refresh is False, mf:210-214): one wave per
// query, theta_t / v / r-hat by the solve prologue, x = x_in (reference theta order)
// instead of a solve, then the solve epilogue's record.
template <class M>
__global__ __launch_bounds__(kSolveThreads) void k_record_x(QueryArgs A, int64_t Q, const double* __restrict__ x_in,
                                                            double* __restrict__ rec, double* __restrict__ x_out) {
  constexpr int K = M::K, D = M::D;
  __shared__ double v[D], g[D], th[D];
  __shared__ double sh[4 * K + 8];
  __shared__ NCFWeights<M::ncf ? K : 2> w;
  __shared__ double sW1[M::ncf ? 2 * K * K : 1];
  __shared__ double sb1[M::ncf ? K : 1];
  if constexpr (M::ncf) {
    load_ncf_weights<K>(w, A.t[6], A.t[7], A.t[8]);
    for (int t = threadIdx.x; t < 2 * K * K; t += blockDim.x) sW1[t] = (double)A.t[4][t];
    for (int t = threadIdx.x; t < K; t += blockDim.x) sb1[t] = (double)A.t[5][t];
  }
  for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
    __syncthreads();
    const int lane = threadIdx.x;
    const int32_t u = A.qu[q], i = A.qi[q];
    double* R = rec + q * M::R;
    const bool ok_id = (u >= 0 && u < A.U && i >= 0 && i < A.I);
    const int64_t n = ok_id ? (A.ptr[0][u + 1] - A.ptr[0][u]) + (A.ptr[1][i + 1] - A.ptr[1][i]) : 0;
    if (n == 0) {
      if (x_out)
        for (int a = lane; a < D; a += kSolveThreads) x_out[q * D + a] = NAN;
      if (lane == 0) R[M::Rec::inv_n] = NAN;
      continue;
    }
    const double rhat_ui = solve_prologue<M, kSolveThreads>(A, u, i, th, g, sh, w, sW1, sb1);
    for (int a = lane; a < D; a += kSolveThreads) v[a] = x_in[q * D + M::ref_index(a)];
    __syncthreads();
    solve_epilogue<M>(A, q, u, i, n, rhat_ui, th, g, v, w, R, x_out);
  }
}

// ------------------------------------------------------------------------------------
// Side-system solve on 16x16 tiles (NCF, MF k >= 32): one wave per (query, side) system.
//
// The side block H_b (NM x NM after the MF bias is eliminated first as a Schur complement)
// lives in registers as its upper tiles U[p][j] (p <= j) in the f64-MFMA C/D layout: lane
// l = 16 g + c holds rows 4 r + g (r = 0..3) of column c.  In that layout a tile is at once
// the A operand of its transpose and the B operand of itself, so the blocked right-looking
// LDL^T needs no transposes:
//   panel p:  the 16 rows of block p, [S | I | U[p][p+1..] | rhs_p], are eliminated by 16
//             pivot steps (VALU; the pivot row goes through a per-wave LDS slot, the
//             multipliers are the same row read at the lane's own rows -- S is symmetric),
//             giving [D L^T | W = L_pp^-1 | Y_j = D Z_j | y_p]
//   trailing: U[i][j] -= Z_i^T Y_j and rhs_i -= Z_i^T y_p on v_mfma_f64_16x16x4_f64, the
//             right-hand side held in "column layout" (every column of its tile = the
//             vector), so the update of the right-hand side is one more MFMA product
//   back:     x_p = W_p^T (z_p - sum_{i>p} Z_i x_i), z_p = D^-1 y_p: a 16-lane DPP row sum
//             and a 4-row permlane sum per block
// Replaces the one-column-per-lane solve (LDS broadcast of every pivot column to every
// lane: LDS-bound, and 256+256 registers with spills at MF k = 64).
// ------------------------------------------------------------------------------------
// waves per SIMD the tile solve is compiled for (registers: 4 tiles of state per 16 coordinates)
template <class M>
constexpr int col_waves() {
  return M::Ds <= 16 ? 4 : 2;     // N = 32: two 32-row columns per lane (128 VGPRs of matrix)
}

template <class M>
constexpr int tile_waves() {
  return (M::ncf ? M::Ds : M::K) <= 32 ? 3 : 2;
}

__device__ __forceinline__ void pin_d4(d4_t& t) {
  double a = t[0], b = t[1], c = t[2], d = t[3];
  asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
  t[0] = a; t[1] = b; t[2] = c; t[3] = d;
}

template <int NT>
__device__ constexpr int ut(int p, int j) { return p * NT - (p * (p - 1)) / 2 + (j - p); }

// Raw loads of one side system (issued together, ahead of the query's dependent prologue):
// the upper tiles of the entity's packed lower Gram G (Ds = NM, + 1 with the MF bias), and
// for the MF bias the bias row at the lane's rows (hr) and column (hc) and its diagonal (hb)
template <int NT, bool EXTRA, bool PAIR = false>
__device__ __forceinline__ void tile_load(const double* __restrict__ G, int g, int c, d4_t (&U)[NT * (NT + 1) / 2],
                                          d4_t (&hr)[NT], double (&hc)[NT], double& hb) {
  // PAIR: NCF k = 16's row-pair Gram layout (gidx)
  auto at = [](int R, int C) { return PAIR ? (R < 16 ? C * 16 + R : (32 - C) * 16 + (31 - R)) : (R * (R + 1)) / 2 + C; };
  constexpr int NM = 16 * NT;
  const double* __restrict__ hrow = G + NM * (NM + 1) / 2;   // MF: packed row NM = the bias row
#pragma unroll
  for (int p = 0; p < NT; ++p)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int R = 16 * p + 4 * r + g;
#pragma unroll
      for (int j = p; j < NT; ++j) {
        const int C = 16 * j + c;
        if (j > p) {
          U[ut<NT>(p, j)][r] = G[at(C, R)];
        } else {
          const int hi = R > C ? R : C, lo = R > C ? C : R;
          U[ut<NT>(p, j)][r] = G[at(hi, lo)];
        }
      }
      if constexpr (EXTRA) hr[p][r] = hrow[R];
    }
  if constexpr (EXTRA) {
#pragma unroll
    for (int j = 0; j < NT; ++j) hc[j] = hrow[16 * j + c];
    hb = hrow[NM];
  }
}

// One side system, from the raw loads: H = (2/n) Gram + (wd + damping) I (the MF bias, not
// decayed, eliminated first: H - h h^T / eta, rhs - h gamma / eta), then the blocked
// LDL^T + solves.  Rt: the right-hand side in column layout (raw, [16p + 4r + g]); gam: its
// bias entry.  xs = the solution [Ds] (LDS, written by lanes 0..15), P = this wave's
// pivot-row slots [2][16 * PS] (LDS).
template <int NT, bool EXTRA>
__device__ void tile_factor(int g, int c, d4_t (&U)[NT * (NT + 1) / 2], d4_t (&Rt)[NT], d4_t (&hr)[NT],
                            double (&hc)[NT], double hb, double gam, double s2n, double wd, double damping,
                            double* __restrict__ xs, double* __restrict__ P) {
  constexpr int NM = 16 * NT, PS = (NT + 3) & ~1;
  d4_t W[NT];
  double ieta = 0.0;
  if constexpr (EXTRA) {
    ieta = 1.0 / (s2n * hb + damping);                       // the bias pivot
#pragma unroll
    for (int j = 0; j < NT; ++j) hc[j] *= s2n;
  }
#pragma unroll
  for (int p = 0; p < NT; ++p)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int R = 16 * p + 4 * r + g;
      const double h = EXTRA ? s2n * hr[p][r] * ieta : 0.0;
#pragma unroll
      for (int j = p; j < NT; ++j) {
        double v = s2n * U[ut<NT>(p, j)][r];
        if (j == p) v += (R == 16 * j + c) ? wd + damping : 0.0;
        if constexpr (EXTRA) v = fma(-h, hc[j], v);
        U[ut<NT>(p, j)][r] = v;
      }
      if constexpr (EXTRA) Rt[p][r] = fma(-h, gam, Rt[p][r]);
    }
  // ---- factor + forward solve, panel by panel ----
#pragma unroll
  for (int p = 0; p < NT; ++p) {
    d4_t I;
#pragma unroll
    for (int r = 0; r < 4; ++r) I[r] = (4 * r + g == c) ? 1.0 : 0.0;
    double dv[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      double* __restrict__ Pb = P + (k & 1) * (16 * PS);
      const int kr = k >> 2, kg = k & 3;
      // pivot row k of the panel: slot [c][t], t = 0 S, 1 I, 2.. U[p][p+1..], last rhs
      if (g == kg) {
        Pb[c * PS + 0] = U[ut<NT>(p, p)][kr];
        Pb[c * PS + 1] = I[kr];
#pragma unroll
        for (int j = p + 1; j < NT; ++j) Pb[c * PS + 1 + j - p] = U[ut<NT>(p, j)][kr];
        Pb[c * PS + NT - p + 1] = Rt[p][kr];
      }
      wave_lds_sync();
      const double dk = Pb[k * PS];
      const double ij = rcp_nr2(dk);
      double f[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (4 * r + 3 <= k) {
          f[r] = 0.0;                                  // rows <= k: finished
        } else {
          const double m = Pb[(4 * r + g) * PS] * ij;  // S[k][row] = S[row][k]
          f[r] = (4 * r > k || g > kg) ? m : 0.0;
        }
      }
      double pv[NT + 2];
#pragma unroll
      for (int t = 0; t < NT - p + 2; ++t) pv[t] = Pb[c * PS + t];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (4 * r + 3 <= k) continue;
        U[ut<NT>(p, p)][r] = fma(-f[r], pv[0], U[ut<NT>(p, p)][r]);
        I[r] = fma(-f[r], pv[1], I[r]);
#pragma unroll
        for (int j = p + 1; j < NT; ++j) U[ut<NT>(p, j)][r] = fma(-f[r], pv[1 + j - p], U[ut<NT>(p, j)][r]);
        Rt[p][r] = fma(-f[r], pv[NT - p + 1], Rt[p][r]);
      }
      if (g == kg) dv[kr] = ij;                        // 1/d of this lane's row k
      // materialise this step's updates here: hipcc otherwise sinks the FMAs of rows not yet
      // needed as pivots to their first use and keeps every step's multipliers live (spills)
      pin_d4(U[ut<NT>(p, p)]);
      pin_d4(I);
#pragma unroll
      for (int j = p + 1; j < NT; ++j) pin_d4(U[ut<NT>(p, j)]);
      pin_d4(Rt[p]);
      asm volatile("" : "+v"(dv[kr]));
    }
    W[p] = I;
    // trailing update: U[i][j] -= Z_i^T Y_j, rhs_i -= Z_i^T y_p; keep -Z_i for the back solve
#pragma unroll
    for (int i = p + 1; i < NT; ++i) {
      d4_t Zn;
#pragma unroll
      for (int r = 0; r < 4; ++r) Zn[r] = -U[ut<NT>(p, i)][r] * dv[r];
#pragma unroll
      for (int j = i; j < NT; ++j)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
          U[ut<NT>(i, j)] = __builtin_amdgcn_mfma_f64_16x16x4f64(Zn[kb], U[ut<NT>(p, j)][kb], U[ut<NT>(i, j)], 0, 0, 0);
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
        Rt[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(Zn[kb], Rt[p][kb], Rt[i], 0, 0, 0);
      U[ut<NT>(p, i)] = Zn;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) Rt[p][r] *= dv[r];     // z_p = D^-1 y_p
  }
  // ---- back solve: x_p = W_p^T (z_p - sum_{i>p} Z_i x_i), x in row layout (lane c) ----
  double xr[NT];
#pragma unroll
  for (int p = NT - 1; p >= 0; --p) {
    double pw = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double w = Rt[p][r];
      if (p + 1 < NT) {
        double s = 0.0;
#pragma unroll
        for (int i = p + 1; i < NT; ++i) s = fma(U[ut<NT>(p, i)][r], xr[i], s);   // (-Z x)[4r+g]
        w += row_sum16(s);
      }
      pw = fma(W[p][r], w, pw);
    }
    xr[p] = col_sum4(pw);
  }
  if constexpr (EXTRA) {                               // the bias: (gamma - h . x) / eta
    double part = 0.0;
#pragma unroll
    for (int j = 0; j < NT; ++j) part = fma(hc[j], xr[j], part);
    part = g == 0 ? part : 0.0;
    const double hx = wave_sum(part);
    if ((threadIdx.x & 63) == 0) xs[NM] = (gam - hx) * ieta;
  }
  if (g == 0) {
#pragma unroll
    for (int p = 0; p < NT; ++p) xs[16 * p + c] = xr[p];
  }
}

// Two waves per query (wave w = side w: user block, item block), persistent over queries;
// NCF weights staged once per workgroup.  Every global load of a query (ids of the next
// query, list pointers, the pair-set probe, both Gram blocks, MF: the right-hand side) is
// issued before its first dependent use, so a query waits on about two memory latencies.
// Queries whose test pair is a train row (coupled blocks) go to `coupled` {count, q...} for
// the full-D k_solve<M, false>.
template <class M>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(tile_waves<M>()))) void k_solve_tile(
    QueryArgs A, int64_t Q, double* __restrict__ rec, double* __restrict__ x_out, int32_t* __restrict__ coupled_out) {
  constexpr int K = M::K, Ds = M::Ds, D = M::D, GS = Ds * (Ds + 1) / 2, GSP = (GS + 1) & ~1;
  constexpr bool EXTRA = !M::ncf;
  constexpr int NM = EXTRA ? K : Ds, NT = NM / 16, PS = (NT + 3) & ~1, NU = NT * (NT + 1) / 2;
  static_assert(NM % 16 == 0 && NT >= 1 && NT <= 4, "tile solve: 16..64 matrix coordinates");
  __shared__ double th[D], g[D], xs[D];
  __shared__ double Pv[2][2 * 16 * PS];
  __shared__ double sh[4 * K + 8];
  __shared__ NCFWeights<M::ncf ? K : 2> w;
  __shared__ double sW1[M::ncf ? 2 * K * K : 1];
  __shared__ double sb1[M::ncf ? K : 1];
  const int wv = threadIdx.x >> 6;
  if constexpr (M::ncf) {
    load_ncf_weights<K>(w, A.t[6], A.t[7], A.t[8]);
    for (int t = threadIdx.x; t < 2 * K * K; t += blockDim.x) sW1[t] = (double)A.t[4][t];
    for (int t = threadIdx.x; t < K; t += blockDim.x) sb1[t] = (double)A.t[5][t];
  }
  int64_t q = blockIdx.x;
  int32_t un = q < Q ? A.qu[q] : 0, in = q < Q ? A.qi[q] : 0;
  for (; q < Q; q += gridDim.x) {
    const int32_t u = un, i = in;
    if (q + gridDim.x < Q) {                           // the next query's ids, in flight
      un = A.qu[q + gridDim.x];
      in = A.qi[q + gridDim.x];
    }
    __syncthreads();                                   // LDS reuse across queries
    int lane = threadIdx.x & 63;                       // opaque per query (no hoisted addresses)
    asm volatile("" : "+v"(lane));
    const int lg = lane >> 4, lc = lane & 15;
    const bool ok_id = (u >= 0 && u < A.U && i >= 0 && i < A.I);
    const int32_t uu = ok_id ? u : 0, ii = ok_id ? i : 0;
    const int64_t pu0 = A.ptr[0][uu], pu1 = A.ptr[0][uu + 1], pi0 = A.ptr[1][ii], pi1 = A.ptr[1][ii + 1];
    const unsigned long long pkey = (unsigned long long)uu * (unsigned long long)A.I + (unsigned long long)ii;
    unsigned long long ph, pk;
    A.pairs.probe_start(pkey, ph, pk);
    const int32_t ent = wv ? ii : uu;
    d4_t U[NU], Rt[NT], hr[NT];
    double hc[NT], hb = 0.0, gam = 0.0;
    // NT <= 2: the Gram loads go out before the prologue (one memory latency per query); at
    // NT >= 3 holding the raw tiles across the prologue spills (MF k=64: 0.42 vs 0.35 ms), so
    // they are issued after it
    constexpr bool EARLY = NT <= 2;
    if constexpr (EARLY) tile_load<NT, EXTRA, pair_layout<M>()>(A.gram[wv] + (int64_t)ent * GSP, lg, lc, U, hr, hc, hb);
    if constexpr (EXTRA) {                             // MF rhs: [other side's embedding ; 1]
      const float* __restrict__ Eo = A.t[wv ? 0 : 1] + (int64_t)(wv ? uu : ii) * K;
#pragma unroll
      for (int p = 0; p < NT; ++p)
#pragma unroll
        for (int r = 0; r < 4; ++r) Rt[p][r] = (double)Eo[16 * p + 4 * r + lg];
      gam = 1.0;
    }
    const int64_t n = ok_id ? (pu1 - pu0) + (pi1 - pi0) : 0;
    if (n == 0) {
      if (wv == 0) {
        if (x_out)
          for (int a = lane; a < D; a += 64) x_out[q * D + a] = NAN;
        if (lane == 0) rec[q * M::R + M::Rec::inv_n] = NAN;
      }
      continue;
    }
    const double s2n = 2.0 / (double)n;
    const double rhat_ui = solve_prologue<M, 128>(A, u, i, th, g, sh, w, sW1, sb1);
    if constexpr (!EXTRA) {                            // NCF rhs from the prologue
#pragma unroll
      for (int p = 0; p < NT; ++p)
#pragma unroll
        for (int r = 0; r < 4; ++r) Rt[p][r] = g[wv * Ds + 16 * p + 4 * r + lg];
    }
    double cdup, rsum;
    A.pairs.probe_finish(pkey, ph, pk, cdup, rsum);
    if (cdup > 0.0) {
      if (threadIdx.x == 0) coupled_append(coupled_out, q);
      continue;
    }
    if constexpr (!EARLY) tile_load<NT, EXTRA, pair_layout<M>()>(A.gram[wv] + (int64_t)ent * GSP, lg, lc, U, hr, hc, hb);
    tile_factor<NT, EXTRA>(lg, lc, U, Rt, hr, hc, hb, gam, s2n, A.wd, A.damping, xs + wv * Ds, &Pv[wv][0]);
    __syncthreads();
    if (wv == 0) solve_epilogue<M>(A, q, u, i, n, rhat_ui, th, g, xs, w, rec + q * M::R, x_out);
  }
}

// ------------------------------------------------------------------------------------
// NCF k <= 16 (side blocks of N = 2k <= 32): QW = 32 / k queries per wave.  A side system
// lives in LS = N / 2 lanes (the user block, then the item block, of each query), lane t
// owning columns t and t + LS in registers: a right-looking LDL^T in which step j publishes
// the pivot column through LDS (every lane stores its two entries A[c][j] = col_c[j]) and
// reads it back as uniform-address ds_read_b128 broadcasts, each value feeding TWO FMAs (one
// per owned column: half the LDS traffic per FMA of a column-per-lane layout, which is what
// bounds this solve).  The forward solve rides along; the backward solve broadcasts x_j by
// DPP row_newbcast.  Every global load of a query is issued before its prologue.
// ------------------------------------------------------------------------------------
// sum over the 2 * LS lanes of one query (its two side systems), every lane of it gets the
// same bits: LS = 16 -- a 16-lane row sum, then rows 2h + 1 and 2h; LS = 8 -- a row sum
template <int LS>
__device__ __forceinline__ double sys_sum(double x) {
  x = row_sum16(x);
  if constexpr (LS == 16) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)(b & 0xffffffffll), hi = (unsigned)(b >> 32);
    const auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    x = __longlong_as_double(((long long)h16[0] << 32) | l16[0]) +
        __longlong_as_double(((long long)h16[1] << 32) | l16[1]);
  } else {
    static_assert(LS == 8, "k = 8 or 16");
  }
  return x;
}

template <int N, int J>
__device__ __forceinline__ double bcast_sys(double x, int t) {
  // lane (J % LS) of each LS-lane system; LS = 16: one system per DPP row, LS = 8: two
  constexpr int LS = N / 2;
  if constexpr (LS == 16) {
    return dpp_d<0x150 + (J % 16)>(x);
  } else {
    static_assert(LS == 8, "k = 8 or 16");
    const double lo = dpp_d<0x150 + (J % 8)>(x), hi = dpp_d<0x150 + 8 + (J % 8)>(x);
    return t >= 0 && (threadIdx.x & 8) ? hi : lo;
  }
}

// NCF prologue for QW queries per wave (LQ = 64 / QW lanes per query): theta_t, v and r-hat
// (ncf:102-145, 181-191; gnn:155) into th[h][D] / g[h][D]; rh[h] = r-hat(u,i)
template <class M, int QW>
__device__ void ncf_prologue_multi(const QueryArgs& A, const int32_t* __restrict__ uq, const int32_t* __restrict__ iq,
                                   double (*th)[M::D], double (*g)[M::D], double (*sh)[4 * M::K + 8],
                                   const NCFWeights<M::K>& w, const double* __restrict__ sW1,
                                   const double* __restrict__ sb1, double* __restrict__ rh) {
  constexpr int K = M::K, Ds = M::Ds, H2 = K / 2, LQ = 64 / QW;
  static_assert(2 * K <= LQ, "one lane per g entry");
  const int h = threadIdx.x / LQ, a = threadIdx.x % LQ;
  const int32_t u = uq[h], i = iq[h];
  double* __restrict__ z1 = sh[h];
  double* __restrict__ d2 = sh[h] + K;
  double* __restrict__ d1 = sh[h] + 2 * K;
  if (a < K) {
    th[h][a] = A.t[0][(int64_t)u * K + a];
    th[h][K + a] = A.t[2][(int64_t)u * K + a];
    th[h][Ds + a] = A.t[1][(int64_t)i * K + a];
    th[h][Ds + K + a] = A.t[3][(int64_t)i * K + a];
    z1[a] = A.l1[0][(int64_t)u * K + a] + A.l1[1][(int64_t)i * K + a] + sb1[a];
  }
  wave_lds_sync();
  double part = 0.0;
  if (a < H2) {
    double z2 = w.b2[a];
#pragma unroll
    for (int c = 0; c < K; ++c) z2 = fma(w.W2[c * H2 + a], z1[c] > 0.0 ? z1[c] : 0.0, z2);
    const bool on = z2 > 0.0;
    d2[a] = on ? w.W3[a] : 0.0;
    part = on ? w.W3[a] * z2 : 0.0;
  }
  if (a < K) part += w.W3[H2 + a] * th[h][K + a] * th[h][Ds + K + a];
#pragma unroll
  for (int off = LQ / 2; off > 0; off >>= 1) part += __shfl_xor(part, off);
  if (a == 0) rh[h] = part + (double)A.t[9][0];
  wave_lds_sync();
  if (a < K) {
    double t = 0.0;
#pragma unroll
    for (int dd = 0; dd < H2; ++dd) t = fma(w.W2[a * H2 + dd], d2[dd], t);
    d1[a] = z1[a] > 0.0 ? t : 0.0;
  }
  wave_lds_sync();
  if (a < 2 * K) {
    // rows a < K: W1[:k] (Pm part, user block); rows a >= K: W1[k:] (Qm part, item block)
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < K; ++c) s = fma(sW1[a * K + c], d1[c], s);
    if (a < K) g[h][a] = s; else g[h][Ds + (a - K)] = s;
  }
  if (a < K) {
    g[h][K + a] = w.W3[H2 + a] * th[h][Ds + K + a];        // d r/d Pg_u = W3g * Qg_i
    g[h][Ds + K + a] = w.W3[H2 + a] * th[h][K + a];        // d r/d Qg_i = W3g * Pg_u
  }
  wave_lds_sync();
}

// Pivot slots of one system: [0, N) the pivot column, N y_J, N + 1 1/d_J.  Every lane
// writes its two entries of column J; the owners of row J add y_J and 1/d_J.
template <int N, int J>
__device__ __forceinline__ void ncf2_publish(const double (&c0)[N], const double (&c1)[N], double y0, double y1,
                                             int t, double* __restrict__ Pb) {
  constexpr int LS = N / 2;
  const int ca = t, cb = t + LS;
  Pb[ca] = c0[J];                                  // A[ca][J] = col_ca[J] (symmetric)
  Pb[cb] = c1[J];
  if (ca == J || cb == J) {                        // the diagonal's owner: y_J and 1/d_J
    const double dj = ca == J ? c0[J] : c1[J];
    const double ij = rcp_nr2(dj);
    Pb[N] = ca == J ? y0 : y1;
    Pb[N + 1] = ij;
  }
}

// Step J, software-pipelined: the pivot data of step J are in LDS; row J + 1 is updated
// first and published (with y_{J+1} and 1/d_{J+1}) before the remaining FMAs of step J, so
// the next step's LDS round trip overlaps them.
template <int N, int J>
__device__ __forceinline__ void ncf2_step(double (&c0)[N], double (&c1)[N], double& y0, double& y1,
                                          double& di0, double& di1, int t, double* __restrict__ P0,
                                          double* __restrict__ P1) {
  constexpr int LS = N / 2;
  const int ca = t, cb = t + LS;
  double* __restrict__ Pb = (J & 1) ? P1 : P0;
  double* __restrict__ Pn = (J & 1) ? P0 : P1;
  wave_lds_sync();
  const double ij = Pb[N + 1], yj = Pb[N];
  if (ca == J) di0 = ij;
  if (cb == J) di1 = ij;
  const double f0 = ca > J ? c0[J] * ij : 0.0;
  const double f1 = cb > J ? c1[J] * ij : 0.0;
  y0 = fma(-f0, yj, y0);
  y1 = fma(-f1, yj, y1);
  if constexpr (J + 1 < N) {
    const double p = Pb[J + 1];
    c0[J + 1] = fma(-p, f0, c0[J + 1]);
    c1[J + 1] = fma(-p, f1, c1[J + 1]);
    ncf2_publish<N, J + 1>(c0, c1, y0, y1, t, Pn);
  }
#pragma unroll
  for (int r = J + 2; r < N; ++r) {
    const double p = Pb[r];
    c0[r] = fma(-p, f0, c0[r]);
    c1[r] = fma(-p, f1, c1[r]);
  }
  if (ca > J) c0[J] = f0;                          // L[ca][J]
  if (cb > J) c1[J] = f1;
  // materialise this step's updates here (hipcc otherwise sinks each row's FMA to the step
  // that first needs it and keeps every step's pivot values live: spills)
#pragma unroll
  for (int r = J; r < N; ++r) asm volatile("" : "+v"(c0[r]), "+v"(c1[r]));
  asm volatile("" : "+v"(y0), "+v"(y1));
}

template <int N, int J>
__device__ __forceinline__ void ncf2_steps(double (&c0)[N], double (&c1)[N], double& y0, double& y1, double& di0,
                                           double& di1, int t, double* __restrict__ P0, double* __restrict__ P1) {
  if constexpr (J < N) {
    ncf2_step<N, J>(c0, c1, y0, y1, di0, di1, t, P0, P1);
    ncf2_steps<N, J + 1>(c0, c1, y0, y1, di0, di1, t, P0, P1);
  }
}

template <int N, int J>
__device__ __forceinline__ void ncf2_back(const double (&c0)[N], const double (&c1)[N], double& y0, double& y1,
                                          double di0, double di1, int t) {
  // L^T x = D^-1 y from the last row: x_J (final in its owner lane) is broadcast to the
  // system's lanes, every lane with a column c < J removes L[J][c] x_J
  if constexpr (J >= 0) {
    constexpr int LS = N / 2;
    const double own = (J < LS) ? y0 : y1;
    const double xj = bcast_sys<N, J>(own, t);
    const int ca = t, cb = t + LS;
    if (ca < J) y0 = fma(-c0[J] * di0, xj, y0);
    if (cb < J) y1 = fma(-c1[J] * di1, xj, y1);
    ncf2_back<N, J - 1>(c0, c1, y0, y1, di0, di1, t);
  }
}

template <class M>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(col_waves<M>()))) void k_solve_col(
    QueryArgs A, int64_t Q, double* __restrict__ rec, double* __restrict__ x_out, int32_t* __restrict__ coupled_out) {
  constexpr int K = M::K, Ds = M::Ds, D = M::D, GS = Ds * (Ds + 1) / 2, GSP = (GS + 1) & ~1, N = Ds;
  constexpr int LS = N / 2, NSYS = 64 / LS, QW = NSYS / 2, PSTR = N + 2;
  static_assert(M::ncf && (N == 16 || N == 32), "NCF k = 8 or 16");
  __shared__ double th[QW][D], g[QW][D], sh[QW][4 * K + 8], rh[QW], s_cd[QW];
  __shared__ int32_t s_u[QW], s_i[QW];
  __shared__ int64_t s_n[QW];
  __shared__ double Pv[2][NSYS * PSTR];
  __shared__ NCFWeights<K> w;
  __shared__ double sW1[2 * K * K];
  __shared__ double sb1[K];
  load_ncf_weights<K>(w, A.t[6], A.t[7], A.t[8]);
  for (int t = threadIdx.x; t < 2 * K * K; t += blockDim.x) sW1[t] = (double)A.t[4][t];
  for (int t = threadIdx.x; t < K; t += blockDim.x) sb1[t] = (double)A.t[5][t];
  const int64_t stride = (int64_t)gridDim.x * QW;
  for (int64_t q0 = (int64_t)blockIdx.x * QW; q0 < Q; q0 += stride) {
    __syncthreads();
    // lane-derived values made opaque per iteration: hoisted out of the loop, the 2N column
    // addresses and lane masks would stay live across it (spills)
    int lane = threadIdx.x;
    asm volatile("" : "+v"(lane));
    const int sys = lane / LS, t = lane % LS, qs = sys >> 1, sd = sys & 1;
    // lane h < QW: query q0 + h -- ids, related count, first pair-set probe
    unsigned long long pk = 0, ph = 0, pv = 0;
    if (lane < QW) {
      const int64_t q = q0 + lane;
      const int32_t u = q < Q ? A.qu[q] : -1, i = q < Q ? A.qi[q] : -1;
      const bool ok = u >= 0 && u < A.U && i >= 0 && i < A.I;
      const int32_t uu = ok ? u : 0, ii = ok ? i : 0;
      const int64_t nn = ok ? (A.ptr[0][uu + 1] - A.ptr[0][uu]) + (A.ptr[1][ii + 1] - A.ptr[1][ii]) : 0;
      pk = (unsigned long long)uu * (unsigned long long)A.I + (unsigned long long)ii;
      A.pairs.probe_start(pk, ph, pv);
      s_u[lane] = uu;                                // clamped ids (n = 0 for invalid ones)
      s_i[lane] = ii;
      s_n[lane] = nn;
    }
    wave_lds_sync();
    const int32_t ent = sd ? s_i[qs] : s_u[qs];
    const double* __restrict__ Gb = A.gram[sd] + (int64_t)ent * GSP;
    const int ca = t, cb = t + LS;
    // the prologue first: holding the 2N loaded columns across it spills
    ncf_prologue_multi<M, QW>(A, s_u, s_i, th, g, sh, w, sW1, sb1, rh);
    double c0[N], c1[N];
#pragma unroll
    for (int r = 0; r < N; ++r) {
      const int h0 = r > ca ? r : ca, l0 = r > ca ? ca : r;
      const int h1 = r > cb ? r : cb, l1 = r > cb ? cb : r;
      c0[r] = Gb[gidx<M>(h0, l0)];
      c1[r] = Gb[gidx<M>(h1, l1)];
    }
    const int64_t n = s_n[qs];
    // H_b = (2/n) Gram_b + (wd + damping) I  (every NCF coordinate is decayed); n = 0: the
    // system is garbage and its query writes NaN below
    const double s2n = n > 0 ? 2.0 / (double)n : 0.0;
#pragma unroll
    for (int r = 0; r < N; ++r) {
      c0[r] *= s2n;
      c1[r] *= s2n;
    }
#pragma unroll
    for (int r = 0; r < N; ++r) {
      if (r == ca) c0[r] += A.wd + A.damping;
      if (r == cb) c1[r] += A.wd + A.damping;
    }
    double y0 = g[qs][sd * N + ca], y1 = g[qs][sd * N + cb];
    const double g0 = y0, g1 = y1;
    ncf2_publish<N, 0>(c0, c1, y0, y1, t, &Pv[0][sys * PSTR]);
    double di0 = 0.0, di1 = 0.0;
    ncf2_steps<N, 0>(c0, c1, y0, y1, di0, di1, t, &Pv[0][sys * PSTR], &Pv[1][sys * PSTR]);
    y0 *= di0;
    y1 *= di1;
    ncf2_back<N, N - 1>(c0, c1, y0, y1, di0, di1, t);
    if (lane < QW) {                                 // is the test pair a train row?
      double cdup, rsum;
      A.pairs.probe_finish(pk, ph, pv, cdup, rsum);
      s_cd[lane] = cdup;
    }
    wave_lds_sync();
    // ---- record + x_out, lane-parallel: this lane holds x at coordinates ca, cb of side sd
    // of query qs ----
    {
      const int64_t q = q0 + qs;
      const int64_t nn = s_n[qs];
      const bool live_q = q < Q && nn > 0 && !(s_cd[qs] > 0.0);
      constexpr int H2 = K / 2;
      using L = typename M::Rec;
      // x . theta over the decayed coordinates (all of NCF's) and x . v, summed over the query's
      // two systems (2 LS lanes)
      double cq = fma(y0, th[qs][sd * N + ca], y1 * th[qs][sd * N + cb]);
      double xv = fma(y0, g0, y1 * g1);
      cq = sys_sum<LS>(cq);
      xv = sys_sum<LS>(xv);
      if (live_q) {
        double* __restrict__ R = rec + q * M::R;
        double* __restrict__ S = L::side(R, sd);
        if (sd == 0 && t == 0) {
          R[L::inv_n] = 1.0 / (double)nn;
          R[L::c_q] = cq * A.wd;
          R[L::x_v] = xv;
          R[L::rhat] = rh[qs];
        }
        // block coordinates: [0, K) mlp, [K, 2K) gmf = x_mlp and w3g_x_gmf, which lie back to back
        S[ca] = ca < K ? y0 : w.W3[H2 + ca - K] * y0;
        S[cb] = cb < K ? y1 : w.W3[H2 + cb - K] * y1;
        if (t == 0) S[L::dup_other] = (double)(sd ? s_u[qs] : s_i[qs]);
        if (x_out) {
          x_out[q * D + M::ref_index(sd * Ds + ca)] = y0;
          x_out[q * D + M::ref_index(sd * Ds + cb)] = y1;
        }
      } else if (q < Q && nn == 0) {
        if (x_out) {
          x_out[q * D + sd * Ds + ca] = NAN;
          x_out[q * D + sd * Ds + cb] = NAN;
        }
        if (sd == 0 && t == 0) rec[q * M::R + M::Rec::inv_n] = NAN;
      } else if (q < Q && sd == 0 && t == 0) {
        coupled_append(coupled_out, q);
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// NCF k = 16 side-system solve by rows (the default for NCF k = 16), two launches:
//  k_ncf_query_pro: one THREAD per query -- n, the pair-set lookup, r-hat(u,i) and
//    v = d r-hat / d theta_t in block order (ncf:102-145, 181-191; gnn:155) into
//    qpro[q] (QPro, kern.h).  The MLP is ~0.8 k FMAs per query; computed
//    wave-cooperatively inside the solve (k_solve_col) it took a fifth of that kernel
//    (LDS round trips between tiny loops, by s_memtime stamps of a diagnostic build).
//  k_solve_rows: 16 lanes per side system (4 systems = 2 queries per wave); lane t owns rows
//    t and 31 - t of the lower triangle, 33 entries, loaded from the Gram's row-pair layout
//    (gidx: one 128-B line per slot and system).  Right-looking LDL^T: step J publishes the
//    pivot column through LDS and every lane updates its two rows; a row's entries live in
//    a[16] (row t) / b[32] (row 31 - t), slots past a row's end are scratch, so no FMA needs
//    a mask -- 616 FMAs per lane for the 4 systems (the column layout's full-column updates:
//    992) at 96 VGPRs of matrix instead of 128 + spills.  Column J + 1 is updated and
//    published before the rest of step J, so the LDS round trip overlaps those FMAs; the
//    forward solve rides along, the backward solve is one 16-lane DPP sum per row.
// ------------------------------------------------------------------------------------
constexpr int kRowsRG = 8;         // pivot reads per group
constexpr int kRowsWaves = 2;      // 198 VGPRs, no spills; at 3 waves (168 VGPRs) 34 spill: 0.252 vs 0.220 ms at yelp-ex

template <class M>
__global__ __launch_bounds__(256) void k_ncf_query_pro(QueryArgs A, int64_t Q, double* __restrict__ qpro) {
  constexpr int K = M::K, H2 = K / 2, Ds = M::Ds;
  using PL = QPro<M>;
  constexpr int EPL = H2 / 4, GPL = 2 * K / 4, FPL = K / 4;   // per-lane shares of a query's outputs
  static_assert(H2 % 4 == 0, "k a multiple of 8");
  // the MLP weights as fp64 in LDS, read per use as broadcasts (per-use scalar loads of the
  // fp32 tables expose a memory latency per weight)
  __shared__ double sW1[2 * K * K], sW2[K * H2], sW3[3 * H2], sb1[K], sb2[H2];
  for (int e = threadIdx.x; e < 2 * K * K; e += 256) sW1[e] = (double)A.t[4][e];
  for (int e = threadIdx.x; e < K * H2; e += 256) sW2[e] = (double)A.t[6][e];
  for (int e = threadIdx.x; e < 3 * H2; e += 256) sW3[e] = (double)A.t[8][e];
  for (int e = threadIdx.x; e < K; e += 256) sb1[e] = (double)A.t[5][e];
  for (int e = threadIdx.x; e < H2; e += 256) sb2[e] = (double)A.t[7][e];
  __syncthreads();
  // four lanes per query (quad sub = 0..3): each computes a quarter of z2 / g / the gmf terms;
  // every lane of a quad stays active for the quad exchanges
  const int sub = threadIdx.x & 3, base = threadIdx.x & 63 & ~3;
  const int64_t q0 = (int64_t)blockIdx.x * 64 + (threadIdx.x >> 2);
  const bool qok = q0 < Q;
  const int64_t q = qok ? q0 : Q - 1;
  const int32_t u = A.qu[q], i = A.qi[q];
  const bool ok = u >= 0 && u < A.U && i >= 0 && i < A.I;
  const int32_t uu = ok ? u : 0, ii = ok ? i : 0;         // clamped ids (n = 0 for invalid ones)
  const double* __restrict__ l1u = A.l1[0] + (int64_t)uu * K;
  const double* __restrict__ l1i = A.l1[1] + (int64_t)ii * K;
  double z1[K];
#pragma unroll
  for (int a = 0; a < K; ++a) z1[a] = l1u[a] + l1i[a] + sb1[a];
  double d2o[EPL], part = 0.0;
#pragma unroll
  for (int m = 0; m < EPL; ++m) {                 // hidden unit e = m * 4 + sub
    const int e = m * 4 + sub;
    double z2 = sb2[e];
#pragma unroll
    for (int c = 0; c < K; ++c) z2 = fma(sW2[c * H2 + e], z1[c] > 0.0 ? z1[c] : 0.0, z2);
    const bool on = z2 > 0.0;
    d2o[m] = on ? sW3[e] : 0.0;
    part += on ? sW3[e] * z2 : 0.0;
  }
  double d2[H2];
#pragma unroll
  for (int e = 0; e < H2; ++e) d2[e] = __shfl(d2o[e / 4], base + (e & 3));
  double* __restrict__ P = qpro + q * PL::stride;
  const float* __restrict__ pg = A.t[2] + (int64_t)uu * K;
  const float* __restrict__ qg = A.t[3] + (int64_t)ii * K;
#pragma unroll
  for (int m = 0; m < FPL; ++m) {
    const int a = m * 4 + sub;
    const double w3g = sW3[H2 + a], pga = (double)pg[a], qga = (double)qg[a];
    part += w3g * pga * qga;
    if (qok) {
      P[PL::v + K + a] = w3g * qga;            // d r / d Pg_u = W3g * Qg_i
      P[PL::v + Ds + K + a] = w3g * pga;       // d r / d Qg_i = W3g * Pg_u
    }
  }
  double d1[K];
#pragma unroll
  for (int c = 0; c < K; ++c) {
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < H2; ++e) s = fma(sW2[c * H2 + e], d2[e], s);
    d1[c] = z1[c] > 0.0 ? s : 0.0;
  }
#pragma unroll
  for (int m = 0; m < GPL; ++m) {      // rows a < K: W1[:k] (user block), a >= K: W1[k:] (item block)
    const int a = m * 4 + sub;
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < K; ++c) s = fma(sW1[a * K + c], d1[c], s);
    if (qok) P[PL::v + (a < K ? a : Ds + (a - K))] = s;
  }
  part += __shfl_xor(part, 1);
  part += __shfl_xor(part, 2);
  if (sub == 0 && qok) {
    const int64_t n = ok ? (A.ptr[0][uu + 1] - A.ptr[0][uu]) + (A.ptr[1][ii + 1] - A.ptr[1][ii]) : 0;
    double cdup, rsum;
    A.pairs.lookup((unsigned long long)uu * (unsigned long long)A.I + (unsigned long long)ii, cdup, rsum);
    P[PL::rhat] = part + (double)A.t[9][0];
    P[PL::n] = (double)n;
    P[PL::cdup] = cdup;
    P[PL::pad] = 0.0;
  }
}

// Step J of k_solve_rows.  P0 / P1: the pivot slots of even / odd steps ([0, 32) the
// column's rows, 32 y_J); lt / lb: the multipliers of rows t / 31 - t (0 unless the row is
// strictly below the pivot, so finished rows and the pivot row take no update).
template <int J>
__device__ __forceinline__ void rows_step(double (&a)[16], double (&b)[32], double& yt, double& yb, double& dit,
                                          double& dib, int t, double* __restrict__ P0, double* __restrict__ P1) {
  const double* __restrict__ Pb = (J & 1) ? P1 : P0;
  double* __restrict__ Pn = (J & 1) ? P0 : P1;
  const int tb = 31 - t;
  wave_lds_sync();
  const double dj = Pb[J], yj = Pb[32];
  const double ij = rcp_nr2(dj);
  double lt = 0.0;
  if constexpr (J < 16) lt = t > J ? a[J] * ij : 0.0;
  const double lb = tb > J ? b[J] * ij : 0.0;
  if (t == J) dit = ij;
  if (tb == J) dib = ij;
  yt = fma(-lt, yj, yt);
  yb = fma(-lb, yj, yb);
  if constexpr (J + 1 < 32) {
    // column J + 1 first, then published for step J + 1 (with y_{J+1} by its owner)
    const double p = Pb[J + 1];
    if constexpr (J + 1 < 16) {
      a[J + 1] = fma(-lt, p, a[J + 1]);
      Pn[t] = a[J + 1];
    }
    b[J + 1] = fma(-lb, p, b[J + 1]);
    Pn[tb] = b[J + 1];
    if constexpr (J + 1 < 16) {
      if (t == J + 1) Pn[32] = yt;
    } else {
      if (tb == J + 1) Pn[32] = yb;
    }
  }
  // the pivot reads in groups of RG columns (a compiler barrier between groups): all of a
  // step's reads hoisted together hold 62 more VGPRs
#pragma unroll
  for (int c = J + 2; c < 16; ++c) {
    if ((c - J - 2) % kRowsRG == kRowsRG - 1) asm volatile("" ::: "memory");
    const double p = Pb[c];
    a[c] = fma(-lt, p, a[c]);
    b[c] = fma(-lb, p, b[c]);
  }
#pragma unroll
  for (int c = (J + 2 > 16 ? J + 2 : 16); c < 32; ++c) {
    if ((c - J - 2) % kRowsRG == kRowsRG - 1) asm volatile("" ::: "memory");
    b[c] = fma(-lb, Pb[c], b[c]);
  }
  if constexpr (J < 16) a[J] = lt;                 // L[t][J], L[31 - t][J]
  b[J] = lb;
  // materialise this step's updates here (hipcc otherwise sinks each row's FMA to the step
  // that first needs it and keeps every step's multipliers live: spills)
#pragma unroll
  for (int c = (J < 16 ? J : 16); c < 16; ++c) asm volatile("" : "+v"(a[c]));
#pragma unroll
  for (int c = J; c < 32; ++c) asm volatile("" : "+v"(b[c]));
  asm volatile("" : "+v"(yt), "+v"(yb));
}

template <int J>
__device__ __forceinline__ void rows_steps(double (&a)[16], double (&b)[32], double& yt, double& yb, double& dit,
                                           double& dib, int t, double* __restrict__ P0, double* __restrict__ P1) {
  if constexpr (J < 32) {
    rows_step<J>(a, b, yt, yb, dit, dib, t, P0, P1);
    rows_steps<J + 1>(a, b, yt, yb, dit, dib, t, P0, P1);
  }
}

// L^T x = z from the last row: x_J = z_J - sum_{r > J} L[r][J] x_r, the sum over the system's
// 16 lanes (each holds L[t][J] x_t + L[31-t][J] x_{31-t}; 0 for rows not below J)
template <int J>
__device__ __forceinline__ void rows_back(const double (&a)[16], const double (&b)[32], double zt, double zb,
                                          double& xt, double& xb, int t) {
  if constexpr (J >= 0) {
    double s = b[J] * xb;
    if constexpr (J < 16) s = fma(a[J], xt, s);
    s = row_sum16(s);
    if constexpr (J < 16) {
      if (t == J) xt = zt - s;
    } else {
      if (31 - t == J) xb = zb - s;
    }
    rows_back<J - 1>(a, b, zt, zb, xt, xb, t);
  }
}

template <class M>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kRowsWaves))) void k_solve_rows(
    QueryArgs A, int64_t Q, const double* __restrict__ qpro, double* __restrict__ rec, double* __restrict__ x_out,
    int32_t* __restrict__ coupled_out) {
  static_assert(pair_layout<M>(), "NCF k = 16 (side blocks of 32)");
  constexpr int K = M::K, H2 = K / 2, Ds = M::Ds, D = M::D, GS = Ds * (Ds + 1) / 2, GSP = (GS + 1) & ~1;
  constexpr int PST = 36;   // 36 doubles: the 4 systems' slots in distinct banks
  using PL = QPro<M>;
  using L = typename M::Rec;
  __shared__ double Pv[2][4 * PST];
  const int lane = threadIdx.x, sys = lane >> 4, t = lane & 15, h = sys >> 1, sd = sys & 1, tb = 31 - t;
  const int64_t q = (int64_t)blockIdx.x * 2 + h;
  const bool qok = q < Q;
  const int64_t qc = qok ? q : Q - 1;
  const int32_t u = A.qu[qc], i = A.qi[qc];
  const bool okid = u >= 0 && u < A.U && i >= 0 && i < A.I;
  const int32_t uu = okid ? u : 0, ii = okid ? i : 0;
  const int32_t ent = sd ? ii : uu;
  const double* __restrict__ Gb = A.gram[sd] + (int64_t)ent * GSP + t;
  const double* __restrict__ P = qpro + qc * PL::stride;
  double a[16], b[32];
#pragma unroll
  for (int s = 0; s <= 32; ++s) {                 // slot s: row t col s | row 31 - t col 32 - s
    const double v = Gb[s * 16];
    if (s < 16) a[s] = v;
    if (s >= 1) b[32 - s] = v;
  }
  const double nd = P[PL::n];
  // H_b = (2/n) Gram_b + (wd + damping) I  (every NCF coordinate is decayed); n = 0: the
  // system is garbage and its query writes NaN below
  const double s2n = nd > 0.0 ? 2.0 / nd : 0.0;
  const double lam = A.wd + A.damping;
#pragma unroll
  for (int c = 0; c < 16; ++c) a[c] *= s2n;
#pragma unroll
  for (int c = 0; c < 32; ++c) b[c] *= s2n;
#pragma unroll
  for (int c = 0; c < 16; ++c)
    if (c == t) a[c] += lam;
#pragma unroll
  for (int c = 16; c < 32; ++c)
    if (c == tb) b[c] += lam;
  double yt = P[PL::v + sd * Ds + t], yb = P[PL::v + sd * Ds + tb], dit = 0.0, dib = 0.0;
  double* __restrict__ P0 = &Pv[0][sys * PST];
  double* __restrict__ P1 = &Pv[1][sys * PST];
  P0[t] = a[0];
  P0[tb] = b[0];
  if (t == 0) P0[32] = yt;
  rows_steps<0>(a, b, yt, yb, dit, dib, t, P0, P1);
  const double zt = yt * dit, zb = yb * dib;
  double xt = 0.0, xb = 0.0;
  rows_back<31>(a, b, zt, zb, xt, xb, t);
  // ---- record + x_out; sums over the query's 2 systems ----
  // (loaded here, not held across the factorization)
  const double rh = P[PL::rhat], cdup = P[PL::cdup];
  const double gt = P[PL::v + sd * Ds + t], gbv = P[PL::v + sd * Ds + tb];
  // theta at the lane's two coordinates: side 0 [Pm_u | Pg_u], side 1 [Qm_i | Qg_i]
  const double tht = (double)A.t[sd][(int64_t)ent * K + t];
  const double thb = (double)A.t[2 + sd][(int64_t)ent * K + (tb - K)];
  const double w3b = (double)A.t[8][H2 + (tb - K)];
  double cq = fma(xt, tht, xb * thb);
  double xv = fma(xt, gt, xb * gbv);
  cq = sys_sum<16>(cq);
  xv = sys_sum<16>(xv);
  const int64_t n = (int64_t)nd;
  if (qok && n > 0 && !(cdup > 0.0)) {
    double* __restrict__ R = rec + q * M::R;
    double* __restrict__ S = L::side(R, sd);
    if (sd == 0 && t == 0) {
      R[L::inv_n] = 1.0 / nd;
      R[L::c_q] = cq * A.wd;
      R[L::x_v] = xv;
      R[L::rhat] = rh;
    }
    S[L::x_mlp + t] = xt;
    S[L::w3g_x_gmf + (tb - K)] = w3b * xb;
    if (t == 0) S[L::dup_other] = (double)(sd ? uu : ii);
    if (x_out) {
      x_out[q * D + M::ref_index(sd * Ds + t)] = xt;
      x_out[q * D + M::ref_index(sd * Ds + tb)] = xb;
    }
  } else if (qok && n == 0) {
    if (x_out) {
      x_out[q * D + sd * Ds + t] = NAN;
      x_out[q * D + sd * Ds + tb] = NAN;
    }
    if (sd == 0 && t == 0) rec[q * M::R + M::Rec::inv_n] = NAN;
  } else if (qok && sd == 0 && t == 0) {
    coupled_append(coupled_out, q);
  }
}

// ------------------------------------------------------------------------------------
// MF, k = 16 (the headline): a quad of lanes per side system, 16 systems (8 queries) per wave.
// Lane j of a quad owns rows j, j + 4, j + 8, j + 12 of the block's embedding coordinates
// (slot s = row 4 s + j: a[s][c] = H[r][c] for c <= r), their bias-row entries hb[s] =
// H[16][r] and right-hand sides y[s] = v_r; the bias pivot H[16][16] (and y_16) is kept by
// every lane of the quad and eliminated last.  Right-looking LDL^T: step J broadcasts the
// pivot column inside the quad by DPP quad_perm (no LDS), every lane updates its rows; the
// back solve sums each row's terms by two quad DPP steps.  A thread per system (k_solve_tps,
// k = 8) held the whole 17 x 17 block in one lane: at k = 16 that was 256 VGPRs with AGPR
// spills, 378 waves for 12 k queries (one per SIMD), every dependent step exposed.
// ------------------------------------------------------------------------------------
// every lane of the quad gets lane L's value (DPP quad_perm [L, L, L, L])
template <int L>
__device__ __forceinline__ double quad_bcast(double x) {
  return dpp_d<(L | (L << 2) | (L << 4) | (L << 6))>(x);
}
__device__ __forceinline__ double quad_sum(double x) {
  x += dpp_d<0xB1>(x);      // quad_perm [1, 0, 3, 2]
  x += dpp_d<0x4E>(x);      // quad_perm [2, 3, 0, 1]
  return x;
}

struct Quad16 {
  double a[4][16];          // slot s: row 4 s + j, columns 0 .. 4 s + 3 (past the row: unused)
  double hb[4], y[4], dinv[4], lbt[4], x[4];
  double hbb, y16;
};

// column J entries H[c][J], c = C .. 15, from lane c % 4 (slot c / 4), before step J scales them
template <int J, int C>
__device__ __forceinline__ void quad_col(const Quad16& Z, double (&hc)[16]) {
  if constexpr (C < 16) {
    hc[C] = quad_bcast<C % 4>(Z.a[C / 4][J]);
    quad_col<J, C + 1>(Z, hc);
  }
}

template <int J, int S>
__device__ __forceinline__ void quad_rows(Quad16& Z, const double (&hc)[16], double ij, double lb, double yj, int j) {
  if constexpr (S < 4) {
    // slot S holds row r = 4 S + j: below the pivot for S > J / 4, for S == J / 4 iff j > J % 4
    const bool below = S > J / 4 || (S == J / 4 && j > J % 4);
    const double l = below ? Z.a[S][J] * ij : 0.0;          // L[r][J]
#pragma unroll
    for (int c = J + 1; c < 4 * S + 4; ++c) Z.a[S][c] = fma(-l, hc[c], Z.a[S][c]);
    Z.hb[S] = below ? fma(-lb, Z.a[S][J], Z.hb[S]) : Z.hb[S];   // H[16][r] -= L[16][J] H[r][J]
    Z.y[S] = fma(-l, yj, Z.y[S]);
    if (below) Z.a[S][J] = l;
    quad_rows<J, S + 1>(Z, hc, ij, lb, yj, j);
  }
}

template <int J>
__device__ __forceinline__ void quad_steps(Quad16& Z, int j) {
  if constexpr (J < 16) {
    constexpr int SJ = J / 4, JJ = J % 4;
    const double dj = quad_bcast<JJ>(Z.a[SJ][J]);
    const double ij = rcp_nr2(dj);
    const double yj = quad_bcast<JJ>(Z.y[SJ]), hj = quad_bcast<JJ>(Z.hb[SJ]);
    const double lb = hj * ij;                              // L[16][J]
    double hc[16];
    quad_col<J, J + 1>(Z, hc);
    quad_rows<J, SJ>(Z, hc, ij, lb, yj, j);
    Z.hbb = fma(-lb, hj, Z.hbb);
    Z.y16 = fma(-lb, yj, Z.y16);
    if (j == JJ) {
      Z.dinv[SJ] = ij;
      Z.lbt[SJ] = lb;
    }
    quad_steps<J + 1>(Z, j);
  }
}

// L^T x = z from row 15 down: x_r = z_r - sum_{c > r} L[c][r] x_c - L[16][r] x_16
template <int R>
__device__ __forceinline__ void quad_back(Quad16& Z, const double (&z)[4], double x16, int j) {
  if constexpr (R >= 0) {
    constexpr int SR = R / 4, JR = R % 4;
    double p = 0.0;
#pragma unroll
    for (int s = SR; s < 4; ++s) {
      const bool below = s > SR || j > JR;                 // row 4 s + j > R
      p = below ? fma(Z.a[s][R], Z.x[s], p) : p;
    }
    p = quad_sum(p);
    if (j == JR) Z.x[SR] = z[SR] - p - Z.lbt[SR] * x16;
    quad_back<R - 1>(Z, z, x16, j);
  }
}

// one wave: the 8 queries [8 wv, 8 wv + 8) -- no LDS, no barrier, nothing read that another wave
// of the launch writes
template <class M>
__device__ __forceinline__ void solve_quad_wave(const QueryArgs& A, int64_t Q, double* __restrict__ rec,
                                                double* __restrict__ x_out, int64_t wv) {
  static_assert(!M::ncf && M::K == 16, "MF k = 16");
  constexpr int K = M::K, Ds = M::Ds, D = M::D, GS = Ds * (Ds + 1) / 2, GSP = (GS + 1) & ~1;
  const int lane = threadIdx.x & 63, qd = lane >> 2, j = lane & 3, h = qd >> 1, sd = qd & 1;
  const int64_t q = wv * 8 + h;
  const bool active = q < Q;
  const int64_t qc = active ? q : Q - 1;
  int32_t u = A.qu[qc], i = A.qi[qc];
  const bool okid = u >= 0 && u < A.U && i >= 0 && i < A.I;
  if (!okid) u = i = 0;
  const int32_t ent = sd ? i : u, oth = sd ? u : i;
  // the block's loads first (rows 4 s + j of the packed triangle, their bias-row entries, the
  // bias diagonal, the rhs), then the list lengths and the pair probe
  const double* __restrict__ G = A.gram[sd] + (int64_t)ent * GSP;
  const float* __restrict__ Eo = A.t[sd ? 0 : 1] + (int64_t)oth * K;
  Quad16 Z;
  double vv[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int r = 4 * s + j;
    const double* __restrict__ Gr = G + (r * (r + 1)) / 2;
#pragma unroll
    for (int c = 0; c < 4 * s + 4; ++c) Z.a[s][c] = Gr[c <= r ? c : r];
    Z.hb[s] = G[tri(K, r)];
    vv[s] = (double)Eo[r];
  }
  Z.hbb = G[tri(K, K)];
  const int64_t n = okid ? (A.ptr[0][u + 1] - A.ptr[0][u]) + (A.ptr[1][i + 1] - A.ptr[1][i]) : 0;
  double cdup = 0.0, rsum = 0.0;
  if (n > 0) A.pairs.lookup((unsigned long long)u * (unsigned long long)A.I + (unsigned long long)i, cdup, rsum);
  // H block = (2/n) Gram + wd on the embedding coordinates + damping
  const double s2n = n > 0 ? 2.0 / (double)n : 0.0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int r = 4 * s + j;
#pragma unroll
    for (int c = 0; c < 4 * s + 4; ++c) Z.a[s][c] = c <= r ? fma(Z.a[s][c], s2n, c == r ? A.wd + A.damping : 0.0) : 0.0;
    Z.hb[s] *= s2n;
    Z.y[s] = vv[s];
    Z.dinv[s] = Z.lbt[s] = Z.x[s] = 0.0;
  }
  Z.hbb = fma(Z.hbb, s2n, A.damping);
  Z.y16 = 1.0;
  quad_steps<0>(Z, j);
  const double i16 = rcp_nr2(Z.hbb);
  const double x16 = Z.y16 * i16;
  double z[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) z[s] = Z.y[s] * Z.dinv[s];
  quad_back<15>(Z, z, x16, j);
  // record pieces: theta block, x.v, wd x.theta, r-hat(u,i) (sums over the query's two systems:
  // the quad, then the neighbouring quad)
  const float* __restrict__ Es = A.t[sd] + (int64_t)ent * K;
  double th[4], cq = 0.0, xg = j == 0 ? x16 : 0.0, pv = 0.0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    th[s] = (double)Es[4 * s + j];
    cq = fma(Z.x[s], th[s], cq);
    xg = fma(Z.x[s], vv[s], xg);
    pv = fma(th[s], vv[s], pv);
  }
  cq = quad_sum(cq);
  xg = quad_sum(xg);
  pv = quad_sum(pv);
  cq = (cq + __shfl_xor(cq, 4)) * A.wd;
  xg += __shfl_xor(xg, 4);
  const double bself = (double)A.t[2 + sd][ent];
  const double gb = (double)A.t[4][0];
  const double bpair = bself + __shfl_xor(bself, 4);
  if (!active) return;
  if (n == 0) {
    if (x_out) {
#pragma unroll
      for (int s = 0; s < 4; ++s) x_out[q * D + M::ref_index(sd * Ds + 4 * s + j)] = NAN;
      if (j == 0) x_out[q * D + M::ref_index(sd * Ds + K)] = NAN;
    }
    if (sd == 0 && j == 0) rec[q * M::R + M::Rec::inv_n] = NAN;
    return;
  }
  if (cdup > 0.0) return;         // the test pair is a train row: the coupled role's (full D)
  double* __restrict__ R = rec + q * M::R;
  using L = typename M::Rec;
  if (sd == 0 && j == 0) {
    R[L::inv_n] = 1.0 / (double)n;
    R[L::c_q] = cq;
    R[L::x_v] = xg;
    R[L::rhat] = pv + bpair + gb;
  }
  double* __restrict__ S = L::side(R, sd);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    S[L::theta + 4 * s + j] = th[s];
    S[L::x + 4 * s + j] = Z.x[s];
  }
  if (j == 0) {
    S[L::bias] = bself + gb;
    S[L::x_bias] = x16;
    S[L::dup_other] = (double)oth;
  }
  if (x_out) {
#pragma unroll
    for (int s = 0; s < 4; ++s) x_out[q * D + M::ref_index(sd * Ds + 4 * s + j)] = Z.x[s];
    if (j == 0) x_out[q * D + M::ref_index(sd * Ds + K)] = x16;
  }
}

// The chunk scan and the side-system solves of one batch in one launch: neither reads what the
// other writes, both are latency-bound and each alone leaves most of the chip empty (ml-1m-ex:
// 24 scan tiles; ~1.5 solve waves per SIMD), so one after the other they cost the sum of two
// latency chains.  Workgroups [0, scan_tiles(Q)) run one tile of k_query_scan<1>'s body each,
// the others eight waves of the quad solve (8 queries per wave, 64 per workgroup).  The register
// budget is the larger role's: the solve's, two waves per SIMD, so a 512-thread workgroup is
// one CU's worth and the static LDS is the scan's.
// No workgroup waits on a workgroup that may not be running: a solve-role workgroup waits on
// nothing any other workgroup writes; a scan-role workgroup waits only on the tile words of
// EARLIER tickets, and a ticket is drawn by a workgroup that has already started -- so whatever
// order the dispatcher starts the roles in, every awaited workgroup is resident and runs to its
// publish without waiting on a later one.
// The last coupled_groups(Q) workgroups are the COUPLED role: the queries whose test pair is a
// train row (the solve role leaves them unwritten).  Workgroup w of the role tests queries
// w, w + groups, ... (kScanThreads at a time, the probe the solve role makes), compacts the hits
// in LDS and solves them full-D, one wave per query on kCplWaves waves (solve_full_wave, the
// body of k_solve), on slabs laid over the scan role's static LDS object -- the launch's LDS
// stays the scan's.  It reads the Gram caches, the parameters and the pair table and writes
// records and x_out rows no other role writes: it waits on no other workgroup either.  So the
// fused path has no `coupled` list and no k_solve launch (usually a role that finds nothing:
// that launch cost 5 us between the solve and the scoring kernel to draw a count of zero), and
// the list's {readers, count} words stay zero for the paths that keep it.
constexpr int kCplWaves = 4, kCplGroups = 32;
inline int64_t coupled_groups(int64_t Q) {
  const int64_t g = (Q + kCplWaves - 1) / kCplWaves;
  return g < kCplGroups ? g : kCplGroups;
}
template <class M>
struct CoupledLds {
  double slab[kCplWaves][kFullSlab<M>];
  NCFWeights<M::ncf ? M::K : 2> w;       // (MF: never read)
  double sW1[1], sb1[1];
  int32_t hits[kScanThreads];
  int32_t nhit;
};
template <class M>
__device__ __forceinline__ void coupled_role(const QueryArgs& A, int64_t Q, double* __restrict__ rec,
                                             double* __restrict__ x_out, int64_t wg, int64_t nwg) {
  static_assert(!M::ncf, "MF: no weights staged");
  static_assert(sizeof(CoupledLds<M>) <= sizeof(ScanFillLds) && alignof(CoupledLds<M>) <= alignof(ScanFillLds),
                "the coupled role's LDS lies inside the scan role's");
  CoupledLds<M>* const L = reinterpret_cast<CoupledLds<M>*>(scan_fill_lds<1>());
  const int wave = threadIdx.x >> 6;
  // (the trip count is the workgroup's: every thread reaches every barrier)
  for (int64_t first = wg; first < Q; first += (int64_t)kScanThreads * nwg) {
    if (threadIdx.x == 0) L->nhit = 0;
    __syncthreads();
    const int64_t q = first + (int64_t)threadIdx.x * nwg;
    if (q < Q) {
      const int32_t u = A.qu[q], i = A.qi[q];
      if (related_count(A, u, i) > 0) {
        double cdup = 0.0, rsum = 0.0;
        A.pairs.lookup((unsigned long long)u * (unsigned long long)A.I + (unsigned long long)i, cdup, rsum);
        if (cdup > 0.0) L->hits[atomicAdd(&L->nhit, 1)] = (int32_t)threadIdx.x;
      }
    }
    __syncthreads();
    const int nh = L->nhit;
    if (wave < kCplWaves)
      for (int h = wave; h < nh; h += kCplWaves)
        solve_full_wave<M>(A, first + (int64_t)L->hits[h] * nwg, rec, x_out, L->slab[wave], L->w, L->sW1, L->sb1);
    __syncthreads();
  }
}

template <class M>
__global__ __launch_bounds__(kScanThreads) void k_solve_quad(ScanArgs S, QueryArgs A, double* __restrict__ rec,
                                                             double* __restrict__ x_out) {
  const unsigned ntiles = (unsigned)((S.Q + 1 + kScanTile - 1) / kScanTile);
  if (blockIdx.x < ntiles) {
    query_scan_body<1>(S);
    return;
  }
  const unsigned nsolve = (unsigned)((S.Q + 63) / 64);
  if (blockIdx.x - ntiles >= nsolve) {
    coupled_role<M>(A, S.Q, rec, x_out, (int64_t)(blockIdx.x - ntiles - nsolve),
                    (int64_t)(gridDim.x - ntiles - nsolve));
    return;
  }
  solve_quad_wave<M>(A, S.Q, rec, x_out,
                     (int64_t)(blockIdx.x - ntiles) * (kScanThreads / 64) + (threadIdx.x >> 6));
}

// ------------------------------------------------------------------------------------
// MF, k <= 16: thread-per-system solve.  Every lane owns one (query, side) block of
// H_t (user block for even lanes, item block for odd lanes) and factors it with
// LDL^T entirely in registers (153 doubles at k=16, fully unrolled), then solves.  A
// query whose test pair is a train row couples the blocks: it is appended to the
// `coupled` list and solved afterwards by k_solve (one wave, full D).
// ------------------------------------------------------------------------------------
template <class M>
__global__ __launch_bounds__(64) void k_solve_tps(QueryArgs A, int64_t Q, double* __restrict__ rec,
                                                  double* __restrict__ x_out, int32_t* __restrict__ coupled) {
  static_assert(!M::ncf, "thread-per-system solve is the MF path");
  constexpr int K = M::K, Ds = M::Ds, D = M::D, GS = Ds * (Ds + 1) / 2, GSP = (GS + 1) & ~1;
  const int lane = threadIdx.x;
  const int64_t sys = (int64_t)blockIdx.x * 64 + lane;
  const int64_t q = sys >> 1;
  const int side = (int)(sys & 1);
  const bool active = q < Q;
  int32_t u = 0, i = 0;
  int64_t n = 0;
  if (active) {
    u = A.qu[q];
    i = A.qi[q];
    if (u >= 0 && u < A.U && i >= 0 && i < A.I)
      n = (A.ptr[0][u + 1] - A.ptr[0][u]) + (A.ptr[1][i + 1] - A.ptr[1][i]);
    else
      u = i = 0;
  }
  const int32_t ent = side == 0 ? u : i;       // this block's entity
  const int32_t oth = side == 0 ? i : u;       // the other endpoint of the test pair
  const float* Eself = side == 0 ? A.t[0] : A.t[1];
  const float* Eoth = side == 0 ? A.t[1] : A.t[0];
  const float* Bself = side == 0 ? A.t[2] : A.t[3];
  // the cached block's loads go out first: they overlap the pair lookup's probe chain
  const double* G = A.gram[side] + (int64_t)ent * GSP;
  double h[GS];
#define HS(t) h[(t)]
#pragma unroll
  for (int t = 0; t < GS; ++t) HS(t) = G[t];
  double cdup = 0.0, rsum = 0.0;
  if (active && n > 0)
    A.pairs.lookup((unsigned long long)u * (unsigned long long)A.I + (unsigned long long)i, cdup, rsum);
  if (active && n > 0 && cdup > 0.0 && side == 0) coupled_append(coupled, q);
  if (active && n == 0) {
    if (x_out)
      for (int a = 0; a < Ds; ++a) x_out[q * D + M::ref_index(side * Ds + a)] = NAN;
    if (side == 0) rec[q * M::R + M::Rec::inv_n] = NAN;
  }
  const bool work = active && n > 0 && cdup == 0.0;

  // H block = (2/n) Gram + wd on the embedding coordinates + damping, in registers (fully
  // unrolled, every index constant)
  const double s2n = n > 0 ? 2.0 / (double)n : 0.0;
#pragma unroll
  for (int t = 0; t < GS; ++t) HS(t) *= s2n;
#pragma unroll
  for (int r = 0; r < Ds; ++r) HS(tri(r, r)) += (r < K ? A.wd : 0.0) + A.damping;

  // right-looking LDL^T: column j holds L[., j], the diagonal holds d
#pragma unroll
  // (the diagonal keeps 1/d, rcp_nr2, and the forward solve multiplies by it)
  for (int j = 0; j < Ds; ++j) {
    const double dj = HS(tri(j, j));
    const double inv = rcp_nr2(dj);
#pragma unroll
    for (int r = j + 1; r < Ds; ++r) {
      const double lr = HS(tri(r, j)) * inv;
#pragma unroll
      for (int c = j + 1; c <= r; ++c) HS(tri(r, c)) = fma(-lr, HS(tri(c, j)), HS(tri(r, c)));
    }
#pragma unroll
    for (int r = j + 1; r < Ds; ++r) HS(tri(r, j)) *= inv;
    HS(tri(j, j)) = inv;
  }
  // v block: user side [q_i ; 1], item side [p_u ; 1]  (gnn:155, mf:194)
  double x[Ds];
  load_row_f32<K>(Eoth + (int64_t)oth * K, x);
  x[K] = 1.0;
#pragma unroll
  for (int j = 0; j < Ds; ++j)
#pragma unroll
    for (int r = j + 1; r < Ds; ++r) x[r] = fma(-HS(tri(r, j)), x[j], x[r]);
#pragma unroll
  for (int j = 0; j < Ds; ++j) x[j] *= HS(tri(j, j));
#pragma unroll
  for (int j = Ds - 1; j >= 0; --j)
#pragma unroll
    for (int c = 0; c < j; ++c) x[c] = fma(-HS(tri(j, c)), x[j], x[c]);
#undef HS

  // record pieces: theta block, x.v, wd x.theta, r-hat(u,i)
  double th[K], vv[K];
  load_row_f32<K>(Eself + (int64_t)ent * K, th);
  load_row_f32<K>(Eoth + (int64_t)oth * K, vv);
  const double bself = (double)Bself[ent];
  const double gb = (double)A.t[4][0];
  double cq = 0.0, xg = x[K], pv = 0.0;
#pragma unroll
  for (int a = 0; a < K; ++a) {
    cq = fma(x[a], th[a], cq);
    xg = fma(x[a], vv[a], xg);
    pv = fma(th[a], vv[a], pv);
  }
  cq *= A.wd;
  cq += __shfl_xor(cq, 1);
  xg += __shfl_xor(xg, 1);
  const double bpair = bself + __shfl_xor(bself, 1);
  if (!work) return;
  double* R = rec + q * M::R;
  using L = typename M::Rec;
  if (side == 0) {
    R[L::inv_n] = 1.0 / (double)n;
    R[L::c_q] = cq;
    R[L::x_v] = xg;
    R[L::rhat] = pv + bpair + gb;
  }
  double* S = L::side(R, side);
#pragma unroll
  for (int a = 0; a < K; ++a) {
    S[L::theta + a] = th[a];
    S[L::x + a] = x[a];
  }
  S[L::bias] = bself + gb;
  S[L::x_bias] = x[K];
  S[L::dup_other] = (double)oth;
  if (x_out)
#pragma unroll
    for (int a = 0; a < Ds; ++a) x_out[q * D + M::ref_index(side * Ds + a)] = x[a];
}

}  // namespace

hipError_t launch_ncf_query_pro(int k, const QueryArgs& A, int64_t Q, double* qpro, hipStream_t s) {
  bool ok = false;
  dispatch_small(FIA_MODEL_NCF, k, [&](auto m) {
    using M = decltype(m);
    if constexpr (pair_layout<M>()) {
      hipLaunchKernelGGL(k_ncf_query_pro<M>, dim3((unsigned)((Q + 63) / 64)), dim3(256), 0, s, A, Q, qpro);
      ok = true;
    }
  });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_record_x(int model, int k, const QueryArgs& A, int64_t Q, const double* x_in, double* rec,
                           double* x_out, hipStream_t s) {
  const bool ok = dispatch_small(model, k, [&](auto m) {
    const int64_t g1 = Q < 8192 ? Q : 8192;
    hipLaunchKernelGGL(k_record_x<decltype(m)>, dim3((unsigned)g1), dim3(kSolveThreads), 0, s, A, Q, x_in, rec, x_out);
  });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

// The side-system solve of the model: non-coupled queries thread-per-system (MF k = 8), a quad
// per system (MF k = 16) or column-parallel blocks; each kernel's grid rule and cap are here.
hipError_t launch_side_solve(int model, int k, fia_ctx* c, const ScanArgs& S, const QueryArgs& A, int64_t Q,
                             double* x_out, int32_t* coupled, hipStream_t s, PhaseSpan ps) {
  double* const rec = c->rec.as<double>();
  const int64_t cus = c->num_cus > 0 ? c->num_cus : 256;
  const bool ok = dispatch_small(model, k, [&](auto m) {
    using M = decltype(m);
    if constexpr (use_quad_solve<M>()) {
      // scan_tiles(Q) scan workgroups, then 64 queries per solve workgroup, then the coupled
      // role's; the solve phase is this one dispatch, which stamps both of its events
      hipExtLaunchKernelGGL(k_solve_quad<M>, dim3((unsigned)(scan_tiles(Q) + (Q + 63) / 64 + coupled_groups(Q))),
                            dim3(kScanThreads), 0, s, ps.a, ps.b, 0, S, A, rec, x_out);
    } else if constexpr (use_tps<M>()) {
      hipLaunchKernelGGL(k_solve_tps<M>, dim3((unsigned)((2 * Q + 63) / 64)), dim3(64), 0, s, A, Q, rec, x_out,
                         coupled);
    } else if constexpr (pair_layout<M>()) {
      hipLaunchKernelGGL(k_solve_rows<M>, dim3((unsigned)((Q + 1) / 2)), dim3(64), 0, s, A, Q,
                         (const double*)c->qwork.as<double>(), rec, x_out, coupled);
    } else if constexpr (use_col_solve<M>()) {
      const int64_t cap = cus * 16;
      constexpr int QW = 32 / M::K;             // queries per wave
      const int64_t need = (Q + QW - 1) / QW;
      const int64_t g1 = need < cap ? need : cap;   // persistent: NCF weights staged once per block
      hipLaunchKernelGGL(k_solve_col<M>, dim3((unsigned)g1), dim3(64), 0, s, A, Q, rec, x_out, coupled);
    } else {
      static_assert(use_tile_solve<M>(), "every small-k model has a side-system solve");
      const int64_t cap = cus * 8;
      const int64_t g1 = Q < cap ? Q : cap;     // persistent: NCF weights staged once per block
      hipLaunchKernelGGL(k_solve_tile<M>, dim3((unsigned)g1), dim3(128), 0, s, A, Q, rec, x_out, coupled);
    }
  });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

// The full-D solve of the queries the side solve listed in `coupled`; its dispatch stamps `end`
// (null: none).  Usually no coupled query: a small grid that exits (a full grid for the large
// full-D systems of k >= 32, should many test pairs be train rows).  MF k = 16 has no such
// launch: the coupled queries are a role of k_solve_quad, in workgroups of their own.  (Folding
// the full-D solve into the last workgroup of k_solve_tps -- an atomic finish count -- made that
// kernel 14 us slower at ml-1m-ex: its LDS and registers in EVERY workgroup, and a wait on all
// of them.  The role waits on nobody, its LDS lies inside the scan role's and the launch keeps
// the side solve's registers.)
hipError_t launch_coupled_solve(int model, int k, const QueryArgs& A, int64_t Q, double* rec, double* x_out,
                                int32_t* coupled, hipStream_t s, hipEvent_t end) {
  bool ok = false;
  dispatch_small(model, k, [&](auto m) {
    using M = decltype(m);
    if constexpr (!use_quad_solve<M>()) {
      const int64_t gc = M::K <= 16 ? 64 : 256;
      const int64_t g2 = Q < gc ? Q : gc;
      hipExtLaunchKernelGGL(k_solve<M>, dim3((unsigned)g2), dim3(kSolveThreads), 0, s, (hipEvent_t) nullptr, end, 0,
                            A, Q, rec, x_out, coupled);
      ok = true;
    }
  });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace fia
