// fia_pair_flip: the smallest set of a user's own ratings that, to first order, puts item j above
// item i, and what the re-solved system says that set does (include/fia.h).  Pair query q = (u, i, j)
// with n, theta_t, H, v, x = H^-1 v and diff of fia_pair_batch (pair.hip):
//
//   val_p  = x . (2 e_p g_p + wd M theta_t) / n for position p of R_u (fia_pair_batch's value there)
//   eligible: the item of p is neither i nor j and val_p < 0 (so not NaN)
//   S      = the eligible positions by (val ascending, position ascending), taken while fewer than
//            max_set are taken, one is left and diff + margin + (sum of the taken val) >= 0
//   H_S    = (1/n) sum_{z in S} (2 g_z g_z^T + wd diag(M))      b_S = (1/n) sum_{z in S} (2 e_z g_z + wd M theta_t)
//   dtheta = (H - H_S)^-1 b_S,  newton = v . dtheta,  first_order = sum of the taken val = x . b_S
//
// Kernels:
//   k_pair_solve (pair.hip, through pair_batch with no list output)  x, diff and the two half records
//   k_flip_select  the hot path: a workgroup per query (grid-stride) walks R_u in tiles of kCandTile
//                  positions, a position per thread scored as k_pair_score's user-list branch does
//                  (coop_dots; NCF stage_z1 + cand_core_ncf; the user block's term only), and keeps
//                  the max_set smallest eligible (val, position) in LDS: after each tile every one of
//                  the tile's 256 and the kept 64 entries counts the entries before it in that total
//                  order and, below max_set, stores itself at that rank.  Positions are unique, so
//                  the kept set is the order's first max_set whatever the tiling.  Then one lane
//                  runs the sequential stop rule and the workgroup writes the outputs.  C_i and C_j
//                  are never read.
//   k_flip_newton  persistent one-wave workgroups, a query each: the packed D3 triangle and v
//                  (pair_assemble, pair_gap_gradient), then per member in selection order the
//                  prologue of (u, b) for e and the user-block gradient, remove_member + the third
//                  block's decay share, member_rhs; one full-range ldlt_solve and the dot with v
// No floating-point atomics; every LDS entry is updated by one lane per member, so a query's bits
// depend on (u, i, j, margin, max_set) alone -- and the members on max_set only through the cut.
#include "pair.h"

namespace fia {
namespace {

constexpr int kFlipMax = FIA_FLIP_MAX_SET;
static_assert(kFlipMax <= kCandTile, "the kept entries are ranked by the tile's threads");

struct FlipArgs : ModelArgs {
  int64_t Q;
  const int32_t* qu;
  const int32_t* qi;
  const int32_t* qj;
  const int32_t* row;       // the user-major lists (train row, item, rating)
  const int32_t* other;
  const float* rating;
  const double* rec;        // [Q * 2 * pair_half] (k_pair_solve)
  const double* diff;       // [Q] (k_pair_solve)
  const double* margin;     // [Q] or null: 0
  int max_set;
  int32_t* size;            // [Q] the caller's array or scratch
  int64_t* entry;           // [Q * max_set] scratch: a member's entry of the user-major lists, -1 unused
  int32_t* set_row;         // [Q * max_set] or null
  double* set_val;          // [Q * max_set] or null
  double* first;            // [Q] or null
};

template <class M>
__global__ __launch_bounds__(kCandTile) void k_flip_select(FlipArgs A) {
  constexpr int KK = M::K, HS = pair_half<M>(), NC = kCandTile + kFlipMax;
  __shared__ NCFWeights<(M::ncf ? KK : 2)> w;
  __shared__ double z1s[M::ncf ? KK * kCandZ1Stride : 1];
  __shared__ double c_val[NC];        // the tile's values, then the kept ones by rank; +inf: none
  __shared__ int32_t c_pos[NC];       // their positions in R_u
  __shared__ int s_size;
  if constexpr (M::ncf) load_ncf_weights<KK>(w, A.t[6], A.t[7], A.t[8]);
  const int tid = threadIdx.x;
  const int ms = A.max_set;           // in [1, kFlipMax] (checked by the caller)
  for (int64_t q = blockIdx.x; q < A.Q; q += gridDim.x) {
    __syncthreads();
    const int32_t u = A.qu[q], i = A.qi[q], j = A.qj[q];
    int32_t* __restrict__ srow = A.set_row ? A.set_row + q * ms : nullptr;
    double* __restrict__ sval = A.set_val ? A.set_val + q * ms : nullptr;
    int64_t* __restrict__ sent = A.entry + q * ms;
    // an id out of range is never used as an index; it, i == j and n == 0: no set
    int64_t ub = 0, du = 0, n = 0;
    if (pair_ids_ok(u, i, j, A.U, A.I) && i != j) {
      ub = A.ptr[0][u];
      du = A.ptr[0][u + 1] - ub;
      n = du + (A.ptr[1][i + 1] - A.ptr[1][i]) + (A.ptr[1][j + 1] - A.ptr[1][j]);
    }
    if (n == 0) {
      for (int t = tid; t < ms; t += kCandTile) {
        if (srow) srow[t] = -1;
        if (sval) sval[t] = NAN;
        sent[t] = -1;
      }
      if (tid == 0) {
        A.size[q] = -1;
        if (A.first) A.first[q] = NAN;
      }
      continue;
    }
    if (tid < kFlipMax) {
      c_val[kCandTile + tid] = INFINITY;
      c_pos[kCandTile + tid] = -1;
    }
    const double base = A.diff[q] + (A.margin ? A.margin[q] : 0.0);
    const double* __restrict__ R0 = A.rec + (2 * q) * HS;
    const int h0 = (int)(2 * q);
    // (j is below i already, or a NaN margin: nothing is taken, so nothing is scored)
    for (int64_t p0 = 0; p0 < du && base >= 0.0; p0 += kCandTile) {
      const int64_t p = p0 + tid;
      int32_t b = 0;
      float y = 0.f;
      bool valid = false;
      if (p < du) {
        b = A.other[ub + p];
        y = A.rating[ub + p];
        valid = b != i && b != j;       // an own-pair row is not the user's to remove here
      }
      // (whole waves from here: the row gathers are cooperative)
      double val = NAN;
      if constexpr (M::ncf) {
        using L = CandRecNCF<KK>;
        stage_z1<KK>(A, valid, u, b, z1s);
        __syncthreads();
        double rg, sgu, sgi;
        coop_dots<KK, true, HS, L::w3g_x_pg, L::w3g_x_qg, true>(valid, u, b, h0, true, false, A.t[2], A.t[3], A.rec,
                                                                A.t[8] + KK / 2, rg, sgu, sgi, h0);
        if (valid) {
          double r, s;
          cand_core_ncf<KK>(A, w, u, b, true, false, R0 + L::y_user, R0 + L::y_item, z1s + tid, r, s);
          s += sgu + sgi;
          r += rg + (double)A.t[9][0];
          val = R0[L::c_q] + 2.0 * (r - (double)y) * s * R0[L::inv_n];
        }
      } else {
        using L = PairRecMF<KK>;
        double r, su, si;
        coop_dots<KK, false, HS, L::x_user, L::x_item, true>(valid, u, b, h0, true, false, A.t[0], A.t[1], A.rec,
                                                             nullptr, r, su, si, h0);
        if (valid) {
          r += (double)A.t[2][u] + (double)A.t[3][b] + (double)A.t[4][0];
          su += R0[L::x_bias_user];
          val = R0[L::c_q] + 2.0 * (r - (double)y) * (su + si) * R0[L::inv_n];
        }
      }
      c_val[tid] = valid && val < 0.0 ? val : INFINITY;
      c_pos[tid] = (int32_t)p;          // (a list is shorter than 2^31: train rows are int32)
      __syncthreads();
      // the rank of every finite entry among the tile's and the kept ones
      double mv[2];
      int32_t mp[2];
      int rk[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int e = tid + h * kCandTile;
        mv[h] = e < NC ? c_val[e] : INFINITY;
        mp[h] = e < NC ? c_pos[e] : -1;
        rk[h] = 0;
        if (mv[h] < INFINITY) {
          for (int x = 0; x < NC; ++x) {
            const double xv = c_val[x];
            rk[h] += (xv < mv[h] || (xv == mv[h] && c_pos[x] < mp[h])) ? 1 : 0;
          }
        }
      }
      __syncthreads();
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (mv[h] < INFINITY && rk[h] < ms) {
          c_val[kCandTile + rk[h]] = mv[h];
          c_pos[kCandTile + rk[h]] = mp[h];
        }
      }
      __syncthreads();
    }
    __syncthreads();
    if (tid == 0) {
      // the stop rule, sequential in selection order
      double sum = 0.0;
      int t = 0;
      while (t < ms && c_val[kCandTile + t] < INFINITY && base + sum >= 0.0) {
        sum += c_val[kCandTile + t];
        ++t;
      }
      s_size = t;
      A.size[q] = t;
      if (A.first) A.first[q] = sum;
    }
    __syncthreads();
    const int taken = s_size;
    for (int t = tid; t < ms; t += kCandTile) {
      const bool in = t < taken;
      const int64_t e = in ? ub + c_pos[kCandTile + t] : -1;
      if (srow) srow[t] = in ? A.row[e] : -1;
      if (sval) sval[t] = in ? c_val[kCandTile + t] : NAN;
      sent[t] = e;
    }
  }
}

// LDS of one k_flip_newton workgroup: k_pair_solve's and two more D3 vectors
template <class M>
constexpr int64_t flip_lds_bytes() {
  return pair_lds_bytes<M>() + 8 * 2 * 3 * M::Ds;
}

template <class M>
__global__ __launch_bounds__(kSolveThreads) void k_flip_newton(QueryArgs A, FlipArgs F, double* __restrict__ newton,
                                                               double* __restrict__ dtheta) {
  constexpr int K = M::K, Ds = M::Ds, D = M::D, D3 = 3 * Ds;
  __shared__ double H[D3 * (D3 + 1) / 2];
  __shared__ double gi[D], gj[D], thi[D], thj[D];     // v^i, v^j and theta of (u, i), (u, j); then a member's in gi / thi
  __shared__ double v[D3], dd[D3], ww[D3];
  __shared__ double bS[D3], th3[D3];                  // b_S, then dtheta; theta_t in block order
  __shared__ double sh[4 * K + 8];
  __shared__ NCFWeights<M::ncf ? K : 2> w;
  __shared__ double sW1[M::ncf ? 2 * K * K : 1];
  __shared__ double sb1[M::ncf ? K : 1];
  stage_ncf<M>(A, w, sW1, sb1);
  const int lane = threadIdx.x;
  const int ms = F.max_set;
  for (int64_t q = blockIdx.x; q < F.Q; q += gridDim.x) {
    __syncthreads();
    const int32_t sz = F.size[q];
    double* __restrict__ dth = dtheta ? dtheta + q * D3 : nullptr;
    const int32_t u = F.qu[q], i = F.qi[q], j = F.qj[q];
    if (sz <= 0 || !pair_ids_ok(u, i, j, A.U, A.I) || i == j) {
      // NaN: no set (a bad id, i == j, n == 0); +0.0: an empty set, without a solve
      const double fill = sz == 0 ? 0.0 : NAN;
      if (dth)
        for (int a = lane; a < D3; a += kSolveThreads) dth[a] = fill;
      if (lane == 0 && newton) newton[q] = fill;
      continue;
    }
    const int64_t ub = A.ptr[0][u], du = A.ptr[0][u + 1] - ub;
    const int64_t n = du + (A.ptr[1][i + 1] - A.ptr[1][i]) + (A.ptr[1][j + 1] - A.ptr[1][j]);
    const double rhat_i = solve_prologue<M, kSolveThreads>(A, u, i, thi, gi, sh, w, sW1, sb1);
    const double rhat_j = solve_prologue<M, kSolveThreads>(A, u, j, thj, gj, sh, w, sW1, sb1);
    pair_assemble<M>(A, u, i, j, n, rhat_i, rhat_j, gi, gj, w, H, lane);
    pair_gap_gradient<M>(gi, gj, v, lane);
    for (int a = lane; a < Ds; a += kSolveThreads) {
      th3[a] = thi[a];
      th3[Ds + a] = thi[Ds + a];
      th3[2 * Ds + a] = thj[Ds + a];
    }
    for (int a = lane; a < D3; a += kSolveThreads) bS[a] = 0.0;
    __syncthreads();
    const double inv_n = 1.0 / (double)n;
    const int members = sz < ms ? sz : ms;
    // ---- the members in selection order (every value below is the same in all lanes) ----
    for (int t = 0; t < members; ++t) {
      const int64_t e_at = F.entry[q * ms + t];
      if (e_at < ub || e_at >= ub + du) continue;       // (k_flip_select's: never outside the user's list)
      const int32_t b = A.other[0][e_at];
      const float yf = A.rating[0][e_at];
      __syncthreads();                                  // the previous member's reads of gi
      const double e = solve_prologue<M, kSolveThreads>(A, u, b, thi, gi, sh, w, sW1, sb1) - (double)yf;
      // g_z: b is neither i nor j, so the user block only
      for (int c = lane; c < Ds; c += kSolveThreads) gi[Ds + c] = 0.0;
      __syncthreads();
      // H -= (2/n) g_z g_z^T on the user block and (wd/n) diag(M) on all three blocks
      remove_member<M>(H, gi, e, inv_n, 0, Ds, false, w, A.wd);
      for (int c = lane; c < Ds; c += kSolveThreads)
        if (M::decayed(c)) H[tri(D + c, D + c)] -= inv_n * A.wd;
      for (int c = lane; c < D; c += kSolveThreads) bS[c] += member_rhs<M>(c, gi, th3, e, inv_n, A.wd);
      for (int c = lane; c < Ds; c += kSolveThreads)
        if (M::decayed(c)) bS[D + c] += inv_n * (A.wd * th3[D + c]);
    }
    __syncthreads();
    ldlt_solve<D3>(H, bS, dd, ww, 0, D3);
    __syncthreads();
    double part = 0.0;
    for (int a = lane; a < D3; a += kSolveThreads) {
      part += v[a] * bS[a];
      if (dth) dth[pair_ref_index<M>(a)] = bS[a];
    }
    part = wave_sum(part);
    if (lane == 0 && newton) newton[q] = part;
  }
}

template <class M>
hipError_t flip_impl(fia_ctx* c, const QueryArgs& QA, FlipArgs F, double* newton, double* dtheta, hipStream_t s) {
  if constexpr (pair_built<M>()) {
    const int64_t Q = F.Q;
    const int64_t cus = c->num_cus > 0 ? c->num_cus : 256;
    phase_begin(c, 2, s);
    // persistent workgroups (NCF weights staged once each), grid-stride over the queries
    const int64_t sel_cap = cus * 8;
    hipLaunchKernelGGL(k_flip_select<M>, dim3((unsigned)(Q < sel_cap ? Q : sel_cap)), dim3(kCandTile), 0, s, F);
    FIA_HIP_TRY(hipGetLastError());
    phase_end(c, 2, s);
    if (newton || dtheta) {
      phase_begin(c, 3, s);
      const int64_t cap = solve_grid_cap(c, flip_lds_bytes<M>());
      hipLaunchKernelGGL(k_flip_newton<M>, dim3((unsigned)(Q < cap ? Q : cap)), dim3(kSolveThreads), 0, s, QA, F,
                         newton, dtheta);
      FIA_HIP_TRY(hipGetLastError());
      phase_end(c, 3, s);
    }
    return hipSuccess;
  } else {
    return hipErrorInvalidValue;            // (pair_supported is checked by the caller)
  }
}

}  // namespace

hipError_t pair_flip(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int32_t* qj,
                     const double* margin, int max_set, int32_t* set_size, int32_t* set_row, double* set_val,
                     double* first_order, double* newton, double* dtheta, double* diff, hipStream_t s) {
  const bool select = set_size || set_row || set_val || first_order || newton || dtheta;
  // context scratch: the gap when the caller does not take it, the members' list entries, the sizes
  // when the caller does not take them
  const size_t n_entry = select ? (size_t)Q * (size_t)max_set : 0;
  const size_t need = sizeof(double) * (size_t)Q + sizeof(int64_t) * n_entry + sizeof(int32_t) * (size_t)Q;
  double* dgap = diff;
  if (select) {
    FIA_HIP_TRY(c->gxq.reserve(need, s));
    if (!dgap) dgap = c->gxq.as<double>();
  }
  // phase 1: k_pair_solve alone -- no list output, so no offsets and no tile bookkeeping -- leaves the
  // two half records per query in c->rec
  FIA_HIP_TRY(pair_batch(c, Q, qu, qi, qj, nullptr, 0, nullptr, nullptr, nullptr, dgap, 0, nullptr, nullptr, nullptr, s));
  if (!select) return hipSuccess;
  FlipArgs F{};
  fill_model_args(c, F);
  F.Q = Q;
  F.qu = qu;
  F.qi = qi;
  F.qj = qj;
  F.row = c->idx.side[0].row.as<int32_t>();
  F.other = c->idx.side[0].other.as<int32_t>();
  F.rating = c->idx.side[0].rating.as<float>();
  F.rec = c->rec.as<double>();
  F.diff = dgap;
  F.margin = margin;
  F.max_set = max_set;
  F.entry = reinterpret_cast<int64_t*>(c->gxq.as<double>() + Q);
  F.size = set_size ? set_size : reinterpret_cast<int32_t*>(F.entry + n_entry);
  F.set_row = set_row;
  F.set_val = set_val;
  F.first = first_order;
  const QueryArgs QA = make_args(c, qu, qi);
  hipError_t e = hipErrorInvalidValue;
  dispatch_small(c->p.model, c->p.k, [&](auto m) { e = flip_impl<decltype(m)>(c, QA, F, newton, dtheta, s); });
  return e;
}

}  // namespace fia
