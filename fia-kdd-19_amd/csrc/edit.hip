// fia_edit_influence: the joint Newton effect on r-hat(u, i) of an EDIT SET -- train rows removed
// and hypothetical ratings added together (include/fia.h).  For query q = (u, i) with n related
// ratings, v, H and the member terms of fia_group_influence, a group's removals R (train rows) and
// additions A (triples c = (a, b, y), each counting once):
//
//   H_R = (1/n) sum_{j in R} m_j (2 g_j g_j^T + 2 e_j C_j + wd M)        b_R = (1/n) sum_{j in R} m_j (2 e_j g_j + wd M theta_t)
//   H_A = (1/n) sum_{c in A} (2 g_c g_c^T + 2 e_c C [both] + wd diag(M))  b_A = (1/n) sum_{c in A} (2 e_c g_c + wd M theta_t)
//   dtheta = (H - H_R + H_A)^-1 (b_R - b_A),  edit = v . dtheta,  first_order = (H^-1 v) . (b_R - b_A)
//
// Neither fia_group_influence's (H - H_R)^-1 b_R nor fia_score_candidates_newton's (H + H_c)^-1 b_c
// adds up to this: every edit set is a system of its own, downdated and updated on the packed
// triangle and solved once.
//
// Kernels (one wave per work item, persistent one-wave workgroups, as group.hip):
//   k_row_rec, k_group_x  group.hip's: the train-row table, and x_q = H^-1 v per query into context
//                  scratch when first_order is asked for
//   k_edit         per group: prologue of (u, i), H from the two Gram caches; then ONE loop over the
//                  members, the removals in list order with k_group's arithmetic and after them
//                  the additions in list order -- a member's (a, b, y) from the row table or from
//                  the addition arrays, prologue of (a, b) for e and g (the blocks of a side that
//                  does not match zeroed; no prologue at all for an addition sharing neither
//                  side), remove_member with the weight m_j / n or, an addition, -1 / n, the
//                  right-hand side += its gradient with the same weight -- one full-range
//                  ldlt_solve and the dot with v.  (Two loops, one per kind, cost NCF k = 16 15
//                  more VGPRs and 50 more spilled SGPRs than k_group: DESIGN.md 3i)
//   k_edit_topk + k_cand_merge  one wave per tile of 256 groups selects per (tile, query) segment;
//                  then the per-query merge of fia_score_candidates
// No floating-point atomics; every LDS entry is updated by one lane per member, members in list
// order (removals, then additions), so the bits depend on (query, the two lists) alone.
#include "cand.h"
#include "solve.h"

namespace fia {
namespace {

struct EditArgs {
  int64_t Q, G, TR, TA;
  const int64_t* grp_off;    // [Q + 1]
  const int64_t* rem_off;    // [G + 1]
  const int32_t* rem_row;    // [TR]
  const int64_t* add_off;    // [G + 1]
  const int32_t* add_u;      // [TA]
  const int32_t* add_i;
  const float* add_y;
  const int4* rowrec;        // [N] train row -> {user, item, rating bits, user-major list position}
  const double* xq;          // [Q * D] H^-1 v, block order (k_group_x); null: no first_order
  double* edit;              // [G] (the caller's array, or scratch for the top-K)
  double* first;             // [G]
  double* dtheta;            // [G * D], reference theta order
};

template <class M>
__global__ __launch_bounds__(kSolveThreads) void k_edit(QueryArgs A, EditArgs E) {
  constexpr int K = M::K, Ds = M::Ds, D = M::D;
  __shared__ double H[D * (D + 1) / 2];
  __shared__ double g[D], th[D], dd[D], ww[D];
  __shared__ double gj[D], thj[D], bS[D];
  __shared__ double sh[4 * K + 8];
  __shared__ NCFWeights<M::ncf ? K : 2> w;
  __shared__ double sW1[M::ncf ? 2 * K * K : 1];
  __shared__ double sb1[M::ncf ? K : 1];
  stage_ncf<M>(A, w, sW1, sb1);
  const int lane = threadIdx.x;
  for (int64_t gi = blockIdx.x; gi < E.G; gi += gridDim.x) {
    __syncthreads();
    // the group's query: the largest q in [0, Q) with grp_off[q] <= gi
    const int64_t q = last_at_most(E.grp_off, (int64_t)0, E.Q - 1, gi);
    const int32_t u = A.qu[q], i = A.qi[q];
    const int64_t n = related_count(A, u, i);
    int64_t r0 = E.rem_off[gi], r1 = E.rem_off[gi + 1];
    r0 = r0 < 0 ? 0 : r0;                             // (never past the member arrays)
    r1 = r1 > E.TR ? E.TR : r1;
    int64_t a0 = E.add_off[gi], a1 = E.add_off[gi + 1];
    a0 = a0 < 0 ? 0 : a0;
    a1 = a1 > E.TA ? E.TA : a1;
    const int64_t nr = r1 > r0 ? r1 - r0 : 0, na = a1 > a0 ? a1 - a0 : 0;
    bool bad = n == 0;
    int neff = 0;
    if (!bad) {
      const double rhat_ui = solve_prologue<M, kSolveThreads>(A, u, i, th, g, sh, w, sW1, sb1);
      assemble_hessian<M>(A, u, i, n, rhat_ui, g, H);
      for (int a = lane; a < D; a += kSolveThreads) bS[a] = 0.0;
      __syncthreads();
      const double inv_n = 1.0 / (double)n;
      // ---- the members in list order, the removals and then the additions (every value below is
      // the same in all lanes); one loop body for both kinds: an addition is a member of weight -1/n
      for (int64_t m = 0; m < nr + na; ++m) {
        const bool add = m >= nr;
        int32_t a, b;
        float yf;
        if (!add) {
          const int32_t row = E.rem_row[r0 + m];
          if (row < 0 || row >= A.N) {                // never used as an index
            bad = true;
            break;
          }
          const int4 rr = E.rowrec[row];
          a = rr.x;
          b = rr.y;
          yf = __int_as_float(rr.z);
        } else {
          a = E.add_u[a0 + (m - nr)];
          b = E.add_i[a0 + (m - nr)];
          yf = E.add_y[a0 + (m - nr)];
          if (!(a >= 0 && a < A.U && b >= 0 && b < A.I)) {   // never used as an index
            bad = true;
            break;
          }
        }
        const bool on_u = a == u, on_i = b == i;
        if (!on_u && !on_i && !add) continue;         // a removed row with m_j = 0: contributes nothing
        ++neff;                                       // (an addition sharing neither side: its decay share)
        __syncthreads();                              // the previous member's reads of gj
        double e = 0.0;
        if (on_u || on_i) e = solve_prologue<M, kSolveThreads>(A, a, b, thj, gj, sh, w, sW1, sb1) - (double)yf;
        // g_j: the blocks of a side that does not match are zero
        if (!on_u)
          for (int c = lane; c < Ds; c += kSolveThreads) gj[c] = 0.0;
        if (!on_i)
          for (int c = lane; c < Ds; c += kSolveThreads) gj[Ds + c] = 0.0;
        __syncthreads();
        // removal: m_j / n; addition: -1 / n, so H += (2/n) g_c g_c^T on the blocks where g_c is nonzero
        // (none: an empty range) + (2 e_c / n) C for the own pair + (wd/n) diag(M), and b -= b_c
        const double mn = add ? -inv_n : ((on_u ? 1.0 : 0.0) + (on_i ? 1.0 : 0.0)) * inv_n;
        remove_member<M>(H, gj, e, mn, on_u ? 0 : Ds, on_i ? D : Ds, on_u && on_i, w, A.wd);
        for (int c = lane; c < D; c += kSolveThreads) bS[c] += member_rhs<M>(c, gj, th, e, mn, A.wd);
      }
      __syncthreads();
    }
    double* __restrict__ dth = E.dtheta ? E.dtheta + gi * D : nullptr;
    if (bad || neff == 0) {
      // NaN: n_q = 0, a query id, a removed row or an added id out of range; +0.0: nothing edited
      const double fill = bad ? NAN : 0.0;
      if (dth)
        for (int a = lane; a < D; a += kSolveThreads) dth[a] = fill;
      if (lane == 0) {
        if (E.edit) E.edit[gi] = fill;
        if (E.first) E.first[gi] = fill;
      }
      continue;
    }
    if (E.first) {
      const double* __restrict__ xq = E.xq + q * D;
      double part = 0.0;
      for (int a = lane; a < D; a += kSolveThreads) part += xq[a] * bS[a];
      part = wave_sum(part);
      if (lane == 0) E.first[gi] = part;
    }
    if (!E.edit && !dth) continue;
    ldlt_solve<D>(H, bS, dd, ww, 0, D);
    __syncthreads();
    double part = 0.0;
    for (int a = lane; a < D; a += kSolveThreads) {
      part += g[a] * bS[a];
      if (dth) dth[M::ref_index(a)] = bS[a];
    }
    part = wave_sum(part);
    if (lane == 0 && E.edit) E.edit[gi] = part;
  }
}

// Per tile of kCandTile consecutive groups of the whole batch, one wave, kScoreRows values per lane
// (cand_newton.hip's tile selection): every (tile, query) segment selects its best min(K, length)
// values by |edit| into slot tile + q, the slots k_cand_merge reads; positions are the group's
// inside its query
__global__ __launch_bounds__(64) void k_edit_topk(int64_t Q, int64_t G, const int64_t* __restrict__ off,
                                                  const double* __restrict__ val, int K,
                                                  int32_t* __restrict__ cand_pos, double* __restrict__ cand_val) {
  static_assert(kCandTile == 64 * kScoreRows, "a tile is one wave's chunk");
  const int lane = threadIdx.x;
  const int64_t g0 = (int64_t)blockIdx.x * kCandTile;     // < G: the grid is ceil(G / tile)
  const int64_t tile_end = g0 + kCandTile < G ? g0 + kCandTile : G;
  const int nact = (int)(tile_end - g0);
  double v[kScoreRows];
#pragma unroll
  for (int r = 0; r < kScoreRows; ++r) v[r] = 64 * r + lane < nact ? val[g0 + 64 * r + lane] : NAN;
  int64_t q = 0;
  int cur = 0;
  while (cur < nact) {                       // every (tile, query) segment, in batch order (wave-uniform)
    q = last_at_most(off, q, Q - 1, g0 + cur);
    const int64_t qb = off[q], qe = off[q + 1];
    int end = (int)((qe < tile_end ? qe : tile_end) - g0);
    if (end <= cur) end = cur + 1;           // (offsets that are not monotone: still terminates)
    const int rounds = K < end - cur ? K : end - cur;
    double ca[kScoreRows];
    int cp[kScoreRows];
#pragma unroll
    for (int r = 0; r < kScoreRows; ++r) {
      const int idx = 64 * r + lane;
      const bool mine = idx >= cur && idx < end;
      ca[r] = mine ? topk_key(v[r]) : -2.0;
      cp[r] = mine ? (int)(g0 + idx - qb) : -1;
    }
    const int64_t slot = ((int64_t)blockIdx.x + q) * K;
    block_topk<kScoreRows, 64>(ca, cp, v, rounds, cand_pos + slot, cand_val + slot, nullptr, nullptr, nullptr);
    for (int t = rounds + lane; t < K; t += 64) {
      cand_pos[slot + t] = -1;
      cand_val[slot + t] = NAN;
    }
    cur = end;
  }
}

// LDS of one k_edit workgroup (k_group's)
template <class M>
constexpr int64_t edit_lds_bytes() {
  constexpr int64_t K = M::K, D = M::D;
  return 8 * (D * (D + 1) / 2 + 7 * D + 4 * K + 8 + (M::ncf ? 2 * K * K + K + K * (K / 2) + 2 * K : 8));
}

template <class M>
hipError_t edit_impl(fia_ctx* c, const QueryArgs& A, EditArgs E, int K, int64_t* topk_pos, double* topk_val,
                     hipStream_t s) {
  constexpr int D = M::D;
  const int64_t tiles = (E.G + kCandTile - 1) / kCandTile;
  if (K > 0) {
    FIA_HIP_TRY(c->cand_pos.reserve(sizeof(int32_t) * (size_t)((tiles + E.Q) * K), s));
    FIA_HIP_TRY(c->cand_val.reserve(sizeof(double) * (size_t)((tiles + E.Q) * K), s));
  }
  if (E.G > 0) {
    FIA_HIP_TRY(ensure_rowrec(c, s));
    E.rowrec = c->rowrec.as<int4>();
    // context scratch: x_q of every query for first_order, then the values of a top-K without `edit`
    const int64_t nx = E.first ? E.Q * D : 0;
    const bool own = K > 0 && !E.edit;
    if (nx > 0 || own) FIA_HIP_TRY(c->gxq.reserve(sizeof(double) * (size_t)(nx + (own ? E.G : 0)), s));
    phase_begin(c, 1, s);
    if (E.first) {
      E.xq = c->gxq.as<double>();
      FIA_HIP_TRY(launch_group_x(c, A, E.Q, c->gxq.as<double>(), s));
    }
    if (own) E.edit = c->gxq.as<double>() + nx;
    // persistent workgroups (NCF weights staged once each), as many as their LDS lets be resident
    const int64_t cap = solve_grid_cap(c, edit_lds_bytes<M>());
    hipLaunchKernelGGL(k_edit<M>, dim3((unsigned)(E.G < cap ? E.G : cap)), dim3(kSolveThreads), 0, s, A, E);
    FIA_HIP_TRY(hipGetLastError());
    phase_end(c, 1, s);
  }
  if (K > 0) {
    phase_begin(c, 3, s);
    if (E.G > 0) {
      hipLaunchKernelGGL(k_edit_topk, dim3((unsigned)tiles), dim3(64), 0, s, E.Q, E.G, E.grp_off, E.edit, K,
                         c->cand_pos.as<int32_t>(), c->cand_val.as<double>());
      FIA_HIP_TRY(hipGetLastError());
    }
    FIA_HIP_TRY(launch_cand_merge(c, E.Q, E.G, E.grp_off, K, topk_pos, topk_val, s));
    phase_end(c, 3, s);
  }
  return hipSuccess;
}

}  // namespace

hipError_t edit_influence(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* grp_offsets,
                          int64_t num_groups, const int64_t* rem_offsets, int64_t total_rem, const int32_t* rem_row,
                          const int64_t* add_offsets, int64_t total_add, const int32_t* add_user,
                          const int32_t* add_item, const float* add_rating, double* edit, double* first_order,
                          double* dtheta, int K, int64_t* topk_pos, double* topk_val, hipStream_t s) {
  const QueryArgs A = make_args(c, qu, qi);
  EditArgs E{};
  E.Q = Q;
  E.G = num_groups;
  E.TR = total_rem;
  E.TA = total_add;
  E.grp_off = grp_offsets;
  E.rem_off = rem_offsets;
  E.rem_row = rem_row;
  E.add_off = add_offsets;
  E.add_u = add_user;
  E.add_i = add_item;
  E.add_y = add_rating;
  E.edit = edit;
  E.first = first_order;
  E.dtheta = dtheta;
  hipError_t e = hipErrorInvalidValue;      // (group_supported is checked by the caller)
  dispatch_small(c->p.model, c->p.k, [&](auto m) { e = edit_impl<decltype(m)>(c, A, E, K, topk_pos, topk_val, s); });
  return e;
}

}  // namespace fia
