// fia_group_influence: the Newton-corrected effect on r-hat(u, i) of removing a SET of train
// rows together (include/fia.h).  For query q = (u, i) with n related ratings, v = d r-hat / d
// theta_t and the assembled H of fia_query_batch, and a group S of train rows j = (a, b, y):
//
//   m_j  = [a == u] + [b == i]                                 occurrences of j in q's related list
//   H_S  = (1/n) sum_{j in S} m_j (2 g_j g_j^T + 2 e_j C_j + wd M)
//   b_S  = (1/n) sum_{j in S} m_j (2 e_j g_j + wd M theta_t)
//   dtheta = (H - H_S)^-1 b_S,  group = v . dtheta,  first_order = (H^-1 v) . b_S
//
// The sum of the single-rating influences (first_order) keeps the curvature of the removed
// ratings in H; a group is a sizeable part of the few hundred ratings H averages over, so the
// system is downdated and solved again.  H_S is not low rank (wd M / n is diagonal), and the
// system is small (D = 2k + 2 or 4k): one exact LDL^T per group, the work of one coupled
// k_solve query.
//
// Kernels (one wave per work item, as k_solve):
//   k_row_rec      once per index: train row -> {user, item, rating, list position}, from the
//                  user-major lists (the owner of a position by binary search in the list
//                  pointers), so a member costs one 16-B load instead of a dependent chain
//   k_group_x      per query, only when first_order is asked for: x_q = H^-1 v (full coupled
//                  LDL^T) into context scratch, block order
//   k_group        per group: prologue of (u, i), H from the two Gram caches, then the members
//                  in list order -- prologue of (a, b) for e_j and g_j (the blocks of a side
//                  that does not match zeroed), H -= the member's terms on the packed triangle,
//                  b_S += its gradient -- then one full-range ldlt_solve and the dot with v
// No floating-point atomics; every LDS entry is updated by one lane per member, members in
// list order, so the same inputs give the same bits wherever the group sits in the batch.
#include "solve.h"

namespace fia {
namespace {

struct GroupArgs {
  int64_t Q, G, TM;
  const int64_t* grp_off;    // [Q + 1]
  const int64_t* mem_off;    // [G + 1]
  const int32_t* mem_row;    // [TM]
  const int4* rowrec;        // [N] train row -> {user, item, rating bits, user-major list position}
  double* xq;                // [Q * D] H^-1 v, block order (k_group_x); null: no first_order
  double* group;             // [G]
  double* first;             // [G]
  double* dtheta;            // [G * D], reference theta order
};

// one thread per position g of the user-major lists; its user: the largest e in [0, U) with
// ptr[e] <= g (ptr[0] = 0 <= g)
__global__ void k_row_rec(int64_t N, int64_t U, const int64_t* __restrict__ ptr, const int32_t* __restrict__ row,
                          const int32_t* __restrict__ other, const float* __restrict__ rating,
                          int4* __restrict__ rec) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= N) return;
  const int64_t lo = last_at_most(ptr, (int64_t)0, U - 1, g);
  rec[row[g]] = make_int4((int)lo, other[g], __float_as_int(rating[g]), (int)g);
}

// x_q = H^-1 v of every query with n_q > 0 (the others' slots are never read)
template <class M>
__global__ __launch_bounds__(kSolveThreads) void k_group_x(QueryArgs A, GroupArgs Gr) {
  constexpr int K = M::K, D = M::D;
  __shared__ double H[D * (D + 1) / 2];
  __shared__ double v[D], g[D], th[D], dd[D], ww[D];
  __shared__ double sh[4 * K + 8];
  __shared__ NCFWeights<M::ncf ? K : 2> w;
  __shared__ double sW1[M::ncf ? 2 * K * K : 1];
  __shared__ double sb1[M::ncf ? K : 1];
  stage_ncf<M>(A, w, sW1, sb1);
  const int lane = threadIdx.x;
  for (int64_t q = blockIdx.x; q < Gr.Q; q += gridDim.x) {
    __syncthreads();
    const int32_t u = A.qu[q], i = A.qi[q];
    const int64_t n = related_count(A, u, i);
    if (n == 0) continue;
    const double rhat_ui = solve_prologue<M, kSolveThreads>(A, u, i, th, g, sh, w, sW1, sb1);
    assemble_hessian<M>(A, u, i, n, rhat_ui, g, H);
    for (int a = lane; a < D; a += kSolveThreads) v[a] = g[a];
    __syncthreads();
    ldlt_solve<D>(H, v, dd, ww, 0, D);
    __syncthreads();
    for (int a = lane; a < D; a += kSolveThreads) Gr.xq[q * D + a] = v[a];
  }
}

template <class M>
__global__ __launch_bounds__(kSolveThreads) void k_group(QueryArgs A, GroupArgs Gr) {
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
  for (int64_t gi = blockIdx.x; gi < Gr.G; gi += gridDim.x) {
    __syncthreads();
    // the group's query: the largest q in [0, Q) with grp_off[q] <= gi
    const int64_t q = last_at_most(Gr.grp_off, (int64_t)0, Gr.Q - 1, gi);
    const int32_t u = A.qu[q], i = A.qi[q];
    const int64_t n = related_count(A, u, i);
    int64_t m0 = Gr.mem_off[gi], m1 = Gr.mem_off[gi + 1];
    m0 = m0 < 0 ? 0 : m0;                             // (never past the member array)
    m1 = m1 > Gr.TM ? Gr.TM : m1;
    bool bad = n == 0;
    int neff = 0;
    if (!bad) {
      const double rhat_ui = solve_prologue<M, kSolveThreads>(A, u, i, th, g, sh, w, sW1, sb1);
      assemble_hessian<M>(A, u, i, n, rhat_ui, g, H);
      for (int a = lane; a < D; a += kSolveThreads) bS[a] = 0.0;
      __syncthreads();
      const double inv_n = 1.0 / (double)n;
      // ---- the members, in list order (every value below is the same in all lanes) ----
      for (int64_t m = m0; m < m1 && !bad; ++m) {
        const int32_t row = Gr.mem_row[m];
        if (row < 0 || row >= A.N) {                  // never used as an index
          bad = true;
          break;
        }
        const int4 rr = Gr.rowrec[row];
        const int32_t a = rr.x, b = rr.y;
        const bool on_u = a == u, on_i = b == i;
        if (!on_u && !on_i) continue;                 // m_j = 0: contributes nothing
        ++neff;
        const double y = (double)__int_as_float(rr.z);
        __syncthreads();                              // the previous member's reads of gj
        const double e = solve_prologue<M, kSolveThreads>(A, a, b, thj, gj, sh, w, sW1, sb1) - y;
        // g_j: the blocks of a side that does not match are zero
        if (!on_u)
          for (int c = lane; c < Ds; c += kSolveThreads) gj[c] = 0.0;
        if (!on_i)
          for (int c = lane; c < Ds; c += kSolveThreads) gj[Ds + c] = 0.0;
        __syncthreads();
        const double mn = ((on_u ? 1.0 : 0.0) + (on_i ? 1.0 : 0.0)) * inv_n;    // m_j / n
        // H -= the member's terms, g_j g_j^T on the blocks where g_j is nonzero; b_S += its gradient
        remove_member<M>(H, gj, e, mn, on_u ? 0 : Ds, on_i ? D : Ds, on_u && on_i, w, A.wd);
        for (int c = lane; c < D; c += kSolveThreads) bS[c] += member_rhs<M>(c, gj, th, e, mn, A.wd);
      }
      __syncthreads();
    }
    double* __restrict__ dth = Gr.dtheta ? Gr.dtheta + gi * D : nullptr;
    if (bad || neff == 0) {
      // NaN: n_q = 0, a query id or a member row out of range; +0.0: nothing removed
      const double fill = bad ? NAN : 0.0;
      if (dth)
        for (int a = lane; a < D; a += kSolveThreads) dth[a] = fill;
      if (lane == 0) {
        if (Gr.group) Gr.group[gi] = fill;
        if (Gr.first) Gr.first[gi] = fill;
      }
      continue;
    }
    if (Gr.first) {
      const double* __restrict__ xq = Gr.xq + q * D;
      double part = 0.0;
      for (int a = lane; a < D; a += kSolveThreads) part += xq[a] * bS[a];
      part = wave_sum(part);
      if (lane == 0) Gr.first[gi] = part;
    }
    if (!Gr.group && !dth) continue;
    // the blocks are coupled when H was or a member is the own pair: the full solve is always right
    ldlt_solve<D>(H, bS, dd, ww, 0, D);
    __syncthreads();
    double part = 0.0;
    for (int a = lane; a < D; a += kSolveThreads) {
      part += g[a] * bS[a];
      if (dth) dth[M::ref_index(a)] = bS[a];
    }
    part = wave_sum(part);
    if (lane == 0 && Gr.group) Gr.group[gi] = part;
  }
}

// LDS of one k_group workgroup (k_group_x holds a little less)
template <class M>
constexpr int64_t group_lds_bytes() {
  constexpr int64_t K = M::K, D = M::D;
  return 8 * (D * (D + 1) / 2 + 7 * D + 4 * K + 8 + (M::ncf ? 2 * K * K + K + K * (K / 2) + 2 * K : 8));
}

template <class M>
hipError_t group_impl(fia_ctx* c, const QueryArgs& A, GroupArgs Gr, hipStream_t s) {
  constexpr int D = M::D;
  FIA_HIP_TRY(ensure_rowrec(c, s));
  Gr.rowrec = c->rowrec.as<int4>();
  // persistent workgroups (NCF weights staged once each), as many as their LDS lets be resident
  const int64_t cap = solve_grid_cap(c, group_lds_bytes<M>());
  if (Gr.first) {
    FIA_HIP_TRY(c->gxq.reserve(sizeof(double) * (size_t)(Gr.Q * D), s));
    Gr.xq = c->gxq.as<double>();
    hipLaunchKernelGGL(k_group_x<M>, dim3((unsigned)(Gr.Q < cap ? Gr.Q : cap)), dim3(kSolveThreads), 0, s, A, Gr);
    FIA_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_group<M>, dim3((unsigned)(Gr.G < cap ? Gr.G : cap)), dim3(kSolveThreads), 0, s, A, Gr);
  return hipGetLastError();
}

}  // namespace

hipError_t ensure_rowrec(fia_ctx* c, hipStream_t s) {
  if (c->rowrec_version == c->idx.version) return hipSuccess;
  const int64_t N = c->idx.N;
  FIA_HIP_TRY(c->rowrec.reserve(sizeof(int4) * (size_t)(N > 0 ? N : 1), s));
  if (N > 0) {
    const Side& us = c->idx.side[0];
    hipLaunchKernelGGL(k_row_rec, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, N, (int64_t)c->p.U,
                       us.ptr.as<int64_t>(), us.row.as<int32_t>(), us.other.as<int32_t>(), us.rating.as<float>(),
                       c->rowrec.as<int4>());
    FIA_HIP_TRY(hipGetLastError());
  }
  c->rowrec_version = c->idx.version;
  return hipSuccess;
}

hipError_t launch_group_x(fia_ctx* c, const QueryArgs& A, int64_t Q, double* xq, hipStream_t s) {
  GroupArgs Gr{};
  Gr.Q = Q;
  Gr.xq = xq;
  hipError_t e = hipErrorInvalidValue;
  dispatch_small(c->p.model, c->p.k, [&](auto m) {
    using M = decltype(m);
    const int64_t cap = solve_grid_cap(c, group_lds_bytes<M>());
    hipLaunchKernelGGL(k_group_x<M>, dim3((unsigned)(Q < cap ? Q : cap)), dim3(kSolveThreads), 0, s, A, Gr);
    e = hipGetLastError();
  });
  return e;
}

bool group_supported(int model, int k) {
  return dispatch_small(model, k, [](auto) {});
}

hipError_t group_influence(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* grp_offsets,
                           int64_t num_groups, const int64_t* mem_offsets, int64_t total_members,
                           const int32_t* mem_row, double* group, double* first_order, double* dtheta,
                           hipStream_t s) {
  const QueryArgs A = make_args(c, qu, qi);
  GroupArgs Gr{};
  Gr.Q = Q;
  Gr.G = num_groups;
  Gr.TM = total_members;
  Gr.grp_off = grp_offsets;
  Gr.mem_off = mem_offsets;
  Gr.mem_row = mem_row;
  Gr.group = group;
  Gr.first = first_order;
  Gr.dtheta = dtheta;
  hipError_t e = hipErrorInvalidValue;      // (group_supported is checked by the caller)
  dispatch_small(c->p.model, c->p.k, [&](auto m) { e = group_impl<decltype(m)>(c, A, Gr, s); });
  return e;
}

}  // namespace fia
