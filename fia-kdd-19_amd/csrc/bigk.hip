// Large-k FIA path: MF k in {128, 256} (side blocks of 129 / 257 coordinates) and
// NCF k in {64, 128, 256} (side blocks of 128 / 256 / 512) -- BASELINE.json config 5
// ("512x512 per-query Hessians, FP64 MFMA Cholesky").  Same math as models.hip
// (mf:164-251, ncf:193-280):
//
//   H_t = (2/n) (A_u (+) B_i) + wd*M + damping*I   (+ coupling iff (u,i) is a train row)
//   x   = H_t^{-1} v,   influence_j = (2 e_j x.g_j + wd x.(M theta)) / n
//
// but every structure is sized for blocks that do not fit a wave's registers or a
// CU's LDS:
//   * per train row, once per prepare: the residual e_j = r-hat_j - y_j and (NCF) the
//     restricted MLP gradient halves g_mlp,side = W1_side . d1_j of both sides
//     (k_resid_mf / k_ncf_rows, the NCF one as four f64-MFMA products per 16 ratings);
//   * per entity: the Gram A_e = sum g g^T in 16x16 tiles (tile-packed lower, fp64),
//     accumulated on v_mfma_f64_16x16x4_f64 from 16-rating slabs staged in LDS
//     (k_big_gram; long lists split into slices, partials summed in slot order);
//   * per (query, side) block -- or per query when the blocks couple -- a blocked
//     left-looking LDL^T (k_big_solve): each 32-column panel is updated from the
//     already-factored columns with MFMA (L streamed from a per-workgroup scratch,
//     D L^T on the fly), factored in LDS, written back.  The right-hand side v rides
//     along as the matrix's extra last row, so its row of L is D^-1 L^-1 v and only the
//     backward solve L^T x = y remains;
//   * scoring over entity chunks shared by every query of the batch with that entity
//     (k_big_score_mfma): the gathered rows / d1_j / e_j are streamed once per chunk
//     into 16 x 16 f64 MFMA products against blocks of 16 query vectors.
//
// This unit is the host side: the Gram work lists, the buffers and the order of the launches of
// prepare_big, big_systems and query_big.  The kernels are in one unit per phase, each behind
// launchers declared in bigk.h: bigk_prepare.hip, bigk_solve.hip (one workgroup per system),
// bigk_solve_batched.hip (the k_bs_* panels) and bigk_score.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "bigk.h"

namespace fia {
namespace {

// Gram work lists: slices of <= kBigSlice ratings of every cached entity, longest lists
// first; items {entity, start, len, dst} with dst >= 0 the cache slot, dst < 0 the partial
// slot -dst-1 of a split list; split lists get a combine entry {cache slot, first partial,
// n partials, 0} summed in slot order.  marks == nullptr: every entity, slot = entity id
// (lists cached per index); else only the marked entities, numbered in entity order.
hipError_t big_work_lists(fia_ctx* c, const std::vector<uint8_t>* marks, hipStream_t s) {
  Index& X = c->idx;
  if (!marks && !c->subset && c->bitems_version == X.version) return hipSuccess;
  for (int sd = 0; sd < 2; ++sd) {
    const std::vector<int64_t>& hp = X.hptr[sd];
    const int64_t ne = (int64_t)hp.size() - 1;
    std::vector<int32_t> slot((size_t)ne, -1);
    int32_t ncache = 0;
    for (int64_t e = 0; e < ne; ++e)
      if (!marks || marks[sd][(size_t)e]) slot[(size_t)e] = ncache++;
    std::vector<int32_t> items, comb;
    int32_t parts = 0;
    for (int32_t e : X.hord[sd]) {
      if (slot[(size_t)e] < 0) continue;
      const int64_t len = hp[(size_t)e + 1] - hp[(size_t)e];
      const int64_t nit = len == 0 ? 1 : (len + kBigSlice - 1) / kBigSlice;
      if (nit > 1) comb.insert(comb.end(), {slot[(size_t)e], parts, (int32_t)nit, 0});
      for (int64_t t = 0; t < nit; ++t) {
        const int64_t st = t * kBigSlice;
        const int64_t ln = std::min<int64_t>(kBigSlice, len - st);
        const int32_t dst = nit > 1 ? -(1 + parts++) : slot[(size_t)e];
        items.insert(items.end(), {e, (int32_t)st, (int32_t)(ln < 0 ? 0 : ln), dst});
      }
    }
    c->n_bitems[sd] = (int64_t)items.size() / 4;
    c->n_bcomb[sd] = (int64_t)comb.size() / 4;
    c->n_bslots[sd] = parts;
    c->n_bcache[sd] = ncache;
    if (!items.empty()) {
      FIA_HIP_TRY(c->bitems[sd].reserve(sizeof(int32_t) * items.size(), s));
      FIA_HIP_TRY(hipMemcpyAsync(c->bitems[sd].ptr, items.data(), sizeof(int32_t) * items.size(), hipMemcpyHostToDevice, s));
    }
    if (!comb.empty()) {
      FIA_HIP_TRY(c->bcomb[sd].reserve(sizeof(int32_t) * comb.size(), s));
      FIA_HIP_TRY(hipMemcpyAsync(c->bcomb[sd].ptr, comb.data(), sizeof(int32_t) * comb.size(), hipMemcpyHostToDevice, s));
    }
    if (marks) {
      FIA_HIP_TRY(c->slot[sd].reserve(sizeof(int32_t) * (size_t)(ne + 1), s));
      FIA_HIP_TRY(hipMemcpyAsync(c->slot[sd].ptr, slot.data(), sizeof(int32_t) * slot.size(), hipMemcpyHostToDevice, s));
    }
    FIA_HIP_TRY(hipStreamSynchronize(s));   // this side's host lists are freed at the end of the iteration
  }
  c->bitems_version = marks ? ~0ull : X.version;
  c->subset = marks != nullptr;
  return hipSuccess;
}

template <class M>
hipError_t prepare_big_impl(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, hipStream_t s) {
  constexpr int K = M::K;
  constexpr int64_t GW = gram_words<M>();
  const int model = c->p.model;
  const int64_t N = c->idx.N;
  const int64_t n_ent[2] = {c->p.U, c->p.I};
  // entity selection first (host round trip), so a too-large cache fails before any work
  std::vector<uint8_t> marks[2];
  if (qu) {
    FIA_HIP_TRY(mark_entities(c, Q, qu, qi, s));
    marks[0].resize((size_t)n_ent[0]);
    marks[1].resize((size_t)n_ent[1]);
    FIA_HIP_TRY(hipMemcpyAsync(marks[0].data(), c->mark.ptr, (size_t)n_ent[0], hipMemcpyDeviceToHost, s));
    FIA_HIP_TRY(hipMemcpyAsync(marks[1].data(), c->mark.as<uint8_t>() + n_ent[0], (size_t)n_ent[1],
                               hipMemcpyDeviceToHost, s));
    FIA_HIP_TRY(hipStreamSynchronize(s));
  }
  FIA_HIP_TRY(big_work_lists(c, qu ? marks : nullptr, s));
  FIA_HIP_TRY(ensure_self(c, s));
  FIA_HIP_TRY(c->resid.reserve(sizeof(double) * (size_t)(N + 1), s));
  if constexpr (M::ncf) {
    for (int sd = 0; sd < 2; ++sd) {
      FIA_HIP_TRY(c->l1[sd].reserve(sizeof(double) * (size_t)(n_ent[sd] * K + 1), s));
      FIA_HIP_TRY(c->gm[sd].reserve(sizeof(double) * (size_t)(N * K + 1), s));
    }
    FIA_HIP_TRY(c->wfrag.reserve(sizeof(double) * (size_t)3 * K * K, s));
  }
  FIA_HIP_TRY(launch_big_rows(model, K, c, qu != nullptr, s));
  for (int sd = 0; sd < 2; ++sd) {
    FIA_HIP_TRY(c->gram[sd].reserve(sizeof(double) * (size_t)((c->n_bcache[sd] > 0 ? c->n_bcache[sd] : 1) * GW), s));
    if (c->n_bslots[sd] > 0) FIA_HIP_TRY(c->gpart[sd].reserve(sizeof(double) * (size_t)(c->n_bslots[sd] * GW), s));
    FIA_HIP_TRY(launch_big_gram(model, K, c, sd, s));
  }
  return hipSuccess;
}

// the per-query work words (n, pair terms, v, theta_t) of a batch and, with `solve`, x = H^-1 v
// in c->xb: the prologue and the two solve launches, for query_big_impl and for group_big.hip
// (`sides` false: every query is known to be a train pair, so there are no side systems)
template <class M>
hipError_t big_systems_impl(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, bool solve, bool sides,
                            hipStream_t s) {
  constexpr int NPs = M::NPs;
  FIA_HIP_TRY(c->rec.reserve(sizeof(double) * (size_t)(Q * M::R + 1), s));
  FIA_HIP_TRY(c->qwork.reserve(sizeof(double) * (size_t)(Q * M::QW + 1), s));
  FIA_HIP_TRY(c->xb.reserve(sizeof(double) * (size_t)(Q * 2 * NPs + 1), s));
  FIA_HIP_TRY(c->syslist.reserve(sizeof(int32_t) * (size_t)(2 * Q + 2), s));
  FIA_HIP_TRY(c->cpllist.reserve(sizeof(int32_t) * (size_t)(Q + 2), s));
  const int model = c->p.model;
  FIA_HIP_TRY(hipMemsetAsync(c->syslist.ptr, 0, sizeof(int32_t), s));
  FIA_HIP_TRY(hipMemsetAsync(c->cpllist.ptr, 0, sizeof(int32_t), s));
  FIA_HIP_TRY(launch_big_prologue(model, M::K, c, Q, qu, qi, s));
  if (!solve) return hipSuccess;
  if (sides) FIA_HIP_TRY(launch_solve_batched(model, M::K, c, Q, qu, qi, s));
  return launch_solve(model, M::K, c, Q, qu, qi, s);
}

template <class M>
hipError_t query_big_impl(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                          int64_t max_chunks, int32_t* rel_idx, double* influence, double* x_out, int K,
                          int64_t* topk_pos, int64_t* topk_idx, double* topk_val, hipStream_t s,
                          const double* x_in) {
  constexpr int NPASS = kScoreRows;
  if (K > 0) {
    FIA_HIP_TRY(c->cand_pos.reserve(sizeof(int32_t) * (size_t)((max_chunks + 1) * K * NPASS), s));
    FIA_HIP_TRY(c->cand_val.reserve(sizeof(double) * (size_t)((max_chunks + 1) * K * NPASS), s));
  }
  const int model = c->p.model;
  phase_begin(c, 4, s);
  FIA_HIP_TRY(build_chunks(c, Q, qu, qi, offsets, max_chunks, true, s));
  FIA_HIP_TRY(build_groups(c, Q, qu, qi, offsets, max_chunks, kBigMfmaQB, s));
  phase_end(c, 4, s);
  phase_begin(c, 1, s);
  // a given inverse HVP (fia_query_batch_x): the records straight from it, no solve
  FIA_HIP_TRY(big_systems_impl<M>(c, Q, qu, qi, x_in == nullptr, true, s));
  if (x_in) FIA_HIP_TRY(launch_big_record_x(model, M::K, c, Q, qu, qi, x_in, s));
  FIA_HIP_TRY(launch_big_finish(model, M::K, c, Q, x_out, s));
  phase_end(c, 1, s);
  FIA_HIP_TRY(launch_big_score(model, M::K, c, qu, qi, max_chunks, rel_idx, influence, K, phase_span(c, 2), s));
  if (K > 0) {
    phase_begin(c, 3, s);
    FIA_HIP_TRY(launch_topk_merge(c, Q, qu, qi, K, NPASS, topk_pos, topk_idx, topk_val, s, max_chunks));
    phase_end(c, 3, s);
  }
  return hipSuccess;
}

}  // namespace

// per-list-position owning entity of both sides (rebuilt when the index changes)
hipError_t ensure_self(fia_ctx* c, hipStream_t s) {
  const Index& X = c->idx;
  if (c->self_version == X.version) return hipSuccess;
  const int64_t N = X.N, n_ent[2] = {X.U, X.I};
  for (int sd = 0; sd < 2; ++sd) {
    FIA_HIP_TRY(c->self[sd].reserve(sizeof(int32_t) * (size_t)(N + 1), s));
    if (N > 0) FIA_HIP_TRY(launch_self(N, n_ent[sd], X.side[sd].ptr.as<int64_t>(), c->self[sd].as<int32_t>(), s));
  }
  c->self_version = X.version;
  return hipSuccess;
}

bool big_supported(int model, int k) {
  return for_big_size<BMF, BNCF>(model, k, [](auto) {});
}

hipError_t prepare_big(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, hipStream_t s) {
  c->small_subset = false;
  return big_dispatch(c->p.model, c->p.k, [&](auto m) { return prepare_big_impl<decltype(m)>(c, Q, qu, qi, s); });
}

hipError_t check_cover(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, int32_t* flag, hipStream_t s) {
  if (!c->subset || Q <= 0) return hipSuccess;
  return launch_check_cover(c, Q, qu, qi, flag, s);
}

hipError_t big_systems(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, bool solve, bool sides,
                       hipStream_t s) {
  return big_dispatch(c->p.model, c->p.k,
                      [&](auto m) { return big_systems_impl<decltype(m)>(c, Q, qu, qi, solve, sides, s); });
}

hipError_t query_big(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                     int64_t max_chunks, int32_t* rel_idx, double* influence, double* x_out, int K,
                     int64_t* topk_pos, int64_t* topk_idx, double* topk_val, hipStream_t s, const double* x_in) {
  return big_dispatch(c->p.model, c->p.k, [&](auto m) {
    return query_big_impl<decltype(m)>(c, Q, qu, qi, offsets, max_chunks, rel_idx, influence, x_out, K, topk_pos,
                                       topk_idx, topk_val, s, x_in);
  });
}

}  // namespace fia
