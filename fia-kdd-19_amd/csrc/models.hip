// FIA hot path for MF and NCF on gfx950: entity Gram caches, per-query exact
// solve, flattened influence scoring with chunk-local top-K, top-K merge.  This unit is the
// host side of the small-k path: the kernel arguments, the buffers, the phase events and the
// order of launches of a prepare and of a query batch, and the model dispatch.  The kernels
// are in small_gram.hip (prepare; MF k <= 16: gram_mf.hip), small_solve.hip, and the scoring
// units score_mf.hip, score_mfma.hip, small_score.hip (the last with the top-K merge).
//
// Math (reference citations inline):
//   theta_t per query (u,i), split into a user block and an item block
//     MF  user [p_u (k), b_u]   item [q_i (k), b_i]            Ds = k+1
//     NCF user [Pm_u, Pg_u]     item [Qm_i, Qg_i]              Ds = 2k
//   g_j = d r_j / d theta_t is nonzero only in the user block for j in R_u and
//   only in the item block for j in C_i (both for the (u,i) row itself), so
//     H_t = (2/n) (A_u (+) B_i) + dup correction + wd*M + damping*I
//   with A_u = sum_{j in R_u} g g^T (per user, independent of i) and B_i the
//   item analogue: the rank-1 second-derivative updates (mf:288-308, 324-351)
//   are accumulated ONCE per entity (k_gram) and every query assembles its
//   Hessian from two cached blocks.
//   x = H_t^{-1} v by an exact fp64 LDL^T in LDS (replaces fmin_ncg, mf:419-433).
//   influence_j = x . (2 e_j g_j + wd*M*theta_t) / n (mf:237-246).
#include "kern.h"
#include "scan.h"    // ScanArgs, chunk_scan_args, launch_chunk_scan

namespace fia {

QueryArgs make_args(fia_ctx* c, const int32_t* qu, const int32_t* qi) {
  QueryArgs A{};
  fill_list_args(c, A);
  A.qu = qu;
  A.qi = qi;
  A.lgm[0] = c->gm[0].as<double>();
  A.lgm[1] = c->gm[1].as<double>();
  A.lres = c->resid.as<double>();
  A.N = c->idx.N;
  return A;
}

namespace {

// the launchers' (model, k) of the traits M
template <class M>
constexpr int kModel = M::ncf ? FIA_MODEL_NCF : FIA_MODEL_MF;

// MF k <= 16 item runs: slice cost target (descriptor cost units per one-wave slice; ml-1m-ex
// same-box A/B, scoring us -- round 4: 8 -> 69.4, 16 -> 68.6, 32 -> 73.5, 64 -> 78.6; round 5
// (this kernel): 4 -> 62.0, 8 -> 58.0-58.6, 16 -> 58.8; chunks of 64 / 192 / 256 ratings at
// 8: 66.3 / 62.0 / 85.8 vs 128; runs of <= 32 queries: 62.6)
constexpr int kRunLambda = 8;

// MF k <= 16: the Gram stream (its descriptors carry the entity in 24 bits)
template <class M>
bool use_gram_stream(const int64_t (&n_ent)[2]) {
  // (and a table's bytes in a 32-bit buffer range)
  return !M::ncf && M::K <= 16 && n_ent[0] < (1 << 23) && n_ent[1] < (1 << 23);
}

template <class M>
hipError_t prepare_impl(fia_ctx* c, hipStream_t s, const uint8_t* mark) {
  constexpr int Ds = M::Ds, GS = Ds * (Ds + 1) / 2, K = M::K;
  const int64_t n_ent[2] = {c->p.U, c->p.I};
  for (int sd = 0; sd < 2; ++sd) FIA_HIP_TRY(c->gram[sd].reserve(sizeof(double) * (size_t)(n_ent[sd] * ((GS + 1) & ~1) + 1), s));
  if constexpr (M::ncf) {
    for (int sd = 0; sd < 2; ++sd) {
      FIA_HIP_TRY(c->l1[sd].reserve(sizeof(double) * (size_t)(n_ent[sd] * K + 1), s));
      if (n_ent[sd] > 0) FIA_HIP_TRY(launch_ncf_l1(K, c->p.t[sd], c->p.t[4], sd, n_ent[sd], c->l1[sd].as<double>(), s));
    }
    if (s == c->aux && c->l1_ev) {       // on the aux stream: the query prologue may start here
      FIA_HIP_TRY(hipEventRecord(c->l1_ev, s));
      c->l1_pending = true;
    }
  }
  constexpr int GSP = (GS + 1) & ~1;
  const Index& X = c->idx;
  // MF k <= 16: the Gram stream (both sides, one launch).  It cuts its own sub-batches
  // (build_gram_stream) and needs neither the slice lists of the per-slice kernels nor their
  // partial-Gram slots; a split list is summed by the workgroup that holds its slices, and only
  // lists beyond a team's reach leave partial slices for the combine (none: no second launch)
  if (use_gram_stream<M>(n_ent)) {
    FIA_HIP_TRY(build_gram_stream(c, K, s));
    for (int sd = 0; sd < 2; ++sd)
      if (X.n_gsslots[sd] > 0) FIA_HIP_TRY(c->gpart[sd].reserve(sizeof(double) * (size_t)(X.n_gsslots[sd] * GSP), s));
    GramStreamArgs GT{};
    GT.desc = X.gsdesc.as<int2>();
    GT.ids = X.gsids.as<uint32_t>();
    GT.wave = X.gswave.as<int32_t>();
    GT.n_waves = X.n_gsw;
    for (int sd = 0; sd < 2; ++sd) {
      GT.emb_other[sd] = c->p.t[sd == 0 ? 1 : 0];
      GT.bytes_other[sd] = (uint32_t)(n_ent[1 - sd] * K * (int64_t)sizeof(float));
      GT.gram[sd] = c->gram[sd].as<double>();
      GT.part[sd] = c->gpart[sd].as<double>();
    }
    GT.mark = mark;
    GT.moff[0] = 0;
    GT.moff[1] = n_ent[0];
    if (X.n_gsw > 0) FIA_HIP_TRY(launch_gram_mf_stream(M::K, GT, s));
    return launch_gram_combine(c, X.n_gscomb[0], X.gscomb[0].as<int32_t>(), X.n_gscomb[1], X.gscomb[1].as<int32_t>(),
                               GS, GSP, mark, s);
  }
  // the per-slice Gram kernels (k_ncf_gram_rows, k_gram_mf_mfma).  Gram slice length: short
  // slices for parallelism, long enough that the partial Grams of split lists (GSP doubles
  // each) stay a few bytes per rating (MI355X: ml-1m-ex MF k=16 best at 256, 20M MF k=64 loses
  // 30% at 256 vs 512)
  int64_t want = 256;
  while (!M::ncf && want < 4096 && want < GSP) want *= 2;   // NCF: 256 (16 slabs per item)
  if (c->idx.gchunk != want) FIA_HIP_TRY(build_gram_lists(c, want, s));
  for (int sd = 0; sd < 2; ++sd)
    if (X.n_gslots[sd] > 0) FIA_HIP_TRY(c->gpart[sd].reserve(sizeof(double) * (size_t)(X.n_gslots[sd] * GSP), s));
  if constexpr (M::ncf) {
    // per list position of each side, written with the Grams: e, and g_mlp coordinate-major
    // [k][N] or (mask path) the ReLU masks int32 [N]
    const int64_t N = X.N;
    const size_t per = mask_path<M>() ? sizeof(int32_t) * (size_t)(N + 2) : sizeof(double) * (size_t)(N * K + 1);
    for (int sd = 0; sd < 2; ++sd) FIA_HIP_TRY(c->gm[sd].reserve(per, s));
    FIA_HIP_TRY(c->resid.reserve(sizeof(double) * (size_t)(2 * N + 1), s));
  } else if constexpr (K == 32 || K == 64) {
    // list-ordered residuals of both sides for k_score_mf_mfma ([0, N) users, [N, 2N) items),
    // written by the Gram pass for every list position of a cached entity
    FIA_HIP_TRY(c->resid.reserve(sizeof(double) * (size_t)(2 * X.N + 1), s));
  }
  FIA_HIP_TRY(launch_gram_slices(kModel<M>, K, c, mark, s));
  return launch_gram_combine(c, n_ent[0] > 0 ? X.n_gcomb[0] : 0, X.gcomb[0].as<int32_t>(),
                             n_ent[1] > 0 ? X.n_gcomb[1] : 0, X.gcomb[1].as<int32_t>(), GS, GSP, mark, s);
}

template <class M>
hipError_t query_impl(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                      int64_t max_chunks, int32_t* rel_idx, double* influence, double* x_out, int K,
                      int64_t* topk_pos, int64_t* topk_idx, double* topk_val, hipStream_t s,
                      const double* x_in) {
  // One scoring schedule per (model, k, K) (measured on MI355X, profiles/): k <= 16 item runs
  // (MF k_score_mf_runs, NCF k_score_ncf_runs: per-query chunks sharing the item's list); MF
  // k in {32, 64} entity-shared, on f64 MFMA for K <= 1 (k_score_mf_mfma, query blocks of 16)
  // and on VALU otherwise (k_score_grouped_mf); NCF k = 32 entity-shared (k_score_ncf)
  constexpr bool grouped = M::ncf ? !mask_path<M>() : M::K >= 32;
  constexpr bool mfma_ok = !M::ncf && (M::K == 32 || M::K == 64);
  const bool use_mfma = mfma_ok && K <= 1;
  // (the MFMA kernel's work item is a group of kWgBlocks query blocks, one per wave)
  const int qblock = use_mfma ? kMfmaQB * kWgBlocks : query_block<M>();
  constexpr bool runs = !grouped;
  constexpr int spc = 1;      // candidate slot sets per chunk
  static_assert(solve_covered<M>(), "every small-k model has a side-system solve");
  FIA_HIP_TRY(c->rec.reserve(sizeof(double) * (size_t)(Q * M::R + 1), s));
  if (K > 0) {
    FIA_HIP_TRY(c->cand_pos.reserve(sizeof(int32_t) * (size_t)((max_chunks + 1) * K * spc), s));
    FIA_HIP_TRY(c->cand_val.reserve(sizeof(double) * (size_t)((max_chunks + 1) * K * spc), s));
  }
  QueryArgs A = make_args(c, qu, qi);
  const int64_t nE = c->idx.U + c->idx.I;
  // every (entity chunk, query block) item covers >= 1 per-query chunk
  const int64_t max_items = max_chunks;
  // the queries whose test pair is a train row are listed in `coupled` {count, q...} by the
  // solve and finished full-D by k_solve, whose last reader leaves {readers, count} zero (the
  // word pair in front of the list: fia_ctx::coupled); zero when (re)allocated.  (MF k = 16
  // neither appends nor reads: its coupled queries are a role of k_solve_quad.)
  if (c->coupled.bytes < sizeof(int32_t) * (size_t)(Q + 2) || !c->coupled.ptr) {
    FIA_HIP_TRY(c->coupled.reserve(sizeof(int32_t) * (size_t)(Q + 2), s));
    FIA_HIP_TRY(hipMemsetAsync(c->coupled.ptr, 0, c->coupled.bytes, s));
  }
  int32_t* const coupled = c->coupled.as<int32_t>() + 1;
  // MF k = 16: the chunk scan, the side-system solves and the coupled solves are one launch
  // (k_solve_quad), timed as the solve phase -- the chunk phase then records nothing.  Without
  // a solve (a given x, an empty batch) the chunk phase is the one scan kernel.  Either way the
  // events are stamped by those kernels' dispatches (a marker packet per event idled the GPU
  // ~5 us: RQ2's single query), and a pair is taken only once its launch is known to proceed.
  constexpr bool ext_phases = runs && !M::ncf && use_quad_solve<M>();
  const bool fused = ext_phases && Q > 0 && !x_in;
  if (!ext_phases) phase_begin(c, 4, s);
  // MF k <= 16 item runs: one wave per equal-cost slice of the descriptor list (descriptor
  // costs vary ~10x: a static stride over descriptors left waves idle for half the kernel);
  // the slice count is known on the device only -- the grid is its bound (total cost <=
  // kRunUserCost per descriptor slot), the surplus waves exit at once
  constexpr int64_t lam = kRunLambda;
  const int64_t runs_grid = (kRunUserCost * (max_chunks + 1)) / lam + 2;
  // (the scan zeroes the coupled count only where it is a launch of its own, ahead of a solve
  // that appends to it; the fused launch has no list)
  ScanArgs S;
  FIA_HIP_TRY(chunk_scan_args(c, Q, qu, qi, offsets, max_chunks, grouped, s, fused ? nullptr : coupled, runs, (int)lam,
                              M::ncf ? kNcfRunChunk : kRunChunk, S));
  if (!fused) {
    const PhaseSpan cspan = ext_phases ? phase_span(c, 4) : PhaseSpan{};
    if (const hipError_t eb = launch_chunk_scan(S, s, cspan.a, cspan.b); eb != hipSuccess) {
      phase_drop(c, 4, cspan);
      return eb;
    }
  }
  if (grouped) FIA_HIP_TRY(build_groups(c, Q, qu, qi, offsets, max_items, qblock, s, use_mfma ? kMfmaCPI : 1));
  // the query-side work that needs no Gram cache, ahead of the join with a pending prepare:
  // NCF k = 16 the per-query MLP prologue (after the layer-1 rows), k <= 16 the d1 table
  // (timed with the chunk lists: the solve phase starts after the join)
  if constexpr (pair_layout<M>()) {
    if (Q > 0 && !x_in) {
      FIA_HIP_TRY(join_l1(c, s));
      FIA_HIP_TRY(c->qwork.reserve(sizeof(double) * (size_t)(Q * QPro<M>::stride + 1), s));
      FIA_HIP_TRY(launch_ncf_query_pro(M::K, A, Q, c->qwork.as<double>(), s));
    }
  }
  if constexpr (mask_path<M>()) {
    if (Q > 0) {
      FIA_HIP_TRY(c->d1tab.reserve(sizeof(double) * (1 << (M::K / 2)) * M::K, s));
      FIA_HIP_TRY(launch_ncf_d1_table(M::K, c->p.t[6], c->p.t[8], c->d1tab.as<double>(), s));
      A.d1tab = c->d1tab.as<double>();
    }
  }
  if (!ext_phases) phase_end(c, 4, s);
  FIA_HIP_TRY(join_prepare(c, s));     // the Gram caches (and NCF rows) of a pending fia_prepare
  const bool ext_solve = fused;
  PhaseSpan sspan;
  if (!ext_solve) phase_begin(c, 1, s);
  // a given inverse HVP: records straight from it, no solve (fia_query_batch_x)
  if (x_in && Q > 0) FIA_HIP_TRY(launch_record_x(kModel<M>, M::K, A, Q, x_in, c->rec.as<double>(), x_out, s));
  if (Q > 0 && !x_in) {
    // MF k = 16: the solve phase is the one dispatch of k_solve_quad, which stamps both of its
    // events; the other models' side solves list their coupled queries for k_solve (usually
    // none: a small grid that exits), whose dispatch would stamp the end
    if constexpr (use_quad_solve<M>()) sspan = phase_span(c, 1);
    hipError_t es = launch_side_solve(kModel<M>, M::K, c, S, A, Q, x_out, coupled, s, sspan);
    if constexpr (!use_quad_solve<M>())
      if (es == hipSuccess)
        es = launch_coupled_solve(kModel<M>, M::K, A, Q, c->rec.as<double>(), x_out, coupled, s, sspan.b);
    if (es != hipSuccess) {
      phase_drop(c, 1, sspan);
      return es;
    }
  }
  if constexpr (mask_path<M>()) {
    // the records' MLP block -> y = W1_side^T x_mlp for k_score_ncf_runs
    if (Q > 0) FIA_HIP_TRY(launch_ncf_rec_y(M::K, Q, c->p.t[4], c->rec.as<double>(), s));
  }
  if (!ext_solve) phase_end(c, 1, s);
  int64_t grid = (max_items + 3) / 4;            // 4 waves (work items) per block
  if (grid < 1) grid = 1;
  // grid cap (measured): NCF 1024 workgroups (yelp-ex score 0.314 -> 0.290 ms), MF 8192
  const int64_t gcap = M::ncf ? 1024 : 8192;
  if (grid > gcap) grid = gcap;
  if (runs) grid = runs_grid;
  // the MFMA kernel: one work item per workgroup (grid-stride)
  if (use_mfma) grid = max_items < 8192 ? (max_items > 0 ? max_items : 1) : 8192;
  const PhaseSpan span = phase_span(c, 2);
  if constexpr (grouped) {
    if (use_mfma)
      FIA_HIP_TRY(launch_score_mf_mfma(M::K, rel_idx && influence, grid, s, span, A, nE, c->wstart.as<int64_t>(),
                                       c->witems.as<int32_t>(), c->gstart.as<int64_t>(), c->gq.as<int32_t>(),
                                       c->qbase.as<int64_t>(), c->rec.as<double>(), rel_idx, influence, K,
                                       c->cand_pos.as<int32_t>(), c->cand_val.as<double>()));
    else
      FIA_HIP_TRY(launch_score_grouped(kModel<M>, M::K, grid, s, span, A, nE, c->wstart.as<int64_t>(),
                                       c->witems.as<int32_t>(), c->gstart.as<int64_t>(), c->gq.as<int32_t>(),
                                       c->qbase.as<int64_t>(), c->rec.as<double>(), rel_idx, influence, K,
                                       c->cand_pos.as<int32_t>(), c->cand_val.as<double>()));
  } else if constexpr (!M::ncf) {
    // k <= 16: item runs
    FIA_HIP_TRY(launch_score_mf_runs(M::K, grid, s, A, Q, c->cdesc.as<ChunkDesc>(), c->qbase.as<int64_t>(),
                                     c->slices.as<int32_t>(), c->rec.as<double>(), rel_idx, influence, K,
                                     c->cand_pos.as<int32_t>(), c->cand_val.as<double>(), span));
  } else {
    FIA_HIP_TRY(launch_score_ncf_runs(M::K, grid, s, A, Q, c->cdesc.as<ChunkDesc>(), c->qbase.as<int64_t>(),
                                      c->slices.as<int32_t>(), c->rec.as<double>(), rel_idx, influence, K,
                                      c->cand_pos.as<int32_t>(), c->cand_val.as<double>(), span));
  }
  if (K > 0 && Q > 0) {
    phase_begin(c, 3, s);
    FIA_HIP_TRY(launch_topk_merge(c, Q, qu, qi, K, spc, topk_pos, topk_idx, topk_val, s, max_chunks));
    phase_end(c, 3, s);
  }
  return hipSuccess;
}

}  // namespace

bool model_supported(int model, int k) {
  return dispatch_any(model, k, [](auto) {});
}

int model_num_params(int model, int k) {
  if (model == FIA_MODEL_MF) return 2 * k + 2;
  if (model == FIA_MODEL_NCF) return 4 * k;
  return 0;
}

hipError_t prepare_model(fia_ctx* c, hipStream_t s, bool& unsupported) {
  unsupported = false;
  c->subset = false;
  c->small_subset = false;
  hipError_t e = hipSuccess;
  if (dispatch_small(c->p.model, c->p.k, [&](auto m) { e = prepare_impl<decltype(m)>(c, s, nullptr); })) return e;
  if (big_supported(c->p.model, c->p.k)) return prepare_big(c, 0, nullptr, nullptr, s);
  unsupported = true;
  return hipSuccess;
}

// fia_prepare_for: the entities referenced by a query set, users [0, U) and items [U, U + I) of
// c->mark.  Small k builds only their Gram caches (NCF: and per-position rows) from the marks on
// the device (no host round trip), and the cover check of later fia_count_related calls reads
// the same marks; large k (bigk.hip) numbers its cache slots from them on the host.
__global__ void k_mark(int64_t Q, const int32_t* __restrict__ qu, const int32_t* __restrict__ qi, int64_t U,
                       int64_t I, uint8_t* __restrict__ mark) {
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < Q; q += (int64_t)gridDim.x * blockDim.x) {
    const int32_t u = qu[q], i = qi[q];
    if (u >= 0 && u < U && i >= 0 && i < I) {
      mark[u] = 1;
      mark[U + i] = 1;
    }
  }
}

hipError_t mark_entities(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, hipStream_t s) {
  const int64_t U = c->p.U, I = c->p.I;
  FIA_HIP_TRY(c->mark.reserve((size_t)(U + I), s));
  FIA_HIP_TRY(hipMemsetAsync(c->mark.ptr, 0, (size_t)(U + I), s));
  if (Q > 0) {
    const int64_t gq = (Q + 255) / 256;
    hipLaunchKernelGGL(k_mark, dim3((unsigned)(gq < 4096 ? gq : 4096)), dim3(256), 0, s, Q, qu, qi, U, I,
                       c->mark.as<uint8_t>());
    FIA_HIP_TRY(hipGetLastError());
  }
  return hipSuccess;
}

__global__ void k_check_mark(int64_t Q, const int32_t* __restrict__ qu, const int32_t* __restrict__ qi, int64_t U,
                             int64_t I, const uint8_t* __restrict__ mark, int32_t* __restrict__ flag) {
  int bad = 0;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < Q; q += (int64_t)gridDim.x * blockDim.x) {
    const int32_t u = qu[q], i = qi[q];
    if (u >= 0 && u < U && i >= 0 && i < I) bad |= !mark[u] || !mark[U + i];
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

hipError_t prepare_model_for(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, hipStream_t s, hipStream_t ps,
                             bool& unsupported, bool mark_only) {
  unsupported = false;
  if (mark_only) {
    FIA_HIP_TRY(mark_entities(c, Q, qu, qi, s));
    c->subset = false;
    c->small_subset = false;
    return hipSuccess;
  }
  hipError_t e = hipSuccess;
  unsupported = !dispatch_small(c->p.model, c->p.k,
                                [&](auto m) { e = prepare_impl<decltype(m)>(c, ps, c->mark.as<uint8_t>()); });
  if (!unsupported && e == hipSuccess) c->small_subset = true;
  return e;
}

hipError_t check_cover_small(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, int32_t* flag,
                             hipStream_t s) {
  if (!c->small_subset || Q <= 0) return hipSuccess;
  const int64_t gq = (Q + 255) / 256;
  hipLaunchKernelGGL(k_check_mark, dim3((unsigned)(gq < 4096 ? gq : 4096)), dim3(256), 0, s, Q, qu, qi, c->p.U, c->p.I,
                     c->mark.as<uint8_t>(), flag);
  return hipGetLastError();
}

hipError_t query_model(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                       int64_t max_chunks, int32_t* rel_idx, double* influence, double* x_out, int K,
                       int64_t* topk_pos, int64_t* topk_idx, double* topk_val, hipStream_t s, bool& unsupported,
                       const double* x_in) {
  unsupported = false;
  hipError_t e = hipSuccess;
  if (dispatch_small(c->p.model, c->p.k, [&](auto m) {
        e = query_impl<decltype(m)>(c, Q, qu, qi, offsets, max_chunks, rel_idx, influence, x_out, K, topk_pos,
                                    topk_idx, topk_val, s, x_in);
      }))
    return e;
  if (big_supported(c->p.model, c->p.k))
    return query_big(c, Q, qu, qi, offsets, max_chunks, rel_idx, influence, x_out, K, topk_pos, topk_idx, topk_val,
                     s, x_in);
  unsupported = true;
  return hipSuccess;
}

}  // namespace fia
