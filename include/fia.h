/*
 * fia.h — C ABI of the MI355X-native FIA (fast influence analysis) library.
 *
 * One shared library (libfia.so, gfx950) replaces the TensorFlow/scipy steps
 * of the reference's per-test-rating influence path:
 *
 *   reference (zz9tf/FIA-KDD-19, src/influence/)        replaced by
 *   -------------------------------------------------   ------------------------
 *   MF.__init__ / NCF.__init__ variables                 fia_set_params
 *     (matrix_factorization.py:89-116, NCF.py:102-145)
 *   DataSet train.x scanned per query                    fia_build_index (once)
 *     (dataset.py:14, matrix_factorization.py:320-321)
 *   get_train_indices_of_test_case                       fia_count_related + fia_related
 *     (matrix_factorization.py:315-322, NCF.py:344-351)
 *   hessian_vector_product_test + minibatch_hessian_     fia_prepare (entity Gram caches)
 *     vector_val (mf:288-308, 324-351; ncf:317-380)       + fia_query_batch (assembly)
 *   get_inverse_hvp -> get_inverse_hvp_cg / fmin_ncg     fia_query_batch (exact fp64 LDL^T)
 *     (genericNeuralNet.py:503-508, mf:419-433, ncf:448-462)
 *   scoring loop of get_influence_on_test_loss           fia_query_batch (influence)
 *     (mf:237-246, ncf:266-274)
 *   top-K of experiments.test_retraining                 fia_query_batch (top-K)
 *     (experiments.py:46-48)
 *   phantom-point branch of get_influence_on_test_loss   fia_score_candidates
 *     (train_idx None, X / Y given: mf:228-235, and the
 *      same branch of NCF.py)
 *   (none: get_influence_on_test_loss asserts            fia_total_influence
 *     len(test_indices) == 1, mf:179 -- the influence of
 *     every train row on a SET of predictions)
 *   (none: one row at a time is scored, mf:237-246 --    fia_group_influence
 *     the effect of removing a SET of train rows)
 *   (none: one test point per call, mf:179 -- every      fia_self_influence
 *     train row's effect on its OWN prediction, the
 *     leverage scan for suspicious ratings)
 *   (none: one test point per call, mf:179 -- which     fia_count_related_pair + fia_pair_batch
 *     ratings put item i above item j for a user, the
 *     influence on r-hat(u, i) - r-hat(u, j))
 *   (none: one test point per call, mf:179 -- which     fia_count_related_slate + fia_slate_batch
 *     ratings shape a user's ranked list, the influence
 *     on sum_l w_l r-hat(u, i_l))
 *
 * Conventions
 *   - All array arguments are DEVICE pointers owned by the caller (PyTorch).
 *     The context owns only its index, caches and scratch.
 *   - Every call is ordered on `stream` (a hipStream_t passed as void*; NULL =
 *     the null stream).  Use one stream per context.  A context is not
 *     thread-safe; use one context per GPU / process.  A call on a new stream first
 *     synchronises the previous one -- except when the new stream is being captured
 *     into a HIP graph (no synchronisation is legal there): finish the previous
 *     stream's work (e.g. an eager warm-up) before the capture begins.  An eager
 *     fia_prepare / fia_prepare_for may run its Gram pass on the context's own aux
 *     stream, joined by the next fia_query_batch / fia_prepare; a capture may only
 *     start once that join has happened (the aux stream is idle to the capture):
 *     otherwise the first call on the capturing stream returns FIA_ERR_STATE.
 *   - Every entry point returns FIA_OK (0) or an error code; no exception
 *     crosses the ABI.  fia_last_error() describes the last failure.
 *   - Ids are int32 in [0, num_users) / [0, num_items); ratings are float32.
 *   - Parameters are float32 device tables in the reference's flat layout.
 *     The math (Hessian assembly, solve, scoring) runs in fp64.
 */
#ifndef FIA_H_
#define FIA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FIA_OK 0
#define FIA_ERR_INVALID 1      /* bad argument (null pointer, size, id range)   */
#define FIA_ERR_HIP 2          /* HIP runtime error                             */
#define FIA_ERR_STATE 3        /* call order: params/index/prepare missing      */
#define FIA_ERR_UNSUPPORTED 4  /* model / embedding size not built into library */
#define FIA_ERR_NOMEM 5

#define FIA_MODEL_MF 0
#define FIA_MODEL_NCF 1

#define FIA_MAX_TOPK 64

typedef struct fia_ctx fia_ctx;

/* Library version (major*10000 + minor*100 + patch). */
int fia_version(void);

/* Create a context bound to HIP device `device`. */
int fia_create(int device, fia_ctx** out);
/* Waits for the context's own work (its aux stream and the stream of its last call, not the
 * whole device), frees its buffers in order on that stream and destroys it. */
int fia_destroy(fia_ctx* ctx);
/* Message of the last failing call on ctx ("" if none).  ctx may be NULL. */
const char* fia_last_error(const fia_ctx* ctx);

/* Register the model parameters (device float32 tables, kept by pointer).
 *   MF  (matrix_factorization.py:30-36), nptrs = 5:
 *     [0] embedding_users [U*k]  [1] embedding_items [I*k]
 *     [2] bias_users [U]         [3] bias_items [I]        [4] global_bias [1]
 *   NCF (NCF.py:29-41, 85-145), nptrs = 10:
 *     [0] mlp/embedding_users [U*k]  [1] mlp/embedding_items [I*k]
 *     [2] gmf/embedding_users [U*k]  [3] gmf/embedding_items [I*k]
 *     [4] h1/weights [2k*k] [5] h1/biases [k] [6] h2/weights [k*k/2]
 *     [7] h2/biases [k/2]  [8] h3/weights [3k/2] [9] h3/biases [1]
 * weight_decay: the reference's wd (variable_with_weight_decay,
 * genericNeuralNet.py:40-65); damping: lambda added to every HVP (mf:306). */
int fia_set_params(fia_ctx* ctx, int model, int k, int64_t num_users, int64_t num_items,
                   const float* const* tables, int nptrs, double weight_decay, double damping);

/* Build the user-major (CSR) and item-major (CSC) rating index from the
 * training ratings (row j = (user[j], item[j], rating[j])).  Inside a user's
 * or an item's list rows keep ascending train-row order, so the related set of
 * (u,i) is exactly np.where(x[:,0]==u) ++ np.where(x[:,1]==i) (mf:320-322).
 * Synchronises `stream` (one-time setup). */
int fia_build_index(fia_ctx* ctx, int64_t n_train, int64_t num_users, int64_t num_items,
                    const int32_t* user, const int32_t* item, const float* rating, void* stream);

/* Per-entity Hessian caches for the current params + index: for every user u
 * the Gram sum over R_u of the restricted prediction gradients, likewise for
 * every item (the rank-1 updates of H_t).  Call after set_params/build_index
 * and again whenever the parameter VALUES change.
 * Ordering: the caches are ready for every later call on the context.  For small k
 * (except MF k <= 16) the pass runs on the context's own stream, forked from `stream`, and
 * the next fia_* call on the context joins it (the query-side scans of fia_query_batch
 * overlap it); until then it still READS the parameter tables and the index, so keep the
 * tables alive and unchanged until the next call on the context -- fia_set_params (which
 * waits for the pass on the host), fia_build_index, fia_prepare*, fia_query_batch* or
 * fia_destroy -- rather than only until `stream` is synchronised. */
int fia_prepare(fia_ctx* ctx, void* stream);

/* Like fia_prepare, but the per-entity caches are built only for the users and items
 * referenced by the Q queries (q_user / q_item, device int32): one GPU's query shard needs
 * its own users and items, not the whole table.  Later fia_count_related calls (with
 * total_out) reject queries outside that set (FIA_ERR_STATE).
 *   large k (MF k >= 128, NCF k >= 64): compacted caches (20M ratings, NCF k=256: 1 MB per
 *     entity); synchronises `stream` (the cache size is decided on the host);
 *   small k: the entities are marked on the device and only their caches are computed (the
 *     layout stays dense); stream-ordered, no synchronisation.
 * Results for covered queries are bitwise identical to those after fia_prepare. */
int fia_prepare_for(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user, const int32_t* q_item, void* stream);

/* offsets[q] = sum_{q'<q} n_q', offsets[Q] = total, with n_q = |R_u| + |C_i|
 * (device int64[Q+1]).  If total_out is non-NULL the total is copied to the
 * host and the stream is synchronised; out-of-range query ids are then
 * reported as FIA_ERR_INVALID. */
int fia_count_related(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user, const int32_t* q_item,
                      int64_t* offsets, int64_t* total_out, void* stream);

/* rel_idx[offsets[q] + p] = p-th train row of the related list of query q (device
 * int32: fia_build_index limits n_train to < 2^31, so every train row fits; the reference's
 * np.where gives int64 -- the Python facade widens on the copy to the host, and the
 * device writes 4 B instead of 8 B per related rating). */
int fia_related(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user, const int32_t* q_item,
                const int64_t* offsets, int32_t* rel_idx, void* stream);

/* Batched FIA: for every query q = (q_user[q], q_item[q]):
 *   H_t x = v solved exactly (fp64 LDL^T), then for every related rating p:
 *   influence[offsets[q]+p] = x . grad L_p / n_q   (mf:237-246),
 *   rel_idx[offsets[q]+p]   = its train row (int32, see fia_related).
 * x_out (nullable): device double[Q * D] in the reference theta order
 *   (MF [p_u, q_i, b_u, b_i], D = 2k+2; NCF [Pm_u, Qm_i, Pg_u, Qg_i], D = 4k).
 * rel_idx / influence may be NULL to skip writing the full vectors.
 * topk (K in [0, FIA_MAX_TOPK]; 0 = off): per query the K related ratings of
 * largest |influence| (ties: lower related position first), as related
 * position (topk_pos), train row (topk_idx) and signed influence (topk_val),
 * device arrays [Q*K]; unused slots hold -1 / NaN (n_q < K).
 * total_rel must equal offsets[Q].  Queries with n_q = 0 produce no ratings
 * and a NaN x (TF's mean over an empty batch).
 * Batch limit, MF k in {32, 64} with K <= 1 (the matrix-core scoring kernel keeps 32-bit
 * element offsets and candidate slots): total_rel <= FIA_MFMA_MAX_TOTAL_REL (2^32) and
 * 2 * num_queries + total_rel / 256 <= FIA_MFMA_MAX_CHUNKS (2^31 - 1); a larger batch is
 * refused with FIA_ERR_INVALID before anything is reserved or launched -- split it.
 * rel_idx / influence need only their types' natural alignment (4 B / 8 B): every scoring
 * kernel stores per element, whatever the base pointers' offset within a cache line. */
#define FIA_MFMA_MAX_TOTAL_REL (1LL << 32)
#define FIA_MFMA_MAX_CHUNKS ((1LL << 31) - 1)
int fia_query_batch(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user, const int32_t* q_item,
                    const int64_t* offsets, int64_t total_rel,
                    int32_t* rel_idx, double* influence, double* x_out,
                    int K, int64_t* topk_pos, int64_t* topk_idx, double* topk_val, void* stream);

/* fia_query_batch with a GIVEN inverse HVP instead of the solve: x_in (device double[Q * D],
 * the reference theta order, as fia_query_batch's x_out) replaces H_t^-1 v; the related sets,
 * influence and top-K follow from it exactly as in fia_query_batch.  Replaces the reference's
 * cached-inverse-HVP branch of get_influence_on_test_loss (force_refresh=False and an existing
 * <model>-cg-normal_loss-test-[t].npz, matrix_factorization.py:210-214).  Every built model:
 * small k records from x directly (k_record_x); large k (MF k >= 128, NCF k >= 64) skips the
 * batched LDL^T panels and writes the padded solution and records from x (k_big_record_x). */
int fia_query_batch_x(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user, const int32_t* q_item,
                      const int64_t* offsets, int64_t total_rel, const double* x_in,
                      int32_t* rel_idx, double* influence,
                      int K, int64_t* topk_pos, int64_t* topk_idx, double* topk_val, void* stream);

/* Influence of HYPOTHETICAL ratings on each query's prediction: the reference's phantom-point
 * branch (train_idx None, X / Y given: matrix_factorization.py:228-235, NCF.py likewise), which
 * cannot run there (it dots the restricted inverse HVP with a full-parameter gradient) and is
 * defined here.  Query q = (q_user[q], q_item[q]) has n_q = |R_u| + |C_i| from the built index
 * (read on the device: no related offsets are passed) and the inverse HVP x_q = x[q*D .. ) in the
 * reference theta order (fia_query_batch's x_out, or any given vector).  Its candidates are
 * c in [cand_offsets[q], cand_offsets[q+1]): (a, b, y) = (cand_user[c], cand_item[c],
 * cand_rating[c]); a candidate need not be a train row and need not share u or i.
 *   e_c    = r-hat(a, b) - y                         (current parameters, fp64)
 *   g_c    = d r-hat(a, b) / d theta_t               user-side blocks zero unless a == u,
 *                                                    item-side blocks zero unless b == i
 *   influence[c] = x_q . (2 e_c g_c + wd * M * theta_t) / n_q
 * with M = [1]*2k + [0, 0] (MF) or all ones (NCF): the expression fia_query_batch scores a
 * related rating with, the train row replaced by the candidate.  The divisor is the query's n_q
 * (not the reference branch's num_train_examples), so a candidate equal to a related train row
 * (u_j, i_j, y_j) gets that row's influence.  A candidate sharing neither u nor i scores the
 * constant x_q . (wd * M * theta_t) / n_q; n_q = 0 gives NaN (x is NaN); duplicates are allowed
 * and score identically.  A candidate id outside [0, num_users) x [0, num_items) is never used
 * as an index: that candidate scores NaN.
 * topk (K in [0, FIA_MAX_TOPK]; 0 = off): per query the K candidates of largest |influence| in
 * fia_query_batch's order (ties: lower position first, NaN last) as position inside the query's
 * candidate list (topk_pos) and signed influence (topk_val), device arrays [Q*K]; unused slots
 * hold -1 / NaN.  There is no topk_idx: a candidate has no train row.  influence may be NULL
 * (with K > 0 only the top-K is written).  The result does not depend on how the lists are cut
 * into work items.
 * Needs params, index and a prepare (else FIA_ERR_STATE).  After fia_prepare_for the QUERIES
 * must be covered (their x came from a covered query); candidate entities may be any in-range
 * id, and the results are bitwise those after fia_prepare.  Ordered on `stream`, no host
 * synchronisation; of a pending small-k Gram pass it waits only for the NCF layer-1 rows.
 * cand_offsets[0] == 0, non-decreasing, cand_offsets[Q] == total_cand.
 * Batch limit: total_cand <= FIA_CAND_MAX_TOTAL (2^31 - 1; the top-K selection keeps a
 * candidate's position in 32 bits, element offsets are 64-bit): a larger batch is refused with
 * FIA_ERR_INVALID before anything is reserved or launched -- split it.  num_queries == 0
 * returns FIA_OK and launches nothing. */
#define FIA_CAND_MAX_TOTAL ((1LL << 31) - 1)
int fia_score_candidates(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user, const int32_t* q_item,
                         const double* x,                 /* device [Q*D], reference theta order          */
                         const int64_t* cand_offsets,     /* device [Q+1], cand_offsets[0] == 0           */
                         int64_t total_cand,              /* == cand_offsets[Q]                           */
                         const int32_t* cand_user, const int32_t* cand_item, const float* cand_rating,
                         double* influence,               /* device [total_cand], nullable                */
                         int K, int64_t* topk_pos, double* topk_val,   /* [Q*K], K in [0, FIA_MAX_TOPK]   */
                         void* stream);

/* Total influence of every TRAIN row on a batch of predictions.  The reference has no
 * counterpart: get_influence_on_test_loss asserts len(test_indices) == 1
 * (matrix_factorization.py:179).  For train row j = (a, b, y) and queries q = (u_q, i_q) with
 * inverse HVPs x_q = x[q*D .. ) (reference theta order, as fia_score_candidates):
 *   total[j] = sum_q m_q(j) * I_q(j)
 *   I_q(j)   = x_q . (2 e_j g_j + wd * M * theta_t(q)) / n_q    the value fia_query_batch_x writes
 *                                                               for row j in q's related list
 *   m_q(j)   = [a == u_q] + [b == i_q]                          how often j occurs in that list
 *                                                               (2: q's pair is row j's own pair)
 *   count[j] = sum_q m_q(j)
 * i.e. total is the scatter-add of fia_query_batch_x's influence by rel_idx, and count the
 * histogram of rel_idx -- computed without the related lists: I_q(j) is linear in x_q and the
 * gradient block that multiplies it depends on the train row only, so each user's and each
 * item's queries are summed first and every train row is scored once (O(Q D + N D)).
 *   - A row no query touches (count 0) gets exactly +0.0.
 *   - A query with n_q = 0 contributes nothing (its NaN x reaches no row); a query whose id is
 *     outside [0, num_users) x [0, num_items) contributes nothing and is never used as an index.
 *   - A non-finite x_q reaches only the rows that query touches.
 *   - x may be any vector: scaling x_q by w_q gives the weighted sum sum_q w_q m_q(j) I_q(j).
 * topk (K in [0, FIA_MAX_TOPK]; 0 = off): the K train rows of largest |total| among the rows
 * with count > 0, in fia_query_batch's order with the train row as position (|v| descending,
 * ties: lower train row first, NaN last), as train row (topk_idx) and signed total (topk_val),
 * device arrays [K]; unused slots hold -1 / NaN.  total and count may be NULL; with K == 0 too
 * the call is FIA_ERR_INVALID.
 * Needs params, index and a prepare (else FIA_ERR_STATE).  It reads only the parameter tables,
 * the index, the train-pair table and, NCF, the dense layer-1 rows, which every prepare writes
 * for all entities: after fia_prepare_for the results are bitwise those after fia_prepare,
 * whatever the cover.  Ordered on `stream`, no host synchronisation; of a pending small-k Gram
 * pass it waits only for the NCF layer-1 rows.  The same inputs give the same bits on every call:
 * no floating-point atomics, each entity's queries are summed in ascending query position.
 * Batch limit: num_queries <= FIA_TOTAL_MAX_QUERIES (2^30, so that count fits in 32 bits): a
 * larger batch is refused with FIA_ERR_INVALID before anything is reserved or launched -- split
 * it, totals add.  num_queries == 0 zeroes total and count, fills the top-K slots with -1 / NaN
 * and returns FIA_OK.  Every size fia_score_candidates is built for (MF and NCF,
 * k in {8, 16, 32, 64, 128, 256}); anything else is FIA_ERR_UNSUPPORTED. */
#define FIA_TOTAL_MAX_QUERIES (1LL << 30)
int fia_total_influence(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user, const int32_t* q_item,
                        const double* x,          /* device [Q*D], reference theta order, as fia_score_candidates */
                        double* total,            /* device [n_train], nullable                                  */
                        int32_t* count,           /* device [n_train], nullable                                  */
                        int K, int64_t* topk_idx, double* topk_val,   /* device [K], K in [0, FIA_MAX_TOPK]      */
                        void* stream);

/* Group removal influence: the predicted change of r-hat(u, i) when a SET of train rows is removed
 * together, with the curvature that leaves with them (one Newton step of the restricted objective
 * without those rows).  The reference has no counterpart: it scores one row at a time against the
 * Hessian of the full related set (matrix_factorization.py:179, 237-246), and the sum of those
 * scores under-predicts as the set grows -- H_t is a mean over only n_q related ratings.
 * Query q = (q_user[q], q_item[q]) has n = n_q related ratings (with multiplicity, from the built
 * index), theta_t in the reference order, v = d r-hat(u, i) / d theta_t and the assembled
 *   H = (2/n) sum_rel (g g^T + e d2 r-hat) + wd * M + damping * I        as fia_query_batch solves it,
 * M = [1]*2k + [0, 0] (MF) or all ones (NCF).  Its groups are g in [grp_offsets[q], grp_offsets[q+1]);
 * the members of group g are the train rows mem_row[mem_offsets[g] .. mem_offsets[g+1]).  For a
 * member j = (a, b, y):
 *   m_j = [a == u] + [b == i]      how often j occurs in q's related list (fia_total_influence's
 *                                  m_q(j): 2 for q's own pair, 0 for an unrelated row)
 *   e_j = r-hat(a, b) - y          (current parameters, fp64)
 *   g_j = d r-hat(a, b) / d theta_t   user-side blocks zero unless a == u, item-side unless b == i
 *   C_j = d2 r-hat / d theta_u d theta_i, nonzero only when a == u and b == i: MF I on the
 *         (p_u, q_i) cross block, NCF diag(W3g) on the (Pg_u, Qg_i) cross block
 *   H_S = (1/n) sum_{j in S} m_j (2 g_j g_j^T + 2 e_j C_j + wd * M)
 *   b_S = (1/n) sum_{j in S} m_j (2 e_j g_j + wd * M * theta_t)
 *   dtheta[g*D ..) = (H - H_S)^-1 b_S     exact fp64 LDL^T of the full coupled D x D system
 *   group[g]       = v . dtheta           predicted change of r-hat(u, i) when S is removed
 *   first_order[g] = (H^-1 v) . b_S       = sum_{j in S} m_j * (the influence fia_query_batch writes for j)
 * The normalisation stays 1 / n_q (removal is the -1/n up-weighting the influence uses), so with
 * H_S dropped group equals first_order.
 *   - An empty group, or one whose members all have m_j = 0, gives exactly +0.0 (group,
 *     first_order, every dtheta entry); a member with m_j = 0 changes no bit of the result.
 *   - A member listed twice is subtracted twice.
 *   - A member row outside [0, n_train) is never used as an index: that group scores NaN, other
 *     groups are unaffected.  n_q = 0, or a query id out of range (never used as an index), gives
 *     NaN for all of the query's groups.
 *   - If S removes every occurrence, H - H_S = damping * I and whatever the LDL^T gives is returned.
 *   - Members are accumulated in list order, no floating-point atomics: the same inputs give the
 *     same bits on every call, wherever the group and its query sit in the batch.
 * group, first_order and dtheta may each be NULL; all three NULL is FIA_ERR_INVALID.
 * grp_offsets[0] == 0, non-decreasing, grp_offsets[Q] == num_groups; mem_offsets likewise with
 * total_members.  Needs params, index and a prepare (else FIA_ERR_STATE).  After fia_prepare_for
 * the QUERIES must be covered, as for fia_query_batch; member rows may be any train row, and the
 * results are bitwise those after fia_prepare.  Ordered on `stream`, no host synchronisation; it
 * reads the entity Gram caches, so it joins a pending small-k Gram pass as fia_query_batch does
 * (and, like it, cannot start a capture before that join).  num_queries == 0 or num_groups == 0
 * returns FIA_OK and launches nothing.
 * Batch limit: num_groups <= FIA_GROUP_MAX_GROUPS and total_members <= FIA_GROUP_MAX_MEMBERS
 * (2^31 - 1 each): a larger batch is refused with FIA_ERR_INVALID before anything is reserved or
 * launched -- split it.
 * Sizes: every size fia_query_batch is built for.  MF k in {8, 16, 32, 64} and NCF k in {8, 16, 32}
 * keep the full packed system of a group in LDS.  The large-k models (MF k in {128, 256}, NCF k in
 * {64, 128, 256}) keep it in device memory: a group is two Gram-shaped downdates in the caches'
 * tile layout (2 * T (T + 1) / 2 * 256 doubles, T = ceil(side block / 16): 0.16 MB at MF k=128,
 * 2.2 MB at NCF k=256), four scalars and a right-hand side, solved by fia_query_batch's coupled
 * blocked LDL^T.  Those downdates are context scratch bounded at 1 GiB per launch: a longer batch
 * runs in chunks of groups on `stream`, still without host synchronisation, and the results do not
 * depend on the chunking.  There, after fia_prepare_for, the groups of a query outside the cover
 * score NaN (as its influences do in fia_query_batch; fia_count_related with a total is the call
 * that refuses such a batch): the members' residuals exist only for covered entities, and nothing
 * of such a group's members is read.  Any other size is FIA_ERR_UNSUPPORTED.
 * The environment variable FIA_BIGK_CHUNK (a positive integer) lowers the large-k chunk length of
 * this call and of fia_self_influence to that many systems per launch: a testing knob; a value
 * above the scratch-derived length is ignored.
 * fia_version stays 100 with these sizes added: no signature, struct or constant changed. */
#define FIA_GROUP_MAX_GROUPS ((1LL << 31) - 1)
#define FIA_GROUP_MAX_MEMBERS ((1LL << 31) - 1)
int fia_group_influence(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user, const int32_t* q_item,
                        const int64_t* grp_offsets,  /* device [Q+1]: groups of query q                */
                        int64_t num_groups,          /* == grp_offsets[Q]                              */
                        const int64_t* mem_offsets,  /* device [G+1]: members of group g               */
                        int64_t total_members,       /* == mem_offsets[G]                              */
                        const int32_t* mem_row,      /* device [total_members]: train rows             */
                        double* group,               /* device [G], nullable                           */
                        double* first_order,         /* device [G], nullable                           */
                        double* dtheta,              /* device [G*D], reference theta order, nullable  */
                        void* stream);

/* Newton-corrected influence of EVERY related rating of a batch of test predictions: what
 * fia_query_batch scores to first order -- each rating against the Hessian of the full related
 * list -- with the rating's own curvature taken out of the system.  H is a mean over only n_q
 * ratings; for a user with a few dozen ratings one rating is a few percent of it, and the
 * corrected and first-order values can differ by the size of the value itself.
 * Query q = (u, i), n = n_q.  Related position p holds train row j = rel[p] = (a, b, y), with m_j,
 * g_j, e_j, H_S, b_S, C and M as in fia_group_influence:
 *   newton[offsets[q] + p] = v . (H - H_{j})^-1 b_{j}
 * exactly the `group` output of fia_group_influence for query q and the group {j}.  A row that is
 * the query's own pair sits in the list twice (m_j = 2): both positions hold the same value, the
 * effect of removing that train row.  For m_j = 1 the first-order counterpart is fia_query_batch's
 * influence[offsets[q] + p].
 * Closed form for m_j = 1 (every row but the own pair; a == u and b == i together mean the own pair):
 *   H'  = H - (wd/n) * diag(M)            the same for every rating of the query
 *   c   = 2/n,  x' = H'^-1 v,  w' = H'^-1 (wd * M * theta_t) / n,  c' = x' . (wd * M * theta_t) / n
 *   s_j = x' . g_j,  t_j = w' . g_j,  h_j = g_j^T H'^-1 g_j
 *   newton_j = 2 e_j s_j / n + c' + c * s_j * (2 e_j h_j / n + t_j) / (1 - c * h_j)
 * one factorisation per query and a quadratic form per rating (g_j is nonzero in one side's block:
 * h_j needs that side's diagonal block of the FULL inverse H'^-1, coupled or not).  1 - c h_j can be
 * small and, for a coupled query (H indefinite through 2 e C), negative: nothing assumes its sign; a
 * zero denominator yields whatever the arithmetic yields (the system is singular there).  Own-pair
 * rows (m_j = 2: coupling block, twice the decay share -- not rank one) get the full downdated
 * solve of fia_self_influence's newton, one per such row, each with its own e_j.
 * Arguments as fia_query_batch (offsets from fia_count_related, total_rel == offsets[Q]); rel_idx
 * (int32 train rows, as fia_query_batch writes them) and newton may be NULL.  topk (K in
 * [0, FIA_MAX_TOPK]; 0 = off): per query the K related ratings of largest |newton| in
 * fia_query_batch's order (ties: lower related position first, NaN last) as related position
 * (topk_pos), train row (topk_idx) and signed value (topk_val), device arrays [Q*K]; unused slots
 * hold -1 / NaN.  A query with n_q = 0 writes nothing; a query id outside [0, num_users) x
 * [0, num_items) is never used as an index and counts as n_q = 0, as in fia_query_batch.
 * num_queries == 0 returns FIA_OK and launches nothing.
 * Needs params, index and a prepare (else FIA_ERR_STATE).  After fia_prepare_for the QUERIES must be
 * covered, and the results are bitwise those after fia_prepare.  Ordered on `stream`, no host
 * synchronisation; it reads the entity Gram caches, so it joins a pending small-k Gram pass as
 * fia_group_influence does.  No floating-point atomics: the same inputs give the same bits wherever
 * the query sits in the batch.
 * Scratch: 2 * Ds^2 + 4 * Ds + 4 doubles per query (Ds the side block, k + 1 or 2k: 68 KB at MF
 * k=64), bounded at 1 GiB per launch: a longer batch runs in chunks of queries on `stream`, and the
 * results do not depend on the chunking.  With newton NULL the own-pair values go to context scratch
 * (total_rel doubles).  The environment variable FIA_NEWTON_CHUNK (a positive integer) lowers the
 * chunk length to that many queries per launch: a testing knob; a larger value is ignored.
 * Sizes: MF k in {8, 16, 32, 64} and NCF k in {8, 16, 32}.  The large-k models (MF k in {128, 256},
 * NCF k in {64, 128, 256}) return FIA_ERR_UNSUPPORTED.  fia_version stays 100: no existing
 * signature, struct or constant changed. */
int fia_query_batch_newton(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user, const int32_t* q_item,
                           const int64_t* offsets, int64_t total_rel,
                           int32_t* rel_idx,         /* device [total_rel], nullable */
                           double* newton,           /* device [total_rel], nullable */
                           int K, int64_t* topk_pos, int64_t* topk_idx, double* topk_val,   /* device [Q*K] */
                           void* stream);

/* Newton-corrected influence of HYPOTHETICAL ratings: fia_score_candidates with the candidate's own
 * curvature in the system -- "what would this prediction do if the user rated b with y", one Newton
 * step of the objective WITH the rating instead of a first-order estimate.  What-if ratings are asked
 * for users with short histories, where one more rating is a large share of H (a mean over n_q
 * ratings) and the first-order value is furthest off.
 * Query q = (u, i), n = n_q; v, H, theta_t, M and C as in fia_group_influence.  Candidate
 * c = (a, b, y) with e_c and g_c as in fia_score_candidates (user-side blocks zero unless a == u,
 * item-side blocks zero unless b == i); both = (a == u and b == i):
 *   H_c = (1/n) (2 g_c g_c^T + 2 e_c C * [both] + wd * diag(M))
 *   b_c = (1/n) (2 e_c g_c + wd * M * theta_t)
 *   newton_add[c] = v . (H + H_c)^-1 b_c
 * The candidate counts once and the normalisation stays 1/n_q, as in fia_score_candidates and
 * fia_group_influence.  Dropping H_c gives exactly fia_score_candidates' influence[c], and the sign
 * convention is that call's: the Newton step's change of r-hat(u, i) after adding the rating is
 * -newton_add[c].
 * Closed form for every candidate that is not `both` (rank one plus a shift common to the query):
 *   H" = H + (wd/n) * diag(M),  c = 2/n,  x" = H"^-1 v,  w" = H"^-1 (wd * M * theta_t) / n,
 *   c" = x" . (wd * M * theta_t) / n
 *   s = x" . g_c,  t = w" . g_c,  h = g_c^T H"^-1 g_c
 *   newton_add = 2 e_c s / n + c" - c * s * (2 e_c h / n + t) / (1 + c * h)
 * one factorisation per query and a quadratic form per candidate.  1 + c h is negative for some
 * coupled queries (H indefinite through 2 e C): nothing assumes its sign; a zero denominator yields
 * whatever the arithmetic yields.  A candidate sharing neither side has g_c = 0 and scores c"; a
 * `both` candidate (g_c = v, and 2 e_c C is not rank one) gets one full solve of
 * H" + (2/n) v v^T + (2 e_c / n) C, as own-pair rows do in fia_query_batch_newton -- they are
 * expected to be few.
 * There is no x argument: the call factorises for itself (fia_query_batch's x belongs to another
 * system).  Arguments as fia_score_candidates: cand_offsets[0] == 0, non-decreasing,
 * cand_offsets[Q] == total_cand; total_cand <= FIA_CAND_MAX_TOTAL and num_queries <=
 * FIA_CAND_NEWTON_MAX_QUERIES (2^30: the partition's sort keys 2 q + side are 32-bit) are checked
 * before anything is reserved or launched; K in [0, FIA_MAX_TOPK] with non-NULL top-K arrays;
 * newton_add NULL with K == 0 is FIA_ERR_INVALID (no output requested); num_queries == 0 returns
 * FIA_OK and launches nothing.  A candidate id outside [0, num_users) x [0, num_items) is never used
 * as an index and scores NaN; a query with n_q = 0, or a query id out of range, gives NaN for all of
 * its candidates.  topk: per query the K candidates of largest |newton_add| in fia_query_batch's
 * order (ties: lower position first, NaN last) as position inside the query's candidate list
 * (topk_pos) and signed value (topk_val), device arrays [Q*K]; unused slots hold -1 / NaN.  With
 * newton_add NULL the values go to context scratch (total_cand doubles).
 * A candidate's value depends on (query, a, b, y) alone: no floating-point atomics, and the bits are
 * the same wherever the candidate sits in its list, wherever the query sits in the batch, whatever
 * else is listed and however the batch is cut into launches.
 * Needs params, index and a prepare (else FIA_ERR_STATE).  After fia_prepare_for the QUERIES must be
 * covered; candidate entities may be any in-range id, and the results are bitwise those after
 * fia_prepare.  Ordered on `stream`, no host synchronisation; it reads the entity Gram caches, so it
 * joins a pending small-k Gram pass as fia_query_batch_newton does.
 * Scratch: fia_query_batch_newton's record per query, bounded at 1 GiB per launch (a longer batch
 * runs in chunks of queries; FIA_NEWTON_CHUNK lowers the chunk here too), and 16 bytes per candidate
 * for the partition by (query, side).
 * Sizes: MF k in {8, 16, 32, 64} and NCF k in {8, 16, 32}.  The large-k models return
 * FIA_ERR_UNSUPPORTED.  Phases (fia_set_profiling): 1 the per-query records, 4 the partition,
 * 2 the scoring, 0 the `both` solves, 3 the top-K.  fia_version stays 100: no existing signature,
 * struct or constant changed. */
#define FIA_CAND_NEWTON_MAX_QUERIES (1LL << 30)
int fia_score_candidates_newton(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user, const int32_t* q_item,
                                const int64_t* cand_offsets,     /* device [Q+1], cand_offsets[0] == 0 */
                                int64_t total_cand,              /* == cand_offsets[Q]                 */
                                const int32_t* cand_user, const int32_t* cand_item, const float* cand_rating,
                                double* newton_add,              /* device [total_cand], nullable      */
                                int K, int64_t* topk_pos, double* topk_val,   /* device [Q*K]          */
                                void* stream);

/* Self-influence: the effect of a train rating on its OWN prediction (its leverage), for every
 * listed train row in one fused pass -- the scan that finds noisy or injected ratings, and what
 * turns a leave-one-out residual into a Cook's-distance style score.  The reference has no
 * counterpart: it scores one test point per call (matrix_factorization.py:179).
 * For position p with train row j = rows[p] = (a, b, y) the query is (a, b):
 *   n       = |R_a| + |C_b| >= 2, theta_t, v = d r-hat(a, b) / d theta_t and the assembled H exactly
 *             as fia_query_batch builds them; M and C as in fia_group_influence
 *   e       = r-hat(a, b) - y
 *   b_j     = (2/n) (2 e v + wd * M * theta_t)          row j occurs twice in its own related list: m_j = 2
 *   H_j     = (2/n) (2 v v^T + 2 e C + wd * M)
 *   first_order[p] = (H^-1 v) . b_j        the sum of the two influences fia_query_batch writes for j
 *   newton[p]      = v . (H - H_j)^-1 b_j  one Newton step of the objective without row j: the
 *                                          predicted change of r-hat(a, b) when the rating is removed
 *   error[p]       = e
 * This equals fia_group_influence for query (a, b) with the single group {j} (its first_order and
 * group outputs; see the definitions there), without the index arrays, the second prologue and the
 * Q * D scratch that call needs for it.  A pair present c times in train gives each of its rows
 * m = 2 and its own y.  Rows are independent of one another; the same row listed twice in rows
 * scores identically.
 *   - A row outside [0, n_train) is never used as an index: its three outputs are NaN, its
 *     neighbours are unaffected.
 *   - No floating-point atomics: the same inputs give the same bits, wherever the row sits in rows
 *     and whatever else is in the batch.
 * topk (K in [0, FIA_MAX_TOPK]; 0 = off): the K positions of largest |newton| in fia_query_batch's
 * order (|v| descending, ties: lower position first, NaN last), as position in rows (topk_pos),
 * train row (topk_idx: the entry of rows as given) and signed newton (topk_val), device arrays [K];
 * unused slots hold -1 / -1 / NaN.  It works with newton NULL (the values go to context scratch).
 * first_order, newton and error may each be NULL (a solve nobody asked for is skipped); all three
 * NULL with K == 0 is FIA_ERR_INVALID.  rows NULL means rows 0 .. n_train - 1, and then num_rows
 * must equal n_train.  num_rows == 0 returns FIA_OK and launches nothing but the fill of the top-K
 * slots.
 * Batch limit: num_rows <= FIA_SELF_MAX_ROWS (2^31 - 1: the top-K keeps a 32-bit position): a larger
 * batch is refused with FIA_ERR_INVALID before anything is reserved or launched -- split it.
 * Needs params, index and a full fia_prepare (else FIA_ERR_STATE): after fia_prepare_for the call
 * returns FIA_ERR_STATE -- a scan touches nearly every entity, a partial cover is the wrong tool.
 * Ordered on `stream`, no host synchronisation; it reads the entity Gram caches, so it joins a
 * pending small-k Gram pass as fia_group_influence does (and, like it, cannot start a capture
 * before that join).  Checks run in fia_group_influence's order: bounds, state, outputs, the empty
 * batch, nulls, support.
 * Sizes: those of fia_group_influence; anything else is FIA_ERR_UNSUPPORTED.  At the large-k sizes
 * (MF k in {128, 256}, NCF k in {64, 128, 256}) the rows run in chunks of 4096 on `stream` (the
 * per-row work words, 8 + 4 * padded side block doubles, and the solutions of a chunk are context
 * scratch: 100 MB at NCF k=256); a row's own downdate needs no slab, error comes from the
 * residuals fia_prepare keeps per train row, and the results do not depend on the chunking. */
#define FIA_SELF_MAX_ROWS ((1LL << 31) - 1)
int fia_self_influence(fia_ctx* ctx,
                       int64_t num_rows,
                       const int32_t* rows,      /* device [num_rows] train rows; NULL = rows 0 .. n_train-1,
                                                    and then num_rows must equal n_train                    */
                       double* first_order,      /* device [num_rows], nullable */
                       double* newton,           /* device [num_rows], nullable */
                       double* error,            /* device [num_rows], nullable */
                       int K, int64_t* topk_pos, int64_t* topk_idx, double* topk_val,   /* device [K] */
                       void* stream);

/* Edit sets: the joint Newton effect on a prediction of train rows REMOVED and hypothetical ratings
 * ADDED together -- "what if this user had rated X with 5 instead of 1" (one removal and one
 * addition on the same pair), "what if a new user answers these five items", "what do these twenty
 * injected ratings do together".  None of these is a sum of fia_group_influence and
 * fia_score_candidates_newton outputs: every call solves a system of its own, and (H - H_R)^-1 b_R
 * and (H + H_c)^-1 b_c do not combine.
 * Query q = (u, i), n = n_q; v, H, theta_t, M, C and, for a train row j, m_j, e_j, g_j as in
 * fia_group_influence; for an added triple c = (a, b, y), e_c and g_c as in
 * fia_score_candidates_newton (user-side blocks zero unless a == u, item-side blocks zero unless
 * b == i; both = (a == u and b == i)).  The groups of query q are g in [grp_offsets[q],
 * grp_offsets[q+1]); group g has two member lists, the removals R = rem_row[rem_offsets[g] ..
 * rem_offsets[g+1]) (train rows) and the additions A = entries [add_offsets[g] .. add_offsets[g+1])
 * of add_user / add_item / add_rating:
 *   H_R = (1/n) sum_{j in R} m_j (2 g_j g_j^T + 2 e_j C_j + wd * M)
 *   b_R = (1/n) sum_{j in R} m_j (2 e_j g_j + wd * M * theta_t)
 *   H_A = (1/n) sum_{c in A} (2 g_c g_c^T + 2 e_c C * [both] + wd * diag(M))
 *   b_A = (1/n) sum_{c in A} (2 e_c g_c + wd * M * theta_t)
 *   dtheta[g*D ..) = (H - H_R + H_A)^-1 (b_R - b_A)     exact fp64 LDL^T of the full coupled system
 *   edit[g]        = v . dtheta       predicted change of r-hat(u, i) once R is removed and A is added
 *   first_order[g] = (H^-1 v) . (b_R - b_A)
 * An addition counts once and the normalisation stays 1/n_q, exactly as in
 * fia_score_candidates_newton.  With A empty edit is fia_group_influence's group; with R empty and
 * A = {c} it is -newton_add[c]; with H_R and H_A dropped it is first_order.
 *   - Members are accumulated removals first, then additions, each in list order.  No floating-point
 *     atomics: the bits depend on (query, the two lists) alone -- the same on every call, wherever
 *     the group sits in its query and the query in the batch.
 *   - A removed row with m_j = 0 changes no bit of the result (as in fia_group_influence).  An
 *     addition sharing neither side has g_c = 0 and adds wd * diag(M) / n to the system and
 *     wd * M * theta_t / n to b_A, as fia_score_candidates_newton scores c" for it.
 *   - A group with no removal of m_j > 0 and no addition at all writes exactly +0.0 (edit,
 *     first_order, every dtheta entry) without solving.
 *   - A member listed twice is taken twice.
 *   - A removal row outside [0, n_train), or an added id outside [0, num_users) x [0, num_items), is
 *     never used as an index: that group is NaN, its neighbours are untouched.  n_q = 0, or a query
 *     id out of range (never used as an index), gives NaN for all of the query's groups.
 * edit, first_order and dtheta (reference theta order) may each be NULL.  topk (K in
 * [0, FIA_MAX_TOPK]; 0 = off): per query the K groups of largest |edit| in fia_query_batch's order
 * (|v| descending, ties: lower position first, NaN last) as the group's position inside its query
 * (topk_pos) and signed value (topk_val), device arrays [Q*K]; unused slots hold -1 / NaN.  With edit
 * NULL the values go to context scratch (num_groups doubles).  All three outputs NULL with K == 0 is
 * FIA_ERR_INVALID.
 * grp_offsets[0] == 0, non-decreasing, grp_offsets[Q] == num_groups; rem_offsets and add_offsets
 * [G+1] likewise with total_rem and total_add.  num_groups <= FIA_EDIT_MAX_GROUPS, total_rem and
 * total_add <= FIA_EDIT_MAX_MEMBERS (2^31 - 1 each): a larger batch is refused with FIA_ERR_INVALID
 * before anything is reserved or launched -- split it.  num_queries == 0, or num_groups == 0 with
 * K == 0, returns FIA_OK and launches nothing.
 * Needs params, index and a prepare (else FIA_ERR_STATE).  After fia_prepare_for only the QUERIES
 * must be covered: members are read from the parameter tables and the dense NCF layer-1 rows, which
 * every prepare writes for all entities, and the results are bitwise those after fia_prepare.
 * Ordered on `stream`, no host synchronisation; it reads the entity Gram caches, so it joins a
 * pending small-k Gram pass as fia_group_influence does.
 * Sizes: MF k in {8, 16, 32, 64} and NCF k in {8, 16, 32} (the full packed system of a group in
 * LDS).  The large-k models (MF k in {128, 256}, NCF k in {64, 128, 256}) return
 * FIA_ERR_UNSUPPORTED: they are the follow-up, as fia_group_influence's device-memory systems were
 * to its first version.  Phases (fia_set_profiling): 1 the solves, 3 the top-K.  fia_version stays
 * 100: no existing signature, struct or constant changed. */
#define FIA_EDIT_MAX_GROUPS ((1LL << 31) - 1)
#define FIA_EDIT_MAX_MEMBERS ((1LL << 31) - 1)
int fia_edit_influence(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user, const int32_t* q_item,
                       const int64_t* grp_offsets,  /* device [Q+1]: groups of query q                */
                       int64_t num_groups,          /* == grp_offsets[Q]                              */
                       const int64_t* rem_offsets,  /* device [G+1]: removals of group g              */
                       int64_t total_rem,           /* == rem_offsets[G]                              */
                       const int32_t* rem_row,      /* device [total_rem]: train rows                 */
                       const int64_t* add_offsets,  /* device [G+1]: additions of group g             */
                       int64_t total_add,           /* == add_offsets[G]                              */
                       const int32_t* add_user, const int32_t* add_item, const float* add_rating,
                       double* edit,                /* device [G], nullable                           */
                       double* first_order,         /* device [G], nullable                           */
                       double* dtheta,              /* device [G*D], reference theta order, nullable  */
                       int K, int64_t* topk_pos, double* topk_val,   /* device [Q*K]                  */
                       void* stream);

/* Pair queries: which ratings put item i ABOVE item j for a user.  A recommender shows an order, and
 * what decides it is the gap d = r-hat(u, i) - r-hat(u, j).  Subtracting two fia_query_batch results
 * is not FIA's answer for d: the two calls restrict to different parameter sets, use different
 * related lists and normalisations, and each re-solves the shared user block against one item only.
 * The reference has no counterpart (one test point per call, matrix_factorization.py:179).
 * Pair query q = (u, i, j) = (q_user[q], q_item_i[q], q_item_j[q]), i != j.  Side block size
 * Ds = k + 1 (MF) or 2k (NCF), D3 = 3 * Ds.
 *   theta_t = (theta_u, theta_i, theta_j): MF (p_u, b_u), (q_i, b_i), (q_j, b_j); NCF (Pm_u, Pg_u),
 *             (Qm_i, Qg_i), (Qm_j, Qg_j)
 *   rel     = where(user == u) ++ where(item == i) ++ where(item == j), each in ascending train-row
 *             order; n = |R_u| + |C_i| + |C_j|.  A train row (u, i) or (u, j) sits in rel twice; no
 *             row sits three times.
 *   For position p with train row (a, b, y): e_p = r-hat(a, b) - y and g_p = d r-hat(a, b) / d theta_t,
 *             whose user block is zero unless a == u, whose i block unless b == i and whose j block
 *             unless b == j -- whichever list the position is in, as fia_query_batch treats the own pair.
 *   H       = (2/n) sum_p (g_p g_p^T + e_p d2 r-hat_p) + wd * diag(M) + damping * I, M as in
 *             fia_group_influence; d2 r-hat is nonzero only for own-pair rows: MF I on the (p_u, q_i)
 *             cross block for (u, i) and on the (p_u, q_j) cross block for (u, j), NCF diag(W3g) on the
 *             (Pg_u, Qg_i) and (Pg_u, Qg_j) cross blocks.  From the caches, with v^i = d r-hat(u, i) /
 *             d (theta_u, theta_i), v^j likewise, A_u / B_i / B_j the entity Grams and (cd, es) = (rows of
 *             the pair in train, the sum of their residuals):
 *               H_uu = (2/n) (A_u + cd_i v^i_u v^i_u^T + cd_j v^j_u v^j_u^T)
 *               H_ii = (2/n) (B_i + cd_i v^i_i v^i_i^T)            H_jj likewise
 *               H_iu = (2/n) 2 (cd_i v^i_i v^i_u^T + es_i C)       H_ju likewise       H_ij = 0
 *             plus the diagonal terms: block diagonal when neither pair is a train row.
 *   v       = d d / d theta_t = (v^i_u - v^j_u, v^i_i, -v^j_j)
 *   x       = H^-1 v: exact fp64 LDL^T, nothing assumed about a pivot's sign (coupling makes H indefinite)
 *   influence[offsets[q] + p] = x . (2 e_p g_p + wd * M * theta_t) / n     fia_query_batch's expression
 *   diff[q] = r-hat(u, i) - r-hat(u, j)                                    current parameters, fp64
 *   x_out [Q * D3]: the reference theta order, extended: MF [p_u, q_i, q_j, b_u, b_i, b_j],
 *             NCF [Pm_u, Qm_i, Qm_j, Pg_u, Qg_i, Qg_j]
 * topk (K in [0, FIA_MAX_TOPK]; 0 = off): per query, as fia_query_batch -- |value| descending, lower
 * related position first, NaN last -- as position in the pair's own related list (topk_pos), train row
 * (topk_idx) and signed value (topk_val), device arrays [Q*K]; unused slots hold -1 / -1 / NaN.
 *   - n = 0 writes no ratings, a NaN x and a NaN-free diff.
 *   - An id outside [0, num_users) x [0, num_items) is never used as an index and counts as n = 0; its
 *     diff is NaN.
 *   - i == j also counts as n = 0 (the two item blocks would be one parameter twice); its diff is +0.0.
 *   - No floating-point atomics: a query's bits do not depend on where it sits in the batch or on what
 *     else is in it.  (A query with a train-row pair takes one full-range LDL^T, one with none three
 *     block-range ones: the two routes are not claimed to agree bitwise, and a query never changes route.)
 * fia_count_related_pair: fia_count_related's contract for the pair list (offsets device int64 [Q+1];
 * with total_out the total is copied to the host, the stream synchronised, out-of-range ids reported as
 * FIA_ERR_INVALID, and a query whose u, i or j is outside a fia_prepare_for cover as FIA_ERR_STATE).
 * Without total_out, bad ids and i == j count zero.  Needs the index only.
 * fia_pair_batch: rel_idx (int32 train rows), influence, x_out and diff are each nullable; all four NULL
 * with K == 0 is FIA_ERR_INVALID.  total_rel must equal offsets[Q].  With influence NULL and K > 0
 * nothing of length total_rel is written.  num_queries == 0 returns FIA_OK and launches nothing.
 * Batch limit: total_rel <= FIA_PAIR_MAX_TOTAL_REL (2^31 - 1: the top-K keeps a 32-bit position) and
 * num_queries <= FIA_PAIR_MAX_QUERIES (2^30: two half records per query, indexed in 32 bits); a larger
 * batch is refused with FIA_ERR_INVALID before anything is reserved or launched -- split it.  Checks
 * run in fia_edit_influence's order: bounds, state, outputs, the empty batch, nulls, support.
 * Needs params, index and a prepare (else FIA_ERR_STATE).  After fia_prepare_for the cover must hold
 * u, i AND j of every query (fia_prepare_for with the pairs (u, i) and (u, j)); the results are then
 * bitwise those after fia_prepare.  Ordered on `stream`, no host synchronisation; it reads the entity
 * Gram caches, so it joins a pending small-k Gram pass as fia_group_influence does.  Stores are per
 * element: the outputs need only their types' natural alignment.
 * Sizes: MF k in {8, 16, 32} and NCF k in {8, 16} -- those whose packed D3 triangle (MF k=32: 4,950
 * doubles), vectors and staged NCF W1 fit one workgroup's LDS; MF k=64 would need 153 KB for the
 * triangle alone.  Every other size (MF k=64, NCF k=32, the large-k models) is FIA_ERR_UNSUPPORTED.
 * Phases (fia_set_profiling): 4 the count and scan (fia_count_related_pair) and the related rows,
 * 1 the solves, 2 the scoring, 3 the top-K.  fia_version stays 100: no existing signature, struct or
 * constant changed. */
#define FIA_PAIR_MAX_TOTAL_REL ((1LL << 31) - 1)
#define FIA_PAIR_MAX_QUERIES (1LL << 30)
int fia_count_related_pair(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user, const int32_t* q_item_i,
                           const int32_t* q_item_j, int64_t* offsets, int64_t* total_out, void* stream);
int fia_pair_batch(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user, const int32_t* q_item_i,
                   const int32_t* q_item_j,
                   const int64_t* offsets,         /* device [Q+1], from fia_count_related_pair */
                   int64_t total_rel,              /* == offsets[Q]                              */
                   int32_t* rel_idx,               /* device [total_rel], nullable               */
                   double* influence,              /* device [total_rel], nullable               */
                   double* x_out,                  /* device [Q*D3], nullable                    */
                   double* diff,                   /* device [Q], nullable                       */
                   int K, int64_t* topk_pos, int64_t* topk_idx, double* topk_val,   /* device [Q*K] */
                   void* stream);

/* Flip sets: the smallest set of the user's OWN ratings that puts item j above item i.  What people do
 * with fia_pair_batch's numbers is the counterfactual explanation -- "had you not rated these three
 * films, we would have shown you j instead of i" (ACCENT, Tran, Ghazimatin and Saha Roy, SIGIR 2021):
 * sort the user's ratings by their influence on the gap, take the shortest prefix whose summed
 * influence closes it.  That sum is first order, and first order is a poor guide for sets, so the call
 * also returns what the re-solved system says the set does.
 * Pair query q = (u, i, j); n, theta_t, M, H, v, x = H^-1 v, e_p, g_p and diff are exactly those of
 * fia_pair_batch.  margin[q] >= 0 is a device array [Q] and may be NULL, which means 0.  max_set is in
 * [1, FIA_FLIP_MAX_SET].
 *   eligible  position p of the user's list R_u (ascending train row) whose item is neither i nor j
 *             and whose val_p = x . (2 e_p g_p + wd * M * theta_t) / n -- the value fia_pair_batch
 *             writes at that position; g_p has the user block only -- is below 0 and not NaN
 *   order     val ascending, ties by lower list position
 *   set       rows taken in that order while the number taken is below max_set, an eligible row is
 *             left, and (diff + margin) + (running sum of the taken val) >= 0; the running sum is in
 *             selection order, sequential
 *   set_size[q]                 the number of rows taken
 *   set_row[q * max_set + t]    the train row of the t-th, set_val[q * max_set + t] its val; unused
 *                               slots hold -1 and NaN
 *   first_order[q]              that running sum, +0.0 for an empty set; "flipped to first order" reads
 *                               diff + first_order < -margin
 *   H_S = (1/n) sum_{z in S} (2 g_z g_z^T + wd * diag(M))      b_S = (1/n) sum_{z in S} (2 e_z g_z + wd * M * theta_t)
 *   dtheta[q * D3 ..) = (H - H_S)^-1 b_S    one exact fp64 LDL^T over the full range, nothing assumed about
 *                               a pivot's sign, in fia_pair_batch's extended reference order
 *   newton[q] = v . dtheta      the predicted change of the gap when S is removed; with H_S dropped it
 *                               equals first_order.  fia_group_influence's definition with m_j = 1 on
 *                               the three-block system.
 *   - An empty set gives exactly +0.0 for newton and every dtheta entry, without a solve: diff + margin
 *     < 0 already, no eligible row, or a user with no ratings but n > 0.
 *   - An id out of range (never used as an index), i == j, or n == 0: set_size -1 and NaN in every
 *     double output; diff is the exception and follows fia_pair_batch's rule (NaN / +0.0 / the gap).
 *   - No floating-point atomics: a query's bits depend on (u, i, j, margin, max_set) alone; the set of a
 *     smaller max_set is a prefix of the set of a larger one.  The result does not depend on how the
 *     user's list is cut into tiles.
 * Every output is nullable; all NULL is FIA_ERR_INVALID.  num_queries <= FIA_PAIR_MAX_QUERIES; checks
 * run in fia_pair_batch's order: bounds (num_queries, max_set), state, outputs, the empty batch, nulls,
 * support.  No count call and no offsets: nothing of length total_rel exists in this call, and the
 * item lists C_i, C_j are never read by the selection.  Needs params, index and a prepare; after
 * fia_prepare_for the cover must hold u, i and j, and the results are then bitwise those after
 * fia_prepare.  Ordered on `stream`, no host synchronisation; it joins a pending small-k Gram pass.
 * Sizes: fia_pair_batch's, MF k in {8, 16, 32} and NCF k in {8, 16}; every other size is
 * FIA_ERR_UNSUPPORTED.  Phases: 1 the solves, 2 the selection, 3 the re-solved sets.  fia_version stays
 * 100. */
#define FIA_FLIP_MAX_SET 64
int fia_pair_flip(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user, const int32_t* q_item_i,
                  const int32_t* q_item_j,
                  const double* margin,           /* device [Q], nullable: 0                    */
                  int max_set,
                  int32_t* set_size,              /* device [Q], nullable                       */
                  int32_t* set_row,               /* device [Q*max_set], nullable               */
                  double* set_val,                /* device [Q*max_set], nullable               */
                  double* first_order,            /* device [Q], nullable                       */
                  double* newton,                 /* device [Q], nullable                       */
                  double* dtheta,                 /* device [Q*D3], nullable                    */
                  double* diff,                   /* device [Q], nullable                       */
                  void* stream);

/* Slates: which ratings shape a user's top-N list.  The explained number is a weighted sum over a
 * ranked list, f = sum_l w_l * r-hat(u, i_l) -- the caller picks the weights: 1 / log2(rank + 1) for a
 * DCG-like score, (1, -1) for fia_pair_batch's gap.  As with the pair call, the weighted sum of m
 * fia_query_batch results is not FIA's answer for f: the single queries restrict to different parameter
 * sets, normalise by different n, and each re-solves the shared user block against one item alone.
 * Slate query q = (u; i_1 .. i_m; w_1 .. w_m) = (q_user[q]; slate_item[slate_offsets[q] ..
 * slate_offsets[q + 1]); slate_weight[likewise]), the items distinct, 1 <= m <= FIA_SLATE_MAX_ITEMS.
 * Side block size Ds = k + 1 (MF) or 2k (NCF), D_q = (m + 1) * Ds.
 *   theta_t = (theta_u, theta_i1, .., theta_im)
 *   rel     = where(user == u) ++ where(item == i_1) ++ .. ++ where(item == i_m), each in ascending
 *             train-row order; n = |rel|.  A train row (u, i_l) sits in rel twice; no row three times.
 *   For position p with train row (a, b, y): e_p = r-hat(a, b) - y and g_p = d r-hat(a, b) / d theta_t,
 *             whose user block is zero unless a == u and whose block l unless b == i_l -- whichever list
 *             the position is in.
 *   H       = (2/n) sum_p (g_p g_p^T + e_p d2 r-hat_p) + wd * diag(M) + damping * I.  From the caches, with
 *             v^l = d r-hat(u, i_l) / d (theta_u, theta_il), A_u / B_i the entity Grams, (cd_l, es_l) = (rows
 *             of (u, i_l) in train, the sum of their residuals) and E the diagonal of the own pair's
 *             d2 r-hat / d theta_i d theta_u (MF: 1 on the k embedding coordinates, 0 on the bias; NCF: W3g
 *             on the GMF coordinates, 0 on the MLP coordinates):
 *               H_uu = (2/n) (A_u + sum_l cd_l v^l_u v^l_u^T)       H_ll = (2/n) (B_il + cd_l v^l_l v^l_l^T)
 *               H_lu = (2/n) 2 (cd_l v^l_l v^l_u^T + es_l diag(E))  H_lm = 0 for l != m
 *             plus the diagonal terms: an arrowhead, block diagonal when the user has rated no slate item.
 *   v       = d f / d theta_t = (sum_l w_l v^l_u, w_1 v^1_1, .., w_m v^m_m)
 *   x       = H^-1 v: exact fp64, block by block -- each item block's LDL^T, the Schur complement of the
 *             rated items taken out of the user block, the user block's LDL^T, then the rated items'
 *             back-substitution; nothing assumed about a pivot's sign
 *   influence[offsets[q] + p] = x . (2 e_p g_p + wd * M * theta_t) / n     fia_query_batch's expression
 *   value[q] = f                                                           current parameters, fp64
 *   x_out   : query q's x starts at Ds * (slate_offsets[q] + q), D_q doubles in the reference theta order,
 *             extended: MF [p_u, q_1 .. q_m, b_u, b_1 .. b_m], NCF [Pm_u, Qm_1 .. Qm_m, Pg_u, Qg_1 .. Qg_m]
 * With m = 2 and w = (1, -1) this is fia_pair_batch's system, with m = 1 and w = (1) fia_query_batch's
 * (equal values; the elimination order differs, so not equal bits).  A zero weight is an ordinary
 * weight: the item stays in theta_t and in rel.
 * topk (K in [0, FIA_MAX_TOPK]; 0 = off): per query, as fia_pair_batch -- position in the slate's own
 * related list (topk_pos), train row (topk_idx), signed value (topk_val), device arrays [Q*K]; unused
 * slots hold -1 / -1 / NaN.
 *   - An id outside [0, num_users) x [0, num_items) is never used as an index and counts as n = 0; the
 *     query's value and x are NaN.  A repeated item, m = 0 and m > FIA_SLATE_MAX_ITEMS are treated alike.
 *   - n = 0 with good ids (an empty user and empty items) writes no ratings, a NaN x and the finite f.
 *   - No floating-point atomics and every sum in slate order: a query's bits depend on (u, the items in
 *     their order, the weights) alone, not on where it sits in the batch or on what else is in it.
 * fia_count_related_slate: fia_count_related_pair's contract for the slate list (offsets device int64
 * [Q+1]; with total_out the total is copied to the host, the stream synchronised, bad ids, repeated
 * items and bad slate lengths reported as FIA_ERR_INVALID, and a query whose u or one of whose items is
 * outside a fia_prepare_for cover as FIA_ERR_STATE).  Without total_out such queries count zero.  Needs
 * the index only.
 * fia_slate_batch: rel_idx (int32 train rows), influence, x_out and value are each nullable; all four
 * NULL with K == 0 is FIA_ERR_INVALID.  total_rel must equal offsets[Q], total_items slate_offsets[Q].
 * With influence NULL and K > 0 nothing of length total_rel is written.  num_queries == 0 returns FIA_OK
 * and launches nothing.  Batch limits: total_items and num_queries <= FIA_SLATE_MAX_TOTAL_ITEMS (2^30: a
 * half record per (query, item), indexed in 32 bits), total_rel <= FIA_SLATE_MAX_TOTAL_REL (2^31 - 1: the
 * top-K keeps a 32-bit position); a larger batch is refused with FIA_ERR_INVALID before anything is
 * reserved or launched -- split it.  Checks run in fia_pair_batch's order: bounds, state, outputs, the
 * empty batch, nulls, support.  Needs params, index and a prepare (else FIA_ERR_STATE).  After
 * fia_prepare_for the cover must hold u and every slate item (fia_prepare_for with the pairs (u, i_l));
 * the results are then bitwise those after fia_prepare.  Ordered on `stream`, no host synchronisation; it
 * reads the entity Gram caches, so it joins a pending small-k Gram pass as fia_pair_batch does.  Stores
 * are per element: the outputs need only their types' natural alignment.
 * Sizes: MF k in {8, 16, 32, 64} and NCF k in {8, 16, 32} -- every small-k size, the two that
 * fia_pair_batch refuses included: a workgroup holds two packed Ds triangles whatever m (MF k=64: 2 x
 * 2,145 doubles).  The large-k models are FIA_ERR_UNSUPPORTED.
 * Phases (fia_set_profiling): 4 the count and scan (fia_count_related_slate) and the related rows,
 * 1 the solves, 2 the scoring, 3 the top-K.  fia_version stays 100: no existing signature, struct or
 * constant changed. */
#define FIA_SLATE_MAX_ITEMS 64
#define FIA_SLATE_MAX_TOTAL_ITEMS (1LL << 30)
#define FIA_SLATE_MAX_TOTAL_REL ((1LL << 31) - 1)
int fia_count_related_slate(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user,
                            const int64_t* slate_offsets,   /* device [Q+1]                              */
                            int64_t total_items,            /* == slate_offsets[Q]                       */
                            const int32_t* slate_item,      /* device [total_items]                      */
                            int64_t* offsets,               /* device [Q+1], written                     */
                            int64_t* total_out,             /* host, nullable                            */
                            void* stream);
int fia_slate_batch(fia_ctx* ctx, int64_t num_queries, const int32_t* q_user, const int64_t* slate_offsets,
                    int64_t total_items, const int32_t* slate_item,
                    const double* slate_weight,     /* device [total_items]                        */
                    const int64_t* offsets,         /* device [Q+1], from fia_count_related_slate */
                    int64_t total_rel,              /* == offsets[Q]                               */
                    int32_t* rel_idx,               /* device [total_rel], nullable                */
                    double* influence,              /* device [total_rel], nullable                */
                    double* x_out,                  /* device [Ds * (total_items + Q)], nullable   */
                    double* value,                  /* device [Q], nullable                        */
                    int K, int64_t* topk_pos, int64_t* topk_idx, double* topk_val,   /* device [Q*K] */
                    void* stream);

/* Number of restricted parameters D of the registered model (0 if none). */
int fia_num_params(const fia_ctx* ctx);

/* Phase timing with HIP events recorded on the call's stream (for the
 * roofline figures of bench.py).  phase_mask bit p enables phase p (0 = off,
 * FIA_PROFILE_ALL = every phase): every fia_prepare / fia_query_batch then
 * records one event pair per enabled phase; fia_profile_read synchronises
 * them, returns per-phase sums (ms) and counts, and clears them.
 * Phases: 0 prepare, 1 solve, 2 score (the dominant gather/scoring kernel),
 * 3 topk merge, 4 chunk build + scan.  Each pair costs a little stream time,
 * so timed runs enable only the phase they price.
 * MF k = 16, fia_query_batch: the chunk scan runs inside the side-system solve's
 * launch, so phase 1 (solve) spans that launch and the coupled solve -- chunk
 * scan included -- and phase 4 records nothing (count 0) for such a call; the sum
 * of phases 4 and 1 means what it meant.  fia_query_batch_x has no solve: there
 * phase 4 is the scan as before.  These pairs are taken right before the launch
 * that stamps them and returned if it fails, so a failed call leaves no
 * unrecorded pair for fia_profile_read. */
#define FIA_NUM_PHASES 5
#define FIA_PROFILE_ALL 0x1f
int fia_set_profiling(fia_ctx* ctx, int phase_mask);
int fia_profile_read(fia_ctx* ctx, double* ms_sum /*[FIA_NUM_PHASES]*/, int64_t* counts /*[FIA_NUM_PHASES]*/);

#ifdef __cplusplus
}
#endif
#endif /* FIA_H_ */
