// Internal definitions shared by the FIA HIP translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "fia.h"

namespace fia {

constexpr int kWave = 64;
constexpr int kScoreThreads = 256;       // scoring workgroup (4 independent waves)
constexpr int kScoreRows = 4;            // related ratings per lane and chunk
constexpr int kChunk = 64 * kScoreRows;  // related ratings per scoring chunk (one wave)
constexpr int kRunQB = 16;               // queries per item-run block (k_score_mf_runs)
constexpr int kRunChunk = 128;           // related ratings per item-run descriptor (k_score_mf_runs)
constexpr int kNcfRunChunk = 64;         // ... for NCF k <= 16 (k_score_ncf_runs: one rating per lane)
constexpr int kRunUserCost = 3;          // scheduling cost of a user-side run descriptor (k_score_mf_runs
                                         // slices): 2 per descriptor + 1 per query of its run

// One scoring chunk: <= kChunk consecutive ratings of ONE side (user list or item
// list) of one query, so every value a wave needs from the query is wave-uniform.
struct ChunkDesc {
  int64_t list_base;   // index into the side's list arrays
  int64_t out_base;    // index into rel_idx / influence
  int32_t q;           // query
  int32_t pos0;        // related position of the chunk's first rating
  int32_t len;         // ratings in the chunk
  int32_t side;        // 0 = user list R_u, 1 = item list C_i
};
constexpr int kPrepThreads = 256;        // Gram workgroup
constexpr int kSolveThreads = 64;        // one wave per query solve
constexpr int kGramChunk = 256;          // list rows per Gram work item (MI355X sweep: 64/128/256/512)
constexpr int kGsSub = 16;              // ratings per Gram-stream sub-batch (4 f64 MFMA row-quads)
constexpr int kGsSlice = 256;           // longest Gram-stream segment (longer lists: partial slices;
                                        // <= 511: a segment's count rides in 9 bits of its descriptor)
constexpr int kGsTarget = 8;            // sub-batches per Gram-stream wave (a range closes at >= this)
// (ml-1m-ex same-box A/B, ms per step: target 16 0.1460-0.1461; 8 0.1446-0.1448; 32 0.1442-0.1453;
//  slices of 128 0.1483; at most 8 segments per range 0.1481.  With 4-wave team workgroups, one
//  batch in flight: target 8 0.1206-0.1215; 12 0.1224-0.1230; 16 0.1257-0.1259; 8 waves
//  0.1252-0.1253; short teams two slices per wave 0.1225-0.1229 -- profiles/gram_teams.md)
constexpr uint32_t kGsNoRow = 0x7fffff00u;   // Gram-stream row offset of no rating: outside any
                                             // table's buffer range, even + a lane's column bytes
constexpr int kGsRing = 8;              // gathered sub-batches in the kernel's register ring
constexpr int kGsMaxSub = 48;           // most sub-batches of one wave's range (a multiple of kGsRing)
constexpr int kGsMaxSeg = 4;            // most segments (Grams) of one wave's range: staged in LDS,
                                        // stored when the range is done
constexpr int kGsWaves = 4;             // waves (ranges) of a Gram-stream workgroup
constexpr int kGsTeamPer = kGsMaxSub / (kGsSlice / kGsSub);   // most slices of a team in one wave (3)
constexpr int kGsTeamSlices = kGsWaves * kGsTeamPer;   // a team's reach: the longest list (in slices)
                                        // whose slices one workgroup sums in LDS; longer: gscomb
constexpr int kGsTeamMinPer = 1;         // fewest slices per wave of a team (1: a short team is spread
                                        // one slice per wave)
constexpr uint32_t kGsTeamBit = 1u << 22;   // descriptor `out`: a team slice {slice << 8 | slices << 3 | per}
constexpr int kMfmaQB = 16;             // queries per MF k in {32, 64} MFMA scoring work item
constexpr int kMfmaCPI = 4;             // list chunks per MFMA scoring work item
constexpr int kWgBlocks = 4;            // query blocks (one per wave) sharing a workgroup's gathered rows
constexpr int kQueryBlock = 8;           // queries per entity-shared scoring work item (small k; 16 measured no better)
static_assert(kGsSlice < 512, "a Gram-stream segment's count rides in 9 bits of its descriptor (out >> 23)");
static_assert(kGsSlice % kGsSub == 0 && kGsTeamPer >= 1 && kGsTeamPer <= kGsMaxSeg && kGsTeamPer < 8 &&
                  kGsTeamSlices < 32,
              "a team wave stages its slices from segment 0; slice and count ride in 5 bits each, per in 3");

// Device buffer with grow-on-demand capacity (never shrinks), allocated from the
// device's stream-ordered pool on the context's stream: growing a buffer frees the old
// block in stream order (kernels already queued on `s` still read it) and allocates
// the new one behind them -- no device-wide synchronisation on the query path.  Work
// queued on ANOTHER stream is covered by the ABI: a call arriving on a different stream
// than the context's previous call first synchronises the device (fia_ctx::stream,
// abi.hip enter_stream), so a stream-ordered free never overtakes a reader there.  A
// regrown buffer gets 25 % headroom so a slowly growing batch does not regrow it
// every call.  Contents are not preserved.
struct DevBuf {
  void* ptr = nullptr;
  size_t bytes = 0;
  hipError_t reserve(size_t want, hipStream_t s) {
    if (want <= bytes && ptr) return hipSuccess;
    // a regrow inside a graph capture would free a block allocated outside the graph:
    // buffers must be sized by an eager call before capture
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
      return hipErrorStreamCaptureUnsupported;
    size_t cap = want < 256 ? 256 : want;
    if (ptr) {
      const size_t grown = bytes + bytes / 4;
      if (grown > cap) cap = grown;
      hipError_t e = hipFreeAsync(ptr, s);
      if (e != hipSuccess) return e;
      ptr = nullptr;
      bytes = 0;
    }
    hipError_t e = hipMallocAsync(&ptr, cap, s);
    if (e == hipSuccess) bytes = cap; else ptr = nullptr;
    return e;
  }
  void release(hipStream_t s) {
    if (ptr) (void)hipFreeAsync(ptr, s);
    ptr = nullptr;
    bytes = 0;
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(ptr); }
};

// User-major (CSR) / item-major (CSC) rating index.  For side s the list of
// entity e is [ptr[e], ptr[e+1]); row = train row (ascending), other = the
// other endpoint's id, rating = train label.
struct Side {
  DevBuf ptr;     // int64 [n_entity + 1]
  DevBuf row;     // int32 [N]
  DevBuf other;   // int32 [N]
  DevBuf rating;  // float [N]
};

struct Index {
  int64_t N = 0, U = 0, I = 0;
  Side side[2];   // 0 = users (R_u), 1 = items (C_i)
  DevBuf order[2];  // int32 [n_entity]: entities by list length, longest first (Gram scheduling)
  // Gram work lists: items of <= kGramChunk list rows {entity, start, len, slot}; slot < 0 =
  // write the entity's Gram directly, else a partial slot summed (in slot order) by a combine
  // pass {entity, first_slot, n_slots, 0}
  DevBuf gitems[2], gcomb[2];
  int64_t n_gitems[2] = {0, 0}, n_gcomb[2] = {0, 0}, n_gslots[2] = {0, 0};
  // open-addressing set of train pairs: key u*I+i -> (#rows, sum of ratings); answers
  // "is the test pair itself a train row?" in O(1) for the Hessian's d2r term
  DevBuf pkey;    // uint64 [pcap], ~0 = empty
  DevBuf pcnt;    // int32  [pcap]
  DevBuf psum;    // double [pcap]
  int64_t pcap = 0;
  std::vector<int64_t> hptr[2];   // host copies of side[s].ptr (Gram work lists)
  std::vector<int32_t> hord[2];   // entities by list length, longest first (host)
  int64_t gchunk = 0;             // list rows per small-k Gram work item of gitems
  // MF k <= 16 Gram stream (build_gram_stream, k_gram_mf_stream): the lists of both sides cut
  // into sub-batches of kGsSub ratings, one descriptor each {meta, out} (meta = valid ratings
  // | last of its segment << 5 | side << 6 | dummy << 7 | entity << 8; out, on a segment's last
  // sub-batch: its rating count << 23 | partial slot + 1, 0 = the entity's own Gram), the byte
  // offsets of their other-side rows in stream order (kGsSub per sub-batch, kGsNoRow past a
  // list's end), and the first descriptor of every wave's range, kGsWaves ranges to a workgroup
  // (n_gsw is a multiple of it).  Whole lists up to kGsSlice ratings; a longer list in kGsSlice
  // slices: up to kGsTeamSlices of them as a team, out = count << 23 | kGsTeamBit | slice << 8 |
  // slices << 3 | slices per wave, all in consecutive waves of one workgroup, which sums them
  // in LDS in slice order.  gscomb {entity, first slot, slots, 0} and n_gsslots cover only the
  // lists beyond that reach: their slices go to partial slots (Ctx::gpart) and k_gram_combine
  // sums them in slot order; both are empty where no list is that long
  DevBuf gsdesc, gsids, gswave, gscomb[2];
  int64_t n_gsw = 0, n_gsdesc = 0, n_gscomb[2] = {0, 0}, n_gsslots[2] = {0, 0};
  uint64_t gs_version = ~0ull;
  int gs_k = 0;
  uint64_t version = 0;           // bumped by every build_index
  bool valid = false;
};

// ---- the (model, k) sizes the library is built for, each spelled once ----
// small k: every structure of a query fits a wave's registers or a workgroup's LDS (models.hip
// and the small_*.hip, score_*.hip and gram_mf.hip kernel units)
#define FIA_SMALL_SIZES(X) X(MF, 8) X(MF, 16) X(MF, 32) X(MF, 64) X(NCF, 8) X(NCF, 16) X(NCF, 32)
// large k (bigk.hip and the bigk_*.hip kernel units)
#define FIA_BIG_SIZES(X) X(MF, 128) X(MF, 256) X(NCF, 64) X(NCF, 128) X(NCF, 256)

// f(MF<k>{}) or f(NCF<k>{}) for the size (model, k) of a list, MF / NCF being the caller's trait
// templates (MFm / NCFm of kern.h, BMF / BNCF of bigk.h); false, and f not called, for a size
// not in the list.  f's own result goes out through its captures.
#define FIA_SIZE_CASE(fam, kv)                \
  if (model == FIA_MODEL_##fam && k == kv) {  \
    f(fam<kv>{});                             \
    return true;                              \
  }
template <template <int> class MF, template <int> class NCF, class F>
bool for_small_size(int model, int k, F&& f) {
  FIA_SMALL_SIZES(FIA_SIZE_CASE)
  return false;
}
template <template <int> class MF, template <int> class NCF, class F>
bool for_big_size(int model, int k, F&& f) {
  FIA_BIG_SIZES(FIA_SIZE_CASE)
  return false;
}
#undef FIA_SIZE_CASE

// ---- device helpers shared by the kernels ----
// the largest e in [lo, hi] with off[e] <= g (off[lo] <= g given): the owner of position g in
// ascending offsets
template <class I, class T>
__device__ __forceinline__ I last_at_most(const T* __restrict__ off, I lo, I hi, T g) {
  while (lo < hi) {
    const I mid = (lo + hi + 1) >> 1;
    if (off[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

constexpr unsigned long long kEmptyKey = ~0ull;

__host__ __device__ inline unsigned long long pair_hash(unsigned long long k) {
  k += 0x9e3779b97f4a7c15ull;
  k = (k ^ (k >> 30)) * 0xbf58476d1ce4e5b9ull;
  k = (k ^ (k >> 27)) * 0x94d049bb133111ebull;
  return k ^ (k >> 31);
}

struct PairTable {
  const unsigned long long* key;
  const int32_t* cnt;
  const double* sum;
  unsigned long long mask;
  __device__ inline void lookup(unsigned long long k, double& c, double& s) const {
    unsigned long long h = pair_hash(k) & mask;
    c = 0.0;
    s = 0.0;
    for (unsigned long long probe = 0; probe <= mask; ++probe) {
      unsigned long long kk = key[h];
      if (kk == k) { c = (double)cnt[h]; s = sum[h]; return; }
      if (kk == kEmptyKey) return;
      h = (h + 1) & mask;
    }
  }
  // the same lookup split in two: the first probe's load is issued early, the rest of the
  // chain (rarely more than one probe at load <= 1/2) resolves later
  __device__ inline void probe_start(unsigned long long k, unsigned long long& h, unsigned long long& kk) const {
    h = pair_hash(k) & mask;
    kk = key[h];
  }
  __device__ inline void probe_finish(unsigned long long k, unsigned long long h, unsigned long long kk, double& c,
                                      double& s) const {
    c = 0.0;
    s = 0.0;
    for (unsigned long long probe = 0; probe <= mask; ++probe) {
      if (kk == k) { c = (double)cnt[h]; s = sum[h]; return; }
      if (kk == kEmptyKey) return;
      h = (h + 1) & mask;
      kk = key[h];
    }
  }
};

// Parameter table pointers (device, float32, owned by the caller).
struct Params {
  int model = -1, k = 0;
  int64_t U = 0, I = 0;
  const float* t[10] = {};
  double wd = 0.0, damping = 0.0;
  bool valid = false;
};

struct PhaseEvents {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[FIA_NUM_PHASES];
  std::vector<hipEvent_t> pool;
};

// First words of a query's scoring record (c->rec), the same at every k; the rest of the record
// is Rec* of kern.h (small k) and BigRec* of bigk.h (large k).  Offsets in doubles.
struct RecHead {
  static constexpr int inv_n = 0;   // 1 / n; NaN: the query has no related rating
  static constexpr int c_q = 1;     // wd * x . theta over the decayed coordinates
  static constexpr int x_v = 2;     // x . v
  static constexpr int rhat = 3;    // r-hat(u, i)
};

}  // namespace fia

struct fia_ctx {
  int device = 0;
  std::string err;
  fia::Params p;
  fia::Index idx;
  // per-entity Gram caches (packed lower triangle, fp64): [U * GS], [I * GS]
  fia::DevBuf gram[2];
  // NCF: per-entity layer-1 halves Pm*W1[:k] and Qm*W1[k:] (fp64) [U*k], [I*k]
  fia::DevBuf l1[2];
  fia::DevBuf gpart[2];   // partial Grams of long lists (fp64, [n_gslots * GSP])
  bool prepared = false;
  // per-batch scratch
  fia::DevBuf rec;        // per-query scoring record (fp64): M::Rec of the model's traits
  fia::DevBuf coff;       // int64 [Q+1] chunk offsets
  fia::DevBuf cdesc;      // ChunkDesc [max chunks]
  fia::DevBuf cand_pos;   // int32 [max chunks * K]
  fia::DevBuf cand_val;   // double [max chunks * K]
  fia::DevBuf qscan;      // k_query_scan tile words + counters (left zero by every launch)
  fia::DevBuf flag;       // int32 [4] device status words
  fia::DevBuf nch;        // int64 [Q+1] chunk counts
  // int32 [Q + 2] {readers, count, q ...}: the queries whose test pair is a train row, appended by
  // the side-system solve and finished by k_solve.  Zero when (re)allocated; k_solve takes the
  // count and counts itself a reader with one 64-bit atomic on the first two words, and its last
  // reader zeroes both, so every call finds the count zero without a memset or a launch
  // (MF k = 16 never touches it: its coupled queries are a role of k_solve_quad)
  fia::DevBuf coupled;
  // query groups per entity (entity-shared scoring): global entity index g = e (users) or
  // U + e (items)
  fia::DevBuf gcnt;       // uint64 [U + I + 1] queries per entity -> exclusive scan in gstart
  fia::DevBuf gstart;     // int64 [U + I + 1]
  fia::DevBuf grank;      // int32 [2Q] rank of query q in its user group / item group
  fia::DevBuf gq;         // int32 [2Q] queries grouped by entity (users then items)
  fia::DevBuf qbase;      // int64 [2Q] per query and side: output base, candidate-slot base
  fia::DevBuf slices;     // int32 [n + 1] first descriptor of each equal-cost slice (k_score_mf_runs)
  fia::DevBuf wstart;     // int64 [U + I + 1] exclusive scan of the work items per entity
  fia::DevBuf gscan;      // k_group_scan tile words + counters (left zero by every launch)
  fia::DevBuf witems;     // int32 [3 * max items] {global entity, list chunk, query block}
  fia::DevBuf d1tab;      // NCF k <= 16: d1 per z2 ReLU mask [2^(k/2)][k] (fp64)
  // fia_total_influence (total.hip), per batch: sort keys / queries (in, out) of the 2Q (entity,
  // query) pairs, per-group aggregates, entity -> group, per-query / per-group words, sort scratch
  fia::DevBuf tkeys, tvals, tagg, tslot, tword, tsort;
  // fia_group_influence (group.hip): train row -> {user, item, rating, list position} (per index),
  // and per batch the queries' x_q = H^-1 v [Q * D] for first_order (fia_self_influence, self.hip:
  // the same row table, and gxq for the newton values [num_rows] of a top-K without the array)
  fia::DevBuf rowrec, gxq;
  uint64_t rowrec_version = ~0ull;
  // the same two calls at large k (group_big.hip), per launch of a chunk of systems: the groups'
  // scalars and right-hand side sums, their two Gram-shaped downdates (tile-packed, as the
  // caches), and fia_self_influence's implicit queries
  fia::DevBuf dwork, dslab, dpairs;
  // large-k path (bigk.hip): per-list-position entity, per-train-row residual / NCF backward
  // vectors, per-query Hessian inputs and solutions, solve lists and LDL^T scratch
  fia::DevBuf self[2];    // int32 [N] entity owning list position p of side s
  uint64_t self_version = ~0ull;
  fia::DevBuf resid;      // double [N]   e_j = r-hat_j - y_j by train row
                          //   (small-k NCF: [2][N] by list position of each side)
  fia::DevBuf gm[2];      // double [N*k] NCF g_mlp = W1_side . d1_j by train row, per side
                          //   (small-k NCF: [k][N] by list position)
  fia::DevBuf wfrag;      // large-k NCF: W2 / W1 as f64 MFMA B fragments [3 k^2] (k_ncf_wfrag)
  fia::DevBuf slot[2];    // int32 [n_entity] Gram cache slot (-1 = not cached) after fia_prepare_for
  fia::DevBuf mark;       // uint8 [U + I] entities referenced by the fia_prepare_for queries
  bool subset = false;    // caches cover only the fia_prepare_for entities (large-k models)
  bool small_subset = false;   // small k after fia_prepare_for: Grams of the `mark`ed entities only
  fia::DevBuf bitems[2], bcomb[2];   // large-k Gram work lists {entity, start, len, slot}
  int64_t n_bitems[2] = {0, 0}, n_bcomb[2] = {0, 0}, n_bslots[2] = {0, 0}, n_bcache[2] = {0, 0};
  uint64_t bitems_version = ~0ull;
  int bitems_k = 0;
  fia::DevBuf qwork;      // double [Q * QW] per-query work words (BigWork, bigk.h; NCF k = 16: QPro, kern.h)
  fia::DevBuf xb;         // double [Q * 2 NPs] per-query solution (padded side blocks)
  fia::DevBuf syslist;    // int32 [1 + 2Q] {count, 2q + side ...} uncoupled side systems
  fia::DevBuf cpllist;    // int32 [1 + Q]  {count, q ...} coupled full systems
  fia::DevBuf lscr;       // double LDL^T factor scratch, one slab per resident solve workgroup
  int num_cus = 0;
  // the stream of the previous call (a switch synchronises first: DevBuf frees are ordered
  // on the calling stream only)
  hipStream_t stream = nullptr;
  bool has_stream = false;
  // small-k fia_prepare runs its Gram pass on `aux`, forked from the calling stream, so the
  // query-side scans of the next calls overlap it; the first consumer of the caches (the
  // solve of fia_query_batch, or any call that rewrites what the pass reads) joins `prep`
  hipStream_t aux = nullptr;
  hipEvent_t fork_ev = nullptr, prep_ev = nullptr;
  bool prep_pending = false;
  // NCF: the per-entity layer-1 rows (the first kernels of the pass), which the query-side MLP
  // prologue reads before the Gram caches are done
  hipEvent_t l1_ev = nullptr;
  bool l1_pending = false;
  unsigned profiling = 0;   // bit p: record phase p (fia_set_profiling)
  fia::PhaseEvents events;
};

namespace fia {

// ---- the context as the kernels' argument structs carry it ----
// What every kernel reads of the model: the table sizes, the list pointers, the parameter tables,
// the dense NCF layer-1 rows and the weight decay.  The argument structs of the kernels that read
// nothing else of the context (score_cand.hip, total.hip) derive from it; QueryArgs (kern.h) and
// BigArgs (bigk.h) hold the same members among their own, in the order their kernels were
// tuned with (moving them changed the register counts of three solve kernels).
struct ModelArgs {
  int64_t U, I;
  const int64_t* ptr[2];
  const float* t[10];
  const double* l1[2];
  double wd;
};
template <class Args>
void fill_model_args(const fia_ctx* c, Args& A) {
  A.U = c->p.U;
  A.I = c->p.I;
  for (int s = 0; s < 2; ++s) {
    A.ptr[s] = c->idx.side[s].ptr.as<int64_t>();
    A.l1[s] = c->l1[s].as<double>();
  }
  for (int j = 0; j < 10; ++j) A.t[j] = c->p.t[j];
  A.wd = c->p.wd;
}

inline PairTable pair_table(const Index& X) {
  return {X.pkey.as<unsigned long long>(), X.pcnt.as<int32_t>(), X.psum.as<double>(),
          (unsigned long long)(X.pcap - 1)};
}

// ... and what the per-list-position kernels read besides: the lists of both sides, the Gram
// caches, the damping and the train-pair table
template <class Args>
void fill_list_args(const fia_ctx* c, Args& A) {
  fill_model_args(c, A);
  for (int s = 0; s < 2; ++s) {
    A.row[s] = c->idx.side[s].row.as<int32_t>();
    A.other[s] = c->idx.side[s].other.as<int32_t>();
    A.rating[s] = c->idx.side[s].rating.as<float>();
    A.gram[s] = c->gram[s].as<double>();
  }
  A.damping = c->p.damping;
  A.pairs = pair_table(c->idx);
}

// ---- launchers implemented in the .hip units ----
hipError_t build_index(fia_ctx* c, int64_t N, int64_t U, int64_t I, const int32_t* user,
                       const int32_t* item, const float* rating, hipStream_t s, std::string& why);
hipError_t count_related(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi,
                         int64_t* offsets, hipStream_t s);
hipError_t write_related(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi,
                         const int64_t* offsets, int32_t* rel, hipStream_t s);
// per-query chunk offsets coff (+ chunk descriptors unless offsets_only; with `runs` the
// descriptors are the compacted work list of k_score_mf_runs: every user-side chunk, the
// item-side chunks of run heads only, their count at qbase[4Q]; and the equal-cost slices of
// that list, c->slices[0 .. n] with n at qbase[4Q + 1], slice_cost units each -- rounded up
// to a power of two)
hipError_t build_chunks(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                        int64_t max_chunks, bool offsets_only, hipStream_t s, int32_t* zero_word = nullptr,
                        bool runs = false, int slice_cost = 0, int run_chunk = kRunChunk);
hipError_t build_gram_lists(fia_ctx* c, int64_t chunk, hipStream_t s);
// the MF k <= 16 Gram stream of the current index (Index::gs*), rebuilt after build_index
hipError_t build_gram_stream(fia_ctx* c, int k, hipStream_t s);
// per-batch query groups + entity-chunk work items (needs build_chunks' coff first)
hipError_t build_groups(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                        int64_t max_items, int qb, hipStream_t s, int cpi = 1);

// model kernels: return hipErrorInvalidValue-style codes, or set `unsupported`
hipError_t prepare_model(fia_ctx* c, hipStream_t s, bool& unsupported);
// small k: caches of the queries' users and items only (fia_prepare_for); marks in c->mark
hipStream_t prepare_stream(fia_ctx* c, hipStream_t s);
hipError_t prepare_record(fia_ctx* c, hipStream_t ps, hipStream_t s);
hipError_t join_prepare(fia_ctx* c, hipStream_t s);
hipError_t join_l1(fia_ctx* c, hipStream_t s);
// fia_prepare_for, small k, in two calls: mark_only marks the queries' entities on s; then
// their Gram caches on ps
hipError_t prepare_model_for(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, hipStream_t s, hipStream_t ps,
                             bool& unsupported, bool mark_only);
// c->mark: 1 for every user u and item U + i of the Q queries (out-of-range queries skipped)
hipError_t mark_entities(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, hipStream_t s);
hipError_t check_cover_small(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, int32_t* flag,
                             hipStream_t s);
hipError_t query_model(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                       int64_t max_chunks, int32_t* rel_idx, double* influence, double* x_out, int K,
                       int64_t* topk_pos, int64_t* topk_idx, double* topk_val, hipStream_t s,
                       bool& unsupported,
                       const double* x_in = nullptr);
int model_num_params(int model, int k);
bool model_supported(int model, int k);

// large-k models (bigk.hip): MF k in {128, 256}, NCF k in {64, 128, 256}
bool big_supported(int model, int k);
hipError_t ensure_self(fia_ctx* c, hipStream_t s);   // c->self[s]: entity of each list position
// contexts alive on a device (abi.hip): > 1 means batches of several contexts share the GPU
int live_contexts(int device);
// qu == nullptr: caches for every entity; else only for the entities of the Q queries
hipError_t prepare_big(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, hipStream_t s);
// flag[2] |= 1 if a query's user or item has no cache after fia_prepare_for
hipError_t check_cover(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, int32_t* flag, hipStream_t s);
hipError_t query_big(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                     int64_t max_chunks, int32_t* rel_idx, double* influence, double* x_out, int K,
                     int64_t* topk_pos, int64_t* topk_idx, double* topk_val, hipStream_t s,
                     const double* x_in = nullptr);
// MF k <= 16 item-run scoring (score_mf.hip); QueryArgs is in kern.h
// a one-kernel phase (scoring) timed by its own dispatch: the event pair goes to
// hipExtLaunchKernelGGL, which stamps the kernel's start and end from the dispatch packet
// (two marker packets around it idled the GPU ~5 us each); both null when not profiling
struct PhaseSpan {
  hipEvent_t a = nullptr, b = nullptr;
};
struct QueryArgs;
// MF k <= 16 Gram caches from the Gram stream (gram_mf.hip)
struct GramStreamArgs {
  const int2* desc;        // {meta, slot} per sub-batch (Index::gsdesc)
  const uint32_t* ids;     // other-side row byte offsets, kGsSub per sub-batch (quad-transposed)
  const int32_t* wave;     // first descriptor of each wave's range [n_waves + 1]
  int64_t n_waves;
  const float* emb_other[2];
  uint32_t bytes_other[2]; // their sizes (buffer ranges: a gather outside reads 0)
  double* gram[2];
  double* part[2];
  const uint8_t* mark;     // fia_prepare_for: entities to build (users [0, U), items [U, U + I)), or null
  int64_t moff[2];
};
hipError_t launch_gram_mf_stream(int k, const GramStreamArgs& G, hipStream_t s);
hipError_t launch_score_mf_runs(int k, int64_t grid, hipStream_t s, const QueryArgs& A, int64_t Q,
                                const ChunkDesc* cdesc, const int64_t* qbase, const int32_t* slices,
                                const double* rec, int32_t* rel_idx, double* influence, int K, int32_t* cand_pos,
                                double* cand_val, PhaseSpan ps);
// NCF k <= 16 item-run scoring (score_mf.hip)
hipError_t launch_score_ncf_runs(int k, int64_t grid, hipStream_t s, const QueryArgs& A, int64_t Q,
                                 const ChunkDesc* cdesc, const int64_t* qbase, const int32_t* slices,
                                 const double* rec, int32_t* rel_idx, double* influence, int K, int32_t* cand_pos,
                                 double* cand_val, PhaseSpan ps);
// MF k in {32, 64}, top-K <= 1 entity-shared f64-MFMA scoring (score_mfma.hip); full = both
// per-rating outputs present
hipError_t launch_score_mf_mfma(int k, bool full, int64_t grid, hipStream_t s, PhaseSpan ps, const QueryArgs& A,
                                int64_t nE, const int64_t* wstart, const int32_t* witems, const int64_t* gstart,
                                const int32_t* gq, const int64_t* qbase, const double* rec, int32_t* rel_idx,
                                double* influence, int K, int32_t* cand_pos, double* cand_val);
// per-query merge of chunk top-K candidates (small_score.hip); spc = candidate slot sets per chunk
hipError_t launch_topk_merge(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, int K, int spc,
                             int64_t* topk_pos, int64_t* topk_idx, double* topk_val, hipStream_t s,
                             int64_t max_chunks);

// fia_score_candidates (score_cand.hip): hypothetical ratings scored from the parameter tables
// (and the dense NCF layer-1 rows c->l1), x read from global memory in the reference order;
// scratch: c->rec, c->cand_pos, c->cand_val
hipError_t score_candidates(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const double* x,
                            const int64_t* cand_offsets, int64_t total_cand, const int32_t* cand_user,
                            const int32_t* cand_item, const float* cand_rating, double* influence, int K,
                            int64_t* topk_pos, double* topk_val, hipStream_t s);

// the per-query merge of the slots tile + q that the (tile, query) segments of tiles of kCandTile
// candidates wrote into c->cand_pos / c->cand_val (score_cand.hip's k_cand_merge, for a caller in
// another unit)
hipError_t launch_cand_merge(fia_ctx* c, int64_t Q, int64_t total, const int64_t* cand_offsets, int K,
                             int64_t* topk_pos, double* topk_val, hipStream_t s);

// fia_total_influence (total.hip): the scatter-add of fia_query_batch_x's influence by train
// row, computed from per-entity aggregates of the queries; scratch: c->rec, c->cand_pos,
// c->cand_val and the t* buffers
hipError_t total_influence(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const double* x,
                           double* total, int32_t* count, int K, int64_t* topk_idx, double* topk_val,
                           hipStream_t s);

// the per-query work words of a batch (c->qwork) and, with `solve`, x = H^-1 v (c->xb): the
// prologue and solve launches of query_big alone; sides = false when every query is a train pair
hipError_t big_systems(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, bool solve, bool sides,
                       hipStream_t s);

// fia_group_influence (group.hip): per group of train rows the re-solved system with the
// group's rows removed; the small-k sizes (group_supported); scratch: c->rowrec, c->gxq.
// group_influence_big / self_influence_big (group_big.hip): the same two calls for the sizes of
// big_supported, the systems in device memory, in chunks of bounded scratch (c->dwork, c->dslab,
// c->dpairs and the per-query buffers of query_big)
hipError_t ensure_rowrec(fia_ctx* c, hipStream_t s);
hipError_t group_influence_big(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi,
                               const int64_t* grp_offsets, int64_t num_groups, const int64_t* mem_offsets,
                               int64_t total_members, const int32_t* mem_row, double* group, double* first_order,
                               double* dtheta, hipStream_t s);
hipError_t self_influence_big(fia_ctx* c, int64_t n, const int32_t* rows, double* first_order, double* newton,
                              double* error, hipStream_t s);
bool group_supported(int model, int k);
hipError_t group_influence(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* grp_offsets,
                           int64_t num_groups, const int64_t* mem_offsets, int64_t total_members,
                           const int32_t* mem_row, double* group, double* first_order, double* dtheta,
                           hipStream_t s);

// fia_self_influence (self.hip): every listed train row against its own prediction, the group
// call's singleton case fused; the sizes of group_supported; scratch: c->rowrec, c->cand_pos,
// c->cand_val, and c->gxq for the newton values when only their top-K is asked for.  n == 0
// only fills the top-K slots.
hipError_t self_influence(fia_ctx* c, int64_t n, const int32_t* rows, double* first_order, double* newton,
                          double* error, int K, int64_t* topk_pos, int64_t* topk_idx, double* topk_val,
                          hipStream_t s);

// fia_query_batch_newton (newton.hip): the Newton-corrected influence of every related rating,
// one factorisation per query and a quadratic form per rating; the small-k sizes
// (newton_supported); scratch: c->rec (the per-query records, in launches of bounded size),
// c->coff, c->cdesc, c->cand_pos, c->cand_val, c->d1tab, and c->gxq for the own-pair values
// when `newton` is NULL
bool newton_supported(int model, int k);
hipError_t query_newton(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                        int64_t total_rel, int32_t* rel_idx, double* newton, int K, int64_t* topk_pos,
                        int64_t* topk_idx, double* topk_val, hipStream_t s);

// fia_score_candidates_newton (cand_newton.hip): hypothetical ratings with their own curvature in
// the system, one factorisation per query and a quadratic form per candidate; the sizes of
// newton_supported; scratch: c->rec (the per-query records, in launches of bounded size), c->tkeys,
// c->tvals, c->tsort (the partition by (query, side)), c->tslot, c->tword, c->d1tab, c->cand_pos,
// c->cand_val, and c->gxq for the values when `newton_add` is NULL
hipError_t score_candidates_newton(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi,
                                   const int64_t* cand_offsets, int64_t total_cand, const int32_t* cand_user,
                                   const int32_t* cand_item, const float* cand_rating, double* newton_add, int K,
                                   int64_t* topk_pos, double* topk_val, hipStream_t s);

// fia_edit_influence (edit.hip): per edit set -- train rows removed, hypothetical ratings added --
// the system downdated and updated and solved once; the sizes of group_supported; scratch:
// c->rowrec, c->gxq (x_q for first_order, then the values of a top-K without `edit`), c->cand_pos,
// c->cand_val
hipError_t edit_influence(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* grp_offsets,
                          int64_t num_groups, const int64_t* rem_offsets, int64_t total_rem, const int32_t* rem_row,
                          const int64_t* add_offsets, int64_t total_add, const int32_t* add_user,
                          const int32_t* add_item, const float* add_rating, double* edit, double* first_order,
                          double* dtheta, int K, int64_t* topk_pos, double* topk_val, hipStream_t s);

// fia_count_related_pair / fia_pair_batch (pair.hip): the system of the gap r-hat(u, i) - r-hat(u, j)
// over theta_t = (theta_u, theta_i, theta_j) and the list R_u ++ C_i ++ C_j, assembled in LDS from
// the three Gram caches and solved once per query; the sizes of pair_supported; scratch: c->qscan
// and c->flag (the count), c->rec (two half records per query), c->coff (the tiles' first
// queries), c->cand_pos, c->cand_val
bool pair_supported(int model, int k);
hipError_t count_related_pair(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int32_t* qj,
                              int64_t* offsets, hipStream_t s);
hipError_t pair_batch(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int32_t* qj,
                      const int64_t* offsets, int64_t total_rel, int32_t* rel_idx, double* influence, double* x_out,
                      double* diff, int K, int64_t* topk_pos, int64_t* topk_idx, double* topk_val, hipStream_t s);

// fia_pair_flip (flip.hip): per pair query the greedy first-order set of the user's own ratings that
// closes the gap (the max_set smallest negative values of R_u, a sequential stop rule) and the
// re-solved three-block system with that set removed; the sizes of pair_supported; scratch: c->rec
// (pair_batch's half records), c->gxq (the gap and the sizes when the caller takes neither, the
// members' list entries)
hipError_t pair_flip(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int32_t* qj,
                     const double* margin, int max_set, int32_t* set_size, int32_t* set_row, double* set_val,
                     double* first_order, double* newton, double* dtheta, double* diff, hipStream_t s);

// fia_count_related_slate / fia_slate_batch (slate.hip): the system of f = sum_l w_l r-hat(u, i_l)
// over theta_t = (theta_u, theta_i1 .. theta_im) and the list R_u ++ C_i1 ++ .. ++ C_im, an arrowhead
// solved block by block (two Ds triangles in LDS whatever m); every small-k size (slate_supported);
// `cover`: the count also flags entities outside a fia_prepare_for cover.  Scratch: c->qscan and
// c->flag (the count), c->rec (a half record per (query, item)), c->coff (the tiles' first queries),
// c->nch (the queries' list starts), c->tkeys (their sorted items and which are scored),
// c->cand_pos, c->cand_val
bool slate_supported(int model, int k);
hipError_t count_related_slate(fia_ctx* c, int64_t Q, const int32_t* qu, const int64_t* slate_offsets,
                               int64_t total_items, const int32_t* slate_item, int64_t* offsets, bool cover,
                               hipStream_t s);
hipError_t slate_batch(fia_ctx* c, int64_t Q, const int32_t* qu, const int64_t* slate_offsets, int64_t total_items,
                       const int32_t* slate_item, const double* slate_weight, const int64_t* offsets,
                       int64_t total_rel, int32_t* rel_idx, double* influence, double* x_out, double* value, int K,
                       int64_t* topk_pos, int64_t* topk_idx, double* topk_val, hipStream_t s);

// phase event helpers (no-ops unless profiling)
void phase_begin(fia_ctx* c, int phase, hipStream_t s);
void phase_end(fia_ctx* c, int phase, hipStream_t s);
// (taken once the launch it times is known to proceed; phase_drop returns the pair of a launch
// that failed after all, so no unrecorded pair is left for fia_profile_read)
PhaseSpan phase_span(fia_ctx* c, int phase);
void phase_drop(fia_ctx* c, int phase, const PhaseSpan& ps);

}  // namespace fia

#define FIA_HIP_TRY(expr)                       \
  do {                                          \
    hipError_t _e = (expr);                     \
    if (_e != hipSuccess) return _e;            \
  } while (0)
