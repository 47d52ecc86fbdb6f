// C ABI entry points (include/fia.h).  Validates arguments, keeps the context
// state machine (params -> index -> prepare -> query), converts HIP errors to
// status codes + a message, and never lets an exception cross the boundary.
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <new>

#include "common.h"

namespace fia {

static bool pooled_event(fia_ctx* c, hipEvent_t* e) {
  if (!c->events.pool.empty()) {
    *e = c->events.pool.back();
    c->events.pool.pop_back();
    return true;
  }
  return hipEventCreate(e) == hipSuccess;
}

void phase_begin(fia_ctx* c, int phase, hipStream_t s) {
  if (!(c->profiling >> phase & 1u)) return;
  hipEvent_t a, b;
  if (!pooled_event(c, &a)) return;
  if (!pooled_event(c, &b)) { c->events.pool.push_back(a); return; }
  (void)hipEventRecord(a, s);
  c->events.ev[phase].push_back({a, b});
}

void phase_end(fia_ctx* c, int phase, hipStream_t s) {
  if (!(c->profiling >> phase & 1u) || c->events.ev[phase].empty()) return;
  (void)hipEventRecord(c->events.ev[phase].back().second, s);
}

PhaseSpan phase_span(fia_ctx* c, int phase) {
  PhaseSpan ps;
  if (!(c->profiling >> phase & 1u)) return ps;
  hipEvent_t a, b;
  if (!pooled_event(c, &a)) return ps;
  if (!pooled_event(c, &b)) { c->events.pool.push_back(a); return ps; }
  c->events.ev[phase].push_back({a, b});
  ps.a = a;
  ps.b = b;
  return ps;
}

void phase_drop(fia_ctx* c, int phase, const PhaseSpan& ps) {
  auto& v = c->events.ev[phase];
  if (!ps.a || v.empty() || v.back().first != ps.a) return;
  c->events.pool.push_back(v.back().first);
  c->events.pool.push_back(v.back().second);
  v.pop_back();
}

// The stream a small-k Gram pass runs on: the context's aux stream, made to wait for
// everything queued on `s` so far; `s` itself while `s` is being captured into a graph (a
// fork there would have to be joined inside the same capture) or when aux is unavailable.
hipStream_t prepare_stream(fia_ctx* c, hipStream_t s) {
  // MF k <= 16: the query scans the fork would overlap (~20 us at ml-1m-ex) barely exceed the
  // cross-queue wait of the join (~10 us on MI355X), and they run slower beside the Gram pass:
  // same-box A/B 0.172-0.173 ms per ml-1m-ex step on one stream vs 0.176-0.182 forked
  if (c->p.model == FIA_MODEL_MF && c->p.k <= 16) return s;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return s;
  if (!c->aux) {
    // the stream and its three events all or nothing (a half-made set would fork work that
    // can never be joined)
    hipStream_t a = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool ok = hipStreamCreateWithFlags(&a, hipStreamNonBlocking) == hipSuccess;
    for (int t = 0; t < 3 && ok; ++t) ok = hipEventCreateWithFlags(&ev[t], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
      for (auto e : ev)
        if (e) (void)hipEventDestroy(e);
      if (a) (void)hipStreamDestroy(a);
      return s;
    }
    c->aux = a;
    c->fork_ev = ev[0];
    c->prep_ev = ev[1];
    c->l1_ev = ev[2];
  }
  if (hipEventRecord(c->fork_ev, s) != hipSuccess || hipStreamWaitEvent(c->aux, c->fork_ev, 0) != hipSuccess) return s;
  return c->aux;
}

// after the pass was queued on ps: the point later consumers on the caller's stream join.
// Called after a failed pass too: the kernels already queued on ps are joined by the next call
// (or, when even the record fails, waited for here) before any buffer they read can be regrown.
hipError_t prepare_record(fia_ctx* c, hipStream_t ps, hipStream_t s) {
  if (ps == s) return hipSuccess;
  hipError_t e = hipEventRecord(c->prep_ev, ps);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ps);
    return e;
  }
  c->prep_pending = true;
  return hipSuccess;
}

hipError_t join_prepare(fia_ctx* c, hipStream_t s) {
  c->l1_pending = false;           // recorded before prep_ev on the same stream
  if (!c->prep_pending) return hipSuccess;
  FIA_HIP_TRY(hipStreamWaitEvent(s, c->prep_ev, 0));
  c->prep_pending = false;
  return hipSuccess;
}

hipError_t join_l1(fia_ctx* c, hipStream_t s) {
  if (!c->l1_pending) return join_prepare(c, s);
  FIA_HIP_TRY(hipStreamWaitEvent(s, c->l1_ev, 0));
  c->l1_pending = false;
  return hipSuccess;
}

}  // namespace fia

namespace {

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

int fail(fia_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

// the state every call that reads the caches needs: parameters, index, and a prepare since either changed
int check_prepared(fia_ctx* c) {
  if (!c->p.valid || !c->idx.valid) return fail(c, FIA_ERR_STATE, "params/index missing");
  if (!c->prepared) return fail(c, FIA_ERR_STATE, "fia_prepare has not been called since params/index changed");
  return FIA_OK;
}

int hip_fail(fia_ctx* c, hipError_t e, const char* where) {
  return fail(c, FIA_ERR_HIP, std::string(where) + ": " + hipGetErrorString(e));
}

#define FIA_GUARDED(ctx, ...)                                          \
  try {                                                                \
    __VA_ARGS__                                                        \
  } catch (const std::bad_alloc&) {                                    \
    return fail(ctx, FIA_ERR_NOMEM, "host allocation failed");         \
  } catch (...) {                                                      \
    return fail(ctx, FIA_ERR_INVALID, "unexpected internal exception"); \
  }

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Every stream-taking entry point starts here.  DevBuf regrows free their old block in
// order on the CALLING stream; when the caller switches streams, kernels of the previous
// call may still be queued on the old one, so that stream is synchronised first (rare: a
// context normally sees one stream).  Only the context's own previous stream is waited for
// -- never the whole device, which would also wait for (and, in global capture mode,
// invalidate a capture on) other contexts' streams.  A previous stream that is capturing
// cannot be synchronised; nothing of ours can be freed under it (DevBuf::reserve refuses to
// regrow during a capture).
// A capture cannot start while a Gram pass forked onto the context's aux stream by an eager
// fia_prepare / fia_prepare_for is still unjoined: the captured kernels would have no edge to
// it (an event recorded outside the capture is no graph dependency, and no host wait is legal
// inside a global-mode capture), so a replay could read Gram caches still being written.
// That call fails with FIA_ERR_STATE; a joining call (fia_query_batch or fia_prepare) on a
// non-capturing stream clears the condition.
int enter_stream(fia_ctx* c, hipStream_t s, const char* where) {
  hipStreamCaptureStatus ns = hipStreamCaptureStatusNone;
  const bool new_capturing = hipStreamIsCapturing(s, &ns) == hipSuccess && ns != hipStreamCaptureStatusNone;
  if (new_capturing && c->prep_pending)
    return fail(c, FIA_ERR_STATE,
                std::string(where) + ": a forked Gram pass of an earlier eager fia_prepare is not joined yet; "
                "call fia_query_batch (or fia_prepare) on a non-capturing stream before starting a capture");
  if (c->has_stream && c->stream != s) {
    if (hipError_t e = fia::join_prepare(c, c->stream); e != hipSuccess) return hip_fail(c, e, where);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    // a capture starting on a new stream (a graph captured after eager warm-up on another
    // stream): no synchronisation is legal inside a global-mode capture, and none is needed
    // -- nothing can be regrown, so nothing freed, while capturing; the caller has finished
    // the warm-up stream (fia.h)
    if (!new_capturing && hipStreamIsCapturing(c->stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) {
      if (hipError_t e = hipStreamSynchronize(c->stream); e != hipSuccess) return hip_fail(c, e, where);
    }
  }
  c->stream = s;
  c->has_stream = true;
  return FIA_OK;
}

// contexts alive per device (fia_create / fia_destroy)
constexpr int kMaxDevices = 64;
std::atomic<int> g_live[kMaxDevices];

}  // namespace

namespace fia {
int live_contexts(int device) { return device >= 0 && device < kMaxDevices ? g_live[device].load() : 1; }
}  // namespace fia

extern "C" {

int fia_version(void) { return 100; }

int fia_create(int device, fia_ctx** out) {
  if (!out) return FIA_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return FIA_ERR_HIP;
  if (device < 0 || device >= n) return FIA_ERR_INVALID;
  fia_ctx* c = new (std::nothrow) fia_ctx();
  if (!c) return FIA_ERR_NOMEM;
  c->device = device;
  if (device < kMaxDevices) g_live[device].fetch_add(1);
  *out = c;
  return FIA_OK;
}

int fia_destroy(fia_ctx* c) {
  if (!c) return FIA_OK;
  {
    DeviceGuard g(c->device);
    // Only the context's own streams are waited for -- never the whole device, which would
    // also wait for (and, in global capture mode, invalidate a capture on) other streams.
    // The buffers are freed in order on the context's stream, then that stream is synchronised
    // so the frees complete before the context goes.  A context that never saw a stream owns
    // no device buffer.  (Destroying a context while its stream is being captured leaves its
    // buffers to the pool: they cannot be freed inside someone else's capture.)
    const hipStream_t ds = c->has_stream ? c->stream : nullptr;
    hipStreamCaptureStatus dcs = hipStreamCaptureStatusNone;
    const bool capturing = c->has_stream && !(hipStreamIsCapturing(ds, &dcs) == hipSuccess &&
                                              dcs == hipStreamCaptureStatusNone);
    const bool can_free = c->has_stream && !capturing;
    // (inside a capture no host wait is legal: the aux stream, like the buffers, is left)
    if (c->aux && !capturing) (void)hipStreamSynchronize(c->aux);
    c->prep_pending = c->l1_pending = false;
    if (can_free) (void)hipStreamSynchronize(ds);
    auto rel = [&](fia::DevBuf& b) {
      if (can_free) b.release(ds);
      else { b.ptr = nullptr; b.bytes = 0; }
    };
    for (int s = 0; s < 2; ++s) {
      for (fia::DevBuf* b : {&c->idx.side[s].ptr, &c->idx.side[s].row, &c->idx.side[s].other, &c->idx.side[s].rating,
                             &c->gram[s], &c->l1[s], &c->idx.order[s], &c->idx.gitems[s], &c->idx.gcomb[s],
                             &c->gpart[s], &c->self[s], &c->gm[s], &c->slot[s], &c->bitems[s], &c->bcomb[s]})
        rel(*b);
    }
    fia::DevBuf* bufs[] = {&c->rec,    &c->coff,   &c->cdesc,    &c->cand_pos,  &c->cand_val, &c->qscan,
                           &c->flag,   &c->nch,    &c->coupled,  &c->idx.pkey,  &c->idx.pcnt, &c->idx.psum,
                           &c->gcnt,   &c->gstart, &c->grank,    &c->gq,        &c->qbase,    &c->gscan,
                           &c->wstart, &c->witems, &c->resid,  &c->qwork,  &c->xb,       &c->syslist,
                           &c->cpllist, &c->lscr, &c->mark, &c->d1tab, &c->slices, &c->wfrag,
                           &c->tkeys, &c->tvals, &c->tagg, &c->tslot, &c->tword, &c->tsort, &c->rowrec, &c->gxq,
                           &c->dwork, &c->dslab, &c->dpairs};
    for (auto* b : bufs) rel(*b);
    if (can_free) (void)hipStreamSynchronize(ds);   // the stream-ordered frees complete
    if (c->aux && !capturing) (void)hipStreamDestroy(c->aux);
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->l1_ev) (void)hipEventDestroy(c->l1_ev);
    if (c->prep_ev) (void)hipEventDestroy(c->prep_ev);
    for (auto& v : c->events.ev)
      for (auto& pr : v) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto e : c->events.pool) (void)hipEventDestroy(e);
  }
  if (c->device >= 0 && c->device < kMaxDevices) g_live[c->device].fetch_sub(1);
  delete c;
  return FIA_OK;
}

const char* fia_last_error(const fia_ctx* c) { return c ? c->err.c_str() : ""; }

int fia_num_params(const fia_ctx* c) {
  if (!c || !c->p.valid) return 0;
  return fia::model_num_params(c->p.model, c->p.k);
}

int fia_set_params(fia_ctx* c, int model, int k, int64_t U, int64_t I, const float* const* tables, int nptrs,
                   double wd, double damping) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    // a small-k Gram pass still queued on the aux stream reads the tables being replaced
    // (this call has no stream to order behind it: wait for the pass on the host)
    if (c->prep_pending && c->aux) {
      DeviceGuard g(c->device);
      if (hipError_t es = hipStreamSynchronize(c->aux); es != hipSuccess) return hip_fail(c, es, "fia_set_params");
      c->prep_pending = c->l1_pending = false;
    }
    if (model != FIA_MODEL_MF && model != FIA_MODEL_NCF) return fail(c, FIA_ERR_INVALID, "unknown model");
    const int need = model == FIA_MODEL_MF ? 5 : 10;
    if (!tables || nptrs != need) return fail(c, FIA_ERR_INVALID, "wrong number of parameter tables");
    for (int t = 0; t < need; ++t)
      if (!tables[t]) return fail(c, FIA_ERR_INVALID, "null parameter table");
    if (U <= 0 || I <= 0 || U >= (1LL << 31) || I >= (1LL << 31)) return fail(c, FIA_ERR_INVALID, "bad table sizes");
    if (!fia::model_supported(model, k))
      return fail(c, FIA_ERR_UNSUPPORTED, "embedding size " + std::to_string(k) + " not built for this model");
    if (!(wd >= 0.0) || !(damping >= 0.0)) return fail(c, FIA_ERR_INVALID, "weight_decay/damping must be >= 0");
    if (c->idx.valid && (c->idx.U != U || c->idx.I != I))
      return fail(c, FIA_ERR_INVALID, "num_users/num_items differ from the built index");
    c->p.model = model;
    c->p.k = k;
    c->p.U = U;
    c->p.I = I;
    for (int t = 0; t < 10; ++t) c->p.t[t] = t < need ? tables[t] : nullptr;
    c->p.wd = wd;
    c->p.damping = damping;
    c->p.valid = true;
    c->prepared = false;
    return FIA_OK;
  })
}

int fia_build_index(fia_ctx* c, int64_t N, int64_t U, int64_t I, const int32_t* user, const int32_t* item,
                    const float* rating, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    if (N < 0 || N >= (1LL << 31)) return fail(c, FIA_ERR_INVALID, "n_train out of range");
    if (U <= 0 || I <= 0 || U >= (1LL << 31) || I >= (1LL << 31)) return fail(c, FIA_ERR_INVALID, "bad entity counts");
    if (N > 0 && (!user || !item || !rating)) return fail(c, FIA_ERR_INVALID, "null training array");
    if (c->p.valid && (c->p.U != U || c->p.I != I))
      return fail(c, FIA_ERR_INVALID, "num_users/num_items differ from the registered params");
    DeviceGuard g(c->device);
    if (int rc = enter_stream(c, as_stream(stream), "fia_build_index"); rc != FIA_OK) return rc;
    if (hipError_t es = fia::join_prepare(c, as_stream(stream)); es != hipSuccess) return hip_fail(c, es, "fia_build_index");
    std::string why;
    hipError_t e = fia::build_index(c, N, U, I, user, item, rating, as_stream(stream), why);
    c->prepared = false;
    if (e != hipSuccess) {
      if (!why.empty()) return fail(c, FIA_ERR_INVALID, why);
      return hip_fail(c, e, "fia_build_index");
    }
    return FIA_OK;
  })
}

int fia_prepare(fia_ctx* c, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    if (!c->p.valid) return fail(c, FIA_ERR_STATE, "fia_set_params has not been called");
    if (!c->idx.valid) return fail(c, FIA_ERR_STATE, "fia_build_index has not been called");
    DeviceGuard g(c->device);
    hipStream_t s = as_stream(stream);
    if (int rc = enter_stream(c, s, "fia_prepare"); rc != FIA_OK) return rc;
    if (hipError_t es = fia::join_prepare(c, s); es != hipSuccess) return hip_fail(c, es, "fia_prepare");
    bool unsup = false;
    // small k: the Gram pass on the aux stream (the large-k prepare synchronises inside)
    const hipStream_t ps = fia::big_supported(c->p.model, c->p.k) ? s : fia::prepare_stream(c, s);
    fia::phase_begin(c, 0, ps);
    hipError_t e = fia::prepare_model(c, ps, unsup);
    fia::phase_end(c, 0, ps);
    if (hipError_t er = fia::prepare_record(c, ps, s); e == hipSuccess) e = er;
    c->prepared = false;
    if (unsup) return fail(c, FIA_ERR_UNSUPPORTED, "model/k not supported");
    if (e == hipErrorOutOfMemory) return fail(c, FIA_ERR_NOMEM, "device memory exhausted by the Hessian caches");
    if (e != hipSuccess) return hip_fail(c, e, "fia_prepare");
    c->prepared = true;
    return FIA_OK;
  })
}

int fia_prepare_for(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    if (!c->p.valid) return fail(c, FIA_ERR_STATE, "fia_set_params has not been called");
    if (!c->idx.valid) return fail(c, FIA_ERR_STATE, "fia_build_index has not been called");
    if (Q < 0 || Q >= (1LL << 31)) return fail(c, FIA_ERR_INVALID, "num_queries out of range");
    if (Q > 0 && (!qu || !qi)) return fail(c, FIA_ERR_INVALID, "null query array");
    DeviceGuard g(c->device);
    hipStream_t s = as_stream(stream);
    if (int rc = enter_stream(c, s, "fia_prepare_for"); rc != FIA_OK) return rc;
    // the marks below are read by a still-queued Gram pass
    if (hipError_t es = fia::join_prepare(c, s); es != hipSuccess) return hip_fail(c, es, "fia_prepare_for");
    bool unsup = false;
    hipError_t e;
    if (fia::big_supported(c->p.model, c->p.k)) {
      fia::phase_begin(c, 0, s);
      e = fia::prepare_big(c, Q, qu, qi, s);
      fia::phase_end(c, 0, s);
    } else {
      // small k: entities marked on s (no sync), their Gram caches on the aux stream
      fia::phase_begin(c, 0, s);
      e = fia::prepare_model_for(c, Q, qu, qi, s, s, unsup, true);
      const hipStream_t ps = e == hipSuccess ? fia::prepare_stream(c, s) : s;
      if (e == hipSuccess && !unsup) e = fia::prepare_model_for(c, Q, qu, qi, s, ps, unsup, false);
      fia::phase_end(c, 0, ps);
      if (hipError_t er = fia::prepare_record(c, ps, s); e == hipSuccess) e = er;
    }
    c->prepared = false;
    if (unsup) return fail(c, FIA_ERR_UNSUPPORTED, "model/k not supported");
    if (e == hipErrorOutOfMemory) return fail(c, FIA_ERR_NOMEM, "device memory exhausted by the Hessian caches");
    if (e != hipSuccess) return hip_fail(c, e, "fia_prepare_for");
    c->prepared = true;
    return FIA_OK;
  })
}

int fia_count_related(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, int64_t* offsets,
                      int64_t* total_out, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    if (!c->idx.valid) return fail(c, FIA_ERR_STATE, "fia_build_index has not been called");
    if (Q < 0 || Q >= (1LL << 31)) return fail(c, FIA_ERR_INVALID, "num_queries out of range");
    if (!offsets || (Q > 0 && (!qu || !qi))) return fail(c, FIA_ERR_INVALID, "null query array");
    DeviceGuard g(c->device);
    hipStream_t s = as_stream(stream);
    if (int rc = enter_stream(c, s, "fia_count_related"); rc != FIA_OK) return rc;
    hipError_t e = hipSuccess;
    if (total_out) {
      e = c->flag.reserve(64, s);
      if (e != hipSuccess) return hip_fail(c, e, "fia_count_related");
      e = hipMemsetAsync(c->flag.ptr, 0, 64, s);
      if (e != hipSuccess) return hip_fail(c, e, "fia_count_related");
    }
    e = fia::count_related(c, Q, qu, qi, offsets, s);
    if (e == hipSuccess && total_out) e = fia::check_cover(c, Q, qu, qi, c->flag.as<int32_t>() + 2, s);
    if (e == hipSuccess && total_out) e = fia::check_cover_small(c, Q, qu, qi, c->flag.as<int32_t>() + 2, s);
    if (e != hipSuccess) return hip_fail(c, e, "fia_count_related");
    if (total_out) {
      int32_t flags[4] = {0, 0, 0, 0};
      e = hipMemcpyAsync(total_out, offsets + Q, sizeof(int64_t), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipMemcpyAsync(flags, c->flag.ptr, sizeof(flags), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) return hip_fail(c, e, "fia_count_related");
      if (flags[1]) return fail(c, FIA_ERR_INVALID, "query ids out of range [0, num_users) x [0, num_items)");
      if (flags[2])
        return fail(c, FIA_ERR_STATE, "a query's user or item has no Hessian cache: it was not among the "
                                      "queries of the last fia_prepare_for");
    }
    return FIA_OK;
  })
}

int fia_related(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                int32_t* rel_idx, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    if (!c->idx.valid) return fail(c, FIA_ERR_STATE, "fia_build_index has not been called");
    if (Q < 0 || Q >= (1LL << 31)) return fail(c, FIA_ERR_INVALID, "num_queries out of range");
    if (Q > 0 && (!qu || !qi || !offsets || !rel_idx)) return fail(c, FIA_ERR_INVALID, "null array");
    DeviceGuard g(c->device);
    if (int rc = enter_stream(c, as_stream(stream), "fia_related"); rc != FIA_OK) return rc;
    hipError_t e = fia::write_related(c, Q, qu, qi, offsets, rel_idx, as_stream(stream));
    if (e != hipSuccess) return hip_fail(c, e, "fia_related");
    return FIA_OK;
  })
}

static int query_batch_common(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                              int64_t total_rel, int32_t* rel_idx, double* influence, double* x_out, int K,
                              int64_t* topk_pos, int64_t* topk_idx, double* topk_val, void* stream,
                              const double* x_in) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    if (int rc = check_prepared(c); rc != FIA_OK) return rc;
    if (Q < 0 || Q >= (1LL << 31)) return fail(c, FIA_ERR_INVALID, "num_queries out of range");
    if (total_rel < 0) return fail(c, FIA_ERR_INVALID, "total_rel < 0");
    if (K < 0 || K > FIA_MAX_TOPK) return fail(c, FIA_ERR_INVALID, "K must be in [0, FIA_MAX_TOPK]");
    if (Q > 0 && (!qu || !qi || !offsets)) return fail(c, FIA_ERR_INVALID, "null query array");
    if (K > 0 && (!topk_pos || !topk_idx || !topk_val)) return fail(c, FIA_ERR_INVALID, "null top-K output");
    if (Q == 0) return FIA_OK;
    // MF k in {32, 64}, K <= 1 (k_score_mf_mfma) keeps its output offsets and candidate slots
    // in 32 bits.  A stored element is el = ob0 + idx with ob0 the run's first element and
    // idx < the run's length, computed modulo 2^32 in a uint32_t: every stored el is
    // < total_rel, so total_rel <= 2^32 is exact.  A candidate slot is an int32_t: slot base +
    // chunk of the list, below the batch's chunk count sum_q ceil(|R_u| / kChunk) +
    // ceil(|C_i| / kChunk) <= 2 Q + total_rel / kChunk, which must stay <= 2^31 - 1.
    if (c->p.model == FIA_MODEL_MF && (c->p.k == 32 || c->p.k == 64) && K <= 1) {
      if (total_rel > FIA_MFMA_MAX_TOTAL_REL)
        return fail(c, FIA_ERR_INVALID, "total_rel > 2^32: split the batch (MF k in {32, 64}, K <= 1)");
      if (2 * Q + total_rel / fia::kChunk > FIA_MFMA_MAX_CHUNKS)
        return fail(c, FIA_ERR_INVALID, "more than 2^31 - 1 list chunks: split the batch (MF k in {32, 64}, K <= 1)");
    }
    DeviceGuard g(c->device);
    if (int rc = enter_stream(c, as_stream(stream), "fia_query_batch"); rc != FIA_OK) return rc;
    // (small k joins the pending Gram pass right before its solve, after the query scans)
    if (fia::big_supported(c->p.model, c->p.k))
      if (hipError_t es = fia::join_prepare(c, as_stream(stream)); es != hipSuccess) return hip_fail(c, es, "fia_query_batch");
    // chunk descriptors / candidate slots: at most 2 per query + one per chunk of the model's
    // shortest chunk length (NCF k <= 16 runs: kNcfRunChunk; else kRunChunk).  (A tighter bound
    // also keeps ml-1m-ex's top-K merge on its thread-per-query kernel.)
    const int64_t clen = c->p.model == FIA_MODEL_NCF && c->p.k <= 16 ? fia::kNcfRunChunk : fia::kRunChunk;
    const int64_t max_chunks = 2 * Q + total_rel / clen + 1;
    bool unsup = false;
    hipError_t e = fia::query_model(c, Q, qu, qi, offsets, max_chunks, rel_idx, influence, x_out, K, topk_pos,
                                    topk_idx, topk_val, as_stream(stream), unsup, x_in);
    if (unsup) return fail(c, FIA_ERR_UNSUPPORTED, "model/k not supported");
    if (e != hipSuccess) return hip_fail(c, e, "fia_query_batch");
    return FIA_OK;
  })
}

int fia_query_batch(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                    int64_t total_rel, int32_t* rel_idx, double* influence, double* x_out, int K,
                    int64_t* topk_pos, int64_t* topk_idx, double* topk_val, void* stream) {
  return query_batch_common(c, Q, qu, qi, offsets, total_rel, rel_idx, influence, x_out, K, topk_pos, topk_idx,
                            topk_val, stream, nullptr);
}

int fia_query_batch_x(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                      int64_t total_rel, const double* x_in, int32_t* rel_idx, double* influence, int K,
                      int64_t* topk_pos, int64_t* topk_idx, double* topk_val, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  if (Q > 0 && !x_in) return fail(c, FIA_ERR_INVALID, "null x_in");
  return query_batch_common(c, Q, qu, qi, offsets, total_rel, rel_idx, influence, nullptr, K, topk_pos, topk_idx,
                            topk_val, stream, x_in);
}

int fia_score_candidates(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const double* x,
                         const int64_t* cand_offsets, int64_t total_cand, const int32_t* cand_user,
                         const int32_t* cand_item, const float* cand_rating, double* influence, int K,
                         int64_t* topk_pos, double* topk_val, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    if (int rc = check_prepared(c); rc != FIA_OK) return rc;
    if (Q < 0 || Q >= (1LL << 31)) return fail(c, FIA_ERR_INVALID, "num_queries out of range");
    if (total_cand < 0) return fail(c, FIA_ERR_INVALID, "total_cand < 0");
    // a candidate's position inside its query's list is kept in 32 bits by the top-K selection
    // (element offsets into the candidate and influence arrays are 64-bit)
    if (total_cand > FIA_CAND_MAX_TOTAL)
      return fail(c, FIA_ERR_INVALID, "total_cand > 2^31 - 1: split the batch");
    if (K < 0 || K > FIA_MAX_TOPK) return fail(c, FIA_ERR_INVALID, "K must be in [0, FIA_MAX_TOPK]");
    if (Q > 0 && (!qu || !qi || !x || !cand_offsets)) return fail(c, FIA_ERR_INVALID, "null query array");
    if (total_cand > 0 && (!cand_user || !cand_item || !cand_rating))
      return fail(c, FIA_ERR_INVALID, "null candidate array");
    if (K > 0 && (!topk_pos || !topk_val)) return fail(c, FIA_ERR_INVALID, "null top-K output");
    if (Q == 0) return FIA_OK;
    if (!fia::model_supported(c->p.model, c->p.k)) return fail(c, FIA_ERR_UNSUPPORTED, "model/k not supported");
    DeviceGuard g(c->device);
    hipStream_t s = as_stream(stream);
    if (int rc = enter_stream(c, s, "fia_score_candidates"); rc != FIA_OK) return rc;
    // of what a pending small-k Gram pass writes, only the NCF layer-1 rows are read here (its
    // first kernels: l1_ev; once that is joined on this stream nothing else is waited for)
    if (c->p.model == FIA_MODEL_NCF && c->l1_pending)
      if (hipError_t es = fia::join_l1(c, s); es != hipSuccess) return hip_fail(c, es, "fia_score_candidates");
    hipError_t e = fia::score_candidates(c, Q, qu, qi, x, cand_offsets, total_cand, cand_user, cand_item,
                                         cand_rating, influence, K, topk_pos, topk_val, s);
    if (e != hipSuccess) return hip_fail(c, e, "fia_score_candidates");
    return FIA_OK;
  })
}

int fia_total_influence(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const double* x, double* total,
                        int32_t* count, int K, int64_t* topk_idx, double* topk_val, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    // the batch bound comes first: nothing of an oversized batch is looked at
    if (Q < 0 || Q > FIA_TOTAL_MAX_QUERIES)
      return fail(c, FIA_ERR_INVALID, "num_queries out of range [0, 2^30]: split the batch (totals add)");
    if (int rc = check_prepared(c); rc != FIA_OK) return rc;
    if (K < 0 || K > FIA_MAX_TOPK) return fail(c, FIA_ERR_INVALID, "K must be in [0, FIA_MAX_TOPK]");
    if (K > 0 && (!topk_idx || !topk_val)) return fail(c, FIA_ERR_INVALID, "null top-K output");
    if (!total && !count && K == 0) return fail(c, FIA_ERR_INVALID, "no output requested (total, count, top-K)");
    if (Q > 0 && (!qu || !qi || !x)) return fail(c, FIA_ERR_INVALID, "null query array");
    if (!fia::model_supported(c->p.model, c->p.k)) return fail(c, FIA_ERR_UNSUPPORTED, "model/k not supported");
    DeviceGuard g(c->device);
    hipStream_t s = as_stream(stream);
    if (int rc = enter_stream(c, s, "fia_total_influence"); rc != FIA_OK) return rc;
    // as fia_score_candidates: of a pending small-k Gram pass only the NCF layer-1 rows are read
    if (c->p.model == FIA_MODEL_NCF && c->l1_pending)
      if (hipError_t es = fia::join_l1(c, s); es != hipSuccess) return hip_fail(c, es, "fia_total_influence");
    hipError_t e = fia::total_influence(c, Q, qu, qi, x, total, count, K, topk_idx, topk_val, s);
    if (e != hipSuccess) return hip_fail(c, e, "fia_total_influence");
    return FIA_OK;
  })
}

int fia_group_influence(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* grp_offsets,
                        int64_t num_groups, const int64_t* mem_offsets, int64_t total_members, const int32_t* mem_row,
                        double* group, double* first_order, double* dtheta, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    // the batch bounds come first: nothing of an oversized batch is looked at
    if (Q < 0 || Q >= (1LL << 31)) return fail(c, FIA_ERR_INVALID, "num_queries out of range");
    if (num_groups < 0 || num_groups > FIA_GROUP_MAX_GROUPS)
      return fail(c, FIA_ERR_INVALID, "num_groups out of range [0, 2^31 - 1]: split the batch");
    if (total_members < 0 || total_members > FIA_GROUP_MAX_MEMBERS)
      return fail(c, FIA_ERR_INVALID, "total_members out of range [0, 2^31 - 1]: split the batch");
    if (int rc = check_prepared(c); rc != FIA_OK) return rc;
    if (!group && !first_order && !dtheta)
      return fail(c, FIA_ERR_INVALID, "no output requested (group, first_order, dtheta)");
    if (Q == 0 || num_groups == 0) return FIA_OK;
    if (!qu || !qi || !grp_offsets || !mem_offsets) return fail(c, FIA_ERR_INVALID, "null query or offset array");
    if (total_members > 0 && !mem_row) return fail(c, FIA_ERR_INVALID, "null member array");
    // small k: the full packed system in LDS (group.hip); large k: in device memory (group_big.hip)
    const bool big = fia::big_supported(c->p.model, c->p.k);
    if (!big && !fia::group_supported(c->p.model, c->p.k))
      return fail(c, FIA_ERR_UNSUPPORTED,
                  "fia_group_influence is built for MF k in {8, 16, 32, 64, 128, 256} and NCF k in {8, 16, 32, 64, "
                  "128, 256}");
    DeviceGuard g(c->device);
    hipStream_t s = as_stream(stream);
    if (int rc = enter_stream(c, s, "fia_group_influence"); rc != FIA_OK) return rc;
    // the Gram caches of a pending small-k pass are read: join it, as fia_query_batch's solve does
    if (hipError_t es = fia::join_prepare(c, s); es != hipSuccess) return hip_fail(c, es, "fia_group_influence");
    // (large k after fia_prepare_for: a query outside the cover gets n = 0 from the prologue, as in
    // fia_query_batch, and its groups NaN before any member is read; fia_count_related with a total
    // is the call that refuses such a batch)
    hipError_t e = big ? fia::group_influence_big(c, Q, qu, qi, grp_offsets, num_groups, mem_offsets, total_members,
                                                  mem_row, group, first_order, dtheta, s)
                       : fia::group_influence(c, Q, qu, qi, grp_offsets, num_groups, mem_offsets, total_members,
                                              mem_row, group, first_order, dtheta, s);
    if (e != hipSuccess) return hip_fail(c, e, "fia_group_influence");
    return FIA_OK;
  })
}

int fia_self_influence(fia_ctx* c, int64_t num_rows, const int32_t* rows, double* first_order, double* newton,
                       double* error, int K, int64_t* topk_pos, int64_t* topk_idx, double* topk_val, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    // the batch bound comes first: nothing of an oversized batch is looked at
    if (num_rows < 0 || num_rows > FIA_SELF_MAX_ROWS)
      return fail(c, FIA_ERR_INVALID, "num_rows out of range [0, 2^31 - 1]: split the batch");
    if (int rc = check_prepared(c); rc != FIA_OK) return rc;
    if (c->subset || c->small_subset)
      return fail(c, FIA_ERR_STATE,
                  "fia_self_influence needs the caches of every entity: the last prepare was fia_prepare_for "
                  "(a partial cover); call fia_prepare");
    if (K < 0 || K > FIA_MAX_TOPK) return fail(c, FIA_ERR_INVALID, "K must be in [0, FIA_MAX_TOPK]");
    if (K > 0 && (!topk_pos || !topk_idx || !topk_val)) return fail(c, FIA_ERR_INVALID, "null top-K output");
    if (!first_order && !newton && !error && K == 0)
      return fail(c, FIA_ERR_INVALID, "no output requested (first_order, newton, error, top-K)");
    DeviceGuard g(c->device);
    hipStream_t s = as_stream(stream);
    if (num_rows == 0) {
      if (K == 0) return FIA_OK;
      if (int rc = enter_stream(c, s, "fia_self_influence"); rc != FIA_OK) return rc;
      hipError_t e = fia::self_influence(c, 0, nullptr, nullptr, nullptr, nullptr, K, topk_pos, topk_idx, topk_val, s);
      if (e != hipSuccess) return hip_fail(c, e, "fia_self_influence");
      return FIA_OK;
    }
    if (!rows && num_rows != c->idx.N)
      return fail(c, FIA_ERR_INVALID, "rows is NULL (every train row): num_rows must equal n_train");
    // (self_influence takes the large-k sizes to group_big.hip)
    if (!fia::group_supported(c->p.model, c->p.k) && !fia::big_supported(c->p.model, c->p.k))
      return fail(c, FIA_ERR_UNSUPPORTED,
                  "fia_self_influence is built for MF k in {8, 16, 32, 64, 128, 256} and NCF k in {8, 16, 32, 64, "
                  "128, 256}");
    if (int rc = enter_stream(c, s, "fia_self_influence"); rc != FIA_OK) return rc;
    // the Gram caches of a pending small-k pass are read: join it, as fia_group_influence does
    if (hipError_t es = fia::join_prepare(c, s); es != hipSuccess) return hip_fail(c, es, "fia_self_influence");
    hipError_t e = fia::self_influence(c, num_rows, rows, first_order, newton, error, K, topk_pos, topk_idx, topk_val, s);
    if (e != hipSuccess) return hip_fail(c, e, "fia_self_influence");
    return FIA_OK;
  })
}

int fia_query_batch_newton(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                           int64_t total_rel, int32_t* rel_idx, double* newton, int K, int64_t* topk_pos,
                           int64_t* topk_idx, double* topk_val, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    if (int rc = check_prepared(c); rc != FIA_OK) return rc;
    if (Q < 0 || Q >= (1LL << 31)) return fail(c, FIA_ERR_INVALID, "num_queries out of range");
    if (total_rel < 0) return fail(c, FIA_ERR_INVALID, "total_rel < 0");
    if (K < 0 || K > FIA_MAX_TOPK) return fail(c, FIA_ERR_INVALID, "K must be in [0, FIA_MAX_TOPK]");
    if (Q > 0 && (!qu || !qi || !offsets)) return fail(c, FIA_ERR_INVALID, "null query array");
    if (K > 0 && (!topk_pos || !topk_idx || !topk_val)) return fail(c, FIA_ERR_INVALID, "null top-K output");
    if (Q == 0) return FIA_OK;
    if (!fia::newton_supported(c->p.model, c->p.k))
      return fail(c, FIA_ERR_UNSUPPORTED,
                  "fia_query_batch_newton is built for MF k in {8, 16, 32, 64} and NCF k in {8, 16, 32}; the large-k "
                  "models are not supported yet");
    DeviceGuard g(c->device);
    hipStream_t s = as_stream(stream);
    if (int rc = enter_stream(c, s, "fia_query_batch_newton"); rc != FIA_OK) return rc;
    // the Gram caches of a pending small-k pass are read: join it, as fia_group_influence does
    if (hipError_t es = fia::join_prepare(c, s); es != hipSuccess) return hip_fail(c, es, "fia_query_batch_newton");
    hipError_t e = fia::query_newton(c, Q, qu, qi, offsets, total_rel, rel_idx, newton, K, topk_pos, topk_idx,
                                     topk_val, s);
    if (e != hipSuccess) return hip_fail(c, e, "fia_query_batch_newton");
    return FIA_OK;
  })
}

int fia_score_candidates_newton(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi,
                                const int64_t* cand_offsets, int64_t total_cand, const int32_t* cand_user,
                                const int32_t* cand_item, const float* cand_rating, double* newton_add, int K,
                                int64_t* topk_pos, double* topk_val, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    if (int rc = check_prepared(c); rc != FIA_OK) return rc;
    // (2 Q + 3 sort keys in 32 bits)
    if (Q < 0 || Q > FIA_CAND_NEWTON_MAX_QUERIES) return fail(c, FIA_ERR_INVALID, "num_queries out of range [0, 2^30]");
    if (total_cand < 0) return fail(c, FIA_ERR_INVALID, "total_cand < 0");
    // a candidate's position is kept in 32 bits by the partition and by the top-K selection
    if (total_cand > FIA_CAND_MAX_TOTAL)
      return fail(c, FIA_ERR_INVALID, "total_cand > 2^31 - 1: split the batch");
    if (K < 0 || K > FIA_MAX_TOPK) return fail(c, FIA_ERR_INVALID, "K must be in [0, FIA_MAX_TOPK]");
    if (Q > 0 && (!qu || !qi || !cand_offsets)) return fail(c, FIA_ERR_INVALID, "null query array");
    if (total_cand > 0 && (!cand_user || !cand_item || !cand_rating))
      return fail(c, FIA_ERR_INVALID, "null candidate array");
    if (K > 0 && (!topk_pos || !topk_val)) return fail(c, FIA_ERR_INVALID, "null top-K output");
    if (!newton_add && K == 0) return fail(c, FIA_ERR_INVALID, "no output requested (newton_add, top-K)");
    if (Q == 0) return FIA_OK;
    if (!fia::newton_supported(c->p.model, c->p.k))
      return fail(c, FIA_ERR_UNSUPPORTED,
                  "fia_score_candidates_newton is built for MF k in {8, 16, 32, 64} and NCF k in {8, 16, 32}; the "
                  "large-k models are not supported yet");
    DeviceGuard g(c->device);
    hipStream_t s = as_stream(stream);
    if (int rc = enter_stream(c, s, "fia_score_candidates_newton"); rc != FIA_OK) return rc;
    // the Gram caches of a pending small-k pass are read: join it, as fia_query_batch_newton does
    if (hipError_t es = fia::join_prepare(c, s); es != hipSuccess)
      return hip_fail(c, es, "fia_score_candidates_newton");
    hipError_t e = fia::score_candidates_newton(c, Q, qu, qi, cand_offsets, total_cand, cand_user, cand_item,
                                                cand_rating, newton_add, K, topk_pos, topk_val, s);
    if (e != hipSuccess) return hip_fail(c, e, "fia_score_candidates_newton");
    return FIA_OK;
  })
}

int fia_edit_influence(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* grp_offsets,
                       int64_t num_groups, const int64_t* rem_offsets, int64_t total_rem, const int32_t* rem_row,
                       const int64_t* add_offsets, int64_t total_add, const int32_t* add_user, const int32_t* add_item,
                       const float* add_rating, double* edit, double* first_order, double* dtheta, int K,
                       int64_t* topk_pos, double* topk_val, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    // the batch bounds come first: nothing of an oversized batch is looked at
    if (Q < 0 || Q >= (1LL << 31)) return fail(c, FIA_ERR_INVALID, "num_queries out of range");
    if (num_groups < 0 || num_groups > FIA_EDIT_MAX_GROUPS)
      return fail(c, FIA_ERR_INVALID, "num_groups out of range [0, 2^31 - 1]: split the batch");
    if (total_rem < 0 || total_rem > FIA_EDIT_MAX_MEMBERS)
      return fail(c, FIA_ERR_INVALID, "total_rem out of range [0, 2^31 - 1]: split the batch");
    if (total_add < 0 || total_add > FIA_EDIT_MAX_MEMBERS)
      return fail(c, FIA_ERR_INVALID, "total_add out of range [0, 2^31 - 1]: split the batch");
    if (int rc = check_prepared(c); rc != FIA_OK) return rc;
    if (K < 0 || K > FIA_MAX_TOPK) return fail(c, FIA_ERR_INVALID, "K must be in [0, FIA_MAX_TOPK]");
    if (K > 0 && (!topk_pos || !topk_val)) return fail(c, FIA_ERR_INVALID, "null top-K output");
    if (!edit && !first_order && !dtheta && K == 0)
      return fail(c, FIA_ERR_INVALID, "no output requested (edit, first_order, dtheta, top-K)");
    if (Q == 0 || (num_groups == 0 && K == 0)) return FIA_OK;
    if (!qu || !qi || !grp_offsets) return fail(c, FIA_ERR_INVALID, "null query or offset array");
    if (num_groups > 0 && (!rem_offsets || !add_offsets)) return fail(c, FIA_ERR_INVALID, "null member offset array");
    if (total_rem > 0 && !rem_row) return fail(c, FIA_ERR_INVALID, "null removal array");
    if (total_add > 0 && (!add_user || !add_item || !add_rating))
      return fail(c, FIA_ERR_INVALID, "null addition array");
    if (!fia::group_supported(c->p.model, c->p.k))
      return fail(c, FIA_ERR_UNSUPPORTED,
                  "fia_edit_influence is built for MF k in {8, 16, 32, 64} and NCF k in {8, 16, 32}; the large-k "
                  "models are not supported yet");
    DeviceGuard g(c->device);
    hipStream_t s = as_stream(stream);
    if (int rc = enter_stream(c, s, "fia_edit_influence"); rc != FIA_OK) return rc;
    // the Gram caches of a pending small-k pass are read: join it, as fia_group_influence does
    if (hipError_t es = fia::join_prepare(c, s); es != hipSuccess) return hip_fail(c, es, "fia_edit_influence");
    hipError_t e = fia::edit_influence(c, Q, qu, qi, grp_offsets, num_groups, rem_offsets, total_rem, rem_row,
                                       add_offsets, total_add, add_user, add_item, add_rating, edit, first_order,
                                       dtheta, K, topk_pos, topk_val, s);
    if (e != hipSuccess) return hip_fail(c, e, "fia_edit_influence");
    return FIA_OK;
  })
}

int fia_count_related_pair(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int32_t* qj,
                           int64_t* offsets, int64_t* total_out, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    if (!c->idx.valid) return fail(c, FIA_ERR_STATE, "fia_build_index has not been called");
    if (Q < 0 || Q >= (1LL << 31)) return fail(c, FIA_ERR_INVALID, "num_queries out of range");
    if (!offsets || (Q > 0 && (!qu || !qi || !qj))) return fail(c, FIA_ERR_INVALID, "null query array");
    DeviceGuard g(c->device);
    hipStream_t s = as_stream(stream);
    if (int rc = enter_stream(c, s, "fia_count_related_pair"); rc != FIA_OK) return rc;
    hipError_t e = hipSuccess;
    if (total_out) {
      e = c->flag.reserve(64, s);
      if (e != hipSuccess) return hip_fail(c, e, "fia_count_related_pair");
      e = hipMemsetAsync(c->flag.ptr, 0, 64, s);
      if (e != hipSuccess) return hip_fail(c, e, "fia_count_related_pair");
    }
    e = fia::count_related_pair(c, Q, qu, qi, qj, offsets, s);
    // the cover of both pairs: (u, i) and (u, j)
    for (const int32_t* it : {qi, qj}) {
      if (e == hipSuccess && total_out) e = fia::check_cover(c, Q, qu, it, c->flag.as<int32_t>() + 2, s);
      if (e == hipSuccess && total_out) e = fia::check_cover_small(c, Q, qu, it, c->flag.as<int32_t>() + 2, s);
    }
    if (e != hipSuccess) return hip_fail(c, e, "fia_count_related_pair");
    if (total_out) {
      int32_t flags[4] = {0, 0, 0, 0};
      e = hipMemcpyAsync(total_out, offsets + Q, sizeof(int64_t), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipMemcpyAsync(flags, c->flag.ptr, sizeof(flags), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) return hip_fail(c, e, "fia_count_related_pair");
      if (flags[1]) return fail(c, FIA_ERR_INVALID, "query ids out of range [0, num_users) x [0, num_items)");
      if (flags[2])
        return fail(c, FIA_ERR_STATE, "a query's user or one of its two items has no Hessian cache: it was not among "
                                      "the queries of the last fia_prepare_for");
    }
    return FIA_OK;
  })
}

int fia_pair_batch(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int32_t* qj,
                   const int64_t* offsets, int64_t total_rel, int32_t* rel_idx, double* influence, double* x_out,
                   double* diff, int K, int64_t* topk_pos, int64_t* topk_idx, double* topk_val, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    // the batch bounds come first: nothing of an oversized batch is looked at
    if (Q < 0 || Q > FIA_PAIR_MAX_QUERIES)
      return fail(c, FIA_ERR_INVALID, "num_queries out of range [0, 2^30]: split the batch");
    // a rating's position inside its query's related list is kept in 32 bits by the top-K selection
    if (total_rel < 0 || total_rel > FIA_PAIR_MAX_TOTAL_REL)
      return fail(c, FIA_ERR_INVALID, "total_rel out of range [0, 2^31 - 1]: split the batch");
    if (int rc = check_prepared(c); rc != FIA_OK) return rc;
    if (K < 0 || K > FIA_MAX_TOPK) return fail(c, FIA_ERR_INVALID, "K must be in [0, FIA_MAX_TOPK]");
    if (K > 0 && (!topk_pos || !topk_idx || !topk_val)) return fail(c, FIA_ERR_INVALID, "null top-K output");
    if (!rel_idx && !influence && !x_out && !diff && K == 0)
      return fail(c, FIA_ERR_INVALID, "no output requested (rel_idx, influence, x_out, diff, top-K)");
    if (Q == 0) return FIA_OK;
    if (!qu || !qi || !qj || !offsets) return fail(c, FIA_ERR_INVALID, "null query or offset array");
    if (!fia::pair_supported(c->p.model, c->p.k))
      return fail(c, FIA_ERR_UNSUPPORTED,
                  "fia_pair_batch is built for MF k in {8, 16, 32} and NCF k in {8, 16} (the three-block system in "
                  "one workgroup's LDS); MF k = 64, NCF k = 32 and the large-k models are not supported yet");
    DeviceGuard g(c->device);
    hipStream_t s = as_stream(stream);
    if (int rc = enter_stream(c, s, "fia_pair_batch"); rc != FIA_OK) return rc;
    // the Gram caches of a pending small-k pass are read: join it, as fia_group_influence does
    if (hipError_t es = fia::join_prepare(c, s); es != hipSuccess) return hip_fail(c, es, "fia_pair_batch");
    hipError_t e = fia::pair_batch(c, Q, qu, qi, qj, offsets, total_rel, rel_idx, influence, x_out, diff, K, topk_pos,
                                   topk_idx, topk_val, s);
    if (e != hipSuccess) return hip_fail(c, e, "fia_pair_batch");
    return FIA_OK;
  })
}

int fia_pair_flip(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int32_t* qj, const double* margin,
                  int max_set, int32_t* set_size, int32_t* set_row, double* set_val, double* first_order,
                  double* newton, double* dtheta, double* diff, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    // the batch bounds come first: nothing of an oversized batch is looked at
    if (Q < 0 || Q > FIA_PAIR_MAX_QUERIES)
      return fail(c, FIA_ERR_INVALID, "num_queries out of range [0, 2^30]: split the batch");
    if (max_set < 1 || max_set > FIA_FLIP_MAX_SET)
      return fail(c, FIA_ERR_INVALID, "max_set must be in [1, FIA_FLIP_MAX_SET]");
    if (int rc = check_prepared(c); rc != FIA_OK) return rc;
    if (!set_size && !set_row && !set_val && !first_order && !newton && !dtheta && !diff)
      return fail(c, FIA_ERR_INVALID,
                  "no output requested (set_size, set_row, set_val, first_order, newton, dtheta, diff)");
    if (Q == 0) return FIA_OK;
    if (!qu || !qi || !qj) return fail(c, FIA_ERR_INVALID, "null query array");
    if (!fia::pair_supported(c->p.model, c->p.k))
      return fail(c, FIA_ERR_UNSUPPORTED,
                  "fia_pair_flip is built for MF k in {8, 16, 32} and NCF k in {8, 16} (the three-block system in "
                  "one workgroup's LDS); MF k = 64, NCF k = 32 and the large-k models are not supported yet");
    DeviceGuard g(c->device);
    hipStream_t s = as_stream(stream);
    if (int rc = enter_stream(c, s, "fia_pair_flip"); rc != FIA_OK) return rc;
    // the Gram caches of a pending small-k pass are read: join it, as fia_pair_batch does
    if (hipError_t es = fia::join_prepare(c, s); es != hipSuccess) return hip_fail(c, es, "fia_pair_flip");
    hipError_t e = fia::pair_flip(c, Q, qu, qi, qj, margin, max_set, set_size, set_row, set_val, first_order, newton,
                                  dtheta, diff, s);
    if (e != hipSuccess) return hip_fail(c, e, "fia_pair_flip");
    return FIA_OK;
  })
}

int fia_count_related_slate(fia_ctx* c, int64_t Q, const int32_t* qu, const int64_t* slate_offsets,
                            int64_t total_items, const int32_t* slate_item, int64_t* offsets, int64_t* total_out,
                            void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    if (!c->idx.valid) return fail(c, FIA_ERR_STATE, "fia_build_index has not been called");
    if (Q < 0 || Q > FIA_SLATE_MAX_TOTAL_ITEMS) return fail(c, FIA_ERR_INVALID, "num_queries out of range");
    if (total_items < 0 || total_items > FIA_SLATE_MAX_TOTAL_ITEMS)
      return fail(c, FIA_ERR_INVALID, "total_items out of range [0, 2^30]: split the batch");
    if (!offsets || (Q > 0 && (!qu || !slate_offsets)) || (total_items > 0 && !slate_item))
      return fail(c, FIA_ERR_INVALID, "null query array");
    DeviceGuard g(c->device);
    hipStream_t s = as_stream(stream);
    if (int rc = enter_stream(c, s, "fia_count_related_slate"); rc != FIA_OK) return rc;
    hipError_t e = hipSuccess;
    if (total_out) {
      e = c->flag.reserve(64, s);
      if (e != hipSuccess) return hip_fail(c, e, "fia_count_related_slate");
      e = hipMemsetAsync(c->flag.ptr, 0, 64, s);
      if (e != hipSuccess) return hip_fail(c, e, "fia_count_related_slate");
    }
    // (the scan checks the cover of u and of every slate item itself)
    e = fia::count_related_slate(c, Q, qu, slate_offsets, total_items, slate_item, offsets, total_out != nullptr, s);
    if (e != hipSuccess) return hip_fail(c, e, "fia_count_related_slate");
    if (total_out) {
      int32_t flags[4] = {0, 0, 0, 0};
      e = hipMemcpyAsync(total_out, offsets + Q, sizeof(int64_t), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipMemcpyAsync(flags, c->flag.ptr, sizeof(flags), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) return hip_fail(c, e, "fia_count_related_slate");
      if (flags[1])
        return fail(c, FIA_ERR_INVALID, "a slate's ids are out of range [0, num_users) x [0, num_items), it repeats an "
                                        "item or its length is outside [1, FIA_SLATE_MAX_ITEMS]");
      if (flags[2])
        return fail(c, FIA_ERR_STATE, "a query's user or one of its slate items has no Hessian cache: it was not "
                                      "among the queries of the last fia_prepare_for");
    }
    return FIA_OK;
  })
}

int fia_slate_batch(fia_ctx* c, int64_t Q, const int32_t* qu, const int64_t* slate_offsets, int64_t total_items,
                    const int32_t* slate_item, const double* slate_weight, const int64_t* offsets, int64_t total_rel,
                    int32_t* rel_idx, double* influence, double* x_out, double* value, int K, int64_t* topk_pos,
                    int64_t* topk_idx, double* topk_val, void* stream) {
  if (!c) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    // the batch bounds come first: nothing of an oversized batch is looked at
    if (Q < 0 || Q > FIA_SLATE_MAX_TOTAL_ITEMS)
      return fail(c, FIA_ERR_INVALID, "num_queries out of range [0, 2^30]: split the batch");
    // a half record per (query, item), indexed in 32 bits
    if (total_items < 0 || total_items > FIA_SLATE_MAX_TOTAL_ITEMS)
      return fail(c, FIA_ERR_INVALID, "total_items out of range [0, 2^30]: split the batch");
    // a rating's position inside its query's related list is kept in 32 bits by the top-K selection
    if (total_rel < 0 || total_rel > FIA_SLATE_MAX_TOTAL_REL)
      return fail(c, FIA_ERR_INVALID, "total_rel out of range [0, 2^31 - 1]: split the batch");
    if (int rc = check_prepared(c); rc != FIA_OK) return rc;
    if (K < 0 || K > FIA_MAX_TOPK) return fail(c, FIA_ERR_INVALID, "K must be in [0, FIA_MAX_TOPK]");
    if (K > 0 && (!topk_pos || !topk_idx || !topk_val)) return fail(c, FIA_ERR_INVALID, "null top-K output");
    if (!rel_idx && !influence && !x_out && !value && K == 0)
      return fail(c, FIA_ERR_INVALID, "no output requested (rel_idx, influence, x_out, value, top-K)");
    if (Q == 0) return FIA_OK;
    if (!qu || !slate_offsets || !offsets || (total_items > 0 && (!slate_item || !slate_weight)))
      return fail(c, FIA_ERR_INVALID, "null query, slate or offset array");
    if (!fia::slate_supported(c->p.model, c->p.k))
      return fail(c, FIA_ERR_UNSUPPORTED,
                  "fia_slate_batch is built for MF k in {8, 16, 32, 64} and NCF k in {8, 16, 32}; the large-k models "
                  "are not supported yet");
    DeviceGuard g(c->device);
    hipStream_t s = as_stream(stream);
    if (int rc = enter_stream(c, s, "fia_slate_batch"); rc != FIA_OK) return rc;
    // the Gram caches of a pending small-k pass are read: join it, as fia_pair_batch does
    if (hipError_t es = fia::join_prepare(c, s); es != hipSuccess) return hip_fail(c, es, "fia_slate_batch");
    hipError_t e = fia::slate_batch(c, Q, qu, slate_offsets, total_items, slate_item, slate_weight, offsets,
                                    total_rel, rel_idx, influence, x_out, value, K, topk_pos, topk_idx, topk_val, s);
    if (e != hipSuccess) return hip_fail(c, e, "fia_slate_batch");
    return FIA_OK;
  })
}

int fia_set_profiling(fia_ctx* c, int phase_mask) {
  if (!c) return FIA_ERR_INVALID;
  c->profiling = (unsigned)phase_mask & ((1u << FIA_NUM_PHASES) - 1u);
  return FIA_OK;
}

int fia_profile_read(fia_ctx* c, double* ms_sum, int64_t* counts) {
  if (!c || !ms_sum || !counts) return FIA_ERR_INVALID;
  FIA_GUARDED(c, {
    DeviceGuard g(c->device);
    int rc = FIA_OK;
    for (int ph = 0; ph < FIA_NUM_PHASES; ++ph) {
      double sum = 0.0;
      int64_t cnt = 0;
      for (auto& pr : c->events.ev[ph]) {
        float ms = 0.f;
        if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
          sum += ms;
          ++cnt;
        } else {
          rc = fail(c, FIA_ERR_HIP, "event timing failed");
        }
        c->events.pool.push_back(pr.first);
        c->events.pool.push_back(pr.second);
      }
      c->events.ev[ph].clear();
      ms_sum[ph] = sum;
      counts[ph] = cnt;
    }
    return rc;
  })
}

}  // extern "C"
