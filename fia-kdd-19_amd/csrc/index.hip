// Rating index (CSR by user, CSC by item), related-set counting and the
// per-batch chunk list.
//
// Replaces the reference's per-query O(N) scans
//   u_indices = np.where(train.x[:, 0] == test_u)   (matrix_factorization.py:320)
//   i_indices = np.where(train.x[:, 1] == test_i)   (matrix_factorization.py:321)
// with a one-time stable radix sort: inside every list train rows stay in
// ascending order, so rel(u,i) = R_u ++ C_i is the reference's concatenation
// bit for bit (mf:322).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "common.h"
#include "scan.h"

namespace fia {
namespace {

__global__ void k_check_ids(const int32_t* __restrict__ user, const int32_t* __restrict__ item, int64_t N,
                            int64_t U, int64_t I, int32_t* __restrict__ flag) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int bad = 0;
  for (; j < N; j += stride) {
    int32_t u = user[j], i = item[j];
    bad |= (u < 0 || u >= U || i < 0 || i >= I);
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

__global__ void k_gather_side(const int32_t* __restrict__ rows, const int32_t* __restrict__ other_src,
                              const float* __restrict__ rating_src, int64_t N, int32_t* __restrict__ other,
                              float* __restrict__ rating) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; j < N; j += stride) {
    int32_t r = rows[j];
    other[j] = other_src[r];
    rating[j] = rating_src[r];
  }
}

// pair set insert: one slot per distinct (u, i), counting duplicate train rows
__global__ void k_pair_insert(const int32_t* __restrict__ user, const int32_t* __restrict__ item,
                              const float* __restrict__ rating, int64_t N, int64_t I, unsigned long long* key,
                              int32_t* cnt, double* sum, unsigned long long mask) {
  int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; j < N; j += stride) {
    const unsigned long long k = (unsigned long long)user[j] * (unsigned long long)I + (unsigned long long)item[j];
    unsigned long long h = pair_hash(k) & mask;
    for (unsigned long long probe = 0; probe <= mask; ++probe) {
      unsigned long long prev = atomicCAS(&key[h], kEmptyKey, k);
      if (prev == kEmptyKey || prev == k) {
        atomicAdd(&cnt[h], 1);
        atomicAdd(&sum[h], (double)rating[j]);
        break;
      }
      h = (h + 1) & mask;
    }
  }
}

// ptr[e] = lower_bound(sorted_keys, e), e in [0, n_entity]
__global__ void k_list_ptr(const int32_t* __restrict__ keys, int64_t N, int64_t n_entity, int64_t* __restrict__ ptr) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e > n_entity) return;
  int64_t lo = 0, hi = N;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < e) lo = mid + 1; else hi = mid;
  }
  ptr[e] = lo;
}

__device__ inline void query_sides(const int32_t* qu, const int32_t* qi, int64_t q, const int64_t* uptr,
                                   const int64_t* iptr, int64_t U, int64_t I, int64_t& ub, int64_t& du, int64_t& ib,
                                   int64_t& di) {
  const int32_t u = qu[q], i = qi[q];
  ub = du = ib = di = 0;
  if (u >= 0 && u < U && i >= 0 && i < I) {
    ub = uptr[u];
    du = uptr[u + 1] - ub;
    ib = iptr[i];
    di = iptr[i + 1] - ib;
  }
}

// ---- single-pass per-query scans (decoupled look-back): the body is in scan.h ----
template <int MODE>
__global__ __launch_bounds__(kScanThreads) void k_query_scan(
    const int32_t* __restrict__ qu, const int32_t* __restrict__ qi, int64_t Q, const int64_t* __restrict__ uptr,
    const int64_t* __restrict__ iptr, int64_t U, int64_t I, int64_t* __restrict__ out,
    unsigned long long* __restrict__ tstate, unsigned int* __restrict__ tctr, int32_t* __restrict__ flag,
    const int64_t* __restrict__ offsets, ChunkDesc* __restrict__ cdesc, int32_t* __restrict__ zero_word,
    int64_t* __restrict__ qbase, int runs, int clen, int lsh, int32_t* __restrict__ slices) {
  query_scan_body<MODE>(qu, qi, Q, uptr, iptr, U, I, out, tstate, tctr, flag, offsets, cdesc, zero_word, qbase, runs,
                        clen, lsh, slices);
}

// ---- query groups (entity-shared scoring) ----
// thread per query: rank inside its user group and its item group; per side the output
// base (offsets[q], offsets[q] + |R_u|) and candidate-slot base (coff[q], coff[q] + chunks of R_u)
__global__ void k_group_count(const int32_t* __restrict__ qu, const int32_t* __restrict__ qi, int64_t Q,
                              const int64_t* __restrict__ uptr, const int64_t* __restrict__ iptr, int64_t U, int64_t I,
                              const int64_t* __restrict__ offsets, const int64_t* __restrict__ coff,
                              unsigned long long* __restrict__ gcnt, int32_t* __restrict__ grank,
                              int64_t* __restrict__ qbase) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Q) return;
  int64_t ub, du, ib, di;
  query_sides(qu, qi, q, uptr, iptr, U, I, ub, du, ib, di);
  const int32_t u = qu[q], i = qi[q];
  const bool ok = (u >= 0 && u < U && i >= 0 && i < I) && (du + di > 0);
  grank[2 * q] = ok ? (int32_t)atomicAdd(&gcnt[u], 1ull) : -1;
  grank[2 * q + 1] = ok ? (int32_t)atomicAdd(&gcnt[U + i], 1ull) : -1;
  qbase[4 * q + 0] = offsets[q];
  qbase[4 * q + 1] = offsets[q] + du;
  qbase[4 * q + 2] = coff[q];
  qbase[4 * q + 3] = coff[q] + (du + kChunk - 1) / kChunk;
}

// thread per query: place it into its user group and its item group
__global__ void k_group_fill(const int32_t* __restrict__ qu, const int32_t* __restrict__ qi, int64_t Q, int64_t U,
                             const int64_t* __restrict__ gstart, const int32_t* __restrict__ grank,
                             int32_t* __restrict__ gq) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < Q && grank[2 * t] >= 0) {
    const int32_t u = qu[t], i = qi[t];
    gq[gstart[u] + grank[2 * t]] = (int32_t)t;
    gq[gstart[U + i] + grank[2 * t + 1]] = (int32_t)t;
  }
}

// Single-pass decoupled look-back scan over the U + I entities (users, then items) of
// the two per-entity counts of the entity-shared schedule: queries per entity (gcnt ->
// gstart) and work items per entity, ceil(deg / (cpi kChunk)) * ceil(gcnt / qb) (->
// wstart; a work item covers cpi consecutive list chunks).
// Both exclusive prefixes (and the totals at [U + I]) in one launch: no library scan, no
// count array.  tstate: two arrays of tile words (queries, work items); the last tile to
// finish re-zeroes them and the two counters.
__global__ __launch_bounds__(kScanThreads) void k_group_scan(
    unsigned long long* __restrict__ gcnt, const int64_t* __restrict__ uptr, const int64_t* __restrict__ iptr,
    int64_t U, int64_t I, int qb, int cpi, int64_t* __restrict__ gstart, int64_t* __restrict__ wstart,
    unsigned long long* __restrict__ tstate, unsigned int* __restrict__ tctr) {
  __shared__ int s_tile;
  __shared__ int64_t s_wa[kScanThreads / 64], s_wb[kScanThreads / 64];
  __shared__ int64_t s_pa, s_pb;
  const int64_t nE = U + I;
  const unsigned ntiles = (unsigned)((nE + 1 + kScanTile - 1) / kScanTile);
  if (threadIdx.x == 0) s_tile = (int)atomicAdd(&tctr[0], 1u);
  __syncthreads();
  const int64_t tile = s_tile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t = tile * kScanTile + threadIdx.x;
  int64_t a = 0, b = 0;
  if (t < nE) {
    a = (int64_t)gcnt[t];
    // this thread is the count's only reader here (k_item_fill takes it from gstart): leave
    // it zero for the next batch's k_group_count -- no memset on the query path
    if (a > 0) gcnt[t] = 0;
    if (a > 0) {
      const int64_t deg = t < U ? uptr[t + 1] - uptr[t] : iptr[t - U + 1] - iptr[t - U];
      b = ((deg + kChunk * cpi - 1) / (kChunk * cpi)) * ((a + qb - 1) / qb);
    }
  }
  int64_t ia = a, ib = b;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int64_t ya = __shfl_up(ia, off), yb = __shfl_up(ib, off);
    if (lane >= off) { ia += ya; ib += yb; }
  }
  if (lane == 63) { s_wa[wave] = ia; s_wb[wave] = ib; }
  __syncthreads();
  int64_t ba = 0, bb = 0, agg_a = 0, agg_b = 0;
#pragma unroll
  for (int w = 0; w < kScanThreads / 64; ++w) {
    if (w < wave) { ba += s_wa[w]; bb += s_wb[w]; }
    agg_a += s_wa[w];
    agg_b += s_wb[w];
  }
  if (wave == 0) {
    const int64_t ea = scan_lookback(tstate, tile, agg_a);
    const int64_t eb = scan_lookback(tstate + ntiles, tile, agg_b);
    if (lane == 0) { s_pa = ea; s_pb = eb; }
  }
  __syncthreads();
  if (t <= nE) {
    gstart[t] = s_pa + ba + ia - a;
    wstart[t] = s_pb + bb + ib - b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // the block's tile-word stores performed before it counts itself done (see k_query_scan)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned done = atomicAdd(&tctr[1], 1u);
    if (done == ntiles - 1) {
      for (unsigned w = 0; w < 2 * ntiles; ++w)
        __hip_atomic_store(&tstate[w], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&tctr[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&tctr[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// thread per work item (grid-stride up to wstart[nE]): its entity by binary search over
// wstart, then {entity, chunk of the entity's list, block of the entity's query group}
__global__ void k_item_fill(const int64_t* __restrict__ wstart, const int64_t* __restrict__ gstart,
                            int64_t nE, int32_t* __restrict__ witems, int qb) {
  const int64_t total = wstart[nE];
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total;
       w += (int64_t)gridDim.x * blockDim.x) {
    const int64_t lo = last_at_most(wstart, (int64_t)0, nE - 1, w);     // last entity t with wstart[t] <= w
    const int64_t b = wstart[lo];
    const int64_t nqb = (gstart[lo + 1] - gstart[lo] + qb - 1) / qb;     // the entity's query count
    witems[3 * w] = (int32_t)lo;
    witems[3 * w + 1] = (int32_t)((w - b) / nqb);    // chunk of the entity's list
    witems[3 * w + 2] = (int32_t)((w - b) % nqb);    // block of the entity's query group
  }
}

// one workgroup per query: rel[offsets[q] + p] = R_u[p] (p < deg u), then C_i
__global__ void k_write_related(const int32_t* __restrict__ qu, const int32_t* __restrict__ qi,
                                const int64_t* __restrict__ offsets, const int64_t* __restrict__ uptr,
                                const int32_t* __restrict__ urow, const int64_t* __restrict__ iptr,
                                const int32_t* __restrict__ irow, int64_t U, int64_t I, int32_t* __restrict__ rel) {
  int64_t q = blockIdx.x;
  int32_t u = qu[q], i = qi[q];
  if (u < 0 || u >= U || i < 0 || i >= I) return;
  int64_t base = offsets[q];
  int64_t ub = uptr[u], du = uptr[u + 1] - ub;
  int64_t ib = iptr[i], di = iptr[i + 1] - ib;
  for (int64_t p = threadIdx.x; p < du; p += blockDim.x) rel[base + p] = urow[ub + p];
  for (int64_t p = threadIdx.x; p < di; p += blockDim.x) rel[base + du + p] = irow[ib + p];
}

}  // namespace

namespace {

inline unsigned bits_for(int64_t n) {
  unsigned b = 1;
  while (b < 31 && ((int64_t)1 << b) < n) ++b;
  return b;
}

inline int grid_for(int64_t n, int threads, int cap = 8192) {
  int64_t g = (n + threads - 1) / threads;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

}  // namespace

// Small-k Gram work lists of the current index: items of <= chunk list rows {entity,
// start, len, slot} (longest lists first), slot < 0 = write the Gram directly, else a
// partial slot; a combine entry {entity, first slot, n slots, 0} per split entity.
hipError_t build_gram_lists(fia_ctx* c, int64_t chunk, hipStream_t s) {
  Index& X = c->idx;
  for (int sd = 0; sd < 2; ++sd) {
    const std::vector<int64_t>& hptr = X.hptr[sd];
    std::vector<int32_t> items, comb;
    int32_t slots = 0;
    for (int32_t e : X.hord[sd]) {
      const int64_t len = hptr[(size_t)e + 1] - hptr[(size_t)e];
      const int64_t nit = len == 0 ? 1 : (len + chunk - 1) / chunk;
      if (nit > 1) comb.insert(comb.end(), {e, slots, (int32_t)nit, 0});
      for (int64_t t = 0; t < nit; ++t) {
        const int64_t st = t * chunk;
        const int64_t ln = std::min<int64_t>(chunk, len - st);
        items.insert(items.end(), {e, (int32_t)st, (int32_t)(ln < 0 ? 0 : ln), nit > 1 ? slots++ : -1});
      }
    }
    X.n_gitems[sd] = (int64_t)items.size() / 4;
    X.n_gcomb[sd] = (int64_t)comb.size() / 4;
    X.n_gslots[sd] = slots;
    if (!items.empty()) {
      FIA_HIP_TRY(X.gitems[sd].reserve(sizeof(int32_t) * items.size(), s));
      FIA_HIP_TRY(hipMemcpyAsync(X.gitems[sd].ptr, items.data(), sizeof(int32_t) * items.size(), hipMemcpyHostToDevice, s));
    }
    if (!comb.empty()) {
      FIA_HIP_TRY(X.gcomb[sd].reserve(sizeof(int32_t) * comb.size(), s));
      FIA_HIP_TRY(hipMemcpyAsync(X.gcomb[sd].ptr, comb.data(), sizeof(int32_t) * comb.size(), hipMemcpyHostToDevice, s));
    }
    FIA_HIP_TRY(hipStreamSynchronize(s));   // this side's host lists are freed at the end of the iteration
  }
  X.gchunk = chunk;
  return hipSuccess;
}

// the other-side rows of the Gram stream as byte offsets into their table (id * k * 4), in
// stream order and quad-transposed: rating 4 q + g of sub-batch d at ids[kGsSub d + 4 g + q]
// (the 16 lanes of MFMA row group g read their four quads' offsets as one 16-B word),
// kGsNoRow past the list's end
__global__ void k_gs_ids(int64_t nd, const int2* __restrict__ desc, const int32_t* __restrict__ pos,
                         const int32_t* __restrict__ other0, const int32_t* __restrict__ other1, int k,
                         uint32_t* __restrict__ ids) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nd * kGsSub;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t d = t / kGsSub;
    const int r = 4 * (int)(t & 3) + (int)((t >> 2) & 3);   // t % 16 = 4 g + q  ->  rating 4 q + g
    const int meta = desc[d].x;
    const int valid = meta & 31, side = (meta >> 6) & 1;
    ids[t] = r < valid ? (uint32_t)(side ? other1 : other0)[pos[d] + r] * (uint32_t)(k * 4) : kGsNoRow;
  }
}

hipError_t build_gram_stream(fia_ctx* c, int k, hipStream_t s) {
  Index& X = c->idx;
  if (X.gs_version == X.version && X.gs_k == k && X.gswave.ptr) return hipSuccess;
  struct Seg {
    int64_t len;
    int side;
    int32_t e, start, slot;
  };
  struct Team {
    int64_t len;
    int side;
    int32_t e, nit;
  };
  struct Range {   // one wave's descriptors and the list positions of their first ratings
    std::vector<int2> d;
    std::vector<int32_t> p;
  };
  std::vector<Seg> segs;
  std::vector<Team> teams;
  std::vector<int32_t> comb[2];
  for (int sd = 0; sd < 2; ++sd) {
    const std::vector<int64_t>& hptr = X.hptr[sd];
    int32_t slots = 0;
    for (int32_t e : X.hord[sd]) {
      const int64_t len = hptr[(size_t)e + 1] - hptr[(size_t)e];
      if (len <= kGsSlice) {
        segs.push_back({len, sd, e, 0, -1});
        continue;
      }
      const int64_t nit = (len + kGsSlice - 1) / kGsSlice;
      if (nit <= kGsTeamSlices) {   // summed by its workgroup
        teams.push_back({len, sd, e, (int32_t)nit});
        continue;
      }
      // beyond a team's reach: partial slots, summed by k_gram_combine
      comb[sd].insert(comb[sd].end(), {e, slots, (int32_t)nit, 0});
      for (int64_t t = 0; t < nit; ++t)
        segs.push_back({std::min<int64_t>(kGsSlice, len - t * kGsSlice), sd, e, (int32_t)(t * kGsSlice), slots++});
    }
    if ((uint32_t)slots >= kGsTeamBit) return hipErrorInvalidValue;   // slot + 1 stays below the team bit
    X.n_gsslots[sd] = slots;
  }
  // longest first (both sides merged): the deep teams, then the slices of the lists beyond a
  // team's reach, then the whole lists
  std::stable_sort(teams.begin(), teams.end(), [](const Team& a, const Team& b) { return a.len > b.len; });
  std::stable_sort(segs.begin(), segs.end(), [](const Seg& a, const Seg& b) { return a.len > b.len; });
  // a segment's sub-batches appended to a range; `out` rides on the last one
  auto emit = [&](Range& r, const Seg& g, uint32_t out_low) {
    const int nsb = g.len == 0 ? 1 : (int)((g.len + kGsSub - 1) / kGsSub);
    for (int t = 0; t < nsb; ++t) {
      const int valid = (int)std::min<int64_t>(kGsSub, g.len - (int64_t)t * kGsSub);
      const bool last = t == nsb - 1;
      const int meta = (valid < 0 ? 0 : valid) | (last ? 1 << 5 : 0) | (g.side << 6) | (g.e << 8);
      const uint32_t out = last ? ((uint32_t)g.len << 23) | out_low : 0u;
      r.d.push_back(int2{meta, (int)out});
      r.p.push_back((int32_t)(X.hptr[g.side][(size_t)g.e] + g.start + (int64_t)t * kGsSub));
    }
    return nsb;
  };
  auto close = [&](Range& r) {
    while (r.d.size() % kGsRing) {   // a multiple of the ring per wave (one ring turn per loop trip)
      r.d.push_back(int2{1 << 7, -1});
      r.p.push_back(0);
    }
  };
  // workgroups of kGsWaves ranges.  A team's slices are the only segments of consecutive ranges
  // of one workgroup, `per` to a range (one while the waves last, up to kGsTeamPer); a team that
  // does not fit behind the last one opens a new workgroup
  std::vector<std::vector<Range>> wgs;
  for (const Team& tm : teams) {
    const int per = std::max(kGsTeamMinPer, (tm.nit + kGsWaves - 1) / kGsWaves), nw = (tm.nit + per - 1) / per;
    if (wgs.empty() || (int)wgs.back().size() + nw > kGsWaves) wgs.emplace_back();
    std::vector<Range>& wg = wgs.back();
    for (int32_t j = 0; j < tm.nit; ++j) {
      if (j % per == 0) wg.emplace_back();
      const Seg g{std::min<int64_t>(kGsSlice, tm.len - (int64_t)j * kGsSlice), tm.side, tm.e, j * kGsSlice, -1};
      emit(wg.back(), g, kGsTeamBit | (uint32_t)j << 8 | (uint32_t)tm.nit << 3 | (uint32_t)per);
      if (j % per == per - 1 || j == tm.nit - 1) close(wg.back());
    }
  }
  // the other segments packed into ranges as before; the ranges fill the waves the teams left
  // free, first workgroup first, then workgroups of their own
  size_t fill = 0;
  auto place = [&](Range&& r) {
    close(r);
    while (fill < wgs.size() && (int)wgs[fill].size() >= kGsWaves) ++fill;
    if (fill == wgs.size()) wgs.emplace_back();
    wgs[fill].push_back(std::move(r));
  };
  {
    Range r;
    int cur = 0, nseg = 0;
    for (const Seg& g : segs) {
      const int nsb = g.len == 0 ? 1 : (int)((g.len + kGsSub - 1) / kGsSub);
      if (cur > 0 && cur + nsb > kGsMaxSub - kGsRing) {
        place(std::move(r));
        r = Range{};
        cur = nseg = 0;
      }
      cur += emit(r, g, (uint32_t)(g.slot + 1));
      if (cur >= kGsTarget || ++nseg >= kGsMaxSeg) {
        place(std::move(r));
        r = Range{};
        cur = nseg = 0;
      }
    }
    if (cur > 0) place(std::move(r));
  }
  std::vector<int2> desc;
  std::vector<int32_t> pos, wave{0};
  for (std::vector<Range>& wg : wgs) {
    wg.resize(kGsWaves);   // a wave without a range walks nothing
    for (const Range& r : wg) {
      desc.insert(desc.end(), r.d.begin(), r.d.end());
      pos.insert(pos.end(), r.p.begin(), r.p.end());
      wave.push_back((int32_t)desc.size());
    }
  }
  const int64_t nd = (int64_t)desc.size();
  X.n_gsdesc = nd;
  X.n_gsw = (int64_t)wave.size() - 1;
  FIA_HIP_TRY(X.gsdesc.reserve(sizeof(int2) * (size_t)(nd + 2), s));
  FIA_HIP_TRY(X.gsids.reserve(sizeof(int32_t) * (size_t)((nd + 2) * kGsSub), s));
  FIA_HIP_TRY(X.gswave.reserve(sizeof(int32_t) * wave.size(), s));
  DevBuf dpos;
  FIA_HIP_TRY(dpos.reserve(sizeof(int32_t) * (size_t)(nd + 1), s));
  if (nd > 0) {
    FIA_HIP_TRY(hipMemcpyAsync(X.gsdesc.ptr, desc.data(), sizeof(int2) * (size_t)nd, hipMemcpyHostToDevice, s));
    FIA_HIP_TRY(hipMemcpyAsync(dpos.ptr, pos.data(), sizeof(int32_t) * (size_t)nd, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_gs_ids, dim3(grid_for(nd * kGsSub, 256)), dim3(256), 0, s, nd, X.gsdesc.as<int2>(),
                       dpos.as<int32_t>(), X.side[0].other.as<int32_t>(), X.side[1].other.as<int32_t>(), k,
                       X.gsids.as<uint32_t>());
    FIA_HIP_TRY(hipGetLastError());
  }
  FIA_HIP_TRY(hipMemsetAsync(X.gsdesc.as<int2>() + nd, 0, sizeof(int2) * 2, s));
  FIA_HIP_TRY(hipMemcpyAsync(X.gswave.ptr, wave.data(), sizeof(int32_t) * wave.size(), hipMemcpyHostToDevice, s));
  for (int sd = 0; sd < 2; ++sd) {
    X.n_gscomb[sd] = (int64_t)comb[sd].size() / 4;
    if (!comb[sd].empty()) {
      FIA_HIP_TRY(X.gscomb[sd].reserve(sizeof(int32_t) * comb[sd].size(), s));
      FIA_HIP_TRY(hipMemcpyAsync(X.gscomb[sd].ptr, comb[sd].data(), sizeof(int32_t) * comb[sd].size(),
                                 hipMemcpyHostToDevice, s));
    }
  }
  dpos.release(s);
  FIA_HIP_TRY(hipStreamSynchronize(s));   // the host vectors go out of scope
  X.gs_version = X.version;
  X.gs_k = k;
  return hipSuccess;
}

hipError_t build_index(fia_ctx* c, int64_t N, int64_t U, int64_t I, const int32_t* user, const int32_t* item,
                       const float* rating, hipStream_t s, std::string& why) {
  Index& X = c->idx;
  X.valid = false;
  FIA_HIP_TRY(c->flag.reserve(64, s));
  FIA_HIP_TRY(hipMemsetAsync(c->flag.ptr, 0, 64, s));
  if (N > 0) {
    hipLaunchKernelGGL(k_check_ids, dim3(grid_for(N, 256)), dim3(256), 0, s, user, item, N, U, I,
                       c->flag.as<int32_t>());
    FIA_HIP_TRY(hipGetLastError());
  }
  int32_t hflag = 0;
  FIA_HIP_TRY(hipMemcpyAsync(&hflag, c->flag.ptr, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  FIA_HIP_TRY(hipStreamSynchronize(s));
  if (hflag) {
    why = "training ids out of range [0, num_users) x [0, num_items)";
    return hipErrorInvalidValue;
  }
  DevBuf keys_sorted, tmp;
  FIA_HIP_TRY(keys_sorted.reserve(sizeof(int32_t) * (size_t)(N > 0 ? N : 1), s));
  const int32_t* key_src[2] = {user, item};
  const int32_t* other_src[2] = {item, user};
  int64_t n_ent[2] = {U, I};
  for (int sd = 0; sd < 2; ++sd) {
    Side& S = X.side[sd];
    size_t nb = sizeof(int32_t) * (size_t)(N > 0 ? N : 1);
    FIA_HIP_TRY(S.row.reserve(nb, s));
    FIA_HIP_TRY(S.other.reserve(nb, s));
    FIA_HIP_TRY(S.rating.reserve(sizeof(float) * (size_t)(N > 0 ? N : 1), s));
    FIA_HIP_TRY(S.ptr.reserve(sizeof(int64_t) * (size_t)(n_ent[sd] + 1), s));
    if (N > 0) {
      unsigned eb = bits_for(n_ent[sd]);
      rocprim::counting_iterator<int32_t> iota(0);
      size_t tb = 0;
      FIA_HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, key_src[sd], keys_sorted.as<int32_t>(), iota,
                                            S.row.as<int32_t>(), (size_t)N, 0u, eb, s));
      FIA_HIP_TRY(tmp.reserve(tb + 16, s));
      tb = tmp.bytes;
      FIA_HIP_TRY(rocprim::radix_sort_pairs(tmp.ptr, tb, key_src[sd], keys_sorted.as<int32_t>(), iota,
                                            S.row.as<int32_t>(), (size_t)N, 0u, eb, s));
      hipLaunchKernelGGL(k_gather_side, dim3(grid_for(N, 256)), dim3(256), 0, s, S.row.as<int32_t>(),
                         other_src[sd], rating, N, S.other.as<int32_t>(), S.rating.as<float>());
      FIA_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_list_ptr, dim3((unsigned)((n_ent[sd] + 1 + 255) / 256)), dim3(256), 0, s,
                       keys_sorted.as<int32_t>(), N, n_ent[sd], S.ptr.as<int64_t>());
    FIA_HIP_TRY(hipGetLastError());
    FIA_HIP_TRY(hipStreamSynchronize(s));   // keys_sorted is reused by the next side
    // entities by list length, longest first: the Gram kernels start the long lists early
    std::vector<int64_t> hptr((size_t)n_ent[sd] + 1);
    FIA_HIP_TRY(hipMemcpyAsync(hptr.data(), S.ptr.ptr, sizeof(int64_t) * hptr.size(), hipMemcpyDeviceToHost, s));
    FIA_HIP_TRY(hipStreamSynchronize(s));
    std::vector<int32_t> ord((size_t)n_ent[sd]);
    for (int64_t e = 0; e < n_ent[sd]; ++e) ord[(size_t)e] = (int32_t)e;
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) {
      return hptr[(size_t)a + 1] - hptr[(size_t)a] > hptr[(size_t)b + 1] - hptr[(size_t)b];
    });
    X.hptr[sd] = hptr;
    FIA_HIP_TRY(X.order[sd].reserve(sizeof(int32_t) * ord.size(), s));
    FIA_HIP_TRY(hipMemcpyAsync(X.order[sd].ptr, ord.data(), sizeof(int32_t) * ord.size(), hipMemcpyHostToDevice, s));
    FIA_HIP_TRY(hipStreamSynchronize(s));
    X.hord[sd] = ord;
  }
  FIA_HIP_TRY(build_gram_lists(c, kGramChunk, s));
  keys_sorted.release(s);
  tmp.release(s);
  // pair set, load factor <= 1/2
  int64_t cap = 1024;
  while (cap < 2 * N) cap <<= 1;
  FIA_HIP_TRY(X.pkey.reserve(sizeof(unsigned long long) * (size_t)cap, s));
  FIA_HIP_TRY(X.pcnt.reserve(sizeof(int32_t) * (size_t)cap, s));
  FIA_HIP_TRY(X.psum.reserve(sizeof(double) * (size_t)cap, s));
  FIA_HIP_TRY(hipMemsetAsync(X.pkey.ptr, 0xff, sizeof(unsigned long long) * (size_t)cap, s));
  FIA_HIP_TRY(hipMemsetAsync(X.pcnt.ptr, 0, sizeof(int32_t) * (size_t)cap, s));
  FIA_HIP_TRY(hipMemsetAsync(X.psum.ptr, 0, sizeof(double) * (size_t)cap, s));
  if (N > 0) {
    hipLaunchKernelGGL(k_pair_insert, dim3(grid_for(N, 256)), dim3(256), 0, s, user, item, rating, N, I,
                       X.pkey.as<unsigned long long>(), X.pcnt.as<int32_t>(), X.psum.as<double>(),
                       (unsigned long long)(cap - 1));
    FIA_HIP_TRY(hipGetLastError());
  }
  FIA_HIP_TRY(hipStreamSynchronize(s));
  X.pcap = cap;
  ++X.version;
  X.N = N;
  X.U = U;
  X.I = I;
  X.valid = true;
  return hipSuccess;
}

// tile words + two counters of k_query_scan, zero when (re)allocated; every launch leaves
// them zero again
static hipError_t scan_state(fia_ctx* c, int64_t Q, hipStream_t s) {
  const int64_t ntiles = (Q + 1 + kScanTile - 1) / kScanTile;
  const size_t need = sizeof(unsigned long long) * (size_t)(2 * ntiles) + 16;   // two tile-word arrays (runs)
  if (c->qscan.bytes >= need && c->qscan.ptr) return hipSuccess;
  // stream-ordered regrow (the previous launches on s still own the old block)
  FIA_HIP_TRY(c->qscan.reserve(need < 4096 ? 4096 : need, s));
  FIA_HIP_TRY(hipMemsetAsync(c->qscan.ptr, 0, c->qscan.bytes, s));
  return hipSuccess;
}

// the scan's arguments over the context's scan state (reserved here)
static hipError_t query_scan_args(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, int64_t* out,
                                  const int64_t* offsets, ChunkDesc* cdesc, int32_t* zero_word, hipStream_t s,
                                  int64_t* qbase, int runs, int clen, int lsh, int32_t* slices, ScanArgs& S) {
  FIA_HIP_TRY(scan_state(c, Q, s));
  FIA_HIP_TRY(c->flag.reserve(64, s));
  unsigned int* ctr = reinterpret_cast<unsigned int*>(c->qscan.as<char>() + c->qscan.bytes - 16);
  S = ScanArgs{qu, qi, Q, c->idx.side[0].ptr.as<int64_t>(), c->idx.side[1].ptr.as<int64_t>(), c->idx.U, c->idx.I, out,
               c->qscan.as<unsigned long long>(), ctr, c->flag.as<int32_t>(), offsets, cdesc, zero_word, qbase, runs,
               clen, lsh, slices};
  return hipSuccess;
}

template <int MODE>
static hipError_t launch_query_scan(const ScanArgs& S, hipStream_t s, hipEvent_t ev_a, hipEvent_t ev_b) {
  hipExtLaunchKernelGGL(k_query_scan<MODE>, dim3((unsigned)scan_tiles(S.Q)), dim3(kScanThreads), 0, s, ev_a, ev_b, 0,
                        S.qu, S.qi, S.Q, S.uptr, S.iptr, S.U, S.I, S.out, S.tstate, S.tctr, S.flag, S.offsets, S.cdesc,
                        S.zero_word, S.qbase, S.runs, S.clen, S.lsh, S.slices);
  return hipGetLastError();
}

hipError_t count_related(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, int64_t* offsets,
                         hipStream_t s) {
  ScanArgs S;
  FIA_HIP_TRY(query_scan_args(c, Q, qu, qi, offsets, nullptr, nullptr, nullptr, s, nullptr, 0, kChunk, 0, nullptr, S));
  return launch_query_scan<0>(S, s, nullptr, nullptr);
}

hipError_t write_related(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                         int32_t* rel, hipStream_t s) {
  if (Q == 0) return hipSuccess;
  hipLaunchKernelGGL(k_write_related, dim3((unsigned)Q), dim3(256), 0, s, qu, qi, offsets,
                     c->idx.side[0].ptr.as<int64_t>(), c->idx.side[0].row.as<int32_t>(),
                     c->idx.side[1].ptr.as<int64_t>(), c->idx.side[1].row.as<int32_t>(), c->idx.U, c->idx.I, rel);
  return hipGetLastError();
}


hipError_t chunk_scan_args(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                           int64_t max_chunks, bool offsets_only, hipStream_t s, int32_t* zero_word, bool runs,
                           int slice_cost, int run_chunk, ScanArgs& S) {
  FIA_HIP_TRY(c->coff.reserve(sizeof(int64_t) * (size_t)(Q + 1), s));
  const bool rq = runs && !offsets_only;
  if (!offsets_only) FIA_HIP_TRY(c->cdesc.reserve(sizeof(ChunkDesc) * (size_t)(max_chunks + 1), s));
  int lsh = 0;                                   // slice cost: the power of two >= slice_cost
  while ((1 << lsh) < slice_cost && lsh < 30) ++lsh;
  const int lam = 1 << lsh;
  if (rq) {
    FIA_HIP_TRY(c->qbase.reserve(sizeof(int64_t) * (size_t)(4 * Q + 2), s));
    // total cost <= (kRunQB + 2) per descriptor
    FIA_HIP_TRY(c->slices.reserve(sizeof(int32_t) * (size_t)((max_chunks + 1) * (kRunQB + 2) / lam + 2), s));
  }
  return query_scan_args(c, Q, qu, qi, c->coff.as<int64_t>(), offsets,
                         offsets_only ? nullptr : c->cdesc.as<ChunkDesc>(), zero_word, s,
                         rq ? c->qbase.as<int64_t>() : nullptr, rq ? kRunQB : 0, rq ? run_chunk : kChunk, lsh,
                         rq ? c->slices.as<int32_t>() : nullptr, S);
}

hipError_t launch_chunk_scan(const ScanArgs& S, hipStream_t s, hipEvent_t ev_a, hipEvent_t ev_b) {
  return launch_query_scan<1>(S, s, ev_a, ev_b);
}

hipError_t build_chunks(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                        int64_t max_chunks, bool offsets_only, hipStream_t s, int32_t* zero_word, bool runs,
                        int slice_cost, int run_chunk) {
  ScanArgs S;
  FIA_HIP_TRY(chunk_scan_args(c, Q, qu, qi, offsets, max_chunks, offsets_only, s, zero_word, runs, slice_cost,
                              run_chunk, S));
  return launch_chunk_scan(S, s);
}

hipError_t build_groups(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                        int64_t max_items, int qb, hipStream_t s, int cpi) {
  const int64_t U = c->idx.U, I = c->idx.I, nE = U + I;
  const int64_t ntiles = (nE + 1 + kScanTile - 1) / kScanTile;
  // per-entity query counts: zero at allocation, left zero by k_group_scan
  if (c->gcnt.bytes < sizeof(int64_t) * (size_t)(nE + 1) || !c->gcnt.ptr) {
    FIA_HIP_TRY(c->gcnt.reserve(sizeof(int64_t) * (size_t)(nE + 1), s));
    FIA_HIP_TRY(hipMemsetAsync(c->gcnt.ptr, 0, c->gcnt.bytes, s));
  }
  FIA_HIP_TRY(c->gstart.reserve(sizeof(int64_t) * (size_t)(nE + 1), s));
  FIA_HIP_TRY(c->wstart.reserve(sizeof(int64_t) * (size_t)(nE + 1), s));
  FIA_HIP_TRY(c->grank.reserve(sizeof(int32_t) * (size_t)(2 * Q + 1), s));
  FIA_HIP_TRY(c->gq.reserve(sizeof(int32_t) * (size_t)(2 * Q + 1), s));
  FIA_HIP_TRY(c->qbase.reserve(sizeof(int64_t) * (size_t)(4 * Q + 1), s));
  FIA_HIP_TRY(c->witems.reserve(sizeof(int32_t) * (size_t)(3 * max_items + 3), s));
  // k_group_scan state: 2 x ntiles tile words + 2 counters, zero at allocation and left zero
  const size_t need = sizeof(unsigned long long) * (size_t)(2 * ntiles) + 16;
  if (c->gscan.bytes < need || !c->gscan.ptr) {
    FIA_HIP_TRY(c->gscan.reserve(need, s));
    FIA_HIP_TRY(hipMemsetAsync(c->gscan.ptr, 0, c->gscan.bytes, s));
  }
  const int64_t* uptr = c->idx.side[0].ptr.as<int64_t>();
  const int64_t* iptr = c->idx.side[1].ptr.as<int64_t>();
  if (Q > 0) {
    hipLaunchKernelGGL(k_group_count, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, qu, qi, Q, uptr, iptr, U, I,
                       offsets, c->coff.as<int64_t>(), c->gcnt.as<unsigned long long>(), c->grank.as<int32_t>(),
                       c->qbase.as<int64_t>());
    FIA_HIP_TRY(hipGetLastError());
  }
  unsigned int* ctr = reinterpret_cast<unsigned int*>(c->gscan.as<char>() + c->gscan.bytes - 16);
  hipLaunchKernelGGL(k_group_scan, dim3((unsigned)ntiles), dim3(kScanThreads), 0, s, c->gcnt.as<unsigned long long>(),
                     uptr, iptr, U, I, qb, cpi, c->gstart.as<int64_t>(), c->wstart.as<int64_t>(),
                     c->gscan.as<unsigned long long>(), ctr);
  FIA_HIP_TRY(hipGetLastError());
  if (Q > 0) {
    hipLaunchKernelGGL(k_group_fill, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, qu, qi, Q, U,
                       c->gstart.as<int64_t>(), c->grank.as<int32_t>(), c->gq.as<int32_t>());
    FIA_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_item_fill, dim3(grid_for(max_items, 256, 16384)), dim3(256), 0, s, c->wstart.as<int64_t>(),
                     c->gstart.as<int64_t>(), nE, c->witems.as<int32_t>(), qb);
  return hipGetLastError();
}

}  // namespace fia
