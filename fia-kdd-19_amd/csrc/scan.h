// Device body of the single-pass per-query scans (decoupled look-back), shared by the thin
// k_query_scan kernels of index.hip and the scan role of the fused scan + side-solve launch of
// small_solve.hip (the library is built without relocatable device code: a kernel that runs the
// scan beside other work has to see the body in its own translation unit).
#pragma once

#include "common.h"

namespace fia {

// ---- single-pass per-query scans (decoupled look-back) ----
// One launch replaces count kernel + two-kernel library scan (+ descriptor fill): tiles of
// kScanTile queries take a dynamic tile number, publish their aggregate, look back over
// the earlier tiles' words {flag (2 bits), value (62 bits)} and write the exclusive
// prefix of every query (+ the total at [Q]).  The last tile to finish clears the tile
// words and counters, so no memset precedes the next launch.
//   MODE 0: n_q = |R_u| + |C_i| -> offsets (fia_count_related); bad ids flag[1]
//   MODE 1: chunks_q = ceil(|R_u|/kChunk) + ceil(|C_i|/kChunk) -> coff, + chunk descriptors
// (ml-1m-ex, both scans per step, same-box A/B: tiles of 64 / 128 / 256 / 512 / 1024 queries
// 33.3 / 24.7 / 20.8 / 19.4 / 20.9 us)
constexpr int kScanThreads = 512, kScanItems = 1, kScanTile = kScanThreads * kScanItems;
constexpr unsigned long long kScanAgg = 1ull << 62, kScanPre = 2ull << 62, kScanVal = (1ull << 62) - 1;

// tiles of a scan over Q queries (Q + 1 entries: the total lands at [Q])
inline int64_t scan_tiles(int64_t Q) { return (Q + 1 + kScanTile - 1) / kScanTile; }

// Wave 0 of a scan block: publish tile `tile`'s aggregate, then look back with the whole
// wave -- lane l reads the word of tile (window end - l); the nearest inclusive prefix ends
// the walk -- and publish the tile's inclusive prefix.  Returns the exclusive prefix (in
// every lane).  Tile words: {flag (2 bits): 1 aggregate / 2 inclusive prefix, value (62 bits)}.
__device__ inline int64_t scan_lookback(unsigned long long* __restrict__ tstate, int64_t tile, int64_t agg) {
  const int lane = threadIdx.x & 63;
  if (lane == 0)
    __hip_atomic_store(&tstate[tile], (tile == 0 ? kScanPre : kScanAgg) | (unsigned long long)agg,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int64_t excl = 0;
  for (int64_t end = tile - 1; end >= 0;) {
    const int64_t p = end - lane;
    const unsigned long long w =
        p >= 0 ? __hip_atomic_load(&tstate[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : kScanPre;
    const unsigned long long f = w >> 62;
    const unsigned long long pre = __ballot(f == 2), inv = __ballot(f == 0);
    const int stop = pre ? __builtin_ctzll(pre) : 64;            // first lane holding a prefix
    const unsigned long long need = stop >= 63 ? ~0ull : ((2ull << stop) - 1);
    if (inv & need) {                                              // a needed tile not published yet
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    int64_t part = lane <= stop ? (int64_t)(w & kScanVal) : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    excl += part;
    if (stop < 64) break;
    end -= 64;
  }
  if (lane == 0 && tile > 0)
    __hip_atomic_store(&tstate[tile], kScanPre | (unsigned long long)(excl + agg), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  return excl;
}

// MODE 1 (runs mode) LDS: per-query fill state (descriptor start; cost prefix; list bases and
// lengths; output base; run length; descriptor count) and the tile's test items with the kRunQB
// after it (run heads and lengths from LDS).  Declared for MODE 1 only: MODE 0 carries none of it.
struct ScanFillLds {
  int64_t c0[kScanTile], cost[kScanTile], ub[kScanTile], ib[kScanTile], base[kScanTile];
  int32_t du[kScanTile], di[kScanTile], nq[kScanTile], nd[kScanTile];
  int32_t qi[kScanTile + kRunQB];
  int64_t wave2[kScanThreads / 64], prefix2;   // the cost scan's wave sums and tile prefix
};
template <int MODE>
__device__ __forceinline__ ScanFillLds* scan_fill_lds() {
  if constexpr (MODE == 1) {
    __shared__ ScanFillLds F;
    return &F;
  } else {
    return nullptr;
  }
}

// One tile of the scan, run by a workgroup of kScanThreads threads whatever its place in the
// grid: the tile number is a ticket drawn from tctr[0], and the tile count, the second
// tile-word array and the last tile's reset all follow from Q, never from gridDim -- so a
// launch may hold workgroups that do other work beside its scan_tiles(Q) scan workgroups.
template <int MODE>
__device__ __forceinline__ void query_scan_body(
    const int32_t* __restrict__ qu, const int32_t* __restrict__ qi, int64_t Q, const int64_t* __restrict__ uptr,
    const int64_t* __restrict__ iptr, int64_t U, int64_t I, int64_t* __restrict__ out,
    unsigned long long* __restrict__ tstate, unsigned int* __restrict__ tctr, int32_t* __restrict__ flag,
    const int64_t* __restrict__ offsets, ChunkDesc* __restrict__ cdesc, int32_t* __restrict__ zero_word,
    int64_t* __restrict__ qbase, int runs, int clen, int lsh, int32_t* __restrict__ slices) {
  __shared__ int s_tile;
  __shared__ int64_t s_wave[kScanThreads / 64];
  __shared__ int64_t s_prefix;
  ScanFillLds* const F = scan_fill_lds<MODE>();   // MODE 1 only
  const unsigned ntiles = (unsigned)((Q + 1 + kScanTile - 1) / kScanTile);
  if (threadIdx.x == 0) s_tile = (int)atomicAdd(&tctr[0], 1u);
  __syncthreads();
  const int64_t tile = s_tile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q0 = tile * kScanTile + (int64_t)threadIdx.x * kScanItems;
  int64_t v[kScanItems];
  // the list bounds (and the output base) stay in registers for the descriptor fill
  // after the look-back, instead of a second dependent qu/qi -> ptr round trip
  int64_t s_ub[kScanItems], s_du[kScanItems], s_ib[kScanItems], s_di[kScanItems], s_base[kScanItems];
  int s_nq[kScanItems];
  int64_t tsum = 0, tsum2 = 0;     // tsum2: runs mode, the descriptors' scheduling cost
  if constexpr (MODE == 1) {
    static_assert(kScanItems == 1, "one query per thread");
    if (runs) {
      const int64_t qa = tile * kScanTile + threadIdx.x;
      F->qi[threadIdx.x] = qa < Q ? qi[qa] : -1;
      if (threadIdx.x < kRunQB) {
        const int64_t qb2 = tile * kScanTile + kScanTile + threadIdx.x;
        F->qi[kScanTile + threadIdx.x] = qb2 < Q ? qi[qb2] : -1;
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int it = 0; it < kScanItems; ++it) {
    const int64_t q = q0 + it;
    int64_t x = 0;
    s_ub[it] = s_du[it] = s_ib[it] = s_di[it] = s_base[it] = 0;
    s_nq[it] = 0;
    if (q < Q) {
      if (MODE == 1 && cdesc) s_base[it] = offsets[q];
      const int32_t u = qu[q], i = qi[q];
      if (u >= 0 && u < U && i >= 0 && i < I) {
        const int64_t ub = uptr[u], ib = iptr[i];
        const int64_t du = uptr[u + 1] - ub, di = iptr[i + 1] - ib;
        s_ub[it] = ub; s_du[it] = du; s_ib[it] = ib; s_di[it] = di;
        x = MODE == 0 ? du + di : (du + kChunk - 1) / kChunk + (di + kChunk - 1) / kChunk;
        if (MODE == 1 && runs) {
          // packed {chunks (candidate slots) << 31 | work descriptors}, chunks of clen ratings:
          // the item-side chunks are work only for a run head (first query of a run of equal
          // test items, runs cut at multiples of `runs`), which scores them for the whole run
          const int tt = threadIdx.x;
          const bool head = (q % runs) == 0 || (tt > 0 ? F->qi[tt - 1] : qi[q - 1]) != i;
          s_nq[it] = 0;
          if (head) {
            int nq = 1;
            const int lim = runs - (int)(q % runs);
#pragma unroll
            for (int j = 1; j < kRunQB; ++j) {
              const bool same = j < lim && F->qi[tt + j] == i;      // -1 past the batch
              nq += (same && nq == j) ? 1 : 0;
            }
            s_nq[it] = nq;
          }
          const int64_t cu = (du + clen - 1) / clen, ci = (di + clen - 1) / clen;
          x = ((cu + ci) << 31) | (cu + (head ? ci : 0));
          tsum2 += cu * kRunUserCost + (head ? ci * (s_nq[it] + 2) : 0);
        }
      } else if (MODE == 0) {
        atomicOr(flag + 1, 1);
      }
    }
    v[it] = x;
    tsum += x;
  }
  // block scan of the per-thread sums
  int64_t inc = tsum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int64_t y = __shfl_up(inc, off);
    if (lane >= off) inc += y;
  }
  int64_t inc2 = tsum2;
  if (MODE == 1 && runs) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int64_t y = __shfl_up(inc2, off);
      if (lane >= off) inc2 += y;
    }
  }
  if (lane == 63) {
    s_wave[wave] = inc;
    if (MODE == 1) F->wave2[wave] = inc2;
  }
  __syncthreads();
  int64_t wbase = 0, agg = 0, wbase2 = 0, agg2 = 0;
#pragma unroll
  for (int w = 0; w < kScanThreads / 64; ++w) {
    if (w < wave) wbase += s_wave[w];
    agg += s_wave[w];
    if (MODE == 1) {
      if (w < wave) wbase2 += F->wave2[w];
      agg2 += F->wave2[w];
    }
  }
  if (wave == 0) {
    const int64_t excl = scan_lookback(tstate, tile, agg);
    // runs mode: the cost prefix on the second tile-word array
    const int64_t excl2 = (MODE == 1 && runs) ? scan_lookback(tstate + ntiles, tile, agg2) : 0;
    if (lane == 0) {
      s_prefix = excl;
      if (MODE == 1) F->prefix2 = excl2;
      if (MODE == 1 && tile == 0 && zero_word) zero_word[0] = 0;   // solve's coupled-query counter
    }
  }
  __syncthreads();
  int64_t run = s_prefix + wbase + inc - tsum;
  int64_t run2 = (MODE == 1 ? F->prefix2 : 0) + wbase2 + inc2 - tsum2;    // cost prefix of this thread's first query
  constexpr int64_t kLo = (1ll << 31) - 1;
#pragma unroll
  for (int it = 0; it < kScanItems; ++it) {
    const int64_t q = q0 + it;
    if (q <= Q) out[q] = (MODE == 1 && runs) ? run >> 31 : run;
    if (MODE == 1 && runs && q == Q) {
      // work descriptors in all; slices in all (cost run2 in slices of lam) and the end mark
      const int64_t nw = run & kLo, ns = (run2 + (1ll << lsh) - 1) >> lsh;
      qbase[4 * Q] = nw;
      qbase[4 * Q + 1] = ns;
      if (slices) slices[ns] = (int32_t)nw;
    }
    if (MODE == 1 && qbase && q < Q) {
      // per query: {out base user, item}, {candidate slot base user, item} (k_score_mf_run)
      const int64_t du = s_du[it], cr = runs ? run >> 31 : run;
      qbase[4 * q + 0] = s_base[it];
      qbase[4 * q + 1] = s_base[it] + du;
      qbase[4 * q + 2] = cr;
      qbase[4 * q + 3] = cr + (du + clen - 1) / clen;
    }
    if (MODE == 1 && runs) {
      // runs mode: this query's descriptors are written by the whole block below
      F->c0[threadIdx.x] = run & kLo;
      F->cost[threadIdx.x] = run2;
      F->ub[threadIdx.x] = s_ub[it];
      F->ib[threadIdx.x] = s_ib[it];
      F->base[threadIdx.x] = s_base[it];
      F->du[threadIdx.x] = (int32_t)s_du[it];
      F->di[threadIdx.x] = (int32_t)s_di[it];
      F->nq[threadIdx.x] = s_nq[it];
      F->nd[threadIdx.x] = (q < Q) ? (int32_t)(v[it] & kLo) : 0;
    } else
    if (MODE == 1 && cdesc && q < Q && v[it] > 0) {
      const int64_t ub = s_ub[it], du = s_du[it], ib = s_ib[it], di = s_di[it];
      int64_t c = run;
      const int64_t base = s_base[it];
      for (int64_t st = 0; st < du; st += kChunk, ++c) {
        ChunkDesc d;
        d.list_base = ub + st;
        d.out_base = base + st;
        d.q = (int32_t)q;
        d.pos0 = (int32_t)st;
        d.len = (int32_t)(du - st < kChunk ? du - st : kChunk);
        d.side = 0;
        cdesc[c] = d;
      }
      for (int64_t st = 0; st < di; st += kChunk, ++c) {
        ChunkDesc d;
        d.list_base = ib + st;
        d.out_base = base + du + st;
        d.q = (int32_t)q;
        d.pos0 = (int32_t)(du + st);
        d.len = (int32_t)(di - st < kChunk ? di - st : kChunk);
        d.side = 1;
        cdesc[c] = d;
      }
    }
    run += v[it];
  }
  if (MODE == 1 && runs && cdesc) {
    // Block-parallel descriptor fill (runs mode): the block's descriptors are one contiguous
    // range; thread t writes descriptors t, t + 256, ... of it, finding the owning query by a
    // binary search over the per-query starts in LDS (a popular item's run head has ~20
    // descriptors: one thread writing them in turn bounded this kernel).  Descriptor j of a
    // query: user chunk j < cu (cost kRunUserCost), else item chunk j - cu (cost nq + 2); the
    // descriptor whose cost range [p, p + w) holds a slice start s << lsh starts slice s
    // (slices of a descriptor costing more than a slice are empty but the last): every
    // descriptor lands in exactly one slice.
    __syncthreads();
    const int64_t dstart = F->c0[0], dend = F->c0[kScanTile - 1] + F->nd[kScanTile - 1];
    {
      for (int64_t c = dstart + threadIdx.x; c < dend; c += kScanThreads) {
        // the owner: the last thread whose start is <= c (starts ascend; a thread with no
        // descriptors shares its start with the next one, so it is never the last such)
        const int t = last_at_most(F->c0, 0, kScanTile - 1, c);
        const int64_t j = c - F->c0[t];
        const int32_t du = F->du[t], di = F->di[t], nq = F->nq[t];
        const int64_t cu = (du + clen - 1) / clen;
        const int64_t qq = tile * kScanTile + t;
        ChunkDesc d;
        int64_t p, w;
        if (j < cu) {
          const int64_t st = j * clen;
          d.list_base = F->ub[t] + st;
          d.out_base = F->base[t] + st;
          d.pos0 = (int32_t)st;
          d.len = (int32_t)(du - st < clen ? du - st : clen);
          d.side = 0 | (1 << 8);
          p = F->cost[t] + j * kRunUserCost;
          w = kRunUserCost;
        } else {
          const int64_t st = (j - cu) * clen;
          d.list_base = F->ib[t] + st;
          d.out_base = F->base[t] + du + st;
          d.pos0 = (int32_t)(du + st);
          d.len = (int32_t)(di - st < clen ? di - st : clen);
          d.side = 1 | (nq << 8);
          p = F->cost[t] + cu * kRunUserCost + (j - cu) * (nq + 2);
          w = nq + 2;
        }
        d.q = (int32_t)qq;
        cdesc[c] = d;
        if (slices)
          for (int64_t sl = (p + (1ll << lsh) - 1) >> lsh; (sl << lsh) < p + w; ++sl) slices[sl] = (int32_t)c;
      }
    }
  }
  // the last tile to finish resets the tile words and the counters for the next launch
  __syncthreads();
  if (threadIdx.x == 0) {
    // this thread published the block's tile words: wait for those stores to be performed
    // before counting the block done, so the last block's reset cannot be overtaken by a
    // straggling publish (the outputs are read by later kernels only)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned done = atomicAdd(&tctr[1], 1u);
    if (done == ntiles - 1) {
      for (unsigned t = 0; t < (MODE == 1 && runs ? 2 * ntiles : ntiles); ++t)
        __hip_atomic_store(&tstate[t], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&tctr[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&tctr[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The scan's launch arguments as a kernel that runs it beside other work carries them
// (k_solve_quad, small_solve.hip); filled by chunk_scan_args (index.hip) after the reserves.
struct ScanArgs {
  const int32_t* qu;
  const int32_t* qi;
  int64_t Q;
  const int64_t* uptr;
  const int64_t* iptr;
  int64_t U, I;
  int64_t* out;
  unsigned long long* tstate;
  unsigned int* tctr;
  int32_t* flag;
  const int64_t* offsets;
  ChunkDesc* cdesc;
  int32_t* zero_word;
  int64_t* qbase;
  int runs, clen, lsh;
  int32_t* slices;
};

template <int MODE>
__device__ __forceinline__ void query_scan_body(const ScanArgs& S) {
  query_scan_body<MODE>(S.qu, S.qi, S.Q, S.uptr, S.iptr, S.U, S.I, S.out, S.tstate, S.tctr, S.flag, S.offsets, S.cdesc,
                        S.zero_word, S.qbase, S.runs, S.clen, S.lsh, S.slices);
}

// build_chunks in two steps (index.hip): the reserves and the scan's arguments, then its launch
// -- or the caller's own launch of a kernel that runs query_scan_body<1> on the first
// scan_tiles(Q) tickets
hipError_t chunk_scan_args(fia_ctx* c, int64_t Q, const int32_t* qu, const int32_t* qi, const int64_t* offsets,
                           int64_t max_chunks, bool offsets_only, hipStream_t s, int32_t* zero_word, bool runs,
                           int slice_cost, int run_chunk, ScanArgs& S);
// ev: the caller's phase events, if any, stamped by the dispatch
hipError_t launch_chunk_scan(const ScanArgs& S, hipStream_t s, hipEvent_t ev_a = nullptr, hipEvent_t ev_b = nullptr);

}  // namespace fia
