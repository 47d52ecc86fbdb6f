// Lane-level device helpers shared by the small-k units (through kern.h) and the large-k units
// (through bigk.h): wave and DPP row reductions and broadcasts, and the top-K order.  Nothing here knows a
// model, a size or a kernel argument struct, so an edit to those reaches no unit through this
// header.  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>
#include <cmath>

namespace fia {

// 4 doubles per lane: an f64 MFMA 16x16 tile (C/D layout: element (4 r + (l >> 4), l & 15) in [r])
typedef double d4_t __attribute__((ext_vector_type(4)));

// lane l's double, broadcast to the wave (v_readlane into SGPRs; l compile-time)
__device__ __forceinline__ double readlane_d(double v, int l) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), l);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

// lane CTRL's double (a DPP control: quad_perm, row_mirror, ...); a disabled source lane gives 0
template <int CTRL>
__device__ __forceinline__ double dpp_d(double x) {
  const long long b = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// sum over the 16 lanes of each row (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror,
// row_mirror); every lane of the row gets the bit-identical sum
__device__ __forceinline__ double row_sum16(double x) {
  x += dpp_d<0xB1>(x);
  x += dpp_d<0x4E>(x);
  x += dpp_d<0x141>(x);
  x += dpp_d<0x140>(x);
  return x;
}
// sum over the 4 rows (lanes c, c+16, c+32, c+48); every lane gets the same sum
__device__ __forceinline__ double col_sum4(double x) {
  const long long b = __double_as_longlong(x);
  const unsigned lo = (unsigned)(b & 0xffffffffll), hi = (unsigned)(b >> 32);
  const auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  const double s = __longlong_as_double(((long long)h16[0] << 32) | l16[0]) +
                   __longlong_as_double(((long long)h16[1] << 32) | l16[1]);   // rows 0+1 | 2+3
  const long long bs = __double_as_longlong(s);
  const unsigned slo = (unsigned)(bs & 0xffffffffll), shi = (unsigned)(bs >> 32);
  const auto l32 = __builtin_amdgcn_permlane32_swap(slo, slo, false, false);
  const auto h32 = __builtin_amdgcn_permlane32_swap(shi, shi, false, false);
  return __longlong_as_double(((long long)h32[0] << 32) | l32[0]) +
         __longlong_as_double(((long long)h32[1] << 32) | l32[1]);
}

// wave-local LDS hand-off: a wave's LDS operations complete in order; this only keeps
// the compiler from moving them across the exchange
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------------
// top-K helpers.  The library's top-K contract, stated here once: the K best candidates by |v|
// descending, then related position ascending, NaN after every real value; fewer than K
// candidates are padded with position -1 and value NaN.  Every selection is K rounds, each
// taking the best candidate (`better`) strictly worse than the previous round's winner, so no
// "taken" marks are needed (positions are unique); invalid lanes carry (-2, INT_MAX, 0).
// ------------------------------------------------------------------------------------
__device__ __forceinline__ double topk_key(double v) {
  double a = fabs(v);
  return (a != a) ? -1.0 : a;     // NaN ranks last among real candidates
}
__device__ __forceinline__ bool better(double a1, int p1, double a2, int p2) {
  return a1 > a2 || (a1 == a2 && p1 < p2);
}

// The best (key, position, value) of the wave, in every lane.  `better` is a strict total
// order on (key, position) -- positions are unique, invalid lanes all carry the same
// (-2, INT_MAX, 0) -- so the result does not depend on the reduction order: DPP row
// rotations inside each 16-lane row, then permlane swaps across the rows (all VALU; the
// ds_bpermute butterfly it replaces waited an LDS round trip per level, six per call)
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int x) {
  // old = x: a disabled source lane returns the lane's own value (a no-op merge)
  return __builtin_amdgcn_update_dpp(x, x, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ void best_take(double& a, int& p, double& v, double oa, int op, double ov) {
  if (better(oa, op, a, p)) { a = oa; p = op; v = ov; }
}
template <int CTRL>
__device__ __forceinline__ void best_dpp_step(double& a, int& p, double& v) {
  const long long ab = __double_as_longlong(a), vb = __double_as_longlong(v);
  const int alo = dpp_i32<CTRL>((int)(ab & 0xffffffffll)), ahi = dpp_i32<CTRL>((int)(ab >> 32));
  const int vlo = dpp_i32<CTRL>((int)(vb & 0xffffffffll)), vhi = dpp_i32<CTRL>((int)(vb >> 32));
  const int op = dpp_i32<CTRL>(p);
  best_take(a, p, v, __longlong_as_double(((long long)ahi << 32) | (unsigned)alo), op,
            __longlong_as_double(((long long)vhi << 32) | (unsigned)vlo));
}
// the other row of the lane's pair: rows 0<->1, 2<->3 (SW32 = false) or 0,1<->2,3 (SW32 = true)
template <bool SW32>
__device__ __forceinline__ unsigned other_rows(unsigned x) {
  const bool up = SW32 ? (threadIdx.x & 32) != 0 : (threadIdx.x & 16) != 0;
  if constexpr (SW32) {
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);   // {[r0 r1 r0 r1], [r2 r3 r2 r3]}
    return up ? r[0] : r[1];
  } else {
    const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);   // {[r0 r0 r2 r2], [r1 r1 r3 r3]}
    return up ? r[0] : r[1];
  }
}
template <bool SW32>
__device__ __forceinline__ void best_row_step(double& a, int& p, double& v) {
  const long long ab = __double_as_longlong(a), vb = __double_as_longlong(v);
  const unsigned alo = other_rows<SW32>((unsigned)(ab & 0xffffffffll)), ahi = other_rows<SW32>((unsigned)(ab >> 32));
  const unsigned vlo = other_rows<SW32>((unsigned)(vb & 0xffffffffll)), vhi = other_rows<SW32>((unsigned)(vb >> 32));
  const int op = (int)other_rows<SW32>((unsigned)p);
  best_take(a, p, v, __longlong_as_double(((long long)ahi << 32) | alo), op,
            __longlong_as_double(((long long)vhi << 32) | vlo));
}
__device__ __forceinline__ void wave_best(double& a, int& p, double& v) {
  best_dpp_step<0x128>(a, p, v);   // row_ror:8
  best_dpp_step<0x124>(a, p, v);   // row_ror:4
  best_dpp_step<0x122>(a, p, v);   // row_ror:2
  best_dpp_step<0x121>(a, p, v);   // row_ror:1 -- every lane of a row holds the row's best
  best_row_step<false>(a, p, v);
  best_row_step<true>(a, p, v);
}

// The best (key, position, value) of a workgroup of NW waves, in every thread (s_*: NW entries)
template <int NW>
__device__ __forceinline__ void block_best(double& ba, int& bp, double& bv, double* s_a, int* s_p, double* s_v) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  wave_best(ba, bp, bv);
  if (NW > 1) {
    if (lane == 0) { s_a[wave] = ba; s_p[wave] = bp; s_v[wave] = bv; }
    __syncthreads();
    ba = s_a[0]; bp = s_p[0]; bv = s_v[0];
#pragma unroll
    for (int w = 1; w < NW; ++w)
      if (better(s_a[w], s_p[w], ba, bp)) { ba = s_a[w]; bp = s_p[w]; bv = s_v[w]; }
    __syncthreads();
  }
}

}  // namespace fia
