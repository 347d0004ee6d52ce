// cld_wgscan.h -- the workgroup scan and the wave-wide search that the group
// entries (cld_group.hip) and the chunk entries (cld_chunks.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cld {
namespace wg {

// Inclusive scan over the workgroup's W waves (sm: W entries; safe to call again at once).
template <typename T, int W>
__device__ __forceinline__ T block_incl_scan(T v, T* sm) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T y = __shfl_up(v, d, 64);
    if (lane >= d) v += y;
  }
  __syncthreads();                          // (an earlier call's sm has been read)
  if (lane == 63) sm[w] = v;
  __syncthreads();
  T before = 0;
#pragma unroll
  for (int k = 0; k < W; ++k) before += k < w ? sm[k] : 0;
  return v + before;
}

// The largest j in [lo, hi) with off[j] <= p, given off[lo] <= p < off[hi]; the whole wave, 64 probes a step.
__device__ __forceinline__ uint32_t wave_find(const uint64_t* __restrict__ off, uint32_t lo, uint32_t hi, uint64_t p,
                                              int lane) {
  while (hi - lo > 1) {
    const uint32_t step = (hi - lo + 63) / 64;
    const uint64_t q = lo + (uint64_t)(lane + 1) * step;
    const bool le = q < hi && off[q] <= p;
    lo += (uint32_t)__popcll(__ballot(le)) * step;       // (off does not decrease: the lanes that hold are the first ones)
    hi = min(hi, lo + step);
  }
  return lo;
}

}  // namespace wg
}  // namespace cld
