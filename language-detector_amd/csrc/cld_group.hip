// cld_group.hip -- a device-resident batch grouped by language, and the
// chosen documents packed into a new batch (cld_group_by_language_device,
// cld_gather_docs_device).
//
// Group: a stable counting sort of the document indices over CLD_GROUP_BINS
// keys.  The batch is cut into at most kGroupWgs contiguous ranges, one per
// workgroup, whatever n is (group_range), so the workspace does not grow with n:
//   k_group_hist     per range, the histogram of its documents (and their byte
//                    totals) in LDS, written to hist[g][bin] / bytes[g][bin]
//   k_group_scan     one wave per bin: the scan of hist[.][bin] over the
//                    ranges, in place (a range's first position within its
//                    bin), the bin's count and its byte total
//   k_group_scatter  per range: the scan of the counts over the bins (every
//                    workgroup makes its own copy in LDS; workgroup 0 writes
//                    it out), then index i to
//                      group_offsets[bin] + hist[g][bin] + rank within the range
//                    The key is computed again from the result, not stored.
// The rank within the range: a workgroup walks its range kGroupTile documents
// at a time, its waves take their turn at the LDS cursors in document order,
// and within a wave the rank among equal keys is the popcount of the lower
// lanes that hold the same key.  No atomic decides a position, so the order is
// the same from run to run.
//
// Gather: lengths -> 64-bit exclusive scan -> copy.
//   k_gather_len     out_offs[j] = length of document index[j] (0 for an index
//                    past the source), per-range sums to the workspace
//   k_gather_scan    per range: the sum of the ranges before it, then the scan
//                    of its own lengths in place; the last range writes out_offs[m]
//   k_gather_copy    the output cut into tiles of kCopyTile bytes at 16-byte
//                    aligned output addresses, a fixed grid striding over them;
//                    each wave finds the documents of the first and the last
//                    of its kCopyWave bytes by a 64-way search in out_offs,
//                    each lane the document of each of its 16-byte pieces
//                    between the two.
// Every launch is complete before the next one reads what it wrote (one
// stream): no workgroup ever waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cld_kernels.h"
#include "cld_wgscan.h"

namespace cld {
namespace group {

using wg::block_incl_scan;
using wg::wave_find;

constexpr int kBins = (int)CLD_GROUP_BINS;
constexpr int kTile = kGroupTile;          // documents per step = threads per workgroup
constexpr int kWaves = kTile / 64;
constexpr int kScanWaves = 4;              // k_group_scan: bins (waves) per workgroup
constexpr int kPerLane = kGroupWgs / 64;   // k_group_scan: ranges per lane
constexpr int kCopyBlock = 256;            // k_gather_copy: a lane takes kCopyChunks times 16 bytes, 1 KB apart,
constexpr int kCopyChunks = 4;             // of its wave's kCopyWave bytes
constexpr int kCopyWave = 64 * 16 * kCopyChunks;
constexpr int kCopyTile = kCopyBlock / 64 * kCopyWave;
constexpr int kCopyWgs = 2048;
static_assert(kBins <= 1024, "peers() compares 10 key bits");
static_assert(kBins <= 2 * kTile, "k_group_scatter scans two bins per thread");
static_assert(kGroupWgs % 64 == 0 && kGroupWgs <= kTile, "k_group_scan / k_gather_scan read the ranges at once");

// The bin of document i: min(key, CLD_NUM_LANGUAGES).  flags is the same for every lane.
__device__ __forceinline__ uint32_t doc_bin(const cld_result* __restrict__ res, uint32_t i, uint32_t flags) {
  const uint32_t* w = (const uint32_t*)(res + i);        // lang3[0..1] | lang3[2], summary_lang | percent3, is_reliable
  uint32_t key = (flags & CLD_GROUP_TOP1) ? (w[0] & 0xFFFFu) : (w[1] >> 16);
  if ((flags & CLD_GROUP_RELIABLE_ONLY) && (w[2] >> 24) == 0) key = 26;   // UNKNOWN_LANGUAGE
  return key < CLD_NUM_LANGUAGES ? key : CLD_NUM_LANGUAGES;
}

// The lanes of the wave that are valid and hold this lane's bin (whole wave converged).
__device__ __forceinline__ uint64_t peers(uint32_t bin, bool valid) {
  uint64_t m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 10; ++b) {
    const bool bit = (bin >> b) & 1;
    const uint64_t s = __ballot(bit);
    m &= bit ? s : ~s;
  }
  return m;
}

__global__ __launch_bounds__(kTile) void k_group_hist(const cld_result* __restrict__ res, uint32_t n, uint32_t range,
                                                     uint32_t flags, const uint64_t* __restrict__ offs,
                                                     uint32_t* __restrict__ hist, uint64_t* __restrict__ bytes) {
  __shared__ uint32_t h[kBins];
  __shared__ unsigned long long hb[kBins];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int b = tid; b < kBins; b += kTile) {
    h[b] = 0;
    hb[b] = 0;
  }
  __syncthreads();
  const uint32_t lo = blockIdx.x * range, hi = min(n, lo + range);
  for (uint32_t t = lo; t < hi; t += kTile) {
    const uint32_t i = t + tid;
    const bool valid = i < hi;
    const uint32_t bin = valid ? doc_bin(res, i, flags) : 0;
    const uint64_t m = peers(bin, valid);
    if (valid) {
      if ((m & ((1ull << lane) - 1)) == 0) atomicAdd(&h[bin], (uint32_t)__popcll(m));   // one add per key of the wave
      if (offs) atomicAdd(&hb[bin], (unsigned long long)(offs[i + 1] - offs[i]));
    }
  }
  __syncthreads();
  for (int b = tid; b < kBins; b += kTile) {
    hist[(size_t)blockIdx.x * kBins + b] = h[b];
    if (offs) bytes[(size_t)blockIdx.x * kBins + b] = hb[b];
  }
}

// One wave per bin; lane l holds ranges kPerLane * l .. kPerLane * l + kPerLane - 1.
__global__ __launch_bounds__(64 * kScanWaves) void k_group_scan(uint32_t* __restrict__ hist,
                                                               const uint64_t* __restrict__ bytes, uint32_t nwg,
                                                               uint32_t* __restrict__ cnt, uint64_t* __restrict__ counts,
                                                               uint64_t* __restrict__ bin_bytes) {
  const int lane = threadIdx.x & 63;
  const uint32_t b = blockIdx.x * kScanWaves + (threadIdx.x >> 6);
  if (b >= (uint32_t)kBins) return;
  uint32_t v[kPerLane], sum = 0;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const uint32_t g = kPerLane * lane + k;
    v[k] = g < nwg ? hist[(size_t)g * kBins + b] : 0;
    sum += v[k];
  }
  uint32_t inc = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(inc, d, 64);
    if (lane >= d) inc += y;
  }
  uint32_t at = inc - sum;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const uint32_t g = kPerLane * lane + k;
    if (g < nwg) hist[(size_t)g * kBins + b] = at;
    at += v[k];
  }
  if (lane == 63) {
    cnt[b] = inc;
    if (counts) counts[b] = inc;
  }
  if (bin_bytes) {
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      const uint32_t g = kPerLane * lane + k;
      s += g < nwg ? bytes[(size_t)g * kBins + b] : 0;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) bin_bytes[b] = s;
  }
}

// order == nullptr: one workgroup, for the group offsets alone.
__global__ __launch_bounds__(kTile) void k_group_scatter(const cld_result* __restrict__ res, uint32_t n, uint32_t range,
                                                        uint32_t flags, const uint32_t* __restrict__ rel,
                                                        const uint32_t* __restrict__ cnt, uint32_t* __restrict__ order,
                                                        uint64_t* __restrict__ group_offsets) {
  __shared__ uint32_t base[kBins + 1];
  __shared__ uint32_t sm[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  {
    const int b0 = 2 * tid, b1 = b0 + 1;
    const uint32_t c0 = b0 < kBins ? cnt[b0] : 0, c1 = b1 < kBins ? cnt[b1] : 0;
    const uint32_t inc = block_incl_scan<uint32_t, kWaves>(c0 + c1, sm);
    if (b0 < kBins) base[b0] = inc - c1 - c0;
    if (b1 < kBins) base[b1] = inc - c1;
  }
  __syncthreads();
  if (blockIdx.x == 0 && group_offsets) {
    for (int b = tid; b < kBins; b += kTile) group_offsets[b] = base[b];
    if (tid == 0) group_offsets[kBins] = n;
  }
  if (!order) return;
  __syncthreads();
  for (int b = tid; b < kBins; b += kTile) base[b] += rel[(size_t)blockIdx.x * kBins + b];
  __syncthreads();
  const uint32_t lo = blockIdx.x * range, hi = min(n, lo + range);
  for (uint32_t t = lo; t < hi; t += kTile) {
    const uint32_t i = t + tid;
    const bool valid = i < hi;
    const uint32_t bin = valid ? doc_bin(res, i, flags) : 0;
    const uint64_t m = peers(bin, valid);
    const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1));
    uint32_t pos = 0;
    for (int w = 0; w < kWaves; ++w) {       // the waves in document order, each key's first lane moves its cursor
      if (wave == w && valid && rank == 0) {
        pos = base[bin];
        base[bin] = pos + (uint32_t)__popcll(m);
      }
      __syncthreads();
    }
    pos = __shfl(pos, valid ? __ffsll((unsigned long long)m) - 1 : lane, 64);
    if (valid) order[pos + rank] = i;
  }
}

// ---------------------------------------------------------------- gather

__global__ __launch_bounds__(kTile) void k_gather_len(const uint64_t* __restrict__ offs, uint32_t n_src,
                                                     const uint32_t* __restrict__ index, uint32_t m, uint32_t range,
                                                     uint64_t* __restrict__ out_offs, uint64_t* __restrict__ sums) {
  __shared__ uint64_t sm[kWaves];
  const uint32_t lo = blockIdx.x * range, hi = min(m, lo + range);
  uint64_t s = 0;
  for (uint32_t j = lo + threadIdx.x; j < hi; j += kTile) {
    const uint32_t i = index[j];
    uint64_t len = 0;
    if (i < n_src) {
      const uint64_t a = offs[i], b = offs[i + 1];
      len = b > a ? b - a : 0;
    }
    out_offs[j] = len;
    s += len;
  }
  const uint64_t inc = block_incl_scan<uint64_t, kWaves>(s, sm);
  if (threadIdx.x == kTile - 1) sums[blockIdx.x] = inc;
}

__global__ __launch_bounds__(kTile) void k_gather_scan(uint32_t m, uint32_t range, uint64_t* __restrict__ out_offs,
                                                      const uint64_t* __restrict__ sums) {
  __shared__ uint64_t sm[kWaves];
  __shared__ uint64_t carry;
  const uint32_t tid = threadIdx.x;
  {
    const uint64_t inc = block_incl_scan<uint64_t, kWaves>(tid < blockIdx.x ? sums[tid] : 0, sm);
    if (tid == kTile - 1) carry = inc;
  }
  __syncthreads();
  const uint32_t lo = blockIdx.x * range, hi = min(m, lo + range);
  for (uint32_t t = lo; t < hi; t += kTile) {
    const uint32_t j = t + tid;
    const uint64_t v = j < hi ? out_offs[j] : 0;
    const uint64_t inc = block_incl_scan<uint64_t, kWaves>(v, sm);
    const uint64_t c = carry;
    __syncthreads();
    if (j < hi) out_offs[j] = c + inc - v;
    if (tid == kTile - 1) carry = c + inc;
    __syncthreads();
  }
  if (hi == m && tid == 0) out_offs[m] = carry;
}

// Output bytes [c0, c1) of one lane, at most 16 and 16-byte aligned when 16; their documents lie in [j0, j1].
// Returns the document of byte c0.
__device__ __forceinline__ uint32_t copy_lane(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ offs,
                                          const uint32_t* __restrict__ index, const uint64_t* __restrict__ out_offs,
                                          uint8_t* __restrict__ out, uint32_t j0, uint32_t j1, int64_t c0, int64_t c1) {
  uint32_t j = j0, e = j1 + 1;                            // out_offs[j0] <= c0 < out_offs[j1 + 1]
  while (e - j > 1) {
    const uint32_t mid = j + (e - j) / 2;
    if (out_offs[mid] <= (uint64_t)c0) j = mid; else e = mid;
  }
  const uint32_t first = j;
  uint64_t at = out_offs[j], end = out_offs[j + 1];
  const uint8_t* src = buf + offs[index[j]];
  auto byte_at = [&](uint64_t p) -> uint32_t {            // output byte p, for p going up (p < out_offs[m]: the walk ends)
    if (p >= end) {
      do { ++j; end = out_offs[j + 1]; } while (p >= end);
      at = out_offs[j];
      src = buf + offs[index[j]];
    }
    return src[p - at];
  };
  if (c1 - c0 == 16) {                                    // the store is aligned, the loads need not be
    uint4 v;
    if (end >= (uint64_t)c1) {                            // 16 bytes of one document
      __builtin_memcpy(&v, src + ((uint64_t)c0 - at), 16);
    } else {                                              // of several: put together byte by byte, stored at once
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int b = 0; b < 16; ++b) w[b >> 2] |= byte_at((uint64_t)c0 + b) << (8 * (b & 3));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *(uint4*)(out + c0) = v;
    return first;
  }
  for (int64_t p = c0; p < c1; ++p) out[p] = (uint8_t)byte_at((uint64_t)p);   // a cut piece: the output's first or last
  return first;
}

__global__ __launch_bounds__(kCopyBlock) void k_gather_copy(const uint8_t* __restrict__ buf,
                                                           const uint64_t* __restrict__ offs,
                                                           const uint32_t* __restrict__ index, uint32_t m,
                                                           const uint64_t* __restrict__ out_offs,
                                                           uint8_t* __restrict__ out, uint64_t cap) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t limit = (int64_t)min(out_offs[m], cap);
  const int64_t skew = (int64_t)((uintptr_t)out & 15);    // position -skew is 16-byte aligned
  const int64_t ntiles = (limit + skew + kCopyTile - 1) / kCopyTile;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t w0 = tile * kCopyTile + (tid >> 6) * kCopyWave - skew;      // the wave's positions
    const int64_t wf = max(w0, (int64_t)0), wl = min(w0 + kCopyWave, limit) - 1;
    if (wf > wl) continue;
    const uint32_t j0 = wave_find(out_offs, 0, m, (uint64_t)wf, lane);
    const uint32_t j1 = out_offs[j0 + 1] > (uint64_t)wl ? j0 : wave_find(out_offs, j0, m, (uint64_t)wl, lane);
    uint32_t j = j0;                                      // (the pieces go up: each starts its search where the last one began)
#pragma unroll
    for (int k = 0; k < kCopyChunks; ++k) {
      const int64_t c = w0 + k * 1024 + lane * 16, c0 = max(c, (int64_t)0), c1 = min(c + 16, limit);
      if (c0 < c1) j = copy_lane(buf, offs, index, out_offs, out, j, j1, c0, c1);
    }
  }
}

}  // namespace group
}  // namespace cld

extern "C" {
hipError_t cld_launch_group(const cld_result* res, uint32_t n, uint32_t flags, const uint64_t* offs, uint64_t* counts,
                            uint64_t* bin_bytes, uint32_t* order, uint64_t* group_offsets, void* work, hipStream_t s) {
  using namespace cld::group;
  if (n == 0) return hipSuccess;
  const uint32_t range = cld_group_range(n), nwg = (n + range - 1) / range;
  uint32_t* hist = (uint32_t*)work;
  uint64_t* bytes = (uint64_t*)(hist + (size_t)kGroupWgs * kBins);
  uint32_t* cnt = (uint32_t*)(bytes + (size_t)kGroupWgs * kBins);
  hipLaunchKernelGGL(k_group_hist, dim3(nwg), dim3(kTile), 0, s, res, n, range, flags, bin_bytes ? offs : nullptr, hist,
                     bytes);
  hipLaunchKernelGGL(k_group_scan, dim3((kBins + kScanWaves - 1) / kScanWaves), dim3(64 * kScanWaves), 0, s, hist, bytes,
                     nwg, cnt, counts, bin_bytes);
  if (order || group_offsets)
    hipLaunchKernelGGL(k_group_scatter, dim3(order ? nwg : 1), dim3(kTile), 0, s, res, n, range, flags, hist, cnt, order,
                       group_offsets);
  return hipGetLastError();
}

hipError_t cld_launch_gather(const uint8_t* buf, const uint64_t* offs, uint32_t n_src, const uint32_t* index, uint32_t m,
                             uint8_t* out, uint64_t cap, uint64_t* out_offs, void* work, hipStream_t s) {
  using namespace cld::group;
  if (m == 0) return hipSuccess;
  const uint32_t range = cld_group_range(m), nwg = (m + range - 1) / range;
  uint64_t* sums = (uint64_t*)work;
  hipLaunchKernelGGL(k_gather_len, dim3(nwg), dim3(kTile), 0, s, offs, n_src, index, m, range, out_offs, sums);
  hipLaunchKernelGGL(k_gather_scan, dim3(nwg), dim3(kTile), 0, s, m, range, out_offs, sums);
  if (cap)
    hipLaunchKernelGGL(k_gather_copy, dim3(kCopyWgs), dim3(kCopyBlock), 0, s, buf, offs, index, m, out_offs, out, cap);
  return hipGetLastError();
}
}
