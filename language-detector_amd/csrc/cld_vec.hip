// cld_vec.hip -- the device-resident ResultChunkVector path
// (cld_detect_batch_device_vec): the steps cld_detect_batch_vec's host code
// runs between its kernels, as kernels, so nothing comes back to the host.
//
//  k_vec_plan     pool region size of every document (then the scan of
//                 cld_strip.hip gives pool_off, which k_long<VEC> reads)
//  k_vec_finish   after k_long<VEC> (and the UTF-8 fixup): chunk count per
//                 document for the scan into chunk_offsets; a document whose
//                 vector outgrew its region (n_chunks -1) is marked
//                 CLD_LANG_FAILED; failed / rejected documents are counted
//  k_vec_gather_chunks   the vectors from their pool regions into document
//                 order, split over output positions: a workgroup owns a tile
//                 of kGatherTile output chunks whatever documents they belong
//                 to, so a million one-chunk documents and one document of
//                 10^5 chunks both spread over the machine
// LDS: 8 KB of source positions + 8 KB of document boundaries per workgroup.
// Algorithmic bytes: every chunk is read once and written once (12 B each).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cld_kernels.h"

namespace cld {
namespace vec {

constexpr int kGatherTile = 1024;    // output chunks per tile
constexpr int kGatherDocs = 1024;    // document boundaries of a tile held in LDS (more: searched in HBM)
constexpr int kGatherBlock = 256;
constexpr int kGatherGridMax = 2048;

__global__ __launch_bounds__(256) void k_vec_plan(const uint64_t* __restrict__ offs, int n, int mode,
                                                 uint64_t* __restrict__ region) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t len = offs[i + 1] - offs[i];
  region[i] = mode == kVecRegionsBig ? 8 * len + 256 : mode == kVecRegionsOne ? 1 : len + len / 4 + 8;
}

__global__ __launch_bounds__(256) void k_vec_finish(const uint64_t* __restrict__ offs, int n,
                                                   const int32_t* __restrict__ n_chunks,
                                                   const int32_t* __restrict__ vp, cld_result* __restrict__ out,
                                                   uint32_t unknown, uint64_t* __restrict__ counts,
                                                   cld_vec_status* __restrict__ status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool failed = false, rejected = false;
  if (i < n) {
    const int32_t m = n_chunks[i];
    failed = m < 0;
    counts[i] = failed ? 0u : (uint64_t)m;
    if (failed) {                                 // as the header documents CLD_LANG_FAILED
      cld_result r;
      r.lang3[0] = r.lang3[1] = r.lang3[2] = (uint16_t)unknown;
      r.summary_lang = (uint16_t)CLD_LANG_FAILED;
      r.percent3[0] = r.percent3[1] = r.percent3[2] = 0;
      r.is_reliable = 0;
      r.text_bytes = 0;
      r.normalized3[0] = r.normalized3[1] = r.normalized3[2] = 0.0;
      out[i] = r;
    }
    if (vp) {                                     // (k_valid_fixup's test: documents are <= INT32_MAX bytes)
      const uint64_t len = offs[i + 1] - offs[i];
      rejected = vp[i] != (int32_t)(len > 0x7FFFFFFFull ? 0x7FFFFFFFull : len);
    }
  }
  // one atomic per wavefront and counter, none where nothing failed
  const uint64_t mf = __ballot(failed), mr = __ballot(rejected);
  if ((threadIdx.x & 63) == 0) {
    if (mf) atomicAdd(&status->failed_docs, (uint32_t)__popcll(mf));
    if (mr) atomicAdd(&status->rejected_docs, (uint32_t)__popcll(mr));
  }
}

// First index in [lo, hi) whose entry is greater than c; hi if there is none.
__device__ __forceinline__ uint32_t upper(const uint64_t* a, uint32_t lo, uint32_t hi, uint64_t c) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] > c) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// The same over HBM by a whole wavefront (all 64 lanes call it): 64 probes per
// round, so a million entries take four dependent loads where the scalar
// search takes twenty -- the tile's start is a chain of load latencies and
// nothing else.  Wave-uniform result.
__device__ __forceinline__ uint32_t wave_upper(const uint64_t* __restrict__ a, uint32_t lo, uint32_t hi, uint64_t c,
                                               uint32_t lane) {
  while (hi - lo > 64u) {
    const uint32_t step = (hi - lo + 63u) / 64u;         // probes lo + k step, k < 64; those at hi and past count as greater
    const uint32_t p = lo + lane * step;
    const uint64_t m = __ballot(p < hi ? a[p] > c : true);
    const uint32_t f = m ? (uint32_t)__builtin_ctzll(m) : 64u;
    if (f == 0) return lo;
    // a[lo + (f - 1) step] <= c and, where it lies inside, a[lo + f step] > c
    const uint32_t nhi = lo + f * step;
    lo = lo + (f - 1u) * step + 1u;
    hi = nhi < hi ? nhi : hi;
  }
  const uint32_t p = lo + lane;
  const uint64_t m = __ballot(p < hi ? a[p] > c : true);
  return m ? lo + (uint32_t)__builtin_ctzll(m) : hi;
}

// coffs[0..n]: the scan of the chunk counts (coffs[n] = all chunks); the first
// min(coffs[n], cap) chunks go to dst.  Per tile: two wave-wide searches give its
// first and last document, their boundaries go to LDS, every chunk finds its
// document there and leaves its pool position in LDS, and the copy then runs
// over the tile's dwords (three per chunk), consecutive lanes storing
// consecutive dwords.
__global__ __launch_bounds__(kGatherBlock) void k_vec_gather_chunks(const cld_chunk* __restrict__ pool,
                                                                   const uint64_t* __restrict__ pool_off,
                                                                   const uint64_t* __restrict__ coffs, int n,
                                                                   cld_chunk* __restrict__ dst, uint64_t cap,
                                                                   cld_vec_status* __restrict__ status) {
  __shared__ uint64_t s_src[kGatherTile];
  __shared__ uint64_t s_off[kGatherDocs + 1];
  __shared__ uint32_t s_lo, s_hi;
  const uint32_t tid = threadIdx.x;
  const uint64_t total = coffs[n];
  if (blockIdx.x == 0 && tid == 0) status->total_chunks = total;
  const uint64_t lim = total < cap ? total : cap;
  const uint64_t ntiles = (lim + kGatherTile - 1) / kGatherTile;
  const uint32_t* __restrict__ src32 = reinterpret_cast<const uint32_t*>(pool);
  uint32_t* __restrict__ dst32 = reinterpret_cast<uint32_t*>(dst);
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const uint64_t c0 = t * kGatherTile;
    const uint64_t c1 = c0 + kGatherTile < lim ? c0 + kGatherTile : lim;
    // the document of chunk c: the last i with coffs[i] <= c (c < coffs[n], coffs[0] = 0: i in [0, n))
    // (wave 0 finds the tile's first document while wave 1 finds its last)
    if (tid < 128) {
      const uint32_t r = wave_upper(coffs, 0, (uint32_t)n + 1, tid < 64 ? c0 : c1 - 1, tid & 63u) - 1;
      if ((tid & 63u) == 0) (tid ? s_hi : s_lo) = r;
    }
    __syncthreads();
    const uint32_t lo = s_lo, nd = s_hi - lo + 1;
    const bool staged = nd <= (uint32_t)kGatherDocs;    // (a long run of empty documents inside the tile: not)
    if (staged)
      for (uint32_t k = tid; k <= nd; k += kGatherBlock) s_off[k] = coffs[lo + k];
    __syncthreads();
    for (uint64_t c = c0 + tid; c < c1; c += kGatherBlock) {
      uint32_t i;
      uint64_t first;
      if (staged) {
        const uint32_t k = upper(s_off, 0, nd, c) - 1;
        i = lo + k;
        first = s_off[k];
      } else {
        i = upper(coffs, lo, lo + nd, c) - 1;
        first = coffs[i];
      }
      s_src[c - c0] = pool_off[i] + (c - first);
    }
    __syncthreads();
    const uint32_t ndw = 3u * (uint32_t)(c1 - c0);
    for (uint32_t j = tid; j < ndw; j += kGatherBlock) {
      const uint32_t q = j / 3u;
      dst32[3 * c0 + j] = src32[3 * s_src[q] + (j - 3u * q)];
    }
    __syncthreads();
  }
}

}  // namespace vec
}  // namespace cld

extern "C" {
hipError_t cld_launch_vec_plan(const uint64_t* offs, int n, int mode, uint64_t* region, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(cld::vec::k_vec_plan, dim3((n + 255) / 256), dim3(256), 0, s, offs, n, mode, region);
  return hipGetLastError();
}

hipError_t cld_launch_vec_finish(const uint64_t* offs, int n, const int32_t* n_chunks, const int32_t* valid_prefix,
                                 cld_result* out, uint32_t unknown_language, uint64_t* counts, cld_vec_status* status,
                                 hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(cld::vec::k_vec_finish, dim3((n + 255) / 256), dim3(256), 0, s, offs, n, n_chunks, valid_prefix,
                     out, unknown_language, counts, status);
  return hipGetLastError();
}

hipError_t cld_launch_vec_gather_chunks(const cld_chunk* pool, const uint64_t* pool_off, const uint64_t* chunk_offs,
                                        int n, cld_chunk* dst, uint64_t cap, cld_vec_status* status, hipStream_t s) {
  using namespace cld::vec;
  if (n <= 0) return hipSuccess;
  // the host knows no chunk count, only the room: a grid-stride loop over the tiles there are
  const uint64_t tiles = (cap + kGatherTile - 1) / kGatherTile;
  const unsigned grid = (unsigned)std::min<uint64_t>(std::max<uint64_t>(tiles, 1), kGatherGridMax);
  hipLaunchKernelGGL(k_vec_gather_chunks, dim3(grid), dim3(kGatherBlock), 0, s, pool, pool_off, chunk_offs, n, dst,
                     cap, status);
  return hipGetLastError();
}
}
