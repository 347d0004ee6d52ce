// cld_chunks.hip -- the chunk vectors of a device-resident batch: per-language
// totals over the chunks, and the pieces in chosen languages packed into a new
// batch (cld_chunk_totals_device, cld_gather_chunks_device).
//
// Document i's vector is chunks[min(co[i], cap) .. min(co[i + 1], cap)), empty
// when inverted; nothing else is assumed of chunk_offsets (co), so a chunk's
// document is never looked up in co itself.  Every chunk word is clipped to its
// document (piece_of) before it addresses anything.
//
// Totals: the documents are cut into at most kGroupWgs contiguous ranges, one
// workgroup each.
//   k_chunk_hist     walks its range kTile documents at a time: the scan of
//                    their vector lengths in LDS, then the chunks of those
//                    documents kTile at a time, each lane finding its chunk's
//                    document by a search in that scan -- a tweet's single chunk
//                    and a page's thousand fill the lanes alike; counts and
//                    bytes per bin in LDS, written to the workspace per range
//   k_chunk_reduce   one wave per bin: the sum over the ranges
//
// Gather: vector lengths -> scan -> output lengths -> scan -> copy -> offsets.
// Chunk "instance" v is the v-th chunk of the batch in document order.
//   k_chunk_vlen     out_offs[i] = length of document i's vector, per-range sums
//   k_chunk_scan     (over the n documents) out_offs = V: V[i] the first instance
//                    of document i, V[n] the number of instances
//   k_chunk_len      one lane per instance, over J = min(V[n], cap) instances cut
//                    into kGroupWgs ranges on the device: its document by a
//                    search in V, pos[v] = output length of its piece (the 0x20
//                    of CLD_CHUNKS_SPACE included), per-range sums
//   k_chunk_scan     (over the J instances) pos[v] = output position of piece v,
//                    pos[J] = the output's length
//   k_chunk_copy     the output cut into tiles at 16-byte aligned addresses, as
//                    k_gather_copy: the wave finds the pieces and documents of
//                    the first and last of its bytes by 64-way searches in pos
//                    and V, each lane those of its 16 bytes between the two
//   k_chunk_offs     out_offs[i] = pos[V[i]], in place
// The instances of one call are at most cap when no two vectors overlap; J is
// clamped to cap for the inputs where they do, so pos (cap + 1 words) holds.
// Every launch is complete before the next one reads what it wrote (one
// stream); no atomic decides a position or a byte (the LDS atomics add integers).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cld_kernels.h"
#include "cld_wgscan.h"

namespace cld {
namespace chunks {

using wg::block_incl_scan;
using wg::wave_find;

constexpr int kBins = (int)CLD_GROUP_BINS;
constexpr int kTile = kGroupTile;
constexpr int kWaves = kTile / 64;
constexpr int kWgs = kGroupWgs;
constexpr int kReduceWaves = 4;
constexpr int kPerLane = kWgs / 64;
constexpr int kCopyBlock = 256;
constexpr int kCopyChunks = 4;
constexpr int kCopyWave = 64 * 16 * kCopyChunks;
constexpr int kCopyTile = kCopyBlock / 64 * kCopyWave;
constexpr int kCopyWgs = 2048;
constexpr uint64_t kMaxInstances = CLD_CHUNKS_MAX;   // ranges and wave_find steps stay within 32 bits
static_assert(kWgs % 64 == 0 && kWgs <= kTile, "k_chunk_scan / k_chunk_reduce read the ranges at once");

// Items per range for m items cut into at most kWgs ranges, a multiple of kTile (cld_group_range on the device).
__device__ __forceinline__ uint32_t range_of(uint32_t m) {
  const uint32_t per = m / kWgs + (m % kWgs != 0);
  return per <= (uint32_t)kTile ? (uint32_t)kTile : (per + kTile - 1) / kTile * kTile;
}

struct Piece {
  int64_t s, e;      // [s, e) of the document, 0 <= s <= e <= len
  uint32_t bin;
};

// The clipped piece of a chunk in a document of len bytes, and its bin.
__device__ __forceinline__ Piece piece_of(const cld_chunk* __restrict__ ch, int64_t len) {
  const int32_t off = ch->offset, bytes = ch->bytes;
  const uint32_t lang = ch->lang1;
  Piece p;
  p.s = min(max((int64_t)off, (int64_t)0), len);
  p.e = min(max((int64_t)off + bytes, p.s), len);
  p.bin = lang < CLD_NUM_LANGUAGES ? lang : CLD_NUM_LANGUAGES;
  return p;
}

__device__ __forceinline__ int64_t doc_len(const uint64_t* __restrict__ offs, uint32_t i) {
  const uint64_t a = offs[i], b = offs[i + 1];
  return b > a ? (int64_t)(b - a) : 0;
}

// ---------------------------------------------------------------- totals

__global__ __launch_bounds__(kTile) void k_chunk_hist(const uint64_t* __restrict__ offs, uint32_t n, uint32_t range,
                                                     const cld_chunk* __restrict__ chunks,
                                                     const uint64_t* __restrict__ co, uint64_t cap,
                                                     uint64_t* __restrict__ hist) {
  __shared__ unsigned long long hc[kBins], hb[kBins];
  __shared__ uint64_t vs[kTile + 1];         // the first chunk of each document of the step, among the step's
  __shared__ uint32_t va[kTile];             // its first chunk in chunks
  __shared__ uint64_t sm[kWaves];
  const int tid = threadIdx.x;
  for (int b = tid; b < kBins; b += kTile) {
    hc[b] = 0;
    hb[b] = 0;
  }
  const uint32_t lo = blockIdx.x * range, hi = min(n, lo + range);
  for (uint32_t t = lo; t < hi; t += kTile) {
    const uint32_t i = t + tid;
    uint64_t a = 0, vl = 0;
    if (i < hi) {
      a = min(co[i], cap);
      const uint64_t b = min(co[i + 1], cap);
      vl = b > a ? b - a : 0;
    }
    const uint64_t inc = block_incl_scan<uint64_t, kWaves>(vl, sm);
    vs[tid] = inc - vl;
    va[tid] = (uint32_t)a;                   // (a < cap <= UINT32_MAX where the vector is not empty)
    if (tid == kTile - 1) vs[kTile] = inc;
    __syncthreads();
    const uint64_t total = vs[kTile];
    for (uint64_t q = 0; q < total; q += kTile) {
      const uint64_t v = q + tid;
      if (v < total) {
        int d = 0, e = kTile;                // vs[0] = 0 <= v < vs[kTile]
        while (e - d > 1) {
          const int mid = (d + e) >> 1;
          if (vs[mid] <= v) d = mid; else e = mid;
        }
        const Piece p = piece_of(chunks + (va[d] + (v - vs[d])), doc_len(offs, t + d));
        atomicAdd(&hc[p.bin], 1ull);
        atomicAdd(&hb[p.bin], (unsigned long long)(p.e - p.s));
      }
    }
    __syncthreads();                         // (vs and va are rewritten)
  }
  __syncthreads();
  for (int b = tid; b < kBins; b += kTile) {
    hist[((size_t)blockIdx.x * 2) * kBins + b] = hc[b];
    hist[((size_t)blockIdx.x * 2 + 1) * kBins + b] = hb[b];
  }
}

// One wave per bin; lane l sums ranges kPerLane * l .. kPerLane * l + kPerLane - 1.
__global__ __launch_bounds__(64 * kReduceWaves) void k_chunk_reduce(const uint64_t* __restrict__ hist, uint32_t nwg,
                                                                   uint64_t* __restrict__ counts,
                                                                   uint64_t* __restrict__ bytes) {
  const int lane = threadIdx.x & 63;
  const uint32_t b = blockIdx.x * kReduceWaves + (threadIdx.x >> 6);
  if (b >= (uint32_t)kBins) return;
  uint64_t c = 0, s = 0;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const uint32_t g = kPerLane * lane + k;
    if (g < nwg) {
      c += hist[((size_t)g * 2) * kBins + b];
      s += hist[((size_t)g * 2 + 1) * kBins + b];
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    c += __shfl_xor(c, d, 64);
    s += __shfl_xor(s, d, 64);
  }
  if (lane == 0) {
    if (counts) counts[b] = c;
    if (bytes) bytes[b] = s;
  }
}

// ---------------------------------------------------------------- gather

// hdr (the workspace's first words): the instances J, then the per-range sums of the two scans.
enum { kHdrJ = 0, kHdrSumsDoc = 8, kHdrSumsInst = kHdrSumsDoc + kWgs, kHdrWords = kHdrSumsInst + kWgs };

__global__ __launch_bounds__(kTile) void k_chunk_vlen(const uint64_t* __restrict__ co, uint64_t cap, uint32_t n,
                                                     uint32_t range, uint64_t* __restrict__ out_offs,
                                                     uint64_t* __restrict__ sums) {
  __shared__ uint64_t sm[kWaves];
  const uint32_t lo = blockIdx.x * range, hi = min(n, lo + range);
  uint64_t s = 0;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += kTile) {
    const uint64_t a = min(co[i], cap), b = min(co[i + 1], cap);
    const uint64_t vl = b > a ? b - a : 0;
    out_offs[i] = vl;
    s += vl;
  }
  const uint64_t inc = block_incl_scan<uint64_t, kWaves>(s, sm);
  if (threadIdx.x == kTile - 1) sums[blockIdx.x] = inc;
}

// The exclusive scan of arr[0..m) in place and arr[m] = the total, m = *mp (nullable) clamped to mcap; a grid
// of kWgs, the ranges of range_of(m); sums: the sum of every range that holds an item.
__global__ __launch_bounds__(kTile) void k_chunk_scan(const uint64_t* __restrict__ mp, uint64_t mcap,
                                                     uint64_t* __restrict__ arr, const uint64_t* __restrict__ sums) {
  __shared__ uint64_t sm[kWaves];
  __shared__ uint64_t carry;
  const uint32_t tid = threadIdx.x;
  const uint32_t m = (uint32_t)(mp ? min(*mp, mcap) : mcap);
  const uint32_t range = range_of(m);
  const uint32_t lo = blockIdx.x * range;
  if (blockIdx.x > 0 && lo >= m) return;     // (whole workgroup; the range of workgroup 0 always counts)
  {
    const uint64_t inc = block_incl_scan<uint64_t, kWaves>(tid < blockIdx.x ? sums[tid] : 0, sm);
    if (tid == kTile - 1) carry = inc;
  }
  __syncthreads();
  const uint32_t hi = min(m, lo + range);
  for (uint32_t t = lo; t < hi; t += kTile) {
    const uint32_t j = t + tid;
    const uint64_t v = j < hi ? arr[j] : 0;
    const uint64_t inc = block_incl_scan<uint64_t, kWaves>(v, sm);
    const uint64_t c = carry;
    __syncthreads();
    if (j < hi) arr[j] = c + inc - v;
    if (tid == kTile - 1) carry = c + inc;
    __syncthreads();
  }
  if (hi == m && tid == 0) arr[m] = carry;
}

// The documents of instances v0 <= v1 of one wave: i0, i1 with V[i0] <= v0 < V[i0 + 1] and likewise i1.
__device__ __forceinline__ void wave_docs(const uint64_t* __restrict__ V, uint32_t n, uint64_t v0, uint64_t v1, int lane,
                                          uint32_t* i0, uint32_t* i1) {
  *i0 = wave_find(V, 0, n, v0, lane);
  *i1 = V[*i0 + 1] > v1 ? *i0 : wave_find(V, *i0, n, v1, lane);
}

// The largest j in [lo, hi] with off[j] <= p, given off[lo] <= p < off[hi + 1]; one lane.
__device__ __forceinline__ uint32_t lane_find(const uint64_t* __restrict__ off, uint32_t lo, uint32_t hi, uint64_t p) {
  uint32_t j = lo, e = hi + 1;
  while (e - j > 1) {
    const uint32_t mid = j + (e - j) / 2;
    if (off[mid] <= p) j = mid; else e = mid;
  }
  return j;
}

__global__ __launch_bounds__(kTile) void k_chunk_len(const uint64_t* __restrict__ offs, uint32_t n,
                                                    const cld_chunk* __restrict__ chunks,
                                                    const uint64_t* __restrict__ co, uint64_t cap,
                                                    const uint8_t* __restrict__ select, uint32_t flags,
                                                    const uint64_t* __restrict__ V, uint64_t* __restrict__ pos,
                                                    uint64_t* __restrict__ hdr) {
  __shared__ uint64_t sm[kWaves];
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t J = (uint32_t)min(V[n], min(cap, kMaxInstances));
  if (blockIdx.x == 0 && tid == 0) hdr[kHdrJ] = J;
  const uint32_t range = range_of(J);
  const uint32_t lo = min((uint64_t)J, (uint64_t)blockIdx.x * range), hi = min((uint64_t)J, (uint64_t)lo + range);
  uint64_t s = 0;
  for (uint32_t t = lo; t < hi; t += kTile) {
    const uint32_t w0 = t + (tid & ~63);                 // the wave's first instance
    if (w0 >= hi) continue;                              // (whole wave)
    uint32_t i0, i1;
    wave_docs(V, n, w0, min(w0 + 63, hi - 1), lane, &i0, &i1);
    const uint32_t v = t + tid;
    if (v >= hi) continue;
    const uint32_t i = lane_find(V, i0, i1, v);
    const uint64_t first = V[i];
    const int64_t len = doc_len(offs, i);
    const uint64_t c = min(co[i], cap) + (v - first);    // < min(co[i + 1], cap)
    const Piece p = piece_of(chunks + c, len);
    uint64_t out = 0;
    if (select[p.bin] && p.e > p.s) {
      out = (uint64_t)(p.e - p.s);
      if ((flags & CLD_CHUNKS_SPACE) && v != first) {
        const Piece q = piece_of(chunks + (c - 1), len);
        if (!(select[q.bin] && q.e > q.s && q.e == p.s)) ++out;
      }
    }
    pos[v] = out;
    s += out;
  }
  const uint64_t inc = block_incl_scan<uint64_t, kWaves>(s, sm);
  if (tid == kTile - 1) hdr[kHdrSumsInst + blockIdx.x] = inc;
}

// One lane's place in the output: piece v of document i, output bytes [at, end), the source of byte at.
struct Cursor {
  const uint8_t* __restrict__ buf;
  const uint64_t* __restrict__ offs;
  const cld_chunk* __restrict__ chunks;
  const uint64_t* __restrict__ co;
  const uint64_t* __restrict__ V;
  const uint64_t* __restrict__ pos;
  uint64_t cap;
  uint32_t v, i;
  uint64_t at, end, next_doc;      // next_doc = V[i + 1]
  const uint8_t* src;              // output byte p of the piece is src[p - at] (p - at == -1: the 0x20)
  bool space;

  __device__ __forceinline__ void load() {      // v, i set; end = pos[v + 1] > at = pos[v]
    const Piece p = piece_of(chunks + (min(co[i], cap) + (v - V[i])), doc_len(offs, i));
    space = end - at > (uint64_t)(p.e - p.s);
    src = buf + offs[i] + p.s;
    if (space) ++at;
  }
  __device__ __forceinline__ uint32_t byte_at(uint64_t p) {   // for p going up, p < pos[J]: the walk ends
    if (p >= end) {
      do { ++v; end = pos[v + 1]; } while (p >= end);
      at = pos[v];
      while (v >= next_doc) { ++i; next_doc = V[i + 1]; }
      load();
    }
    return p < at ? 0x20u : src[p - at];
  }
};

__global__ __launch_bounds__(kCopyBlock) void k_chunk_copy(const uint8_t* __restrict__ buf,
                                                          const uint64_t* __restrict__ offs, uint32_t n,
                                                          const cld_chunk* __restrict__ chunks,
                                                          const uint64_t* __restrict__ co, uint64_t cap,
                                                          const uint64_t* __restrict__ V,
                                                          const uint64_t* __restrict__ pos,
                                                          const uint64_t* __restrict__ hdr, uint8_t* __restrict__ out,
                                                          uint64_t out_cap) {
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t J = (uint32_t)hdr[kHdrJ];
  const int64_t limit = (int64_t)min(pos[J], out_cap);
  const int64_t skew = (int64_t)((uintptr_t)out & 15);    // position -skew is 16-byte aligned
  const int64_t ntiles = (limit + skew + kCopyTile - 1) / kCopyTile;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t w0 = tile * kCopyTile + (tid >> 6) * kCopyWave - skew;      // the wave's positions
    const int64_t wf = max(w0, (int64_t)0), wl = min(w0 + kCopyWave, limit) - 1;
    if (wf > wl) continue;
    const uint32_t v0 = wave_find(pos, 0, J, (uint64_t)wf, lane);
    const uint32_t v1 = pos[v0 + 1] > (uint64_t)wl ? v0 : wave_find(pos, v0, J, (uint64_t)wl, lane);
    uint32_t i0, i1;
    wave_docs(V, n, v0, v1, lane, &i0, &i1);
    Cursor cur{buf, offs, chunks, co, V, pos, cap};
    uint32_t vj = v0;                                     // (the pieces go up: each search starts where the last one began)
#pragma unroll
    for (int k = 0; k < kCopyChunks; ++k) {
      const int64_t c = w0 + k * 1024 + lane * 16, c0 = max(c, (int64_t)0), c1 = min(c + 16, limit);
      if (c0 >= c1) continue;
      vj = lane_find(pos, vj, v1, (uint64_t)c0);
      cur.v = vj;
      cur.i = lane_find(V, i0, i1, vj);
      cur.at = pos[vj];
      cur.end = pos[vj + 1];
      cur.next_doc = V[cur.i + 1];
      cur.load();
      if (c1 - c0 == 16) {                                // the store is aligned, the loads need not be
        uint4 x;
        if ((uint64_t)c0 >= cur.at && cur.end >= (uint64_t)c1) {   // 16 bytes of one piece
          __builtin_memcpy(&x, cur.src + ((uint64_t)c0 - cur.at), 16);
        } else {                                          // of several: put together byte by byte, stored at once
          uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
          for (int b = 0; b < 16; ++b) w[b >> 2] |= cur.byte_at((uint64_t)c0 + b) << (8 * (b & 3));
          x = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *(uint4*)(out + c0) = x;
      } else {                                            // a cut piece: the output's first or last
        for (int64_t p = c0; p < c1; ++p) out[p] = (uint8_t)cur.byte_at((uint64_t)p);
      }
    }
  }
}

__global__ __launch_bounds__(kTile) void k_chunk_offs(uint32_t n, const uint64_t* __restrict__ pos,
                                                     const uint64_t* __restrict__ hdr, uint64_t* __restrict__ out_offs) {
  const uint64_t J = hdr[kHdrJ];
  for (uint64_t i = (uint64_t)blockIdx.x * kTile + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * kTile)
    out_offs[i] = pos[min(out_offs[i], J)];
}

}  // namespace chunks
}  // namespace cld

extern "C" {
hipError_t cld_launch_chunk_totals(const uint64_t* offs, uint32_t n, const cld_chunk* chunks, const uint64_t* chunk_offs,
                                   uint64_t chunk_cap, uint64_t* counts, uint64_t* bytes, void* work, hipStream_t s) {
  using namespace cld::chunks;
  if (n == 0) return hipSuccess;
  const uint32_t range = cld_chunk_doc_range(n), nwg = (n + range - 1) / range;
  uint64_t* hist = (uint64_t*)work;
  hipLaunchKernelGGL(k_chunk_hist, dim3(nwg), dim3(kTile), 0, s, offs, n, range, chunks, chunk_offs, chunk_cap, hist);
  hipLaunchKernelGGL(k_chunk_reduce, dim3((kBins + kReduceWaves - 1) / kReduceWaves), dim3(64 * kReduceWaves), 0, s, hist,
                     nwg, counts, bytes);
  return hipGetLastError();
}

hipError_t cld_launch_chunk_gather(const uint8_t* buf, const uint64_t* offs, uint32_t n, const cld_chunk* chunks,
                                   const uint64_t* chunk_offs, uint64_t chunk_cap, const uint8_t* select, uint32_t flags,
                                   uint8_t* out, uint64_t out_cap, uint64_t* out_offs, void* work, hipStream_t s) {
  using namespace cld::chunks;
  if (n == 0) return hipSuccess;
  static_assert(kChunkWorkFixed >= kHdrWords * sizeof(uint64_t), "the header fits the fixed part");
  uint64_t* hdr = (uint64_t*)work;
  uint64_t* pos = (uint64_t*)((uint8_t*)work + kChunkWorkFixed);
  const uint32_t range = cld_group_range(n);
  hipLaunchKernelGGL(k_chunk_vlen, dim3(kWgs), dim3(kTile), 0, s, chunk_offs, chunk_cap, n, range, out_offs,
                     hdr + kHdrSumsDoc);
  hipLaunchKernelGGL(k_chunk_scan, dim3(kWgs), dim3(kTile), 0, s, (const uint64_t*)nullptr, (uint64_t)n, out_offs,
                     hdr + kHdrSumsDoc);
  hipLaunchKernelGGL(k_chunk_len, dim3(kWgs), dim3(kTile), 0, s, offs, n, chunks, chunk_offs, chunk_cap, select, flags,
                     out_offs, pos, hdr);
  hipLaunchKernelGGL(k_chunk_scan, dim3(kWgs), dim3(kTile), 0, s, hdr + kHdrJ, (uint64_t)UINT32_MAX, pos,
                     hdr + kHdrSumsInst);
  if (out_cap)
    hipLaunchKernelGGL(k_chunk_copy, dim3(kCopyWgs), dim3(kCopyBlock), 0, s, buf, offs, n, chunks, chunk_offs, chunk_cap,
                       out_offs, pos, hdr, out, out_cap);
  hipLaunchKernelGGL(k_chunk_offs, dim3(std::min<uint32_t>(kWgs, n / kTile + 1)), dim3(kTile), 0, s, n, pos, hdr, out_offs);
  return hipGetLastError();
}
}
