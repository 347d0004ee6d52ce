// cld_lines.hip -- a device-resident batch split into lines, zero-copy: a new
// offsets array over the same text (cld_split_lines_device), and the per-line
// results turned into one cld_chunk vector per document
// (cld_lines_to_chunks_device).  The definitions are in cld_mi355x.h.
//
// The text [c0, cN) (every offset clamped to buf_bytes) is cut into tiles of
// kLinesTile bytes at 16-byte aligned addresses, one wave per tile, 16 bytes
// per lane.  A line start is a position of the text where a non-empty document
// begins, or the position after an LF (a "pure" start when no document begins
// there); the final boundary cN is no position of the text.  The rank of a
// start among the kept starts is its line: line_offsets[rank] = position.
//   k_lines_count   per tile: the kept starts, as 16-bit masks per lane from the
//                   bytes (SWAR) and the documents of the lane's bytes (the wave
//                   finds those of its first and last byte, a lane its own
//                   between the two); one word per tile.  A wave takes a run of
//                   consecutive tiles: one wave_find over all of offsets for
//                   the first, then 64 neighbouring offsets probed at once
//   k_lines_tcin    (kLinesWgs ranges of tiles) CLD_LINES_JOIN_BLANK: the carry
//                   into every tile -- has a byte above 0x20 been seen since the
//                   last start? -- from two bits per tile: the tile holds a start,
//                   and a byte above 0x20 follows its last start (or is anywhere
//                   in it, if it has none).  The carry is 1 where the last tile
//                   before with the second bit is not before the last one with
//                   the first: two running maxima.  Only the first start of a
//                   tile depends on the carry, so k_lines_count counts without
//                   it and says whether one more start is kept with it.
//                   Per-range sums of the counts.
//   k_lines_tscan   the exclusive scan of the tile counts; [ntiles] = m
//   k_lines_emit    the tiles again, now with carry and rank: line_offsets,
//                   line_doc, doc_lines of the non-empty documents, and the
//                   longest line (the start before a tile's first one comes
//                   from the nearest tile before that holds one)
//   k_lines_fill    doc_lines of the empty documents (the next non-empty one's,
//                   by a search in offsets), line_offsets[m], the status
// A blank run is never walked backwards, and a page of megabytes fills the
// lanes like a million tweets.  Every launch is complete before the next one
// reads what it wrote (one stream).  No atomic decides a position: the atomics
// are integer maxima (the per-range ones of k_lines_tcin's carry).  Every store is a plain vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cld_kernels.h"
#include "cld_wgscan.h"

namespace cld {
namespace lines {

using wg::block_incl_scan;
using wg::wave_find;

constexpr int kTileBytes = kLinesTile;
constexpr int kBlock = 256;                  // the text kernels: 4 waves, a tile each
constexpr int kBlockWaves = kBlock / 64;
constexpr int kTextWgs = 2048;              // resident at once: 8 workgroups on each of 256 CUs
constexpr int kWgs = kLinesWgs;
constexpr int kScan = kGroupTile;            // the tile-word kernels
constexpr int kScanWaves = kScan / 64;
static_assert(kTileBytes == 64 * 16, "one wave, 16 bytes per lane");
static_assert(kWgs <= kScan, "k_lines_tcin / k_lines_tscan read the ranges at once");

// hdr (the workspace's first kHdrBytes, zeroed per call): the per-range maxima (u32 pairs) and sums; then
// the longest line each wave of k_lines_emit saw (kLinesWaves words, every one written); the tile words
// follow at kLinesWorkFixed.
enum { kHdrAgg = 8, kHdrSums = kHdrAgg + kWgs, kHdrWords = kHdrSums + kWgs };
constexpr size_t kHdrBytes = 8192;
static_assert(kHdrBytes >= kHdrWords * sizeof(uint64_t) && kLinesWorkFixed == kHdrBytes + kLinesWaves * sizeof(uint64_t) &&
                  (size_t)kTextWgs * kBlockWaves <= kLinesWaves, "the fixed part of the workspace");

// A tile's word.  k_lines_count: starts kept without carry [0,11), one more with it [11], the two bits
// [12], [13], the last start kept without carry [14,24) and the tile's first start [24,34), both as
// offsets in the tile.  k_lines_tcin: the kept starts [0,11), the carry [11], [12] and [13] as they were,
// the last kept start [14,24).  k_lines_tscan adds the kept starts before the tile from bit 24 up.
constexpr uint64_t kWCnt = 0x7FF, kWLow = 0xFFFFFF;
constexpr int kWExtra = 11, kWCin = 11, kWHs = 12, kWNa = 13, kWLast = 14, kWFirst = 24, kWRank = 24;

struct Geo {
  uint64_t c0, cN;       // the text
  int64_t a0;            // the first tile's first position, 16-byte aligned as an address
  uint64_t ntiles;
};

__device__ __forceinline__ Geo geo_of(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ offs, uint32_t n,
                                      uint64_t bb) {
  Geo g;
  g.c0 = min(offs[0], bb);
  g.cN = max(min(offs[n], bb), g.c0);
  const uint64_t skew = (uint64_t)((uintptr_t)(buf + g.c0) & 15);
  g.a0 = (int64_t)g.c0 - (int64_t)skew;
  g.ntiles = g.cN > g.c0 ? (g.cN - g.c0 + skew + kTileBytes - 1) / kTileBytes : 0;
  return g;
}

// Tiles per range for nt tiles cut into at most kWgs ranges.
__device__ __forceinline__ uint64_t range_of(uint64_t nt) {
  const uint64_t per = nt / kWgs + (nt % kWgs != 0);
  return per ? per : 1;
}

// Bit b of the result: byte b of w has its top bit set.
__device__ __forceinline__ uint32_t top_bits(uint32_t w) { return (((w >> 7) & 0x01010101u) * 0x01020408u) >> 24 & 0xFu; }
__device__ __forceinline__ uint32_t lf_bits(uint32_t w) {
  const uint32_t x = w ^ 0x0A0A0A0Au;
  return top_bits(~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu));
}
__device__ __forceinline__ uint32_t nonblank_bits(uint32_t w) { return top_bits(((w & 0x7F7F7F7Fu) + 0x5F5F5F5Fu) | w); }

__device__ __forceinline__ uint32_t lane_find(const uint64_t* __restrict__ off, uint32_t lo, uint32_t hi, uint64_t p) {
  uint32_t j = lo, e = hi + 1;               // the largest j in [lo, hi] with off[j] <= p, off[lo] <= p < off[hi + 1]
  while (e - j > 1) {
    const uint32_t mid = j + (e - j) / 2;
    if (off[mid] <= p) j = mid; else e = mid;
  }
  return j;
}

// wave_find for a p that is near: the largest j in [lo, hi) with off[j] <= p, given off[lo] <= p < off[hi]; the
// whole wave probes the 64 entries behind lo at once (four cache lines) and searches on only past those.
__device__ __forceinline__ uint32_t wave_near(const uint64_t* __restrict__ off, uint32_t lo, uint32_t hi, uint64_t p,
                                              int lane) {
  const uint64_t q = (uint64_t)lo + 1 + lane;
  const uint32_t cnt = (uint32_t)__popcll(__ballot(q < hi && off[q] <= p));
  return cnt < 64 ? lo + cnt : wave_find(off, lo + 64, hi, p, lane);
}

// The wave's run of consecutive tiles [*t, *te): the tiles are dealt out in runs, so a wave searches all of
// offsets for its first tile only and goes on from the documents of the tile before.
__device__ __forceinline__ void wave_run(uint64_t ntiles, uint64_t* t, uint64_t* te) {
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6), per = (ntiles + waves - 1) / waves;
  *t = min(ntiles, ((uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * per);
  *te = min(ntiles, *t + per);
}

template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = max(v, (T)__shfl_xor(v, d, 64));
  return v;
}

// Inclusive running maximum over the workgroup (sm: kScanWaves entries); *total: that of the whole workgroup.
__device__ __forceinline__ uint32_t block_incl_max(uint32_t v, uint32_t* sm, uint32_t* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(v, d, 64);
    if (lane >= d) v = max(v, y);
  }
  __syncthreads();
  if (lane == 63) sm[w] = v;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < kScanWaves; ++k) {
    before = max(before, k < w ? sm[k] : 0u);
    all = max(all, sm[k]);
  }
  *total = all;
  return max(v, before);
}

// One lane's 16 positions [p, p + 16) of a tile.
struct LaneLines {
  uint32_t D;            // a document begins here
  uint32_t S;            // every start: D and the positions after an LF
  uint32_t K;            // the kept starts
  uint32_t doc;          // the document of the lane's first position of the text
  uint32_t i1;           // the document of the wave's last one
  bool extra;            // the tile's first start is kept with the carry, and only with it
  uint64_t HS, NA;       // the two bits of every lane (kJoin)
};

// tile_cin: the carry into the tile (k_lines_count: false).  The whole wave; wf <= wl are the tile's first
// and last positions of the text.  *docs: the document of wl of the tile before in the wave's run (negative:
// there is none), replaced by this tile's.
template <bool kJoin>
__device__ __forceinline__ LaneLines lane_lines(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ offs,
                                                uint32_t n, uint64_t bb, const Geo& g, int64_t p, uint64_t wf,
                                                uint64_t wl, int lane, bool tile_cin, int64_t* docs) {
  LaneLines r;
  uint32_t L = 0, N = 0, V = 0;
  if (p >= (int64_t)g.c0 && p + 16 <= (int64_t)g.cN) {
    const uint4 x = *(const uint4*)(buf + p);
    L = lf_bits(x.x) | lf_bits(x.y) << 4 | lf_bits(x.z) << 8 | lf_bits(x.w) << 12;
    N = nonblank_bits(x.x) | nonblank_bits(x.y) << 4 | nonblank_bits(x.z) << 8 | nonblank_bits(x.w) << 12;
    V = 0xFFFFu;
  } else {                                               // the text's first and last lanes
    for (int k = 0; k < 16; ++k) {
      const int64_t q = p + k;
      if (q >= (int64_t)g.c0 && q < (int64_t)g.cN) {
        const uint32_t b = buf[q];
        V |= 1u << k;
        L |= (uint32_t)(b == 0x0A) << k;
        N |= (uint32_t)(b > 0x20) << k;
      }
    }
  }
  // the documents
  const uint32_t i0 = *docs < 0 ? wave_find(offs, 0, n, wf, lane) : wave_near(offs, (uint32_t)*docs, n, wf, lane);
  const uint32_t i1 = offs[i0 + 1] > wl ? i0 : wave_near(offs, i0, n, wl, lane);
  *docs = i1;
  r.i1 = i1;
  r.doc = i0;
  uint32_t D = 0;
  if (V) {
    const uint64_t pf = (uint64_t)(p + __builtin_ctz(V));
    const uint32_t i = i0 == i1 ? i0 : lane_find(offs, i0, i1, pf);
    r.doc = i;
    const int64_t d0 = (int64_t)offs[i] - p;
    if (d0 >= 0 && d0 < 16) D |= 1u << d0;
    for (uint32_t j = i + 1; j <= i1; ++j) {             // (empty documents set the bit of the next non-empty one)
      const int64_t d = (int64_t)min(offs[j], bb) - p;
      if (d >= 16) break;
      if (d >= 0) D |= 1u << d;
    }
    D &= V;
  }
  // the byte before the lane
  uint32_t before = __shfl_up(L >> 15, 1, 64);
  if (lane == 0) before = (V && p > (int64_t)g.c0) ? (uint32_t)(buf[p - 1] == 0x0A) : 0u;
  const uint32_t S = (D | ((L << 1 | before) & 0xFFFFu)) & V;
  r.D = D;
  r.S = S;
  r.extra = false;
  r.HS = r.NA = 0;
  if (!kJoin) {
    r.K = S;
    return r;
  }
  const bool na = S ? (N >> (31 - __builtin_clz(S))) != 0 : N != 0;
  const uint64_t HS = __ballot(S != 0), NA = __ballot(na);
  r.HS = HS;
  r.NA = NA;
  const uint64_t lower = ((uint64_t)1 << lane) - 1, below = HS & lower;
  bool cin, in_wave = true;
  if (below) {
    const int j = 63 - __builtin_clzll(below);
    cin = ((NA & lower) >> j) != 0;
  } else {
    in_wave = (NA & lower) != 0;
    cin = in_wave || tile_cin;
  }
  uint32_t K = D, m = S, done = 0;
  bool first = true;
  while (m) {
    const uint32_t bit = m & (0u - m);
    m ^= bit;
    const bool seg = (N & (bit - 1) & ~done) != 0;       // a byte above 0x20 between the start before and this one
    if (seg || (first && cin)) K |= bit;
    else if (first && !below && !in_wave && !(D & bit)) r.extra = true;
    done = bit - 1;
    first = false;
  }
  r.K = K;
  return r;
}

template <bool kJoin>
__global__ __launch_bounds__(kBlock) void k_lines_count(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ offs,
                                                       uint32_t n, uint64_t bb, uint64_t* __restrict__ hdr,
                                                       uint64_t* __restrict__ words) {
  const int lane = threadIdx.x & 63;
  const Geo g = geo_of(buf, offs, n, bb);
  const uint64_t range = range_of(g.ntiles);
  uint32_t* aggS = (uint32_t*)(hdr + kHdrAgg);
  uint32_t* aggN = aggS + kWgs;
  uint64_t t, te;
  wave_run(g.ntiles, &t, &te);
  int64_t docs = -1;
  uint32_t rg = 0, maxS = 0, maxN = 0;                   // the maxima of the run's tiles in range rg, not yet added
  for (; t < te; ++t) {
    const int64_t w0 = g.a0 + (int64_t)(t * kTileBytes);
    const uint64_t wf = (uint64_t)max(w0, (int64_t)g.c0), wl = min((uint64_t)(w0 + kTileBytes), g.cN) - 1;
    const LaneLines r = lane_lines<kJoin>(buf, offs, n, bb, g, w0 + lane * 16, wf, wl, lane, false, &docs);
    uint32_t cnt = (uint32_t)__popc(r.K);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    const uint64_t HK = __ballot(r.K != 0);
    const int mylast = lane * 16 + (r.K ? 31 - __builtin_clz(r.K) : 0);
    const int myfirst = lane * 16 + (r.S ? __builtin_ctz(r.S) : 0);
    const int last0 = __shfl(mylast, HK ? 63 - __builtin_clzll(HK) : 0, 64);
    uint64_t w = cnt | (uint64_t)last0 << kWLast;
    if (kJoin) {
      const bool hs = r.HS != 0;
      const bool na = hs ? (r.NA >> (63 - __builtin_clzll(r.HS))) != 0 : r.NA != 0;
      const bool extra = __ballot(r.extra) != 0;
      const int first = __shfl(myfirst, hs ? __builtin_ctzll(r.HS) : 0, 64);
      w |= (uint64_t)extra << kWExtra | (uint64_t)hs << kWHs | (uint64_t)na << kWNa | (uint64_t)first << kWFirst;
      const uint32_t code = (uint32_t)t + 2, trg = (uint32_t)(t / range);
      if (trg != rg) {                                   // (uniform)
        if (lane == 0 && maxS) atomicMax(&aggS[rg], maxS);
        if (lane == 0 && maxN) atomicMax(&aggN[rg], maxN);
        rg = trg;
        maxS = maxN = 0;
      }
      if (hs) maxS = code;
      if (na) maxN = code;
    }
    if (lane == 0) words[t] = w;
  }
  if (kJoin && lane == 0) {
    if (maxS) atomicMax(&aggS[rg], maxS);
    if (maxN) atomicMax(&aggN[rg], maxN);
  }
}

__global__ __launch_bounds__(kScan) void k_lines_tcin(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ offs,
                                                     uint32_t n, uint64_t bb, uint32_t join, uint64_t* __restrict__ hdr,
                                                     uint64_t* __restrict__ words) {
  __shared__ uint32_t smm[kScanWaves];
  __shared__ uint64_t sm[kScanWaves];
  const uint32_t tid = threadIdx.x;
  const Geo g = geo_of(buf, offs, n, bb);
  const uint64_t range = range_of(g.ntiles);
  const uint64_t lo = blockIdx.x * range;
  if (lo >= g.ntiles) return;                            // (whole workgroup; its sum stays zero)
  const uint64_t hi = min(g.ntiles, lo + range);
  uint32_t cS = 0, cN = 0;                               // the running maxima over the tiles before the step
  if (join) {
    const uint32_t* aggS = (const uint32_t*)(hdr + kHdrAgg);
    const uint32_t* aggN = aggS + kWgs;
    uint32_t tS, tN;
    block_incl_max(tid < blockIdx.x ? aggS[tid] : 0u, smm, &tS);
    block_incl_max(tid < blockIdx.x ? aggN[tid] : 0u, smm, &tN);
    cN = (tN != 0 && tN >= tS) ? 1u : 0u;                // (code 1: before every tile of the range)
  }
  uint64_t sum = 0;
  for (uint64_t t0 = lo; t0 < hi; t0 += kScan) {
    const uint64_t t = t0 + tid;
    const uint64_t w = t < hi ? words[t] : 0;
    bool cin = false;
    if (join) {                                          // (uniform)
      // thread tid brings the bits of the tile before its own, so the inclusive maxima end before tile t;
      // bits 12 and 13 of a word stay where they are when it is rewritten below
      uint32_t s = tid == 0 ? cS : 0u, nn = tid == 0 ? cN : 0u;
      if (t > lo && t <= hi) {
        const uint64_t wp = words[t - 1];
        if (wp >> kWHs & 1) s = max(s, (uint32_t)(t - 1) + 2);
        if (wp >> kWNa & 1) nn = max(nn, (uint32_t)(t - 1) + 2);
      }
      const uint32_t iS = block_incl_max(s, smm, &cS);
      const uint32_t iN = block_incl_max(nn, smm, &cN);
      cin = iN != 0 && iN >= iS;
      __syncthreads();                                   // (every words[t - 1] has been read)
    }
    if (t < hi) {
      const uint32_t cnt = (uint32_t)(w & kWCnt), extra = (uint32_t)(w >> kWExtra & 1);
      const uint32_t c = cnt + (cin ? extra : 0u);
      const uint64_t last = cnt ? (w >> kWLast & 0x3FF) : (w >> kWFirst & 0x3FF);
      words[t] = c | (uint64_t)cin << kWCin | (w & ((uint64_t)3 << kWHs)) | last << kWLast;
      sum += c;
    }
    __syncthreads();                                     // (the next step reads the word of this step's last tile)
  }
  const uint64_t inc = block_incl_scan<uint64_t, kScanWaves>(sum, sm);
  if (tid == kScan - 1) hdr[kHdrSums + blockIdx.x] = inc;
}

__global__ __launch_bounds__(kScan) void k_lines_tscan(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ offs,
                                                      uint32_t n, uint64_t bb, const uint64_t* __restrict__ hdr,
                                                      uint64_t* __restrict__ words) {
  __shared__ uint64_t sm[kScanWaves];
  __shared__ uint64_t carry;
  const uint32_t tid = threadIdx.x;
  const Geo g = geo_of(buf, offs, n, bb);
  const uint64_t range = range_of(g.ntiles);
  const uint64_t lo = blockIdx.x * range;
  if (blockIdx.x > 0 && lo >= g.ntiles) return;          // (whole workgroup; the range of workgroup 0 always counts)
  {
    const uint64_t inc = block_incl_scan<uint64_t, kScanWaves>(tid < blockIdx.x ? hdr[kHdrSums + tid] : 0, sm);
    if (tid == kScan - 1) carry = inc;
  }
  __syncthreads();
  const uint64_t hi = min(g.ntiles, lo + range);
  for (uint64_t t0 = lo; t0 < hi; t0 += kScan) {
    const uint64_t t = t0 + tid;
    const uint64_t w = t < hi ? words[t] : 0;
    const uint64_t v = w & kWCnt;
    const uint64_t inc = block_incl_scan<uint64_t, kScanWaves>(v, sm);
    const uint64_t c = carry;
    __syncthreads();
    if (t < hi) words[t] = (c + inc - v) << kWRank | (w & kWLow);
    if (tid == kScan - 1) carry = c + inc;
    __syncthreads();
  }
  if (hi == g.ntiles && tid == 0) words[g.ntiles] = carry << kWRank;
}

template <bool kJoin>
__global__ __launch_bounds__(kBlock) void k_lines_emit(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ offs,
                                                      uint32_t n, uint64_t bb, uint64_t* __restrict__ line_offsets,
                                                      uint32_t* __restrict__ line_doc, uint64_t cap,
                                                      uint64_t* __restrict__ doc_lines, uint64_t* __restrict__ wmax,
                                                      const uint64_t* __restrict__ words) {
  const int lane = threadIdx.x & 63;
  uint64_t run_longest = 0;
  const Geo g = geo_of(buf, offs, n, bb);
  uint64_t t, te;
  wave_run(g.ntiles, &t, &te);
  int64_t docs = -1;
  for (; t < te; ++t) {
    const int64_t w0 = g.a0 + (int64_t)(t * kTileBytes);
    const uint64_t wf = (uint64_t)max(w0, (int64_t)g.c0), wl = min((uint64_t)(w0 + kTileBytes), g.cN) - 1;
    const uint64_t word = words[t];
    const int64_t p = w0 + lane * 16;
    const LaneLines r = lane_lines<kJoin>(buf, offs, n, bb, g, p, wf, wl, lane, (word >> kWCin & 1) != 0, &docs);
    const uint32_t cnt = (uint32_t)__popc(r.K);
    uint32_t inc = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(inc, d, 64);
      if (lane >= d) inc += y;
    }
    uint64_t rank = (word >> kWRank) + inc - cnt;
    const uint64_t HK = __ballot(r.K != 0);
    const bool last_tile = t + 1 == g.ntiles;
    // the kept start before the tile's first one: in the nearest tile before that holds one
    int64_t tile_prev = 0;
    if (t > 0 && (HK != 0 || last_tile)) {               // (uniform)
      uint64_t s = t - 1, ws = words[s];
      if ((ws & kWCnt) == 0) {
        const uint64_t pt = word >> kWRank;              // > 0: the text's first byte begins a document, in tile 0
        uint64_t a = 0, b = t;                           // the largest a with fewer kept starts before it
        while (b - a > 1) {
          const uint64_t mid = a + (b - a) / 2;
          if ((words[mid] >> kWRank) < pt) a = mid; else b = mid;
        }
        s = a;
        ws = words[s];
      }
      tile_prev = g.a0 + (int64_t)(s * kTileBytes) + (int64_t)(ws >> kWLast & 0x3FF);
    }
    const int mylast = lane * 16 + (r.K ? 31 - __builtin_clz(r.K) : 0);
    const uint64_t belowK = HK & (((uint64_t)1 << lane) - 1);
    const int from = __shfl(mylast, belowK ? 63 - __builtin_clzll(belowK) : 0, 64);
    const int tile_last = __shfl(mylast, HK ? 63 - __builtin_clzll(HK) : 0, 64);
    int64_t prev = belowK ? w0 + from : tile_prev;
    bool has_prev = belowK != 0 || t > 0;
    uint64_t longest = 0;
    uint32_t doc = r.doc, m = r.K;
    while (m) {
      const uint32_t bit = m & (0u - m);
      m ^= bit;
      const int64_t s = p + __builtin_ctz(bit);
      if (has_prev && s > prev) longest = max(longest, (uint64_t)(s - prev));
      prev = s;
      has_prev = true;
      while (doc < r.i1 && min(offs[doc + 1], bb) <= (uint64_t)s) ++doc;
      if (line_offsets && rank <= cap) line_offsets[rank] = (uint64_t)s;
      if (line_doc && rank < cap) line_doc[rank] = doc;
      if (r.D & bit) doc_lines[doc] = rank;
      ++rank;
    }
    if (last_tile && lane == 0) {                        // the last line ends at cN
      const int64_t last = HK ? w0 + tile_last : tile_prev;
      if ((HK != 0 || t > 0) && (int64_t)g.cN > last) longest = max(longest, (uint64_t)((int64_t)g.cN - last));
    }
    run_longest = max(run_longest, longest);
  }
  run_longest = wave_max(run_longest);                   // (one slot per wave: no atomics of every wave on one address)
  if (lane == 0) wmax[blockIdx.x * kBlockWaves + (threadIdx.x >> 6)] = run_longest;
}

__global__ __launch_bounds__(kScan) void k_lines_fill(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ offs,
                                                     uint32_t n, uint64_t bb, uint64_t* __restrict__ line_offsets,
                                                     uint64_t cap, uint64_t* __restrict__ doc_lines,
                                                     cld_lines_status* __restrict__ status,
                                                     const uint64_t* __restrict__ wmax, uint32_t nwaves,
                                                     const uint64_t* __restrict__ words) {
  __shared__ uint64_t sm[kScanWaves];
  const Geo g = geo_of(buf, offs, n, bb);
  const uint64_t m = words[g.ntiles] >> kWRank;
  for (uint64_t i = (uint64_t)blockIdx.x * kScan + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * kScan) {
    const uint64_t c = min(offs[i], bb);
    if (i < n && min(offs[i + 1], bb) > c && c >= g.c0 && c < g.cN) continue;   // not empty: k_lines_emit wrote it
    uint64_t v = m;
    if (c >= g.c0 && c < g.cN) {                         // the document that begins here: the last one at or before c
      const uint32_t j = lane_find(offs, (uint32_t)i, n - 1, c);
      if (j != i) v = doc_lines[j];
    }
    doc_lines[i] = v;
  }
  if (blockIdx.x != 0) return;
  if (threadIdx.x == 0 && line_offsets && m <= cap) line_offsets[m] = g.cN;
  if (!status) return;
  uint64_t longest = 0;
  for (uint32_t k = threadIdx.x; k < nwaves; k += kScan) longest = max(longest, wmax[k]);
  longest = wave_max(longest);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = longest;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kScanWaves; ++k) longest = max(longest, sm[k]);
    status->total_lines = m;
    status->max_line_bytes = longest;
  }
}

__global__ __launch_bounds__(kBlock) void k_lines_chunks(const cld_result* __restrict__ res,
                                                        const uint64_t* __restrict__ line_offsets,
                                                        const uint32_t* __restrict__ line_doc, uint64_t cap,
                                                        const uint64_t* __restrict__ offs, uint32_t n,
                                                        const uint64_t* __restrict__ doc_lines, uint32_t gflags,
                                                        cld_chunk* __restrict__ chunks) {
  const uint64_t m = min(doc_lines[n], cap);
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kBlock) {
    uint32_t key = (gflags & CLD_GROUP_TOP1) ? res[j].lang3[0] : res[j].summary_lang;
    if ((gflags & CLD_GROUP_RELIABLE_ONLY) && res[j].is_reliable == 0) key = 26;   // UNKNOWN_LANGUAGE
    const uint32_t i = line_doc[j];
    cld_chunk c;
    c.offset = 0;
    c.bytes = 0;
    c.lang1 = (uint16_t)key;
    c.pad = 0;
    if (i < n) {
      const uint64_t a = line_offsets[j], b = line_offsets[j + 1], o = offs[i];
      c.offset = (int32_t)min(a > o ? a - o : (uint64_t)0, (uint64_t)INT32_MAX);
      c.bytes = (int32_t)min(b > a ? b - a : (uint64_t)0, (uint64_t)INT32_MAX);
    }
    chunks[j] = c;
  }
}

}  // namespace lines
}  // namespace cld

extern "C" {
hipError_t cld_launch_split_lines(const uint8_t* buf, const uint64_t* offs, uint32_t n, uint64_t buf_bytes, uint32_t flags,
                                  uint64_t* line_offsets, uint32_t* line_doc, uint64_t line_cap, uint64_t* doc_lines,
                                  cld_lines_status* status, void* work, uint32_t max_wgs, hipStream_t s) {
  using namespace cld::lines;
  if (n == 0) return hipSuccess;
  uint64_t* hdr = (uint64_t*)work;
  uint64_t* wmax = (uint64_t*)((uint8_t*)work + kHdrBytes);
  uint64_t* words = (uint64_t*)((uint8_t*)work + kLinesWorkFixed);
  const bool join = (flags & CLD_LINES_JOIN_BLANK) != 0;
  const uint64_t tiles = buf_bytes / kTileBytes + 2;
  const uint32_t wgs = max_wgs ? std::min<uint32_t>(max_wgs, kTextWgs) : (uint32_t)kTextWgs;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((tiles + kBlockWaves - 1) / kBlockWaves, wgs);
  hipError_t e = hipMemsetAsync(hdr, 0, kHdrBytes, s);
  if (e != hipSuccess) return e;
  if (join)
    hipLaunchKernelGGL(k_lines_count<true>, dim3(grid), dim3(kBlock), 0, s, buf, offs, n, buf_bytes, hdr, words);
  else
    hipLaunchKernelGGL(k_lines_count<false>, dim3(grid), dim3(kBlock), 0, s, buf, offs, n, buf_bytes, hdr, words);
  hipLaunchKernelGGL(k_lines_tcin, dim3(kWgs), dim3(kScan), 0, s, buf, offs, n, buf_bytes, (uint32_t)join, hdr, words);
  hipLaunchKernelGGL(k_lines_tscan, dim3(kWgs), dim3(kScan), 0, s, buf, offs, n, buf_bytes, hdr, words);
  if (join)
    hipLaunchKernelGGL(k_lines_emit<true>, dim3(grid), dim3(kBlock), 0, s, buf, offs, n, buf_bytes, line_offsets, line_doc,
                       line_cap, doc_lines, wmax, words);
  else
    hipLaunchKernelGGL(k_lines_emit<false>, dim3(grid), dim3(kBlock), 0, s, buf, offs, n, buf_bytes, line_offsets,
                       line_doc, line_cap, doc_lines, wmax, words);
  hipLaunchKernelGGL(k_lines_fill, dim3(std::min<uint32_t>(kWgs, n / kScan + 1)), dim3(kScan), 0, s, buf, offs, n,
                     buf_bytes, line_offsets, line_cap, doc_lines, status, wmax, grid * kBlockWaves, words);
  return hipGetLastError();
}

hipError_t cld_launch_lines_to_chunks(const cld_result* res, const uint64_t* line_offsets, const uint32_t* line_doc,
                                      uint64_t line_cap, const uint64_t* offs, uint32_t n, const uint64_t* doc_lines,
                                      uint32_t group_flags, cld_chunk* chunks, hipStream_t s) {
  using namespace cld::lines;
  if (line_cap == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((line_cap + kBlock - 1) / kBlock, kTextWgs);
  hipLaunchKernelGGL(k_lines_chunks, dim3(grid), dim3(kBlock), 0, s, res, line_offsets, line_doc, line_cap, offs, n,
                     doc_lines, group_flags, chunks);
  return hipGetLastError();
}
}
