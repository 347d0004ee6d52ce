// cld_valid.hip -- the reference's checked entry points on the GPU.
//
// DetectLanguageCheckUTF8 (compact_lang_det.cc:44-56) and
// ExtDetectLanguageSummaryCheckUTF8 (compact_lang_det.cc:317-355) first run
// SpanInterchangeValid (compact_lang_det_impl.cc:72-80) over the buffer and
// score it only when the whole of it is interchange-valid UTF-8.  The state
// table behind it reduces to a closed form in which a byte's verdict depends
// on bytes p-3 .. p+3 of its own document (cld_valid_rule.h), so the check is
// byte-local and tiles freely.
//
// k_valid        one wave per document.  Documents of at most kShortMax bytes
//                are checked here, one byte per lane and one ballot per 64
//                bytes, stopping at the first step with an error; a longer
//                document only gets its prefix preset to its length.
// k_valid_tiles  the longer documents.  The batch's text is cut into tiles of
//                kTile bytes at kTile-aligned addresses; one wave takes one
//                tile at a time (a run of consecutive tiles per wave of a
//                persistent grid): 16 aligned bytes per lane in one load, the neighbour
//                lanes' edge dwords by cross-lane moves, the 4 bytes either
//                side of the tile by two dword loads.  Bytes outside the
//                document in hand are masked to 0, so nothing is read across
//                a document end.  The first error of a tile goes into
//                valid_prefix[d] with atomicMin; a tile that starts at or
//                past the current minimum skips its work.  Lanes whose 24-byte
//                window is all ASCII test their 16 bytes four at a time.
// k_valid_lens / k_valid_copy / k_valid_fixup: CLD_FLAG_CHECK_UTF8 -- the
//                prepared batch in which a rejected document has length 0 (so
//                no scoring kernel sees its bytes), and the fixed "rejected"
//                result of the reference written over that document's result.
// k_scrub / k_scrub_tiles: CLD_FLAG_SCRUB_UTF8 and cld_scrub_utf8_* -- the
//                same two shapes, with every byte at an error position
//                replaced by 0x20 in a copy that keeps the source's offsets
//                (no length kernel, no scan, nothing rejected).  Overwriting
//                an error position with a space changes no other byte's
//                verdict (a space covers nothing and completes no sequence),
//                so one pass equals the reference's "replace the byte at the
//                valid prefix, check again" loop run to its end.  k_scrub
//                writes the documents of at most kShortMax bytes; the tile
//                kernel writes the bytes of the longer ones: a lane merges the
//                error masks of every long document its 16 bytes touch and
//                stores them once (byte stores where some of the 16 bytes
//                belong to a short document or lie outside the batch).  The
//                replaced bytes are counted per document (one atomic per
//                wave, tile and document that has any), the first of them
//                goes into valid_prefix[d] with atomicMin.
// No LDS, no scratch.  Algorithmic bytes: the text is read once by the check;
// the prepared copy reads and writes the valid documents once more.  The scrub
// pass reads each input byte once (plus 8 edge bytes per 1 KB tile, and the
// 6 neighbour bytes per lane of a short document from cache) and writes each
// output byte once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cld_kernels.h"
#include "cld_valid_rule.h"

namespace cld {
namespace valid {

constexpr int kWPB = 4;            // waves per workgroup
constexpr int kShortMax = kValidShortMax;   // longest document of the one-wave shape
constexpr int kTile = kValidTile;           // 64 lanes x 16 bytes
constexpr int kTileBlocks = 2048;  // persistent grid of the tile kernels: 256 CUs x 8 workgroups

__device__ __forceinline__ uint32_t ldz(const uint8_t* p, int64_t i, int64_t n) {
  return (i >= 0 && i < n) ? (uint32_t)p[i] : 0u;        // outside the document: 0
}

__device__ __forceinline__ int32_t clamp_len(uint64_t len) {
  return (int32_t)(len < 0x7FFFFFFFull ? len : 0x7FFFFFFFull);
}

__global__ __launch_bounds__(64 * kWPB) void k_valid(const uint8_t* __restrict__ buf,
                                                     const uint64_t* __restrict__ offs, int n,
                                                     int32_t* __restrict__ vp) {
  const int d = blockIdx.x * kWPB + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (d >= n) return;
  const uint64_t a = offs[d], b = offs[d + 1];
  const int64_t len = (int64_t)(b - a);
  if (len > kShortMax) {           // k_valid_tiles takes it from here
    if (lane == 0) vp[d] = clamp_len((uint64_t)len);
    return;
  }
  const uint8_t* p = buf + a;
  int32_t res = (int32_t)len;
  for (int64_t base = 0; base < len; base += 64) {
    const int64_t i = base + lane;
    const uint32_t m3 = ldz(p, i - 3, len), m2 = ldz(p, i - 2, len), m1 = ldz(p, i - 1, len), c = ldz(p, i, len);
    const uint32_t p1 = ldz(p, i + 1, len), p2 = ldz(p, i + 2, len), p3 = ldz(p, i + 3, len);
    const bool err = i < len && is_error(c, char_len(c, p1, p2, p3), char_len(m1, c, p1, p2),
                                         char_len(m2, m1, c, p1), char_len(m3, m2, m1, c));
    const uint64_t e = __ballot(err);
    if (e) {
      res = (int32_t)base + __ffsll((long long)e) - 1;
      break;
    }
  }
  if (lane == 0) vp[d] = res;
}

// Mask of the bytes of the dword at address s that lie in [a, b).
__device__ __forceinline__ uint32_t keep(int64_t s, int64_t a, int64_t b) {
  int64_t lo = a - s, hi = b - s;
  lo = lo < 0 ? 0 : lo > 4 ? 4 : lo;
  hi = hi < 0 ? 0 : hi > 4 ? 4 : hi;
  const uint32_t below_lo = lo >= 4 ? 0xFFFFFFFFu : (1u << (8 * (int)lo)) - 1u;
  const uint32_t below_hi = hi >= 4 ? 0xFFFFFFFFu : (1u << (8 * (int)hi)) - 1u;
  return below_hi & ~below_lo;
}

// Bit 7 of each byte of x (all bytes below 0x80) that is no interchange-valid
// ASCII: below 0x20 and none of TAB LF FF CR, or 0x7F.
__device__ __forceinline__ uint32_t ascii_bad(uint32_t x) {
  const uint32_t h = 0x80808080u;
  auto eq = [&](uint32_t v) { return ~((x ^ (v * 0x01010101u)) + 0x7F7F7F7Fu) & h; };   // byte == v
  const uint32_t lt20 = ~(x + 0x60606060u) & h;
  const uint32_t is7f = (x + 0x01010101u) & h;
  return (lt20 & ~(eq(0x09) | eq(0x0A) | eq(0x0C) | eq(0x0D))) | is7f;
}

// The four flag bits (7, 15, 23, 31) of f as bits 0-3.
__device__ __forceinline__ uint32_t flags4(uint32_t f) {
  return ((f >> 7) & 1u) | ((f >> 14) & 2u) | ((f >> 21) & 4u) | ((f >> 28) & 8u);
}

// First document of [0, n) that ends after offset x (x < offs[n]).
__device__ __forceinline__ int first_doc_after(const uint64_t* __restrict__ offs, int n, uint64_t x) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (offs[mid + 1] > x) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// Error bits of one lane's 16 bytes at address q0 (bit j: byte q0 + j), from
// the window w: the six dwords at q0 - 4 .. q0 + 20 with every byte outside the
// document already 0.
__device__ __forceinline__ uint32_t lane_errors(const uint32_t (&w)[6]) {
  if (((w[0] | w[1] | w[2] | w[3] | w[4] | w[5]) & 0x80808080u) == 0) {   // ASCII around: no sequences to follow
    const uint32_t f0 = ascii_bad(w[1]), f1 = ascii_bad(w[2]), f2 = ascii_bad(w[3]), f3 = ascii_bad(w[4]);
    if ((f0 | f1 | f2 | f3) == 0) return 0;
    return flags4(f0) | (flags4(f1) << 4) | (flags4(f2) << 8) | (flags4(f3) << 12);
  }
  uint32_t B[22];                  // bytes q0 - 3 .. q0 + 18
#pragma unroll
  for (int k = 0; k < 22; ++k) B[k] = (w[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xFFu;
  uint32_t L[19];                  // char_len at q0 - 3 .. q0 + 15
#pragma unroll
  for (int k = 0; k < 19; ++k) L[k] = char_len(B[k], B[k + 1], B[k + 2], B[k + 3]);
  uint32_t e = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) e |= (is_error(B[j + 3], L[j + 3], L[j + 2], L[j + 1], L[j]) ? 1u : 0u) << j;
  return e;
}

__global__ __launch_bounds__(64 * kWPB) void k_valid_tiles(const uint8_t* __restrict__ buf,
                                                           const uint64_t* __restrict__ offs, int n,
                                                           int32_t* __restrict__ vp) {
  if (n <= 0) return;
  const int lane = threadIdx.x & 63;
  const int64_t A0 = (int64_t)(uintptr_t)buf;
  const int64_t ga = A0 + (int64_t)offs[0], gb = A0 + (int64_t)offs[n];   // the batch's text, as addresses
  if (gb <= ga) return;
  const int64_t tile0 = ga & ~(int64_t)(kTile - 1);
  const int64_t ntiles = (gb - tile0 + kTile - 1) / kTile;
  const int64_t wave = (int64_t)blockIdx.x * kWPB + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * kWPB;
  // each wave takes a run of consecutive tiles: the document index then carries from tile to tile
  // (a binary search per tile was a chain of ~17 dependent loads, longer than the tile's own work),
  // and once a wave has found an error in a document it skips that document's later tiles
  const int64_t per = (ntiles + nwaves - 1) / nwaves;
  const int64_t t0 = wave * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
  int dnext = -1;                  // first document that ends after the next tile's start, if known
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t T = tile0 + t * kTile, TE = T + kTile;
    const int64_t q0 = T + 16 * lane;
    bool loaded = false;
    uint32_t w[6] = {0, 0, 0, 0, 0, 0};
    const int d0 = dnext >= 0 ? dnext : first_doc_after(offs, n, (uint64_t)((T > ga ? T : ga) - A0));
    dnext = -1;
    for (int db = d0; db < n; db += 64) {
      const int dl = db + lane;
      const uint64_t oa = dl < n ? offs[dl] : 0, ob = dl < n ? offs[dl + 1] : 0;
      const bool in = dl < n && A0 + (int64_t)oa < TE;
      if (dnext < 0) {
        const uint64_t nx = __ballot(dl < n && A0 + (int64_t)ob > TE);
        if (nx) dnext = db + __ffsll((long long)nx) - 1;
      }
      uint64_t m = __ballot(in && ob - oa > (uint64_t)kShortMax);
      while (m) {
        const int j = __ffsll((long long)m) - 1, d = db + j;
        m &= m - 1;
        const int64_t a = A0 + (int64_t)__shfl(oa, j, 64), b = A0 + (int64_t)__shfl(ob, j, 64);
        const int64_t lo = T > a ? T : a;                 // this tile's part of the document: [lo, hi)
        const int64_t hi = TE < b ? TE : b;
        if (hi <= lo) continue;
        uint4 v = make_uint4(0, 0, 0, 0);
        uint32_t edge = 0;
        if (!loaded) {
          // aligned loads that hold at least one byte of the batch: they cannot leave its pages.
          // Issued before the prefix is read, so the two round trips overlap.
          if (q0 + 16 > ga && q0 < gb) v = *reinterpret_cast<const uint4*>(buf + (q0 - A0));
          if (lane == 0 && T > ga) edge = *reinterpret_cast<const uint32_t*>(buf + (T - 4 - A0));
          if (lane == 63 && TE < gb) edge = *reinterpret_cast<const uint32_t*>(buf + (TE - A0));
        }
        const int32_t cur = __builtin_amdgcn_readfirstlane(__atomic_load_n(&vp[d], __ATOMIC_RELAXED));
        if (!loaded) {
          uint32_t prev = __shfl_up(v.w, 1, 64), next = __shfl_down(v.x, 1, 64);
          if (lane == 0) prev = edge;
          if (lane == 63) next = edge;
          w[0] = prev; w[1] = v.x; w[2] = v.y; w[3] = v.z; w[4] = v.w; w[5] = next;
          loaded = true;
        }
        // (another tile has already found an error before this one's first byte)
        if (lo - a >= (int64_t)cur) continue;
        uint32_t x[6];
        if (a <= T - 4 && b >= TE + 4) {                  // the document covers every window of the tile
#pragma unroll
          for (int k = 0; k < 6; ++k) x[k] = w[k];
        } else {
#pragma unroll
          for (int k = 0; k < 6; ++k) x[k] = w[k] & keep(q0 - 4 + 4 * k, a, b);
        }
        uint32_t e = lane_errors(x);
        // only this lane's bytes inside the document count (a masked byte reads as NUL)
        int64_t jl = a - q0, jh = b - q0;
        jl = jl < 0 ? 0 : jl > 16 ? 16 : jl;
        jh = jh < 0 ? 0 : jh > 16 ? 16 : jh;
        e &= ((1u << (int)jh) - 1u) & ~((1u << (int)jl) - 1u);
        const uint64_t any = __ballot(e != 0);
        if (any) {
          const int fl = __ffsll((long long)any) - 1;
          const int jb = __shfl(__ffs((int)e) - 1, fl, 64);
          if (lane == 0) atomicMin(&vp[d], (int32_t)(T + 16 * fl + jb - a));
        }
      }
      if (__ballot(in) != ~0ull) break;                   // the tile ends inside these 64 documents
    }
  }
}

// 0xFF in every byte of the dword whose bit (0-3) of m is set.
__device__ __forceinline__ uint32_t spread4(uint32_t m) {
  return (((m & 0xFu) * 0x00204081u) & 0x01010101u) * 0xFFu;
}

// The short shape of the scrub: one wave per document of at most kShortMax
// bytes writes its scrubbed copy, its replaced count and its valid prefix.  A
// longer document only gets its count zeroed and its prefix preset to its
// length (k_scrub_tiles adds to / lowers them).  replaced, vp: nullable.
__global__ __launch_bounds__(64 * kWPB) void k_scrub(const uint8_t* __restrict__ buf,
                                                     const uint64_t* __restrict__ offs, int n,
                                                     uint8_t* __restrict__ out, int32_t* __restrict__ replaced,
                                                     int32_t* __restrict__ vp) {
  const int d = blockIdx.x * kWPB + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (d >= n) return;
  const uint64_t a = offs[d], b = offs[d + 1];
  const int64_t len = (int64_t)(b - a);
  if (len > kShortMax) {
    if (lane == 0) {
      if (vp) vp[d] = clamp_len((uint64_t)len);
      if (replaced) replaced[d] = 0;
    }
    return;
  }
  const uint8_t* p = buf + a;
  int32_t first = (int32_t)len, cnt = 0;
  for (int64_t base = 0; base < len; base += 64) {
    const int64_t i = base + lane;
    const uint32_t m3 = ldz(p, i - 3, len), m2 = ldz(p, i - 2, len), m1 = ldz(p, i - 1, len), c = ldz(p, i, len);
    const uint32_t p1 = ldz(p, i + 1, len), p2 = ldz(p, i + 2, len), p3 = ldz(p, i + 3, len);
    const bool err = i < len && is_error(c, char_len(c, p1, p2, p3), char_len(m1, c, p1, p2),
                                         char_len(m2, m1, c, p1), char_len(m3, m2, m1, c));
    if (i < len) out[a + i] = err ? (uint8_t)0x20 : (uint8_t)c;
    const uint64_t e = __ballot(err);
    if (e) {
      if (cnt == 0) first = (int32_t)base + __ffsll((long long)e) - 1;
      cnt += __popcll(e);
    }
  }
  if (lane == 0) {
    if (vp) vp[d] = first;
    if (replaced) replaced[d] = cnt;
  }
}

// The tile shape of the scrub: tiles, lanes, loads and windows as in
// k_valid_tiles, but every long document of a tile is looked at whatever its
// prefix already says.  wide: out - buf is a multiple of 16, so a lane's 16
// bytes go out in one aligned store; else they go byte by byte.
__global__ __launch_bounds__(64 * kWPB) void k_scrub_tiles(const uint8_t* __restrict__ buf,
                                                           const uint64_t* __restrict__ offs, int n,
                                                           uint8_t* __restrict__ out, int32_t* __restrict__ replaced,
                                                           int32_t* __restrict__ vp) {
  if (n <= 0) return;
  const int lane = threadIdx.x & 63;
  const int64_t A0 = (int64_t)(uintptr_t)buf;
  const bool wide = (((int64_t)(uintptr_t)out - A0) & 15) == 0;
  const int64_t ga = A0 + (int64_t)offs[0], gb = A0 + (int64_t)offs[n];   // the batch's text, as addresses
  if (gb <= ga) return;
  const int64_t tile0 = ga & ~(int64_t)(kTile - 1);
  const int64_t ntiles = (gb - tile0 + kTile - 1) / kTile;
  const int64_t wave = (int64_t)blockIdx.x * kWPB + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * kWPB;
  const int64_t per = (ntiles + nwaves - 1) / nwaves;   // a run of consecutive tiles per wave (k_valid_tiles)
  const int64_t t0 = wave * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
  int dnext = -1;                  // first document that ends after the next tile's start, if known
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t T = tile0 + t * kTile, TE = T + kTile;
    const int64_t q0 = T + 16 * lane;
    bool loaded = false;
    uint32_t w[6] = {0, 0, 0, 0, 0, 0};
    uint32_t errs = 0, cover = 0;  // of this lane's 16 bytes: error positions; bytes inside a long document
    const int d0 = dnext >= 0 ? dnext : first_doc_after(offs, n, (uint64_t)((T > ga ? T : ga) - A0));
    dnext = -1;
    for (int db = d0; db < n; db += 64) {
      const int dl = db + lane;
      const uint64_t oa = dl < n ? offs[dl] : 0, ob = dl < n ? offs[dl + 1] : 0;
      const bool in = dl < n && A0 + (int64_t)oa < TE;
      if (dnext < 0) {
        const uint64_t nx = __ballot(dl < n && A0 + (int64_t)ob > TE);
        if (nx) dnext = db + __ffsll((long long)nx) - 1;
      }
      uint64_t m = __ballot(in && ob - oa > (uint64_t)kShortMax);
      while (m) {
        const int j = __ffsll((long long)m) - 1, d = db + j;
        m &= m - 1;
        const int64_t a = A0 + (int64_t)__shfl(oa, j, 64), b = A0 + (int64_t)__shfl(ob, j, 64);
        const int64_t lo = T > a ? T : a;                 // this tile's part of the document: [lo, hi)
        const int64_t hi = TE < b ? TE : b;
        if (hi <= lo) continue;
        if (!loaded) {
          // aligned loads that hold at least one byte of the batch: they cannot leave its pages
          uint4 v = make_uint4(0, 0, 0, 0);
          uint32_t edge = 0;
          if (q0 + 16 > ga && q0 < gb) v = *reinterpret_cast<const uint4*>(buf + (q0 - A0));
          if (lane == 0 && T > ga) edge = *reinterpret_cast<const uint32_t*>(buf + (T - 4 - A0));
          if (lane == 63 && TE < gb) edge = *reinterpret_cast<const uint32_t*>(buf + (TE - A0));
          uint32_t prev = __shfl_up(v.w, 1, 64), next = __shfl_down(v.x, 1, 64);
          if (lane == 0) prev = edge;
          if (lane == 63) next = edge;
          w[0] = prev; w[1] = v.x; w[2] = v.y; w[3] = v.z; w[4] = v.w; w[5] = next;
          loaded = true;
        }
        uint32_t x[6];
        if (a <= T - 4 && b >= TE + 4) {                  // the document covers every window of the tile
#pragma unroll
          for (int k = 0; k < 6; ++k) x[k] = w[k];
        } else {
#pragma unroll
          for (int k = 0; k < 6; ++k) x[k] = w[k] & keep(q0 - 4 + 4 * k, a, b);
        }
        uint32_t e = lane_errors(x);
        // only this lane's bytes inside the document count (a masked byte reads as NUL)
        int64_t jl = a - q0, jh = b - q0;
        jl = jl < 0 ? 0 : jl > 16 ? 16 : jl;
        jh = jh < 0 ? 0 : jh > 16 ? 16 : jh;
        const uint32_t mine = ((1u << (int)jh) - 1u) & ~((1u << (int)jl) - 1u);
        e &= mine;
        errs |= e;
        cover |= mine;
        const uint64_t any = __ballot(e != 0);
        if (any) {
          if (replaced) {
            int32_t c = __popc(e);
#pragma unroll
            for (int k = 32; k > 0; k >>= 1) c += __shfl_xor(c, k, 64);
            if (lane == 0) atomicAdd(&replaced[d], c);
          }
          if (vp) {
            const int fl = __ffsll((long long)any) - 1;
            const int jb = __shfl(__ffs((int)e) - 1, fl, 64);
            if (lane == 0) atomicMin(&vp[d], (int32_t)(T + 16 * fl + jb - a));
          }
        }
      }
      if (__ballot(in) != ~0ull) break;                   // the tile ends inside these 64 documents
    }
    if (!cover) continue;                                 // (also: no long document in this tile, nothing loaded)
    uint8_t* o = out + (q0 - A0);
    if (wide && cover == 0xFFFFu) {                       // 16 bytes of long documents, all inside the batch
      uint4 v;
      const uint32_t b0 = spread4(errs), b1 = spread4(errs >> 4), b2 = spread4(errs >> 8), b3 = spread4(errs >> 12);
      v.x = (w[1] & ~b0) | (0x20202020u & b0);
      v.y = (w[2] & ~b1) | (0x20202020u & b1);
      v.z = (w[3] & ~b2) | (0x20202020u & b2);
      v.w = (w[4] & ~b3) | (0x20202020u & b3);
      *reinterpret_cast<uint4*>(o) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if ((cover >> k) & 1u) o[k] = ((errs >> k) & 1u) ? (uint8_t)0x20 : (uint8_t)(w[1 + (k >> 2)] >> (8 * (k & 3)));
    }
  }
}

// Prepared length per document: its own when the check passed, else 0.
__global__ __launch_bounds__(256) void k_valid_lens(const uint64_t* __restrict__ offs, int n,
                                                    const int32_t* __restrict__ vp, uint64_t* __restrict__ len) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= n) return;
  const uint64_t l = offs[d + 1] - offs[d];
  len[d] = vp[d] == clamp_len(l) ? l : 0;
}

// The valid documents, byte for byte, at out + out_offs[d]; tiles of the
// source as in k_valid_tiles, 64 consecutive bytes per step.
__global__ __launch_bounds__(64 * kWPB) void k_valid_copy(const uint8_t* __restrict__ buf,
                                                          const uint64_t* __restrict__ offs, int n,
                                                          const uint64_t* __restrict__ out_offs,
                                                          uint8_t* __restrict__ out) {
  if (n <= 0) return;
  const int lane = threadIdx.x & 63;
  const uint64_t ga = offs[0], gb = offs[n];
  if (gb <= ga) return;
  const uint64_t ntiles = (gb - ga + kTile - 1) / kTile;
  const uint64_t wave = (uint64_t)blockIdx.x * kWPB + (threadIdx.x >> 6), nwaves = (uint64_t)gridDim.x * kWPB;
  for (uint64_t t = wave; t < ntiles; t += nwaves) {
    const uint64_t T = ga + t * kTile, TE = T + kTile < gb ? T + kTile : gb;
    for (int d = first_doc_after(offs, n, T); d < n; ++d) {
      const uint64_t a = offs[d], b = offs[d + 1];
      if (a >= TE) break;
      const uint64_t o = out_offs[d];
      if (out_offs[d + 1] - o != b - a) continue;         // rejected (or empty): nothing to copy
      const uint64_t lo = T > a ? T : a, hi = TE < b ? TE : b;
      for (uint64_t q = lo + lane; q < hi; q += 64) out[o + (q - a)] = buf[q];
    }
  }
}

// The reference's result for a rejected document (compact_lang_det.cc:331-334
// returns UNKNOWN_LANGUAGE with is_reliable false before anything is scored).
__global__ __launch_bounds__(256) void k_valid_fixup(const uint64_t* __restrict__ offs, int n,
                                                     const int32_t* __restrict__ vp, cld_result* __restrict__ out,
                                                     int32_t* __restrict__ n_chunks, uint32_t unknown) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= n) return;
  if (vp[d] == clamp_len(offs[d + 1] - offs[d])) return;
  cld_result r;
  r.lang3[0] = r.lang3[1] = r.lang3[2] = (uint16_t)unknown;
  r.summary_lang = (uint16_t)unknown;
  r.percent3[0] = r.percent3[1] = r.percent3[2] = 0;
  r.is_reliable = 0;
  r.text_bytes = 0;
  r.normalized3[0] = r.normalized3[1] = r.normalized3[2] = 0.0;
  out[d] = r;
  if (n_chunks) n_chunks[d] = 0;
}

}  // namespace valid
}  // namespace cld

extern "C" {
// valid_prefix[i] of documents [buf + offs[i], buf + offs[i+1]), i < n.
// bytes_hint: offs[n] - offs[0] when the host knows it (sizes the tile grid), else 0.
hipError_t cld_launch_valid_prefix(const uint8_t* buf, const uint64_t* offs, int n, int32_t* vp, uint64_t bytes_hint,
                                   hipStream_t s) {
  using namespace cld::valid;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_valid, dim3((n + kWPB - 1) / kWPB), dim3(64 * kWPB), 0, s, buf, offs, n, vp);
  int blocks = kTileBlocks;
  if (bytes_hint) blocks = (int)std::min<uint64_t>(kTileBlocks, (bytes_hint / kTile + 2 + kWPB - 1) / kWPB);
  hipLaunchKernelGGL(k_valid_tiles, dim3(blocks), dim3(64 * kWPB), 0, s, buf, offs, n, vp);
  return hipGetLastError();
}

// out[offs[i] + j] = byte j of scrub(document i), i < n: the documents with every
// error position of the check replaced by 0x20, indexed like buf.  replaced[i]
// (nullable): the number of such positions; vp[i] (nullable): the first of them,
// the valid prefix of the document as given.  bytes_hint as above.  buf is not
// written; out may not overlap it.
hipError_t cld_launch_scrub(const uint8_t* buf, const uint64_t* offs, int n, uint8_t* out, int32_t* replaced,
                            int32_t* vp, uint64_t bytes_hint, hipStream_t s) {
  using namespace cld::valid;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_scrub, dim3((n + kWPB - 1) / kWPB), dim3(64 * kWPB), 0, s, buf, offs, n, out, replaced, vp);
  int blocks = kTileBlocks;
  if (bytes_hint) blocks = (int)std::min<uint64_t>(kTileBlocks, (bytes_hint / kTile + 2 + kWPB - 1) / kWPB);
  hipLaunchKernelGGL(k_scrub_tiles, dim3(blocks), dim3(64 * kWPB), 0, s, buf, offs, n, out, replaced, vp);
  return hipGetLastError();
}

// len[i] (n entries) = document i's length if vp says it is valid, else 0.
hipError_t cld_launch_valid_lens(const uint64_t* offs, int n, const int32_t* vp, uint64_t* len, hipStream_t s) {
  using namespace cld::valid;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_valid_lens, dim3((n + 255) / 256), dim3(256), 0, s, offs, n, vp, len);
  return hipGetLastError();
}

// Copies every document whose prepared length (out_offs) is its own to out.
hipError_t cld_launch_valid_copy(const uint8_t* buf, const uint64_t* offs, int n, const uint64_t* out_offs,
                                 uint8_t* out, uint64_t bytes_hint, hipStream_t s) {
  using namespace cld::valid;
  if (n <= 0) return hipSuccess;
  int blocks = kTileBlocks;
  if (bytes_hint) blocks = (int)std::min<uint64_t>(kTileBlocks, (bytes_hint / kTile + 1 + kWPB - 1) / kWPB);
  hipLaunchKernelGGL(k_valid_copy, dim3(blocks), dim3(64 * kWPB), 0, s, buf, offs, n, out_offs, out);
  return hipGetLastError();
}

// Overwrites the result (and, when n_chunks is given, the vector size) of every rejected document.
hipError_t cld_launch_valid_fixup(const uint64_t* offs, int n, const int32_t* vp, cld_result* out, int32_t* n_chunks,
                                  uint32_t unknown_language, hipStream_t s) {
  using namespace cld::valid;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_valid_fixup, dim3((n + 255) / 256), dim3(256), 0, s, offs, n, vp, out, n_chunks,
                     unknown_language);
  return hipGetLastError();
}
}
