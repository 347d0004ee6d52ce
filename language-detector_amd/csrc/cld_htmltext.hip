// cld_htmltext.hip -- the text of HTML pages with a map back to the page
// (cld_html_text_device), and chunk vectors on the text carried back to byte
// ranges of the page (cld_chunks_to_page_device).  The definitions are in
// cld_mi355x.h.
//
// k_html_text has the shape of k_html_rewrite (cld_html.hip), the private step
// in front of the scoring kernels: one wavefront per page, in three steps per
// segment of the page (whole 64-byte windows holding at most kHtmlTextCands
// '<' / '&' candidates):
//   1. the page goes to LDS (up to kHtmlTextStage bytes, NUL padded; a longer
//      page is read in place, every read bounded by its length); each lane
//      evaluates one '&' as if the walk reached it (ReadEntity: bytes consumed,
//      bytes decoded) into an LDS list;
//   2. the walk's order decides which candidates it reaches: one inside an
//      earlier reached tag or entity is skipped (a scalar walk over the list);
//      a reached '<' is scanned there by the whole wave, 64 bytes per step;
//   3. per 64-byte window each byte's output -- a text byte: itself; a reached
//      tag: its separator; a reached entity: its decoded bytes; a dropped '&' or
//      a byte inside a reached tag / entity: nothing -- is placed by a prefix
//      sum, with its source position where pos is wanted.
// What the scoring path needs and the text does not -- the well-formedness and
// HTML-lowering conditions, the lookahead marks, the gap starts after dropped
// '&'s -- is not here; what it does not need is: the separator choice (the lane
// that owns a reached '<' reads at most 12 bytes of the name and compares its
// 6-bit code against the list, a switch over constants), pos for every page,
// the padding of every page, the counts.  Every store of out and pos is guarded
// by the page's range; the range is clamped to buf_bytes.
//
// This translation unit states TagTables / scan_tag_wave and the candidate
// steps again instead of sharing them with cld_html.hip, which stays as it is:
// that kernel's code is the scoring path's and is not to move for this entry.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cld_kernels.h"
// cld_prims.hip defines one __constant__ with external linkage; this
// translation unit's copy of it (unused here) gets a name of its own.
#define kWordMask0 kWordMask0_htmltext
#include "cld_prims.hip"
#include "cld_wave.hip"
#undef kWordMask0

namespace cld {
namespace htext {

using wave::dpp_scan_incl;
using wave::excl_scan;
using wave::lanemask_lt;
using wave::OpMax;
using wave::rdl;
using wave::rdlu;
using wave::wshr1;
using wave::wsum;
using wave::wsync;

constexpr uint32_t kStage = kHtmlTextStage;   // pages up to this size are staged in LDS, larger ones read in place
constexpr int kCands = kHtmlTextCands;        // '<' / '&' candidates per segment of a page
constexpr int kWPB = 4;                       // waves (pages) per workgroup
// Windows whose bytes a wave loads before it works on the first of them: a page
// read in place costs one HBM latency per group of windows and step, not per window.
#ifndef HTMLTEXT_AHEAD
#define HTMLTEXT_AHEAD 4
#endif
constexpr int kAhead = HTMLTEXT_AHEAD;

// The tag parser's transition function as two LDS tables (tag_class / tag_next,
// cld_prims.hip), one lookup per byte and no branch per state.
constexpr int kTagStates = 40, kTagClasses = TC_PL + 1;
struct TagTables {
  uint8_t cls[256];
  uint8_t next[kTagStates * kTagClasses];
};

struct Smem {
  uint8_t text[kStage + 16];           // the page (up to kStage bytes)
  uint32_t pos[kCands];                // candidate positions, in page order
  uint32_t len[kCands];                // bytes the walk consumes there
  uint32_t dec[kCands];                // an entity's decoded bytes
  uint8_t meta[kCands];                // kind (0 tag, 1 entity, 2 dropped '&') | plen << 2 | reached << 6
};

// ScanToPossibleLetter by the whole wave (uniform arguments): text[start, lim).
// The parser sits in one state over long stretches, so each step tests the
// next 64 bytes at once -- the transition each would make from the current
// state -- and jumps to the first byte that changes the state.  No byte at or
// past lim is read.
__device__ __forceinline__ uint32_t scan_tag_wave(const TagTables& tt, const uint8_t* text, uint32_t start, uint32_t lim,
                                                  int lane) {
  uint32_t src = start;
  int e = 0, st = 0;
  while (src < lim) {
    const uint32_t x = src + (uint32_t)lane;
    const int ns = tt.next[st * kTagClasses + tt.cls[x < lim ? text[x] : 0]];
    const uint64_t chg = __ballot(x < lim && ns != st);
    if (!chg) {                                  // 64 bytes (or the rest) in this state
      e = st;
      src = lim - src > 64 ? src + 64 : lim;
      continue;
    }
    const int k = __builtin_ctzll(chg);
    e = rdl(ns, k);
    src += (uint32_t)k + 1;
    if (e <= 1) {
      --src;
      break;
    }
    st = e;
  }
  if (src >= lim) return lim - start;
  if (e != 0 && e != 2) {
    uint32_t off = src - start - 1;
    while (0 < off && text[start + off] != '<') --off;
    return off + 1;
  }
  return src - start;
}

// The block tags (CLD_HTMLTEXT_BLOCK_TAGS): a name of up to 10 letters and
// digits as 6 bits per character, compared as one 64-bit constant.
constexpr uint64_t tag_code(const char* s) {
  uint64_t v = 0;
  for (; *s; ++s) v = v << 6 | (uint64_t)(*s >= 'a' ? *s - 'a' + 1 : *s - '0' + 27);
  return v;
}
__device__ __forceinline__ bool block_code(uint64_t c) {
  switch (c) {
    case tag_code("address"): case tag_code("article"): case tag_code("aside"): case tag_code("blockquote"):
    case tag_code("body"): case tag_code("br"): case tag_code("dd"): case tag_code("div"): case tag_code("dl"):
    case tag_code("dt"): case tag_code("fieldset"): case tag_code("figcaption"): case tag_code("figure"):
    case tag_code("footer"): case tag_code("form"): case tag_code("h1"): case tag_code("h2"): case tag_code("h3"):
    case tag_code("h4"): case tag_code("h5"): case tag_code("h6"): case tag_code("head"): case tag_code("header"):
    case tag_code("hr"): case tag_code("html"): case tag_code("li"): case tag_code("main"): case tag_code("nav"):
    case tag_code("ol"): case tag_code("option"): case tag_code("p"): case tag_code("pre"): case tag_code("script"):
    case tag_code("section"): case tag_code("style"): case tag_code("table"): case tag_code("tbody"):
    case tag_code("td"): case tag_code("tfoot"): case tag_code("th"): case tag_code("thead"): case tag_code("title"):
    case tag_code("tr"): case tag_code("ul"):
      return true;
    default:
      return false;
  }
}
// The tag at d[p] == '<' is a block tag: at most 12 bytes after the '<' are
// read ('/', ten of a name, the byte that ends it), none past the page.
__device__ __forceinline__ bool block_tag(const DocView& d, int p) {
  int x = p + 1;
  if (d.at(x) == '/') ++x;
  uint64_t code = 0;
  for (int k = 0; k < 11; ++k) {
    const uint32_t c = d.at(x + k), l = c | 0x20;
    const uint32_t v = (l >= 'a' && l <= 'z') ? l - 'a' + 1 : (c >= '0' && c <= '9') ? c - '0' + 27 : 0u;
    if (v == 0) break;
    if (k == 10) return false;                   // longer than every listed name
    code = code << 6 | v;
  }
  return block_code(code);
}

// runetochar (getonescriptspan.cc:249-286) into a register: byte k at bits [8k, 8k + 8).
__device__ __forceinline__ uint32_t utf8_pack(uint32_t c, int* n) {
  if (c <= 0x7F) { *n = 1; return c; }
  if (c <= 0x7FF) { *n = 2; return (0xC0 | (c >> 6)) | (0x80 | (c & 0x3F)) << 8; }
  if (c > 0x10FFFF) c = 0xFFFD;
  if (c <= 0xFFFF) {
    *n = 3;
    return (0xE0 | (c >> 12)) | (0x80 | ((c >> 6) & 0x3F)) << 8 | (0x80 | (c & 0x3F)) << 16;
  }
  *n = 4;
  return (0xF0 | (c >> 18)) | (0x80 | ((c >> 12) & 0x3F)) << 8 | (0x80 | ((c >> 6) & 0x3F)) << 16 |
         (0x80 | (c & 0x3F)) << 24;
}

constexpr uint32_t kLdsPerCU = 160 * 1024;
constexpr uint32_t kBlocksPerCU =
    std::min<uint32_t>(8, kLdsPerCU / (uint32_t)(kWPB * sizeof(Smem) + sizeof(TagTables)));   // 7

struct Counts {                                  // (wave-uniform)
  uint32_t tags, entities, dropped;
};

// One page (steps 1-3 above): txt is the page in LDS (kStaged, up to kStage
// bytes) or in place in HBM, L <= INT32_MAX its length, o / hp (nullable) its
// range of out / pos.  Returns text_len.
template <bool kStaged>
__device__ __forceinline__ uint32_t text_page(const DevTables& T, const TagTables& tt, Smem& S, const uint8_t* txt,
                                              const uint32_t L, uint8_t* __restrict__ o, uint32_t* __restrict__ hp,
                                              const bool block_lf, const int lane, Counts& cnt) {
  const DocView dv{txt, (int)L};
  uint32_t q = 0;                                              // output bytes so far
  uint32_t cover = 0;                                          // end of the last reached candidate so far
  uint32_t cur = 0;                                            // the walk's position after the last reached one
  for (uint32_t P0 = 0; P0 < L;) {
    // 1a. the segment's candidates, in page order: whole windows while they fit
    int K = 0;
    uint32_t P1 = P0;
    bool full = false;
    for (uint32_t g0 = P0; g0 < L && !full; g0 += 64 * kAhead) {
      uint32_t c[kAhead];                                      // kAhead windows' bytes in flight at once
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const uint32_t p = g0 + 64 * u + (uint32_t)lane;
        c[u] = p < L ? txt[p] : 0u;
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const uint32_t w0 = g0 + 64 * u;
        if (w0 >= L || full) break;
        const bool cand = c[u] == '<' || c[u] == '&';
        const uint64_t m = __ballot(cand);
        if (K + __popcll(m) > kCands) {                        // (a window holds at most 64)
          full = true;
          break;
        }
        if (cand) S.pos[K + __popcll(m & lanemask_lt(lane))] = w0 + (uint32_t)lane;
        K += __popcll(m);
        P1 = L - w0 > 64 ? w0 + 64 : L;
      }
    }
    wsync();
    // 1b. each candidate as if the walk reached it
    for (int j = lane; j < K; j += 64) {
      const int p = (int)S.pos[j];
      int ln = 0, kind = 0, plen = 0;                          // (a reached tag is scanned in step 2)
      uint32_t dec = 0;
      if (txt[p] == '&') {
        int tlen = 0;
        const int32_t v = read_entity(T, dv, p, (int)L - p, &tlen);
        if (v > 0) {
          kind = 1;
          ln = tlen;
          dec = utf8_pack((uint32_t)v, &plen);
        } else {
          kind = 2;                                            // undecodable: the '&' is dropped
          ln = 1;
        }
      }
      S.len[j] = (uint32_t)ln;
      S.dec[j] = dec;
      S.meta[j] = (uint8_t)(kind | (plen << 2));
    }
    wsync();
    // 2. which candidates the walk reaches: past the end of the last reached one
    for (int j0 = 0; j0 < K; j0 += 64) {
      const int j = j0 + lane;
      const uint32_t p = j < K ? S.pos[j] : 0xFFFFFFFFu, ln = j < K ? S.len[j] : 0u;
      const int m = K - j0 < 64 ? K - j0 : 64;
      const uint64_t tag_m = __ballot(j < K && (S.meta[j] & 3) == 0);
      uint64_t reach = 0;
      for (int t = 0; t < m; ++t) {
        const uint32_t pt = rdlu(p, t);
        if (pt >= cur) {
          reach |= 1ull << t;
          uint32_t lt = rdlu(ln, t);
          if ((tag_m >> t) & 1) {                              // a reached tag: ScanToPossibleLetter, by the wave
            lt = scan_tag_wave(tt, txt, pt, L, lane);
            if (lane == t) S.len[j] = lt;
          }
          cur = pt + lt;
        }
      }
      if (j < K) S.meta[j] = (uint8_t)(S.meta[j] | (((reach >> lane) & 1) ? 0x40 : 0));
    }
    wsync();
    // 3. the output, window by window
    int cb = 0;
    auto window = [&](const uint32_t w0, const uint32_t c) {
      const uint32_t p = w0 + (uint32_t)lane;
      const bool in = p < L;
      const bool cand = in && (c == '<' || c == '&');
      const uint64_t cm = __ballot(cand);
      const int j = cand ? cb + __popcll(cm & lanemask_lt(lane)) : 0;
      cb += __popcll(cm);
      const uint32_t meta = cand ? S.meta[j] : 0u;
      const bool reached = (meta & 0x40) != 0;
      const uint32_t end = reached ? p + S.len[j] : 0u;
      // covered: inside a reached candidate that starts before p (the running
      // maximum of reached ends, carried across windows and segments)
      const uint32_t mx = dpp_scan_incl(end, 0u, OpMax());
      const uint32_t before = wshr1(mx, 0u);
      const uint32_t cov_end = before > cover ? before : cover;
      const bool covered = in && !reached && p < cov_end;
      const int kind = meta & 3, plen = (meta >> 2) & 7;
      const bool text = in && !covered && !reached;
      const bool tag = reached && kind == 0, ent = reached && kind == 1;
      const int emit = ent ? plen : (tag || text) ? 1 : 0;
      const uint32_t at = q + (uint32_t)excl_scan(emit, lane);
      if (text || tag) {
        const uint8_t b = text ? (uint8_t)c : (block_lf && block_tag(dv, (int)p)) ? (uint8_t)0x0A : (uint8_t)0x20;
        if (at < L) {
          o[at] = b;
          if (hp) hp[at] = p;
        }
      } else if (ent) {
        const uint32_t d = S.dec[j];
        for (int k = 0; k < plen; ++k)
          if (at + k < L) {
            o[at + k] = (uint8_t)(d >> (8 * k));
            if (hp) hp[at + k] = p + k;
          }
      }
      cnt.tags += (uint32_t)__popcll(__ballot(tag));
      cnt.entities += (uint32_t)__popcll(__ballot(ent));
      cnt.dropped += (uint32_t)__popcll(__ballot(reached && kind == 2));
      q = rdlu(at + (uint32_t)emit, 63);
      const uint32_t wmx = rdlu(mx, 63);
      cover = wmx > cover ? wmx : cover;
    };
    for (uint32_t g0 = P0; g0 < P1; g0 += 64 * kAhead) {
      uint32_t c[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const uint32_t p = g0 + 64 * u + (uint32_t)lane;
        c[u] = p < L ? txt[p] : 0u;
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
        if (g0 + 64 * u < P1) window(g0 + 64 * u, c[u]);
    }
    wsync();                                                   // S.* reused by the next segment
    P0 = P1;
  }
  q = q < L ? q : L;
  // the page keeps its length: spaces after the text
  for (uint32_t p = q + (uint32_t)lane; p < L; p += 64) {
    o[p] = ' ';
    if (hp) hp[p] = L;
  }
  return q;
}

__global__ __launch_bounds__(64 * kWPB) void k_html_text(const DevTables* __restrict__ Tp, const uint8_t* __restrict__ buf,
                                                        const uint64_t* __restrict__ offs, uint32_t n, uint64_t bb,
                                                        uint32_t flags, uint8_t* __restrict__ out,
                                                        int32_t* __restrict__ text_len, uint32_t* __restrict__ pos,
                                                        cld_htmltext_status* __restrict__ status) {
  __shared__ Smem smem[kWPB];
  __shared__ TagTables tt;
  for (int t = threadIdx.x; t < 256 + kTagStates * kTagClasses; t += blockDim.x) {
    if (t < 256) tt.cls[t] = (uint8_t)tag_class((uint8_t)t);
    else tt.next[t - 256] = (uint8_t)tag_next((t - 256) / kTagClasses, (t - 256) % kTagClasses);
  }
  __syncthreads();
  const DevTables& T = *Tp;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  Smem& S = smem[wv];
  const bool block_lf = (flags & CLD_HTMLTEXT_BLOCK_LF) != 0;
  Counts cnt{0, 0, 0};
  uint64_t text_bytes = 0, tags = 0;
  const uint32_t nw = gridDim.x * kWPB;
  for (uint32_t i = blockIdx.x * kWPB + (uint32_t)wv; i < n; i += nw) {
    // the page's range, inside [0, buf_bytes) whatever the offsets say
    const uint64_t a = min(offs[i], bb), b = min(offs[i + 1], bb);
    const uint32_t L = (uint32_t)min(b > a ? b - a : (uint64_t)0, (uint64_t)0x7FFFFFFF);
    uint32_t* hp = pos ? pos + a : nullptr;
    uint32_t q;
    cnt.tags = 0;
    if (L > kStage) {
      q = text_page<false>(T, tt, S, buf + a, L, out + a, hp, block_lf, lane, cnt);
    } else {
      // the page into LDS, NUL padded
      const uint8_t* g = buf + a;
      for (uint32_t p = (uint32_t)lane * 4; p < L + 16; p += 256) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) v |= (uint32_t)(p + k < L ? g[p + k] : 0) << (8 * k);
        *reinterpret_cast<uint32_t*>(&S.text[p]) = v;
      }
      wsync();
      q = text_page<true>(T, tt, S, S.text, L, out + a, hp, block_lf, lane, cnt);
    }
    text_bytes += q;
    tags += cnt.tags;
    if (text_len && lane == 0) text_len[i] = (int32_t)q;
    wsync();
  }
  // integer sums: the status is the same whatever order the waves arrive in
  if (status && lane == 0) {
    if (text_bytes) atomicAdd((unsigned long long*)&status->text_bytes, (unsigned long long)text_bytes);
    if (tags) atomicAdd((unsigned long long*)&status->tags, (unsigned long long)tags);
    if (cnt.entities) atomicAdd(&status->entities, cnt.entities);
    if (cnt.dropped) atomicAdd(&status->dropped, cnt.dropped);
  }
}

// Chunk vectors on the text to chunk vectors on the page: one wave per
// document, lanes over its chunks.  A lane reads its chunk before it writes it
// (out may be chunks).
__global__ __launch_bounds__(256) void k_chunks_to_page(const uint64_t* __restrict__ offs, uint32_t n,
                                                       const uint32_t* __restrict__ pos, const cld_chunk* chunks,
                                                       uint64_t chunk_cap, const uint64_t* __restrict__ coffs,
                                                       cld_chunk* out) {
  const uint32_t lane = threadIdx.x & 63, nw = gridDim.x * (blockDim.x >> 6);
  for (uint32_t i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n; i += nw) {
    const uint64_t a = offs[i], b = offs[i + 1];
    const int64_t len = b > a ? (int64_t)(b - a) : 0;
    const uint64_t end = min(coffs[i + 1], chunk_cap);
    const uint32_t* dp = pos + a;
    for (uint64_t c = coffs[i] + lane; c < end; c += 64) {
      const cld_chunk ch = chunks[c];
      const int64_t s = min(max((int64_t)ch.offset, (int64_t)0), len);
      const int64_t e = min(max((int64_t)ch.offset + ch.bytes, s), len);
      const int64_t ps = s < len ? min((int64_t)dp[s], len) : len;
      const int64_t pe = e < len ? min((int64_t)dp[e], len) : len;
      cld_chunk r;
      r.offset = (int32_t)min(ps, (int64_t)INT32_MAX);
      r.bytes = (int32_t)min(max(pe - ps, (int64_t)0), (int64_t)INT32_MAX);
      r.lang1 = ch.lang1;
      r.pad = 0;
      out[c] = r;
    }
  }
}

}  // namespace htext
}  // namespace cld

extern "C" {
hipError_t cld_launch_html_text(const DevTables* d_T, const uint8_t* buf, const uint64_t* offs, uint32_t n,
                                uint64_t buf_bytes, uint32_t flags, uint8_t* out, int32_t* text_len, uint32_t* pos,
                                cld_htmltext_status* status, uint32_t max_wgs, hipStream_t s) {
  using namespace cld::htext;
  if (status) {
    hipError_t e = hipMemsetAsync(status, 0, sizeof(cld_htmltext_status), s);
    if (e != hipSuccess) return e;
  }
  if (n == 0) return hipSuccess;
  // persistent, pages by stride: as many workgroups as are resident at once (LDS bounds them), so that no
  // wave starts on its pages only when another has finished all of its own
  static const uint32_t resident = [] {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0)
      cus = 256;
    return (uint32_t)cus * kBlocksPerCU;
  }();
  const uint32_t cap = max_wgs ? std::min<uint32_t>(max_wgs, resident) : resident;
  const uint32_t blocks = std::min<uint32_t>((n + kWPB - 1) / kWPB, cap);
  hipLaunchKernelGGL(k_html_text, dim3(blocks), dim3(64 * kWPB), 0, s, d_T, buf, offs, n, buf_bytes, flags, out, text_len,
                     pos, status);
  return hipGetLastError();
}

hipError_t cld_launch_chunks_to_page(const uint64_t* offs, uint32_t n, const uint32_t* pos, const cld_chunk* chunks,
                                     uint64_t chunk_cap, const uint64_t* chunk_offs, cld_chunk* out, hipStream_t s) {
  using namespace cld::htext;
  if (n == 0 || chunk_cap == 0) return hipSuccess;
  const uint32_t blocks = std::min<uint32_t>((n + 3) / 4, 2048u);
  hipLaunchKernelGGL(k_chunks_to_page, dim3(blocks), dim3(256), 0, s, offs, n, pos, chunks, chunk_cap, chunk_offs, out);
  return hipGetLastError();
}
}
