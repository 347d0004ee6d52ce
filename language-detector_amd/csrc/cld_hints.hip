// cld_hints.hip -- ApplyHints on the GPU: per document the CLDLangPriors, the
// 16 langprobs they become and the routing byte enqueue() expects.
//
// The device restatement of cld_hints.cpp, which stays the specification (it
// is pinned to the reference's compact_lang_det_hint_code.cc by
// tests/test_html_hints.py); tests/test_gpu_device_hints.py holds this kernel
// to it bit for bit.  One wavefront per document:
//
//  1. HTML only: the scan window (the first min(len, 8192) bytes) is staged in
//     LDS.  Bytes at and past the bound do not exist for the scanner.
//  2. The window goes by in tiles of 64 bytes.  One ballot finds the '<' bytes
//     of a tile; every one of them that has a '>', '<' or '&' after it inside
//     the window starts a tag (GetLangTagsFromHtml resumes at the terminator,
//     so no '<' is ever skipped), and the tags are independent.  Each lane
//     parses the tag that starts at its byte (parse_tag<false>) and reports
//     whether it holds a language attribute with a quoted value.
//  3. Only the merge depends on page order.  The tags that reported a value
//     are taken in lane order, and the whole wave runs parse_tag<true> on one
//     of them at a time with wave-uniform arguments: every lane computes the
//     same thing, lane 0 writes the value behind the accumulated string in
//     LDS, and all lanes share the substring search (out.find(t)).  Six commas
//     in the accumulated string end the scan: more than four are left after
//     the last byte is erased, and such a list is ignored whole.
//  4. Lane 0 alone: the tokens (at most five, of at most 16 bytes) through the
//     two lang-tag tables, then the content-language hint (its text goes
//     through LDS in pieces, staged by the wave), TLD, encoding and language
//     hints, the stable trim to four, the boosts and close-set whacks.
//
// All per-document state that is indexed at run time (priors, rings, close-set
// counts, tokens, the lookup key) lives in LDS, so the kernel needs no scratch.
// Every global read is of the document's own bytes [offs[i], offs[i+1]), of
// hint_text[0, hint_text_bytes), of hints[i] or of the table blob.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cld_kernels.h"
#include "cldt_format.h"

namespace hnt {

constexpr int kWindow = 8 << 10;       // compact_lang_det_impl.cc:1596-1611: the first 8 KB
constexpr int kTile = 64;              // bytes per ballot
constexpr int kOutCap = kWindow;       // the accumulated string fits the window: a value of r bytes copies to at
                                       // most r + 1, and it sits in the window behind at least seven bytes of
                                       // its own (` lang="`, `:lang="`, ` content="`), disjoint from every other
constexpr int kMaxPriors = 14;         // kMaxOneCLDLangPrior (compact_lang_det_hint_code.h:34)
constexpr int kMaxTok = 5;             // a list of more than 4 commas is ignored whole
constexpr int kTokBytes = 16;          // a longer token is skipped
constexpr int kCloseSetSize = 10;      // lang_script.cc:258

struct Smem {
  uint8_t win[kWindow + 32];           // window byte p at win[mis + p] (mis: the document's address mod 16)
  uint8_t out[kOutCap];                // accumulated values; then the content-language text, piece by piece
  uint8_t action[256], remap[256];     // kLangCodeAction / kLangCodeRemap
  uint8_t tok[kMaxTok][kTokBytes];
  int32_t tok_len[kMaxTok];
  uint8_t key[kTokBytes + 4];
  int16_t pri[kMaxPriors];
  uint32_t ring[16];                   // boost latn, boost othr, whack latn, whack othr: 4 each
  int32_t ring_n[4];
  int32_t count[kCloseSetSize + 1];
};

struct Ctx {
  Smem* s;
  int W;          // window bytes
  int mis;
  int olen;       // bytes accumulated in s->out
  int commas;     //   and the commas among them
  bool dead;      // six commas: nothing later can matter
};

#define HNT_FN __device__ __forceinline__

// Window byte i; bytes outside the window read as NUL (the host scans a copy
// padded with NULs).
HNT_FN int B(const Ctx& c, int i) { return (unsigned)i < (unsigned)c.W ? c.s->win[c.mis + i] : 0; }

HNT_FN bool is_term(int ch) { return ch == '>' || ch == '<' || ch == '&'; }

// The scanners of GetLangTagsFromHtml, as in cld_hints.cpp.
HNT_FN int find_quote_start(const Ctx& c, int pos, int max_pos) {
  for (int i = pos; i < max_pos; ++i) {
    const int ch = B(c, i);
    if (ch == '"' || ch == '\'') return i;
    if (ch != ' ') return -1;
  }
  return -1;
}
HNT_FN int find_quote_end(const Ctx& c, int pos, int max_pos) {
  for (int i = pos; i < max_pos; ++i) {
    const int ch = B(c, i);
    if (ch == '"' || ch == '\'') return i;
    if (ch == '>' || ch == '=' || ch == '<' || ch == '&') return i - 1;
  }
  return -1;
}
HNT_FN int find_equal_sign(const Ctx& c, int pos, int max_pos) {
  for (int i = pos; i < max_pos; ++i) {
    const int ch = B(c, i);
    if (ch == '=') return i;
    if (ch == '"' || ch == '\'') {               // skip the quoted run (backslash escapes)
      int j = i + 1;
      for (; j < max_pos; ++j) {
        const int d = B(c, j);
        if (d == ch) break;
        if (d == '\\') ++j;
      }
      i = j;
    }
  }
  return -1;
}
template <int N>
HNT_FN bool find_before(const Ctx& c, int min_pos, int pos, const char (&lit)[N]) {
  constexpr int len = N - 1;
  if (pos - min_pos < len) return false;
  int i = pos;
  while (i > min_pos + len && B(c, i - 1) == ' ') --i;
  i -= len;
  if (i < min_pos) return false;
#pragma unroll
  for (int j = 0; j < len; ++j)
    if ((B(c, i + j) | 0x20) != lit[j]) return false;
  return true;
}
template <int N>
HNT_FN bool find_after(const Ctx& c, int pos, int max_pos, const char (&lit)[N]) {
  constexpr int len = N - 1;
  if (max_pos - pos < len) return false;
  int i = pos;
  while (i < max_pos - len) {
    const int ch = B(c, i);
    if (ch == ' ' || ch == '"' || ch == '\'') ++i;
    else break;
  }
#pragma unroll
  for (int j = 0; j < len; ++j)
    if ((B(c, i + j) | 0x20) != lit[j]) return false;
  return true;
}

// One step of the three-state language-attribute copier (CopyOneQuotedString):
// the byte it emits, or -1.
HNT_FN int copier_step(const Smem* s, int ch, int* state) {
  const int e = s->action[ch] >> (3 * *state);
  *state = e & 3;
  if (!(e & 4)) return -1;
  return *state == 0 ? s->remap[ch] : ',';
}

// The value in window bytes [p0, p1) through the copier, appended to the
// accumulated string unless it is empty or already a substring of it.  The
// whole wave calls this with the same arguments.
HNT_FN void merge_value(Ctx& c, int p0, int p1, int lane) {
  Smem* s = c.s;
  int state = 1, tl = 0, tc = 0;
  auto push = [&](int o) {
    if (lane == 0 && c.olen + tl < kOutCap) s->out[c.olen + tl] = (uint8_t)o;
    tc += o == ',';
    ++tl;
  };
  for (int i = p0; i < p1; ++i) {
    const int o = copier_step(s, B(c, i), &state);
    if (o >= 0) push(o);
  }
  if (state == 0) push(',');
  if (tl == 0) return;
  if (c.olen + tl > kOutCap) {         // (cannot happen, see kOutCap)
    c.dead = true;
    return;
  }
  __syncthreads();
  bool found = false;
  const int last = c.olen - tl;        // the last start at which the value still fits
  for (int s0 = 0; s0 <= last; s0 += 64) {
    const int p = s0 + lane;
    bool hit = false;
    if (p <= last) {
      int k = 0;
      while (k < tl && s->out[p + k] == s->out[c.olen + k]) ++k;
      hit = k == tl;
    }
    if (__ballot(hit)) {
      found = true;
      break;
    }
  }
  __syncthreads();                     // the next value overwrites out[olen ..)
  if (!found) {
    c.olen += tl;
    c.commas += tc;
    if (c.commas >= 6) c.dead = true;
  }
}

// The tag whose '<' is at st and whose content ends before en.  MERGE false
// (each lane its own tag): does the tag hold a language attribute with a
// quoted value?  MERGE true (the whole wave, one tag): merge those values.
template <bool MERGE>
HNT_FN bool parse_tag(Ctx& c, int st, int en, int lane) {
  if (find_after(c, st + 1, en, "!--") || find_after(c, st + 1, en, "font ") || find_after(c, st + 1, en, "script ") ||
      find_after(c, st + 1, en, "link ") || find_after(c, st + 1, en, "img ") || find_after(c, st + 1, en, "a "))
    return false;
  const bool in_meta = find_after(c, st + 1, en, "meta ");
  bool content_is_lang = false;
  int kk = st + 1, eq;
  while ((eq = find_equal_sign(c, kk, en)) >= 0) {
    if (in_meta) {
      if (find_before(c, kk, eq, " http-equiv") && find_after(c, eq + 1, en, "content-language ")) {
        content_is_lang = true;
      } else if (find_before(c, kk, eq, " name") &&
                 (find_after(c, eq + 1, en, "dc.language ") || find_after(c, eq + 1, en, "language "))) {
        content_is_lang = true;
      }
    }
    if ((content_is_lang && find_before(c, kk, eq, " content")) || find_before(c, kk, eq, " lang") ||
        find_before(c, kk, eq, ":lang")) {
      const int q0 = find_quote_start(c, eq + 1, en);
      const int q1 = q0 < 0 ? -1 : find_quote_end(c, q0 + 1, en);
      if (q1 >= 0) {
        if constexpr (!MERGE) {
          return true;
        } else {
          merge_value(c, q0 + 1, q1, lane);
          if (c.dead) return true;
        }
      }
    }
    kk = eq + 1;
  }
  return false;
}

// GetLangTagsFromHtml over the staged window: the accumulated string in s->out.
HNT_FN void scan_window(Ctx& c, int lane) {
  for (int t0 = 0; t0 < c.W && !c.dead; t0 += kTile) {
    const int p = t0 + lane;
    const int ch = B(c, p);
    const bool lt = ch == '<';
    const uint64_t ltm = __ballot(lt);
    if (!ltm) continue;
    const uint64_t tm = __ballot(is_term(ch));
    // the tile's last '<' may end in a later tile: the wave looks for that terminator together
    const uint64_t above = lane == 63 ? 0 : tm >> (lane + 1);
    int far = -1;
    if (__ballot(lt && !above)) {
      for (int t1 = t0 + kTile; t1 < c.W; t1 += kTile) {
        const uint64_t m2 = __ballot(is_term(B(c, t1 + lane)));
        if (m2) {
          far = t1 + __builtin_ctzll(m2);
          break;
        }
      }
    }
    // a tag without '=' holds no attribute: the tags that end inside the tile are told by one more ballot
    const uint64_t eqm = __ballot(ch == '=');
    int en = -1;
    bool cand = false;
    if (lt) {
      const int k = above ? __builtin_ctzll(above) : 0;          // the terminator is k + 1 bytes on
      const int e = above ? p + 1 + k : far;
      const bool has_eq = !above || ((eqm >> (lane + 1)) & ((1ull << k) - 1)) != 0;
      if (e >= 0 && has_eq) {                        // (e < 0, no terminator inside the window: not a tag)
        en = B(c, e) == '>' ? e : e - 1;             // FindTagEnd
        cand = parse_tag<false>(c, p, en, lane);
      }
    }
    uint64_t cm = __ballot(cand);
    while (cm && !c.dead) {
      const int j = __builtin_ctzll(cm);
      cm &= cm - 1;
      parse_tag<true>(c, __shfl(p, j, 64), __shfl(en, j, 64), lane);
    }
  }
}

// ---- the tokens of a comma list (SetCLDLangTagsHint's walk), collected while
// the list goes by: at most kMaxTok when the list counts at all.  Wave-uniform;
// lane 0 writes.
struct Sink {
  int ntok = 0, cur = 0, commas = 0;
};
HNT_FN void sink_close(Smem* s, Sink& k, int lane) {
  if (k.ntok < kMaxTok && lane == 0) s->tok_len[k.ntok] = k.cur;
  ++k.ntok;
  k.cur = 0;
}
HNT_FN void sink_feed(Smem* s, Sink& k, int ch, int lane) {
  if (ch == ',') {
    ++k.commas;
    sink_close(s, k, lane);
  } else {
    if (k.cur < kTokBytes && k.ntok < kMaxTok && lane == 0) s->tok[k.ntok][k.cur] = (uint8_t)ch;
    ++k.cur;
  }
}
// -> the number of tokens to look up (0: the list is ignored)
HNT_FN int sink_finish(Smem* s, Sink& k, int lane) {
  if (k.cur > 0) sink_close(s, k, lane);            // a last token without its comma
  return k.commas > 4 ? 0 : (k.ntok < kMaxTok ? k.ntok : kMaxTok);
}

// ---- lane 0: priors
HNT_FN int weight(int16_t olp) { return olp >> 10; }               // GetCLDPriorWeight
HNT_FN int lang_of(int16_t olp) { return olp & 0x3FF; }            // GetCLDPriorLang
HNT_FN int16_t with_weight(int16_t olp, int w) { return (int16_t)((olp & 0x3FF) + w * 1024); }

HNT_FN void merge_max(Smem* s, int* n, int16_t olp) {              // MergeCLDLangPriorsMax
  if (olp == 0) return;
  for (int i = 0; i < *n; ++i)
    if (lang_of(s->pri[i]) == lang_of(olp)) {
      const int a = weight(s->pri[i]), b = weight(olp);
      s->pri[i] = with_weight(s->pri[i], a >= b ? a : b);
      return;
    }
  if (*n < kMaxPriors) s->pri[(*n)++] = olp;
}
HNT_FN void merge_boost(Smem* s, int* n, int16_t olp) {            // MergeCLDLangPriorsBoost
  if (olp == 0) return;
  for (int i = 0; i < *n; ++i)
    if (lang_of(s->pri[i]) == lang_of(olp)) {
      s->pri[i] = with_weight(s->pri[i], weight(s->pri[i]) + 2);
      return;
    }
  if (*n < kMaxPriors) s->pri[(*n)++] = olp;
}
HNT_FN int absw(int16_t olp) {
  const int w = weight(olp);
  return w < 0 ? -w : w;
}
HNT_FN void trim(Smem* s, int* n, int max_entries) {               // TrimCLDLangPriors
  if (*n <= max_entries) return;
  for (int i = 0; i < *n; ++i) {                                   // insertion sort by |weight|, stable
    const int16_t t = s->pri[i];
    const int w = absw(t);
    int k = i;
    for (; k > 0 && absw(s->pri[k - 1]) < w; --k) s->pri[k] = s->pri[k - 1];
    s->pri[k] = t;
  }
  *n = max_entries;
}

// Binary search of a CLDT hint table for the NUL-terminated key (the runtime
// has checked that every key of the table ends inside its pool).
HNT_FN bool lookup(const uint8_t* sec, const uint8_t* key, int16_t* p1, int16_t* p2) {
  const uint32_t n = *(const uint32_t*)sec;
  const cldt_hint_entry* e = (const cldt_hint_entry*)(sec + 4);
  const uint8_t* pool = (const uint8_t*)(e + n);
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const uint8_t* a = pool + e[mid].key_off;
    int cmp = 0;
    for (int k = 0;; ++k) {
      const int x = a[k], y = key[k];
      if (x != y) {
        cmp = x < y ? -1 : 1;
        break;
      }
      if (!x) break;
    }
    if (cmp < 0) lo = mid + 1;
    else if (cmp > 0) hi = mid;
    else {
      *p1 = e[mid].prior1;
      *p2 = e[mid].prior2;
      return true;
    }
  }
  return false;
}

// SetCLDLangTagsHint over the collected tokens.
HNT_FN void lang_tags_hint(const DevHints& H, Smem* s, int ntok, int* n) {
  for (int t = 0; t < ntok; ++t) {
    const int len = s->tok_len[t];
    if (len > kTokBytes) continue;
    for (int k = 0; k < len; ++k) s->key[k] = s->tok[t][k];
    s->key[len] = 0;
    int16_t p1, p2;
    if (lookup(H.langtag1, s->key, &p1, &p2)) {
      merge_max(s, n, p1);
      merge_max(s, n, p2);
      continue;
    }
    int l = 0;                                       // the part before the first hyphen
    while (s->key[l] && s->key[l] != '-') ++l;
    s->key[l] = 0;
    if (l <= 3 && lookup(H.langtag2, s->key, &p1, &p2)) {
      merge_max(s, n, p1);
      merge_max(s, n, p2);
    }
  }
}

// ---- lane 0: boosts and whacks (compact_lang_det_impl.cc:1645-1684)
HNT_FN bool is_latn(const DevHints& H, int lang) { return (uint32_t)lang < H.l2p_size && lang == H.p2l_latn[H.l2p[lang]]; }
HNT_FN bool is_othr(const DevHints& H, int lang) { return (uint32_t)lang < H.l2p_size && lang == H.p2l_othr[H.l2p[lang]]; }
HNT_FN int close_set(const DevHints& H, int lang) { return (uint32_t)lang < H.n_langs ? H.close_set[lang] : 0; }
// MakeLangProb with kLgProbV2TblBackmap = {0, 0, 1, 3, 6, 10, ..., 66}: q (q - 1) / 2, q clamped to 12
HNT_FN uint32_t make_lang_prob(const DevHints& H, int lang, int qprob) {
  const uint32_t ps = (uint32_t)lang < H.l2p_size ? H.l2p[lang] : 0;
  const int q = qprob > 12 ? 12 : qprob;
  return (ps << 8) | (uint32_t)(q * (q - 1) / 2);
}
HNT_FN void ring_push(Smem* s, int r, uint32_t v) {
  s->ring[4 * r + s->ring_n[r]] = v;
  s->ring_n[r] = (s->ring_n[r] + 1) & 3;
}
HNT_FN void add_one_whack(const DevHints& H, Smem* s, int whacker, int whackee) {
  const uint32_t lp = make_lang_prob(H, whackee, 1);
  if (is_latn(H, whacker) && is_latn(H, whackee)) ring_push(s, 2, lp);
  if (is_othr(H, whacker) && is_othr(H, whackee)) ring_push(s, 3, lp);
}
HNT_FN void add_close_lang_whack(const DevHints& H, Smem* s, int lang) {
  if ((uint32_t)lang == H.chinese) { add_one_whack(H, s, lang, (int)H.chinese_t); return; }
  if ((uint32_t)lang == H.chinese_t) { add_one_whack(H, s, lang, (int)H.chinese); return; }
  const int base = close_set(H, lang);
  if (base == 0) return;
  for (uint32_t i = 0; i < H.l2p_size; ++i)
    if (close_set(H, (int)i) == base && (int)i != lang) add_one_whack(H, s, lang, (int)i);
}
HNT_FN void hint_boosts(const DevHints& H, Smem* s, int n) {
  for (int k = 0; k < 16; ++k) s->ring[k] = 0;
  for (int k = 0; k < 4; ++k) s->ring_n[k] = 0;
  for (int k = 0; k <= kCloseSetSize; ++k) s->count[k] = 0;
  for (int i = 0; i < n; ++i) {
    const int lang = lang_of(s->pri[i]), q = weight(s->pri[i]);
    if (q > 0) {
      const uint32_t lp = make_lang_prob(H, lang, q);
      if (is_latn(H, lang)) ring_push(s, 0, lp);
      if (is_othr(H, lang)) ring_push(s, 1, lp);
    }
  }
  for (int i = 0; i < n; ++i) {
    const int lang = lang_of(s->pri[i]);
    const int cs = close_set(H, lang);
    if (cs >= 0 && cs <= kCloseSetSize) ++s->count[cs];
    if ((uint32_t)lang == H.chinese || (uint32_t)lang == H.chinese_t) ++s->count[kCloseSetSize];
  }
  for (int i = 0; i < n; ++i) {
    const int lang = lang_of(s->pri[i]), q = weight(s->pri[i]);
    if (q <= 0) continue;
    const int cs = close_set(H, lang);
    if (cs > 0 && cs <= kCloseSetSize && s->count[cs] == 1) add_close_lang_whack(H, s, lang);
    if (((uint32_t)lang == H.chinese || (uint32_t)lang == H.chinese_t) && s->count[kCloseSetSize] == 1)
      add_close_lang_whack(H, s, lang);
  }
}

__global__ __launch_bounds__(64) void k_apply_hints(DevHints H, const uint8_t* __restrict__ buf,
                                                     const uint64_t* __restrict__ offs, int n,
                                                     const cld_hints_dev* __restrict__ hints,
                                                     const uint8_t* __restrict__ hint_text, uint64_t hint_text_bytes,
                                                     int plain, const uint32_t* __restrict__ doc_flags,
                                                     int16_t* __restrict__ priors14,
                                                     uint32_t* __restrict__ boosts16, uint8_t* __restrict__ special) {
  __shared__ __align__(16) Smem sm;
  Smem* s = &sm;
  const int doc = blockIdx.x, lane = threadIdx.x;
  if (doc >= n) return;
  // the document's own mode (the _docflags entries): the word is the caller's,
  // possibly unchecked device memory, so only its three bits count
  const uint32_t df = doc_flags ? doc_flags[doc] & (CLD_FLAG_HTML | CLD_FLAG_SCORE_AS_QUADS | CLD_FLAG_BEST_EFFORT) : 0u;
  if (df & CLD_FLAG_HTML) plain = 0;
  ((uint32_t*)s->action)[lane] = ((const uint32_t*)H.action)[lane];
  ((uint32_t*)s->remap)[lane] = ((const uint32_t*)H.remap)[lane];
  int np = 0;                                          // priors so far (lane 0's counts)
  const uint64_t a = offs[doc], b = offs[doc + 1];
  const uint64_t len = b > a ? b - a : 0;
  if (!plain && len) {
    Ctx c;
    c.s = s;
    c.W = (int)(len < (uint64_t)kWindow ? len : (uint64_t)kWindow);
    const uint8_t* g = buf + a;
    c.mis = (int)((uintptr_t)g & 15);
    c.olen = 0;
    c.commas = 0;
    c.dead = false;
    // 16 bytes per lane from aligned addresses; the vectors that reach outside the window byte by byte
    const uint8_t* base = g - c.mis;
    const int end = c.mis + c.W, nv = (end + 15) >> 4;
    for (int v = lane; v < nv; v += 64) {
      const int lo = 16 * v;
      if (lo >= c.mis && lo + 16 <= end) {
        *(uint4*)&s->win[lo] = *(const uint4*)(base + lo);
      } else {
        for (int k = 0; k < 16; ++k)
          if (lo + k >= c.mis && lo + k < end) s->win[lo + k] = base[lo + k];
      }
    }
    __syncthreads();
    scan_window(c, lane);
    __syncthreads();
    if (!c.dead && c.olen > 0) {
      const int tl = c.olen > 1 ? c.olen - 1 : c.olen;   // the last byte is erased
      Sink k;
      for (int i = 0; i < tl && k.commas <= 4; ++i) sink_feed(s, k, s->out[i], lane);
      const int ntok = sink_finish(s, k, lane);
      __syncthreads();
      if (lane == 0) lang_tags_hint(H, s, ntok, &np);
    }
  } else {
    __syncthreads();
  }
  if (hints) {
    const cld_hints_dev h = hints[doc];
    uint64_t cl = 0;
    if (h.content_language_len && (uint64_t)h.content_language_off < hint_text_bytes) {
      cl = hint_text_bytes - h.content_language_off;
      if (cl > h.content_language_len) cl = h.content_language_len;
    }
    if (cl) {
      // the text up to its first NUL through the copier, in pieces staged in s->out
      const uint8_t* t = hint_text + h.content_language_off;
      Sink k;
      int state = 1;
      bool stop = false;
      for (uint64_t p0 = 0; p0 < cl && !stop; p0 += kOutCap) {
        const int piece = (int)(cl - p0 < (uint64_t)kOutCap ? cl - p0 : (uint64_t)kOutCap);
        __syncthreads();
        for (int i = lane; i < piece; i += 64) s->out[i] = t[p0 + i];
        __syncthreads();
        for (int i = 0; i < piece; ++i) {
          const int ch = s->out[i];
          if (!ch || k.commas > 4) {
            stop = true;
            break;
          }
          const int o = copier_step(s, ch, &state);
          if (o >= 0) sink_feed(s, k, o, lane);
        }
      }
      if (state == 0) sink_feed(s, k, ',', lane);
      const int ntok = sink_finish(s, k, lane);
      __syncthreads();
      if (lane == 0) lang_tags_hint(H, s, ntok, &np);
    }
    if (lane == 0) {
      if (h.tld[0] && !h.tld[3]) {                     // SetCLDTLDHint: at most 3 bytes, lowercased
        int l = 0;
        for (; l < 3 && h.tld[l]; ++l) s->key[l] = (uint8_t)(h.tld[l] | 0x20);
        s->key[l] = 0;
        int16_t p1, p2;
        if (lookup(H.tld, s->key, &p1, &p2)) {
          merge_boost(s, &np, p1);
          merge_boost(s, &np, p2);
        }
      }
      if (h.encoding_hint != CLD_UNKNOWN_ENCODING && h.encoding_hint >= 0 && (uint32_t)h.encoding_hint < H.n_enc)
        merge_boost(s, &np, H.enc[h.encoding_hint]);   // SetCLDEncodingHint
      if (h.language_hint != (int32_t)H.unknown_language)   // SetCLDLanguageHint
        merge_boost(s, &np, (int16_t)((8u << 10) + (uint32_t)h.language_hint));
    }
  }
  if (lane == 0) {
    trim(s, &np, 4);
    if (priors14)
      for (int i = 0; i < kMaxPriors; ++i) priors14[(size_t)doc * kMaxPriors + i] = i < np ? s->pri[i] : (int16_t)0;
    if (boosts16 || special) {
      hint_boosts(H, s, np);
      uint32_t any = 0;
      for (int k = 0; k < 16; ++k) {
        any |= s->ring[k];
        if (boosts16) boosts16[(size_t)doc * 16 + k] = s->ring[k];
      }
      if (special)
        special[doc] = (uint8_t)((plain ? 0 : kSpecialHtml) | (any ? kSpecialPriors : 0) | cld_cflags_special(df));
    }
  }
}

}  // namespace hnt

extern "C" hipError_t cld_launch_apply_hints(const DevHints* H, const uint8_t* buf, const uint64_t* offs, int n,
                                             const cld_hints_dev* hints, const uint8_t* hint_text,
                                             uint64_t hint_text_bytes, int plain, const uint32_t* doc_flags,
                                             int16_t* priors14, uint32_t* boosts16, uint8_t* special, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(hnt::k_apply_hints, dim3(n), dim3(64), 0, s, *H, buf, offs, n, hints, hint_text, hint_text_bytes,
                     plain, doc_flags, priors14, boosts16, special);
  return hipGetLastError();
}
