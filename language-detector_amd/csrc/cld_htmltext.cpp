// cld_htmltext.cpp -- the host reference of cld_html_text: the walk of
// cld_mi355x.h ("The text of HTML pages") over one page, sequential, with the
// tag automaton and the entity reader restated for the host (the device's are
// in cld_prims.hip; tests/test_htmltext_*.py pin this one to the oracle's and to
// the reference itself).
#include "cld_htmltext.h"

#include <string.h>

namespace cld {
namespace {

// A byte of text[0, len); NUL past the end.
struct View {
  const uint8_t* p;
  int64_t len;
  uint8_t at(int64_t i) const { return i >= 0 && i < len ? p[i] : 0; }
};

// The byte classes and transitions of the reference's tag parser
// (getonescriptspan.cc:150-203), as cld_prims.hip states them.
enum { TC_LT, TC_GT, TC_EX, TC_HY, TC_QU, TC_AP, TC_SL, TC_S, TC_C, TC_R, TC_I, TC_P, TC_T, TC_Y, TC_L, TC_E,
       TC_CR, TC_NL, TC_PL };
int tag_class(uint8_t c) {
  switch (c) {
    case '<': return TC_LT; case '>': return TC_GT; case '!': return TC_EX; case '-': return TC_HY;
    case '"': return TC_QU; case '\'': return TC_AP; case '/': return TC_SL; case '\n': case '\r': return TC_CR;
    case '&': case '@': case '`': return TC_PL;
    default: break;
  }
  if ((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z')) {
    switch (c | 0x20) {
      case 's': return TC_S; case 'c': return TC_C; case 'r': return TC_R; case 'i': return TC_I;
      case 'p': return TC_P; case 't': return TC_T; case 'y': return TC_Y; case 'l': return TC_L;
      case 'e': return TC_E; default: return TC_PL;
    }
  }
  return c >= 0xC0 ? TC_PL : TC_NL;
}
int tag_common(int k, int other) { return k == TC_LT ? 1 : k == TC_GT ? 2 : k == TC_QU ? 10 : k == TC_AP ? 11 : other; }
int tag_next(int s, int k) {
  switch (s) {
    case 0: case 2: return k == TC_LT ? 3 : ((k >= TC_S && k <= TC_E) || k == TC_PL) ? 0 : 2;
    case 3: return k == TC_EX ? 4 : k == TC_S ? 13 : (k == TC_HY || k == TC_SL) ? 9 : tag_common(k, 9);
    case 4: return k == TC_HY ? 5 : tag_common(k, 9);
    case 5: return k == TC_HY ? 6 : tag_common(k, 9);
    case 6: return k == TC_HY ? 7 : 6;
    case 7: return k == TC_HY ? 8 : 6;
    case 8: return k == TC_GT ? 2 : k == TC_HY ? 8 : 6;
    case 9: return tag_common(k, 9);
    case 10: return k == TC_QU ? 9 : k == TC_CR ? 12 : 10;
    case 11: return k == TC_AP ? 9 : k == TC_CR ? 12 : 11;
    case 12: return k == TC_LT ? 1 : k == TC_GT ? 2 : 12;
    case 13: return k == TC_C ? 14 : k == TC_T ? 28 : tag_common(k, 9);
    case 14: return k == TC_R ? 15 : tag_common(k, 9);
    case 15: return k == TC_I ? 16 : tag_common(k, 9);
    case 16: return k == TC_P ? 17 : tag_common(k, 9);
    case 17: return k == TC_T ? 18 : tag_common(k, 9);
    case 18: return (k == TC_GT || k == TC_CR || k == TC_NL) ? 19 : tag_common(k, 9);
    case 19: return k == TC_LT ? 20 : 19;
    case 20: return k == TC_SL ? 21 : 19;
    case 21: return k == TC_S ? 22 : (k == TC_CR || k == TC_NL) ? 21 : 19;
    case 22: return k == TC_C ? 23 : 19;
    case 23: return k == TC_R ? 24 : 19;
    case 24: return k == TC_I ? 25 : 19;
    case 25: return k == TC_P ? 26 : 19;
    case 26: return k == TC_T ? 27 : 19;
    case 27: return k == TC_GT ? 2 : 19;
    case 28: return k == TC_Y ? 29 : tag_common(k, 9);
    case 29: return k == TC_L ? 30 : tag_common(k, 9);
    case 30: return k == TC_E ? 31 : tag_common(k, 9);
    case 31: return (k == TC_GT || k == TC_CR || k == TC_NL) ? 32 : tag_common(k, 9);
    case 32: return k == TC_LT ? 33 : 32;
    case 33: return k == TC_SL ? 34 : 32;
    case 34: return k == TC_S ? 35 : (k == TC_CR || k == TC_NL) ? 34 : 32;
    case 35: return k == TC_T ? 36 : 32;
    case 36: return k == TC_Y ? 37 : 32;
    case 37: return k == TC_L ? 38 : 32;
    case 38: return k == TC_E ? 39 : 32;
    case 39: return k == TC_GT ? 2 : 32;
    default: return 1;
  }
}

bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
bool is_xdigit(uint8_t c) { return is_digit(c) || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F'); }
bool is_alnum(uint8_t c) { return is_digit(c) || ((c | 0x20) >= 'a' && (c | 0x20) <= 'z'); }

// FixUnicodeValue (fixunicodevalue.cc)
int32_t fix_unicode_value(const EntityView& v, int32_t uv) {
  const uint32_t u = (uint32_t)uv;
  if (u < 0x100) return (int32_t)v.cp1252[u];
  if (u < 0xD800) return uv;
  if ((u & ~0x0Fu) == 0xFDD0 || (u & ~0x0Fu) == 0xFDE0 || (u & 0xFFFEu) == 0xFFFE) return 0xFFFD;
  if (0xE000 <= u && u <= 0x10FFFF) return uv;
  return 0xFFFD;
}

// strto32_base10 / _base16 (getonescriptspan.cc:325-391), quirks kept
int32_t entity_number(const EntityView& v, const View& d, int64_t p, int64_t lim, bool hex, int64_t* endp) {
  *endp = p;
  while (p < lim && d.at(p) == '0') ++p;
  if (p == lim || !(hex ? is_xdigit(d.at(p)) : is_digit(d.at(p)))) return -1;
  int64_t e = p;
  while (e < lim && (hex ? is_xdigit(d.at(e)) : is_digit(d.at(e)))) ++e;
  *endp = e;
  const int64_t n = e - p;
  bool fits;
  if (hex) {
    fits = n < 8 || (n == 8 && d.at(p) < '8');
  } else {
    fits = n < 9;
    if (n == 10) fits = memcmp(d.p + p, "2147483647", 10) <= 0;
  }
  if (!fits) return 0xFFFD;
  int32_t val = 0;
  for (; p < e; ++p) {
    const uint8_t c = d.at(p);
    val = hex ? (int32_t)(((uint32_t)val << 4) + (uint32_t)(is_digit(c) ? c - '0' : (c | 0x20) - 'a' + 10))
              : val * 10 + (c - '0');
  }
  return fix_unicode_value(v, val);
}

// LookupEntity (:292-300): binary search of the sorted entity names
int32_t lookup_entity(const EntityView& v, const View& d, int64_t p, int64_t n) {
  if (n >= 16) return -1;
  uint32_t cnt;
  memcpy(&cnt, v.names, 4);
  const uint8_t* off = v.names + 4;
  const char* base = reinterpret_cast<const char*>(v.names + 4 + 4 * ((size_t)cnt + 1));
  uint32_t lo = 0, hi = cnt;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    uint32_t o;
    memcpy(&o, off + 4 * (size_t)mid, 4);
    const char* s = base + o;
    int c = 0;
    for (int64_t i = 0;; ++i) {                      // strcmp(name, key)
      const int a = (uint8_t)s[i], b = i < n ? d.at(p + i) : 0;
      if (a != b || a == 0) { c = a - b; break; }
    }
    if (c < 0) lo = mid + 1;
    else if (c > 0) hi = mid;
    else return v.values[mid];
  }
  return -1;
}

// ReadEntity (:393-451) at d[0] == '&'
int32_t read_entity(const EntityView& v, const View& d, int64_t* consumed) {
  const int64_t end = d.len;
  if (end == 0 || d.at(0) != '&') { *consumed = 0; return -1; }
  *consumed = 1;
  const int64_t st = 1;
  int64_t en;
  int32_t val;
  if (st < end && d.at(st) == '#') {
    if (st + 2 >= end) return -1;
    const uint8_t x = d.at(st + 1);
    val = (x == 'x' || x == 'X') ? entity_number(v, d, st + 2, end, true, &en) : entity_number(v, d, st + 1, end, false, &en);
    if (val == -1 || en > end) return -1;
  } else {
    for (en = st; en < end && is_alnum(d.at(en)); ++en) {}
    val = lookup_entity(v, d, st, en - st);
    if (val < 0) return -1;
    if (val >= 256 && !(en < end && d.at(en) == ';')) return -1;
  }
  if (en < end && d.at(en) == ';') ++en;
  *consumed = en - 0;
  return val;
}

// runetochar (:249-286)
int rune_to_utf8(uint8_t* s, uint32_t c) {
  if (c <= 0x7F) { s[0] = (uint8_t)c; return 1; }
  if (c <= 0x7FF) { s[0] = (uint8_t)(0xC0 | (c >> 6)); s[1] = (uint8_t)(0x80 | (c & 0x3F)); return 2; }
  if (c > 0x10FFFF) c = 0xFFFD;
  if (c <= 0xFFFF) {
    s[0] = (uint8_t)(0xE0 | (c >> 12)); s[1] = (uint8_t)(0x80 | ((c >> 6) & 0x3F)); s[2] = (uint8_t)(0x80 | (c & 0x3F));
    return 3;
  }
  s[0] = (uint8_t)(0xF0 | (c >> 18)); s[1] = (uint8_t)(0x80 | ((c >> 12) & 0x3F));
  s[2] = (uint8_t)(0x80 | ((c >> 6) & 0x3F)); s[3] = (uint8_t)(0x80 | (c & 0x3F));
  return 4;
}

}  // namespace

int html_scan_tag(const uint8_t* text, int64_t len) {
  const View d{text, len};
  int64_t src = 0;
  int e = 0, st = 0;
  while (src < len) {
    e = tag_next(st, tag_class(d.at(src++)));
    if (e <= 1) { --src; break; }
    st = e;
  }
  if (src >= len) return (int)len;
  if (e != 0 && e != 2) {
    int64_t off = src - 1;
    while (0 < off && d.at(off) != '<') --off;
    return (int)(off + 1);
  }
  return (int)src;
}

int html_read_entity(const EntityView& v, const uint8_t* text, int64_t len, uint8_t dst[4], int* plen) {
  int64_t tlen = 0;
  const int32_t val = read_entity(v, View{text, len}, &tlen);
  if (val > 0) {
    *plen = rune_to_utf8(dst, (uint32_t)val);
    return (int)tlen;
  }
  *plen = 0;
  return 1;
}

bool html_block_tag(const uint8_t* text, int64_t len) {
  int64_t p = 1;
  if (p < len && text[p] == '/') ++p;
  char name[12];
  int n = 0;
  for (; p < len && is_alnum(text[p]); ++p) {
    if (n == 11) return false;                       // (longer than every listed name)
    name[n++] = (char)(text[p] | (is_digit(text[p]) ? 0 : 0x20));
  }
  if (n == 0) return false;
  name[n] = 0;
  // the list, one name after the other between single spaces
  static const char kList[] = " " CLD_HTMLTEXT_BLOCK_TAGS " ";
  for (const char* s = kList; (s = strstr(s, name)) != nullptr; ++s)
    if (s[-1] == ' ' && s[n] == ' ') return true;
  return false;
}

int64_t html_text_page(const EntityView& v, const uint8_t* page, int64_t L, uint32_t flags, uint8_t* out,
                       uint32_t* pos, cld_htmltext_status* st) {
  int64_t q = 0;
  auto put = [&](uint8_t b, int64_t src) {             // (never past the page's range: "no growth")
    if (q < L) {
      out[q] = b;
      if (pos) pos[q] = (uint32_t)src;
    }
    ++q;
  };
  for (int64_t p = 0; p < L;) {
    const uint8_t c = page[p];
    if (c == '<') {
      const int t = html_scan_tag(page + p, L - p);
      put(((flags & CLD_HTMLTEXT_BLOCK_LF) && html_block_tag(page + p, L - p)) ? 0x0A : 0x20, p);
      p += t > 0 ? t : 1;
      ++st->tags;
    } else if (c == '&') {
      uint8_t dec[4];
      int plen = 0;
      const int tlen = html_read_entity(v, page + p, L - p, dec, &plen);
      for (int k = 0; k < plen; ++k) put(dec[k], p + k);
      p += tlen;
      if (plen > 0) ++st->entities;
      else ++st->dropped;
    } else {
      put(c, p);
      ++p;
    }
  }
  const int64_t text_len = q < L ? q : L;
  for (q = text_len; q < L; ++q) {
    out[q] = 0x20;
    if (pos) pos[q] = (uint32_t)L;
  }
  st->text_bytes += (uint64_t)text_len;
  return text_len;
}

}  // namespace cld
