// cld_valid_rule.h -- "interchange valid" UTF-8 (SpanInterchangeValid,
// compact_lang_det_impl.cc:72-80, over utf8acceptinterchange.h) as a closed
// form, shared by the host check (cld_valid_prefix_host) and the kernels
// (cld_valid.hip).
//
// With bytes outside the document read as 0, the byte at position p is an
// error position iff
//   * it starts no valid character: an ASCII control other than TAB LF FF CR
//     (NUL included), 7F, the leads C0 C1 F5-FF, or a lead C2-F4 whose
//     sequence is truncated, overlong, a surrogate, above U+10FFFF or one of
//     the code points the interchange set leaves out (U+0080-U+009F,
//     U+FDD0-U+FDEF, U+nFFFE, U+nFFFF); or
//   * it is a continuation byte 80-BF that no valid lead at p-1, p-2 or p-3
//     covers.
// The valid prefix of a document is its first error position (its length if
// it has none).  A byte's verdict depends on bytes p-3 .. p+3 only.
#ifndef CLD_VALID_RULE_H_
#define CLD_VALID_RULE_H_
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CLD_HD __host__ __device__ __forceinline__
#else
#define CLD_HD inline
#endif

namespace cld {
namespace valid {

// Length (1-4) of the interchange-valid character starting with byte b0 and
// followed by b1 b2 b3; 0 if none starts there (continuation bytes included).
CLD_HD uint32_t char_len(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
  if (b0 < 0x80) return (b0 >= 0x20 ? b0 != 0x7F : (b0 == 0x09 || b0 == 0x0A || b0 == 0x0C || b0 == 0x0D)) ? 1u : 0u;
  if (b0 < 0xC2 || b0 > 0xF4) return 0;
  const bool c2 = (b2 ^ 0x80) < 0x40, c3 = (b3 ^ 0x80) < 0x40;
  if (b0 < 0xE0) return (b1 >= (b0 == 0xC2 ? 0xA0u : 0x80u) && b1 <= 0xBF) ? 2u : 0u;
  if (b0 < 0xF0) {
    const uint32_t lo = b0 == 0xE0 ? 0xA0u : 0x80u, hi = b0 == 0xED ? 0x9Fu : 0xBFu;
    if (b1 < lo || b1 > hi || !c2) return 0;
    if (b0 == 0xEF && ((b1 == 0xB7 && b2 >= 0x90 && b2 <= 0xAF) || (b1 == 0xBF && b2 >= 0xBE))) return 0;
    return 3;
  }
  const uint32_t lo = b0 == 0xF0 ? 0x90u : 0x80u, hi = b0 == 0xF4 ? 0x8Fu : 0xBFu;
  if (b1 < lo || b1 > hi || !c2 || !c3) return 0;
  if ((b1 & 0x0F) == 0x0F && b2 == 0xBF && b3 >= 0xBE) return 0;
  return 4;
}

// The byte c at position p is an error position; l0 = char_len at p, l1 l2 l3
// = char_len at p-1, p-2, p-3 (0 before the document's start).
CLD_HD bool is_error(uint32_t c, uint32_t l0, uint32_t l1, uint32_t l2, uint32_t l3) {
  return (c ^ 0x80) < 0x40 ? !(l1 >= 2 || l2 >= 3 || l3 == 4) : l0 == 0;
}

}  // namespace valid
}  // namespace cld
#endif
