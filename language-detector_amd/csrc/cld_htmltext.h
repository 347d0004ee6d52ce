// cld_htmltext.h -- text(page) on the host (cld_html_text, cld_chunks_to_page):
// the host references of cld_htmltext.hip, written from the definition in
// cld_mi355x.h.
#ifndef CLD_HTMLTEXT_H_
#define CLD_HTMLTEXT_H_
#include <stddef.h>
#include <stdint.h>

#include "../../include/cld_mi355x.h"

namespace cld {

// The entity sections of the CLDT blob (CLDT_ENTITY_NAMES / _VALUES, CLDT_CP1252_FIX).
struct EntityView {
  const uint8_t* names = nullptr;      // u32 count, u32 offsets[count + 1], the sorted NUL-terminated names
  const int32_t* values = nullptr;     // one code point per name
  const uint32_t* cp1252 = nullptr;    // FixUnicodeValue's table for values below 0x100
  bool ok() const { return names && values && cp1252; }
};

// ScanToPossibleLetter (getonescriptspan.cc:150-203, 503-541) over text[0, len).
int html_scan_tag(const uint8_t* text, int64_t len);
// EntityToBuffer (:454-468) at text[0] == '&', len bytes available: the bytes
// consumed; *plen decoded bytes in dst[0..4) (0: undecodable, one byte consumed).
int html_read_entity(const EntityView& v, const uint8_t* text, int64_t len, uint8_t dst[4], int* plen);
// The tag at text[0] == '<' is a block tag (CLD_HTMLTEXT_BLOCK_TAGS).
bool html_block_tag(const uint8_t* text, int64_t len);

// text(page) of one page of L bytes into out[0, L) (and pos[0, L), nullable),
// padded; the counts are added to *st.  Returns text_len.
int64_t html_text_page(const EntityView& v, const uint8_t* page, int64_t L, uint32_t flags, uint8_t* out,
                       uint32_t* pos, cld_htmltext_status* st);

}  // namespace cld
#endif
