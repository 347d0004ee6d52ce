"""Cases and the model of the HTML text entries (cld_html_text*, cld_chunks_to_page*).

The model is a sequential walk written from the definition in cld_mi355x.h.  Its
tag lengths and entity values come from the oracle's cldo_scan_tag and
cldo_read_entity, which tests/test_html_hints.py pins to the reference; the
block-tag list is restated here.  Nothing under the reference tree is needed."""
import ctypes

import numpy as np

import cld_amd
import corpus

STAGE, CANDS, BLOCK_LF = cld_amd.HTMLTEXT_STAGE, cld_amd.HTMLTEXT_CANDS, cld_amd.HTMLTEXT_BLOCK_LF
BLOCK_TAGS = ("address article aside blockquote body br dd div dl dt fieldset figcaption figure footer form "
              "h1 h2 h3 h4 h5 h6 head header hr html li main nav ol option p pre script section style table tbody td "
              "tfoot th thead title tr ul").split()
ALNUM = frozenset(b"0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ")
LENGTHS = (0, 1, 63, 64, 65, STAGE - 1, STAGE, STAGE + 1, 4 * STAGE + 1)
FORMS = ("text", "amp", "lt", "onetag")


def utf8(v):
    """runetochar (getonescriptspan.cc:249-286)."""
    if v <= 0x7F:
        return bytes([v])
    if v <= 0x7FF:
        return bytes([0xC0 | v >> 6, 0x80 | v & 63])
    if v > 0x10FFFF:
        v = 0xFFFD
    if v <= 0xFFFF:
        return bytes([0xE0 | v >> 12, 0x80 | v >> 6 & 63, 0x80 | v & 63])
    return bytes([0xF0 | v >> 18, 0x80 | v >> 12 & 63, 0x80 | v >> 6 & 63, 0x80 | v & 63])


class Scanner:
    """The oracle's tag parser and entity reader over one page, without copying the page per call."""

    def __init__(self, oracle, page):
        self.keep = ctypes.create_string_buffer(bytes(page) + b"\0" * 16, len(page) + 16)
        self.base, self.L = ctypes.addressof(self.keep), len(page)
        self.scan = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int)(("cldo_scan_tag", oracle.lib))
        self.read = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int))(
            ("cldo_read_entity", oracle.lib))

    def tag(self, p):
        return int(self.scan(self.base + p, self.L - p))

    def entity(self, p):
        """-> (bytes consumed, decoded bytes): EntityToBuffer."""
        c = ctypes.c_int()
        v = int(self.read(self.base + p, self.L - p, ctypes.byref(c)))
        return (c.value, utf8(v)) if v > 0 else (1, b"")


def is_block_tag(page, p):
    q = p + 1
    if q < len(page) and page[q] == 0x2F:
        q += 1
    e = q
    while e < len(page) and page[e] in ALNUM:
        e += 1
    return bytes(page[q:e]).lower().decode("latin-1") in BLOCK_TAGS


def model_page(oracle, page, flags):
    """text(page) -> (text bytes, source positions, tags, entities, dropped)."""
    page = bytes(page)
    sc = Scanner(oracle, page)
    L, p = len(page), 0
    text, pos = bytearray(), []
    tags = entities = dropped = 0
    while p < L:
        c = page[p]
        if c == 0x3C:
            t = sc.tag(p)
            assert 1 <= t <= L - p
            text.append(0x0A if (flags & BLOCK_LF) and is_block_tag(page, p) else 0x20)
            pos.append(p)
            p += t
            tags += 1
        elif c == 0x26:
            tlen, dec = sc.entity(p)
            assert 1 <= tlen <= L - p and len(dec) <= tlen, "an entity that grows: %r" % page[p:p + 12]
            text += dec
            pos += [p + k for k in range(len(dec))]
            p += tlen
            entities += bool(dec)
            dropped += not dec
        else:
            text.append(c)
            pos.append(p)
            p += 1
    return bytes(text), pos, tags, entities, dropped


def model(oracle, buf, offs, flags):
    """The expected output of cld_html_text on a well-formed batch: out and pos indexed like buf (bytes before
    offsets[0] and after offsets[n] are None: not written), text_len, status."""
    buf = np.asarray(buf, np.uint8)
    offs = [int(x) for x in offs]
    size = max(len(buf), offs[-1])
    out, pos = np.zeros(size, np.uint8), np.zeros(size, np.uint32)
    text_len, st = [], [0, 0, 0, 0]
    sources = []
    for a, b in zip(offs[:-1], offs[1:]):
        L = b - a
        t, ps, tags, ents, drops = model_page(oracle, buf[a:b].tobytes(), flags)
        assert len(t) <= L and all(x < y for x, y in zip(ps, ps[1:])), "no growth; strictly increasing positions"
        out[a:b] = 0x20
        out[a:a + len(t)] = np.frombuffer(t, np.uint8)
        pos[a:b] = L
        pos[a:a + len(t)] = ps
        text_len.append(len(t))
        sources.append(ps)
        st = [st[0] + len(t), st[1] + tags, st[2] + ents, st[3] + drops]
    return {"out": out, "pos": pos, "text_len": np.array(text_len, np.int32).reshape(-1), "status": st, "sources": sources,
            "lo": offs[0], "hi": offs[-1]}


def check(got, want, what, pos=True):
    """got: dict of out / text_len / pos / status as the entries write them (missing keys are not compared)."""
    lo, hi = want["lo"], want["hi"]
    assert np.array_equal(got["out"][lo:hi], want["out"][lo:hi]), "%s: text or padding differ at %d" % (
        what, lo + int(np.flatnonzero(got["out"][lo:hi] != want["out"][lo:hi])[0]))
    if "text_len" in got:
        assert np.array_equal(np.asarray(got["text_len"]).reshape(-1), want["text_len"]), what + ": text_len"
    if pos and "pos" in got:
        assert np.array_equal(got["pos"][lo:hi], want["pos"][lo:hi]), "%s: pos differs at %d" % (
            what, lo + int(np.flatnonzero(got["pos"][lo:hi] != want["pos"][lo:hi])[0]))
    if "status" in got:
        have = status_list(got["status"])
        assert have == want["status"], "%s: status %s, expected %s" % (what, have, want["status"])


def status_list(st):
    """A cld_htmltext_status, as an HTMLTEXT_STATUS_DTYPE record or as its three 64-bit words ->
    [text_bytes, tags, entities, dropped]."""
    if getattr(st, "dtype", None) is not None and st.dtype.names:
        return [int(st[f]) for f in ("text_bytes", "tags", "entities", "dropped")]
    r = np.asarray(st, np.uint64)
    return [int(r[0]), int(r[1]), int(r[2]) & 0xFFFFFFFF, int(r[2]) >> 32]


def pack(pages, lead=0):
    """Pages back to back after `lead` bytes that belong to no page -> (buf, offs)."""
    offs = np.zeros(len(pages) + 1, np.uint64)
    offs[0] = lead
    np.cumsum([len(p) for p in pages], out=offs[1:])
    offs[1:] += np.uint64(lead)
    return np.frombuffer(b"\xEE" * lead + b"".join(pages), np.uint8).copy(), offs


def words(n, seed=0):
    """n bytes of lower-case words."""
    rng = np.random.default_rng(1000 + seed)
    out = bytearray()
    while len(out) < n:
        out += bytes(rng.integers(97, 123, size=int(rng.integers(2, 9))).astype(np.uint8)) + b" "
    return bytes(out[:n])


def form_page(L, form):
    if form == "text":
        return words(L, L)
    if form == "amp":
        return b"&" * L                    # every byte an undecodable '&': the text is empty
    if form == "lt":
        return b"<" * L                    # every byte a tag of one byte
    tag = b"<div class='x > y'>"
    k = max(L - len(tag), 0) // 2
    return (words(k, L) + tag + words(L, L + 1))[:L]


def length_pages():
    return [form_page(L, f) for L in LENGTHS for f in FORMS]


CONSTRUCTS = (b"<a href=x>", b'<a title="x > y <b> &amp;" id=q>', b"<!-- a <b> -- &lt; -->",
              b"<script type='t'>var s = '<b>&amp;</b>';</script>", b"<STYLE>p > a { x: '&lt;' }</style >")
ENTITIES = (b"&amp;", b"&#233;", b"&#x4e2d;", b"&eacute;", b"&#x1F600;", b"&bogus;", b"&lang", b"&amp")
CUT = (b"&am", b"&#", b"&#x", b"&#12", b"&", b"&#x4e2", b"&eacute")


def seam_pages():
    """Tags, quoted attributes, comments, script and style bodies and entities across a 64-byte window boundary
    and across byte STAGE of a page that is read in place; entities cut by the page end, each followed by a
    page that starts with what would have completed it."""
    pages = []
    for k, c in enumerate(CONSTRUCTS + ENTITIES):
        for at in (64, STAGE, 3 * 64):
            for cut in sorted({1, len(c) // 2, len(c) - 1}):
                pages.append(words(at - cut, k) + c + words(90, k + 1))
    for k, c in enumerate(CUT):
        pages += [words(40 + k, k) + c, b"p;234; " + words(30, k)]
        pages += [words(64 - len(c), k) + c, b"12;" + words(5, k)]          # ... at the end of a whole window
    return pages


def candidate_pages():
    """Exactly CANDS and CANDS + 1 candidates in a segment, a segment cut where a window would overflow it, and
    a reached tag that covers every candidate of the segment after its own."""
    return [b"<b>x" * CANDS + words(200, 1),
            b"<b>x" * (CANDS + 1) + words(200, 2),
            b"&lt;" * CANDS + b"<" + words(100, 3) + b"&amp;" * 40,
            b"<i>" * 400 + words(100, 4),
            b"<b>x" * (CANDS - 1) + b"<!-- " + b"<i>&amp;" * (CANDS // 2) + b" --> " + words(100, 5) + b"&amp;<b>",
            b"<b>x" * (CANDS - 1) + b"<script>" + b"<&" * (CANDS + 40) + b"</script>after &gt; it"]


def end_pages():
    """'<' as the last byte; a tag, a comment and a script left open at the end of a page, each followed by a
    page that begins with what would close it and must read as if alone; an empty page between two pages."""
    return [words(30, 1) + b"<",
            words(70, 2) + b"<div class='abc", b"' id=x> visible <b>one</b>",
            words(50, 3) + b"<!-- open comment", b"--> visible &amp; two",
            words(90, 4) + b"<script>var x = 1;", b"</script> visible three",
            words(STAGE + 10, 5) + b"<style>p {", b"}</style> visible four",
            b"", words(10, 6), b"", b"", b"<p>", b""]


def block_pages():
    """Every listed name in lower, upper and mixed case, as open and close tags and with attributes (one page per
    name and case, so that <script> and <style> swallow only their own page); near misses; names cut by the end."""
    pages = []
    for name in BLOCK_TAGS:
        mixed = "".join(c.upper() if i % 2 else c for i, c in enumerate(name))
        for nm in (name, name.upper(), mixed):
            n = nm.encode()
            pages.append(b"a<" + n + b">b</" + n + b">c<" + n + b" id='1'>d<" + n + b"/>e<" + n + b"\n>f")
    # (letters between the tags: the tag parser runs on over digits and spaces to the next possible letter)
    pages += [b"x<pre y>a<prefix>b<p1>c<h7>d<b>e<brx>f<br/>g< p>h</ p>i<p\t>j<P>k<h0>m<span>n<!-- p -->o<figcaptions>q<//p>u",
              b"text<di", b"text<p", b"text</", b"text</p", b"text<blockquot", b"text<blockquote", b"text<h", b"text<h1",
              b"<", b"<p", b"</p", b"<figcaption"]
    return pages


CORPUS_SEED = 0xC1D20007


def corpus_pages(n=64):
    """corpus.html(n, emoji=0.25).  Not the generator's default seed, 0xC1D20006: its page 38 holds "b&#1044;",
    a Latin letter whose script lookahead lands on an entity.  HTML mode sees the raw '&' there and keeps the
    decoded Cyrillic letter in the Latin span; the text has the letter itself and ends the span -- one of the two
    exactness details of HTML mode that the text cannot show (test_htmltext_reference.py), found by comparing the
    spans of the page and of its text.  With this seed the reference gives no difference on any of the 64 pages."""
    buf, offs = corpus.html(n, seed=CORPUS_SEED, emoji=0.25)
    return [bytes(buf[offs[i]:offs[i + 1]]) for i in range(n)]


def host_batches():
    """name -> pages: every case of the suite."""
    return {"lengths": length_pages(), "seams": seam_pages(), "candidates": candidate_pages(), "ends": end_pages(),
            "blocks": block_pages(), "corpus": corpus_pages()}


def expected_to_page(offs, pos, chunks, coffs, cap):
    """cld_chunks_to_page from its definition, in numpy / Python integers."""
    out = np.zeros(max(cap, 1), cld_amd.CHUNK_DTYPE)[:cap]
    offs = [int(x) for x in offs]
    for i in range(len(offs) - 1):
        a = offs[i]
        L = max(offs[i + 1] - a, 0)
        P = lambda x: min(int(pos[a + x]), L) if x < L else L
        for c in range(int(coffs[i]), min(int(coffs[i + 1]), cap)):
            o, b = int(chunks["offset"][c]), int(chunks["bytes"][c])
            s = min(max(o, 0), L)
            e = min(max(o + b, s), L)
            out[c] = (P(s), max(P(e) - P(s), 0), chunks["lang1"][c], 0)
    return out
