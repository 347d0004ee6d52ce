"""cld_html_text and cld_chunks_to_page, the host references (no GPU), against the
model of htmltext_cases.py: a sequential walk written from the definition in
cld_mi355x.h over the oracle's tag parser and entity reader.  Everything is
integers and every comparison is exact."""
import numpy as np
import pytest

import cld_amd
import htmltext_cases as hc

FLAGS = (0, hc.BLOCK_LF)
BATCHES = hc.host_batches()


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_host_entry_equals_model(oracle, name, flags):
    """Text, text_len, pos, status and padding; bytes outside [offsets[0], offsets[n]) stay as they were; the
    model itself asserts no growth and strictly increasing positions on every page."""
    buf, offs = hc.pack(BATCHES[name], lead=37)
    buf = np.concatenate([buf, np.full(11, 0xEE, np.uint8)])          # bytes after the last page
    want = hc.model(oracle, buf, offs, flags)
    got = cld_amd.html_text(buf, offs, flags, pos=True)
    hc.check(got, want, "%s, flags %d" % (name, flags))
    lo, hi = want["lo"], want["hi"]
    for f in ("out", "pos"):
        assert not got[f][:lo].any() and not got[f][hi:].any(), f + " was written outside the pages"
    assert (got["text_len"] <= np.diff(offs.astype(np.int64))).all()
    assert want["status"][0] == int(want["text_len"].sum())
    # without pos, the same text
    again = cld_amd.html_text(buf, offs, flags)
    assert "pos" not in again and np.array_equal(again["out"], got["out"])


def test_cases_are_what_they_claim(oracle):
    m = {name: hc.model(oracle, *hc.pack(pages), hc.BLOCK_LF) for name, pages in BATCHES.items()}
    tl = m["lengths"]["text_len"].reshape(len(hc.LENGTHS), len(hc.FORMS))
    L = np.array(hc.LENGTHS)
    assert (tl[:, 0] == L).all() and (tl[:, 1] == 0).all() and (tl[:, 2] == L).all(), "all text, all '&', all '<'"
    assert m["lengths"]["status"][3] == int(L.sum()) and m["lengths"]["status"][1] >= int(L.sum())
    assert m["corpus"]["status"][2] > 200 and m["corpus"]["status"][3] > 40 and m["corpus"]["status"][1] > 500
    # every block page has its five separators as LF, every near miss as space
    buf, offs = hc.pack(BATCHES["blocks"])
    out = m["blocks"]["out"]
    for i in range(3 * len(hc.BLOCK_TAGS)):
        t = bytes(out[int(offs[i]):int(offs[i]) + int(m["blocks"]["text_len"][i])])
        name = hc.BLOCK_TAGS[i // 3]
        if name in ("script", "style"):
            assert t.startswith(b"a\n") and b" " not in t, (name, t)
        else:
            assert t == b"a\nb\nc\nd\ne\nf", (name, t)
    i = 3 * len(hc.BLOCK_TAGS)
    t = bytes(out[int(offs[i]):int(offs[i]) + int(m["blocks"]["text_len"][i])])
    assert t == b"x\na b c d e f\ng h i\nj\nk m n o q u", t
    ends = {bytes(p): bytes(out[int(offs[k]):int(offs[k]) + int(m["blocks"]["text_len"][k])])
            for k, p in enumerate(BATCHES["blocks"]) if k > i}
    assert ends[b"text<p"] == ends[b"text</p"] == ends[b"text<blockquote"] == ends[b"text<h1"] == b"text\n"
    assert ends[b"text<di"] == ends[b"text</"] == ends[b"text<blockquot"] == ends[b"text<h"] == b"text "
    assert ends[b"<p"] == ends[b"</p"] == ends[b"<figcaption"] == b"\n" and ends[b"<"] == b" "
    # the page after an open construct reads as if alone
    buf, offs = hc.pack(BATCHES["ends"])
    for k, p in enumerate(BATCHES["ends"]):
        alone = hc.model(oracle, *hc.pack([p]), hc.BLOCK_LF)
        a = int(offs[k])
        assert np.array_equal(m["ends"]["out"][a:a + len(p)], alone["out"])
    assert sum(b"visible" in bytes(m["ends"]["out"][int(a):int(b)]) for a, b in zip(offs[:-1], offs[1:])) == 4
    # segments: the counts the candidate pages are built for
    cands = [sum(1 for b in p if b in b"<&") for p in BATCHES["candidates"]]
    assert cands[0] == hc.CANDS and cands[1] == hc.CANDS + 1 and cands[3] == 400 and cands[4] > 2 * hc.CANDS


ENTITY_NAMES = 32                                    # cldt_format.h CLDT_ENTITY_NAMES


def test_no_entity_grows(oracle, blob):
    """plen <= tlen for every entity the oracle's reader decodes -- every name of the table's entity section
    with and without ';', the numeric forms at 1-10 decimal and 1-8 hex digits with their boundary values:
    the page-aligned layout rests on it."""
    names = [s.encode() for s in blob.strings(ENTITY_NAMES)]
    assert len(names) > 200
    forms = []
    for n in names:
        forms += [b"&" + n + b";", b"&" + n, b"&" + n + b" ", b"&" + n + b";x"]
    dec = ["9", "10", "99", "127", "128", "159", "160", "255", "256", "999", "2047", "2048", "9999", "55295", "55296",
           "57343", "57344", "65533", "65535", "65536", "99999", "999999", "1114111", "1114112", "9999999", "99999999",
           "999999999", "2147483647", "2147483648", "4294967295", "9999999999", "0", "00009", "0000000065"]
    hexd = ["9", "A", "7F", "80", "9F", "A0", "FF", "100", "7FF", "800", "FFF", "D7FF", "D800", "DFFF", "E000", "FFFD",
            "FFFE", "FFFF", "10000", "FFFFF", "10FFFF", "110000", "FFFFFF", "7FFFFFFF", "80000000", "FFFFFFFF", "0", "0009"]
    for d in dec:
        forms += [b"&#" + d.encode(), b"&#" + d.encode() + b";"]
    for h in hexd:
        forms += [b"&#x" + h.encode(), b"&#X" + h.lower().encode() + b";"]
    for k in range(1, 11):
        forms += [b"&#" + b"1" * k, b"&#" + b"9" * k + b";"]
    for k in range(1, 9):
        forms += [b"&#x" + b"1" * k, b"&#xF" + b"f" * (k - 1) + b";"]
    decoded, shortest = 0, {}
    for f in forms:
        tlen, d = hc.Scanner(oracle, f).entity(0)
        assert 1 <= tlen <= len(f) and len(d) <= tlen, "%r: %d bytes from %d" % (f, len(d), tlen)
        if d:
            decoded += 1
            shortest[len(d)] = min(shortest.get(len(d), 99), tlen)
    assert decoded > 500
    assert shortest == {1: 3, 2: 4, 3: 4, 4: 7}, shortest          # "&#9", "&lt" / "&#xA0", "&ni;", "&#65536"


def test_tiling_text_chunks_tile_the_page(oracle):
    """Pieces that tile the text map to pieces that tile the page, and no piece starts inside a tag or entity."""
    pages = hc.corpus_pages(8)
    buf, offs = hc.pack(pages, lead=3)
    m = hc.model(oracle, buf, offs, hc.BLOCK_LF)
    got = cld_amd.html_text(buf, offs, hc.BLOCK_LF, pos=True)
    rng = np.random.default_rng(2)
    chunks, coffs = [], [0]
    for i, p in enumerate(pages):
        cuts = sorted({0, len(p), *[int(x) for x in rng.integers(0, len(p) + 1, size=12)]})
        chunks += [(s, e - s, i, 0) for s, e in zip(cuts, cuts[1:])]
        coffs.append(len(chunks))
    ch = np.array(chunks, cld_amd.CHUNK_DTYPE)
    out = cld_amd.chunks_to_page(offs, got["pos"], ch, np.array(coffs, np.uint64))
    for i, p in enumerate(pages):
        v = out[coffs[i]:coffs[i + 1]]
        assert int(v["offset"][0]) == 0 and int(v["offset"][-1] + v["bytes"][-1]) == len(p)
        assert (v["offset"][1:] == v["offset"][:-1] + v["bytes"][:-1]).all()
        legal = set(m["sources"][i]) | {len(p)}
        assert all(int(o) in legal for o in v["offset"]), "a chunk starts inside a tag or an entity"
