"""cld_scrub_utf8_host -- scrub(doc): every error position of the
interchange-valid check (csrc/cld_valid_rule.h) replaced by 0x20 -- against the
reference's own loop, byte for byte: call SpanInterchangeValid
(compact_lang_det_impl.cc:72-80, exported by oracle/_ref/librefcld2.so), set the
byte at the valid prefix to a space, call again, until the prefix is the length
(what compact_lang_det.h:73-79 and :161-173 tell a caller of the checked
entries to do).  Same inputs as the check's own host test.  No GPU."""
import ctypes

import numpy as np

import cld_amd
from test_gpu_corrupt import BAD
from test_valid_prefix_host import (code_point_docs, random_docs, ref_span, truncation_docs,   # noqa: F401 (fixture)
                                    two_byte_docs)


def ref_scrub(span, doc):
    """The reference's loop -> (bytes, number of bytes it changed).  It goes on from the byte
    after the prefix: the prefix is valid and ends on a character boundary."""
    d = bytearray(doc)
    n = len(d)
    at = changed = 0
    while at < n:
        tail = bytes(d[at:])
        vp = span(tail, len(tail))
        assert 0 <= vp <= len(tail)
        at += vp
        if at < n:
            d[at] = 0x20
            changed += 1
            at += 1
    return bytes(d), changed


def host_scrub(doc):
    out = ctypes.create_string_buffer(max(len(doc), 1))
    r = cld_amd.lib().cld_scrub_utf8_host(doc, len(doc), out)
    return out.raw[:len(doc)], r


def check(span, docs, what):
    for d in docs:
        want, changed = ref_scrub(span, d)
        got, replaced = host_scrub(d)
        assert got == want, "%s: %r: got %r, the reference's loop %r" % (what, d, got, want)
        # (a space is valid, so the loop never overwrites one: it changed `changed` bytes)
        assert replaced == changed == sum(a != b for a, b in zip(d, got)), (what, d)
        assert len(got) == len(d)
        if changed:
            assert span(got, len(got)) == len(got), (what, d)          # the output is interchange-valid
            assert host_scrub(got) == (got, 0), (what, d)              # and scrubbing it replaces nothing
            buf = ctypes.create_string_buffer(d, len(d))               # in place: out == doc
            assert cld_amd.lib().cld_scrub_utf8_host(buf, len(d), buf) == replaced and buf.raw[:len(d)] == want, \
                (what, d)


def test_every_code_point(ref_span):
    docs = code_point_docs()
    check(ref_span, docs, "code points")
    assert sum(host_scrub(d)[1] > 0 for d in docs) == 2175


def test_two_byte_strings(ref_span):
    check(ref_span, two_byte_docs(), "two-byte strings")


def test_truncations_and_bad_forms(ref_span):
    check(ref_span, truncation_docs() + BAD + [b"ok " + b + b" ok" for b in BAD] + [b""], "truncations / bad forms")
    assert host_scrub("xyé".encode()[:3]) == (b"xy ", 1)
    assert host_scrub(b"a\x00b") == (b"a b", 1)                        # NUL is an error position


def test_random_strings(ref_span):
    docs = random_docs()
    check(ref_span, docs, "random strings")
    # valid documents, and the ones that needed nothing, come back as they are (checked for all of them)
    for d in docs[:20000]:
        got, replaced = host_scrub(d)
        assert (got == d) == (replaced == 0)
        assert ref_span(got, len(got)) == len(got) and host_scrub(got) == (got, 0)
        buf = ctypes.create_string_buffer(d, len(d)) if d else ctypes.create_string_buffer(1)
        assert cld_amd.lib().cld_scrub_utf8_host(buf, len(d), buf) == replaced and buf.raw[:len(d)] == got


def test_replaced_counts_changed_bytes():
    """No error position holds a space, so `replaced` is the number of bytes that differ."""
    for d in random_docs(20000, seed=6):
        got, replaced = host_scrub(d)
        assert replaced == int(np.count_nonzero(np.frombuffer(d, np.uint8) != np.frombuffer(got, np.uint8)))


def test_python_binding():
    assert cld_amd.scrub_utf8_host(b"caf\xe9 ol\xc3\xa9") == (b"caf  ol\xc3\xa9", 1)
    assert cld_amd.scrub_utf8_host("plain") == (b"plain", 0)
    assert cld_amd.scrub_utf8_host(b"") == (b"", 0)


def test_errors():
    L = cld_amd.lib()
    out = ctypes.create_string_buffer(8)
    assert L.cld_scrub_utf8_host(None, 0, None) == 0
    assert L.cld_scrub_utf8_host(None, 3, out) == cld_amd.EINVAL
    assert L.cld_scrub_utf8_host(b"abc", 3, None) == cld_amd.EINVAL
    assert L.cld_scrub_utf8_host(b"x", 1 << 31, out) == cld_amd.EINVAL
