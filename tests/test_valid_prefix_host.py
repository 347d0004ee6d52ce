"""cld_valid_prefix_host -- the closed form of "interchange valid" UTF-8
(csrc/cld_valid_rule.h) -- against the reference's own SpanInterchangeValid
(compact_lang_det_impl.cc:72-80, exported by oracle/_ref/librefcld2.so),
exactly: every code point, every two-byte string with a high first byte,
truncations at a buffer end, the overlong / surrogate / too-large forms of the
corruption sweep, and 200 K seeded random strings weighted towards the bytes
at which a rule changes.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import cld_amd
import refcld
from test_gpu_corrupt import BAD   # the overlong, surrogate and too-large forms of the corruption sweep

SPAN_VALID = "_ZN4CLD220SpanInterchangeValidEPKci"
BOUNDARY = bytes.fromhex("00090A0B0C0D1F20417E7F808F909FA0AFB7BEBFC0C1C2DFE0E1ECEDEEEFF0F1F3F4F5F8FF")


def encode(cp):
    """UTF-8 form of any value 0..0x10FFFF, surrogates included."""
    if cp < 0x80:
        return bytes([cp])
    if cp < 0x800:
        return bytes([0xC0 | cp >> 6, 0x80 | cp & 0x3F])
    if cp < 0x10000:
        return bytes([0xE0 | cp >> 12, 0x80 | (cp >> 6) & 0x3F, 0x80 | cp & 0x3F])
    return bytes([0xF0 | cp >> 18, 0x80 | (cp >> 12) & 0x3F, 0x80 | (cp >> 6) & 0x3F, 0x80 | cp & 0x3F])


def rejected_code_point(cp):
    return (cp < 0x20 and cp not in (9, 10, 12, 13)) or 0x7F <= cp <= 0x9F or 0xD800 <= cp <= 0xDFFF or \
        0xFDD0 <= cp <= 0xFDEF or (cp & 0xFFFE) == 0xFFFE


def code_point_docs():
    return [b"ab" + encode(cp) + b"cd" for cp in range(0x110000)]


def two_byte_docs():
    return [bytes([a, b]) for a in range(0x80, 0x100) for b in range(0x100)]


def truncation_docs():
    out = []
    for ch in ("é", "中", "😀"):
        e = ch.encode()
        out += [b"xy" + e[:k] for k in range(1, len(e))] + [e[:k] for k in range(1, len(e))]
    return out


def random_docs(n=200_000, seed=5):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 25, n)
    uni = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    bnd = np.frombuffer(BOUNDARY, np.uint8)[rng.integers(0, len(BOUNDARY), int(lens.sum()))]
    kind = np.repeat(np.arange(n) % 3 == 0, lens)          # one third uniform bytes, two thirds boundary bytes
    data = np.where(kind, uni, bnd).astype(np.uint8).tobytes()
    ends = np.cumsum(lens)
    return [data[e - l:e] for e, l in zip(ends.tolist(), lens.tolist())]


@pytest.fixture(scope="module")
def ref_span():
    refcld.verify_build()
    lib = refcld.instance(os.environ["CLD_MI355X_TABLES"]).lib
    f = getattr(lib, SPAN_VALID)
    f.argtypes = [ctypes.c_char_p, ctypes.c_int]
    f.restype = ctypes.c_int
    return f


def ref_prefixes(ref_span, docs):
    return np.fromiter((ref_span(d, len(d)) for d in docs), dtype=np.int32, count=len(docs))


def host_prefixes(docs):
    f = cld_amd.lib().cld_valid_prefix_host
    return np.fromiter((f(d, len(d)) for d in docs), dtype=np.int32, count=len(docs))


def same(got, want, docs, what):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%s: %d of %d differ, first %r: got %d, reference %d" % (
        what, len(bad), len(docs), docs[bad[0]], got[bad[0]], want[bad[0]])


def test_every_code_point(ref_span):
    docs = code_point_docs()
    want = ref_prefixes(ref_span, docs)
    same(host_prefixes(docs), want, docs, "code points")
    rej = np.array([rejected_code_point(cp) for cp in range(0x110000)])
    assert int(rej.sum()) == 2175
    lens = np.array([len(d) for d in docs], dtype=np.int32)
    assert np.array_equal(want, np.where(rej, 2, lens))   # the rejected ones stop at the character's first byte


def test_two_byte_strings(ref_span):
    docs = two_byte_docs()
    same(host_prefixes(docs), ref_prefixes(ref_span, docs), docs, "two-byte strings")


def test_truncations_and_bad_forms(ref_span):
    docs = truncation_docs() + BAD + [b"ok " + b + b" ok" for b in BAD] + [b""]
    same(host_prefixes(docs), ref_prefixes(ref_span, docs), docs, "truncations / bad forms")
    assert cld_amd.valid_prefix_host("xyé".encode()[:3]) == 2   # a truncated character counts from its lead byte


def test_random_strings(ref_span):
    docs = random_docs()
    want = ref_prefixes(ref_span, docs)
    same(host_prefixes(docs), want, docs, "random strings")


def test_errors():
    assert cld_amd.lib().cld_valid_prefix_host(None, 0) == 0
    assert cld_amd.lib().cld_valid_prefix_host(None, 3) == cld_amd.EINVAL
    assert cld_amd.lib().cld_valid_prefix_host(b"x", 1 << 31) == cld_amd.EINVAL
