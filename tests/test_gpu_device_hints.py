"""HTML mode and CLDHints on the device-resident interface: ApplyHints as a GPU
kernel (cld_hints.hip; cld_hint_boosts_device) against the host hint code
(cld_hint_priors, itself pinned to the reference's hint code by
test_html_hints.py), and cld_detect_batch_device_hints against
cld_detect_batch_ex and the reference CLD2 (oracle/_ref/librefcld2.so).

The device entries run in one child process (device_hints_child.py) in which
torch initialises the GPU first; it leaves its outputs in an .npz file and the
tests here assert on that.  Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import corpus
import refcld
from test_gpu_html_hints import random_hints
from test_gpu_parity import assert_same
from test_html_hints import hint_cases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WINDOW = 8192       # the lang= scan reads the first 8 KB (compact_lang_det_impl.cc:1596-1611)
TILE = 64           # cld_hints.hip kTile: bytes per ballot
BAD_LEADS = (0xC0, 0xC1, 0xF5, 0xF6, 0xF7)


def tag_at(pos, tag=b'<p lang="de">', tail=b" der Hund lief die Strasse entlang"):
    """A page whose only tag starts at byte pos."""
    return b"a" * pos + tag + tail


def edge_pages():
    t = b'<p lang="de">'
    pages = [b"", b"x", b"<", b"<html lang=fr", b'<html lang="fr"', b'<html lang="fr">', b">", b"&", b"<<", b"<&", b"<>"]
    # the 8192 boundary: the tag's '>' at 8191 (inside), 8192 and 8193 (not a tag), a tag starting at 8190,
    # a 20 KB page whose only lang= lies past 8 KB
    pages += [tag_at(k - (len(t) - 1)) for k in (WINDOW - 1, WINDOW, WINDOW + 1)]
    pages += [tag_at(WINDOW - 2), tag_at(WINDOW - 1, b"<"), b"le chat noir " * 800 + t + b"le chat noir " * 800]
    assert len(pages[-1]) > 20000
    # the terminator of an earlier tag right at the bound: '<' of the next tag at 8191 ends it, at 8192 does not
    pages += [b"a" * (k - len(t) + 1) + t[:-1] + b"<b>x" for k in (WINDOW - 1, WINDOW)]
    # tile edges
    pages += [tag_at(k) for k in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 4095, 4096, 4097)]
    pages += [b"a" * (TILE - 5) + b'<p lang="fr"><b lang="de">x',            # a tag across a tile edge, one after it
              b"a" * (TILE - 1) + b"<" + b"b" * 200 + b' lang="fr">',          # terminator three tiles on
              b"a" * 63 + b'<p lang="es">' + b"b" * 38 + b'<p lang="it">' + b"c" * 51 + b'<p lang="pt">']
    # tag counts and sizes
    pages += [b"<b>x</b>" * 100 + t + b"<i>y</i>" * 100,
              b"".join(b'<p lang="%s">' % l for l in (b"en", b"fr") * 40),
              b"<" * 1500 + t, b"<a" * 1100 + b'<p lang="fr">', b"&<" * 1100 + b'<p lang="fr">',
              b'<p title="' + b"x" * 8000 + b'" lang="fr">' + b" texte",
              b"<p " + b"x" * 9000 + b' lang="fr">',
              b'<p lang="' + b"x" * 8000 + b'"><b lang="fr">',                # a window-long value
              b'<p lang="' + b"x" * 100 + b'"><b lang="' + b"x" * 50 + b'"><i lang="' + b"x" * 100 + b'y">',
              b'<p lang="' + b"y" * 4000 + b'"><b lang="' + b"y" * 3900 + b'z"><i lang="fr">']
    assert pages[-8].count(b"<") > 1024
    # the six skipped tag kinds, each carrying a lang=
    pages += [b'<!-- lang="fr" -->', b'<font lang="fr">', b'<script lang="fr">', b'<link lang="fr">', b'<img lang="fr">',
              b'<a lang="fr">', b'<FONT LANG="fr">', b'< font lang="fr">', b'<\'a lang="fr">', b'<fonts lang="fr">',
              b'<abbr lang="fr">', b'<!- lang="fr">']
    # letter case, quoting and spacing
    pages += [b'<HTML LANG="FR">', b'<Html LaNg="Fr">', b"<html lang='fr'>", b"<html lang=fr>", b'<html lang ="fr">',
              b'<html lang= "fr">', b'<html lang  =  "fr" >', b'<html lang="fr\'>', b'<p title="a=b" lang="fr">',
              b'<p lang="f=r">', b'<p title="x>y" lang="fr">', b'<p title="x\\"y" lang="fr">', b'<p title="x\\" lang="fr">',
              b'<p title=\'it"s\' lang="fr">', b'<p title="unterminated lang="fr">', b'<p lang="">', b'<p lang=" ">',
              b'<p lang="fr" lang="de">', b'<p slang="fr">', b'<p lang="FR-ca; q=1">', b'<p lang="\xc3\xa9,fr">']
    # <meta> forms, :lang
    pages += [b'<meta http-equiv="Content-Language" content="de">', b'<meta content="de" http-equiv="Content-Language">',
              b'<meta http-equiv=content-language content="de">', b'<meta name="language" content="de">',
              b"<meta name=language content='de'>", b'<meta name="dc.language" content="de">',
              b'<meta name="DC.Language" content="de">', b'<meta name="keywords" content="de">',
              b'<meta http-equiv="Content-Language" x="1" content="de" content="it">',
              b'<p http-equiv="Content-Language" content="de">', b'<p xml:lang="es">', b'<p xml:lang=\'es,pt\'>']
    # repeats, the substring drop, commas and token length, hyphens
    pages += [b'<html lang="fr"><p lang="fr">', b'<html lang="xfr"><p lang="fr">', b'<html lang="fr"><p lang="xfr">',
              b'<html lang="en,fr,de,es,it">', b'<html lang="en,fr,de,es,it,pt">', b'<html lang="en,,fr">', b'<html lang=",">',
              b"".join(b'<p lang="%s">' % l for l in (b"en", b"fr", b"de", b"es", b"it", b"pt", b"nl")),
              b"".join(b'<p lang="%s">' % l for l in (b"en", b"fr", b"de", b"es", b"it")),
              b"".join(b'<p lang="%s">' % l for l in (b"en", b"fr", b"de", b"es", b"it", b"pt")),
              b'<html lang="abcdefghijklmnopq,fr">', b'<html lang="abcdefghijklmnop,fr">', b'<html lang="zh-hant">',
              b'<html lang="sr-latn">', b'<html lang="x-klingon">', b'<html lang="zh-tw,zh-cn">', b'<html lang="nb-no-x">']
    return pages


def language_id(gpu, code):
    return [i for i in range(300) if gpu.language_code(i) == code][0]


def edge_batch(gpu):
    """(pages, hint records, hint text, the host Hints each record stands for)."""
    pages = edge_pages()
    n_pages = len(pages)
    indonesian, chinese = language_id(gpu, "id"), language_id(gpu, "zh")
    made = [(None, None, gpu.UNKNOWN_ENCODING, gpu.UNKNOWN_LANGUAGE)] * n_pages
    made += [("fr," + "x" * 297, None, 23, 26), ("en," * 100, None, 23, 26), ("x" * 300, None, 23, 26),
             ("en,fr,de,es", None, 23, 26), ("en,fr,de,es,it", None, 23, 26), ("EN-gb; fr", None, 23, 26),
             (None, "ID", 23, 26), (None, "abcd", 23, 26), (None, "fr", 23, 26), (None, "x", 23, 26),
             (None, None, 23, indonesian), ("ms", None, 23, indonesian), (None, "id", 23, indonesian),
             (None, None, 23, chinese), ("zh-tw", None, 23, chinese), (None, "tw", 23, chinese),
             (None, None, 0, 26), (None, None, 74, 26), (None, None, 75, 26), (None, None, 1000, 26),
             (None, None, -1, 26), (None, None, 23, 1023), (None, None, 23, 1024), (None, None, 23, 70000),
             (None, None, 23, -1), ("fr", "fr", 16, language_id(gpu, "fr"))]
    hints = [gpu.Hints.make(*m) for m in made]
    # the last two hinted entries also sit on pages of their own
    pages = pages + [b""] * (len(made) - n_pages - 2) + [b'<html lang="de">', b'<html lang="fr">']
    rec, text = gpu.pack_hints(hints, len(hints))
    # by hand: a range reaching past the text, one starting past it, an embedded NUL
    text = bytearray(text.tobytes()) + b"de\0frxx" + b"it"
    extra = np.zeros(3, dtype=gpu.HINTS_DEV_DTYPE)
    extra["encoding_hint"], extra["language_hint"] = gpu.UNKNOWN_ENCODING, gpu.UNKNOWN_LANGUAGE
    extra["content_language_off"] = [len(text) - 2, len(text) + 5, len(text) - 9]
    extra["content_language_len"] = [10, 4, 5]
    hints += [gpu.Hints.make("it"), gpu.Hints.make(), gpu.Hints.make("de")]
    pages += [b"", b"", b""]
    return pages, np.concatenate([rec, extra]), np.frombuffer(bytes(text), np.uint8), hints


def host_rows(gpu, pages, html, hints=None):
    """cld_hint_priors per document -> (priors [n, 14], boosts [n, 16])."""
    pri = np.zeros((len(pages), 14), np.int16)
    boo = np.zeros((len(pages), 16), np.uint32)
    for i, d in enumerate(pages):
        p, boo[i] = gpu.hint_priors(d, html=html, hints=None if hints is None else hints[i])
        pri[i, :len(p)] = p
    return pri, boo


def docs_of(buf, offs):
    return [bytes(buf[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)]


@pytest.fixture(scope="module")
def inputs(gpu):
    """Every batch the child runs, with what the parent needs to judge it."""
    calls, want = {}, {}

    def kernel_call(key, pages, plain, rec=None, text=None, hints=None):
        calls[key + "_buf"], calls[key + "_offs"] = gpu.pack(pages)
        calls[key + "_plain"] = np.uint8(plain)
        if rec is not None:
            calls[key + "_rec"], calls[key + "_text"] = rec, text
        want[key] = (pages, not plain, hints)

    cases = hint_cases(8, 3000)
    for key, sel in (("k0", [c for c in cases if c[0]]), ("k1", [c for c in cases if not c[0]])):
        hints = [gpu.Hints.make(cl or None, tld or None, enc, lang) for _, cl, tld, enc, lang in sel]
        kernel_call(key, [c[0] for c in sel], key == "k1", *gpu.pack_hints(hints, len(hints)), hints)
    hb, ho = corpus.html(1500, seed=21)
    html_pages = docs_of(hb, ho)
    kernel_call("k2", html_pages, False)                               # d_hints = NULL
    pages, rec, text, hints = edge_batch(gpu)
    kernel_call("k3", pages, False, rec, text, hints)
    kernel_call("k4", pages, True, rec, text, hints)                   # is_plain_text = 1 on the same pages: no scan
    kernel_call("k5", pages, False)                                    # ... and without their hints
    # end to end
    h_html = random_hints(gpu, len(html_pages), seed=51)
    cb, co = corpus.c2(5000)
    h_c2 = random_hints(gpu, 5000, seed=52)
    calls["d0_buf"], calls["d0_offs"], calls["d0_flags"] = hb, ho, np.uint32(gpu.FLAG_HTML)
    calls["d0_rec"], calls["d0_text"] = gpu.pack_hints(h_html, len(h_html))
    calls["d1s_buf"], calls["d1s_offs"], calls["d1s_flags"] = cb, co, np.uint32(0)          # on a torch stream
    calls["d1s_rec"], calls["d1s_text"] = gpu.pack_hints(h_c2, 5000)
    c4b, c4o = corpus.c4(5000)
    calls["d2_buf"], calls["d2_offs"], calls["d2_flags"] = c4b, c4o, np.uint32(0)            # d_hints = NULL, flags 0
    calls["p0_buf"], calls["p0_offs"] = c4b, c4o
    calls["d3_buf"], calls["d3_offs"] = gpu.pack(html_pages[:300])
    calls["d3_flags"] = np.uint32(gpu.FLAG_HTML | gpu.FLAG_BEST_EFFORT)
    calls["d4_buf"], calls["d4_offs"], calls["d4_flags"] = hb, ho, np.uint32(gpu.FLAG_HTML)  # HTML without hints
    return calls, want, {"html": (hb, ho, h_html), "c2": (cb, co, h_c2)}


@pytest.fixture(scope="module")
def child(inputs, tmp_path_factory):
    """The child's outputs; a child that ends abnormally fails every test of the module, and nothing else is started."""
    d = tmp_path_factory.mktemp("device_hints")
    np.savez(d / "in.npz", **inputs[0])
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    r = subprocess.run([sys.executable, os.path.join(HERE, "device_hints_child.py"), str(d / "in.npz"), str(d / "out.npz")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "device_hints_child.py ended with %d: %s" % (r.returncode, r.stderr[-3000:])
    return np.load(d / "out.npz")


def assert_rows(gpu, child, inputs, key):
    pages, html, hints = inputs[1][key]
    want_p, want_b = host_rows(gpu, pages, html, hints)
    got_p, got_b = child[key + "_priors"], child[key + "_boosts"]
    bad = np.nonzero((got_p != want_p).any(axis=1) | (got_b != want_b).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d documents differ; first %d (%r): priors %s / host %s, boosts %s / host %s" % (
        key, len(bad), len(pages), bad[0], pages[bad[0]][:80], got_p[bad[0]], want_p[bad[0]], got_b[bad[0]], want_b[bad[0]])
    return want_p, want_b


def test_kernel_equals_host_on_hint_cases(gpu, child, inputs):
    """The 3000 cases test_hint_priors_match_reference pins to the reference (HTML half, plain half)."""
    with_prior = 0
    for key in ("k0", "k1"):
        want_p, _ = assert_rows(gpu, child, inputs, key)
        with_prior += int((want_p != 0).any(axis=1).sum())
        assert (want_p[:, 4:] == 0).all()                              # trimmed to 4
    assert with_prior > 1500


def test_kernel_equals_host_on_html_corpus(gpu, child, inputs):
    _, want_b = assert_rows(gpu, child, inputs, "k2")
    assert (want_b != 0).any(axis=1).sum() > 1500 // 2                 # lang= attributes became priors


def test_kernel_equals_host_on_edges(gpu, child, inputs):
    pages, _, hints = inputs[1]["k3"]
    want_p, want_b = assert_rows(gpu, child, inputs, "k3")
    have = {bytes(p): (want_p[i], want_b[i]) for i, p in enumerate(pages) if p}
    # the edges are what they are meant to be (on the host code, the specification)
    t = b'<p lang="de">'
    assert have[tag_at(WINDOW - len(t))][0].any() and not have[tag_at(WINDOW - len(t) + 1)][0].any()
    assert not have[b'<a lang="fr">'][0].any() and have[b'<abbr lang="fr">'][0].any()
    assert not have[b'<meta content="de" http-equiv="Content-Language">'][0].any()
    assert have[b'<html lang="en,fr,de,es,it">'][0].any() and not have[b'<html lang="en,fr,de,es,it,pt">'][0].any()
    # a language hint in a close set alone whacks; with a second member of the set it does not
    k = len(edge_pages())
    assert want_b[k + 10][8:].any() and not want_b[k + 11][8:].any()
    assert want_b[k + 13][8:].any() and not want_b[k + 14][8:].any()   # Chinese alone, Chinese with ChineseT
    assert (want_p[-3:, 0] != 0).tolist() == [True, False, True]       # clipped range, range past the text, NUL cut


def test_kernel_call_variants(gpu, child, inputs):
    """is_plain_text = 1 on HTML pages (no scan), d_hints = NULL on pages with hints."""
    want_p, _ = assert_rows(gpu, child, inputs, "k4")
    assert not want_p[:len(edge_pages())].any()
    assert_rows(gpu, child, inputs, "k5")


def leads_free(buf):
    return not np.isin(np.asarray(buf), BAD_LEADS).any()


def test_end_to_end(gpu, child, inputs):
    ref = refcld.instance(gpu.SYNTH_TABLES)
    for key, name, html in (("d0", "html", True), ("d1s", "c2", False)):
        buf, offs, hints = inputs[2][name]
        n = len(offs) - 1
        got = child[key + "_out"]
        assert_same(got, gpu.detect_batch_ex(buf=buf, offsets=offs, hints=hints, html=html), name + " vs detect_batch_ex")
        assert leads_free(buf)                                          # nothing left out: the reference is defined on all
        want = ref.detect_batch(buf, offs, plain=np.full(n, 0 if html else 1, np.uint8), hints=hints, threads=16)
        assert_same(got, want, name + " vs the reference")
        plain = child["d4_out"] if html else gpu.detect_batch(buf=buf, offsets=offs)
        assert (plain["lang3"] != got["lang3"]).any()                   # the hints changed answers
    buf, offs, _ = inputs[2]["html"]
    assert_same(child["d4_out"], gpu.detect_batch_ex(buf=buf, offsets=offs, html=True), "html without hints")


def test_no_hints_is_detect_batch_device(child):
    assert_same(child["d2_out"], child["p0_out"], "device_hints(NULL, 0) == detect_batch_device")
    assert (child["p0_out"]["text_bytes"] > 0).any()


def test_best_effort_html(gpu, child, inputs):
    buf, offs = inputs[0]["d3_buf"], inputs[0]["d3_offs"]
    assert leads_free(buf)
    want = refcld.instance(gpu.SYNTH_TABLES).detect_batch(buf, offs, plain=np.zeros(300, np.uint8), threads=16,
                                                          flags=gpu.FLAG_BEST_EFFORT)
    assert_same(child["d3_out"], want, "BestEffort | HTML vs the reference")
