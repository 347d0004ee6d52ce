"""cld_html_text_device and cld_chunks_to_page_device on the GPU.  The expected
values come from the model of htmltext_cases.py (a sequential walk over the
oracle's tag parser and entity reader), computed here in the parent; the device
entries run in child processes (htmltext_device_child.py) in which torch owns the
GPU and the buffers, with guard bytes around every output.  Everything is
integers: every comparison is exact.  Needs an MI355X."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cld_amd
import htmltext_cases as hc
import line_cases as lc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LF = hc.BLOCK_LF
ALIGNS = (0, 1, 3, 8, 15)


def run_child(tmp, mode, env=None, **arrays):
    """A child that ends abnormally fails the test that needs it, and nothing else is started."""
    np.savez(tmp / (mode + "_in.npz"), **arrays)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p), **(env or {}))
    r = subprocess.run([sys.executable, os.path.join(HERE, "htmltext_device_child.py"), mode, str(tmp / (mode + "_in.npz")),
                        str(tmp / (mode + "_out.npz"))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "htmltext_device_child.py %s ended with %d: %s" % (mode, r.returncode, r.stderr[-3000:])
    return np.load(tmp / (mode + "_out.npz"))


class Cases:
    """The cases of one child run: name -> (index, buf, offs, runs, hostile)."""

    def __init__(self, oracle):
        self.oracle, self.by_name, self.arrays, self.models = oracle, {}, {}, {}

    def add(self, name, buf, offs, runs, hostile=False):
        """runs: (flags, alignment of d_buf + offsets[0], text_len wanted, pos wanted, status wanted)."""
        k = len(self.by_name)
        self.by_name[name] = (k, buf, offs, runs, hostile)
        self.arrays.update({"buf%d" % k: buf, "offs%d" % k: offs, "runs%d" % k: np.array(runs, np.int64).reshape(-1, 5),
                            "hostile%d" % k: np.array(int(hostile))})

    def run(self, tmp, variants, env=None):
        return run_child(tmp, "cases", env=env, cases=np.array(len(self.by_name)),
                         variants=np.array(self.by_name[variants][0]), **self.arrays)

    def want(self, name, flags):
        """The model on the pages as the entry sees them: every offset clamped to buf_bytes."""
        if (name, flags) not in self.models:
            _, buf, offs, _, _ = self.by_name[name]
            self.models[name, flags] = hc.model(self.oracle, buf, np.minimum(offs, np.uint64(len(buf))), flags)
        return self.models[name, flags]


def got_of(got, key):
    g = {"out": got[key + "out"]}
    for f, name in (("tl", "text_len"), ("pos", "pos"), ("st", "status")):
        if key + f in got.files:
            g[name] = got[key + f]
    return g


def check(cases, got, name):
    k, buf, offs, runs, hostile = cases.by_name[name]
    for r, (flags, align, wl, wp, ws) in enumerate(runs):
        key = "r%d_%d_" % (k, r)
        assert [key + f in got.files for f in ("tl", "pos", "st")] == [bool(wl), bool(wp), bool(ws)]
        hc.check(got_of(got, key), cases.want(name, flags), "%s, flags %d, alignment %d" % (name, flags, align))
    return [cases.want(name, f) for f in sorted({r[0] for r in runs})]


def both(k=0):
    return [(f, (5 * k + 3 * f) % 16, 1, 1, 1) for f in (0, LF)]


def hostile_case():
    """Offsets that go down, and offsets above buf_bytes."""
    buf, offs = hc.pack(hc.seam_pages()[:40], lead=5)
    offs = offs.copy()
    offs[5] = offs[3] - 7
    offs[20] = offs[17]
    offs[-3] = len(buf) + 1000
    offs[9] = 1 << 40
    assert (np.diff(offs.astype(np.int64)) < 0).sum() >= 3 and offs.max() > len(buf)
    return buf, offs


def many_pages(n=257):
    pages = hc.block_pages() + hc.seam_pages() + hc.end_pages()
    assert len(pages) >= n
    return pages[:n]


@pytest.fixture(scope="module")
def main_run(gpu, oracle, tmp_path_factory):
    cases = Cases(oracle)
    cases.add("lengths", *hc.pack(hc.length_pages(), lead=37), both(0) + [(LF, 1, 1, 1, 1)])
    for k, name in enumerate(("seams", "candidates", "ends", "blocks")):
        cases.add(name, *hc.pack(hc.host_batches()[name], lead=3 * k), both(k + 1))
    cases.add("align", *hc.pack(hc.end_pages() + hc.candidate_pages()[:2], lead=37), [(LF, a, 1, 1, 1) for a in ALIGNS])
    cases.add("align_lead0", *hc.pack(hc.end_pages(), lead=0), [(0, a, 1, 1, 1) for a in (0, 15)])
    buf, offs = hc.pack(hc.corpus_pages())
    cases.add("corpus", buf, offs, both(2))
    cases.add("optional", *hc.pack(hc.corpus_pages(16), lead=9),
              [(LF, 5, 0, 1, 1), (LF, 5, 1, 0, 1), (LF, 5, 1, 1, 0), (0, 5, 0, 0, 0)])
    cases.add("one", *hc.pack(hc.corpus_pages(1), lead=1), both(3))
    cases.add("n257", *hc.pack(many_pages(), lead=11), both(4))
    # offsets above buf_bytes: the last pages are cut off, one of them in its middle
    buf, offs = hc.pack(hc.end_pages() + hc.corpus_pages(4))
    cases.add("clamped", buf[:int(offs[-3]) + 100].copy(), offs, both(5))
    cases.add("hostile", *hostile_case(), [(0, 2, 1, 1, 1), (LF, 13, 1, 1, 1), (LF, 0, 0, 0, 0)], hostile=True)
    return cases, cases.run(tmp_path_factory.mktemp("main"), "corpus")


def test_page_lengths_and_forms(main_run):
    """Lengths 0, 1, 63, 64, 65, the LDS stage - 1, the stage, the stage + 1 (staged against in place) and 4
    stages + 1; at each: all text, all '&' (text_len 0), all '<', text with one tag."""
    want = check(*main_run, "lengths")[0]
    tl = want["text_len"].reshape(len(hc.LENGTHS), len(hc.FORMS))
    assert (tl[:, 1] == 0).all() and (tl[:, 0] == np.array(hc.LENGTHS)).all()
    assert {hc.STAGE - 1, hc.STAGE, hc.STAGE + 1, 4 * hc.STAGE + 1, 0, 1, 63, 64, 65} == set(hc.LENGTHS)


@pytest.mark.parametrize("name", ["seams", "candidates", "ends", "blocks"])
def test_seams_segments_ends_and_block_tags(main_run, name):
    want = check(*main_run, name)
    if name == "blocks":
        assert int((want[1]["out"] == 0x0A).sum()) > 5 * 3 * (len(hc.BLOCK_TAGS) - 2) and not (want[0]["out"] == 0x0A).any()
    if name == "candidates":
        assert want[0]["status"][1] > 3 * hc.CANDS and want[0]["status"][2] > hc.CANDS


def test_alignments(main_run):
    check(*main_run, "align")
    check(*main_run, "align_lead0")
    assert {r[1] for r in main_run[0].by_name["align"][3]} == set(ALIGNS)


def test_optional_outputs_absent_in_turn(main_run):
    check(*main_run, "optional")


def test_one_page_and_257_pages(main_run):
    check(*main_run, "one")
    check(*main_run, "n257")
    assert len(main_run[0].by_name["n257"][2]) - 1 == 257 and len(main_run[0].by_name["one"][2]) - 1 == 1


def test_offsets_above_buf_bytes_are_clamped(main_run):
    want = check(*main_run, "clamped")[0]
    k, buf, offs, _, _ = main_run[0].by_name["clamped"]
    assert int(offs[-1]) > len(buf) > int(offs[-3]) and want["text_len"][-1] == 0 and want["text_len"][-3] > 0
    assert want["hi"] == len(buf)


def test_hostile_offsets(main_run):
    """Only that the calls return CLD_OK and that the child found every guard intact."""
    cases, got = main_run
    k = cases.by_name["hostile"][0]
    assert all("r%d_%d_out" % (k, r) in got.files for r in range(3))


def test_corpus_equals_host_entry(main_run):
    """Byte for byte, pos, padding and status included; on a stream of torch's, and the same from run to run."""
    cases, got = main_run
    check(cases, got, "corpus")
    k, buf, offs, runs, _ = cases.by_name["corpus"]
    for r, (flags, _, _, _, _) in enumerate(runs):
        host = cld_amd.html_text(buf, offs, flags, pos=True)
        key = "r%d_%d_" % (k, r)
        assert np.array_equal(got[key + "out"], host["out"]) and np.array_equal(got[key + "pos"], host["pos"])
        assert np.array_equal(got[key + "tl"], host["text_len"].view(np.uint32))
        assert hc.status_list(got[key + "st"]) == hc.status_list(host["status"])
    for tag in ("stream_", "again_"):
        for f in ("out", "tl", "pos", "st"):
            assert np.array_equal(got[tag + f], got["r%d_0_%s" % (k, f)]), "the output differs from run to run"


def test_no_pages(main_run):
    got = main_run[1]
    assert list(got["empty_st"]) == [0, 0, 0] and bool(got["empty_untouched"])


@pytest.fixture(scope="module")
def stride_run(gpu, oracle, tmp_path_factory):
    """The kernel on 2 workgroups (8 waves): 257 pages make every wave take 32 pages by the grid stride, and
    the last one a 33rd."""
    cases = Cases(oracle)
    cases.add("n257", *hc.pack(many_pages(), lead=11), both(4))
    cases.add("lengths", *hc.pack(hc.length_pages(), lead=37), both(0))
    cases.add("hostile", *hostile_case(), [(LF, 7, 1, 1, 1)], hostile=True)
    return cases, cases.run(tmp_path_factory.mktemp("stride"), "n257", env={"CLD_HTMLTEXT_WGS": "2"})


@pytest.mark.parametrize("name", ["n257", "lengths"])
def test_grid_stride(stride_run, name):
    check(*stride_run, name)


# ---------------------------------------------------------------- end to end

def test_text_lines_detect_chunks_back_to_the_page(gpu, oracle, tmp_path):
    pages = hc.corpus_pages(32)
    buf, offs = hc.pack(pages)
    n = len(pages)
    m = hc.model(oracle, buf, offs, LF)
    got = run_child(tmp_path, "e2e", buf=buf, offs=offs)
    hc.check({"out": got["text"], "pos": got["pos"], "text_len": got["tl"], "status": got["st"]}, m, "text")
    # the host entries on the same inputs
    host = cld_amd.split_lines(got["text"], offs, cld_amd.LINES_JOIN_BLANK)
    lc.assert_same(got["lo"], host["line_offsets"], "line_offsets")
    lc.assert_same(got["ld"], host["line_doc"], "line_doc")
    lc.assert_same(got["dl"], host["doc_lines"], "doc_lines")
    lines = len(host["line_doc"])
    assert lines > 4 * n, "block tags should cut the pages into lines"
    res = got["results"].view(cld_amd.RESULT_DTYPE)
    chunks = cld_amd.lines_to_chunks(res, host["line_offsets"], host["line_doc"], offs, host["doc_lines"])
    assert np.array_equal(got["chunks"], chunks.view(np.uint32))
    on_page = cld_amd.chunks_to_page(offs, got["pos"], chunks, host["doc_lines"])
    assert np.array_equal(got["page_chunks"], on_page.view(np.uint32)), "device chunks differ from the host entry's"
    assert np.array_equal(got["in_place"], got["page_chunks"]), "in place differs"
    assert np.array_equal(on_page.view(np.uint8), hc.expected_to_page(offs, got["pos"], chunks, host["doc_lines"], lines).view(np.uint8))
    dl = host["doc_lines"].astype(np.int64)
    for i, p in enumerate(pages):
        v = on_page[dl[i]:dl[i + 1]]
        assert int(v["offset"][0]) == 0 and int(v["offset"][-1] + v["bytes"][-1]) == len(p), "page %d is not tiled" % i
        assert (v["offset"][1:] == v["offset"][:-1] + v["bytes"][:-1]).all(), "page %d is not tiled" % i
        legal = set(m["sources"][i]) | {len(p)}
        assert all(int(o) in legal for o in v["offset"]), "page %d: a chunk starts inside a tag or an entity" % i
    assert len(set(on_page["lang1"].tolist())) > 4


def test_text_scores_as_the_page_scores(gpu, tmp_path):
    """The text batch scored as plain text equals the pages scored in HTML mode (CLD_FLAG_HTML), for the pages and
    the hint handling of test_htmltext_reference.py: HTML mode makes priors from the pages' lang= attributes,
    which do not survive the extraction, so the text is scored through cld_detect_batch_device_hints with the
    content-language hint that restates them; without any hint it is cld_detect_batch_device, also compared
    against that entry on the same text from the host."""
    pages = hc.corpus_pages()
    buf, offs = hc.pack(pages)
    hints = []
    for p in pages:
        want, _ = cld_amd.hint_priors(p, html=True)
        h = cld_amd.Hints.make(content_language=re.match(rb'<html lang="([^"]*)"', p).group(1)) if len(want) else None
        assert cld_amd.hint_priors(b"", html=False, hints=h)[0].tolist() == want.tolist()
        hints.append(h)
    rec, text = cld_amd.pack_hints(hints)
    got = run_child(tmp_path, "detect", buf=buf, offs=offs, hints=rec.view(np.uint8), hint_text=text)
    for flags in (0, LF):
        a = got["on_text%d" % flags].view(cld_amd.RESULT_DTYPE)
        b = got["on_page%d" % flags].view(cld_amd.RESULT_DTYPE)
        bad = [i for i in range(len(pages)) if a[i].tobytes() != b[i].tobytes()]
        assert not bad, "flags %d: pages %s score differently as text" % (flags, bad)
        host = cld_amd.html_text(buf, offs, flags)
        plain = gpu.detect_batch(buf=host["out"], offsets=offs)
        assert np.array_equal(got["plain%d" % flags].view(cld_amd.RESULT_DTYPE).view(np.uint8), plain.view(np.uint8))
    assert len(set(b["summary_lang"].tolist())) > 8
