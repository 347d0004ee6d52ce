"""cld_split_lines_device and cld_lines_to_chunks_device on the GPU.  The expected
values come from numpy (line_cases.expected_split / expected_chunks), computed
here in the parent straight from the definitions; the host entries must agree
with numpy on the same inputs.  The device entries run in child processes
(lines_device_child.py) in which torch owns the GPU and the buffers, with guard
bytes around every output.  Everything is integers: every comparison is exact.
Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chunk_cases as cc
import cld_amd
import corpus
import line_cases as lc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TILE, WGS, JOIN = lc.TILE, lc.WGS, lc.JOIN
# one byte; around a lane's 16 bytes; around a tile; several tiles; most ranges of tiles used and a ragged last one
SIZES = (1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 4 * TILE + 1, lc.ranges_size())
LF = lc.LF


def run_child(tmp, mode, env=None, **arrays):
    """A child that ends abnormally fails the test that needs it, and nothing else is started."""
    np.savez(tmp / (mode + "_in.npz"), **arrays)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p), **(env or {}))
    r = subprocess.run([sys.executable, os.path.join(HERE, "lines_device_child.py"), mode, str(tmp / (mode + "_in.npz")),
                        str(tmp / (mode + "_out.npz"))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "lines_device_child.py %s ended with %d: %s" % (mode, r.returncode, r.stderr[-3000:])
    return np.load(tmp / (mode + "_out.npz"))


class Cases:
    """The cases of one child run: name -> (index, buf, offs, runs, results, group flags)."""

    def __init__(self):
        self.by_name, self.arrays = {}, {}

    def add(self, name, buf, offs, runs, gflags=0, hostile=False):
        """runs: (flags, capacity: None exact / -1 sizing / lines, alignment of d_buf + offsets[0], line_doc wanted,
        status wanted)."""
        k = len(self.by_name)
        want = {} if hostile else {f: lc.expected_split(buf, offs, f) for f in {r[0] for r in runs}}
        res = lc.random_results(max([w["total"] for w in want.values()] + [1]), seed=k)
        rows = [(f, want[f]["total"] if cap is None else cap, align, int(doc), int(st)) for f, cap, align, doc, st in runs]
        self.by_name[name] = (k, buf, offs, rows, want, res, gflags)
        self.arrays.update({"buf%d" % k: buf, "offs%d" % k: offs, "runs%d" % k: np.array(rows, np.int64).reshape(-1, 5),
                            "res%d" % k: res.view(np.uint8), "gflags%d" % k: np.array(gflags),
                            "hostile%d" % k: np.array(int(hostile))})

    def run(self, tmp, variants, env=None):
        return run_child(tmp, "cases", env=env, cases=np.array(len(self.by_name)),
                         variants=np.array(self.by_name[variants][0]), **self.arrays)


def check(cases, got, name):
    """Every run of one case: the device against numpy; once per flag value the host entry against numpy."""
    k, buf, offs, rows, want, res, gflags = cases.by_name[name]
    n = len(offs) - 1
    for f, w in want.items():
        lc.check_invariants(buf, offs, f, w)
        host = cld_amd.split_lines(buf, offs, f)
        for key in ("line_offsets", "doc_lines", "line_doc"):
            lc.assert_same(host[key], w[key], "%s, flags %d: host %s" % (name, f, key))
        assert (int(host["status"]["total_lines"]), int(host["status"]["max_line_bytes"])) == (w["total"], w["longest"])
    for r, (f, cap, align, doc, st) in enumerate(rows):
        w, key = want[f], "r%d_%d_" % (k, r)
        what = "%s, flags %d, capacity %d of %d, alignment %d" % (name, f, cap, w["total"], align)
        lc.assert_same(got[key + "dl"], w["doc_lines"], what + ": doc_lines")
        if st:
            assert list(got[key + "st"]) == [w["total"], w["longest"]], what + ": status %s" % got[key + "st"]
        else:
            assert key + "st" not in got.files
        if cap < 0:
            assert key + "lo" not in got.files
            continue
        m = min(w["total"], cap)
        lc.assert_same(got[key + "lo"][:m + 1], w["line_offsets"][:m + 1], what + ": line_offsets")   # (the child checks the rest)
        if doc:
            lc.assert_same(got[key + "ld"][:m], w["line_doc"][:m], what + ": line_doc")
            ch = lc.expected_chunks(res, w["line_offsets"], w["line_doc"], offs, w["doc_lines"], gflags, cap)
            lc.assert_same(got[key + "ch"], ch.view(np.uint32), what + ": chunks")
            assert len(ch) == m
        else:
            assert key + "ld" not in got.files
    return want


def both_flags(k=0, cap=None):
    return [(f, cap, (7 * k + 5 * f) % 16, True, True) for f in (0, JOIN)]


# ---------------------------------------------------------------- sizes and layouts

@pytest.fixture(scope="module")
def layout_run(gpu, tmp_path_factory):
    cases = Cases()
    for total in SIZES:
        for la in lc.LAYOUTS:
            k = len(cases.by_name)
            cases.add("%d_%s" % (total, la), *lc.layout_case(total, la, seed=total + len(la)), both_flags(k),
                      gflags=k % 4)
    return cases, cases.run(tmp_path_factory.mktemp("layouts"), "%d_tweets" % SIZES[-1])


@pytest.mark.parametrize("total", SIZES)
def test_split_and_chunks_by_size(layout_run, total):
    cases, got = layout_run
    for la in lc.LAYOUTS:
        want = check(cases, got, "%d_%s" % (total, la))
        offs = cases.by_name["%d_%s" % (total, la)][2]
        docs = int((np.diff(offs.astype(np.int64)) > 0).sum())
        if la == "alllf":
            assert want[0]["total"] == total and want[JOIN]["total"] == docs
        if la == "nolf":
            assert want[0]["total"] == want[JOIN]["total"] == docs
        if la == "tweets" and total > TILE:
            assert docs > 8 * (total // TILE), "many documents per tile"
        if la == "one":
            assert docs == 1
        if la == "mixed" and total > 40:
            assert (np.diff(offs.astype(np.int64)) == 0).sum() >= 3
    if total == SIZES[-1]:
        tiles = -(-(total + 15) // TILE)
        per = -(-tiles // WGS)
        assert per > 1 and WGS * 3 // 4 < -(-tiles // per) < WGS and tiles % per, "most ranges, a ragged last one"


def test_variants(layout_run):
    cases, got = layout_run
    name = "%d_tweets" % SIZES[-1]
    k, buf, offs, rows, want, res, gflags = cases.by_name[name]
    f = rows[0][0]
    w = want[f]
    assert w["total"] > 10000
    for tag in ("stream_", "again_"):
        lc.assert_same(got[tag + "lo"], w["line_offsets"], tag + "line_offsets")
        lc.assert_same(got[tag + "ld"], w["line_doc"], tag + "line_doc")
        lc.assert_same(got[tag + "dl"], w["doc_lines"], tag + "doc_lines")
        assert list(got[tag + "st"]) == [w["total"], w["longest"]]
        for key in ("lo", "ld", "dl", "st"):
            assert np.array_equal(got[tag + key], got["r%d_0_%s" % (k, key)]), "the output differs from run to run"
    assert int(got["short_rc"]) == cld_amd.ENOSPC
    assert bool(got["short_untouched"]), "a call that returned CLD_ENOSPC wrote something"


def test_no_documents(layout_run):
    got = layout_run[1]
    assert list(got["empty_dl"]) == [0] and list(got["empty_st"]) == [0, 0] and bool(got["empty_lo_untouched"])


# ---------------------------------------------------------------- alignments, seams, blank runs, capacities

def hostile_case():
    """Offsets that go down, and one past buf_bytes."""
    buf, offs = lc.layout_case(3 * TILE + 9, "tweets", seed=99)
    offs = offs.copy()
    offs[5] = offs[3] - 7
    offs[len(offs) // 2] = offs[len(offs) // 2 - 3]
    offs[-3] = len(buf) + 1000
    assert (np.diff(offs.astype(np.int64)) < 0).sum() >= 3 and offs.max() > len(buf)
    return buf, offs


@pytest.fixture(scope="module")
def special_run(gpu, tmp_path_factory):
    cases = Cases()
    cases.add("align", *lc.layout_case(2 * TILE + 3, "tweets", seed=41),
              [(f, None, a, True, True) for a in range(16) for f in (0, JOIN)], gflags=cld_amd.GROUP_TOP1)
    cases.add("align_lead0", *lc.layout_case(TILE + 30, "mixed", seed=42, lead=0), [(JOIN, None, a, True, True) for a in (0, 9)])
    cases.add("seams", *lc.seam_case(), [(0, None, 0, True, True), (JOIN, None, 0, True, True)])
    for name, (buf, offs) in lc.join_cases().items():
        cases.add("join_" + name, buf, offs, [(0, None, 0, True, True), (JOIN, None, 0, True, True), (JOIN, None, 11, True, True)])
    buf, offs = lc.layout_case(5 * TILE + 1, "mixed", seed=43)
    m = lc.expected_split(buf, offs, JOIN)["total"]
    assert m > 40
    cases.add("capacity", buf, offs,
              [(JOIN, cap, 3, True, True) for cap in (m, m - 1, m // 2, 1, -1, m + 5)] +
              [(JOIN, m // 2, 3, False, True), (JOIN, m, 3, True, False), (0, -1, 3, True, False), (0, 7, 3, False, False)],
              gflags=cld_amd.GROUP_RELIABLE_ONLY)
    cases.add("hostile", *hostile_case(), [(0, 50, 2, True, True), (JOIN, 50, 13, True, True), (JOIN, -1, 0, True, True),
                                           (0, 5000, 5, True, False)], hostile=True)
    cases.add("dense", *lc.dense_case(), both_flags(1) + both_flags(2))
    return cases, cases.run(tmp_path_factory.mktemp("special"), "capacity")


def test_dense_and_empty_documents(special_run):
    """More than 64 document starts in a tile (the probe of 64 offsets does not reach the tile's last document),
    and hundreds of empty documents at one position in the middle of the text."""
    check(*special_run, "dense")
    offs = special_run[0].by_name["dense"][2].astype(np.int64)
    per_tile = np.bincount((np.unique(offs)[:-1] - offs[0]) // TILE)
    assert per_tile[0] > 300 and per_tile[1] > 300
    empty = np.flatnonzero(np.diff(offs) == 0)
    assert len(empty) == 370 and offs[0] + TILE < offs[empty[0]] < offs[empty[-1]] < offs[-1] - 200


def test_every_alignment(special_run):
    check(*special_run, "align")
    rows = special_run[0].by_name["align"][3]
    assert {(r[0], r[2]) for r in rows} == {(f, a) for f in (0, JOIN) for a in range(16)}
    check(*special_run, "align_lead0")
    assert int(special_run[0].by_name["align_lead0"][2][0]) == 0 < int(special_run[0].by_name["align"][2][0])


def test_seams(special_run):
    """An LF at the last byte of a tile, at the first byte of the next, at the last byte of a range; document
    boundaries at a tile seam and at a range seam (the text's first byte is 16-byte aligned: tile t is text bytes
    [t * TILE, (t + 1) * TILE), two tiles per range)."""
    want = check(*special_run, "seams")
    buf, offs = special_run[0].by_name["seams"][1:3]
    base = int(offs[0])
    tiles = -(-(int(offs[-1]) - base) // TILE)
    assert -(-tiles // WGS) == 2
    starts = set(int(x) - base for x in want[0]["line_offsets"])
    assert {TILE, 2 * TILE, 3 * TILE + 1, 5 * TILE, 5 * TILE + 1, 14 * TILE, 18 * TILE + 1, 40 * TILE} <= starts
    docs = set(int(x) - base for x in offs)
    assert {4 * TILE, 8 * TILE, 22 * TILE, 40 * TILE} <= docs and 40 * TILE - 1 + base in np.flatnonzero(buf == LF)


@pytest.mark.parametrize("name", sorted(lc.join_cases()))
def test_join_blank_runs(special_run, name):
    want = check(*special_run, "join_" + name)
    assert want[JOIN]["total"] < want[0]["total"], "the flag does not act here"
    if name == "long_run":
        assert want[JOIN]["longest"] > 3 * TILE
    if name == "cut_by_doc":                     # the run is two lines: its part before the boundary, and the rest with the text after
        offs = special_run[0].by_name["join_" + name][2]
        lo = want[JOIN]["line_offsets"]
        j = int(want[JOIN]["doc_lines"][1])
        assert int(lo[j]) == int(offs[1]) and int(lo[j] - lo[j - 1]) >= 290 and int(lo[j + 1] - lo[j]) > TILE


def test_capacities_and_optional_outputs(special_run):
    want = check(*special_run, "capacity")
    rows = special_run[0].by_name["capacity"][3]
    m = want[JOIN]["total"]
    assert [r[1] for r in rows[:6]] == [m, m - 1, m // 2, 1, -1, m + 5]
    assert [(r[3], r[4]) for r in rows[6:]] == [(0, 1), (1, 0), (1, 0), (0, 0)]


def test_hostile_offsets(special_run):
    """Only that the call returns CLD_OK and that the child found every guard intact."""
    cases, got = special_run
    k = cases.by_name["hostile"][0]
    assert all("r%d_%d_dl" % (k, r) in got.files for r in range(4))


# ---------------------------------------------------------------- runs of tiles

RUN_WGS = 2                                      # CLD_LINES_WGS: 8 waves for the two text kernels
RUN_CASES = ["seams", "dense", "capacity", "tweets", "mixed", "alllf"] + ["join_" + k for k in sorted(lc.join_cases())]


@pytest.fixture(scope="module")
def runs_run(gpu, tmp_path_factory):
    """The cases above again in a child whose split runs its two text kernels on 8 waves, so that every wave takes
    a run of many consecutive tiles -- what a batch of more than 8 MB does at the full grid: the documents carried
    from tile to tile, runs that cross range seams, blank runs and document boundaries inside a run."""
    cases = Cases()
    cases.add("seams", *lc.seam_case(), [(0, None, 0, True, True), (JOIN, None, 0, True, True)])
    for name, (buf, offs) in lc.join_cases().items():
        cases.add("join_" + name, buf, offs, [(0, None, 0, True, True), (JOIN, None, 0, True, True), (JOIN, None, 11, True, True)])
    for la in ("tweets", "mixed", "alllf"):
        cases.add(la, *lc.layout_case(SIZES[-1], la, seed=SIZES[-1] + len(la)), both_flags(len(cases.by_name)), gflags=3)
    cases.add("dense", *lc.dense_case(), both_flags(1))
    buf, offs = lc.layout_case(20 * TILE + 1, "mixed", seed=44)
    m = lc.expected_split(buf, offs, JOIN)["total"]
    cases.add("capacity", buf, offs, [(JOIN, cap, 3, True, True) for cap in (m, m // 2, -1)] + [(0, 7, 5, False, False)])
    cases.add("hostile", *hostile_case(), [(0, 50, 2, True, True), (JOIN, 5000, 13, True, True)], hostile=True)
    return cases, cases.run(tmp_path_factory.mktemp("runs"), "tweets", env={"CLD_LINES_WGS": str(RUN_WGS)})


@pytest.mark.parametrize("name", RUN_CASES)
def test_runs_of_tiles(runs_run, name):
    cases, got = runs_run
    want = check(cases, got, name)
    offs = cases.by_name[name][2]
    tiles = -(-int(offs[-1] - offs[0]) // TILE)
    if name != "dense":                          # (4 tiles: one per wave; the others: runs of 3 to 92 tiles)
        assert tiles // (4 * RUN_WGS) >= 2
    if name.startswith("join_"):
        assert want[JOIN]["total"] < want[0]["total"]
        assert -(-tiles // WGS) == 2 and tiles // (4 * RUN_WGS) == 64, "runs of 64 tiles over ranges of 2"


def test_runs_variants_and_hostile(runs_run):
    cases, got = runs_run
    k, buf, offs, rows, want, res, gflags = cases.by_name["tweets"]
    w = want[rows[0][0]]
    for tag in ("stream_", "again_"):
        lc.assert_same(got[tag + "lo"], w["line_offsets"], tag + "line_offsets")
        assert list(got[tag + "st"]) == [w["total"], w["longest"]]
    k = cases.by_name["hostile"][0]
    assert all("r%d_%d_dl" % (k, r) in got.files for r in range(2))


# ---------------------------------------------------------------- end to end

def pages():
    """~300 pages, each 3..40 corpus tweets of several generators joined by LF; some with blank lines between
    the tweets, some with a trailing LF."""
    parts = [corpus.GENERATORS["c2"](4200), corpus.GENERATORS["c2n"](1500), corpus.GENERATORS["c4"](800)]
    docs = [bytes(b[o[i]:o[i + 1]]).replace(b"\n", b" ") for b, o in parts for i in range(len(o) - 1)]
    rng = np.random.default_rng(23)
    docs = [docs[i] for i in rng.permutation(len(docs))]
    out = []
    while len(docs) >= 40 and len(out) < 300:
        k = int(rng.integers(3, 41))
        sep = [b"\n", b"\n\n", b"\n \t\n\r\n"][int(rng.integers(0, 3))] if rng.random() < 0.4 else b"\n"
        page = sep.join(docs[:k]) + (b"\n" if rng.random() < 0.5 else b"")
        out.append(page)
        docs = docs[k:]
    return out


def test_split_detect_chunks_gather_group(gpu, tmp_path):
    docs = pages()
    buf, offs = cld_amd.pack(docs)
    buf, offs = np.asarray(buf, np.uint8), np.asarray(offs, np.uint64)
    n = len(docs)
    assert 250 <= n <= 300
    want = lc.expected_split(buf, offs, JOIN)
    m = want["total"]
    # the case is not vacuous: checked with the host entries first
    host = cld_amd.split_lines(buf, offs, JOIN)
    lc.assert_same(host["line_offsets"], want["line_offsets"], "host line_offsets")
    assert m < lc.expected_split(buf, offs, 0)["total"], "blank lines between tweets"
    res = gpu.detect_batch(buf=buf, offsets=want["line_offsets"])
    chunks = lc.expected_chunks(res, want["line_offsets"], want["line_doc"], offs, want["doc_lines"])
    lc.assert_same(cld_amd.lines_to_chunks(res, host["line_offsets"], host["line_doc"], offs, host["doc_lines"]).view(np.uint8),
                   chunks.view(np.uint8), "host chunks")
    c = {"buf": buf, "offs": offs, "chunks": chunks, "coffs": want["doc_lines"], "cap": m}
    totals = cc.expected_totals(c)
    real = np.arange(cc.BINS) != cld_amd.UNKNOWN_LANGUAGE
    assert int((totals["chunk_counts"][real] > 0).sum()) >= 4, "the pages should hold several languages besides UNKNOWN"
    dl = want["doc_lines"].astype(np.int64)
    assert sum(len(set(chunks["lang1"][dl[i]:dl[i + 1]])) > 1 for i in range(n)) >= 20, "pages with lines in several languages"

    got = run_child(tmp_path, "e2e", buf=buf, offs=offs)
    lc.assert_same(got["lo"], want["line_offsets"], "line_offsets")
    lc.assert_same(got["ld"], want["line_doc"], "line_doc")
    lc.assert_same(got["dl"], want["doc_lines"], "doc_lines")
    assert list(got["st"]) == [m, want["longest"]]
    assert np.array_equal(got["results"].view(cld_amd.RESULT_DTYPE).view(np.uint8), res.view(np.uint8)), \
        "detection on the line batch differs from detection of the same lines from the host"
    lc.assert_same(got["chunks"], chunks.view(np.uint32), "chunks")
    cc.assert_same(got["chunk_counts"], totals["chunk_counts"], "chunk counts")
    cc.assert_same(got["chunk_bytes"], totals["chunk_bytes"], "chunk bytes")
    assert int(got["chunk_bytes"].sum()) == int(offs[-1] - offs[0]), "the lines tile the text"
    bins = [int(b) for b in got["bins"]]
    assert len(bins) == 4
    for b in bins:
        sel = np.zeros(cc.BINS, np.uint8)
        sel[b] = 1
        data, o = cc.expected_gather(c, sel, 0)
        cc.assert_same(got["bin%d_offs" % b], o, "bin %d: offsets" % b)
        cc.assert_same(got["bin%d_buf" % b], data, "bin %d: bytes" % b)
    grouped = cld_amd.group_by_language(res, offsets=want["line_offsets"])
    cc.assert_same(got["group_counts"], grouped["counts"], "lines per language")
    cc.assert_same(got["group_bin_bytes"], grouped["bin_bytes"], "line bytes per language")
    assert int(got["group_bin_bytes"].sum()) == int(offs[-1] - offs[0]) and int(got["group_counts"].sum()) == m
    lc.assert_same(got["group_bin_bytes"], totals["chunk_bytes"], "the two ways to the bytes per language")
