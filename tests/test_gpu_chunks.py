"""cld_chunk_totals_device and cld_gather_chunks_device on the GPU.  The expected
values come from numpy (chunk_cases.expected_totals / expected_gather), computed
here in the parent straight from the definitions; the host entries must agree
with numpy on the same inputs.  The device entries run in child processes
(chunks_device_child.py) in which torch owns the GPU and the buffers.
Everything is integers and bytes: every comparison is exact.  Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chunk_cases as cc
import cld_amd
import corpus

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TILE = cld_amd.GROUP_TILE
# one chunk; around a wave; around a workgroup's step; several steps per range of chunks, most
# ranges used and a ragged last one
SIZES = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 200003)
LAYOUTS = ("ones", "one", "mixed", "inverted")
SELECTS = cc.select_sets()
SELECT_IDS = {name: k for k, name in enumerate(SELECTS)}
SPACE = cld_amd.CHUNKS_SPACE


def run_child(tmp, mode, **arrays):
    """A child that ends abnormally fails the test that needs it, and nothing else is started."""
    np.savez(tmp / (mode + "_in.npz"), **arrays)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    r = subprocess.run([sys.executable, os.path.join(HERE, "chunks_device_child.py"), mode, str(tmp / (mode + "_in.npz")),
                        str(tmp / (mode + "_out.npz"))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "chunks_device_child.py %s ended with %d: %s" % (mode, r.returncode, r.stderr[-3000:])
    return np.load(tmp / (mode + "_out.npz"))


class Cases:
    """The cases of one child run: name -> (index, case, [(select name, flags, capacity, alignment, want)])."""

    def __init__(self):
        self.by_name, self.arrays, self.limits = {}, {}, {}

    def add(self, name, c, runs, limit=None):
        """runs: (select name, flags, capacity: None exact / -1 sizing / bytes, output alignment).
        limit: the chunk instances the device gather places (chunk_cases.instances); the host entry takes all."""
        k = len(self.by_name)
        rows, kept = [], []
        self.limits[name] = limit
        for sel, flags, cap, align in runs:
            data, offs = cc.expected_gather(c, SELECTS[sel], flags, limit)
            cap = len(data) if cap is None else cap
            rows.append((SELECT_IDS[sel], flags, cap, len(data), align))
            kept.append((sel, flags, cap, align, data, offs))
        self.by_name[name] = (k, c, kept)
        self.arrays.update({"buf%d" % k: c["buf"], "offs%d" % k: c["offs"], "chunks%d" % k: c["chunks"].view(np.uint8),
                            "coffs%d" % k: c["coffs"], "cap%d" % k: np.array(c["cap"]),
                            "runs%d" % k: np.array(rows, np.int64).reshape(-1, 5)})

    def run(self, tmp, variants):
        sel = {"select%d" % k: SELECTS[name] for name, k in SELECT_IDS.items()}
        return run_child(tmp, "cases", cases=np.array(len(self.by_name)), variants=np.array(self.by_name[variants][0]),
                         **sel, **self.arrays)


def check(cases, got, name):
    """Totals and every gather of one case: the device against numpy, and the host entries against numpy."""
    k, c, runs = cases.by_name[name]
    want = cc.expected_totals(c)
    host = cld_amd.chunk_totals(c["offs"], c["chunks"], c["coffs"], chunk_cap=c["cap"])
    for f, key in (("chunk_counts", "t%d_counts" % k), ("chunk_bytes", "t%d_bytes" % k)):
        cc.assert_same(got[key], want[f], "%s: device %s" % (name, f))
        cc.assert_same(host[f], want[f], "%s: host %s" % (name, f))
    for r, (sel, flags, cap, align, data, offs) in enumerate(runs):
        what = "%s, select %s, flags %d, capacity %d of %d, alignment %d" % (name, sel, flags, cap, len(data), align)
        cc.assert_same(got["g%d_%d_offs" % (k, r)], offs, what + ": device offsets")
        cc.assert_same(got["g%d_%d_buf" % (k, r)], data[:max(cap, 0)], what + ": device bytes")   # (the child checks every byte outside)
        if cases.limits[name] is not None:           # (overlapping vectors: the host entry takes every instance)
            data, offs = cc.expected_gather(c, SELECTS[sel], flags)
        hb, ho = cld_amd.gather_chunks(c["buf"], c["offs"], c["chunks"], c["coffs"], SELECTS[sel], flags,
                                       chunk_cap=c["cap"], out_cap=max(cap, 0))
        cc.assert_same(ho, offs, what + ": host offsets")
        cc.assert_same(hb, data[:max(cap, 0)], what + ": host bytes")
    return want, runs


def all_runs(k=0):
    return [(sel, flags, None, (5 * k + 3 * r) % 16) for r, (sel, flags) in
            enumerate((s, f) for s in SELECTS for f in (0, SPACE))]


# ---------------------------------------------------------------- sizes and layouts

def layouts_of(total):
    return [la for la in LAYOUTS if la != "inverted" or total >= 63]


@pytest.fixture(scope="module")
def layout_run(gpu, tmp_path_factory):
    cases = Cases()
    for total in SIZES:
        for la in layouts_of(total):
            cases.add("%d_%s" % (total, la), cc.layout_case(total, la, seed=total + len(la)), all_runs(len(cases.by_name)))
    return cases, cases.run(tmp_path_factory.mktemp("layouts"), "200003_mixed")


@pytest.mark.parametrize("total", SIZES)
def test_totals_and_gather_by_size(layout_run, total):
    cases, got = layout_run
    for la in layouts_of(total):
        name = "%d_%s" % (total, la)
        want, runs = check(cases, got, name)
        c = cases.by_name[name][1]
        if la != "inverted":
            assert int(want["chunk_counts"].sum()) == total
        else:                            # some chunks belong to two documents, some to none
            assert (np.diff(c["coffs"].astype(np.int64)) < 0).sum() == 3
        for sel, flags, cap, align, data, offs in runs:
            if sel == "one" and flags == 0:          # the totals size the buffer of one language exactly
                assert len(data) == int(want["chunk_bytes"][3])
            if sel == "none":
                assert len(data) == 0 and not offs.any()
        if total >= 63:
            assert sum(len(r[4]) for r in runs) > 0


def test_variants(layout_run):
    cases, got = layout_run
    k, c, runs = cases.by_name["200003_mixed"]
    want = cc.expected_totals(c)
    sel, flags, cap, align, data, offs = runs[0]
    assert len(data) > 100000
    cc.assert_same(got["stream_counts"], want["chunk_counts"], "on a torch stream: counts")
    cc.assert_same(got["stream_bytes"], want["chunk_bytes"], "on a torch stream: bytes")
    cc.assert_same(got["stream_buf"], data, "on a torch stream: gathered bytes")
    cc.assert_same(got["stream_offs"], offs, "on a torch stream: offsets")
    cc.assert_same(got["only_counts"], want["chunk_counts"], "counts alone")   # (the child checks that the other stays untouched)
    cc.assert_same(got["only_bytes"], want["chunk_bytes"], "bytes alone")
    assert np.array_equal(got["again_buf"], got["g%d_0_buf" % k]) and np.array_equal(got["again_offs"], got["g%d_0_offs" % k]), \
        "the output differs from run to run"
    assert int(got["short_rc_totals"]) == cld_amd.ENOSPC and int(got["short_rc_gather"]) == cld_amd.ENOSPC
    assert bool(got["short_untouched"]), "a call that returned CLD_ENOSPC wrote something"


def test_no_documents(layout_run):
    got = layout_run[1]
    assert not got["empty_counts"].any() and not got["empty_bytes"].any() and list(got["empty_offs"]) == [0]
    assert len(got["empty_counts"]) == cc.BINS


# ---------------------------------------------------------------- pieces, hostile words, capacities

@pytest.fixture(scope="module")
def special_run(gpu, tmp_path_factory):
    cases = Cases()
    # every piece length at every source alignment, at every output alignment
    cases.add("lengths", cc.lengths_case(), [("all", 0, None, a) for a in range(16)] +
              [("all", SPACE, None, 0), ("but26", SPACE, None, 5), ("one", 0, None, 11), ("but26", 0, None, 7)])
    cases.add("hostile", cc.hostile_case(), all_runs(1) + all_runs(2))
    capped = cc.capped_case()
    cases.add("capped", capped, all_runs(3))
    c = cc.layout_case(TILE + 1, "mixed", seed=77)
    total = len(cc.expected_gather(c, SELECTS["but26"], SPACE)[0])
    assert total > 2000
    cases.add("capacity", c, [("but26", SPACE, cap, 9) for cap in (total, total - 1, total // 2, -1)] +
              [("all", 0, 1, 0), ("all", 0, 17, 15)])
    c = cc.overlap_case()
    cases.add("overlap", c, all_runs(4), limit=c["cap"])
    return cases, cases.run(tmp_path_factory.mktemp("special"), "hostile")


def test_piece_lengths_and_alignments(special_run):
    want, runs = check(*special_run, "lengths")
    assert int(want["chunk_bytes"][41]) == cc.BIG_PIECE
    c = special_run[0].by_name["lengths"][1]
    assert set(cc.PIECE_LENGTHS) | {cc.BIG_PIECE} <= set(int(x) for x in c["chunks"]["bytes"])
    assert {r[3] for r in runs} == set(range(16))


def test_hostile_chunk_words(special_run):
    want, runs = check(*special_run, "hostile")
    ch = special_run[0].by_name["hostile"][1]["chunks"]
    assert {-1, 40, 41, cc.I32MAX} <= set(int(x) for x in ch["offset"]) and {-1, 0, cc.I32MAX} <= set(int(x) for x in ch["bytes"])
    assert {613, 614, 0xFFFF} <= set(int(x) for x in ch["lang1"])
    assert want["chunk_counts"][613] == 1 and want["chunk_counts"][614] == 3
    # the neighbour relations of CLD_CHUNKS_SPACE, document 3 under "one" (language 3 kept): the slow reference by hand
    c = special_run[0].by_name["hostile"][1]
    data, offs = cc.slow_gather(c, SELECTS["one"], SPACE)
    doc = bytes(c["buf"][int(c["offs"][3]):int(c["offs"][4])])
    assert bytes(data[int(offs[3]):int(offs[4])]) == doc[0:9] + b" " + doc[12:15] + b" " + doc[20:25] + b" " + doc[25:30] + \
        b" " + doc[35:40]
    for sel, flags, cap, align, d, o in runs:
        s, so = cc.slow_gather(c, SELECTS[sel], flags)
        assert np.array_equal(s, d) and np.array_equal(so, o)


def test_chunk_cap_inside_a_vector(special_run):
    want, _ = check(*special_run, "capped")
    c = special_run[0].by_name["capped"][1]
    assert int(want["chunk_counts"].sum()) == c["cap"] < int(c["coffs"][-1])


def test_overlapping_vectors_past_chunk_cap(special_run):
    """The documented limit: vectors that together hold more than chunk_cap chunks.  The device gather places the
    first chunk_cap instances in document order (and writes nothing outside its output: the child's guards);
    the totals, on the device too, and the host gather count every instance."""
    cases = special_run[0]
    c = cases.by_name["overlap"][1]
    want, runs = check(*special_run, "overlap")
    assert int(want["chunk_counts"].sum()) == len(cc.instances(c)[0]) > 3 * c["cap"]
    short = [len(r[4]) for r in runs]
    full = [len(cc.expected_gather(c, SELECTS[r[0]], r[1])[0]) for r in runs]
    assert all(a < b for a, b, r in zip(short, full, runs) if r[0] != "none") and max(short) > 2000


def test_output_capacity(special_run):
    _, runs = check(*special_run, "capacity")
    assert [r[2] < len(r[4]) for r in runs] == [False, True, True, True, True, True]


# ---------------------------------------------------------------- end to end

def mixed_documents():
    """A few hundred corpus documents, a third of them two or three documents of different generators joined."""
    parts = [corpus.GENERATORS["c2"](260), corpus.GENERATORS["c4"](120)]
    docs = [bytes(b[o[i]:o[i + 1]]) for b, o in parts for i in range(len(o) - 1)]
    rng = np.random.default_rng(17)
    docs = [docs[i] for i in rng.permutation(len(docs))]
    joined = []
    while docs:
        k = int(rng.integers(2, 4)) if rng.random() < 0.33 else 1
        joined.append(b" ".join(docs[:k]))
        docs = docs[k:]
    return joined


def test_detect_vec_totals_gather_detect(gpu, tmp_path):
    docs = mixed_documents()
    buf, offs = cld_amd.pack(docs)
    n = len(docs)
    assert 200 <= n <= 400
    got = run_child(tmp_path, "e2e", buf=buf, offs=offs)
    res, chunks, coffs = cld_amd.detect_batch_vec(buf=buf, offsets=offs)
    assert np.array_equal(got["coffs"], coffs) and np.array_equal(got["chunks"].view(cld_amd.CHUNK_DTYPE), chunks), \
        "the device vectors are not cld_detect_batch_vec's"
    assert np.array_equal(got["results"].view(cld_amd.RESULT_DTYPE).view(np.uint8), res.view(np.uint8))
    c = {"buf": np.asarray(buf, np.uint8), "offs": np.asarray(offs, np.uint64), "chunks": chunks, "coffs": coffs,
         "cap": len(chunks)}
    want = cc.expected_totals(c)
    cc.assert_same(got["chunk_counts"], want["chunk_counts"], "device counts")
    cc.assert_same(got["chunk_bytes"], want["chunk_bytes"], "device bytes")
    _, _, s, e, _ = cc.pieces(c)
    assert int(got["chunk_bytes"].sum()) == int((e - s).sum())
    assert int((want["chunk_counts"] > 0).sum()) >= 4, "the corpus should hold several languages"
    langs_per_doc = [len(set(chunks["lang1"][int(coffs[i]):int(coffs[i + 1])])) for i in range(n)]
    assert sum(k > 1 for k in langs_per_doc) >= 20, "joined documents should have vectors of several languages"
    bins = [int(b) for b in got["bins"]]
    assert len(bins) == 4
    for b in bins:
        sel = np.zeros(cc.BINS, np.uint8)
        sel[b] = 1
        for flags in (0, SPACE):
            key = "bin%d_f%d_" % (b, flags)
            data, o = cc.expected_gather(c, sel, flags)
            cc.assert_same(got[key + "offs"], o, key + "offsets")
            cc.assert_same(got[key + "buf"], data, key + "bytes")
            again = gpu.detect_batch(buf=data, offsets=o)
            assert np.array_equal(got[key + "results"].view(cld_amd.RESULT_DTYPE).view(np.uint8), again.view(np.uint8)), \
                key + ": detection on the gathered batch differs from detection of the same bytes from the host"
