"""cld_group_by_language_device and cld_gather_docs_device on the GPU.  The
expected values come from numpy (group_cases.expected, Python's concatenation),
computed here in the parent, and the host entry must agree with numpy on the
same inputs.  The device entries run in child processes (group_device_child.py)
in which torch owns the GPU and the buffers.  Everything is integers and bytes:
every comparison is exact.  Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cld_amd
import corpus
import group_cases as gc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TILE = cld_amd.GROUP_TILE
# one document; around a wave; around a workgroup's range (one step of it, at these sizes);
# several steps per range, most ranges used and a ragged tail
SIZES = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 200003)
VARIANTS_N = 200003


def run_child(tmp, mode, **arrays):
    """A child that ends abnormally fails the test that needs it, and nothing else is started."""
    np.savez(tmp / (mode + "_in.npz"), **arrays)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    r = subprocess.run([sys.executable, os.path.join(HERE, "group_device_child.py"), mode, str(tmp / (mode + "_in.npz")),
                        str(tmp / (mode + "_out.npz"))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "group_device_child.py %s ended with %d: %s" % (mode, r.returncode, r.stderr[-3000:])
    return np.load(tmp / (mode + "_out.npz"))


# ---------------------------------------------------------------- group

@pytest.fixture(scope="module")
def group_run(gpu, tmp_path_factory):
    """Every case on the device in one child: [(n, name, results, offsets)], the variants' case, the outputs."""
    assert cld_amd.group_range(VARIANTS_N) == 2 * TILE and cld_amd.group_range(TILE + 1) == TILE
    cases, arrays = [], {}
    for n in SIZES:
        offs = gc.lengths_for(n, seed=n)
        for name, keys in gc.key_sets(n, seed=n).items():
            k = len(cases)
            res = gc.results_for(keys, seed=k)
            cases.append((n, name, res, offs))
            arrays["res%d" % k] = res.view(np.uint8)
            arrays["offs%d" % k] = offs
            arrays["flags%d" % k] = np.array(gc.FLAG_SETS)
    variants = [k for k, c in enumerate(cases) if c[0] == VARIANTS_N and c[1] == "runs"][0]
    got = run_child(tmp_path_factory.mktemp("group"), "group", cases=np.array(len(cases)), variants=np.array(variants),
                    **arrays)
    return cases, variants, got


@pytest.mark.parametrize("n", SIZES)
def test_group_key_sets(group_run, n):
    cases, _, got = group_run
    seen = 0
    for k, (cn, name, res, offs) in enumerate(cases):
        if cn != n:
            continue
        for flags in gc.FLAG_SETS:
            want = gc.expected(res, offs, flags)
            what = "%s, n %d, flags %d" % (name, n, flags)
            gc.assert_group({f: got["c%d_f%d_%s" % (k, flags, f)] for f in want}, want, "device: " + what)
            gc.assert_group(cld_amd.group_by_language(res, offsets=offs, flags=flags), want, "host: " + what)
            seen += 1
    assert seen == 4 * len(gc.key_sets(2))


def test_group_variants(group_run):
    cases, variants, got = group_run
    n, name, res, offs = cases[variants]
    want = gc.expected(res, offs, 0)
    assert int((want["counts"] > 0).sum()) > 100                      # runs of many keys
    gc.assert_group({f: got["stream_" + f] for f in want}, want, "on a torch stream")
    for skip in ("bin_bytes", "order", "group_offsets"):              # (the child checks that the one left out stays untouched)
        gc.assert_group({f: got["no_%s_%s" % (skip, f)] for f in want if f != skip}, want, "without " + skip)
    assert np.array_equal(got["only_counts"], want["counts"])
    assert np.array_equal(got["again_order"], got["c%d_f0_order" % variants]), "order differs from run to run"
    assert int(got["short_rc"]) == cld_amd.ENOSPC and int(got["short_rc2"]) == cld_amd.ENOSPC
    assert bool(got["short_untouched"]), "a call that returned CLD_ENOSPC wrote something"


def test_group_of_no_documents(group_run):
    got = group_run[2]
    assert not got["empty_counts"].any() and not got["empty_bin_bytes"].any() and not got["empty_group_offsets"].any()
    assert len(got["empty_group_offsets"]) == gc.BINS + 1


# ---------------------------------------------------------------- gather

LENGTHS = (0, 1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, (1 << 20) + 3)


@pytest.fixture(scope="module")
def gather_run(gpu, tmp_path_factory):
    rng = np.random.default_rng(11)
    lens = list(LENGTHS[:-1]) + [0, 0, 3, 40, 700, 5000, 0, 33, 64, 4096, 1] + [LENGTHS[-1]] + [0, 2, 31, 100, 0]
    docs = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in lens]
    buf, offs = cld_amd.pack(docs)
    n = len(docs)
    ident = np.arange(n, dtype=np.uint32)
    empties = np.array([i for i, k in enumerate(lens) if k == 0], dtype=np.uint32)
    tiny = np.array([i for i, k in enumerate(lens) if k <= 17], dtype=np.uint32)
    past = ident.copy()
    past[[1, 4, 9, n - 1]] = [n, n + 5, 0xFFFFFFFF, 0x80000000]
    sets = {"identity": ident, "reversed": ident[::-1].copy(), "twice": np.repeat(ident, 2),
            "empties": np.tile(empties, 3), "past": past,
            # more indices than one range holds, then more than every range's first step: the scan's carries
            "many": tiny[rng.integers(0, len(tiny), 70001)], "more": tiny[rng.integers(0, len(tiny), 140001)]}
    arrays, want = {}, {}
    for name, idx in sets.items():
        sel = [docs[i] if i < n else b"" for i in idx]
        data = b"".join(sel)
        o = np.zeros(len(idx) + 1, np.uint64)
        np.cumsum([len(d) for d in sel], out=o[1:])
        total = len(data)
        want[name] = (np.frombuffer(data, np.uint8), o)
        arrays["idx_" + name] = idx
        arrays["total_" + name] = np.array(total)
        arrays["caps_" + name] = np.array(sorted({total, max(total - 1, 0), total // 2}) + [-1])   # -1: the sizing pass
    assert len(want["empties"][0]) == 0 and len(want["twice"][0]) == 2 * len(buf)
    got = run_child(tmp_path_factory.mktemp("gather"), "gather", buf=buf, offs=offs, **arrays)
    return arrays, want, got


@pytest.mark.parametrize("name", ["identity", "reversed", "twice", "empties", "past", "many", "more"])
def test_gather(gather_run, name):
    arrays, want, got = gather_run
    data, offs = want[name]
    for cap in arrays["caps_" + name]:
        what = "%s, capacity %d of %d" % (name, cap, len(data))
        o = got["%s_%d_offs" % (name, cap)]
        assert np.array_equal(o, offs), what + ": the offsets are not the true totals"
        b = got["%s_%d_buf" % (name, cap)]
        w = data[:max(int(cap), 0)]                                  # (the child checks every byte outside it)
        assert len(b) == len(w)
        bad = np.nonzero(b != w)[0]
        assert len(bad) == 0, "%s: %d bytes differ, first at %d: got %#x, want %#x" % (what, len(bad), bad[0], b[bad[0]],
                                                                                     w[bad[0]])


def test_gather_of_no_documents(gather_run):
    assert list(gather_run[2]["empty_offs"]) == [0]


# ---------------------------------------------------------------- end to end

def test_detect_group_gather_detect(gpu, tmp_path):
    parts = [corpus.GENERATORS["c2"](1900), corpus.GENERATORS["c3"](6), corpus.GENERATORS["c4"](90)]
    docs = [bytes(b[o[i]:o[i + 1]]) for b, o in parts for i in range(len(o) - 1)]
    docs = [docs[i] for i in np.random.default_rng(5).permutation(len(docs))]
    buf, offs = cld_amd.pack(docs)
    n = len(docs)
    got = run_child(tmp_path, "e2e", buf=buf, offs=offs)
    res = got["results"].view(cld_amd.RESULT_DTYPE)
    assert np.array_equal(res.view(np.uint8), gpu.detect_batch(buf=buf, offsets=offs).view(np.uint8))
    want = gc.expected(res, offs, 0)
    gc.assert_group({f: got[f] for f in want}, want, "device results")
    gc.assert_group(cld_amd.group_by_language(res, offsets=offs), want, "host entry")
    bins = np.nonzero(want["counts"])[0]
    assert len(bins) >= 5, "the corpus should hold several languages"
    for b in bins:
        sel = want["order"][int(want["group_offsets"][b]):int(want["group_offsets"][b + 1])]
        assert (np.diff(sel.astype(np.int64)) > 0).all()
        sbuf, soffs = cld_amd.pack([docs[i] for i in sel])
        assert np.array_equal(got["bin%d_offs" % b], soffs) and np.array_equal(got["bin%d_buf" % b], sbuf), \
            "bin %d: the gathered batch is not the host's selection" % b
        again = got["bin%d_results" % b].view(cld_amd.RESULT_DTYPE)
        assert np.array_equal(again.view(np.uint8), res[sel].view(np.uint8)), \
            "bin %d: detection on the gathered batch differs from the documents' first results" % b
