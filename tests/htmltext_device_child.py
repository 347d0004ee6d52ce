"""Child process of test_gpu_htmltext.py: torch initialises the GPU first (the
library then shares its HIP runtime, as in bench.py), the inputs go to HBM as
torch tensors and the HTML text device entries run on them.

argv: mode, input .npz, output .npz.
  cases   every case <k> of the input (buf<k>, offs<k>, hostile<k>): one
          cld_html_text_device per row of runs<k> = (flags, the alignment 0..15 of
          d_buf + offsets[0], text_len wanted, pos wanted, status wanted) ->
          r<k>_<row>_out / _tl / _pos / _st.  The pages sit between guard bytes and
          buf_bytes is their exact extent; out and pos start as PATTERN between guards
          and must still be PATTERN outside [offsets[0], offsets[n]) (a hostile case:
          outside [0, buf_bytes); it is only run: guards and rc); every input is
          compared before and after.  On the case named by `variants`: a torch stream,
          the same call twice, and n == 0.
  e2e     cld_html_text_device(BLOCK_LF, pos) -> cld_split_lines_device(JOIN_BLANK)
          -> cld_detect_batch_device on the lines -> cld_lines_to_chunks_device ->
          cld_chunks_to_page_device (into a second array, and in place), all on the
          library's stream with no host wait in between once the lines are sized.
  detect  the text batch scored as plain text with the given hints, and the pages
          scored in HTML mode without."""
import sys

import numpy as np
import torch

torch.cuda.set_device(0)
import cld_amd  # noqa: E402

cld_amd.init_device(0)
dev = torch.device("cuda", 0)
mode = sys.argv[1]
inp = np.load(sys.argv[2])
out = {}
GUARD = 64                     # words either side of an array of words
BGUARD = 256                   # bytes either side of the pages
PATTERN = 0x5A


def filled(nbytes):
    return torch.full((max(nbytes, 1),), PATTERN, dtype=torch.uint8, device=dev)


def upload(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


class Guarded:
    """count words of `size` bytes in HBM between two guards, all PATTERN."""

    def __init__(self, count, size):
        self.count, self.size = count, size
        self.t = filled((count + 2 * GUARD) * size)
        self.ptr = self.t.data_ptr() + GUARD * size

    def get(self, what, lo=0, hi=None):
        """The words as numpy; the guards, and the words outside [lo, hi), must be intact."""
        h = self.t.cpu().numpy()
        a, b = GUARD * self.size, (GUARD + self.count) * self.size
        hi = self.count if hi is None else hi
        assert (h[:a + lo * self.size] == PATTERN).all() and (h[a + hi * self.size:] == PATTERN).all(), \
            what + ": written outside its extent"
        return h[a:b].view({1: np.uint8, 4: np.uint32, 8: np.uint64}[self.size]).copy()

    def untouched(self):
        return bool((self.t == PATTERN).all())


class Pages:
    """Pages in HBM, d_buf + offsets[0] at a chosen alignment."""

    def __init__(self, buf, offs):
        self.n, self.nb = len(offs) - 1, len(buf)
        self.buf, self.offs0 = np.ascontiguousarray(buf), int(offs[0])
        self.lo, self.hi = min(int(offs[0]), self.nb), min(max(int(offs[-1]), int(offs[0])), self.nb)
        self.d_offs = upload(offs)
        self.place(0)

    def place(self, align):
        self.d_in = filled(self.nb + 2 * BGUARD + 32)
        assert self.d_in.data_ptr() % 256 == 0
        self.at = BGUARD + (align - self.offs0) % 16
        if self.nb:
            self.d_in[self.at:self.at + self.nb] = torch.from_numpy(self.buf).to(dev)
        self.ptr = self.d_in.data_ptr() + self.at
        assert (self.ptr + self.offs0) % 16 == align
        self.before = [self.d_in.clone(), self.d_offs.clone()]

    def unchanged(self):
        return torch.equal(self.d_in, self.before[0]) and torch.equal(self.d_offs, self.before[1])

    def text(self, flags, align, want_len=True, want_pos=True, want_status=True, stream=None, hostile=False, what=""):
        self.place(align)
        g = {"out": Guarded(self.nb, 1)}
        if want_len:
            g["tl"] = Guarded(self.n, 4)
        if want_pos:
            g["pos"] = Guarded(self.nb, 4)
        if want_status:
            g["st"] = Guarded(3, 8)
        torch.cuda.synchronize()             # (torch filled the tensors on its own stream, not the library's)
        cld_amd.html_text_device(0, self.ptr, self.d_offs.data_ptr(), self.n, self.nb, g["out"].ptr, flags=flags,
                                 d_text_len_ptr=g["tl"].ptr if want_len else None,
                                 d_pos_ptr=g["pos"].ptr if want_pos else None,
                                 d_status_ptr=g["st"].ptr if want_status else None, stream_ptr=stream)
        torch.cuda.synchronize()
        lo, hi = (0, self.nb) if hostile else (self.lo, self.hi)
        got = {"out": g["out"].get(what + " out", lo, hi)}
        if want_len:
            got["tl"] = g["tl"].get(what + " text_len")
        if want_pos:
            got["pos"] = g["pos"].get(what + " pos", lo, hi)
        if want_status:
            got["st"] = g["st"].get(what + " status")
        assert self.unchanged(), what + ": an input was written"
        return got, g


if mode == "cases":
    for k in range(int(inp["cases"])):
        b = Pages(inp["buf%d" % k], inp["offs%d" % k])
        hostile = bool(inp["hostile%d" % k])
        runs = [tuple(int(x) for x in row) for row in inp["runs%d" % k]]
        for r, (flags, align, wl, wp, ws) in enumerate(runs):
            got, _ = b.text(flags, align, bool(wl), bool(wp), bool(ws), hostile=hostile, what="case %d, run %d" % (k, r))
            for f, v in got.items():
                out["r%d_%d_%s" % (k, r, f)] = v
        if k == int(inp["variants"]):
            flags, align = runs[0][:2]
            s = torch.cuda.Stream()
            got, _ = b.text(flags, align, stream=s.cuda_stream, what="on a torch stream")
            for f, v in got.items():
                out["stream_" + f] = v
            got, _ = b.text(flags, align, what="again")
            for f, v in got.items():
                out["again_" + f] = v
    z = {"out": Guarded(8, 1), "tl": Guarded(1, 4), "pos": Guarded(8, 4), "st": Guarded(3, 8)}
    torch.cuda.synchronize()
    cld_amd.html_text_device(0, None, None, 0, 0, None, flags=cld_amd.HTMLTEXT_BLOCK_LF, d_status_ptr=z["st"].ptr)
    cld_amd.html_text_device(0, None, None, 0, 0, None)
    cld_amd.html_text_device(0, z["out"].ptr, None, 0, 8, z["out"].ptr, d_text_len_ptr=z["tl"].ptr, d_pos_ptr=z["pos"].ptr)
    torch.cuda.synchronize()
    out["empty_st"] = z["st"].get("n == 0 status")
    out["empty_untouched"] = np.array(all(z[f].untouched() for f in ("out", "tl", "pos")))

elif mode == "e2e":
    buf, offs = inp["buf"], inp["offs"]
    n, nb = len(offs) - 1, len(buf)
    JOIN = cld_amd.LINES_JOIN_BLANK
    d_buf, d_offs = upload(buf), upload(offs)
    text, pos, tl, st = Guarded(nb, 1), Guarded(nb, 4), Guarded(n, 4), Guarded(3, 8)
    dl, lst = Guarded(n + 1, 8), Guarded(2, 8)
    wb = cld_amd.lines_work_bytes(n, nb)
    w = torch.full((wb,), 0xC3, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    cld_amd.html_text_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, text.ptr, flags=cld_amd.HTMLTEXT_BLOCK_LF,
                             d_text_len_ptr=tl.ptr, d_pos_ptr=pos.ptr, d_status_ptr=st.ptr)
    cld_amd.split_lines_device(0, text.ptr, d_offs.data_ptr(), n, nb, None, None, 0, dl.ptr, w.data_ptr(), wb, flags=JOIN,
                               d_status_ptr=lst.ptr)
    torch.cuda.synchronize()
    m = int(lst.get("sizing status")[0])
    lo, ld, ch, pg = Guarded(m + 1, 8), Guarded(m, 4), Guarded(m * 3, 4), Guarded(m * 3, 4)
    d_res = filled(m * 40)
    torch.cuda.synchronize()
    cld_amd.split_lines_device(0, text.ptr, d_offs.data_ptr(), n, nb, lo.ptr, ld.ptr, m, dl.ptr, w.data_ptr(), wb, flags=JOIN,
                               d_status_ptr=lst.ptr)
    cld_amd.detect_batch_device(0, text.ptr, lo.ptr, m, d_res.data_ptr())
    cld_amd.lines_to_chunks_device(0, d_res.data_ptr(), lo.ptr, ld.ptr, m, d_offs.data_ptr(), n, dl.ptr, ch.ptr)
    cld_amd.chunks_to_page_device(0, d_offs.data_ptr(), n, pos.ptr, ch.ptr, m, dl.ptr, pg.ptr)
    torch.cuda.synchronize()
    out["text"], out["pos"], out["tl"], out["st"] = text.get("text"), pos.get("pos"), tl.get("text_len"), st.get("status")
    out["lo"], out["ld"], out["dl"] = lo.get("line_offsets"), ld.get("line_doc"), dl.get("doc_lines")
    out["results"] = d_res.cpu().numpy()[:m * 40]
    out["chunks"], out["page_chunks"] = ch.get("chunks"), pg.get("page chunks")
    cld_amd.chunks_to_page_device(0, d_offs.data_ptr(), n, pos.ptr, ch.ptr, m, dl.ptr, ch.ptr)
    torch.cuda.synchronize()
    out["in_place"] = ch.get("chunks in place")

else:
    buf, offs = inp["buf"], inp["offs"]
    n, nb = len(offs) - 1, len(buf)
    d_buf, d_offs = upload(buf), upload(offs)
    d_hints, d_htext = upload(inp["hints"]), upload(inp["hint_text"])
    for flags in (0, cld_amd.HTMLTEXT_BLOCK_LF):
        text = Guarded(nb, 1)
        d_page, d_text, d_plain = filled(n * 40), filled(n * 40), filled(n * 40)
        torch.cuda.synchronize()
        cld_amd.html_text_device(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, text.ptr, flags=flags)
        cld_amd.detect_batch_device_hints(0, text.ptr, d_offs.data_ptr(), n, nb, d_text.data_ptr(), d_hints_ptr=d_hints.data_ptr(),
                                          d_hint_text_ptr=d_htext.data_ptr(), hint_text_bytes=len(inp["hint_text"]))
        cld_amd.detect_batch_device(0, text.ptr, d_offs.data_ptr(), n, d_plain.data_ptr())
        cld_amd.detect_batch_device_hints(0, d_buf.data_ptr(), d_offs.data_ptr(), n, nb, d_page.data_ptr(),
                                          flags=cld_amd.FLAG_HTML)
        torch.cuda.synchronize()
        out["on_text%d" % flags], out["on_page%d" % flags] = d_text.cpu().numpy(), d_page.cpu().numpy()
        out["plain%d" % flags] = d_plain.cpu().numpy()
        text.get("text")

np.savez(sys.argv[3], **out)
