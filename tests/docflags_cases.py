"""Batches for the _docflags entries (per-document is_plain_text and CLD2 flags
within one batch), shared by test_gpu_docflags.py and test_gpu_device_docflags.py:
the documents of each case, their mode words, and the judge -- the reference
CLD2 itself (oracle/_ref/librefcld2.so), called once per distinct flags value
over the whole batch with is_plain_text per document, each document's row taken
from the call that matches its own flags.

Every document is free of the lead bytes C0, C1, F5-F7, on which the reference
is undefined (test_reference_pin.defined)."""
import numpy as np

import corpus
from test_gpu_html_hints import random_hints
from test_gpu_parity import FIELDS
from test_reference_pin import defined as leads_free
from test_reference_pin import flag_docs

HTML, QUADS, BEST = 4, 0x0100, 0x4000          # CLD_FLAG_HTML, CLD_FLAG_SCORE_AS_QUADS, CLD_FLAG_BEST_EFFORT
CLD2 = QUADS | BEST
# the eight combinations of {HTML, QUADS, BEST}: mode m has bit 0 = HTML, 1 = QUADS, 2 = BEST
MODE_WORDS = np.array([(HTML if m & 1 else 0) | (QUADS if m & 2 else 0) | (BEST if m & 4 else 0) for m in range(8)],
                      dtype=np.uint32)


def assign_modes(n, seed):
    """One mode word per document: the eight combinations in seeded shuffles, one after
    another, so that every run of eight documents holds all eight and neighbours differ."""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype=np.uint32)
    last = -1
    for a in range(0, n, 8):
        p = rng.permutation(8)
        while p[0] == last:
            p = rng.permutation(8)
        last = int(p[-1])
        out[a:a + 8] = MODE_WORDS[p][:n - a]
    return out


def docs_of(buf, offs):
    return [bytes(buf[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)]


def cut(doc, size):
    """The first size bytes of doc, less a character cut in two."""
    if len(doc) <= size:
        return doc
    k = size
    while k > 0 and (doc[k] & 0xC0) == 0x80:
        k -= 1
    return doc[:k]


def page_of(doc, lang=b"fr", every=7):
    """doc with markup between its words: tags, entities, a lang= attribute and a script
    block -- text an HTML scan reads differently from a plain one."""
    w = doc.split(b" ")
    out = [b"<html lang=\"" + lang + b"\"><body><p>"]
    marks = (b"<b>", b"</b> &amp;", b"caf&eacute;", b"<span class='x > y'>", b"</span>", b"&lt;&gt;",
             b"<script>var s = 'le <b>chat</b>';</script>", b"<!-- note -->")
    for k, x in enumerate(w):
        out.append(x)
        if k % every == every - 1:
            out.append(marks[(k // every) % len(marks)])
    out.append(b"</p></body></html>")
    return b" ".join(out)


# short pages (<= 256 bytes): markup, entities and lang= attributes k_wave's documents can carry
SNIPPETS = [
    b"<p lang=\"fr\">le chat noir mange la souris grise</p>",
    b"<html lang='de'><b>der Hund</b> l&auml;uft &uuml;ber die Stra&szlig;e</html>",
    b"caf&eacute; cr&egrave;me br&ucirc;l&eacute;e &amp; th&eacute;",
    b"<meta http-equiv=\"content-language\" content=\"es\">el perro corre por la calle larga",
    b"<script>var x = 'the quick brown fox';</script> il gatto nero dorme sul divano",
    b"<!-- the quick brown fox jumps --> de kat zit op de mat en slaapt",
    b"&#1044;&#1086;&#1084; &#1089;&#1090;&#1086;&#1080;&#1090; &#1085;&#1072; &#1075;&#1086;&#1088;&#1077;",
    b"<span lang=\"id\">saya suka makan nasi goreng</span> <i>setiap hari</i>",
    "<p>Ελληνικά κείμενο</p> <b>ภาษาไทย</b> &amp; ქართული".encode(),
    "<div class='a > b'>русский текст здесь</div> и ещё &lt;немного&gt;".encode(),
]


def short_documents(golden):
    """Case 1 (k_wave): documents of at most 256 bytes -- the reference's unit-test strings
    and the mixed tweets of flag_docs (where ScoreAsQuads and BestEffort are known to
    matter), 100 C2 tweets, and short pages."""
    fd = [d for d in flag_docs(golden) if len(d) <= 256]
    mixed = fd[-100:]                                          # a few words each of several languages
    units = [cut(d, 256) for d in flag_docs(golden)[:80]]      # the unit-test strings, cut to k_wave's size
    b, o = corpus.c2(100)
    docs = units + mixed + fd[100:260] + docs_of(b, o) + SNIPPETS * 6
    docs = [d for d in docs if leads_free(d)]
    assert max(len(d) for d in docs) <= 256
    return docs, assign_modes(len(docs), 0xD0C1)


def script_units(golden):
    """The reference's unit-test strings in scripts that are scored by the script alone
    (Armenian, Cherokee, Thaana, Georgian, Greek, ...: the 20 that follow the English
    one), which ScoreAsQuads sends to the quadgram path (scoreonescriptspan.cc:1318-1320)."""
    docs = [bytes.fromhex(t["text_hex"]) for t in golden["test_pairs"]]
    return [d for d in docs if leads_free(d)][1:21]


def with_unit_text(doc, unit, size=1500):
    """doc with about size bytes of a unit-test string in its middle."""
    at = doc.find(b" ", len(doc) // 2)
    if at < 0:
        return doc
    piece = b" ".join([unit] * (size // (len(unit) + 1) + 1))
    return doc[:at] + b" " + cut(piece, size) + doc[at:]


def fused_pages(golden):
    """Case 2 (the fused k_long): 48 pages of C3, so the long list is at most 64; every
    other one with markup, two of three with unit-test text."""
    b, o = corpus.c3(48)
    units = script_units(golden)
    docs = docs_of(b, o)
    docs = [with_unit_text(d, units[i % len(units)]) if i % 3 != 2 else d for i, d in enumerate(docs)]
    docs = [page_of(d) if i % 2 else d for i, d in enumerate(docs)]
    return docs, assign_modes(len(docs), 0xD0C2)


def many_span_documents(units, n=24, big=8):
    """Documents of hundreds of spans, the first `big` of them of more than 2,000 (the
    span-parallel groups of the staged path: more than 48 spans, in a batch of pages more
    than 2,000): the words of four-script pages, of a unit-test string and of a few
    tweets, shuffled, so that scripts alternate every word or few."""
    rng = np.random.default_rng(0xD0C9)
    b, o = corpus.c3(n, seed=175, page=8192)
    bb, ob = corpus.c3(big, seed=176, page=40960)
    b2, o2 = corpus.c2(8 * n, seed=508)
    pages, tw = docs_of(bb, ob) + docs_of(b, o)[big:], docs_of(b2, o2)
    out = []
    for k, d in enumerate(pages):
        # (with a few words each of eight tweets: languages of small percents, where BestEffort matters)
        w = d.split()
        few = b" ".join(cut(x, 40) for x in tw[8 * k:8 * k + 8]).split()
        if k < big:
            w += units[k % len(units)].split() * 30 + few * 6
        else:
            w = w[:600] + units[k % len(units)].split() * 4 + few
        rng.shuffle(w)
        out.append(b" ".join(w if k < big else w[:int(rng.integers(len(w) // 2, len(w)))]))
    return out


def staged_documents(golden):
    """Case 3 (the staged path with span-parallel groups): C3 pages and one C5 request,
    more than 64 long documents; every third one with markup, every fourth with
    unit-test text; in front of them 24 many-span documents, eight of them of more
    than 2,000 spans."""
    b3, o3 = corpus.c3(300)
    b5, o5 = corpus.c5(1000)
    units = script_units(golden)
    docs = docs_of(b3, o3) + docs_of(b5, o5)
    docs = [with_unit_text(d, units[i % len(units)], 600) if i % 4 == 0 else d for i, d in enumerate(docs)]
    docs = [page_of(d, every=5) if i % 3 == 0 else d for i, d in enumerate(docs)]
    docs = many_span_documents(units) + docs
    docs = [d for d in docs if leads_free(d)]
    return docs, assign_modes(len(docs), 0xD0C3)


def sequential_documents(golden):
    """Case 4 (the sequential span source, cld_seq.hip): the documents of test_gpu_seq.py
    the reference is defined on -- blocks of words wider than the LDS window, one 20 KB
    word, ordinary tweets; not the ones with malformed UTF-8, on which the reference's
    unchecked entries are undefined (compact_lang_det.h:74) and differ from the oracle
    that test uses -- with characters whose lowercase form has another length, and pages
    the HTML rewrite does not take; every third document ends in a unit-test string."""
    import cld_amd
    from test_gpu_seq import seq_docs
    rng = np.random.default_rng(8)
    docs = [d for d in seq_docs(rng, big=False, ordinary=120) if cld_amd.valid_prefix_host(d) == len(d)]
    b2, o2 = corpus.c2(200, seed=33)
    tw = docs_of(b2, o2)
    longer = ["İstanbul'da KIŞ İZMİR İYİ ", "Ⱥ Ⱦ ȺȺȺ ȾȾȾ ", "İİİ ȺȾȺ "]      # lowercase forms one byte longer
    for k in range(24):
        docs.append((longer[k % 3] * (3 + k)).encode() + b" ".join(tw[4 * k:4 * k + 4 + k]))
    for k in range(24):                                        # unrewritable pages: HTML lowering differs
        docs.append(b"<p lang=tr>" + ("İstanbul &#304;zmir " * (2 + k)).encode() + b"<b>" +
                    b" ".join(tw[100 + 3 * k:103 + 3 * k + k]) + b"</b> caf&eacute;</p>")
    units = script_units(golden)
    docs = [d + b" " + units[i % len(units)] if i % 3 == 0 else d for i, d in enumerate(docs)]
    order = rng.permutation(len(docs))
    docs = [docs[i] for i in order]
    return docs, assign_modes(len(docs), 0xD0C4)


def lang_pages():
    """Pages whose only lang= attribute lies inside the first 8 KB (the scan window,
    compact_lang_det_impl.cc:1596-1611), and twins whose attribute lies just behind it."""
    v = corpus.vocab()
    out = []
    for k, (tag, lang) in enumerate((("id", "ms"), ("ms", "id"), ("hr", "sr"), ("da", "no"), ("gl", "es"), ("sk", "cs"))):
        words = b" ".join(v[lang][i % len(v[lang])] for i in range(17 * k, 17 * k + 1800))
        head, tail = words[:8100 - 40 * k], words[8100 - 40 * k:]
        mark = b" <span lang=\"" + tag.encode() + b"\">x</span> "
        out.append(head[:head.rfind(b" ")] + mark + tail)                  # attribute inside the window
        out.append(words[:8200] + mark + words[8200:])                     # attribute behind it
    return out


def html_mix(gpu, golden, with_hints):
    """Case 5: 300 HTML pages (every fourth with unit-test text), half of them flagged HTML
    by the shuffle and half plain; 100 tweets, an empty document and the lang= pages
    flagged HTML."""
    hb, ho = corpus.html(300)
    b2, o2 = corpus.c2(100, seed=77)
    pages, tweets, lp = docs_of(hb, ho), docs_of(b2, o2), lang_pages()
    units = script_units(golden)
    pages = [with_unit_text(d, units[i % len(units)], 300) if i % 4 == 0 else d for i, d in enumerate(pages)]
    docs = pages + tweets + [b""] + lp
    words = assign_modes(len(docs), 0xD0C5)
    words[len(pages):] |= HTML
    keep = [i for i, d in enumerate(docs) if leads_free(d)]
    docs, words = [docs[i] for i in keep], words[keep]
    hints = random_hints(gpu, len(docs), 0xD0C6) if with_hints else None
    return docs, words, hints


def reference_rows(ref, buf, offs, words, hints=None, threads=16):
    """The reference's answer for every document under its own mode."""
    words = np.asarray(words, dtype=np.uint32)
    plain = ((words & HTML) == 0).astype(np.uint8)
    out = None
    for f in np.unique(words & CLD2):
        r = ref.detect_batch(buf, offs, plain=plain, hints=hints, threads=threads, flags=int(f))
        out = r.copy() if out is None else out
        sel = (words & CLD2) == f
        out[sel] = r[sel]
    return out


def reference_vectors(ref, buf, offs, words, threads=16):
    """(results, per-document chunk lists) of the reference in vector mode, each document under its own mode."""
    words = np.asarray(words, dtype=np.uint32)
    n = len(offs) - 1
    plain = ((words & HTML) == 0).astype(np.uint8)
    res, vec = None, [None] * n
    for f in np.unique(words & CLD2):
        r, ch, co = ref.detect_batch_vec(buf, offs, plain=plain, threads=threads, flags=int(f))
        res = r.copy() if res is None else res
        for i in np.nonzero((words & CLD2) == f)[0]:
            res[i] = r[i]
            vec[i] = ch[int(co[i]):int(co[i + 1])]
    return res, vec


def differs(a, b):
    n = len(a)
    bad = np.zeros(n, bool)
    for f in FIELDS:
        bad |= (a[f].astype(np.float64) != b[f].astype(np.float64)).reshape(n, -1).any(axis=1)
    return bad


def assert_modes_matter(ref, buf, offs, words, want, hints, what):
    """The condition on the inputs: every non-zero mode occurs, and for each of them some
    document's reference result under its own mode differs from its result under mode 0
    (plain text, flags 0) -- computed from the reference alone."""
    n = len(offs) - 1
    base = ref.detect_batch(buf, offs, plain=np.ones(n, np.uint8), hints=hints, threads=16, flags=0)
    moved = differs(want, base)
    counts = {}
    for w in MODE_WORDS[1:]:
        sel = np.asarray(words) == w
        assert sel.any(), "%s: no document has mode %#x" % (what, w)
        counts[int(w)] = int(moved[sel].sum())
        assert counts[int(w)] >= 1, "%s: mode %#x changes no document's reference result" % (what, w)
    return counts
