"""text(page) judged by the reference CLD2 itself (CPU, oracle/refcld as
test_reference_pin.py uses it): for every page of corpus.html(64, emoji=0.25) the
reference's result on the page with is_plain_text = false equals its result on
text(page) (cld_html_text, which test_htmltext_host.py holds to the model) with
is_plain_text = true -- lang3, percent3, text_bytes, is_reliable, summary -- for
both flag values of the extraction.

Hints: the page-mode call takes none and makes its priors from the page's lang=
attributes, which do not survive the extraction.  The text-mode call is given
them explicitly, as the content-language hint that yields the same priors
(SetCLDContentLangHint and the lang= scan feed one SetCLDLangTagsHint,
compact_lang_det_hint_code.cc:1394-1442): the page's own <html lang="..."> value,
checked here against cld_hint_priors of the page for every page.  test_gpu_htmltext.py
handles the hints of its HTML-mode agreement test the same way.

Two exactness details of HTML mode are invisible in the text: a script lookahead
that lands on an entity (the scanner sees the raw '&', script 0, where the text
has the decoded letter) and the lowercaser's HTML half.  The generator's default
seed has one such page: page 38 of corpus.html(64, seed=0xC1D20006, emoji=0.25)
holds "b&#1044;", HTML mode keeps the decoded Cyrillic letter in the Latin span
and the text ends the span there (located by comparing the oracle's spans of the
page and of its text: they agree up to that byte).  So the seed is replaced
(htmltext_cases.CORPUS_SEED); with it the reference gives 0 differences on all
64 pages and no page is skipped.  All pages are under kMaxScriptBytes (40,928),
so the span soft limit plays no part."""
import os
import re

import numpy as np
import pytest

import cld_amd
import htmltext_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNTH = os.path.join(ROOT, "language-detector_amd", "data", "cld2_synth_q1.cldt")
FIELDS = ("lang3", "percent3", "text_bytes", "is_reliable", "summary_lang")


def _have_ref():
    import refcld
    return os.path.exists(refcld.LIB) or os.path.isdir("/root/reference/cld2/internal")


needs_ref = pytest.mark.skipif(not _have_ref(), reason="reference library not built and sources absent")


def page_hints(pages):
    """One Hints per page whose priors in plain-text mode equal the priors of the page in HTML mode."""
    hints = []
    for p in pages:
        want, _ = cld_amd.hint_priors(p, html=True)
        m = re.match(rb'<html lang="([^"]*)"', p)
        h = cld_amd.Hints.make(content_language=m.group(1)) if len(want) else None
        got, _ = cld_amd.hint_priors(b"", html=False, hints=h)
        assert got.tolist() == want.tolist(), "the content-language hint does not restate the page's lang= priors"
        hints.append(h)
    return hints


@needs_ref
@pytest.mark.parametrize("flags", [0, hc.BLOCK_LF])
def test_reference_reads_the_text_as_it_reads_the_page(flags):
    import refcld
    ref = refcld.instance(SYNTH)
    pages = hc.corpus_pages()
    assert len(pages) == 64 and max(map(len, pages)) < 40928
    buf, offs = hc.pack(pages)
    got = cld_amd.html_text(buf, offs, flags)
    texts = [bytes(got["out"][int(a):int(a) + int(k)]) for a, k in zip(offs[:-1], got["text_len"])]
    assert all(texts)
    hints = page_hints(pages)
    assert sum(h is not None for h in hints) > 32
    none = cld_amd.Hints.make()
    on_page = ref.detect_batch(buf, offs, plain=np.zeros(len(pages), np.uint8))
    tbuf, toffs = hc.pack(texts)
    on_text = ref.detect_batch(tbuf, toffs, plain=np.ones(len(pages), np.uint8), hints=[h or none for h in hints])
    bad = [i for i in range(len(pages))
           if any(on_page[f][i].tolist() != on_text[f][i].tolist() for f in FIELDS)]
    assert not bad, "pages %s: the reference reads the text differently from the page" % bad
    assert len(set(on_page["summary_lang"].tolist())) > 8, "the pages should be in many languages"
