"""The device-resident hint interface without a GPU: the record layout of
cld_hints_dev (include/cld_mi355x.h), pack_hints, and the argument checks of
cld_detect_batch_device_hints that come before any GPU is touched."""
import numpy as np
import pytest

from test_html_hints import hint_cases


def test_hints_dev_layout():
    import cld_amd
    d = cld_amd.HINTS_DEV_DTYPE
    assert d.itemsize == 20
    assert {k: d.fields[k][1] for k in d.names} == {"content_language_off": 0, "content_language_len": 4, "tld": 8,
                                                    "encoding_hint": 12, "language_hint": 16}
    assert d.fields["tld"][0].itemsize == 4


def test_pack_hints_round_trip():
    import cld_amd
    cases = hint_cases(8, 200)
    hints = [cld_amd.Hints.make(cl or None, tld or None, enc, lang) for _, cl, tld, enc, lang in cases]
    rec, text = cld_amd.pack_hints(hints, len(hints))
    assert rec.dtype == cld_amd.HINTS_DEV_DTYPE and rec.shape == (200,) and text.dtype == np.uint8
    raw = text.tobytes()
    seen = 0
    for r, (_, cl, tld, enc, lang) in zip(rec, cases):
        off, ln = int(r["content_language_off"]), int(r["content_language_len"])
        assert ln == len(cl)
        if cl:
            assert raw[off:off + ln] == cl and raw[off + ln] == 0      # each text ends in a NUL
            seen += 1
        assert r.tobytes()[8:12] == tld.ljust(4, b"\0")
        assert (int(r["encoding_hint"]), int(r["language_hint"])) == (enc, lang)
    assert seen > 50
    with pytest.raises(ValueError):
        cld_amd.pack_hints(hints, 199)
    # no hint: the reference's defaults
    rec, text = cld_amd.pack_hints([None, cld_amd.Hints.make()])
    assert len(text) == 0 and rec["content_language_len"].tolist() == [0, 0] and rec["tld"].tolist() == [b"", b""]
    assert rec["encoding_hint"].tolist() == [cld_amd.UNKNOWN_ENCODING] * 2
    assert rec["language_hint"].tolist() == [cld_amd.UNKNOWN_LANGUAGE] * 2
    # a TLD longer than 3 bytes stays marked as such
    rec, _ = cld_amd.pack_hints([cld_amd.Hints.make(tld="museum")])
    assert rec.tobytes()[8:12] == b"muse"


@pytest.mark.parametrize("flags", [1, 2, 8, 4 | 8, 0x10000, 1 << 31], ids=["strip_extras", "cstring", "check_utf8",
                                                                           "html_check_utf8", "unknown", "unknown31"])
def test_detect_batch_device_hints_rejects_flags(flags):
    """Preparation flags and unknown bits: CLD_EINVAL before cld_init, so also where no GPU is."""
    import cld_amd
    assert (cld_amd.FLAG_STRIP_EXTRAS, cld_amd.FLAG_CSTRING, cld_amd.FLAG_CHECK_UTF8) == (1, 2, 8)
    L = cld_amd.lib()
    assert L.cld_detect_batch_device_hints(0, None, None, 0, 0, None, None, 0, None, flags, None) == cld_amd.EINVAL
    with pytest.raises(cld_amd.CldError, match="%d" % cld_amd.EINVAL):
        cld_amd.detect_batch_device_hints(0, None, None, 0, 0, None, flags=flags)
