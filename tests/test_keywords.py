"""The host side of keyword spotting: decode.KeywordSet's encoding, case folding
and validation, the Recognizer's and the replica factory's keyword arguments,
the pickling of what crosses the ReplicaPool's queues, and the C entry's
argument checks. Nothing is launched."""
import math
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cnn_lstm_ctc_ocr_amd import mjsynth
from cnn_lstm_ctc_ocr_amd.decode import KeywordSet, Lexicon
from cnn_lstm_ctc_ocr_amd.server import (KeywordHit, KeywordRecognition, LexiconRecognition, Recognition, Recognizer,
                                         gpu_recognizer)

KEYWORDS = ["TOTAL", "gst", "Change Due", "receipt no.", "a", "x" * 32]


def _stub_store():
    """What Recognizer.__init__ reads of a ParamStore."""
    return SimpleNamespace(cfg=SimpleNamespace(dtype=torch.float32), device=torch.device("cpu"), version=0)


def test_encoding_is_mjsynth_encode():
    ks = KeywordSet(KEYWORDS)
    assert len(ks) == len(KEYWORDS) and ks.keywords == tuple(KEYWORDS) and ks.case_insensitive is False
    lab, alt, ln = ks.tensors("cpu")
    assert alt is None                                     # case-sensitive: the entry gets no alternatives table
    assert lab.dtype == torch.int32 and ln.dtype == torch.int32
    assert tuple(lab.shape) == (len(KEYWORDS), 32) and lab.is_contiguous()
    for i, w in enumerate(KEYWORDS):
        assert ln[i].item() == len(w)
        assert lab[i, :len(w)].tolist() == mjsynth.encode(w)
        assert lab[i, len(w):].tolist() == [0] * (32 - len(w))
    assert int(lab.max()) < mjsynth.num_classes()          # never the blank
    assert np.all(ks.alternatives == -1)
    assert ks.tensors("cpu")[0] is lab                     # cached per device
    assert KeywordSet(iter(KEYWORDS)).keywords == tuple(KEYWORDS)


def test_case_folding_and_the_alternatives_table():
    ks = KeywordSet(["Total: 9", "gst"], case_insensitive=True)
    lab, alt, ln = ks.tensors("cpu")
    assert alt.dtype == torch.int32 and alt.shape == lab.shape == (2, 8) and ln.tolist() == [8, 3]
    assert lab[0].tolist() == mjsynth.encode("Total: 9")
    # a letter's alternative is its other case; ':', ' ' and '9' have none
    want = mjsynth.encode("tOTAL") + [-1, -1, -1]
    assert alt[0].tolist() == want
    assert alt[1].tolist() == mjsynth.encode("GST") + [-1] * 5          # -1 past the keyword's end too
    assert all(a != l for a, l in zip(alt[0, :5].tolist(), lab[0, :5].tolist()))
    # duplicates are judged after folding, and only then
    assert len(KeywordSet(["total", "TOTAL"])) == 2
    with pytest.raises(ValueError, match="duplicate"):
        KeywordSet(["total", "gst", "TOTAL"], case_insensitive=True)


@pytest.mark.parametrize("words, match", [
    ([], "empty"),
    (["ab", ""], "empty string"),
    (["ab", "café"], "outside the charset"),
    (["ab", "tab\there"], "outside the charset"),
    (["ab", "cd", "ab"], "duplicate"),
    (["ab", "x" * 33], "33 characters"),
    (["ab", 7], "not a string"),
])
def test_bad_keyword_lists_raise(words, match):
    for ci in (False, True):
        with pytest.raises(ValueError, match=match):
            KeywordSet(words, case_insensitive=ci)


@pytest.mark.parametrize("ci", [False, True])
def test_keyword_set_pickles_as_its_arguments(ci):
    ks = KeywordSet(KEYWORDS, case_insensitive=ci)
    ks.tensors("cpu")
    assert ks.__reduce__() == (KeywordSet, (KEYWORDS, ci))
    back = pickle.loads(pickle.dumps(ks))
    assert back.keywords == ks.keywords and back.case_insensitive is ci
    np.testing.assert_array_equal(back.labels, ks.labels)
    np.testing.assert_array_equal(back.alternatives, ks.alternatives)
    np.testing.assert_array_equal(back.lengths, ks.lengths)


def test_recognizer_keyword_arguments():
    store = _stub_store()
    r = Recognizer(store)
    assert r.keywords is None and r.keyword_threshold == math.log(0.5)
    ks = KeywordSet(KEYWORDS, case_insensitive=True)
    assert Recognizer(store, keywords=ks).keywords is ks
    r = Recognizer(store, keywords=tuple(KEYWORDS), keyword_threshold=-3, case_insensitive=True, detail=True)
    assert isinstance(r.keywords, KeywordSet) and r.keywords.keywords == tuple(KEYWORDS)
    assert r.keywords.case_insensitive is True and r.keyword_threshold == -3.0 and r.lexicon is None
    assert Recognizer(store, keywords=KEYWORDS).keywords.case_insensitive is False
    assert Recognizer(store, keywords=KEYWORDS, keyword_threshold=0).keyword_threshold == 0.0
    for bad in (7, 1.5, {"ab": 1}, {"ab", "cd"}, (w for w in KEYWORDS), "abc"):
        with pytest.raises(TypeError, match="keywords"):
            Recognizer(store, keywords=bad)
    with pytest.raises(ValueError, match="duplicate"):
        Recognizer(store, keywords=["ab", "AB"], case_insensitive=True)
    for bad in (1e-6, 1, float("nan")):
        with pytest.raises(ValueError, match="keyword_threshold"):
            Recognizer(store, keywords=ks, keyword_threshold=bad)
    for lex in (["ab", "cd"], Lexicon(["ab", "cd"])):
        with pytest.raises(ValueError, match="keywords and lexicon"):
            Recognizer(store, keywords=ks, lexicon=lex)


def test_factory_carries_the_keywords_as_strings():
    f = gpu_recognizer(keywords=KeywordSet(KEYWORDS, case_insensitive=True), keyword_threshold=-2.5, detail=True)
    assert f.keywords == KEYWORDS and type(f.keywords) is list and f.case_insensitive is True
    g = pickle.loads(pickle.dumps(f))
    assert g.keywords == KEYWORDS and g.case_insensitive is True and g.keyword_threshold == -2.5 and g.detail is True
    f = gpu_recognizer(keywords=KEYWORDS, case_insensitive=True)
    assert f.keywords == KEYWORDS and f.case_insensitive is True and f.keyword_threshold == math.log(0.5)
    assert gpu_recognizer(keywords=KEYWORDS).case_insensitive is False
    assert gpu_recognizer().keywords is None
    # checked in the parent, before anything is pickled or spawned
    with pytest.raises(ValueError, match="duplicate"):
        gpu_recognizer(keywords=["ab", "ab"])
    with pytest.raises(ValueError, match="keyword_threshold"):
        gpu_recognizer(keywords=KEYWORDS, keyword_threshold=0.5)
    with pytest.raises(ValueError, match="keywords and lexicon"):
        gpu_recognizer(keywords=KEYWORDS, lexicon=["ab"])
    with pytest.raises(TypeError, match="keywords"):
        gpu_recognizer(keywords="abc")


def test_keyword_recognition_pickles():
    hit = KeywordHit("TOTAL", -0.25, 4, 17, 10.5, 36.5)
    det = Recognition("SUB TOTAL 9", 0.5, (0.9,) * 11, ((0.0, 1.0),) * 11)
    for r in (KeywordRecognition("SUB TOTAL 9", None, (hit,)), KeywordRecognition("SUB TOTAL 9", det, ())):
        back = pickle.loads(pickle.dumps(r))
        assert back == r and type(back) is KeywordRecognition
    assert type(back.detail) is Recognition
    assert KeywordHit._fields == ("keyword", "score", "first_frame", "end_frame", "x0", "x1")
    assert KeywordRecognition._fields == ("text", "detail", "hits")
    # untouched
    assert Recognition._fields == ("text", "confidence", "char_confidence", "char_px")
    assert LexiconRecognition._fields[:3] == ("text", "confidence", "lexicon_posterior")


def test_bad_scalar_arguments_launch_nothing():
    """The entry's argument checks, with no device pointer in sight (tests/test_abi.py's way)."""
    from cnn_lstm_ctc_ocr_amd import _lib

    def spot(T=125, B=64, C=96, n_kw=64, max_kw_len=16, ws_bytes=1 << 40):
        _lib.call("ocrk_ctc_spot", None, None, T, B, C, None, None, None, n_kw, max_kw_len, None, None, None, None,
                  None, ws_bytes, None)

    for kwargs, match in [(dict(T=0), "T=0"), (dict(T=4097), "T=4097"), (dict(C=257), "C=257"), (dict(C=1), "C=1"),
                          (dict(B=-1), "B=-1"), (dict(B=65536), "B=65536"), (dict(n_kw=0), "n_kw=0"),
                          (dict(n_kw=(1 << 20) + 1), "n_kw="), (dict(max_kw_len=0), "max_kw_len=0"),
                          (dict(max_kw_len=256), "max_kw_len=256"), (dict(ws_bytes=1024), "workspace too small"),
                          (dict(), "null pointer")]:
        with pytest.raises(_lib.InvalidArgumentError, match=match):
            spot(**kwargs)
    spot(B=0)                                              # an empty batch is no error and touches nothing
    size = _lib.lib().ocrk_ctc_spot_workspace_size
    # the rel table and one int per keyword
    assert size(125, 64, 96, 64, 16) == 125 * 64 * 96 * 4 + 64 * 4
    assert size(125, 64, 96, 65, 40) == 125 * 64 * 96 * 4 + 272      # rounded to 16 B
    assert size(0, 64, 96, 64, 16) == 0 and size(125, 64, 96, 0, 16) == 0 and size(125, 64, 96, 10, 256) == 0
