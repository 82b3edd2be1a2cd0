"""The host side of lexicon-constrained recognition: decode.Lexicon's encoding
and validation, the Recognizer's lexicon argument, and the pickling of what
crosses the ReplicaPool's queues. Nothing is launched."""
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cnn_lstm_ctc_ocr_amd import mjsynth
from cnn_lstm_ctc_ocr_amd.decode import Lexicon
from cnn_lstm_ctc_ocr_amd.server import LexiconRecognition, Recognition, Recognizer, gpu_recognizer

WORDS = ["Impeaching", "a", "supremacy", "to be, or not?", "AA", mjsynth.out_charset[::-1][:40]]


def _stub_store():
    """What Recognizer.__init__ reads of a ParamStore."""
    return SimpleNamespace(cfg=SimpleNamespace(dtype=torch.float32), device=torch.device("cpu"), version=0)


def test_encoding_is_mjsynth_encode():
    lex = Lexicon(WORDS)
    assert len(lex) == len(WORDS) and lex.words == tuple(WORDS)
    lab, ln = lex.tensors("cpu")
    assert lab.dtype == torch.int32 and ln.dtype == torch.int32
    assert tuple(lab.shape) == (len(WORDS), max(map(len, WORDS))) and lab.is_contiguous()
    for i, w in enumerate(WORDS):
        assert ln[i].item() == len(w)
        assert lab[i, :len(w)].tolist() == mjsynth.encode(w)
        assert lab[i, len(w):].tolist() == [0] * (lab.shape[1] - len(w))
    assert int(lab.max()) < mjsynth.num_classes()         # never the blank
    assert lex.tensors("cpu")[0] is lab                    # cached per device
    assert Lexicon(iter(WORDS)).words == tuple(WORDS)      # any iterable of strings


@pytest.mark.parametrize("words, match", [
    ([], "empty"),
    (["ab", ""], "empty string"),
    (["ab", "café"], "outside the charset"),
    (["ab", "tab\there"], "outside the charset"),
    (["ab", "cd", "ab"], "duplicate"),
    (["ab", "x" * 256], "256 characters"),
    (["ab", 7], "not a string"),
])
def test_bad_word_lists_raise(words, match):
    with pytest.raises(ValueError, match=match):
        Lexicon(words)


def test_longest_word_allowed():
    assert Lexicon(["x" * 255]).tensors("cpu")[0].shape == (1, 255)


def test_lexicon_pickles_as_strings():
    lex = Lexicon(WORDS)
    lex.tensors("cpu")
    assert lex.__reduce__() == (Lexicon, (WORDS,))
    back = pickle.loads(pickle.dumps(lex))
    assert back.words == lex.words
    np.testing.assert_array_equal(back.labels, lex.labels)
    np.testing.assert_array_equal(back.lengths, lex.lengths)


def test_recognizer_lexicon_argument():
    store = _stub_store()
    assert Recognizer(store).lexicon is None
    lex = Lexicon(WORDS)
    assert Recognizer(store, lexicon=lex).lexicon is lex
    r = Recognizer(store, lexicon=tuple(WORDS), lexicon_top=3)
    assert isinstance(r.lexicon, Lexicon) and r.lexicon.words == tuple(WORDS) and r.lexicon_top == 3
    for bad in (7, 1.5, {"ab": 1}, {"ab", "cd"}, (w for w in WORDS), "abc"):
        with pytest.raises(TypeError, match="lexicon"):
            Recognizer(store, lexicon=bad)
    with pytest.raises(ValueError, match="duplicate"):
        Recognizer(store, lexicon=["ab", "ab"])
    for bad in (0, 33):
        with pytest.raises(ValueError, match="lexicon_top"):
            Recognizer(store, lexicon=lex, lexicon_top=bad)


def test_factory_carries_the_lexicon_as_strings():
    f = gpu_recognizer(lexicon=Lexicon(WORDS), lexicon_top=5, detail=True)
    assert f.lexicon == WORDS and type(f.lexicon) is list
    g = pickle.loads(pickle.dumps(f))
    assert g.lexicon == WORDS and g.lexicon_top == 5 and g.detail is True
    assert gpu_recognizer(lexicon=WORDS).lexicon == WORDS
    assert gpu_recognizer().lexicon is None
    with pytest.raises(ValueError, match="duplicate"):
        gpu_recognizer(lexicon=["ab", "ab"])


def test_bad_scalar_arguments_launch_nothing():
    """The entry's argument checks, with no device pointer in sight (tests/test_abi.py's way)."""
    from cnn_lstm_ctc_ocr_amd import _lib

    def score(T=125, B=64, C=96, n_words=1000, max_word_len=12, top_k=1, ws_bytes=1 << 40):
        _lib.call("ocrk_ctc_lexicon_score", None, None, T, B, C, None, None, n_words, max_word_len, top_k, None, None,
                  None, None, None, None, None, ws_bytes, None)

    for kwargs, match in [(dict(T=0), "T=0"), (dict(T=4097), "T=4097"), (dict(C=257), "C=257"), (dict(C=1), "C=1"),
                          (dict(n_words=0), "n_words=0"), (dict(n_words=(1 << 20) + 1), "n_words="),
                          (dict(max_word_len=256), "max_word_len=256"), (dict(max_word_len=-1), "max_word_len=-1"),
                          (dict(top_k=0), "top_k=0"), (dict(top_k=33), "top_k=33"), (dict(B=-1), "B=-1"),
                          (dict(ws_bytes=1024), "workspace too small"), (dict(), "null pointer")]:
        with pytest.raises(_lib.InvalidArgumentError, match=match):
            score(**kwargs)
    size = _lib.lib().ocrk_ctc_lexicon_workspace_size
    # the normalised frames, one int per word, a [B][n_words] score buffer
    assert size(125, 64, 96, 1000, 12) == 125 * 64 * 96 * 4 + 1000 * 4 + 64 * 1000 * 4
    assert size(0, 64, 96, 1000, 12) == 0 and size(125, 64, 96, 0, 12) == 0 and size(125, 64, 96, 10, 256) == 0


def test_lexicon_recognition_pickles():
    r = LexiconRecognition("ab", 0.5, 0.9, (("ab", -0.6931), ("cd", -3.0)), (0.9, 0.8), ((2.5, 6.5), (6.5, 10.5)))
    back = pickle.loads(pickle.dumps(r))
    assert back == r and type(back) is LexiconRecognition
    assert back.text == "ab" and back.alternatives[1] == ("cd", -3.0) and back.lexicon_posterior == 0.9
    assert Recognition._fields == ("text", "confidence", "char_confidence", "char_px")   # untouched
