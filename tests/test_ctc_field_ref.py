"""tests/ctc_field_ref.py (the NumPy restatement of ocrk_ctc_field's recursion
the GPU tests compare with bit for bit) against enumeration of the pattern's
language through the already pinned tests/ctc_spot_ref.py, and the host side of
field reading: decode.FieldSet's grammar and limits, pickling, and the
Recognizer's and the replica factory's arguments. Nothing is launched."""
import math
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ctc_field_ref as F
import ctc_spot_ref as R
from cnn_lstm_ctc_ocr_amd import mjsynth
from cnn_lstm_ctc_ocr_amd.decode import FieldSet, KeywordSet, compile_field
from cnn_lstm_ctc_ocr_amd.server import (FieldHit, FieldRecognition, KeywordHit, KeywordRecognition, Recognition,
                                         Recognizer, gpu_recognizer)

C = 5
PATTERNS = F.SMALL_PATTERNS


def _logits(rng, kind, L):
    """The two kinds of tests/test_gpu_ctc_spot.py: ReLU'd small integers (exact ties everywhere) or Gaussian."""
    if kind == "int":
        return np.maximum(rng.integers(-3, 4, (L, C)), 0).astype(np.float32)
    return np.maximum(rng.standard_normal((L, C)) * 3, 0).astype(np.float32)


def test_recursion_equals_enumeration_of_the_language():
    rng = np.random.default_rng(3)
    cases = feasible = unique = 0
    for _draw in range(3):
        for kind in ("int", "gauss"):
            for L in range(1, 11):
                row = _logits(rng, kind, L)
                spots = {}                                               # string -> spot(row, string), shared
                for cls, opt in PATTERNS:
                    cases += 1
                    score, first, end, text = F.field(row, cls, opt)
                    strings = set(F.language(cls, opt))
                    for s in strings - spots.keys():
                        spots[s] = R.spot(row, list(s))
                    want = max(spots[s][0] for s in strings)
                    # (a) the score is the best of the language, bytewise
                    assert np.float32(score).tobytes() == np.float32(want).tobytes(), (cls, opt, L)
                    if np.isneginf(want):
                        assert (first, end) == (-1, -1) and text == (-1,) * len(cls)
                        continue
                    feasible += 1
                    assert score <= 0 and 0 <= first < end <= L
                    assert all(t == -1 or t in c for t, c in zip(text, cls))
                    assert all(t >= 0 for t, o in zip(text, opt) if not o)
                    best = [s for s in strings if spots[s][0] == want]
                    # (b) the text is one of the maximising strings
                    assert tuple(t for t in text if t >= 0) in best
                    if len(best) == 1:
                        # (c) a unique maximiser: its start, and an end no earlier than its first end
                        unique += 1
                        assert first == spots[best[0]][1] and end >= spots[best[0]][2]
                    if all(len(c) == 1 for c in cls) and not any(opt):
                        # (d) one string: the spotter's score bytewise and its start
                        (only,) = strings
                        assert np.float32(score).tobytes() == np.float32(spots[only][0]).tobytes()
                        assert first == spots[only][1]
    assert cases == 480 and feasible >= 400
    assert 3 * unique >= feasible                                        # the text check (c) is not vacuous


def test_planted_strings_score_zero_and_extend():
    logits = np.zeros((8, C), np.float32)
    for t, c in enumerate([4, 1, 1, 4, 2, 0, 4, 4]):                     # greedy path ". 1 1 . 2 0 . ."
        logits[t, c] = 1.0
    assert F.field(logits, [[1], [0, 2]], [0, 1]) == (0.0, 1, 5, (1, 2))  # "1" ends at 2, then extends over "2"
    assert F.field(logits, [[1, 2], [0]], [0, 0]) == (0.0, 4, 6, (2, 0))
    assert F.field(logits, [[1], [1]], [0, 0])[0] < 0                    # "11" needs a blank between
    assert F.field(logits, [[3]], [0])[0] == -1.0


def test_infeasible_patterns():
    logits = np.zeros((2, C), np.float32)
    for cls, opt in [([[0], [1], [2]], [0, 0, 0]), ([[1], [1]], [0, 0]), ([[0, 1], [2], [3], [0]], [0, 0, 0, 1])]:
        score, first, end, text = F.field(logits, cls, opt)
        assert np.isneginf(score) and (first, end) == (-1, -1) and text == (-1,) * len(cls)
    score, span, text = F.field_batch(np.zeros((3, 2, C), np.float32), [3, 0], [([[0]], [0]), ([[0]] * 3, [0] * 3)])
    assert score.tolist() == [[0.0, -np.inf], [-np.inf, -np.inf]]
    # all ties: the hit keeps its start and extends for as long as the score stays equal
    assert span.tolist() == [[[0, 3], [-1, -1]], [[-1, -1], [-1, -1]]]
    assert text.tolist() == [[[0, -1, -1], [-1, -1, -1]], [[-1, -1, -1], [-1, -1, -1]]]


# ------------------------------------------------------------------ the grammar
def _labels(chars):
    return sorted(mjsynth.out_charset.index(c) for c in chars)


DIGITS = "0123456789"


@pytest.mark.parametrize("pattern, classes, optional", [
    ("TOTAL", ["T", "O", "T", "A", "L"], [0, 0, 0, 0, 0]),
    (r"\d\.\d\d", [DIGITS, ".", DIGITS, DIGITS], [0, 0, 0, 0]),
    (r"[1-9]\d{0,3}\.\d{1,2}", ["123456789"] + [DIGITS] * 3 + ["."] + [DIGITS] * 2, [0, 1, 1, 1, 0, 0, 1]),
    (r"[1-9]\d?\.\d\d", ["123456789", DIGITS, ".", DIGITS, DIGITS], [0, 1, 0, 0, 0]),
    (r"a{3}", ["a", "a", "a"], [0, 0, 0]),
    (r"a{2,4}b?", ["a"] * 4 + ["b"], [0, 0, 1, 1, 1]),
    (r"x{1,1}y{0}z", ["x", "z"], [0, 0]),
    (r"[a-cX\]\-]", ["abcX]-"], [0]),
    (r"[\d#]-", [DIGITS + "#", "-"], [0, 0]),
    (r"[a-]b", ["a-", "b"], [0, 0]),
    (r"\$\(\)\|\^\*\+\?\{\}\[\\", list("$()|^*+?{}[\\"), [0] * 12),
    (r"No\. [0-9a-f]{4}", ["N", "o", ".", " "] + ["0123456789abcdef"] * 4, [0] * 8),
    ("a" * 16, ["a"] * 16, [0] * 16),
])
def test_accepted_spellings(pattern, classes, optional):
    cls, opt = compile_field("f", pattern)
    assert cls == [_labels(c) for c in classes]
    assert [int(o) for o in opt] == optional


@pytest.mark.parametrize("pattern, match", [
    ("a.b", "unsupported"), ("a*", "unsupported"), ("a+", "unsupported"), ("(ab)", "unsupported"),
    ("a|b", "unsupported"), ("^a", "unsupported"), ("a$", "unsupported"), ("[^a]", "unsupported"),
    (r"\w", "unsupported"), (r"\s", "unsupported"),
    ("a]", "stray"), ("a}", "stray"), ("?a", "stray"), ("a??", "stray"), ("{2}", "stray"),
    ("[ab", "unterminated"), ("[]", "empty class"), ("[a.b]", "inside a class"), ("[z-a]", "bad range"),
    ("a\\", "backslash"),
    ("a{,2}", "bad quantifier"), ("a{2", "bad quantifier"), ("a{x}", "bad quantifier"), ("a{1,2,3}", "bad quantifier"),
    ("a{3,2}", "m <= n"), ("a{0,4}", "m <= n"), ("ab{1,5}", "m <= n"),
    ("", "0 positions"), ("a{0}", "0 positions"), ("a" * 17, "17 positions"), (r"\d{16}a", "17 positions"),
    ("[a-q]", "17 characters"), (r"[\da-g]", "17 characters"),
    ("a?b", "begins with an optional"), ("a{0,2}b", "begins with an optional"),
    ("ab?c?d?e?f", "optional positions in a row"), (r"a\d{0,3}b?", "optional positions in a row"),
    ("café", "outside the charset"), ("a\tb", "outside the charset"), ("[aé]", "outside the charset"),
])
def test_rejected_spellings(pattern, match):
    with pytest.raises(ValueError, match=match) as err:
        FieldSet({"amount": "1", "the field": pattern})
    assert "'the field'" in str(err.value)                               # the message names the pattern


def test_field_set_tensors():
    fs = FieldSet({"amount": r"[1-9]\d{0,3}\.\d{1,2}", "gst": r"\d\.\d\d"})
    assert len(fs) == 2 and fs.names == ("amount", "gst")
    cls, opt, ln = fs.tensors("cpu")
    assert cls.dtype == opt.dtype == ln.dtype == torch.int32
    assert tuple(cls.shape) == (2, 7, 16) and tuple(opt.shape) == (2, 7) and ln.tolist() == [7, 4]
    assert cls[0, 0].tolist() == _labels("123456789") + [-1] * 7
    assert cls[1, 1].tolist() == _labels(".") + [-1] * 15
    assert bool((cls[1, 4:] == -1).all())                                # past the pattern's end
    assert opt.tolist() == [[0, 1, 1, 1, 0, 0, 1], [0] * 7]
    assert int(cls.max()) < mjsynth.num_classes()                        # never the blank
    assert fs.tensors("cpu")[0] is cls                                   # cached per device
    for c, o in fs.compiled:                                             # what the C entry asks of a pattern
        assert F.structure_ok(o) and all(sorted(set(x)) == x and 1 <= len(x) <= 16 for x in c)
    assert fs.strings([[mjsynth.encode("12") + [-1] + mjsynth.encode(".5") + [-1, -1]], [[-1] * 7]]) == [["12.5"], [""]]
    with pytest.raises(ValueError, match="empty"):
        FieldSet({})
    with pytest.raises(TypeError, match="mapping"):
        FieldSet([r"\d"])
    with pytest.raises(ValueError, match="not a string"):
        FieldSet({"a": 7})


def test_field_set_pickles_as_its_mapping():
    patterns = {"amount": r"[1-9]\d{0,3}\.\d{1,2}", "no": r"#\d{4,6}"}
    fs = FieldSet(patterns)
    fs.tensors("cpu")
    assert fs.__reduce__() == (FieldSet, (patterns,))
    back = pickle.loads(pickle.dumps(fs))
    assert back.patterns == patterns and back.names == fs.names and back.compiled == fs.compiled
    np.testing.assert_array_equal(back.classes, fs.classes)
    np.testing.assert_array_equal(back.optional, fs.optional)
    np.testing.assert_array_equal(back.lengths, fs.lengths)


def _stub_store():
    """What Recognizer.__init__ reads of a ParamStore."""
    return SimpleNamespace(cfg=SimpleNamespace(dtype=torch.float32), device=torch.device("cpu"), version=0)


def test_recognizer_field_arguments():
    store = _stub_store()
    r = Recognizer(store)
    assert r.fields is None and r.field_threshold == math.log(0.5)
    fs = FieldSet({"gst": r"\d\.\d\d"})
    assert Recognizer(store, fields=fs).fields is fs
    r = Recognizer(store, fields={"gst": r"\d\.\d\d"}, field_threshold=-3, keywords=["TOTAL"], detail=True)
    assert isinstance(r.fields, FieldSet) and r.fields.names == ("gst",) and r.field_threshold == -3.0
    assert isinstance(r.keywords, KeywordSet)
    for bad in (7, [r"\d"], "abc", {r"\d"}):
        with pytest.raises(TypeError, match="fields"):
            Recognizer(store, fields=bad)
    with pytest.raises(ValueError, match="unsupported"):
        Recognizer(store, fields={"a": "x+"})
    for bad in (1e-6, 1, float("nan")):
        with pytest.raises(ValueError, match="field_threshold"):
            Recognizer(store, fields=fs, field_threshold=bad)
    for lex in (["ab", "cd"],):
        with pytest.raises(ValueError, match="fields and lexicon"):
            Recognizer(store, fields=fs, lexicon=lex)


def test_factory_carries_the_fields_as_a_mapping():
    patterns = {"gst": r"\d\.\d\d"}
    f = gpu_recognizer(fields=FieldSet(patterns), field_threshold=-2.5, keywords=["TOTAL"])
    assert f.fields == patterns and type(f.fields) is dict and f.field_threshold == -2.5 and f.keywords == ["TOTAL"]
    g = pickle.loads(pickle.dumps(f))
    assert g.fields == patterns and g.field_threshold == -2.5
    assert gpu_recognizer(fields=patterns).field_threshold == math.log(0.5)
    assert gpu_recognizer().fields is None
    with pytest.raises(ValueError, match="unsupported"):                 # checked in the parent
        gpu_recognizer(fields={"a": "(x)"})
    with pytest.raises(ValueError, match="field_threshold"):
        gpu_recognizer(fields=patterns, field_threshold=0.5)
    with pytest.raises(ValueError, match="fields and lexicon"):
        gpu_recognizer(fields=patterns, lexicon=["ab"])
    with pytest.raises(TypeError, match="fields"):
        gpu_recognizer(fields=[r"\d"])


def test_field_recognition_pickles():
    hit = FieldHit("amount", "112.50", -0.25, 10, 18, 22.5, 38.5)
    kw = KeywordHit("TOTAL", 0.0, 3, 9, 8.5, 20.5)
    det = Recognition("TOTAL $112.50", 0.5, (0.9,) * 13, ((0.0, 1.0),) * 13)
    for r in (FieldRecognition("TOTAL $112.50", None, (), (hit,)), FieldRecognition("TOTAL $112.50", det, (kw,), ())):
        back = pickle.loads(pickle.dumps(r))
        assert back == r and type(back) is FieldRecognition
    assert all(type(v) in (str, float, int) for v in hit)
    assert FieldHit._fields == ("name", "text", "score", "first_frame", "end_frame", "x0", "x1")
    assert FieldRecognition._fields == ("text", "detail", "hits", "fields")
    assert KeywordRecognition._fields == ("text", "detail", "hits")      # untouched


def test_bad_scalar_arguments_launch_nothing():
    """The entry's argument checks, with no device pointer in sight (tests/test_abi.py's way)."""
    from cnn_lstm_ctc_ocr_amd import _lib

    def field(T=125, B=64, C=96, n_pat=8, max_pat_len=7, ws_bytes=1 << 40):
        _lib.call("ocrk_ctc_field", None, None, T, B, C, None, None, None, n_pat, max_pat_len, None, None, None, None,
                  None, None, ws_bytes, None)

    for kwargs, match in [(dict(T=0), "T=0"), (dict(T=4097), "T=4097"), (dict(C=257), "C=257"), (dict(C=1), "C=1"),
                          (dict(B=-1), "B=-1"), (dict(B=65536), "B=65536"), (dict(n_pat=0), "n_pat=0"),
                          (dict(n_pat=(1 << 20) + 1), "n_pat="), (dict(max_pat_len=0), "max_pat_len=0"),
                          (dict(max_pat_len=256), "max_pat_len=256"), (dict(ws_bytes=1024), "workspace too small"),
                          (dict(), "null pointer")]:
        with pytest.raises(_lib.InvalidArgumentError, match=match):
            field(**kwargs)
    field(B=0)                                             # an empty batch is no error and touches nothing
    size = _lib.lib().ocrk_ctc_field_workspace_size
    assert size(125, 64, 96, 8, 7) == 125 * 64 * 96 * 4 + 32           # the rel table and one int per pattern
    assert size(125, 64, 96, 41, 16) == 125 * 64 * 96 * 4 + 176         # rounded to 16 B
    assert size(0, 64, 96, 8, 7) == 0 and size(125, 64, 96, 0, 7) == 0 and size(125, 64, 96, 8, 256) == 0
