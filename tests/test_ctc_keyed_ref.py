"""tests/ctc_keyed_ref.py (the NumPy restatement of ocrk_ctc_keyed_field's
definition the GPU tests compare with bit for bit) against ctc_field_ref.field
and against brute-force enumeration of every keyword segment, gap, field
segment and frame labelling; the definition's tie and gap-cost rules; and the
host side of keyed fields: decode.KeyedFieldSet's validation and pickling, the
Recognizer's and the replica factory's arguments, the entry's argument checks.
Nothing is launched."""
import itertools
import math
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ctc_field_ref as FR
import ctc_keyed_ref as KR
from ctc_spot_ref import relative
from cnn_lstm_ctc_ocr_amd import mjsynth
from cnn_lstm_ctc_ocr_amd.decode import FieldSet, KeyedFieldSet, KeywordSet, compile_field
from cnn_lstm_ctc_ocr_amd.server import (FieldHit, FieldRecognition, KeyedHit, KeyedRecognition, KeywordHit,
                                         Recognition, Recognizer, gpu_recognizer)

F32 = np.float32
MAPPING = {"total": (["total", "amount", "ttl"], r"[1-9]\d{0,3}\.\d{1,2}"), "gst": (["gst", "G.S.T."], r"\d\.\d\d")}


def _stub_store():
    """What Recognizer.__init__ reads of a ParamStore."""
    return SimpleNamespace(cfg=SimpleNamespace(dtype=torch.float32), device=torch.device("cpu"), version=0)


def test_zero_entry_is_the_field_reader():
    rng = np.random.default_rng(5)
    n = 0
    for draw in range(4):
        for L in range(0, 9):
            row = np.maximum(rng.standard_normal((L, 5)) * 3, 0).astype(F32) if draw % 2 else \
                np.maximum(rng.integers(-3, 4, (L, 5)), 0).astype(F32)
            rel = relative(row) if L else row
            for cls, opt in FR.SMALL_PATTERNS:
                want = FR.field(row, cls, opt)
                got = KR.field_with_entry(rel, cls, opt, [F32(0)] * L)
                assert F32(got[0]).tobytes() == F32(want[0]).tobytes() and got[1:] == want[1:], (L, cls, opt)
                n += 1
    assert n == 4 * 9 * len(FR.SMALL_PATTERNS)


# ------------------------------------------------------------------ brute force
BRUTE_C = 4
BRUTE_PATTERNS = [([[0, 1]], [0]), ([[0], [1, 2]], [0, 1]), ([[2], [2]], [0, 0]), ([[1], [0, 2], [1]], [0, 1, 0])]
BRUTE_GROUPS = [[[0]], [[2, 2]], [[1, 2], [0]], [[0, 1], [1], [2, 0]]]     # one symbol, a repeat, groups of 2 and 3


def _collapse(path, blank):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return tuple(out)


def _brute(row, keywords, cls, opt, cost):
    """max over f < e <= g < h, every labelling of [f, e) and [g, h) with non-blank first and last frames, the
    first collapsing to a keyword and the second to a string of the language, of kw + field - cost (g - e).
    Every term is a multiple of 1/4: float64 sums are exact and equal the float32 ones."""
    L, C = row.shape
    rel = relative(row).astype(np.float64)
    lang = set(FR.language(cls, opt))
    kws = {tuple(k) for k in keywords}
    seg_kw, seg_f = {}, {}                                   # (a, b) -> the best keyword / language labelling
    for a in range(L):
        for b in range(a + 1, L + 1):
            bk = bf = -np.inf
            for path in itertools.product(range(C), repeat=b - a):
                if path[0] == C - 1 or path[-1] == C - 1:
                    continue
                s = _collapse(path, C - 1)
                if s in kws or s in lang:
                    v = sum(rel[a + i, c] for i, c in enumerate(path))
                    if s in kws:
                        bk = max(bk, v)
                    if s in lang:
                        bf = max(bf, v)
            seg_kw[a, b], seg_f[a, b] = bk, bf
    best = -np.inf
    for f in range(L):
        for e in range(f + 1, L + 1):
            for g in range(e, L):
                for h in range(g + 1, L + 1):
                    best = max(best, seg_kw[f, e] + seg_f[g, h] - cost * (g - e))
    return best


def test_helper_equals_brute_force():
    rng = np.random.default_rng(0)
    cases = feasible = 0
    for it in range(160):
        L = int(rng.integers(0, 7))
        row = (rng.integers(-8, 1, size=(L, BRUTE_C)) / 4).astype(F32)       # a grid of 1/4: every sum is exact
        cls, opt = BRUTE_PATTERNS[it % 4]
        keywords = BRUTE_GROUPS[(it // 4) % 4]
        cost = [0.0, 0.25][(it // 16) % 2]
        score, span, k, kw_score, text = KR.keyed(row, keywords, None, cls, opt, cost)
        want = _brute(row, keywords, cls, opt, cost) if L else -np.inf
        assert F32(score).tobytes() == F32(want).tobytes(), (it, L, score, want)
        cases += 1
        if np.isneginf(want):
            assert span == (-1, -1, -1, -1) and k == -1 and np.isneginf(kw_score) and text == (-1,) * len(cls)
            continue
        feasible += 1
        f, e, g, h = span
        assert 0 <= f < e <= g < h <= L and 0 <= k < len(keywords) and score <= kw_score <= 0
        assert tuple(x for x in text if x >= 0) in set(FR.language(cls, opt))
    assert cases >= 150 and 3 * feasible >= cases, (cases, feasible)


# -------------------------------------------------------------- the definition's rules
def _spell(frames, C, margin=4.0):
    """Logits whose argmax path is `frames` (labels, C - 1 the blank) with `margin` over the rest."""
    row = np.zeros((len(frames), C), F32)
    for t, c in enumerate(frames):
        row[t, c] = margin
    return row


def test_ties_go_to_the_leftmost_keyword_and_value():
    # "K 7 K 7" twice on the argmax path: keyword label 0, value label 1, blank 3
    b = 3
    frames = [0, b, 1, b, b, 0, b, 1, b]
    row = _spell(frames, 4)
    score, span, k, kw_score, text = KR.keyed(row, [[0]], None, [[1, 2]], [0], 0.0)
    assert score == 0 and kw_score == 0 and span == (0, 1, 2, 3) and k == 0 and text == (1,)
    # two keywords of the group, both spelled: the earliest-ending one, whatever its index
    frames = [2, b, 0, b, 1, b, 1]
    score, span, k, _kv, text = KR.keyed(_spell(frames, 4), [[0], [2]], None, [[1]], [0], 0.0)
    assert score == 0 and span == (0, 1, 4, 5) and k == 1
    # keyword and value may abut
    score, span, _k, _kv, _t = KR.keyed(_spell([0, 1], 4), [[0]], None, [[1]], [0], 0.5)
    assert score == 0 and span == (0, 1, 1, 2)


def test_gap_cost_prefers_the_near_value():
    # keyword 0, then a value (label 1) read slightly worse than the value further on
    b = 3
    frames = [0, b, 1, b, b, b, 1]
    row = _spell(frames, 4)
    row[2, 1] -= 0.5                                        # the near value: label 2 is the frame's argmax by 0.5
    row[2, 2] = row[2, 1] + 0.5
    far = KR.keyed(row, [[0]], None, [[1]], [0], 0.0)
    assert far[0] == 0 and far[1] == (0, 1, 6, 7)
    near = KR.keyed(row, [[0]], None, [[1]], [0], 0.25)
    assert near[1] == (0, 1, 2, 3) and near[0] == F32(-0.5) - F32(0.25)    # one frame of gap, then -0.5
    assert F32(-0.75) > F32(0) - 5 * F32(0.25)              # the far value would pay five frames of gap


# ------------------------------------------------------------------ KeyedFieldSet
def test_keyed_field_set_encodes_keyword_sets_and_patterns():
    for ci in (False, True):
        k = KeyedFieldSet(MAPPING, case_insensitive=ci)
        assert len(k) == 2 and k.names == ("total", "gst")
        assert k.keywords == ("total", "amount", "ttl", "gst", "G.S.T.") and k.groups.tolist() == [0, 0, 0, 1, 1]
        flat = KeywordSet(["total", "amount", "ttl", "gst", "G.S.T."], case_insensitive=ci)
        np.testing.assert_array_equal(k.labels, flat.labels)
        np.testing.assert_array_equal(k.alternatives, flat.alternatives)
        np.testing.assert_array_equal(k.kw_lengths, flat.lengths)
        fs = FieldSet({n: p for n, (_w, p) in MAPPING.items()})
        np.testing.assert_array_equal(k.classes, fs.classes)
        np.testing.assert_array_equal(k.optional, fs.optional)
        np.testing.assert_array_equal(k.lengths, fs.lengths)
        assert k.compiled == tuple(compile_field(n, p) for n, (_w, p) in MAPPING.items())
        t = k.tensors("cpu")
        assert k.tensors("cpu") is t and len(t) == 7 and (t[1] is None) == (not ci)
        assert all(x.dtype == torch.int32 for x in t if x is not None)
    assert k.strings(np.array([[mjsynth.out_charset.index("7"), -1, mjsynth.out_charset.index("5")]])) == ["75"]
    # a keyword may serve two fields; duplicates are judged within one
    both = KeyedFieldSet({"a": (["no"], r"\d"), "b": (["no", "nr"], r"\d\d")})
    assert both.keywords == ("no", "no", "nr") and both.groups.tolist() == [0, 1, 1]


@pytest.mark.parametrize("mapping, match", [
    ({}, "empty"),
    ({"a": ([], r"\d")}, "empty"),
    ({"a": (["ab", ""], r"\d")}, "empty string"),
    ({"a": (["café"], r"\d")}, "outside the charset"),
    ({"a": (["ab", "cd", "ab"], r"\d")}, "duplicate"),
    ({"a": (["x" * 33], r"\d")}, "33 characters"),
    ({"a": (["ab", 7], r"\d")}, "not a string"),
    ({"a": ("total", r"\d")}, "sequence of strings"),
    ({"a": (["ab"], r"\d", 3)}, "pair"),
    ({"a": r"\d"}, "pair"),
    ({"a": 7}, "pair"),
    ({7: (["ab"], r"\d")}, "not a string"),
    ({"a": (["ab"], 7)}, "not a string"),
    ({"a": (["ab"], r"\d*")}, "unsupported"),
    ({"a": (["ab"], r"\d?\d")}, "optional position"),
    ({"a": (["ab"], r"\d{17}")}, "positions"),
])
def test_bad_keyed_mappings_raise(mapping, match):
    for ci in (False, True):
        with pytest.raises(ValueError, match=match):
            KeyedFieldSet(mapping, case_insensitive=ci)


def test_keyed_field_set_more_errors_and_pickling():
    with pytest.raises(ValueError, match="duplicate"):
        KeyedFieldSet({"a": (["ab", "AB"], r"\d")}, case_insensitive=True)
    KeyedFieldSet({"a": (["ab", "AB"], r"\d")})                               # distinct when case-sensitive
    for bad in (["ab"], "ab", 7, None):
        with pytest.raises(TypeError, match="mapping"):
            KeyedFieldSet(bad)
    for ci in (False, True):
        k = KeyedFieldSet(MAPPING, case_insensitive=ci)
        k.tensors("cpu")
        assert k.__reduce__() == (KeyedFieldSet, ({n: (list(w), p) for n, (w, p) in MAPPING.items()}, ci))
        back = pickle.loads(pickle.dumps(k))
        assert back.keywords == k.keywords and back.names == k.names and back.case_insensitive is ci
        for name in ("labels", "alternatives", "kw_lengths", "groups", "classes", "optional", "lengths"):
            np.testing.assert_array_equal(getattr(back, name), getattr(k, name))


# ------------------------------------------------------------------ Recognizer
def test_recognizer_keyed_arguments():
    store = _stub_store()
    r = Recognizer(store)
    assert r.keyed_fields is None and r.keyed_threshold == math.log(0.5) and r.keyed_gap_cost == 0.0
    k = KeyedFieldSet(MAPPING, case_insensitive=True)
    assert Recognizer(store, keyed_fields=k).keyed_fields is k
    r = Recognizer(store, keyed_fields=MAPPING, keyed_threshold=-3, keyed_gap_cost=0.05, case_insensitive=True,
                   keywords=["TOTAL"], fields={"amount": r"\d\.\d\d"}, detail=True)
    assert isinstance(r.keyed_fields, KeyedFieldSet) and r.keyed_fields.case_insensitive is True
    assert r.keyed_threshold == -3.0 and r.keyed_gap_cost == 0.05 and r.keywords is not None and r.fields is not None
    assert Recognizer(store, keyed_fields=MAPPING).keyed_fields.case_insensitive is False
    for bad in (7, ["total"], "total", (("a", (["ab"], r"\d")),)):
        with pytest.raises(TypeError, match="keyed_fields"):
            Recognizer(store, keyed_fields=bad)
    with pytest.raises(ValueError, match="duplicate"):
        Recognizer(store, keyed_fields={"a": (["ab", "AB"], r"\d")}, case_insensitive=True)
    for bad in (1e-6, 1, float("nan")):
        with pytest.raises(ValueError, match="keyed_threshold"):
            Recognizer(store, keyed_fields=k, keyed_threshold=bad)
    for bad in (-1e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="keyed_gap_cost"):
            Recognizer(store, keyed_fields=k, keyed_gap_cost=bad)
    with pytest.raises(ValueError, match="keyed_fields and lexicon"):
        Recognizer(store, keyed_fields=k, lexicon=["ab", "cd"])


def test_factory_carries_the_keyed_fields_as_a_mapping():
    f = gpu_recognizer(keyed_fields=KeyedFieldSet(MAPPING, case_insensitive=True), keyed_threshold=-2.5,
                       keyed_gap_cost=0.1)
    assert f.keyed_fields == {n: (list(w), p) for n, (w, p) in MAPPING.items()} and type(f.keyed_fields) is dict
    g = pickle.loads(pickle.dumps(f))
    assert g.keyed_fields == f.keyed_fields and g.keyed_case_insensitive is True
    assert g.keyed_threshold == -2.5 and g.keyed_gap_cost == 0.1
    f = gpu_recognizer(keyed_fields=MAPPING, case_insensitive=True)
    assert f.keyed_case_insensitive is True and f.keyed_threshold == math.log(0.5) and f.keyed_gap_cost == 0.0
    assert gpu_recognizer().keyed_fields is None
    with pytest.raises(ValueError, match="duplicate"):
        gpu_recognizer(keyed_fields={"a": (["ab", "ab"], r"\d")})
    with pytest.raises(ValueError, match="keyed_threshold"):
        gpu_recognizer(keyed_fields=MAPPING, keyed_threshold=0.5)
    with pytest.raises(ValueError, match="keyed_gap_cost"):
        gpu_recognizer(keyed_fields=MAPPING, keyed_gap_cost=-1)
    with pytest.raises(ValueError, match="keyed_fields and lexicon"):
        gpu_recognizer(keyed_fields=MAPPING, lexicon=["ab"])
    with pytest.raises(TypeError, match="keyed_fields"):
        gpu_recognizer(keyed_fields=["total"])


def test_keyed_recognition_pickles():
    hit = KeyedHit("total", "TOTAL", "12.50", -0.25, -0.125, 2, 12, 6.5, 26.5, 14, 24, 30.5, 50.5)
    det = Recognition("TOTAL 12.50", 0.5, (0.9,) * 11, ((0.0, 1.0),) * 11)
    kh = KeywordHit("TOTAL", -0.125, 2, 12, 6.5, 26.5)
    fh = FieldHit("amount", "12.50", -0.125, 14, 24, 30.5, 50.5)
    for r in (KeyedRecognition("TOTAL 12.50", None, (), (), (hit,)), KeyedRecognition("TOTAL 12.50", det, (kh,), (fh,), ())):
        back = pickle.loads(pickle.dumps(r))
        assert back == r and type(back) is KeyedRecognition
    assert type(back.detail) is Recognition and type(back.hits[0]) is KeywordHit and type(back.fields[0]) is FieldHit
    assert KeyedHit._fields == ("name", "keyword", "text", "score", "keyword_score", "kw_first_frame", "kw_end_frame",
                                "kw_x0", "kw_x1", "first_frame", "end_frame", "x0", "x1")
    assert KeyedRecognition._fields == ("text", "detail", "hits", "fields", "keyed")
    assert FieldRecognition._fields == ("text", "detail", "hits", "fields")         # untouched


def test_bad_scalar_arguments_launch_nothing():
    """The entry's argument checks, with no device pointer in sight (tests/test_keywords.py's way)."""
    from cnn_lstm_ctc_ocr_amd import _lib

    def keyed(T=125, B=64, C=96, n_kw=20, max_kw_len=16, n_key=7, max_pat_len=16, gap_cost=0.0, ws_bytes=1 << 40):
        _lib.call("ocrk_ctc_keyed_field", None, None, T, B, C, None, None, None, None, n_kw, max_kw_len, None, None,
                  None, n_key, max_pat_len, gap_cost, None, None, None, None, None, None, None, None, None, ws_bytes,
                  None)

    for kwargs, match in [(dict(T=0), "T=0"), (dict(T=4097), "T=4097"), (dict(C=257), "C=257"), (dict(C=1), "C=1"),
                          (dict(B=-1), "B=-1"), (dict(B=65536), "B=65536"), (dict(n_kw=0), "n_kw=0"),
                          (dict(n_kw=(1 << 20) + 1), "n_kw="), (dict(max_kw_len=0), "max_kw_len=0"),
                          (dict(max_kw_len=256), "max_kw_len=256"), (dict(n_key=0), "n_key=0"),
                          (dict(n_key=(1 << 20) + 1), "n_key="), (dict(max_pat_len=0), "max_pat_len=0"),
                          (dict(max_pat_len=256), "max_pat_len=256"), (dict(gap_cost=-0.5), "gap_cost"),
                          (dict(gap_cost=float("nan")), "gap_cost"), (dict(ws_bytes=1024), "workspace too small"),
                          (dict(), "null pointer")]:
        with pytest.raises(_lib.InvalidArgumentError, match=match):
            keyed(**kwargs)
    keyed(B=0)                                             # an empty batch is no error and touches nothing
    size = _lib.lib().ocrk_ctc_keyed_field_workspace_size
    assert size(125, 64, 96, 20, 16, 7, 16) >= 4 * 64 * 125 * 96 + 8 * 64 * 20 * 125 + 16 * 64 * 7 * 125
    assert size(0, 64, 96, 20, 16, 7, 16) == 0 and size(125, 64, 96, 20, 16, 0, 16) == 0
