"""tests/ctc_spot_fuzzy_ref.py (the NumPy restatement of ocrk_ctc_spot_fuzzy's
recursion the GPU tests compare with bit for bit) against an enumeration of
state paths over forward edges: L <= 6, C in {3, 4}, keywords of 1..3 symbols,
up to 2 edits, logits and edit_cost on a grid of 1/4 so every float32 sum is
exact and maxima can be compared with ==. And the host side of the feature:
decode.FuzzyKeywordSet, the Recognizer's arguments, the entry's argument checks.
Nothing is launched."""
import math
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ctc_spot_fuzzy_ref as R
import ctc_spot_ref as X

INF = float("inf")


def _grid_logits(rng, L, C):
    return (rng.integers(-8, 9, (L, C)) / 4).astype(np.float32)


def _planted_logits(path, C, L=None):
    """Logits whose argmax path is `path` (2 at the planted class, 0 elsewhere; -1 = the blank)."""
    logits = np.zeros((len(path) if L is None else L, C), np.float32)
    for t, c in enumerate(path):
        logits[t, C - 1 if c < 0 else c] = 2.0
    return logits


# ------------------------------------------------------------------ enumeration
def _enumerate(logits, kw, alts, E, cost):
    """{(first, end, errors): the best sum} over every state path, walked along the forward edges of the
    lattice: from a state of frame t - 1 to the states of frame t it may move to."""
    rel = X.relative(logits).astype(np.float64)
    L, C = rel.shape
    n = len(kw)
    S = 2 * n - 1
    sets = X.sets(kw, alts)
    nb = rel[:, :C - 1].max(axis=1)
    a = [int(np.argmax(rel[t, :C - 1])) for t in range(L)]

    def emis(kind, s, t):
        if kind == "W":
            return nb[t]
        if s % 2:
            return rel[t, C - 1]
        return max(rel[t, c] for c in sets[s // 2])

    def edges(kind, e, s, t):
        """The states of frame t reachable from (kind, e, s) of frame t - 1, with the cost of the move."""
        out = []
        if kind == "M":
            out.append(("M", e, s, 0.0))
            if s + 1 < S:
                out.append(("M", e, s + 1, 0.0))
            if s % 2 == 0 and s + 2 < S and not (sets[s // 2] & sets[s // 2 + 1]):
                out.append(("M", e, s + 2, 0.0))
            if e < E:
                if s % 2 == 1:                               # after a blank: a wild, or the next symbol deleted
                    out.append(("W", e + 1, s, cost))
                    out.append(("W", e + 1, s + 1, cost))    # s + 1 < S always for a blank
                    if s + 3 < S:
                        out.append(("M", e + 1, s + 3, cost))
                else:                                        # after symbol s / 2: a wild of another class
                    if a[t] not in sets[s // 2]:
                        if s + 1 < S:
                            out.append(("W", e + 1, s + 1, cost))
                        if s + 2 < S:
                            out.append(("W", e + 1, s + 2, cost))
                    if s + 4 < S and not (sets[s // 2] & sets[s // 2 + 2]):
                        out.append(("M", e + 1, s + 4, cost))
        else:
            if a[t] == a[t - 1]:
                out.append(("W", e, s, 0.0))
            elif e == 1 and E >= 2 and s + 1 < S:
                out.append(("W", 2, s + 1, cost))
            if s % 2 == 1:
                out.append(("M", e, s, 0.0))                 # the blank after an inserted symbol
                if a[t - 1] not in sets[(s + 1) // 2]:
                    out.append(("M", e, s + 1, 0.0))
            else:
                if s + 1 < S:
                    out.append(("M", e, s + 1, 0.0))
                if s + 2 < S and a[t - 1] not in sets[s // 2 + 1]:
                    out.append(("M", e, s + 2, 0.0))
        return out

    memo = {}

    def suffix(kind, e, s, t):
        """{(end, errors): best sum of what follows the state (kind, e, s) of frame t}."""
        key = (kind, e, s, t)
        if key in memo:
            return memo[key]
        res = {}
        if s == S - 1:
            res[(t + 1, e)] = 0.0
        if t + 1 < L:
            for k2, e2, s2, c in edges(kind, e, s, t + 1):
                step = emis(k2, s2, t + 1) - c
                for fin, v in suffix(k2, e2, s2, t + 1).items():
                    if step + v > res.get(fin, -INF):
                        res[fin] = step + v
        memo[key] = res
        return res

    table = {}
    for f in range(L):
        starts = [("M", 0, 0, 0.0)] + ([("W", 1, 0, cost)] if E >= 1 else [])
        for kind, e, s, c in starts:
            for (end, err), v in suffix(kind, e, s, f).items():
                tot = emis(kind, s, f) - c + v
                if tot > table.get((f, end, err), -INF):
                    table[(f, end, err)] = tot
    return {k: v for k, v in table.items() if v > -INF}


def _random_keyword(rng, C, with_alts):
    n = int(rng.integers(1, 4))
    kw = [int(c) for c in rng.integers(0, C - 1, n)]
    if n >= 2 and rng.random() < 0.3:
        kw[1] = kw[0]                                        # an adjacent repeat
    if not with_alts:
        return kw, None
    return kw, [int(x) if rng.random() < 0.6 else -1 for x in rng.integers(0, C - 1, n)]


def _kinds(path, S):
    """Which edit mechanisms a traced path takes."""
    got = set()
    for kind, _e, s, code in path:
        if kind == "W":
            got.add("insertion" if s % 2 else "substitution")
            if s == 0:
                got.add("substituted first symbol")
            if s == S - 1:
                got.add("substituted last symbol")
            if code == R.W_WILD:
                got.add("wild -> wild")
        elif code == R.M_DEL4:
            got.add("deletion direct")
        elif code == R.M_DEL3:
            got.add("deletion after a blank")
    return got


def _check(logits, kw, alts, E, cost):
    """The helper's (score, span, errors) and its backtrace against the enumeration; returns the mechanisms of
    the best path."""
    L = logits.shape[0]
    score, first, end, errors, path = R.spot(logits, kw, alts, E, cost, trace=True)
    table = _enumerate(logits, kw, alts, E, cost)
    if not table:
        assert np.isneginf(score) and (first, end, errors) == (-1, -1, -1) and path is None
        return set()
    want = max(table.values())
    assert score.dtype == np.float32 and float(score) == want
    assert 0 <= first < end <= L and 0 <= errors <= E
    assert table[(first, end, errors)] == want               # the result is one of the maximisers
    # among equal scores the earliest end, then the fewest edits
    best = [k for k, v in table.items() if v == want]
    assert end == min(k[1] for k in best)
    assert errors == min(k[2] for k in best if k[1] == end)
    # the backtrace is a path of that span whose emissions and costs sum to the score
    S = 2 * len(kw) - 1
    assert len(path) == end - first and path[-1][2] == S - 1 and path[-1][1] == errors
    assert [p[1] for p in path] == sorted(p[1] for p in path)
    if errors == 0:
        assert all(p[0] == "M" for p in path)
    return _kinds(path, S)


PLANTED_C = 7                                                # classes 0..5 and the blank
PLANTED = [
    # keyword, the greedy path (-1 = blank), budget, the mechanism it plants
    ([0, 1, 0], [0, 2, 0], 1, "substitution"),
    ([0, 1, 2], [0, 3, 1, 2], 1, "insertion"),
    ([0, 1, 2], [0, 2], 1, "deletion direct"),
    ([0, 1, 2], [0, -1, 2], 1, "deletion after a blank"),
    ([0, 1, 2], [0, 3, 4, 2], 2, "wild -> wild"),
    ([0, 1], [2, 1], 1, "substituted first symbol"),
    ([0, 1], [0, 2], 1, "substituted last symbol"),
    ([0, 1, 2], [1, 1, 0, 2], 2, "substitution"),            # first symbol substituted and one more edit
    ([0, 0, 1], [0, 1, -1, 1], 2, "substitution"),           # repeats around a wild
    ([2, 1, 2], [2, 2, 2, 1, 1, 2], 1, "substitution"),      # long runs
]


@pytest.mark.parametrize("with_alts", [False, True])
def test_recursion_equals_enumeration(with_alts):
    rng = np.random.default_rng(31 + with_alts)
    seen, no_path, used = set(), 0, [0, 0, 0]
    for j in range(300):
        C = 3 + j % 2
        L = int(rng.integers(1, 7))
        kw, alts = _random_keyword(rng, C, with_alts)
        E = int(rng.integers(0, R.max_budget(len(kw)) + 1))
        cost = float(rng.integers(0, 5)) / 4
        logits = _grid_logits(rng, L, C)
        got = _check(logits, kw, alts, E, cost)
        seen |= got
        res = R.spot(logits, kw, alts, E, cost)
        no_path += res[3] < 0
        if res[3] >= 0:
            used[res[3]] += 1
    for kw, greedy, E, _kind in PLANTED:                     # the planted lines, with and without alternatives
        alts = None
        if with_alts:
            alts = [-1] * len(kw)
            alts[0] = 5                                      # class 5 never tops a planted frame
        for cost in (0.0, 0.25):
            got = _check(_planted_logits(greedy, PLANTED_C), kw, alts, E, cost)
            seen |= got
    assert no_path >= 5 and min(used) >= 1, (no_path, used)
    # coverage is a condition: every mechanism is on the best path of at least one case
    assert seen == {"substitution", "insertion", "deletion direct", "deletion after a blank", "wild -> wild",
                    "substituted first symbol", "substituted last symbol"}


@pytest.mark.parametrize("kw, greedy, E, kind", PLANTED[:7])
def test_planted_edits(kw, greedy, E, kind):
    """A line whose greedy path is the keyword with the planted edits scores 0 with that many errors at
    edit_cost 0, over exactly the planted frames; the exact spotter scores below 0."""
    logits = _planted_logits(greedy, PLANTED_C)
    score, first, end, errors, path = R.spot(logits, kw, None, E, 0.0, trace=True)
    assert score == 0 and (first, end) == (0, len(greedy)) and errors == E
    assert kind in _kinds(path, 2 * len(kw) - 1)
    assert X.spot(logits, kw, None)[0] < 0
    assert R.spot(logits, kw, None, E, 0.5)[0] == -0.5 * E   # each edit charged once
    frames, collapsed = R.labelling(logits, kw, None, path, first)
    assert collapsed == [c for c in greedy if c >= 0]


def _levenshtein(a, b):
    d = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, d[0] = d[0], i
        for j, y in enumerate(b, 1):
            prev, d[j] = d[j], min(d[j] + 1, d[j - 1] + 1, prev + (x != y))
    return d[len(b)]


def test_soundness():
    """The CTC collapse of the best path's frame labelling is within `errors` edits of the keyword."""
    rng = np.random.default_rng(37)
    edited = 0
    for _ in range(400):
        C = int(rng.integers(3, 6))
        n = int(rng.integers(2, 7))
        L = int(rng.integers(1, 14))
        kw = [int(c) for c in rng.integers(0, C - 1, n)]
        E = int(rng.integers(1, R.max_budget(n) + 1))
        logits = _grid_logits(rng, L, C)
        score, first, end, errors, path = R.spot(logits, kw, None, E, float(rng.integers(0, 3)) / 4, trace=True)
        if path is None:
            continue
        _frames, collapsed = R.labelling(logits, kw, None, path, first)
        assert _levenshtein(collapsed, kw) <= errors, (kw, collapsed, errors)
        edited += errors > 0
    assert edited >= 50


@pytest.mark.parametrize("with_alts", [False, True])
def test_budget_zero_is_the_exact_spotter(with_alts):
    rng = np.random.default_rng(41 + with_alts)
    for _ in range(200):
        C = int(rng.integers(3, 6))
        L = int(rng.integers(1, 10))
        n = int(rng.integers(1, 6))
        kw = [int(c) for c in rng.integers(0, C - 1, n)]
        alts = [int(x) if rng.random() < 0.5 else -1 for x in rng.integers(0, C - 1, n)] if with_alts else None
        logits = _grid_logits(rng, L, C)
        want = X.spot(logits, kw, alts)
        for E, cost in ((0, 0.0), (0, 0.75), (R.max_budget(n), INF)):
            got = R.spot(logits, kw, alts, E, cost)
            assert np.float32(got[0]).tobytes() == np.float32(want[0]).tobytes() and got[1:3] == want[1:]
            assert got[3] == (0 if np.isfinite(want[0]) else -1)


def test_batch_matches_rows_and_budgets_are_monotone():
    rng = np.random.default_rng(43)
    T, B, C = 9, 4, 4
    logits = (rng.integers(-8, 9, (T, B, C)) / 4).astype(np.float32)
    seq = [9, 4, 0, 1]
    kws = [[0], [0, 1], [1, 1, 2], [2, 0, 1, 0]]
    scores = []
    for e in range(3):
        errs = [min(e, R.max_budget(len(k))) for k in kws]
        score, span, errors = R.spot_batch(logits, seq, kws, None, errs, 0.25)
        for b in range(B):
            for k, kw in enumerate(kws):
                want = R.spot(np.ascontiguousarray(logits[:seq[b], b]), kw, None, errs[k], 0.25)
                assert (score[b, k], span[b, k, 0], span[b, k, 1], errors[b, k]) == want
        scores.append(score)
    assert np.all(scores[2] >= scores[1]) and np.all(scores[1] >= scores[0])
    assert np.all(np.isneginf(scores[2][2]))                 # the row without frames


# ------------------------------------------------------------- the host side
KEYWORDS = ["TOTAL", "gst", "Change Due", "receipt no.", "a", "x" * 32, "Subtotal:", "CASH"]


def _stub_store():
    """What Recognizer.__init__ reads of a ParamStore."""
    return SimpleNamespace(cfg=SimpleNamespace(dtype=torch.float32), device=torch.device("cpu"), version=0)


def test_fuzzy_keyword_set():
    from cnn_lstm_ctc_ocr_amd.decode import FuzzyKeywordSet, KeywordSet
    ks = FuzzyKeywordSet(KEYWORDS)
    assert isinstance(ks, KeywordSet) and ks.max_errors == "auto" and ks.case_insensitive is False
    # min(2, (len + 1) // 5): 5 -> 1, 3 -> 0, 10 -> 2, 11 -> 2, 1 -> 0, 32 -> 2, 9 -> 2, 4 -> 1
    assert ks.errors.tolist() == [1, 0, 2, 2, 0, 2, 2, 1] and ks.errors.dtype == np.int32
    plain = KeywordSet(KEYWORDS)
    np.testing.assert_array_equal(ks.labels, plain.labels)
    np.testing.assert_array_equal(ks.lengths, plain.lengths)
    lab, alt, ln, err = ks.fuzzy_tensors("cpu")
    assert alt is None and err.dtype == torch.int32 and err.tolist() == ks.errors.tolist()
    assert ks.fuzzy_tensors("cpu")[3] is err and ks.tensors("cpu")[0] is lab
    assert FuzzyKeywordSet(["TOTAL", "ab"], 1).errors.tolist() == [1, 1]
    assert FuzzyKeywordSet(["TOTAL", "ab", "a"], [2, 1, 0], case_insensitive=True).errors.tolist() == [2, 1, 0]
    assert FuzzyKeywordSet(["TOTAL"], 0).errors.tolist() == [0]
    for words, errs, match in [(["TOTAL", "a"], 1, "'a'"), (["ab"], 2, "0..1 errors"), (["TOTAL"], 3, "0..2 errors"),
                               (["TOTAL"], -1, "not -1"), (["TOTAL", "gst"], [1], "1 budgets for 2"),
                               (["TOTAL"], [1.0], "not an int"), (["TOTAL"], "most", "'auto'"),
                               (["TOTAL"], 1.5, "'auto'"), (["TOTAL"], True, "'auto'")]:
        with pytest.raises(ValueError, match=match):
            FuzzyKeywordSet(words, errs)
    with pytest.raises(ValueError, match="duplicate"):
        FuzzyKeywordSet(["ab", "AB"], 0, case_insensitive=True)


@pytest.mark.parametrize("errs", ["auto", 0, [1, 0, 2, 1, 0, 2, 0, 1]])
def test_fuzzy_keyword_set_pickles_as_its_arguments(errs):
    from cnn_lstm_ctc_ocr_amd.decode import FuzzyKeywordSet
    ks = FuzzyKeywordSet(KEYWORDS, errs, case_insensitive=True)
    ks.fuzzy_tensors("cpu")
    want = errs if isinstance(errs, (str, list)) else [errs] * len(KEYWORDS)
    assert ks.__reduce__() == (FuzzyKeywordSet, (KEYWORDS, want, True))
    back = pickle.loads(pickle.dumps(ks))
    assert type(back) is FuzzyKeywordSet and back.keywords == ks.keywords and back.case_insensitive is True
    np.testing.assert_array_equal(back.errors, ks.errors)
    np.testing.assert_array_equal(back.alternatives, ks.alternatives)


def test_recognizer_fuzzy_arguments():
    from cnn_lstm_ctc_ocr_amd.decode import FuzzyKeywordSet, KeywordSet
    from cnn_lstm_ctc_ocr_amd.server import Recognizer, gpu_recognizer
    store = _stub_store()
    r = Recognizer(store, keywords=KEYWORDS)
    assert type(r.keywords) is KeywordSet and r.fuzzy_keywords is False and r.keyword_edit_cost == 0.0
    r = Recognizer(store, keywords=KEYWORDS, keyword_errors="auto", keyword_edit_cost=0.5, case_insensitive=True)
    assert type(r.keywords) is FuzzyKeywordSet and r.fuzzy_keywords and r.keyword_edit_cost == 0.5
    assert r.keywords.case_insensitive is True and r.keywords.errors.tolist() == [1, 0, 2, 2, 0, 2, 2, 1]
    r = Recognizer(store, keywords=KeywordSet(KEYWORDS, True), keyword_errors=0)
    assert type(r.keywords) is FuzzyKeywordSet and r.keywords.case_insensitive and not r.keywords.errors.any()
    fs = FuzzyKeywordSet(KEYWORDS, "auto")
    r = Recognizer(store, keywords=fs, keyword_edit_cost=INF)
    assert r.keywords is fs and r.fuzzy_keywords and r.keyword_edit_cost == INF
    with pytest.raises(ValueError, match="needs keywords"):
        Recognizer(store, keyword_errors=1)
    with pytest.raises(ValueError, match="budgets already"):
        Recognizer(store, keywords=fs, keyword_errors=1)
    with pytest.raises(ValueError, match="errors"):
        Recognizer(store, keywords=KEYWORDS, keyword_errors=2)           # "a" takes none
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="keyword_edit_cost"):
            Recognizer(store, keywords=fs, keyword_edit_cost=bad)
    with pytest.raises(ValueError, match="keyword_edit_cost needs"):
        Recognizer(store, keywords=KEYWORDS, keyword_edit_cost=0.5)
    with pytest.raises(ValueError, match="keywords and lexicon"):
        Recognizer(store, keywords=fs, lexicon=["ab"])
    # the replica factory carries the budgets as plain ints
    f = pickle.loads(pickle.dumps(gpu_recognizer(keywords=fs, keyword_edit_cost=0.25)))
    assert f.keywords == KEYWORDS and f.keyword_errors == fs.errors.tolist() and f.keyword_edit_cost == 0.25
    assert all(type(e) is int for e in f.keyword_errors)
    f = gpu_recognizer(keywords=KEYWORDS, keyword_errors="auto", case_insensitive=True)
    assert f.keyword_errors == fs.errors.tolist() and f.case_insensitive is True
    assert gpu_recognizer(keywords=KEYWORDS).keyword_errors is None
    with pytest.raises(ValueError, match="needs keywords"):
        gpu_recognizer(keyword_errors=1)


def test_fuzzy_hit_pickles():
    from cnn_lstm_ctc_ocr_amd.server import FuzzyKeywordHit, KeywordHit, KeywordRecognition
    hit = FuzzyKeywordHit("TOTAL", -0.25, 4, 17, 10.5, 36.5, 1)
    assert FuzzyKeywordHit._fields == KeywordHit._fields + ("errors",)
    back = pickle.loads(pickle.dumps(KeywordRecognition("T0TAL 9", None, (hit,))))
    assert type(back.hits[0]) is FuzzyKeywordHit and back.hits[0] == hit


def test_spotter_refuses_what_it_cannot_run():
    from cnn_lstm_ctc_ocr_amd import decode
    logits, seq = torch.zeros(4, 1, 96), torch.tensor([4])
    with pytest.raises(TypeError, match="FuzzyKeywordSet"):
        decode.ctc_fuzzy_keyword_spotter(logits, seq, decode.KeywordSet(["ab"]))
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="edit_cost"):
            decode.ctc_fuzzy_keyword_spotter(logits, seq, decode.FuzzyKeywordSet(["ab"]), bad)


def test_bad_scalar_arguments_launch_nothing():
    """The entry's argument checks, with no device pointer in sight (tests/test_abi.py's way)."""
    from cnn_lstm_ctc_ocr_amd import _lib

    def spot(T=125, B=64, C=96, n_kw=64, max_kw_len=16, edit_cost=0.0, ws_bytes=1 << 40):
        _lib.call("ocrk_ctc_spot_fuzzy", None, None, T, B, C, None, None, None, None, n_kw, max_kw_len, edit_cost,
                  None, None, None, None, None, None, ws_bytes, None)

    for kwargs, match in [(dict(T=0), "T=0"), (dict(T=4097), "T=4097"), (dict(C=257), "C=257"), (dict(C=1), "C=1"),
                          (dict(B=-1), "B=-1"), (dict(B=65536), "B=65536"), (dict(n_kw=0), "n_kw=0"),
                          (dict(n_kw=(1 << 20) + 1), "n_kw="), (dict(max_kw_len=0), "max_kw_len=0"),
                          (dict(max_kw_len=256), "max_kw_len=256"), (dict(edit_cost=-0.25), "edit_cost"),
                          (dict(edit_cost=math.nan), "edit_cost"), (dict(ws_bytes=1024), "workspace too small"),
                          (dict(), "null pointer"), (dict(edit_cost=INF), "null pointer")]:
        with pytest.raises(_lib.InvalidArgumentError, match=match):
            spot(**kwargs)
    spot(B=0)                                              # an empty batch is no error and touches nothing
    size = _lib.lib().ocrk_ctc_spot_fuzzy_workspace_size
    # the rel table, (nb, a) per frame and one int per keyword
    assert size(125, 64, 96, 64, 16) == 125 * 64 * 96 * 4 + 125 * 64 * 8 + 64 * 4
    assert size(125, 64, 96, 65, 40) == 125 * 64 * 96 * 4 + 125 * 64 * 8 + 272     # rounded to 16 B
    assert size(0, 64, 96, 64, 16) == 0 and size(125, 64, 96, 0, 16) == 0 and size(125, 64, 96, 10, 256) == 0
