"""tests/ctc_spot_ref.py (the NumPy restatement of ocrk_ctc_spot's recursion the
GPU tests compare with bit for bit) against brute-force enumeration: L <= 6,
C = 4, keywords of 1..3 symbols, logits on a grid of 1/4 so every float32 sum
is exact and maxima can be compared with ==."""
import itertools

import numpy as np
import pytest

import ctc_spot_ref as R

C = 4
BLANK = C - 1


def _grid_logits(rng, L):
    return (rng.integers(-8, 9, (L, C)) / 4).astype(np.float32)


def _segment_labellings(rel, f, e, kw):
    """The best sum of rel over frames [f, e) among the frame labellings whose first and last frames are
    non-blank and whose CTC collapse is kw (-inf if there is none)."""
    import ctc_align_ref as A
    best = -np.inf
    for lab in itertools.product(range(C), repeat=e - f):
        if lab[0] == BLANK or lab[-1] == BLANK or A.collapse(lab, BLANK) != list(kw):
            continue
        best = max(best, float(sum(np.float64(rel[f + j, c]) for j, c in enumerate(lab))))
    return best


def _segment_state_paths(emis, skip, f, e):
    """The best sum of emissions over frames [f, e) among the monotone state paths from state 0 to state
    S - 1 (stay, one on, or two on where skip allows)."""
    S = emis.shape[1]
    best = -np.inf

    def walk(t, s, acc):
        nonlocal best
        acc += float(emis[t, s])
        if t == e - 1:
            if s == S - 1:
                best = max(best, acc)
            return
        walk(t + 1, s, acc)
        if s + 1 < S:
            walk(t + 1, s + 1, acc)
        if s + 2 < S and skip[s + 2]:
            walk(t + 1, s + 2, acc)

    walk(f, 0, 0.0)
    return best


def _random_keyword(rng, with_alts):
    n = int(rng.integers(1, 4))
    kw = [int(c) for c in rng.integers(0, BLANK, n)]
    if n >= 2 and rng.random() < 0.4:
        kw[1] = kw[0]                                        # an adjacent repeat
    if not with_alts:
        return kw, None
    alts = [int(a) if rng.random() < 0.6 else -1 for a in rng.integers(0, BLANK, n)]
    return kw, alts


def _check(logits, kw, alts):
    """The helper's (score, span) against enumeration over every segment; returns the score."""
    L = logits.shape[0]
    rel = R.relative(logits)
    score, first, end = R.spot(logits, kw, alts)
    if alts is None:
        seg = lambda f, e: _segment_labellings(rel, f, e, kw)
    else:
        emis, skip = R.emissions(rel, kw, alts), R.skips(kw, alts)
        seg = lambda f, e: _segment_state_paths(emis, skip, f, e)
    table = {(f, e): seg(f, e) for f in range(L) for e in range(f + 1, L + 1)}
    want = max(table.values(), default=-np.inf)
    if R.required_time(kw, alts) > L:
        assert want == -np.inf
        assert np.isneginf(score) and (first, end) == (-1, -1)
        return score
    assert np.isfinite(want) and score.dtype == np.float32
    assert float(score) == want and score <= 0
    assert 0 <= first < end <= L and table[(first, end)] == want   # the span is one of the maximisers
    # among equal scores the earliest end
    assert end == min(e for (f, e), v in table.items() if v == want)
    return score


@pytest.mark.parametrize("with_alts", [False, True])
def test_recursion_equals_enumeration(with_alts):
    rng = np.random.default_rng(7 + with_alts)
    infeasible = exact_hits = 0
    for _ in range(300):
        L = int(rng.integers(1, 7))
        kw, alts = _random_keyword(rng, with_alts)
        score = _check(_grid_logits(rng, L), kw, alts)
        infeasible += bool(np.isneginf(score))
        exact_hits += bool(score == 0)
    assert infeasible >= 10 and exact_hits >= 10             # both kinds were met


@pytest.mark.parametrize("kw, alts, span", [
    ([0], None, (0, 1)),
    ([0, 1], None, (0, 2)),
    ([1, 1], None, (0, 3)),                                  # the repeat needs its blank
    ([0, 1, 2], None, (0, 3)),
    ([0, 1], [1, -1], (0, 3)),                               # overlapping sets {0, 1} and {1}: a repeat
    ([0, 1], [2, -1], (0, 2)),
])
def test_all_ties(kw, alts, span):
    """Constant logits: every labelling scores 0. The earliest end wins, and with it the start the tie order
    (stay before one back before two back before entry) produces: the hit begins at frame 0."""
    logits = np.zeros((6, C), np.float32)
    assert _check(logits, kw, alts) == 0
    assert R.spot(logits, kw, alts)[1:] == span


def test_planted_keyword_scores_zero_at_its_frames():
    logits = np.zeros((6, C), np.float32)
    for t, c in enumerate([BLANK, 2, 0, 0, BLANK, 1]):       # greedy path ". 2 0 0 . 1"
        logits[t, c] = 1.0
    assert R.spot(logits, [2, 0], None) == (0.0, 1, 3)       # ends as early as it can: one frame of 0
    assert R.spot(logits, [0, 1], None) == (0.0, 2, 6)
    # "0 0" needs a blank: 0 0 . 0 on frames 2..5 costs the last frame alone (-1); ending at 5 would cost 2.
    # Starting at 3 ties; state 0 stays (start 2) before it re-enters.
    assert R.spot(logits, [0, 0], None) == (-1.0, 2, 6)
    assert R.spot(logits, [1, 2], None)[0] < 0
    assert R.spot(logits, [1, 0], [2, -1]) == (0.0, 1, 3)    # the alternative spells it


def test_infeasible_pairs():
    logits = np.zeros((2, C), np.float32)
    for kw, alts in [([0, 1, 2], None), ([1, 1], None), ([0, 1], [1, -1]), ([0, 1], [-1, 0])]:
        score, first, end = R.spot(logits, kw, alts)
        assert np.isneginf(score) and (first, end) == (-1, -1)
    score, span = R.spot_batch(np.zeros((3, 2, C), np.float32), [3, 0], [[0], [0, 0, 0]])
    assert score.tolist() == [[0.0, -np.inf], [-np.inf, -np.inf]]
    assert span.tolist() == [[[0, 1], [-1, -1]], [[-1, -1], [-1, -1]]]
