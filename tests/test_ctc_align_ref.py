"""The float32 restatement of the alignment recursion (tests/ctc_align_ref.py)
against brute-force enumeration of every path, the frame -> pixel mapping, and
the Recognition tuple (host only)."""
import pickle

import numpy as np
import pytest

import ctc_align_ref as R


def _bruteforce_best(logits, label):
    """Best score over all C^T paths that collapse to `label` (None if there is
    none). Integer-valued logits: every float32 sum is exact."""
    T, C = logits.shape
    blank = C - 1
    paths = np.indices((C,) * T).reshape(T, -1).T                     # [C^T, T]
    prev = np.concatenate([np.full((len(paths), 1), -1), paths[:, :-1]], axis=1)
    keep = (paths != blank) & (paths != prev)
    n = len(label)
    ok = keep.sum(axis=1) == n
    if n:
        idx = np.clip(np.cumsum(keep, axis=1) - 1, 0, n - 1)
        ok &= np.all(~keep | (np.asarray(label)[idx] == paths), axis=1)
    if not ok.any():
        return None
    scores = logits[np.arange(T), paths].sum(axis=1, dtype=np.float32)
    return scores[ok].max()


def test_restatement_finds_the_bruteforce_optimum():
    rng = np.random.default_rng(0)
    feasible = 0
    for _ in range(400):
        T, C = int(rng.integers(1, 7)), int(rng.integers(2, 5))
        label = [int(c) for c in rng.integers(0, C - 1, int(rng.integers(0, 4)))]
        logits = rng.integers(0, 4, (T, C)).astype(np.float32)         # small integers: ties abound
        want = _bruteforce_best(logits, label)
        assert (want is not None) == R.feasible(label, T)
        if want is None:
            continue
        feasible += 1
        states, score = R.best_path(logits, label)
        ext = R.extended(label, C - 1)
        assert R.collapse(ext[states], C - 1) == label
        assert np.all(np.diff(states) >= 0) and np.all(np.diff(states) <= 2)
        assert score == want == logits[np.arange(T), ext[states]].sum(dtype=np.float32)
        sp = R.spans(states, len(label))
        assert np.all(sp[:, 1] > sp[:, 0])                             # every symbol has a non-empty run
    assert feasible >= 200


def test_ties_keep_the_lower_predecessor():
    """All-equal logits: every comparison ties, so the path stays in a state as
    long as it can -- the label is emitted in the first frames that allow it."""
    logits = np.zeros((6, 4), np.float32)
    states, score = R.best_path(logits, [0, 1])
    assert states.tolist() == [1, 3, 4, 4, 4, 4] and score == 0
    states, _ = R.best_path(logits, [2, 2])                            # a repeat needs its blank
    assert states.tolist() == [1, 2, 3, 4, 4, 4]


@pytest.mark.parametrize("W", [32, 33, 64, 97, 128, 255, 256, 1000])
def test_frame_pixel_mapping_matches_the_sequence_length(W):
    from cnn_lstm_ctc_ocr_amd.decode import frame_center_px, frames_to_px
    T = (W - 2) // 2 - 2                                               # model.py:152-163
    assert frame_center_px(0) == 3.5
    last = frame_center_px(T - 1)
    assert last == 2 * (T - 1) + 3.5 and last <= W - 1
    if W % 2 == 0:                                                     # symmetric about the crop's middle
        assert frame_center_px(0) + last == W - 1
    if W == 256:
        assert (T, last) == (125, 251.5)
    # every frame owns the 2 columns around its centre; runs tile without gaps; all inside the crop
    for t in (0, T // 2, T - 1):
        x0, x1 = frames_to_px(t, t + 1, W)
        assert (x0, x1) == (frame_center_px(t) - 1, frame_center_px(t) + 1)
    assert frames_to_px(0, 5, W)[1] == frames_to_px(5, 9, W)[0]
    x0, x1 = frames_to_px(0, T, W)
    assert 0 <= x0 < x1 <= W
    assert frames_to_px(0, 10 * W, W) == (2.5, float(W))               # clipped to the true width
    assert frames_to_px(T, T, 4.0) == (4.0, 4.0)


def test_recognition_pickles():
    from cnn_lstm_ctc_ocr_amd.server import Recognition
    r = Recognition("ab", 0.75, (0.9, 0.8), ((2.5, 6.5), (8.5, 12.5)))
    assert r._fields == ("text", "confidence", "char_confidence", "char_px")
    back = pickle.loads(pickle.dumps(r))
    assert back == r and type(back) is Recognition and back.text == "ab"
