"""page.plan_page: the host planner of the page -> crops launch (no GPU)."""
import numpy as np
import pytest

from cnn_lstm_ctc_ocr_amd import page as P
from cnn_lstm_ctc_ocr_amd.server import LocalServer


def _box_of_width(nw, y=0, x=0):
    """A 32-high box whose crop is nw wide (pad=0)."""
    return (y, x, y + 32, x + nw)


@pytest.mark.parametrize("accept_narrow", [False, True])
def test_bucket_is_the_local_servers(accept_narrow):
    srv = LocalServer(None, accept_narrow=accept_narrow)
    for nw in range(32 if accept_narrow else 33, 1001):
        crop = np.zeros((32, nw), np.uint8)
        takes = [k for k, b in enumerate(srv.buckets) if b.addImgToBucket("0", 0, 0.0, crop)]
        assert len(takes) == 1
        plan = P.plan_page([_box_of_width(nw)], (32, 1000), accept_narrow=accept_narrow, pad=0)
        assert not plan.skipped and len(plan.batches) == 1
        b = plan.batches[0]
        assert b.bucket == takes[0] and b.Wb == srv.buckets[takes[0]].widthrange[1], nw
        assert b.widths[0] == nw and P.bucket_of(nw, accept_narrow) == (b.bucket, b.Wb)


def test_skip_reasons():
    boxes = [(10, 10, 10, 50),           # no rows
             (0, 300, 40, 400),          # beyond the page's 200 columns
             (0, 0, 64, 62),             # nw = 31
             (0, 0, 32, 32),             # nw = 32: no bucket without accept_narrow
             (0, 0, 4, 130),             # nw = 1040
             (0, 0, 32, 100)]            # kept
    plan = P.plan_page(boxes, (96, 200), pad=0)
    assert plan.skipped == [(0, "empty"), (1, "empty"), (2, "narrow"), (3, "narrow"), (4, "wide")]
    assert plan.n_boxes == 6 and [b.boxes[0] for b in plan.batches] == [5]
    narrow = P.plan_page(boxes, (96, 200), pad=0, accept_narrow=True)
    assert narrow.skipped == [(0, "empty"), (1, "empty"), (2, "narrow"), (4, "wide")]
    assert narrow.batches[0].Wb == 32 and narrow.batches[0].bucket == 0 and narrow.batches[0].boxes[0] == 3
    padded = P.plan_page(boxes[:1], (96, 200), pad=1)        # pad gives the empty box two rows
    assert padded.skipped == [] and padded.jobs[0, :5].tolist() == [9, 9, 2, 42, P.new_width(2, 42)]


def test_pad_and_clip_at_the_corner():
    plan = P.plan_page([(70, 120, 96, 200), (0, 0, 20, 90)], (96, 200), pad=3)
    rows = {int(r[7]): r[:5].tolist() for r in plan.jobs if r[7] >= 0}
    assert rows[0] == [67, 117, 29, 83, P.new_width(29, 83)]          # clipped at the bottom right
    assert rows[1] == [0, 0, 23, 93, P.new_width(23, 93)]             # clipped at the top left


def test_batches_and_top_ups():
    bs = 16
    widths = [65 + (k % 31) for k in range(2 * bs + 3)]                # all in (64, 96]
    plan = P.plan_page([_box_of_width(w) for w in widths], (32, 200), bucket_size=bs, pad=0)
    assert [len(b.widths) for b in plan.batches] == [bs, bs, bs] and all(b.Wb == 96 for b in plan.batches)
    assert plan.batches[0].boxes.tolist() == list(range(bs))
    assert plan.batches[1].boxes.tolist() == list(range(bs, 2 * bs))
    last = plan.batches[2]
    assert last.boxes.tolist() == [2 * bs, 2 * bs + 1, 2 * bs + 2] + [-1] * 13
    assert last.widths.tolist() == widths[2 * bs:] + [widths[2 * bs]] * 13
    assert plan.jobs.shape == (3 * bs, 8) and plan.jobs.dtype == np.int32
    top = plan.jobs[2 * bs + 3:]
    assert (top[:, :5] == 0).all() and (top[:, 5] == 96).all() and (top[:, 7] == -1).all()
    one = P.plan_page([_box_of_width(70)], (32, 200), bucket_size=1, pad=0)
    assert len(one.batches) == 1 and one.batches[0].boxes.tolist() == [0] and one.jobs.shape == (1, 8)


def test_layout_is_aligned_and_tiles_the_arena():
    rng = np.random.default_rng(0)
    boxes = []
    for _ in range(60):
        h, w = int(rng.integers(8, 60)), int(rng.integers(30, 400))
        boxes.append((5, 3, 5 + h, 3 + w))
    plan = P.plan_page(boxes, (96, 500), bucket_size=4)
    assert len({b.Wb for b in plan.batches}) > 3
    used = np.zeros(plan.arena_bytes, np.int32)
    row = 0
    for b in plan.batches:
        assert b.Wb % 32 == 0 and b.offset % (32 * 32) == 0           # whole 32-byte rows before it
        for r in range(len(b.widths)):
            y0, x0, h, w, nw, Wb, off32, box = plan.jobs[row].tolist()
            assert Wb == b.Wb and off32 * 32 == b.offset + r * 32 * Wb and box == b.boxes[r]
            assert (nw == b.widths[r] and 1 <= nw <= Wb) if box >= 0 else (nw == 0 and b.widths[r] == b.widths[0])
            used[off32 * 32:off32 * 32 + 32 * Wb] += 1
            row += 1
    assert row == len(plan.jobs) and (used == 1).all()                # no overlap, no gap
    kept = sorted(int(i) for b in plan.batches for i in b.boxes if i >= 0)
    assert kept == sorted(set(range(60)) - {i for i, _ in plan.skipped})


def test_errors_and_empty_input():
    for bad in ([[0, 0, 1]], [[0.0, 0.0, 32.0, 64.0]], np.zeros((2, 2, 4), np.int32), [1, 2, 3, 4]):
        with pytest.raises(ValueError):
            P.plan_page(bad, (96, 200))
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            P.plan_page([(0, 0, 32, 64)], (96, 200), bucket_size=bad)
    for empty in ([], np.zeros((0, 4), np.int32)):
        plan = P.plan_page(empty, (96, 200))
        assert plan.n_boxes == 0 and plan.batches == [] and plan.skipped == []
        assert plan.jobs.shape == (0, 8) and plan.arena_bytes == 0
