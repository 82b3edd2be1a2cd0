"""ocrk_page_minmax / ocrk_page_crops against tests/page_crops_ref.py, the entry's
validation, and Recognizer.page against the host path it replaces (reference crops through
LocalServer's Bucket + fill_batch into Recognizer.__call__).

Exact cases: a uint8 page without normalisation and boxes 32, 64 (even width), 16 and 8 rows
high. Every weight is then dyadic and every intermediate a small multiple of a power of two
below 256, so float32 evaluates the rule exactly in any order, fused or not: torch.equal.

Tolerance cases: with v the float64 reference value and DELTA = 1e-3 every pixel must lie in
[floor(v - DELTA), floor(v + DELTA)]. About ten float32 roundings on magnitudes <= 255 bound
the error near 1.5e-4, so DELTA has a margin of about 6; at most CAP = 0.5 % of the pixels may
have two admissible values (asserted on the inputs used here), so the rule cannot hide a
wrong kernel."""
import numpy as np
import pytest
import torch

import page_crops_ref as R
from oracle import ref_model as M

pytestmark = pytest.mark.gpu

H, W = 96, 200
FILL, GUARD = 7, 4096
DELTA, CAP = 1e-3, 0.005
SIZES = (64, 64)

# (y0, x0, y1, x1) with pad = 0: heights 32, 64 (even widths), 16, 8; the page's corners and edges;
# five crops 100 wide, so that their bucket makes two batches of four
EXACT_BOXES = [(10, 7, 42, 107), (0, 0, 32, 33), (64, 100, 96, 200), (50, 20, 82, 120), (3, 20, 67, 140),
               (32, 0, 96, 200), (5, 5, 21, 45), (80, 150, 96, 200), (40, 10, 48, 30), (88, 0, 96, 50),
               (0, 0, 64, 62), (20, 20, 20, 90)]                       # the last two: narrow, empty
# with pad = 2: heights 7, 23, 45, 96 after padding and clipping, the right and bottom edges
TOL_BOXES = [(2, 2, 94, 98), (-5, 100, 120, 210), (91, 150, 96, 198), (60, 30, 79, 72), (75, 154, 100, 204),
             (30, 105, 71, 193), (53, 112, 96, 198), (2, 12, 5, 180)]
TOL_PAD = 2


def _u8_page(seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.uint8)


def _f32_page(seed=1):
    return (np.random.default_rng(seed).random((H, W), dtype=np.float32) * 1.5 - 0.25).astype(np.float32)


def _launch(cuda, page, plan, normalize, jobs=None, arena_bytes=None):
    """The arena (NumPy) and the guard behind it after one launch on a buffer prefilled with FILL."""
    from cnn_lstm_ctc_ocr_amd import kernels as K
    jobs = plan.jobs if jobs is None else jobs
    n = plan.arena_bytes if arena_bytes is None else arena_bytes
    buf = torch.full((n + GUARD,), FILL, dtype=torch.uint8, device=cuda)
    dpage = torch.from_numpy(page).to(cuda)
    if normalize:
        mm, scale = K.page_minmax(dpage), 0.999 * 255.0
    else:
        mm, scale = None, (1.0 if page.dtype == np.uint8 else 255.0)
    try:
        K.page_crops(dpage, torch.from_numpy(jobs).to(cuda), jobs, buf[:n], mm, scale)
    finally:
        out = buf.cpu().numpy()
    return out[:n], out[n:]


def _bounds(page, plan, normalize, delta):
    """(lowest, highest) admissible arena bytes and the mask of sampled pixels."""
    lo = np.zeros(plan.arena_bytes, np.uint8)
    hi = np.zeros(plan.arena_bytes, np.uint8)
    sampled = np.zeros(plan.arena_bytes, bool)
    for y0, x0, h, w, nw, Wb, off32, box in plan.jobs.tolist():
        if box < 0:
            continue
        v = R.crop_values(page, (y0, x0, y0 + h, x0 + w), nw, normalize)
        view = slice(off32 * 32, off32 * 32 + 32 * Wb)
        lo[view].reshape(32, Wb)[:, :nw] = R.to_u8(v - delta)
        hi[view].reshape(32, Wb)[:, :nw] = R.to_u8(v + delta)
        sampled[view].reshape(32, Wb)[:, :nw] = True
    return lo, hi, sampled


def test_exact_cases(cuda):
    from cnn_lstm_ctc_ocr_amd import page as P
    page = _u8_page()
    plan = P.plan_page(EXACT_BOXES, (H, W), bucket_size=4, pad=0)
    assert plan.skipped == [(10, "narrow"), (11, "empty")]
    assert sorted({int(r[2]) for r in plan.jobs if r[7] >= 0}) == [8, 16, 32, 64]
    assert [b.Wb for b in plan.batches] == [64, 96, 128, 128, 224] and (plan.jobs[:, 7] < 0).sum() == 10
    want, same, _ = _bounds(page, plan, False, 0.0)
    assert (want == same).all()
    arena, guard = _launch(cuda, page, plan, False)
    assert torch.equal(torch.from_numpy(arena), torch.from_numpy(want))     # samples, padding and top-ups
    assert (guard == FILL).all()
    # the public call gives the same bytes as views of its own arena, and the widths
    got = P.page_crops(page, plan, normalize=False, device=cuda)
    assert len(got) == len(plan.batches)
    for (batch, widths), b in zip(got, plan.batches):
        assert batch.shape == (4, 32, b.Wb, 1) and batch.dtype == torch.uint8 and batch.is_contiguous()
        assert widths.dtype == torch.int32 and widths.cpu().tolist() == b.widths.tolist()
        assert torch.equal(batch.cpu().reshape(-1), torch.from_numpy(want[b.offset:b.offset + 4 * 32 * b.Wb]))
    dev = P.page_crops(torch.from_numpy(page).to(cuda), plan, normalize=False)   # a device page
    assert all(torch.equal(a[0], b[0]) for a, b in zip(dev, got))
    assert P.page_crops(page, P.plan_page([], (H, W)), device=cuda) == []


@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_tolerance_cases(cuda, kind):
    from cnn_lstm_ctc_ocr_amd import page as P
    page = _f32_page() if kind == "f32" else _u8_page(2)
    plan = P.plan_page(TOL_BOXES, (H, W), bucket_size=3, pad=TOL_PAD)
    real = plan.jobs[plan.jobs[:, 7] >= 0]
    assert plan.skipped == [] and {7, 23, 45, 96} <= set(real[:, 2].tolist())
    assert {33, 64, 65} <= set(real[:, 4].tolist())
    assert (real[:, 0] + real[:, 2] == H).any() and (real[:, 1] + real[:, 3] == W).any()
    lo, hi, sampled = _bounds(page, plan, True, DELTA)
    two = int((lo != hi).sum())
    print(f"{kind}: {two} of {int(sampled.sum())} pixels have two admissible values "
          f"({100.0 * two / sampled.sum():.3f} %)")
    assert two <= CAP * sampled.sum()
    arena, guard = _launch(cuda, page, plan, True)
    off = (arena < lo) | (arena > hi)
    print(f"{kind}: {int(off.sum())} pixels outside [floor(v - {DELTA}), floor(v + {DELTA})]")
    assert not off.any()
    assert (arena[~sampled] == 0).all() and (guard == FILL).all()


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (H, W)])
def test_minmax(cuda, shape):
    from cnn_lstm_ctc_ocr_amd import kernels as K
    rng = np.random.default_rng(shape[0])
    f32 = (rng.standard_normal(shape) * 3).astype(np.float32)
    u8 = rng.integers(3, 250, shape).astype(np.uint8)
    for page in (f32, u8):
        got = K.page_minmax(torch.from_numpy(page).to(cuda)).cpu().numpy()
        assert got.dtype == np.float32 and got.tolist() == [float(page.min()), float(page.max())]
        # the same pixels one element off the allocation's alignment: the scalar head and tail
        flat = torch.from_numpy(np.concatenate([page.reshape(-1)[:1], page.reshape(-1)])).to(cuda)
        got = K.page_minmax(flat[1:].view(*shape)).cpu().numpy()
        assert got.tolist() == [float(page.min()), float(page.max())]
    if shape == (H, W):
        assert f32.min() < 0 < f32.max()
        f32[50, 100], f32[95, 199] = -1e30, 3e38                              # one pixel decides each
        assert K.page_minmax(torch.from_numpy(f32).to(cuda)).cpu().tolist() == [float(np.float32(-1e30)),
                                                                                float(np.float32(3e38))]


@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_constant_page_normalized_is_all_zero(cuda, kind):
    from cnn_lstm_ctc_ocr_amd import page as P
    page = np.full((H, W), 0.75, np.float32) if kind == "f32" else np.full((H, W), 200, np.uint8)
    plan = P.plan_page(TOL_BOXES, (H, W), bucket_size=3, pad=TOL_PAD)
    arena, guard = _launch(cuda, page, plan, True)
    assert (arena == 0).all() and (guard == FILL).all()


def test_validation_launches_nothing(cuda):
    from cnn_lstm_ctc_ocr_amd import _lib
    from cnn_lstm_ctc_ocr_amd import kernels as K
    from cnn_lstm_ctc_ocr_amd import page as P
    page = _u8_page()
    plan = P.plan_page(EXACT_BOXES, (H, W), bucket_size=4, pad=0)
    k = int(np.nonzero(plan.jobs[:, 7] >= 0)[0][-1])
    outside, past, wide = plan.jobs.copy(), plan.jobs.copy(), plan.jobs.copy()
    outside[k, 1] = W - outside[k, 3] + 1                                     # one column beyond the page
    past[-1, 6] += 1                                                         # the last crop ends 32 bytes late
    wide[k, 4] = wide[k, 5] + 1                                               # nw > Wb
    dpage = torch.from_numpy(page).to(cuda)
    for jobs, what in ((outside, "lie outside the 96 x 200 page"), (past, "lie outside the arena"), (wide, "nw=")):
        buf = torch.full((plan.arena_bytes + GUARD,), FILL, dtype=torch.uint8, device=cuda)
        with pytest.raises(_lib.InvalidArgumentError, match=what):
            K.page_crops(dpage, torch.from_numpy(jobs).to(cuda), jobs, buf[:plan.arena_bytes], None, 1.0)
        torch.cuda.synchronize()
        assert (buf == FILL).all()


def _store(cuda, seed=0):
    from cnn_lstm_ctc_ocr_amd import ModelConfig, ParamStore
    vals = M.init_params(seed=seed, rnn_sizes=SIZES)
    for k in vals:
        if "lstm_cell/kernel" in k:
            vals[k] = (vals[k] * 20).astype(np.float32)
    return ParamStore(ModelConfig(rnn_sizes=SIZES, dtype=torch.float32), device=cuda, values=vals)


@pytest.mark.parametrize("mode", ["plain", "detail", "graphs"])
def test_recognizer_page_end_to_end(cuda, mode):
    from cnn_lstm_ctc_ocr_amd.server import PageLines, Recognition, Recognizer
    page = _u8_page()
    rec = Recognizer(_store(cuda), detail=mode == "detail", graphs=mode == "graphs")
    # the host path: reference crops -> Bucket padding -> fill_batch -> Recognizer.__call__ on NumPy
    lines = R.page_lines(page, EXACT_BOXES, normalize=False, pad=0)
    batches = R.host_batches(lines, bucket_size=4)
    assert sum(b[1].shape[2] == 128 for b in batches) == 2                    # one bucket makes two batches
    want = [None] * len(EXACT_BOXES)
    for boxes, batch, widths in batches:
        for i, res in zip(boxes, rec(batch, widths)):
            if i >= 0:
                want[i] = res
    got = rec.page(page, EXACT_BOXES, normalize=False, bucket_size=4, pad=0)
    assert isinstance(got, PageLines) and got.skipped == [(10, "narrow"), (11, "empty")]
    assert got.results[10] is None and got.results[11] is None
    assert sum(r is not None for r in got.results) == 10
    assert all(isinstance(r, Recognition if mode == "detail" else str) for r in got.results[:10])
    assert got.results == want
    assert len({r.text if mode == "detail" else r for r in want[:10]}) > 1    # the strings say something
    # a NumPy batch and the same batch as device tensors read the same
    boxes, batch, widths = batches[0]
    assert rec(torch.from_numpy(batch).to(cuda), torch.from_numpy(widths).to(cuda)) == rec(batch, widths)
