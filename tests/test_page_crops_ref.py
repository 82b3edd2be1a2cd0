"""tests/page_crops_ref.py against itself: the cases where the half-pixel-centre bilinear
rule has a closed form (no GPU)."""
import numpy as np

import page_crops_ref as R


def _page(seed=0, shape=(96, 200)):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def test_height_32_same_width_is_the_source():
    page = _page()
    box = (10, 7, 42, 107)                                   # h = 32, w = 100 -> nw = 100
    assert R.new_width(32, 100) == 100
    np.testing.assert_array_equal(R.crop_values(page, box, 100, False), page[10:42, 7:107].astype(np.float64))


def test_height_64_even_width_is_the_2x2_block_means():
    page = _page(1)
    box = (3, 20, 67, 140)                                   # h = 64, w = 120 -> nw = 60
    assert R.new_width(64, 120) == 60
    src = page[3:67, 20:140].astype(np.float64)
    means = src.reshape(32, 2, 60, 2).mean(axis=(1, 3))
    np.testing.assert_array_equal(R.crop_values(page, box, 60, False), means)


def test_constant_page_gives_a_constant():
    page = np.full((50, 80), 0.25, np.float32)
    v = R.crop_values(page, (5, 3, 28, 77), R.new_width(23, 74), False)
    np.testing.assert_array_equal(v, np.full_like(v, 0.25 * 255.0))
    assert (R.crop_values(page, (5, 3, 28, 77), R.new_width(23, 74), True) == 0).all()   # max == min: gain 0


def test_values_stay_within_the_source_range():
    rng = np.random.default_rng(2)
    page = rng.random((96, 200), dtype=np.float32)
    for h, w in ((7, 40), (23, 100), (45, 91), (96, 200), (8, 12)):
        src = page[96 - h:, 200 - w:]
        out = R.resize(src, max(R.new_width(h, w), 1))
        assert out.shape == (32, max(R.new_width(h, w), 1))
        assert src.min() <= out.min() and out.max() <= src.max()


def test_axis_rule_against_the_float_formula():
    """The integer form of (i, f) is the half-pixel-centre formula."""
    for n, s in ((32, 7), (32, 96), (65, 131), (33, 8), (100, 100), (5, 1)):
        i, f = R.axis(n, s)
        c = (np.arange(n) + 0.5) * s / n - 0.5
        fi = np.floor(c).astype(np.int64)
        low, high = fi < 0, fi >= s - 1
        np.testing.assert_array_equal(i, np.where(low, 0, np.where(high, s - 1, fi)))
        np.testing.assert_allclose(f, np.where(low | high, 0.0, c - fi), atol=1e-12)


def test_normalized_output_spans_0_to_254():
    page = _page(3)
    lo, gain = R.lo_gain(page, True)
    assert lo == page.min() and gain == 0.999 * 255.0 / (float(page.max()) - float(page.min()))
    out = R.to_u8(R.crop_values(page, (0, 0, 32, 200), 200, True))
    assert out.min() == 0 and out.max() == 254               # 0.999 * 255 = 254.745
