"""The page -> line crop rule in float64 NumPy: the statement the device kernel
(ocrk_page_crops) is checked against, and the host path it replaces.

A box is (y0, x0, y1, x1), half-open, already inside the page. Its crop is 32 x nw, sampled
with the half-pixel-centre bilinear rule of cv2.resize(..., INTER_LINEAR), per axis: for
destination index d of n over s source pixels

    c = (d + 0.5) * s / n - 0.5,  i = floor(c),  f = c - i,
    i < 0 -> (0, 0),  i >= s - 1 -> (s - 1, 0),
    value = p[i] * (1 - f) + p[min(i + 1, s - 1)] * f

with i and f taken from integers (num = (2d + 1) s - n, i = num div 2n, f = (num - 2n i) /
2n), so nothing depends on where the box lies in the page. The output pixel is
clamp(floor((value - lo) * gain), 0, 255); crop_values returns (value - lo) * gain, the
number before the floor.
"""
import numpy as np

HEIGHT = 32


def new_width(h, w):
    """pagepredictor.py:324, in Python float64."""
    return int(32.0 / h * w)


def axis(n, s):
    """(i int64 [n], f float64 [n]) of the n destination indices over s source pixels."""
    d = np.arange(n, dtype=np.int64)
    num = (2 * d + 1) * s - n
    i = np.floor_divide(num, 2 * n)
    f = (num - 2 * n * i) / float(2 * n)
    low, high = i < 0, i >= s - 1
    i = np.where(low, 0, np.where(high, s - 1, i))
    f = np.where(low | high, 0.0, f)
    return i, f


def resize(src, nw):
    """The 32 x nw bilinear resize of src [h, w] (any real dtype), float64."""
    src = np.asarray(src, np.float64)
    h, w = src.shape
    iy, fy = axis(HEIGHT, h)
    ix, fx = axis(nw, w)
    iy1, ix1 = np.minimum(iy + 1, h - 1), np.minimum(ix + 1, w - 1)
    rows = src[:, ix] * (1.0 - fx) + src[:, ix1] * fx                       # [h, nw]
    return rows[iy] * (1.0 - fy)[:, None] + rows[iy1] * fy[:, None]       # [32, nw]


def lo_gain(page, normalize):
    """(lo, gain) of the output pixel: normalize = cv2.normalize(page, None, 0, 0.999, NORM_MINMAX)
    then * 255; else a float32 page is [0, 1] and a uint8 page grey levels."""
    if normalize:
        lo, hi = float(page.min()), float(page.max())
        return lo, (0.999 * 255.0 / (hi - lo) if hi > lo else 0.0)
    return 0.0, (1.0 if page.dtype == np.uint8 else 255.0)


def crop_values(page, box, nw, normalize):
    """(value - lo) * gain, float64 [32, nw]: the crop of `box` before the floor."""
    y0, x0, y1, x1 = box
    lo, gain = lo_gain(page, normalize)
    return (resize(page[y0:y1, x0:x1], nw) - lo) * gain


def to_u8(values):
    return np.clip(np.floor(values), 0, 255).astype(np.uint8)


def clip_box(box, page_shape, pad):
    """extract_line (pagepredictor.py:240-247): grown by pad, clipped to the page; None if empty."""
    H, W = page_shape
    y0, x0, y1, x1 = (int(v) for v in box)
    y0, y1 = min(max(y0 - pad, 0), H), min(max(y1 + pad, 0), H)
    x0, x1 = min(max(x0 - pad, 0), W), min(max(x1 + pad, 0), W)
    return (y0, x0, y1, x1) if y0 < y1 and x0 < x1 else None


def page_lines(page, boxes, normalize=True, pad=1, accept_narrow=False):
    """The host path per box: the uint8 crop [32, nw], or None where pagepredictor.py:325 (and the
    32-wide crop no bucket takes) skips the box."""
    out = []
    for box in boxes:
        box = clip_box(box, page.shape, pad)
        if box is None:
            out.append(None)
            continue
        nw = new_width(box[2] - box[0], box[3] - box[1])
        if nw < 32 or nw > 1000 or (nw == 32 and not accept_narrow):
            out.append(None)
            continue
        out.append(to_u8(crop_values(page, box, nw, normalize)))
    return out


def host_batches(lines, bucket_size=16, accept_narrow=False):
    """LocalServer's bucketing of the crops of page_lines: [(box indices (-1 for a top-up row),
    batch uint8 [bs, 32, Wb, 1], widths int32 [bs])], buckets ascending, crops in box order, the
    last batch of a bucket topped up by server.fill_batch."""
    from cnn_lstm_ctc_ocr_amd.server import LocalServer, fill_batch
    srv = LocalServer(None, bucket_size=bucket_size, bucket_max_time=0.0, accept_narrow=accept_narrow)
    for i, line in enumerate(lines):
        if line is not None:
            srv.addImage("0", i, 0.0, line)
    out, now = [], 0.0
    for bucket in srv.buckets:
        while bucket.imgs:
            now += 1.0                                       # past bucket_max_time since the last batch
            infos, batch, widths = fill_batch(*bucket.getBatch(now=now), bucket_size)
            out.append(([int(imgid) if cid != "-1" else -1 for cid, imgid in infos], batch, widths))
    return out
