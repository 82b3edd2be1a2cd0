"""A page and its line boxes -> the recogniser's bucket batches, on the GPU.

The step before the recogniser in the reference, src/processing/pagepredictor.py:274,
319-328: min-max normalise the page, cut each line box (extract_line, :240-247: grown by
`pad`, clipped to the page), cv2.resize it to height 32 and width int(32.0 / h * w), * 255
as uint8; then server.LocalServer zero-pads each crop to its width bucket and tops a short
batch up with zero crops (server.py:29-34, 123-128). Here the page is uploaded once and two
launches (ocrk_page_minmax, ocrk_page_crops) leave every bucket's batch in device
memory, where server.Recognizer reads it.

plan_page is host-only bookkeeping (NumPy, no device): which boxes are kept, their buckets
and batches, and the job table the kernel walks. page_crops runs a plan on a page.
"""
from typing import List, NamedTuple, Tuple

import numpy as np

from .server import BUCKET_MAX_WIDTH, BUCKET_STEP

HEIGHT = 32                    # the recogniser's crop height
JOB_WORDS = 8                  # y0, x0, h, w, nw, Wb, arena offset / 32, box index (-1: a top-up crop)
NORMALIZED_MAX = 0.999         # cv2.normalize(page, None, 0.0, 0.999, NORM_MINMAX), pagepredictor.py:274


class PageBatch(NamedTuple):
    """One batch of a plan: rows [offset, offset + len(widths) * 32 * Wb) of the arena are its
    uint8 [bs, 32, Wb, 1] image."""
    bucket: int                # index into LocalServer(accept_narrow=...).buckets
    Wb: int                    # the bucket's upper width: every crop of the batch is padded to it
    offset: int                # first byte of the batch in the arena (a multiple of 32 * 32)
    widths: np.ndarray         # i32 [bs]: nw per crop; a top-up row carries widths[0]
    boxes: np.ndarray          # i32 [bs]: the box index per row, -1 for a top-up row


class PagePlan(NamedTuple):
    page_shape: Tuple[int, int]
    n_boxes: int
    jobs: np.ndarray                       # i32 [jobs, 8], one row per output crop (top-ups included)
    arena_bytes: int
    batches: List[PageBatch]
    skipped: List[Tuple[int, str]]         # (box index, "empty" | "narrow" | "wide"), in box order


def new_width(h, w):
    """The reference's newwidth (pagepredictor.py:324), in Python float64."""
    return int(32.0 / h * w)


def bucket_of(nw, accept_narrow=False):
    """(index into LocalServer(accept_narrow=...).buckets, upper width Wb) of the bucket (lo, lo + 32]
    that takes a crop nw wide, or None where no bucket does."""
    if nw < 1 or nw > BUCKET_MAX_WIDTH or (nw <= BUCKET_STEP and not accept_narrow):
        return None
    lo = (nw - 1) // BUCKET_STEP * BUCKET_STEP
    return lo // BUCKET_STEP - (0 if accept_narrow else 1), lo + BUCKET_STEP


def plan_page(boxes, page_shape, bucket_size=16, accept_narrow=False, pad=1):
    """Plan the crops of one page. boxes: integers [n, 4], rows (y0, x0, y1, x1), half-open, in
    page pixels. A box that gives no crop is skipped and listed in .skipped, never raised on."""
    boxes = np.asarray(boxes)
    if boxes.size == 0 and boxes.ndim <= 2:
        boxes = np.zeros((0, 4), np.int64)
    if boxes.ndim != 2 or boxes.shape[1] != 4 or not np.issubdtype(boxes.dtype, np.integer):
        raise ValueError(f"plan_page: boxes is an integer array [n, 4], not {boxes.dtype} {list(boxes.shape)}")
    if int(bucket_size) != bucket_size or bucket_size < 1:
        raise ValueError(f"plan_page: bucket_size is an integer >= 1 (got {bucket_size})")
    bucket_size, pad = int(bucket_size), int(pad)
    H, W = int(page_shape[0]), int(page_shape[1])
    skipped, kept = [], {}                                   # bucket -> [(box, y0, x0, h, w, nw)]
    for i, (y0, x0, y1, x1) in enumerate(boxes.tolist()):
        y0, y1 = min(max(y0 - pad, 0), H), min(max(y1 + pad, 0), H)
        x0, x1 = min(max(x0 - pad, 0), W), min(max(x1 + pad, 0), W)
        if not (y0 < y1 and x0 < x1):
            skipped.append((i, "empty"))
            continue
        h, w = y1 - y0, x1 - x0
        nw = new_width(h, w)
        if nw < HEIGHT or (nw == HEIGHT and not accept_narrow):
            skipped.append((i, "narrow"))
        elif nw > BUCKET_MAX_WIDTH:
            skipped.append((i, "wide"))
        else:
            kept.setdefault(bucket_of(nw, accept_narrow), []).append((i, y0, x0, h, w, nw))
    jobs, batches, offset = [], [], 0
    for (bucket, Wb), crops in sorted(kept.items()):
        for k in range(0, len(crops), bucket_size):
            part = crops[k:k + bucket_size]
            widths = [c[5] for c in part] + [part[0][5]] * (bucket_size - len(part))
            idx = [c[0] for c in part] + [-1] * (bucket_size - len(part))
            for r in range(bucket_size):
                off32 = (offset + r * HEIGHT * Wb) // 32
                if r < len(part):
                    i, y0, x0, h, w, nw = part[r]
                    jobs.append((y0, x0, h, w, nw, Wb, off32, i))
                else:
                    jobs.append((0, 0, 0, 0, 0, Wb, off32, -1))
            batches.append(PageBatch(bucket, Wb, offset, np.array(widths, np.int32), np.array(idx, np.int32)))
            offset += bucket_size * HEIGHT * Wb
    table = np.array(jobs, np.int32).reshape(-1, JOB_WORDS)
    return PagePlan((H, W), len(boxes), table, offset, batches, skipped)


def page_crops(page, plan, normalize=True, device=None):
    """Run `plan` on `page`: [(batch uint8 [bs, 32, Wb, 1], widths int32 [bs]), ...] on the device,
    one pair per plan.batches entry, all views of one arena.

    page: uint8 or float32 [H, W], a NumPy array (uploaded once) or a device tensor. normalize:
    the reference's min-max normalisation of the page to [0, 0.999] before the * 255 (the minimum
    and maximum stay on the device); without it a float32 page is taken as [0, 1] and a uint8
    page as grey levels. One launch of each kernel, no host sync."""
    import torch

    from . import kernels as K
    if isinstance(page, torch.Tensor):
        if not page.is_cuda:
            page = page.to(device if device is not None else "cuda", non_blocking=True)
    else:
        page = np.ascontiguousarray(page)
        if page.dtype not in (np.uint8, np.float32):
            raise TypeError(f"page_crops takes a uint8 or float32 page, not {page.dtype}")
        page = torch.from_numpy(page).to(device if device is not None else "cuda", non_blocking=True)
    if page.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"page_crops takes a uint8 or float32 page, not {page.dtype}")
    if tuple(page.shape) != tuple(plan.page_shape):
        raise ValueError(f"page_crops: the page is {tuple(page.shape)}, the plan was made for {plan.page_shape}")
    if not plan.batches:
        return []
    dev = page.device
    page = page.contiguous()
    widths = np.concatenate([b.widths for b in plan.batches])
    # the table and the widths travel in one small upload: [jobs, 8] then [jobs]
    both = torch.from_numpy(np.concatenate([plan.jobs.reshape(-1), widths])).to(dev, non_blocking=True)
    n = plan.jobs.shape[0]
    jobs, widths = both[:n * JOB_WORDS].view(n, JOB_WORDS), both[n * JOB_WORDS:]
    arena = torch.empty(plan.arena_bytes, dtype=torch.uint8, device=dev)
    if normalize:
        K.page_crops(page, jobs, plan.jobs, arena, K.page_minmax(page), NORMALIZED_MAX * 255.0)
    else:
        K.page_crops(page, jobs, plan.jobs, arena, None, 255.0 if page.dtype == torch.float32 else 1.0)
    out, row = [], 0
    for b in plan.batches:
        bs = len(b.widths)
        out.append((arena[b.offset:b.offset + bs * HEIGHT * b.Wb].view(bs, HEIGHT, b.Wb, 1), widths[row:row + bs]))
        row += bs
    return out
