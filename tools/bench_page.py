"""Timing of ocrk_page_minmax + ocrk_page_crops, a page's line crops cut, resized and
bucketed on the GPU, against the host path they replace.

The workload: a 1536 x 2048 float32 page (seeded noise) with 120 line boxes, heights
20..60 and widths 200..1400, planned by page.plan_page (bucket_size 16).

  minmax    the C entry alone on preallocated buffers: its 16-byte workspace memset and
            one kernel; reads the page once.
  crops     the C entry alone: one launch for every crop; reads the four neighbours of
            every sampled pixel (counted once each: 16 bytes per sample, an upper bound on
            what reaches HBM, since neighbours share cache lines), writes the arena.
  both      the two entries back to back, as page.page_crops issues them.
  public    page.page_crops on a device page: the same with its allocations and the
            upload of the job table and widths.
  host      the path the launch replaces, wall clock: the float64 NumPy crops of
            tests/page_crops_ref.py, Bucket padding and fill_batch (server.py), and one
            upload per batch ending in a synchronise; the NumPy part and the uploads
            are also given apart. The NumPy reference stands in for cv2.resize, which
            is not a dependency here: it is slower than OpenCV's C++ would be, so the
            upload share is the part of this figure that does not depend on that.

Device routes are timed with device events, each run ending in a synchronise; medians of
--runs runs (>= 20) after --warmup warm-up runs, the routes alternating. The fraction of
HBM bandwidth is bytes / time over 8 TB/s (the MI355X's peak). Prints one JSON object;
--out writes it.

    python tools/bench_page.py [--out profiles/page_crops_time.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import page_crops_ref as R
from cnn_lstm_ctc_ocr_amd import _lib
from cnn_lstm_ctc_ocr_amd import page as P

HBM_PEAK = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--host-runs", type=int, default=3, help="repetitions of the host path (seconds each)")
args = ap.parse_args()
if args.runs < 20:
    ap.error("--runs must be at least 20")
if not torch.cuda.is_available():
    sys.exit("bench_page.py needs the GPU: there is no CPU route to time")
dev = torch.device("cuda:0")
rng = np.random.default_rng(1234)
H, W, NBOX = 1536, 2048, 120
page = rng.random((H, W), dtype=np.float32)
boxes = []
for _ in range(NBOX):
    h, w = int(rng.integers(20, 61)), int(rng.integers(200, 1401))
    y0, x0 = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
    boxes.append((y0, x0, y0 + h, x0 + w))
plan = P.plan_page(boxes, (H, W), bucket_size=16)
kept = plan.jobs[plan.jobs[:, 7] >= 0]
samples = int(32 * kept[:, 4].sum())

dpage = torch.from_numpy(page).to(dev)
djobs = torch.from_numpy(plan.jobs).to(dev)
arena = torch.empty(plan.arena_bytes, dtype=torch.uint8, device=dev)
mm = torch.empty(2, dtype=torch.float32, device=dev)
ws = torch.empty(16, dtype=torch.uint8, device=dev)
mm_args = (_lib.ptr(dpage), _lib.F32, H * W, _lib.ptr(mm), _lib.ptr(ws), _lib.stream_ptr(dev))
crop_args = (_lib.ptr(dpage), _lib.F32, H, W, _lib.ptr(djobs), ctypes.c_void_p(plan.jobs.ctypes.data),
             plan.jobs.shape[0], _lib.ptr(arena), plan.arena_bytes, _lib.ptr(mm), P.NORMALIZED_MAX * 255.0,
             _lib.stream_ptr(dev))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def both():
    _lib.call("ocrk_page_minmax", *mm_args)
    _lib.call("ocrk_page_crops", *crop_args)


routes = {
    "minmax_c_entry": lambda: _lib.call("ocrk_page_minmax", *mm_args),
    "crops_c_entry": lambda: _lib.call("ocrk_page_crops", *crop_args),
    "both_c_entries": both,
    "public_page_crops_device_page": lambda: P.page_crops(dpage, plan),
}
for fn in routes.values():
    for _ in range(args.warmup):
        fn()
torch.cuda.synchronize()
times = {name: [] for name in routes}
for _ in range(args.runs):                                   # alternating: every route sees the same machine
    for name, fn in routes.items():
        times[name].append(timed(fn))


def stats(ts, nbytes=None):
    med = float(np.median(ts))
    out = {"median_us": round(med, 1), "min_us": round(float(np.min(ts)), 1), "max_us": round(float(np.max(ts)), 1)}
    if nbytes is not None:
        out["bytes"] = int(nbytes)
        out["GB_per_s"] = round(nbytes / med / 1e3, 1)
        out["fraction_of_hbm_peak"] = round(nbytes / (med * 1e-6) / HBM_PEAK, 4)
    return out


bytes_mm = {"read": H * W * 4, "written": 8}
bytes_crops = {"read_upper_bound": samples * 16 + plan.jobs.nbytes, "written": plan.arena_bytes}


def host_path():
    """(total, numpy, upload) seconds of the path the launch replaces, and its batches."""
    t0 = time.perf_counter()
    lines = R.page_lines(page, boxes, normalize=True, pad=1)
    batches = R.host_batches(lines, bucket_size=16)
    t1 = time.perf_counter()
    on_dev = [(torch.from_numpy(b).to(dev), torch.from_numpy(w).to(dev)) for _, b, w in batches]
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return t2 - t0, t1 - t0, t2 - t1, on_dev


host = [host_path() for _ in range(args.host_runs)]
host_batches = host[-1][3]

# the launch and the host path must describe the same batches: every pixel within one grey level
got = P.page_crops(dpage, plan)
assert len(got) == len(host_batches)
worst, differing, total = 0, 0, 0
for (gb, gw), (hb, hw) in zip(got, host_batches):
    assert gb.shape == hb.shape and torch.equal(gw, hw)
    d = (gb.to(torch.int16) - hb.to(torch.int16)).abs()
    worst, differing, total = max(worst, int(d.max())), differing + int((d != 0).sum()), total + d.numel()

res = {
    "command": f"python tools/bench_page.py --runs {args.runs} --warmup {args.warmup}",
    "library": os.path.basename(_lib.LIB_PATH),
    "workload": {"page": [H, W], "dtype": "float32", "boxes": NBOX, "box_heights": [20, 60],
                 "kept": int(len(kept)), "skipped": len(plan.skipped), "batches": len(plan.batches),
                 "jobs": int(plan.jobs.shape[0]), "sampled_pixels": samples, "arena_bytes": plan.arena_bytes,
                 "bucket_size": 16},
    "runs": args.runs, "warmup": args.warmup, "hbm_peak_bytes_per_s": HBM_PEAK,
    "minmax_c_entry": dict(stats(times["minmax_c_entry"], sum(bytes_mm.values())), **bytes_mm),
    "crops_c_entry": dict(stats(times["crops_c_entry"], sum(bytes_crops.values())), **bytes_crops),
    "both_c_entries": stats(times["both_c_entries"], sum(bytes_mm.values()) + sum(bytes_crops.values())),
    "public_page_crops_device_page": stats(times["public_page_crops_device_page"]),
    "host_path_replaced": {
        "runs": args.host_runs,
        "total_ms": round(float(np.median([h[0] for h in host])) * 1e3, 2),
        "numpy_crops_and_bucket_padding_ms": round(float(np.median([h[1] for h in host])) * 1e3, 2),
        "per_batch_uploads_ms": round(float(np.median([h[2] for h in host])) * 1e3, 3),
        "uploaded_bytes": int(sum(b.numel() + 4 * w.numel() for b, w in host_batches)),
    },
    "agreement_with_host_path": {"pixels": total, "differing": differing, "largest_difference": worst},
}
print(json.dumps(res, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
