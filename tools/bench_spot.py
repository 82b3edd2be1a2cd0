"""Timing of ocrk_ctc_spot, keyword spotting on the CTC lattice (DESIGN.md
section 3d).

The fp32 serving shape: B = 64 rows of T = 125 frames, C = 96 (ReLU'd Gaussian
logits from a seed), and the 64 keywords of 3..16 characters below.

  entry     the C entry alone on preallocated buffers (no allocator, no wrapper
            work beyond the ctypes call), case-sensitive (no alternatives table)
            and case-insensitive (an alternative per letter).
  wrapper   kernels.ctc_spot: the same call with its allocations.
  lexicon   for scale, ocrk_ctc_lexicon_score on the same logits with the same 64
            labels as a word list (the C entry alone): the full CTC sum of every
            word over the whole row, where spotting is a max-plus recursion with a
            free start and end.
  service   Recognizer(store, keywords=...) against the same Recognizer without
            keywords: wall time per batch of 64 crops of 32 x 256 (a seed-0 fp32
            LSTM 512/512 store), read-back and host work included.

The device routes are timed with device events and each run ends in a
synchronise; medians of --runs runs (>= 20) after --warmup warm-up runs. Prints
one JSON object; --out writes it.

    python tools/bench_spot.py [--out profiles/ctc_spot_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cnn_lstm_ctc_ocr_amd import _lib, decode
from cnn_lstm_ctc_ocr_amd import kernels as K

# What a receipt reader looks for inside its lines; 3..16 characters each.
KEYWORDS = [
    "total", "subtotal", "sub total", "grand total", "total due", "amount due", "balance", "balance due",
    "gst", "vat", "tax", "sales tax", "service charge", "tip", "gratuity", "rounding",
    "cash", "change", "change due", "tendered", "card", "visa", "mastercard", "debit",
    "credit", "approved", "auth code", "terminal", "merchant", "merchant id", "batch", "invoice",
    "invoice no", "receipt", "receipt no.", "order", "order no", "table", "guests", "server",
    "cashier", "date", "time", "tel", "phone", "fax", "www.", "reg no",
    "tax invoice", "qty", "item", "price", "amount", "discount", "member", "points",
    "thank you", "welcome", "refund", "exchange", "no refund", "net total", "total amount due", "items sold",
]

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--no-service", action="store_true", help="skip the Recognizer timing (kernel variants)")
args = ap.parse_args()
if args.runs < 20:
    ap.error("--runs must be at least 20")
if not torch.cuda.is_available():
    sys.exit("bench_spot.py needs the GPU: there is no CPU route to time")
dev = torch.device("cuda:0")
rng = np.random.default_rng(1234)
T, B, C = 125, 64, 96
logits = torch.from_numpy(np.maximum(rng.standard_normal((T, B, C)) * 3, 0).astype(np.float32)).to(dev)
seq = torch.full((B,), T, dtype=torch.int32, device=dev)
kset = decode.KeywordSet(KEYWORDS, case_insensitive=True)
NK = len(kset)
assert NK == 64 and 3 <= int(kset.lengths.min()) and int(kset.lengths.max()) <= 16
lab, alt, ln = kset.tensors(dev)
W = lab.shape[1]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def spot_entry(with_alt):
    nb = _lib.lib().ocrk_ctc_spot_workspace_size(T, B, C, NK, W)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    score = torch.empty(B, NK, dtype=torch.float32, device=dev)
    span = torch.empty(B, NK, 2, dtype=torch.int32, device=dev)
    st = torch.empty(NK, dtype=torch.int32, device=dev)
    a = (_lib.ptr(logits), _lib.ptr(seq), T, B, C, _lib.ptr(lab), _lib.ptr(alt) if with_alt else None, _lib.ptr(ln),
         NK, W, _lib.ptr(score), _lib.ptr(span), _lib.ptr(st), None, _lib.ptr(ws), nb, _lib.stream_ptr(dev))
    keep = (ws, score, span, st)
    return lambda: (_lib.call("ocrk_ctc_spot", *a), keep)


def lexicon_entry():
    nb = _lib.lib().ocrk_ctc_lexicon_workspace_size(T, B, C, NK, W)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    logp = torch.empty(B, NK, dtype=torch.float32, device=dev)
    ti = torch.empty(B, 1, dtype=torch.int32, device=dev)
    tl = torch.empty(B, 1, dtype=torch.float32, device=dev)
    nm = torch.empty(B, dtype=torch.float32, device=dev)
    st = torch.empty(NK, dtype=torch.int32, device=dev)
    a = (_lib.ptr(logits), _lib.ptr(seq), T, B, C, _lib.ptr(lab), _lib.ptr(ln), NK, W, 1, _lib.ptr(logp),
         _lib.ptr(ti), _lib.ptr(tl), _lib.ptr(nm), _lib.ptr(st), None, _lib.ptr(ws), nb, _lib.stream_ptr(dev))
    keep = (ws, logp, ti, tl, nm, st)
    return lambda: (_lib.call("ocrk_ctc_lexicon_score", *a), keep)


def stats(ts):
    return {"median_us": round(float(np.median(ts)), 1), "min_us": round(float(np.min(ts)), 1),
            "max_us": round(float(np.max(ts)), 1)}


routes = {
    "c_entry_case_sensitive": spot_entry(False),
    "c_entry_case_insensitive": spot_entry(True),
    "wrapper_case_sensitive": lambda: K.ctc_spot(logits, seq, lab, None, ln),
    "wrapper_case_insensitive": lambda: K.ctc_spot(logits, seq, lab, alt, ln),
    "lexicon_score_c_entry_same_labels": lexicon_entry(),
}
for fn in routes.values():
    for _ in range(args.warmup):
        fn()
torch.cuda.synchronize()
times = {name: [] for name in routes}
for _ in range(args.runs):                                   # alternating: every route sees the same machine
    for name, fn in routes.items():
        times[name].append(timed(fn))
K.check_status(dev)

res = {
    "command": f"python tools/bench_spot.py --runs {args.runs} --warmup {args.warmup}",
    "library": os.path.basename(_lib.LIB_PATH),
    "shape": {"T": T, "B": B, "C": C, "n_kw": NK, "kw_len": [int(kset.lengths.min()), int(kset.lengths.max())],
              "label_width": W, "dtype": "float32"},
    "runs": args.runs, "warmup": args.warmup,
}
res.update({name: stats(ts) for name, ts in times.items()})
score, span, _ = K.ctc_spot(logits, seq, lab, alt, ln)
res["hits_at_ln_half"] = int((score >= np.log(0.5)).sum().item())

if not args.no_service:
    from cnn_lstm_ctc_ocr_amd import ModelConfig, ParamStore
    from cnn_lstm_ctc_ocr_amd.server import Recognizer
    store = ParamStore(ModelConfig(cell="lstm", rnn_sizes=(512, 512), dtype=torch.float32), device=dev, seed=0)
    batch = rng.integers(0, 256, (B, 32, 256, 1)).astype(np.uint8)
    widths = np.full(B, 256, np.int32)

    def wall(rec):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec(batch, widths)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    service = {}
    for graphs in (False, True):
        # an untrained store's logits are nearly flat, so at the default threshold most keywords "hit" and the
        # host builds thousands of KeywordHit tuples; threshold 0 (exact hits only) shows the cost without them
        recs = {"plain": Recognizer(store, graphs=graphs),
                "keywords": Recognizer(store, graphs=graphs, keywords=kset),
                "keywords_thr0": Recognizer(store, graphs=graphs, keywords=kset, keyword_threshold=0.0)}
        for rec in recs.values():
            for _ in range(args.warmup):
                rec(batch, widths)
        ts = {name: [] for name in recs}
        for _ in range(args.runs):
            for name, rec in recs.items():
                ts[name].append(wall(rec))
        med = {name: float(np.median(v)) for name, v in ts.items()}
        hits = {name: sum(len(r.hits) for r in recs[name](batch, widths)) for name in ("keywords", "keywords_thr0")}
        service["graphs" if graphs else "eager"] = {
            "plain_ms": round(med["plain"], 3),
            "with_keywords_ms": round(med["keywords"], 3), "overhead_ms": round(med["keywords"] - med["plain"], 3),
            "hits_per_batch": hits["keywords"],
            "with_keywords_threshold_0_ms": round(med["keywords_thr0"], 3),
            "overhead_threshold_0_ms": round(med["keywords_thr0"] - med["plain"], 3),
            "hits_per_batch_threshold_0": hits["keywords_thr0"]}
    res["recognizer_wall_per_64_crop_batch"] = dict(service, crop="32 x 256", store="fp32 LSTM 512/512, seed 0")

print(json.dumps(res, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
