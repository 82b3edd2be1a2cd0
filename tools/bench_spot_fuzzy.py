"""Timing of ocrk_ctc_spot_fuzzy, error-tolerant keyword spotting on the CTC
lattice, beside ocrk_ctc_spot on the same inputs.

tools/bench_spot.py's shape and keyword list: B = 64 rows of T = 125 frames,
C = 96 (ReLU'd Gaussian logits from the same seed), 64 keywords of 3..16
characters, case-insensitive (an alternative per letter), edit_cost 0.5.

  exact     ocrk_ctc_spot, the C entry alone on preallocated buffers.
  budget_0 / budget_1 / budget_2
            ocrk_ctc_spot_fuzzy, the C entry alone, every keyword with that
            budget (cut to len - 1).
  auto      the budgets of decode.FuzzyKeywordSet(..., "auto"):
            min(2, (len + 1) // 5).
  wrapper_auto
            kernels.ctc_spot_fuzzy: the same call with its allocations.
  service   Recognizer(store, keywords=..., keyword_errors="auto") against the
            same Recognizer with exact keywords and without keywords: wall time
            per batch of 64 crops of 32 x 256 (a seed-0 fp32 LSTM 512/512 store),
            read-back and host work included, at keyword_threshold 0.

The device routes alternate in one process, are timed with device events and
each run ends in a synchronise; medians of --runs runs (>= 20) after --warmup
warm-up runs. Prints one JSON object; --out writes it.

    python tools/bench_spot_fuzzy.py [--out profiles/ctc_spot_fuzzy_time.json]"""
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

# tools/bench_spot.py's list: what a receipt reader looks for inside its lines; 3..16 characters each.
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
EDIT_COST = 0.5

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--no-service", action="store_true", help="skip the Recognizer timing")
args = ap.parse_args()
if args.runs < 20:
    ap.error("--runs must be at least 20")
if not torch.cuda.is_available():
    sys.exit("bench_spot_fuzzy.py needs the GPU: there is no CPU route to time")
dev = torch.device("cuda:0")
rng = np.random.default_rng(1234)
T, B, C = 125, 64, 96
logits = torch.from_numpy(np.maximum(rng.standard_normal((T, B, C)) * 3, 0).astype(np.float32)).to(dev)
seq = torch.full((B,), T, dtype=torch.int32, device=dev)
kset = decode.FuzzyKeywordSet(KEYWORDS, "auto", case_insensitive=True)
NK = len(kset)
assert NK == 64 and 3 <= int(kset.lengths.min()) and int(kset.lengths.max()) <= 16
lab, alt, ln, auto = kset.fuzzy_tensors(dev)
W = lab.shape[1]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def exact_entry():
    nb = _lib.lib().ocrk_ctc_spot_workspace_size(T, B, C, NK, W)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    score = torch.empty(B, NK, dtype=torch.float32, device=dev)
    span = torch.empty(B, NK, 2, dtype=torch.int32, device=dev)
    st = torch.empty(NK, dtype=torch.int32, device=dev)
    a = (_lib.ptr(logits), _lib.ptr(seq), T, B, C, _lib.ptr(lab), _lib.ptr(alt), _lib.ptr(ln), NK, W,
         _lib.ptr(score), _lib.ptr(span), _lib.ptr(st), None, _lib.ptr(ws), nb, _lib.stream_ptr(dev))
    keep = (ws, score, span, st)
    return lambda: (_lib.call("ocrk_ctc_spot", *a), keep)


def fuzzy_entry(err):
    nb = _lib.lib().ocrk_ctc_spot_fuzzy_workspace_size(T, B, C, NK, W)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    score = torch.empty(B, NK, dtype=torch.float32, device=dev)
    span = torch.empty(B, NK, 2, dtype=torch.int32, device=dev)
    errors = torch.empty(B, NK, dtype=torch.int32, device=dev)
    st = torch.empty(NK, dtype=torch.int32, device=dev)
    a = (_lib.ptr(logits), _lib.ptr(seq), T, B, C, _lib.ptr(lab), _lib.ptr(alt), _lib.ptr(ln), _lib.ptr(err), NK, W,
         EDIT_COST, _lib.ptr(score), _lib.ptr(span), _lib.ptr(errors), _lib.ptr(st), None, _lib.ptr(ws), nb,
         _lib.stream_ptr(dev))
    keep = (ws, score, span, errors, st, err)
    return lambda: (_lib.call("ocrk_ctc_spot_fuzzy", *a), keep)


def stats(ts):
    return {"median_us": round(float(np.median(ts)), 1), "min_us": round(float(np.min(ts)), 1),
            "max_us": round(float(np.max(ts)), 1)}


def capped(e):
    return torch.minimum(torch.full_like(ln, e), ln - 1).contiguous()


routes = {
    "exact_c_entry": exact_entry(),
    "budget_0_c_entry": fuzzy_entry(capped(0)),
    "budget_1_c_entry": fuzzy_entry(capped(1)),
    "budget_2_c_entry": fuzzy_entry(capped(2)),
    "auto_c_entry": fuzzy_entry(auto),
    "wrapper_auto": lambda: K.ctc_spot_fuzzy(logits, seq, lab, alt, ln, auto, EDIT_COST),
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
    "command": f"python tools/bench_spot_fuzzy.py --runs {args.runs} --warmup {args.warmup}",
    "library": os.path.basename(_lib.LIB_PATH),
    "shape": {"T": T, "B": B, "C": C, "n_kw": NK, "kw_len": [int(kset.lengths.min()), int(kset.lengths.max())],
              "label_width": W, "dtype": "float32", "case_insensitive": True, "edit_cost": EDIT_COST,
              "auto_budgets": {str(e): int((kset.errors == e).sum()) for e in (0, 1, 2)}},
    "runs": args.runs, "warmup": args.warmup,
}
res.update({name: stats(ts) for name, ts in times.items()})
score, span, errors, _ = K.ctc_spot_fuzzy(logits, seq, lab, alt, ln, auto, EDIT_COST)
res["auto_hits_at_ln_half"] = int((score >= np.log(0.5)).sum().item())
res["auto_best_paths_by_errors"] = {str(e): int((errors == e).sum().item()) for e in (0, 1, 2)}

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
        # threshold 0 (hits that cost nothing only): an untrained store's logits are nearly flat, and at the
        # default threshold the host would build thousands of hit tuples (tools/bench_spot.py)
        recs = {"plain": Recognizer(store, graphs=graphs),
                "exact": Recognizer(store, graphs=graphs, keywords=KEYWORDS, case_insensitive=True,
                                    keyword_threshold=0.0),
                "fuzzy": Recognizer(store, graphs=graphs, keywords=kset, keyword_edit_cost=EDIT_COST,
                                    keyword_threshold=0.0)}
        for rec in recs.values():
            for _ in range(args.warmup):
                rec(batch, widths)
        ts = {name: [] for name in recs}
        for _ in range(args.runs):
            for name, rec in recs.items():
                ts[name].append(wall(rec))
        med = {name: float(np.median(v)) for name, v in ts.items()}
        service["graphs" if graphs else "eager"] = {
            "plain_ms": round(med["plain"], 3),
            "with_keywords_ms": round(med["exact"], 3), "with_keyword_errors_ms": round(med["fuzzy"], 3),
            "overhead_keywords_ms": round(med["exact"] - med["plain"], 3),
            "overhead_keyword_errors_ms": round(med["fuzzy"] - med["plain"], 3)}
    res["recognizer_wall_per_64_crop_batch"] = dict(service, crop="32 x 256", store="fp32 LSTM 512/512, seed 0",
                                                    keyword_threshold=0.0)

print(json.dumps(res, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
