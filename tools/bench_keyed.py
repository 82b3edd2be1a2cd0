"""Timing of ocrk_ctc_keyed_field, keyed field reading on the CTC lattice
(DESIGN.md section 3f).

The fp32 serving shape: B = 64 rows of T = 125 frames, C = 96 (ReLU'd Gaussian
logits from a seed), and the receipt-style keyed fields below: seven fields,
each a group of keywords and the pattern of the value that follows them.

  entry     the C entry alone on preallocated buffers (no allocator, no wrapper
            work beyond the ctypes call), on the LDS route and with CTC_LDS=0 on
            the workspace route.
  wrapper   kernels.ctc_keyed_field: the same call with its allocations.
  separate  for scale, ocrk_ctc_spot on the same flat keyword list and
            ocrk_ctc_field on the same patterns, each the C entry alone: the work
            the keyed entry contains, without the join (and without its answer).

The routes are timed with device events and each run ends in a synchronise; the
routes alternate in one process; medians of --runs runs (>= 20) after --warmup
warm-up runs. Nothing is gated on a time. Prints one JSON object; --out writes it.

    python tools/bench_keyed.py [--out profiles/ctc_keyed_time.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cnn_lstm_ctc_ocr_amd import _lib, decode, options
from cnn_lstm_ctc_ocr_amd import kernels as K

MONEY = r"[1-9]\d{0,3}\.\d{1,2}"
# What a receipt reader pairs: the words that announce a value, and the value's shape. Every keyword is within
# the spotter's 32 symbols.
KEYED = {
    "total": (["total", "grand total", "amount", "amount due", "total due", "balance due", "to pay", "net total",
               "sum", "ttl", "total incl. tax", "card", "paid"], MONEY),
    "subtotal": (["subtotal", "sub-total", "sub total", "subttl"], MONEY),
    "cash": (["cash", "cash tendered", "cash paid"], MONEY),
    "changedue": (["change", "change due", "your change", "cash back"], MONEY),
    "gst": (["gst", "G.S.T.", "gst incl.", "tax", "vat", "incl. gst", "tax amount"], r"\d{1,2}\.\d\d"),
    "servicecharge": (["service charge", "service chg", "svc charge", "SVC CHG", "serv. charge", "service fee"],
                      MONEY),
    "receiptid": (["receipt", "receipt no.", "receipt #", "rcpt", "rcpt no.", "bill", "bill no.", "invoice",
                   "invoice no.", "inv", "inv no.", "check", "chk", "order", "order no.", "ref", "ref no.", "doc no.",
                   "ticket", "ticket no.", "slip", "slip no.", "txn", "txn id", "trans", "trans no.", "serial",
                   "serial no.", "docket", "no."], r"\d{4,7}"),
}

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()
if args.runs < 20:
    ap.error("--runs must be at least 20")
if not torch.cuda.is_available():
    sys.exit("bench_keyed.py needs the GPU: there is no CPU route to time")
dev = torch.device("cuda:0")
rng = np.random.default_rng(1234)
T, B, C = 125, 64, 96
logits = torch.from_numpy(np.maximum(rng.standard_normal((T, B, C)) * 3, 0).astype(np.float32)).to(dev)
seq = torch.full((B,), T, dtype=torch.int32, device=dev)
keyed = decode.KeyedFieldSet(KEYED, case_insensitive=True)
lab, alt, ln, grp, cls, opt, pln = keyed.tensors(dev)
NK, WK = lab.shape
P, WP = opt.shape
GAP_COST = 0.02
p = _lib.ptr


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def buffers(*shapes):
    return [torch.empty(shape, dtype=dt, device=dev) for shape, dt in shapes]


def keyed_entry(lds=1):
    nb = _lib.lib().ocrk_ctc_keyed_field_workspace_size(T, B, C, NK, WK, P, WP)
    ws, score, span, kwi, kws, text, kst, pst = buffers(
        (nb, torch.uint8), ((B, P), torch.float32), ((B, P, 4), torch.int32), ((B, P), torch.int32),
        ((B, P), torch.float32), ((B, P, WP), torch.int32), (NK, torch.int32), (P, torch.int32))
    a = (p(logits), p(seq), T, B, C, p(lab), p(alt), p(ln), p(grp), NK, WK, p(cls), p(opt), p(pln), P, WP, GAP_COST,
         p(score), p(span), p(kwi), p(kws), p(text), p(kst), p(pst), None, p(ws), nb, _lib.stream_ptr(dev))
    keep = (ws, score, span, kwi, kws, text, kst, pst)

    def run():
        if not lds:
            before = options.set("CTC_LDS", 0)
        _lib.call("ocrk_ctc_keyed_field", *a)
        if not lds:
            options.set("CTC_LDS", before)
        return keep
    return run


def spot_entry():
    nb = _lib.lib().ocrk_ctc_spot_workspace_size(T, B, C, NK, WK)
    ws, score, span, st = buffers((nb, torch.uint8), ((B, NK), torch.float32), ((B, NK, 2), torch.int32),
                                  (NK, torch.int32))
    a = (p(logits), p(seq), T, B, C, p(lab), p(alt), p(ln), NK, WK, p(score), p(span), p(st), None, p(ws), nb,
         _lib.stream_ptr(dev))
    keep = (ws, score, span, st)
    return lambda: (_lib.call("ocrk_ctc_spot", *a), keep)


def field_entry():
    nb = _lib.lib().ocrk_ctc_field_workspace_size(T, B, C, P, WP)
    ws, score, span, text, st = buffers((nb, torch.uint8), ((B, P), torch.float32), ((B, P, 2), torch.int32),
                                        ((B, P, WP), torch.int32), (P, torch.int32))
    a = (p(logits), p(seq), T, B, C, p(cls), p(opt), p(pln), P, WP, p(score), p(span), p(text), p(st), None, p(ws),
         nb, _lib.stream_ptr(dev))
    keep = (ws, score, span, text, st)
    return lambda: (_lib.call("ocrk_ctc_field", *a), keep)


def stats(ts):
    return {"median_us": round(float(np.median(ts)), 1), "min_us": round(float(np.min(ts)), 1),
            "max_us": round(float(np.max(ts)), 1)}


routes = {
    "c_entry": keyed_entry(),
    "c_entry_workspace_route": keyed_entry(lds=0),
    "wrapper": lambda: K.ctc_keyed_field(logits, seq, lab, alt, ln, grp, cls, opt, pln, GAP_COST),
    "ctc_spot_same_keywords": spot_entry(),
    "ctc_field_same_patterns": field_entry(),
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
    "command": f"python tools/bench_keyed.py --runs {args.runs} --warmup {args.warmup}",
    "library": os.path.basename(_lib.LIB_PATH),
    "shape": {"T": T, "B": B, "C": C, "n_key": P, "n_kw": NK, "keywords_per_field": np.bincount(keyed.groups).tolist(),
              "keyword_symbols": [int(keyed.kw_lengths.min()), int(keyed.kw_lengths.max())],
              "positions": [int(keyed.lengths.min()), int(keyed.lengths.max())], "case_insensitive": True,
              "gap_cost": GAP_COST, "dtype": "float32",
              "fields": {n: {"keywords": k, "pattern": pat} for n, (k, pat) in KEYED.items()}},
    "runs": args.runs, "warmup": args.warmup,
}
res.update({name: stats(ts) for name, ts in times.items()})
res["separate_calls_sum_median_us"] = round(res["ctc_spot_same_keywords"]["median_us"] +
                                            res["ctc_field_same_patterns"]["median_us"], 1)
res["c_entry_over_separate_calls"] = round(res["c_entry"]["median_us"] / res["separate_calls_sum_median_us"], 3)
score = K.ctc_keyed_field(logits, seq, lab, alt, ln, grp, cls, opt, pln, GAP_COST)[0]
res["finite_results"] = int(torch.isfinite(score).sum().item())
res["hits_at_ln_half"] = int((score >= np.log(0.5)).sum().item())

print(json.dumps(res, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
