"""Timing of ocrk_ctc_field, field reading on the CTC lattice (DESIGN.md
section 3e).

The fp32 serving shape: B = 64 rows of T = 125 frames, C = 96 (ReLU'd Gaussian
logits from a seed), and the eight receipt-style patterns below.

  entry     the C entry alone on preallocated buffers (no allocator, no wrapper
            work beyond the ctypes call), on the LDS route and with CTC_LDS=0 on
            the workspace route.
  wrapper   kernels.ctc_field: the same call with its allocations.
  positions one pattern alone of 4, 8 and 16 digit positions: the three
            unrollings of the scoring kernel.
  language  for scale, the only lattice route there was before: the language of
            [1-9]\\d?\\.\\d\\d (9,900 strings) as keywords through ocrk_ctc_spot
            and a row-wise max on the device, against that one pattern through
            ocrk_ctc_field (both the C entries alone, on the same logits).
  service   Recognizer(store, fields=...) against the same Recognizer without
            fields: wall time per batch of 64 crops of 32 x 256 (a seed-0 fp32
            LSTM 512/512 store), read-back and host work included.

The device routes are timed with device events and each run ends in a
synchronise; the routes alternate in one process; medians of --runs runs (>= 20)
after --warmup warm-up runs. Prints one JSON object; --out writes it.

    python tools/bench_field.py [--out profiles/ctc_field_time.json]"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cnn_lstm_ctc_ocr_amd import _lib, decode, options
from cnn_lstm_ctc_ocr_amd import kernels as K

# What a receipt reader takes out of its lines once a keyword is found.
FIELDS = {
    "amount": r"[1-9]\d{0,3}\.\d{1,2}",
    "dollars": r"\$\d{1,4}\.\d\d",
    "gst": r"\d\.\d\d",
    "percent": r"\d{1,2}%",
    "receipt_no": r"No\.?\d{4,7}",
    "date": r"\d{1,2}/\d{1,2}/\d{2,4}",
    "time": r"\d{1,2}:\d\d",
    "quantity": r"\d{1,3} ?x",
}
ONE = r"[1-9]\d?\.\d\d"

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--no-service", action="store_true", help="skip the Recognizer timing (kernel variants)")
args = ap.parse_args()
if args.runs < 20:
    ap.error("--runs must be at least 20")
if not torch.cuda.is_available():
    sys.exit("bench_field.py needs the GPU: there is no CPU route to time")
dev = torch.device("cuda:0")
rng = np.random.default_rng(1234)
T, B, C = 125, 64, 96
logits = torch.from_numpy(np.maximum(rng.standard_normal((T, B, C)) * 3, 0).astype(np.float32)).to(dev)
seq = torch.full((B,), T, dtype=torch.int32, device=dev)
fset = decode.FieldSet(FIELDS)
assert len(fset) == 8


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def field_entry(fs, lds=1):
    cls, opt, ln = fs.tensors(dev)
    P, W = opt.shape
    nb = _lib.lib().ocrk_ctc_field_workspace_size(T, B, C, P, W)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    score = torch.empty(B, P, dtype=torch.float32, device=dev)
    span = torch.empty(B, P, 2, dtype=torch.int32, device=dev)
    text = torch.empty(B, P, W, dtype=torch.int32, device=dev)
    st = torch.empty(P, dtype=torch.int32, device=dev)
    a = (_lib.ptr(logits), _lib.ptr(seq), T, B, C, _lib.ptr(cls), _lib.ptr(opt), _lib.ptr(ln), P, W, _lib.ptr(score),
         _lib.ptr(span), _lib.ptr(text), _lib.ptr(st), None, _lib.ptr(ws), nb, _lib.stream_ptr(dev))
    keep = (cls, opt, ln, ws, score, span, text, st)

    def run():
        if not lds:
            before = options.set("CTC_LDS", 0)
        _lib.call("ocrk_ctc_field", *a)
        if not lds:
            options.set("CTC_LDS", before)
        return keep
    return run


def language_entry(fs):
    """Every string of the single pattern as a keyword through ocrk_ctc_spot, then the row-wise max."""
    (cls, opt), = fs.compiled
    per = [[(l,) for l in c] + ([()] if o else []) for c, o in zip(cls, opt)]
    strings = sorted({tuple(itertools.chain.from_iterable(pick)) for pick in itertools.product(*per)})
    NK, W = len(strings), max(map(len, strings))
    lab = np.zeros((NK, W), np.int32)
    for i, s in enumerate(strings):
        lab[i, :len(s)] = s
    lab = torch.from_numpy(lab).to(dev)
    ln = torch.tensor([len(s) for s in strings], dtype=torch.int32, device=dev)
    nb = _lib.lib().ocrk_ctc_spot_workspace_size(T, B, C, NK, W)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    score = torch.empty(B, NK, dtype=torch.float32, device=dev)
    span = torch.empty(B, NK, 2, dtype=torch.int32, device=dev)
    st = torch.empty(NK, dtype=torch.int32, device=dev)
    a = (_lib.ptr(logits), _lib.ptr(seq), T, B, C, _lib.ptr(lab), None, _lib.ptr(ln), NK, W, _lib.ptr(score),
         _lib.ptr(span), _lib.ptr(st), None, _lib.ptr(ws), nb, _lib.stream_ptr(dev))
    keep = (lab, ln, ws, span, st)
    return NK, score, lambda: (_lib.call("ocrk_ctc_spot", *a), score.max(dim=1), keep)


def stats(ts):
    return {"median_us": round(float(np.median(ts)), 1), "min_us": round(float(np.min(ts)), 1),
            "max_us": round(float(np.max(ts)), 1)}


one = decode.FieldSet({"amount": ONE})
n_strings, spot_scores, language = language_entry(one)
cls, opt, ln = fset.tensors(dev)
routes = {
    "c_entry": field_entry(fset),
    "c_entry_workspace_route": field_entry(fset, lds=0),
    "wrapper": lambda: K.ctc_field(logits, seq, cls, opt, ln),
    "c_entry_one_pattern_4_positions": field_entry(decode.FieldSet({"d": r"\d{4}"})),
    "c_entry_one_pattern_8_positions": field_entry(decode.FieldSet({"d": r"\d{8}"})),
    "c_entry_one_pattern_16_positions": field_entry(decode.FieldSet({"d": r"\d{16}"})),
    "c_entry_one_pattern": field_entry(one),
    "language_through_ctc_spot_and_max": language,
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
    "command": f"python tools/bench_field.py --runs {args.runs} --warmup {args.warmup}",
    "library": os.path.basename(_lib.LIB_PATH),
    "shape": {"T": T, "B": B, "C": C, "n_pat": len(fset), "patterns": FIELDS,
              "positions": [int(fset.lengths.min()), int(fset.lengths.max())], "dtype": "float32"},
    "one_pattern": {"pattern": ONE, "strings": n_strings},
    "runs": args.runs, "warmup": args.warmup,
}
res.update({name: stats(ts) for name, ts in times.items()})
score, _span, _text, _st = K.ctc_field(logits, seq, *one.tensors(dev))
res["one_pattern"]["scores_equal_the_language_max_bytewise"] = bool(
    torch.equal(score[:, 0].view(torch.int32), spot_scores.max(dim=1).values.view(torch.int32)))
score, _span, _text, _st = K.ctc_field(logits, seq, cls, opt, ln)
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
        # an untrained store's logits are nearly flat, so at the default threshold most patterns "hit" and the
        # host builds a FieldHit per crop and pattern; threshold 0 (exact hits only) shows the cost without them
        recs = {"plain": Recognizer(store, graphs=graphs),
                "fields": Recognizer(store, graphs=graphs, fields=fset),
                "fields_thr0": Recognizer(store, graphs=graphs, fields=fset, field_threshold=0.0)}
        for rec in recs.values():
            for _ in range(args.warmup):
                rec(batch, widths)
        ts = {name: [] for name in recs}
        for _ in range(args.runs):
            for name, rec in recs.items():
                ts[name].append(wall(rec))
        med = {name: float(np.median(v)) for name, v in ts.items()}
        hits = {name: sum(len(r.fields) for r in recs[name](batch, widths)) for name in ("fields", "fields_thr0")}
        service["graphs" if graphs else "eager"] = {
            "plain_ms": round(med["plain"], 3),
            "with_fields_ms": round(med["fields"], 3), "overhead_ms": round(med["fields"] - med["plain"], 3),
            "hits_per_batch": hits["fields"],
            "with_fields_threshold_0_ms": round(med["fields_thr0"], 3),
            "overhead_threshold_0_ms": round(med["fields_thr0"] - med["plain"], 3),
            "hits_per_batch_threshold_0": hits["fields_thr0"]}
    res["recognizer_wall_per_64_crop_batch"] = dict(service, crop="32 x 256", store="fp32 LSTM 512/512, seed 0")

print(json.dumps(res, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
