"""Timing of ocrk_ctc_align and of Recognizer(detail=True).

HIP events around the C entry alone on preallocated buffers at the C2 shape
(B = 64, 32x256 crops: T = 125, C = 96; LSTM 512/512 fp32 at the reference
initialisers) with the greedy decode of those logits and with labels of the
C2 benchmark's kind (lengths U{2..19}), at B = 256, on the workspace route
(CTC_LDS = 0) and at a wide bucket (T = 497, B = 16, 30..70 characters);
kernels.ctc_loss beside each for comparison; then the wall time of one
Recognizer call per batch, detail=False against detail=True, for both
decoders, eager and graph-replayed. Prints one JSON object; --out writes it.

    python tools/bench_ctc_align.py [--out profiles/ctc_align_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cnn_lstm_ctc_ocr_amd import ModelConfig, ParamStore, _lib, decode, model, options
from cnn_lstm_ctc_ocr_amd import kernels as K
from cnn_lstm_ctc_ocr_amd.server import Recognizer

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
rng = np.random.default_rng(1234)
B, W = 64, 256
store = ParamStore(ModelConfig(cell="lstm", rnn_sizes=(512, 512), dtype=torch.float32), device=dev, seed=0)
batch = rng.integers(0, 256, (B, 32, W, 1)).astype(np.uint8)
widths = np.full(B, W, np.int32)
with torch.no_grad():
    feats, seq = model.convnet_layers(torch.from_numpy(batch).to(dev), torch.from_numpy(widths).to(dev), model.INFER, store)
    logits = model.rnn_layers(feats, seq, 95, store).float().contiguous()
T = logits.shape[0]
out, out_len, _ = decode.ctc_greedy_decoder_raw(logits, seq)
dl = out_len.cpu().tolist()
res = {"T": T, "B": B, "C": logits.shape[2],
       "decoded_len": {"min": min(dl), "max": max(dl), "mean": round(sum(dl) / len(dl), 2)}}

def ev_time(fn, n=200, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    singles = []
    for _ in range(50):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        singles.append(a.elapsed_time(b) * 1e3)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record(); b.synchronize()
    return {"median_single_us": round(float(np.median(singles)), 2), "back_to_back_us": round(a.elapsed_time(b) * 1e3 / n, 2)}

def raw_align(lg, lab, ln, sq):
    """The C entry alone on preallocated buffers (no allocator, no Python wrapper work beyond the ctypes call)."""
    T_, B_, C_ = lg.shape
    Lm = lab.shape[1]
    nb = _lib.lib().ocrk_ctc_align_workspace_size(T_, B_, Lm)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
    fs = torch.empty(B_, T_, dtype=torch.int32, device=dev); sp = torch.empty(B_, Lm, 2, dtype=torch.int32, device=dev)
    cc = torch.empty(B_, Lm, dtype=torch.float32, device=dev); pl = torch.empty(B_, dtype=torch.float32, device=dev)
    st = torch.empty(B_, dtype=torch.int32, device=dev)
    s = _lib.stream_ptr(dev)
    args = (_lib.ptr(lg), _lib.ptr(lab), _lib.ptr(ln), _lib.ptr(sq), T_, B_, C_, Lm, _lib.ptr(fs), _lib.ptr(sp), _lib.ptr(cc),
            _lib.ptr(pl), _lib.ptr(st), None, _lib.ptr(ws), nb, s)
    return lambda: _lib.call("ocrk_ctc_align", *args)

seq32 = seq.to(torch.int32).contiguous()
# (a) the greedy decode of these logits
wmax = max(int(out_len.max().item()), 1)
lab_g, ln_g = decode._masked_labels(out[:, :wmax], out_len)
res["align_greedy_labels"] = dict(width=wmax, **ev_time(raw_align(logits, lab_g, ln_g, seq32)))
# (b) labels of the C2 benchmark's kind: lengths U{2..19}
lens = rng.integers(2, 20, B)
lab_s = torch.zeros(B, 19, dtype=torch.int32)
for b in range(B):
    lab_s[b, :lens[b]] = torch.from_numpy(rng.integers(0, 94, lens[b]).astype(np.int32))
lab_s, ln_s = lab_s.to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev)
res["align_synth_labels_B64"] = ev_time(raw_align(logits, lab_s, ln_s, seq32))
with options.override(CTC_LDS=0):
    res["align_synth_labels_B64_ws_route"] = ev_time(raw_align(logits, lab_s, ln_s, seq32))
res["loss_nograd_synth_B64_wrapper"] = ev_time(lambda: K.ctc_loss(logits, lab_s, ln_s, seq32, need_grad=False))
res["loss_grad_synth_B64_wrapper"] = ev_time(lambda: K.ctc_loss(logits, lab_s, ln_s, seq32))
res["align_synth_B64_wrapper"] = ev_time(lambda: K.ctc_align(logits, lab_s, ln_s, seq32))
# B = 256, the loss figure's shape
lg4 = logits.repeat(1, 4, 1).contiguous(); lab4 = lab_s.repeat(4, 1).contiguous(); ln4 = ln_s.repeat(4).contiguous(); sq4 = seq32.repeat(4).contiguous()
res["align_synth_labels_B256"] = ev_time(raw_align(lg4, lab4, ln4, sq4))
res["loss_grad_synth_B256_wrapper"] = ev_time(lambda: K.ctc_loss(lg4, lab4, ln4, sq4))

# a wide bucket (W = 1000: T = 497), B = 16, labels of 30..70 characters: the global-memory route
Tw, Bw = 497, 16
lgw = torch.from_numpy(np.maximum(rng.standard_normal((Tw, Bw, 96)) * 3, 0).astype(np.float32)).to(dev)
lensw = rng.integers(30, 71, Bw)
labw = torch.zeros(Bw, 70, dtype=torch.int32)
for b in range(Bw):
    labw[b, :lensw[b]] = torch.from_numpy(rng.integers(0, 94, lensw[b]).astype(np.int32))
labw, lnw = labw.to(dev), torch.from_numpy(lensw.astype(np.int32)).to(dev)
sqw = torch.full((Bw,), Tw, dtype=torch.int32, device=dev)
res["align_wide_T497_B16_len30_70"] = ev_time(raw_align(lgw, labw, lnw, sqw))
res["loss_nograd_wide_T497_B16_wrapper"] = ev_time(lambda: K.ctc_loss(lgw, labw, lnw, sqw, need_grad=False))

def wall(rec, n=30, warm=5):
    for _ in range(warm):
        rec(batch, widths)
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter(); rec(batch, widths); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 3)

for graphs in (False, True):
    for dec in ("greedy", "beam"):
        p = wall(Recognizer(store, decoder=dec, graphs=graphs))
        d = wall(Recognizer(store, decoder=dec, graphs=graphs, detail=True))
        res[f"recognizer_{dec}_graphs{int(graphs)}_ms"] = {"detail_false": p, "detail_true": d, "overhead": round(d - p, 3)}
print(json.dumps(res, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
