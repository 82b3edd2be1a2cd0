"""Ping-pong GEMM engine (csrc/gemm_pp.hip) on the train step's shapes:
time per launch, TFLOP/s and the error against a float32 torch reference
computed from the same bf16 operands (diagnostic; the parity tests are in
tests/). The convolution rows time the routed conv engines beside them: the
ping-pong engine has no convolution form.

    python tools/bench_pp.py                 # default routing (engine on)
    OCRK_GEMM_PP=0 python tools/bench_pp.py  # the plain GEMMs on the NT engine
    python tools/bench_pp.py --ab [reps]     # the plain GEMMs, GEMM_W4=0 against GEMM_W4=2 (the
                                             # one-wave-per-SIMD engine, csrc/gemm_w4.hip): interleaved in
                                             # this process, `reps` (5) repetitions of 20 launches each
    python tools/bench_pp.py --ab 5 --parent LIB   # and a third engine beside them: GEMM_W4=2 of another
                                             # commit's libocrk.so (tools/second_lib.py)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from cnn_lstm_ctc_ocr_amd import kernels as K  # noqa: E402

B = 256
CONV = [(30, 254, 32, 32), (15, 127, 32, 64), (15, 127, 64, 64), (7, 126, 64, 128), (7, 126, 128, 128),
        (3, 125, 128, 256), (3, 125, 256, 256)]


def timed(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def rel(x, ref):
    return float((x.float() - ref).norm() / ref.norm().clamp_min(1e-30))


PLAIN = [(32000, 4096, 256, "proj L1"), (32000, 4096, 1024, "proj L2"), (32000, 1024, 4096, "dx L2"),
         (32000, 256, 4096, "dx L1"), (32000, 1024, 96, "logits dx")]


def ab_w4(reps):
    """Old and new engine interleaved; a shape is won if the new engine's slowest repetition beats
    the old engine's fastest."""
    from cnn_lstm_ctc_ocr_amd import options
    import second_lib
    var = second_lib.variants(second_lib.parent_from_argv())
    torch.manual_seed(0)
    dev = torch.device("cuda")
    bf = torch.bfloat16
    print(f"{'shape':12s} {'engine':8s} {'min us':>9s} {'max us':>9s} {'TFLOP/s (min)':>14s}   repetitions (us)")
    for (M, N, Kd, tag) in PLAIN:
        a = (torch.rand(M, Kd, device=dev) * 2 - 1).to(bf)
        w = ((torch.rand(N, Kd, device=dev) * 2 - 1) * 0.05).to(bf)
        bias = torch.randn(N, device=dev) if "proj" in tag else None
        f = lambda: K.gemm(a, w, trans_b=True, bias=bias, out_dtype=bf)  # noqa: E731
        t = {name: [] for name, _, _ in var}
        outs = {}
        for _ in range(reps):
            for name, handle, mode in var:
                with second_lib.use(handle), options.override(GEMM_W4=mode):
                    outs[name] = f()
                    t[name].append(timed(f) * 1e3)
        same = all(torch.equal(outs["old"], o) for o in outs.values())
        for name, _, _ in var:
            v = t[name]
            print(f"{tag:12s} {name:8s} {min(v):9.1f} {max(v):9.1f} {2.0 * M * N * Kd / min(v) / 1e6:14.1f}   "
                  + " ".join(f"{x:.1f}" for x in v))
        print(f"{tag:12s} {'won' if max(t['w4']) < min(t['old']) else 'not won'}; bit-identical: {same}", flush=True)


def main():
    if "--ab" in sys.argv:
        i = sys.argv.index("--ab")
        return ab_w4(int(sys.argv[i + 1]) if len(sys.argv) > i + 1 and sys.argv[i + 1].isdigit() else 5)
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    torch.manual_seed(0)
    dev = torch.device("cuda")
    bf = torch.bfloat16
    rows = []
    for (M, N, Kd, tag) in [(32000, 4096, 256, "proj L1"), (32000, 4096, 1024, "proj L2"),
                            (32000, 1024, 4096, "dx L2"), (32000, 256, 4096, "dx L1"),
                            (32000, 1024, 96, "logits dx")]:
        if only and only not in tag:
            continue
        a = (torch.rand(M, Kd, device=dev) * 2 - 1).to(bf)
        w = ((torch.rand(N, Kd, device=dev) * 2 - 1) * 0.05).to(bf)
        bias = torch.randn(N, device=dev)
        out = K.gemm(a, w, trans_b=True, bias=bias, out_dtype=bf)
        ref = a.float() @ w.float().t() + bias
        ms = timed(lambda: K.gemm(a, w, trans_b=True, bias=bias, out_dtype=bf))
        rows.append((tag, ms, 2.0 * M * N * Kd, rel(out, ref)))
    for (H, W, Ci, Co) in ([] if only else CONV):
        x = (torch.rand(B, H, W, Ci, device=dev) * 2 - 1).to(bf)
        w = ((torch.rand(Co, 3, 3, Ci, device=dev) * 2 - 1) * 0.05).to(bf)          # [Cout][kh][kw][Cin]
        w_nk = w.reshape(Co, 9 * Ci).contiguous()
        bias = torch.randn(Co, device=dev)
        fl = 2.0 * B * H * W * 9 * Ci * Co
        y = K.conv3x3_fwd(x, w_nk, bias, relu=True)
        ref = F.relu(F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), bias, padding=1))
        err = rel(y.permute(0, 3, 1, 2), ref)
        ms = timed(lambda: K.conv3x3_fwd(x, w_nk, bias, relu=True))
        rows.append((f"conv fwd {Ci}->{Co} {H}x{W}", ms, fl, err))
        dy = (torch.rand(B, H, W, Co, device=dev) * 2 - 1).to(bf)
        w_bwd = w.permute(3, 1, 2, 0).reshape(Ci, 9 * Co).contiguous()     # [Cin][kh][kw][Cout] (flip: address mode)
        dx = K.conv3x3_bwd_data(dy, w_bwd)
        ref = F.conv_transpose2d(dy.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), padding=1)
        err = rel(dx.permute(0, 3, 1, 2), ref)
        ms = timed(lambda: K.conv3x3_bwd_data(dy, w_bwd))
        rows.append((f"conv bwd-data {Co}->{Ci} {H}x{W}", ms, fl, err))
    tot = 0.0
    for tag, ms, fl, err in rows:
        tot += ms
        print(f"{tag:32s} {ms * 1e3:9.1f} us  {fl / ms / 1e9:8.1f} TFLOP/s  rel.err {err:.2e}")
    print(f"total {tot:.3f} ms  (OCRK_GEMM_PP={os.environ.get('OCRK_GEMM_PP', '1')}, "
          "no vendor route)", flush=True)


if __name__ == "__main__":
    main()
