"""Weight-gradient (TN) GEMMs of the train step: time per call and TFLOP/s on
the engine the dispatcher picks (OCRK_GEMM_PPTN=0: the 4-wave engine).

    python tools/bench_tn.py --ab [reps]   # GEMM_W4=0 against GEMM_W4=2 (the one-wave-per-SIMD engine,
                                           # csrc/gemm_w4tn.hip), interleaved, `reps` (5) repetitions each
    python tools/bench_tn.py --ab 5 --parent LIB   # and GEMM_W4=2 of another commit's libocrk.so beside them
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from cnn_lstm_ctc_ocr_amd import kernels as K  # noqa: E402
from cnn_lstm_ctc_ocr_amd.model import _splits  # noqa: E402

R = 32000
dev = torch.device("cuda")
SHAPES = [(1024, 2048, 4096, "L2 dW_x (per dir)"), (512, 2048, 4096, "dW_h (per dir)"),
          (256, 2048, 4096, "L1 dW_x (per dir)"), (1024, 96, 96, "logits dW")]


def _timed(f, n=10):
    f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def ab_w4(reps):
    """Old and new engine interleaved (split-K reduce included in both); a shape is won if the new
    engine's slowest repetition beats the old engine's fastest."""
    from cnn_lstm_ctc_ocr_amd import options
    import second_lib
    var = second_lib.variants(second_lib.parent_from_argv())
    print(f"{'shape':20s} {'engine':6s} {'min us':>9s} {'max us':>9s} {'TFLOP/s (min)':>14s}   repetitions (us)")
    for n_in, N, ldb, tag in SHAPES:
        x = (torch.rand(R, n_in, device=dev) * 2 - 1).bfloat16()
        dG = (torch.rand(R, ldb, device=dev) * 2 - 1).bfloat16()
        sp = _splits(n_in, N, R)
        t = {name: [] for name, _, _ in var}
        outs = {}
        for _ in range(reps):
            for name, handle, mode in var:
                with second_lib.use(handle), options.override(GEMM_W4=mode):
                    gk = torch.zeros(n_in, N, device=dev)
                    f = lambda: K.gemm(x, dG, trans_a=True, out=gk, accumulate=True, M=n_in, N=N, K=R,  # noqa: E731
                                       lda=n_in, ldb=ldb, ldc=N, splits=sp)
                    f()
                    outs[name] = gk.clone()
                    t[name].append(_timed(f) * 1e3)
        same = all(torch.equal(outs["old"], o) for o in outs.values())
        for name, _, _ in var:
            v = t[name]
            print(f"{tag:20s} {name:6s} {min(v):9.1f} {max(v):9.1f} {2.0 * n_in * N * R / min(v) / 1e6:14.1f}   "
                  + " ".join(f"{q:.1f}" for q in v))
        print(f"{tag:20s} splits {sp}: {'won' if max(t['w4']) < min(t['old']) else 'not won'}; bit-identical: {same}",
              flush=True)


if "--ab" in sys.argv:
    _i = sys.argv.index("--ab")
    ab_w4(int(sys.argv[_i + 1]) if len(sys.argv) > _i + 1 and sys.argv[_i + 1].isdigit() else 5)
    sys.exit(0)

tot = 0.0
for n_in, N, ldb, tag in SHAPES:
    x = (torch.rand(R, n_in, device=dev) * 2 - 1).bfloat16()
    dG = (torch.rand(R, ldb, device=dev) * 2 - 1).bfloat16()
    gk = torch.zeros(n_in, N, device=dev)
    sp = _splits(n_in, N, R)
    f = lambda: K.gemm(x, dG, trans_a=True, out=gk, accumulate=True, M=n_in, N=N, K=R, lda=n_in, ldb=ldb,  # noqa: E731
                       ldc=N, splits=sp)
    f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        f()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / 10
    tot += ms * (4 if "dir" in tag else 1)
    print(f"{tag:20s} splits {sp:3d} {ms * 1e3:8.1f} us {2.0 * n_in * N * R / ms / 1e9:8.1f} TFLOP/s", flush=True)
print(f"per-step total (x4 for the per-direction GEMMs of both layers' dW_x / dW_h): {tot:.3f} ms")
