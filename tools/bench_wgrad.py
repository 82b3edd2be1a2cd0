"""Conv weight gradients of the train step (B=256, 32x256 crops) in isolation:
time per ocrk_conv3x3_bwd_weight call (whatever route the dispatcher picks:
row-walking, 4-wave TN, ping-pong / one-wave-per-SIMD TN im2col) and TFLOP/s.

    python tools/bench_wgrad.py              # every layer, default routing
    python tools/bench_wgrad.py --ab [reps]  # conv7 / conv8, GEMM_W4=0 (gemm_pptn) against GEMM_W4=2
                                             # (gemm_w4tn), interleaved in this process, `reps` (5)
                                             # repetitions of 20 calls each, incl. the split-K reduce
    python tools/bench_wgrad.py --ab 5 --parent LIB   # and GEMM_W4=2 of another commit's libocrk.so beside them
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from cnn_lstm_ctc_ocr_amd import kernels as K  # noqa: E402

dev = torch.device("cuda")
B = int(os.environ.get("B", "256"))
LAYERS = [("conv2", 30, 254, 32, 32), ("conv3", 15, 127, 32, 64), ("conv4", 15, 127, 64, 64),
          ("conv5", 7, 126, 64, 128), ("conv6", 7, 126, 128, 128), ("conv7", 3, 125, 128, 256),
          ("conv8", 3, 125, 256, 256)]


def timed(f, warm, reps):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def ab_w4(reps):
    """Old and new engine interleaved; a layer is won if the new engine's slowest repetition beats
    the old engine's fastest."""
    from cnn_lstm_ctc_ocr_amd import options
    import second_lib
    var = second_lib.variants(second_lib.parent_from_argv())
    for name, H, W, cin, cout in LAYERS[5:]:
        x = (torch.rand(B, H, W, cin, device=dev) * 2 - 1).bfloat16()
        dy = (torch.rand(B, H, W, cout, device=dev) * 2 - 1).bfloat16()
        dw = torch.zeros(9 * cin, cout, device=dev)
        f = lambda: K.conv3x3_bwd_weight(x, dy, dw, accumulate=False)  # noqa: E731
        t = {n: [] for n, _, _ in var}
        outs = {}
        for _ in range(reps):
            for n, handle, mode in var:
                with second_lib.use(handle), options.override(GEMM_W4=mode):
                    t[n].append(timed(f, 3, 20))
                    outs[n] = dw.clone()
        fl = 2.0 * B * H * W * 9 * cin * cout
        for n, _, mode in var:
            v = t[n]
            print(f"{name} {cin}->{cout} {n:6s} GEMM_W4={mode}: " + " ".join(f"{u:6.1f}" for u in v) +
                  f"  us   fastest {min(v):6.1f} slowest {max(v):6.1f}  {fl / min(v) / 1e6:6.1f} TFLOP/s at fastest")
        same = all(torch.equal(outs["old"], o) for o in outs.values())
        print(f"{name}: bitwise equal {same}; won {max(t['w4']) < min(t['old'])}", flush=True)


def main():
    if "--ab" in sys.argv:
        i = sys.argv.index("--ab")
        return ab_w4(int(sys.argv[i + 1]) if len(sys.argv) > i + 1 and sys.argv[i + 1].isdigit() else 5)
    for name, H, W, cin, cout in LAYERS:
        x = (torch.rand(B, H, W, cin, device=dev) * 2 - 1).bfloat16()
        dy = (torch.rand(B, H, W, cout, device=dev) * 2 - 1).bfloat16()
        dw = torch.zeros(9 * cin, cout, device=dev)
        us = timed(lambda: K.conv3x3_bwd_weight(x, dy, dw, accumulate=False), 1, 10)
        fl = 2.0 * B * H * W * 9 * cin * cout
        print(f"{name} {cin}->{cout}: {us:7.1f} us  {fl / us / 1e6:6.1f} TFLOP/s", flush=True)


if __name__ == "__main__":
    main()
