"""Conv weight gradients of the train step (B=256, 32x256 crops) in isolation:
time per ocrk_conv3x3_bwd_weight call (whatever route the dispatcher picks:
row-walking, 4-wave TN, ping-pong / one-wave-per-SIMD TN im2col) and TFLOP/s.

    python tools/bench_wgrad.py              # every layer, default routing
    python tools/bench_wgrad.py --ab [reps]  # conv7 / conv8, GEMM_W4=0 (gemm_pptn) against GEMM_W4=2
                                             # (gemm_w4tn), interleaved in this process, `reps` (5)
                                             # repetitions of 20 calls each, incl. the split-K reduce
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
    for name, H, W, cin, cout in LAYERS[5:]:
        x = (torch.rand(B, H, W, cin, device=dev) * 2 - 1).bfloat16()
        dy = (torch.rand(B, H, W, cout, device=dev) * 2 - 1).bfloat16()
        dw = torch.zeros(9 * cin, cout, device=dev)
        f = lambda: K.conv3x3_bwd_weight(x, dy, dw, accumulate=False)  # noqa: E731
        t = {0: [], 2: []}
        outs = {}
        for _ in range(reps):
            for mode in (0, 2):
                with options.override(GEMM_W4=mode):
                    t[mode].append(timed(f, 3, 20))
                    outs[mode] = dw.clone()
        fl = 2.0 * B * H * W * 9 * cin * cout
        for mode in (0, 2):
            v = t[mode]
            print(f"{name} {cin}->{cout} GEMM_W4={mode}: " + " ".join(f"{u:6.1f}" for u in v) +
                  f"  us   fastest {min(v):6.1f} slowest {max(v):6.1f}  {fl / min(v) / 1e6:6.1f} TFLOP/s at fastest")
        print(f"{name}: bitwise equal {bool(torch.equal(outs[0], outs[2]))}; won {max(t[2]) < min(t[0])}", flush=True)


def main():
    if "--ab" in sys.argv:
        i = sys.argv.index("--ab")
        return ab_w4(int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else 5)
    for name, H, W, cin, cout in LAYERS:
        x = (torch.rand(B, H, W, cin, device=dev) * 2 - 1).bfloat16()
        dy = (torch.rand(B, H, W, cout, device=dev) * 2 - 1).bfloat16()
        dw = torch.zeros(9 * cin, cout, device=dev)
        us = timed(lambda: K.conv3x3_bwd_weight(x, dy, dw, accumulate=False), 1, 10)
        fl = 2.0 * B * H * W * 9 * cin * cout
        print(f"{name} {cin}->{cout}: {us:7.1f} us  {fl / us / 1e6:6.1f} TFLOP/s", flush=True)


if __name__ == "__main__":
    main()
