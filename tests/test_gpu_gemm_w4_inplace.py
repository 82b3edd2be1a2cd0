"""The item boundary of the one-wave-per-SIMD GEMM engines (csrc/gemm_w4.hip, csrc/gemm_w4tn.hip,
option GEMM_W4): an item's accumulators are no longer zeroed by a pass of their own but defined by
the MFMAs of the item's first k-block, which take the literal 0 as C (the peeled first K-tile).
The cases put that first k-block everywhere it can sit: as the only k-block (K = 32), in the only
K-tile, in front of a partial and of several further K-tiles, behind another item's epilogue in
the same registers (persistent workgroups walking three items), and over an output that held NaN.
As tests/test_gpu_gemm_w4.py: every case runs under GEMM_W4=0 and GEMM_W4=2, the second run must
move GEMM_W4_LAUNCHES by one per call, its result must be torch.equal to the first, and it is
checked against the float64 product of the bf16 operands with that file's bounds."""
import pytest
import torch

from cnn_lstm_ctc_ocr_amd import kernels as K
from cnn_lstm_ctc_ocr_amd import options

pytestmark = pytest.mark.gpu

BF16_OUT = 4e-3          # tests/test_gpu_bf16.py
F32_TN = 1e-5            # tests/test_gpu_bf16.py::test_bf16_tn_weight_gradient_recurrent_shape


def _rel(a, ref):
    return float((a.double() - ref).norm() / ref.norm().clamp_min(1e-30))


def _launches():
    return options.get("GEMM_W4_LAUNCHES")


def _both(ocrk_opts, fn, calls=1):
    """fn() under GEMM_W4=0 and =2; asserts only the second ran on the new engine."""
    ocrk_opts("GEMM_W4", 0)
    n0 = _launches()
    old = fn()
    torch.cuda.synchronize()
    assert _launches() == n0, "GEMM_W4=0 must not reach the new engine"
    ocrk_opts("GEMM_W4", 2)
    new = fn()
    torch.cuda.synchronize()
    assert _launches() == n0 + calls, "GEMM_W4=2: the call fell back to another engine"
    return old, new


def _randn(cuda, seed, *shape, scale=1.0):
    g = torch.Generator(device=cuda).manual_seed(seed)
    return (torch.randn(*shape, device=cuda, generator=g) * scale).bfloat16()


def _check_nt(out, ref):
    assert _rel(out, ref) < BF16_OUT
    err = (out.double() - ref).abs()
    assert bool((err <= 2 ** -8 * ref.abs() + 1e-3 * ref.abs().max()).all())


def _nt_case(cuda, ocrk_opts, M, N, Kd, relu):
    a = _randn(cuda, 1 + Kd, M, Kd)
    w = _randn(cuda, 2 + N, N, Kd, scale=Kd ** -0.5)
    g = torch.Generator(device=cuda).manual_seed(3)
    bias = torch.randn(N, device=cuda, generator=g)
    old, new = _both(ocrk_opts, lambda: K.gemm(a, w, trans_b=True, bias=bias, relu=relu, out_dtype=torch.bfloat16))
    assert torch.equal(old, new)
    ref = a.double() @ w.double().t() + bias.double()
    _check_nt(new, ref.clamp_min(0) if relu else ref)


# The 256 x 128 tile (N = 128 / 136: its items cover less than half of the CUs). K = 32: the first
# k-block is the only one (the K-tile's second k-block is zero fill); 64: one K-tile; 72: a partial
# second K-tile; 200: several. 4104 x 136: the last row tile has 8 rows, the last column tile 8 columns.
@pytest.mark.parametrize("M,N,Kd", [(4096, 128, 32), (4096, 128, 64), (4096, 128, 72), (4096, 128, 200),
                                    (4104, 136, 72)])
def test_nt_narrow_tile_first_k_block(cuda, ocrk_opts, M, N, Kd):
    _nt_case(cuda, ocrk_opts, M, N, Kd, relu=False)


# The 256 x 256 tile, 520 items on 256 workgroups: three items per workgroup (all in flight at once
# when K = 64), so each item's first k-block follows another item's epilogue in the same registers.
@pytest.mark.parametrize("Kd,relu", [(64, False), (192, True)])
def test_nt_three_items_per_workgroup(cuda, ocrk_opts, Kd, relu):
    _nt_case(cuda, ocrk_opts, 133120, 256, Kd, relu)


def test_nt_twice_over_nan_output(cuda, ocrk_opts):
    """Two launches into an output pre-filled with NaN: nothing of a previous item or launch (and
    nothing of the output's old contents) survives in an accumulator."""
    M, N, Kd = 4096, 512, 64
    a = _randn(cuda, 71, M, Kd)
    w = _randn(cuda, 72, N, Kd, scale=Kd ** -0.5)
    g = torch.Generator(device=cuda).manual_seed(73)
    bias = torch.randn(N, device=cuda, generator=g)

    def run():
        outs = []
        c = torch.full((M, N), float("nan"), device=cuda, dtype=torch.bfloat16)
        for _ in range(2):
            K.gemm(a, w, trans_b=True, bias=bias, out=c)
            outs.append(c.clone())
        return outs

    old, new = _both(ocrk_opts, run, calls=2)
    assert torch.equal(new[0], new[1])
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])
    _check_nt(new[1], a.double() @ w.double().t() + bias.double())


def _wgrad_ref(x, dy):
    """float64 dW[(kh, kw, c)][cout] = sum over pixels of x[b, h+kh-1, w+kw-1, c] * dy[b, h, w, cout]."""
    B, H, W, C = x.shape
    xp = torch.nn.functional.pad(x.double(), (0, 0, 1, 1, 1, 1))
    d = dy.double().reshape(B * H * W, -1)
    taps = [xp[:, kh:kh + H, kw:kw + W, :].reshape(B * H * W, C).t() @ d for kh in range(3) for kw in range(3)]
    return torch.cat(taps, 0)


# The im2col instance through the public conv weight-gradient entry: the three-slice geometries of
# tests/test_gpu_gemm_w4_conv.py (B = 17 at 3 x 125, B = 7 at 7 x 126; a ragged last slice whose
# last K-tile is partial) on conv7's and conv8's channel counts.
@pytest.mark.parametrize("cin,cout", [(128, 256), (256, 256)])
@pytest.mark.parametrize("B,H,W", [(17, 3, 125), (7, 7, 126)])
def test_wgrad_im2col_three_slices(cuda, ocrk_opts, B, H, W, cin, cout):
    x = _randn(cuda, 1 + B + cin, B, H, W, cin)
    dy = _randn(cuda, 2 + W + cout, B, H, W, cout)

    def run():
        dw = torch.full((9 * cin, cout), float("nan"), device=cuda)
        K.conv3x3_bwd_weight(x, dy, dw, accumulate=False)
        return dw

    old, new = _both(ocrk_opts, run)
    assert torch.equal(old, new)
    assert _rel(new, _wgrad_ref(x, dy)) < F32_TN
