"""The conv forms of the one-wave-per-SIMD GEMM engines (option GEMM_W4): the im2col weight
gradient on csrc/gemm_w4tn.hip (A_IM2COL_T, conv7 / conv8: Cin % 64 == 0, Cout >= 256).
As tests/test_gpu_gemm_w4.py: every case runs under GEMM_W4=0 and GEMM_W4=2, the second run
must move GEMM_W4_LAUNCHES by one, its result must be torch.equal to the first (the ping-pong
engine it stands in for accumulates the same f32 sequence per element, split-K partials
included), and it is checked against the float64 product of the bf16 operands with the bound
of the f32 weight-gradient form (1e-5, tests/test_gpu_bf16.py).

The number of K slices is chosen by the library from the pixel count (conv.hip::wgrad_splits:
one slice per 2048 pixels at most), so the single-slice cases run at B = 3 / B = 2 and the
three-slice cases at the smallest batch that yields three slices."""
import pytest
import torch

from cnn_lstm_ctc_ocr_amd import kernels as K
from cnn_lstm_ctc_ocr_amd import options

pytestmark = pytest.mark.gpu

F32_TN = 1e-5            # tests/test_gpu_bf16.py::test_bf16_tn_weight_gradient_recurrent_shape


def _rel(a, ref):
    return float((a.double() - ref).norm() / ref.norm().clamp_min(1e-30))


def _launches():
    return options.get("GEMM_W4_LAUNCHES")


def _both(ocrk_opts, fn):
    """fn() under GEMM_W4=0 and =2; asserts only the second ran on the new engine."""
    ocrk_opts("GEMM_W4", 0)
    n0 = _launches()
    old = fn()
    torch.cuda.synchronize()
    assert _launches() == n0, "GEMM_W4=0 must not reach the new engine"
    ocrk_opts("GEMM_W4", 2)
    new = fn()
    torch.cuda.synchronize()
    assert _launches() == n0 + 1, "GEMM_W4=2: the call fell back to another engine"
    return old, new


def _randn(cuda, seed, *shape):
    g = torch.Generator(device=cuda).manual_seed(seed)
    return torch.randn(*shape, device=cuda, generator=g).bfloat16()


def _wgrad_ref(x, dy):
    """float64 dW[(kh, kw, c)][cout] = sum over pixels of x[b, h+kh-1, w+kw-1, c] * dy[b, h, w, cout]."""
    B, H, W, C = x.shape
    xp = torch.nn.functional.pad(x.double(), (0, 0, 1, 1, 1, 1))
    d = dy.double().reshape(B * H * W, -1)
    taps = [xp[:, kh:kh + H, kw:kw + W, :].reshape(B * H * W, C).t() @ d for kh in range(3) for kw in range(3)]
    return torch.cat(taps, 0)


def _slices(B, H, W, cin, cout):
    """K slices the library uses for this weight gradient (mirrors conv.hip::wgrad_splits, 192 items)."""
    M = B * H * W
    tiles = -(-9 * cin // 256) * -(-cout // 256)
    want = max(1, min(192 // tiles, M // 2048))
    chunk = -(-(-(-M // want)) // 32) * 32
    return -(-M // chunk), M - (-(-M // chunk) - 1) * chunk


# (B, H, W, slices): 3 x 125 -- every pixel row has border taps, K-tiles straddle rows and images;
# 7 x 126 is conv6-8's other geometry; 5 x 9: a K-tile of 64 pixels spans rows and images (the
# pixel stepping wraps both coordinates). The three-slice cases have a ragged last slice whose
# last K-tile is partial (2087 and 2014 pixels).
GEOM = [(3, 3, 125, 1), (2, 7, 126, 1), (40, 5, 9, 1), (17, 3, 125, 3), (7, 7, 126, 3)]


@pytest.mark.parametrize("cin,cout", [(128, 256), (256, 256)])
@pytest.mark.parametrize("B,H,W,slices", GEOM)
def test_wgrad_matches_pingpong_bitwise(cuda, ocrk_opts, B, H, W, slices, cin, cout):
    got, last = _slices(B, H, W, cin, cout)
    assert got == slices and (slices == 1 or last % 64 != 0)
    x = _randn(cuda, 1 + B + cin, B, H, W, cin)
    dy = _randn(cuda, 2 + W + cout, B, H, W, cout)
    g = torch.Generator(device=cuda).manual_seed(3)
    c0 = torch.randn(9 * cin, cout, device=cuda, generator=g)

    def run():
        dw = c0.clone()
        K.conv3x3_bwd_weight(x, dy, dw, accumulate=True)
        return dw

    old, new = _both(ocrk_opts, run)
    assert torch.equal(old, new)
    assert _rel(new, c0.double() + _wgrad_ref(x, dy)) < F32_TN


@pytest.mark.parametrize("B,H,W,slices", [(3, 3, 125, 1), (17, 3, 125, 3)])
def test_wgrad_overwrites_without_accumulate(cuda, ocrk_opts, B, H, W, slices):
    cin, cout = 128, 256
    assert _slices(B, H, W, cin, cout)[0] == slices
    x = _randn(cuda, 11, B, H, W, cin)
    dy = _randn(cuda, 12, B, H, W, cout)

    def run():
        dw = torch.full((9 * cin, cout), 7.0, device=cuda)
        K.conv3x3_bwd_weight(x, dy, dw, accumulate=False)
        return dw

    old, new = _both(ocrk_opts, run)
    assert torch.equal(old, new)
    assert _rel(new, _wgrad_ref(x, dy)) < F32_TN


def test_wgrad_cout_not_a_tile_multiple(cuda, ocrk_opts):
    """Cout = 264: the second column tile has 8 columns."""
    B, H, W, cin, cout = 3, 3, 125, 128, 264
    x = _randn(cuda, 21, B, H, W, cin)
    dy = _randn(cuda, 22, B, H, W, cout)

    def run():
        dw = torch.zeros(9 * cin, cout, device=cuda)
        K.conv3x3_bwd_weight(x, dy, dw, accumulate=False)
        return dw

    old, new = _both(ocrk_opts, run)
    assert torch.equal(old, new)
    assert _rel(new, _wgrad_ref(x, dy)) < F32_TN


BF16_OUT = 4e-3          # tests/test_gpu_bf16.py


def _check_nt(out, ref):
    assert _rel(out, ref) < BF16_OUT
    err = (out.double() - ref).abs()
    assert bool((err <= 2 ** -8 * ref.abs() + 1e-3 * ref.abs().max()).all())


# The 256 x 128 tile of csrc/gemm_w4.hip (taken where 256 x 256 items would cover at most half of
# the CUs): M = 4104 -- the last row tile has 8 rows; N = 264 / 136 -- three / two column tiles, the
# last 8 columns wide; K = 72 -- a partial second K-tile, 64 / 8 -- one K-tile, 4096 -- the layer-1
# data gradient's depth. 8448 x 1024 (132 items of 256 x 256) stays on the 256 x 256 tile.
@pytest.mark.parametrize("M,N,Kd", [(4104, 264, 72), (4104, 136, 72), (4104, 264, 4096), (4104, 136, 4096),
                                    (4104, 136, 64), (4104, 264, 8), (8448, 1024, 64), (8448, 1024, 72),
                                    (8448, 1024, 8)])
@pytest.mark.parametrize("epi", ["plain", "bias", "bias_relu"])
def test_nt_narrow_tile_matches_pingpong_bitwise(cuda, ocrk_opts, M, N, Kd, epi):
    a = _randn(cuda, 41 + Kd, M, Kd)
    w = (_randn(cuda, 42 + N, N, Kd).float() * Kd ** -0.5).bfloat16()
    g = torch.Generator(device=cuda).manual_seed(43)
    bias = torch.randn(N, device=cuda, generator=g) if epi != "plain" else None
    relu = epi == "bias_relu"
    old, new = _both(ocrk_opts, lambda: K.gemm(a, w, trans_b=True, bias=bias, relu=relu, out_dtype=torch.bfloat16))
    assert torch.equal(old, new)
    ref = a.double() @ w.double().t()
    if bias is not None:
        ref = ref + bias.double()
    if relu:
        ref = ref.clamp_min(0)
    _check_nt(new, ref)


def test_nt_narrow_tile_strided_views(cuda, ocrk_opts):
    """lda > K and ldc > N on the 256 x 128 tile: nothing is written outside the output view."""
    M, N, Kd, lda, ldc = 4104, 136, 200, 264, 1056
    abuf = _randn(cuda, 51, M, lda)
    w = (_randn(cuda, 52, N, Kd).float() * Kd ** -0.5).bfloat16()
    g = torch.Generator(device=cuda).manual_seed(53)
    bias = torch.randn(N, device=cuda, generator=g)
    a = abuf[:, 32:32 + Kd]

    def run():
        cbuf = torch.full((M, ldc), 7.0, device=cuda, dtype=torch.bfloat16)
        K.gemm(a, w, trans_b=True, bias=bias, out=cbuf[:, 16:16 + N], M=M, N=N, K=Kd, lda=lda, ldb=Kd, ldc=ldc)
        return cbuf

    old, new = _both(ocrk_opts, run)
    assert torch.equal(old, new)
    _check_nt(new[:, 16:16 + N], a.double() @ w.double().t() + bias.double())
    assert bool((new[:, :16] == 7.0).all()) and bool((new[:, 16 + N:] == 7.0).all())


def test_nt_narrow_tile_repeat_launches_are_identical(cuda, ocrk_opts):
    ocrk_opts("GEMM_W4", 2)
    a = _randn(cuda, 61, 4104, 4096)
    w = (_randn(cuda, 62, 264, 4096).float() / 64).bfloat16()
    n0 = _launches()
    outs = [K.gemm(a, w, trans_b=True, out_dtype=torch.bfloat16) for _ in range(20)]
    torch.cuda.synchronize()
    assert _launches() == n0 + 20
    assert all(torch.equal(outs[0], o) for o in outs[1:])


def test_wgrad_repeat_launches_are_identical(cuda, ocrk_opts):
    """20 launches of one three-slice weight gradient into fresh outputs give the same bits."""
    ocrk_opts("GEMM_W4", 2)
    B, H, W, cin, cout = 17, 3, 125, 256, 256
    x = _randn(cuda, 31, B, H, W, cin)
    dy = _randn(cuda, 32, B, H, W, cout)
    n0 = _launches()
    outs = []
    for _ in range(20):
        dw = torch.zeros(9 * cin, cout, device=cuda)
        K.conv3x3_bwd_weight(x, dy, dw, accumulate=False)
        outs.append(dw)
    torch.cuda.synchronize()
    assert _launches() == n0 + 20
    assert all(torch.equal(outs[0], o) for o in outs[1:])
