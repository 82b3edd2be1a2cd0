"""The one-wave-per-SIMD 256 x 256 GEMM engines (csrc/gemm_w4.hip, csrc/gemm_w4tn.hip,
option GEMM_W4): every case runs under GEMM_W4=2 (every covered shape), must have run
on the new engine (the GEMM_W4_LAUNCHES counter moves by one per call) and is checked
(a) bitwise against the same call under GEMM_W4=0 -- the ping-pong engines it stands in
for accumulate the same f32 sequence per output element -- and (b) against the float64
product of the bf16 operands with the bounds of the existing GEMM parity tests
(tests/test_gpu_bf16.py: BF16_OUT = 4e-3 and the per-element bf16 rounding bound for a
bf16 C; 1e-5 for the f32 weight-gradient form)."""
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


def _randn(cuda, seed, *shape, scale=1.0):
    g = torch.Generator(device=cuda).manual_seed(seed)
    return (torch.randn(*shape, device=cuda, generator=g) * scale).bfloat16()


def _check_nt(out, ref):
    assert _rel(out, ref) < BF16_OUT
    err = (out.double() - ref).abs()
    assert bool((err <= 2 ** -8 * ref.abs() + 1e-3 * ref.abs().max()).all())


# K = 64: one K-tile (the prologue is the epilogue); 72: a partial second K-tile; 8: one chunk;
# 4104 x 520: the last row tile has 8 rows, the last column tile 8 columns;
# 8448 x 2048 x 136: 264 items on 256 CUs, so a workgroup walks two items
@pytest.mark.parametrize("M,N,Kd", [(4096, 512, 64), (4096, 512, 72), (4096, 512, 8), (4104, 520, 72),
                                    (4104, 520, 200), (8448, 2048, 136)])
def test_nt_matches_pingpong_bitwise(cuda, ocrk_opts, M, N, Kd):
    a = _randn(cuda, 1 + Kd, M, Kd)
    w = _randn(cuda, 2 + N, N, Kd, scale=Kd ** -0.5)
    g = torch.Generator(device=cuda).manual_seed(3)
    bias = torch.randn(N, device=cuda, generator=g)
    old, new = _both(ocrk_opts, lambda: K.gemm(a, w, trans_b=True, bias=bias, out_dtype=torch.bfloat16))
    assert torch.equal(old, new)
    _check_nt(new, a.double() @ w.double().t() + bias.double())


@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_nt_bias_relu(cuda, ocrk_opts, use_bias, relu):
    M, N, Kd = 4104, 520, 136
    a = _randn(cuda, 11, M, Kd)
    w = _randn(cuda, 12, N, Kd, scale=Kd ** -0.5)
    g = torch.Generator(device=cuda).manual_seed(13)
    bias = torch.randn(N, device=cuda, generator=g) if use_bias else None
    old, new = _both(ocrk_opts, lambda: K.gemm(a, w, trans_b=True, bias=bias, relu=relu, out_dtype=torch.bfloat16))
    assert torch.equal(old, new)
    ref = a.double() @ w.double().t()
    if use_bias:
        ref = ref + bias.double()
    if relu:
        ref = ref.clamp_min(0)
    _check_nt(new, ref)


def test_nt_strided_views(cuda, ocrk_opts):
    """lda > K and ldc > N: operands and output as column views of wider buffers, as model.py
    passes the concatenated layer inputs and gate blocks."""
    M, N, Kd, lda, ldc = 4104, 520, 136, 200, 1056
    abuf = _randn(cuda, 21, M, lda)
    w = _randn(cuda, 22, N, Kd, scale=Kd ** -0.5)
    g = torch.Generator(device=cuda).manual_seed(23)
    bias = torch.randn(N, device=cuda, generator=g)
    a = abuf[:, 32:32 + Kd]

    def run():
        cbuf = torch.full((M, ldc), 7.0, device=cuda, dtype=torch.bfloat16)
        K.gemm(a, w, trans_b=True, bias=bias, out=cbuf[:, 16:16 + N], M=M, N=N, K=Kd, lda=lda, ldb=Kd, ldc=ldc)
        return cbuf

    old, new = _both(ocrk_opts, run)
    assert torch.equal(old, new)
    _check_nt(new[:, 16:16 + N], a.double() @ w.double().t() + bias.double())
    assert bool((new[:, :16] == 7.0).all()) and bool((new[:, 16 + N:] == 7.0).all())   # nothing outside the view


@pytest.mark.parametrize("splits", [1, 3])
def test_tn_ragged_split_k(cuda, ocrk_opts, splits):
    """M = N = 264 (8-wide last tiles), K = 1032: the last K-tile is partial, and with 3 slices
    k_chunk rounds to 352 so the last slice is ragged."""
    M = N = 264
    R = 1032
    x = _randn(cuda, 31, R, M)
    dG = _randn(cuda, 32, R, N)
    old, new = _both(ocrk_opts, lambda: K.gemm(x, dG, trans_a=True, M=M, N=N, K=R, lda=M, ldb=N, splits=splits))
    assert torch.equal(old, new)
    assert _rel(new, x.double().t() @ dG.double()) < F32_TN


@pytest.mark.parametrize("stride_a", [0, 256])
def test_tn_batched_accumulate(cuda, ocrk_opts, stride_a):
    """The batched weight gradients of model.py's recurrent backward at H = 64, In = 256, R = 2056:
    batch = direction, dG column block d * 4H (ldb = 8H, stride_b = 4H), gradient d * (In+H) * 4H,
    accumulated onto a non-zero C. stride_a = 0 is dW_x (both directions read x); the per-direction
    operand form of dW_h (a column block per direction) is run at 256 columns per direction, the
    narrowest the 256-row engines cover (h_prev's own 64 stay on the 128-wide engine)."""
    H, n_in, R = 64, 256, 2056
    G4, sk = 4 * H, (n_in + H) * 4 * H
    M = n_in
    lda = M if stride_a == 0 else 2 * M
    x = _randn(cuda, 41, R, lda)
    dG = _randn(cuda, 42, R, 2 * G4)
    g = torch.Generator(device=cuda).manual_seed(43)
    c0 = torch.randn(2 * sk, device=cuda, generator=g)

    def run():
        c = c0.clone()
        K.gemm(x, dG, trans_a=True, out=c, accumulate=True, M=M, N=G4, K=R, lda=lda, ldb=2 * G4, ldc=G4, batch=2,
               stride_a=stride_a, stride_b=G4, stride_c=sk, splits=2)
        return c

    old, new = _both(ocrk_opts, run)
    assert torch.equal(old, new)
    for d in range(2):
        xa = x[:, d * stride_a:d * stride_a + M].double()
        ref = c0[d * sk:d * sk + M * G4].view(M, G4).double() + xa.t() @ dG[:, d * G4:(d + 1) * G4].double()
        assert _rel(new[d * sk:d * sk + M * G4].view(M, G4), ref) < F32_TN
        tail = slice(d * sk + M * G4, (d + 1) * sk)
        assert torch.equal(new[tail], c0[tail])                                         # rows In .. In+H untouched


def test_repeat_launches_are_identical(cuda, ocrk_opts):
    """20 launches of one NT and one TN case into fresh outputs give the same bits: the counted
    waits of the new barrier structure order every read behind its DMA (a fixed count)."""
    ocrk_opts("GEMM_W4", 2)
    a = _randn(cuda, 51, 8448, 136)
    w = _randn(cuda, 52, 2048, 136, scale=136 ** -0.5)
    x = _randn(cuda, 53, 1032, 264)
    dG = _randn(cuda, 54, 1032, 264)
    n0 = _launches()
    nt = [K.gemm(a, w, trans_b=True, out_dtype=torch.bfloat16) for _ in range(20)]
    tn = [K.gemm(x, dG, trans_a=True, M=264, N=264, K=1032, lda=264, ldb=264, splits=3) for _ in range(20)]
    torch.cuda.synchronize()
    assert _launches() == n0 + 40
    assert all(torch.equal(nt[0], o) for o in nt[1:])
    assert all(torch.equal(tn[0], o) for o in tn[1:])
