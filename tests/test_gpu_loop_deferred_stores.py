"""Where the 16-row persistent LSTM loops (csrc/lstm_persistent.hip,
lstm_fwd_r16_kernel / lstm_bwd_r16_kernel) put their saved tensors: every step's
output, h_prev, c_prev, gate activations and dG at that step's own time row.
Written for the forms that store step s's tensors inside step s + 1 and flush
the last step's after the loop (measured slower, not kept);
they pin the kernels as they are and any later change of the store placement.
A moved store goes wrong at the first step, at the last step (a flush after the
loop) or by a one-step address slip, so the shapes are the smallest that have
those places: T = 1, 2, 3, 7 with ragged lengths (full, 1, T - 1, 2), H = 512,
the smallest batch the persistent loops admit, B = 64 (XCD-grouped workgroup
map) and B = 96 (linear map). The references are the 32-row forward
(LSTM_FWD_R16=0) and the gather BPTT (LSTM_BWD_R16=0), compared per time step;
the exact structural checks catch a slip bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, N_IN = 512, 32
TS = (1, 2, 3, 7)
_CASES = {}


def _batches():
    from cnn_lstm_ctc_ocr_amd import kernels as K
    K._PERSISTENT.clear()
    first = 32 if K.lstm_persistent_ok(32, H, torch.bfloat16) else 64
    return [first, 64, 96]


def _case(cuda, ocrk_opts, T, B):
    """Inputs and the outputs of both kernel forms for (T, B): computed once, shared, never written."""
    if (T, B) in _CASES:
        return _CASES[(T, B)]
    from cnn_lstm_ctc_ocr_amd import kernels as K
    rng = np.random.default_rng(1000 * T + B)
    bf = lambda a: torch.from_numpy(a.astype(np.float32)).to(cuda).bfloat16()   # noqa: E731
    x = bf(rng.standard_normal((T * B, N_IN)))
    ks = [rng.standard_normal((N_IN + H, 4 * H)) * 0.1 for _ in range(2)]
    bias = torch.from_numpy((rng.standard_normal(8 * H) * 0.2).astype(np.float32)).to(cuda)
    seq = rng.integers(1, T + 1, B).astype(np.int32)
    seq[:4] = [T, 1, max(1, T - 1), min(2, T)]
    wxT = bf(np.ascontiguousarray(np.concatenate([k[:N_IN].T for k in ks], 0)))
    whT = bf(np.ascontiguousarray(np.stack([k[N_IN:].T for k in ks])))
    wh = bf(np.ascontiguousarray(np.stack([k[N_IN:] for k in ks])))
    gx = K.gemm(x, wxT, trans_b=True, bias=bias, out_dtype=torch.bfloat16)
    seq_d = torch.from_numpy(seq).to(cuda)
    dout = bf(rng.standard_normal((T, B, 2 * H)))
    K._PERSISTENT.clear()
    assert K.lstm_persistent_ok(B, H, torch.bfloat16)
    K.lstm_error_word(cuda).zero_()
    c = {"seq": torch.from_numpy(seq.astype(np.int64)).to(cuda), "gx": gx, "whT": whT, "wh": wh, "seq_d": seq_d,
         "dout": dout}
    for r16 in (1, 0):
        ocrk_opts("LSTM_FWD_R16", r16)
        c["fwd", r16] = K.lstm_fwd(gx, whT, seq_d, T, B, H, torch.bfloat16)
    ocrk_opts.reset("LSTM_FWD_R16")
    _, _, cprev, acts = c["fwd", 1]
    for r16 in (1, 0):
        ocrk_opts("LSTM_BWD_R16", r16)
        db = torch.zeros(2 * 4 * H, device=cuda)
        c["bwd", r16] = (K.lstm_bwd(wh, seq_d, dout, cprev, acts, T, B, H, dbias=db), db)
    ocrk_opts.reset("LSTM_BWD_R16")
    torch.cuda.synchronize()
    assert K.lstm_error_word(cuda).item() == 0
    _CASES[(T, B)] = c
    return c


def _cases():
    # the batch list needs the GPU: the parametrisation carries an index into it
    # (where the smallest admitted batch is 64, index 0 repeats the shared B = 64 case)
    return [(T, bi) for T in TS for bi in range(3)]


def _tb(T, bi):
    return T, _batches()[bi]


@pytest.mark.parametrize("T,bi", _cases())
def test_forward_r16_matches_32row_every_step(cuda, ocrk_opts, T, bi):
    T, B = _tb(T, bi)
    c = _case(cuda, ocrk_opts, T, B)
    for name, a, b in zip(("out", "hprev", "cprev", "acts"), c["fwd", 1], c["fwd", 0]):
        a, b = a.float(), b.float()
        tol = 1e-2 * max(1.0, b.abs().max().item())
        err = (a - b).abs().reshape(T, -1).max(dim=1).values.cpu().numpy()
        print(f"T={T} B={B} {name}: max |r16 - 32row| per t {np.array2string(err, precision=4)} (tol {tol:.3g})")
        assert np.all(err < tol), (name, err, tol)


@pytest.mark.parametrize("T,bi", _cases())
def test_forward_r16_saved_tensors_sit_at_their_own_step(cuda, ocrk_opts, T, bi):
    T, B = _tb(T, bi)
    c = _case(cuda, ocrk_opts, T, B)
    out, hprev, cprev, acts = c["fwd", 1]
    out = out.view(T, B, 2, H)
    ln = c["seq"][None, :]                                   # [1, B]
    tt = torch.arange(T, device=cuda)[:, None]               # [T, 1]
    invalid = tt >= ln                                       # [T, B]
    for name, a in (("out", out), ("hprev", hprev), ("cprev", cprev), ("acts", acts)):
        assert torch.all(a[invalid] == 0), f"{name} not exactly 0 past the length"
    assert torch.all(out[~invalid].float().abs().amax(dim=-1) > 0)      # every valid step was written
    assert torch.all(hprev[0, :, 0] == 0)
    # forward direction: hprev[t] is out[t - 1] for 1 <= t < len
    m = (~invalid)[1:]
    assert torch.equal(hprev[1:, :, 0][m], out[:-1, :, 0][m])
    # reverse direction: hprev[t] is out[t + 1] for t + 1 < len, and 0 at t = len - 1
    m = (tt + 1 < ln)[:-1]
    assert torch.equal(hprev[:-1, :, 1][m], out[1:, :, 1][m])
    rows = torch.arange(B, device=cuda)
    assert torch.all(hprev[c["seq"] - 1, rows, 1] == 0)


@pytest.mark.parametrize("T,bi", _cases())
def test_bptt_r16_matches_gather_every_step(cuda, ocrk_opts, T, bi):
    T, B = _tb(T, bi)
    c = _case(cuda, ocrk_opts, T, B)
    (d16, db16), (d32, _) = c["bwd", 1], c["bwd", 0]
    scale = d32.float().abs().max().item()
    tol = 2e-2 * max(scale, 1e-6)
    diff = (d16.float() - d32.float()).abs()
    err = diff.reshape(T, -1).max(dim=1).values.cpu().numpy()
    print(f"T={T} B={B} dG: max |r16 - gather| per t {np.array2string(err, precision=4)} (tol {tol:.3g})")
    assert np.all(err < tol), (err, tol)
    ln = c["seq"][None, :]
    invalid = torch.arange(T, device=cuda)[:, None] >= ln
    assert torch.all(d16[invalid] == 0), "dG not exactly 0 past the length"
    # the rows of the last reverse step (s = 0), stored by the flush after the loop:
    # t = 0 forward, t = len - 1 in the reverse direction
    rows = torch.arange(B, device=cuda)
    for last, lastdiff in ((d16[0, :, 0], diff[0, :, 0]), (d16[c["seq"] - 1, rows, 1], diff[c["seq"] - 1, rows, 1])):
        assert torch.all(last.float().abs().amax(dim=-1) > 0)
        assert lastdiff.max().item() < tol
    # the fused bias partials against the column sums of the kernel's own dG
    own = d16.float().sum(dim=(0, 1)).reshape(-1)
    rel = (torch.linalg.norm(db16 - own) / torch.linalg.norm(own)).item()
    print(f"T={T} B={B} bias partials vs own dG column sums: rel {rel:.3e}")
    assert rel < 5e-3


@pytest.mark.parametrize("T,bi", [(1, 0), (7, 0), (3, 2)])
def test_back_to_back_launches_are_deterministic(cuda, ocrk_opts, T, bi):
    """Three forward + BPTT pairs on one stream with no synchronisation between them:
    the flush after a loop runs against the next launch's counting flags."""
    from cnn_lstm_ctc_ocr_amd import kernels as K
    T, B = _tb(T, bi)
    c = _case(cuda, ocrk_opts, T, B)
    K._PERSISTENT.clear()
    K.lstm_error_word(cuda).zero_()
    runs = []
    for _ in range(3):
        f = K.lstm_fwd(c["gx"], c["whT"], c["seq_d"], T, B, H, torch.bfloat16)
        d = K.lstm_bwd(c["wh"], c["seq_d"], c["dout"], f[2], f[3], T, B, H)
        runs.append(tuple(f) + (d,))
    torch.cuda.synchronize()
    assert K.lstm_error_word(cuda).item() == 0
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)
    for a, b in zip(runs[0], tuple(c["fwd", 1]) + (c["bwd", 1][0],)):
        assert torch.equal(a, b)
