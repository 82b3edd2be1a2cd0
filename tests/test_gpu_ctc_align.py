"""ocrk_ctc_align (forced alignment of a label to the logits) against the
float32 restatement of its recursion (tests/ctc_align_ref.py), and the detailed
result of the serving Recognizer built on it."""
import math
import threading

import numpy as np
import pytest
import torch

import ctc_align_ref as R
from oracle import ref_graph as G
from oracle import ref_model as M

pytestmark = pytest.mark.gpu


def _logits(rng, kind, T, B, C):
    """ReLU'd logits, as the model's: small integers (exact ties everywhere) or Gaussian."""
    if kind == "int":
        return np.maximum(rng.integers(-3, 4, (T, B, C)), 0).astype(np.float32)
    return np.maximum(rng.standard_normal((T, B, C)) * 3, 0).astype(np.float32)


def _dense(labels, width=None):
    Lmax = max([len(l) for l in labels] + [0]) if width is None else width
    d = np.zeros((len(labels), Lmax), np.int32)
    for i, l in enumerate(labels):
        d[i, :len(l)] = l
    return d, np.array([len(l) for l in labels], np.int32)


def _align(cuda, logits, labels, seq, width=None):
    from cnn_lstm_ctc_ocr_amd import kernels as K
    lab, ln = _dense(labels, width)
    out = K.ctc_align(torch.from_numpy(logits).to(cuda), torch.from_numpy(lab).to(cuda),
                      torch.from_numpy(ln).to(cuda), torch.from_numpy(np.asarray(seq, np.int32)).to(cuda))
    return [o.cpu().numpy() for o in out]


def _check_exact(cuda, logits, labels, seq, width=None):
    fs, span, conf, logp, status = _align(cuda, logits, labels, seq, width)
    assert status.tolist() == [0] * len(labels)
    want_fs, want_span = R.align_batch(logits, labels, seq)
    np.testing.assert_array_equal(fs, want_fs)
    np.testing.assert_array_equal(span[:, :want_span.shape[1]], want_span)
    assert np.all(span[:, want_span.shape[1]:] == -1) and np.all(conf[:, want_span.shape[1]:] == 0)
    for b, l in enumerate(labels):
        assert np.all(conf[b, len(l):] == 0) and np.all(conf[b, :len(l)] > 0)
    return fs, span, conf, logp


def _labels(rng, C, lens):
    return [[int(c) for c in rng.integers(0, C - 1, n)] for n in lens]


def _cases(rng, C):
    """name -> (T, labels, seq_len, label tensor width or None): the smallest
    shapes at which each route of the kernel can go wrong."""
    cases = {}
    # ragged rows, label lengths 0 / 1 / 2 / 8; adjacent repeats (skip forbidden);
    # a row with zero slack (seq_len = len + repeats: one feasible path)
    labels = _labels(rng, C, [0, 1, 2, 8, 8]) + [[1, 1, 2, 2, 2], [3, 3, 0, 0, 0, 1]]
    seq = [1, 7, 19, 33, 40, 23, R.required_time(labels[6])]
    seq = [max(s, R.required_time(l)) for s, l in zip(seq, labels)]
    cases["ragged"] = (40, labels, seq, None)
    cases["one_frame"] = (1, [[], [2]], [1, 1], None)
    # S = 63 / 65 / 67: around the one-register boundary at lanes 63 / 64, together (two registers
    # for every row) and each alone (its own register count)
    l3 = _labels(rng, C, [31, 32, 33])
    cases["boundary"] = (100, l3, [100, 93, 100], None)
    for l in l3:
        cases[f"boundary_{len(l)}"] = (100, [l], [100], None)
    cases["four_registers_lds"] = (110, _labels(rng, C, [70, 3]), [110, 41], None)
    cases["eight_registers_lds"] = (50, _labels(rng, C, [20, 25]), [50, 44], 130)   # a wide label tensor, short labels
    cases["len200_workspace"] = (512, _labels(rng, C, [200]), [512], None)
    cases["len255_workspace"] = (1024, _labels(rng, C, [255, 100]), [1024, 700], None)
    return cases


CASE_NAMES = ["ragged", "one_frame", "boundary", "boundary_31", "boundary_32", "boundary_33", "four_registers_lds",
              "eight_registers_lds", "len200_workspace", "len255_workspace"]


@pytest.mark.parametrize("C", [96, 5])
@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_path_is_bit_exact(cuda, name, kind, C):
    rng = np.random.default_rng(CASE_NAMES.index(name) * 7 + C)
    T, labels, seq, width = _cases(rng, C)[name]
    for l, s in zip(labels, seq):
        assert R.feasible(l, s)
    _check_exact(cuda, _logits(rng, kind, T, len(labels), C), labels, seq, width)


@pytest.mark.parametrize("name", ["ragged", "boundary"])
def test_workspace_route_at_small_shapes(cuda, ocrk_opts, name):
    """CTC_LDS = 0 sends every shape down the route with the backpointers in
    the workspace and the emissions read from the logits."""
    ocrk_opts("CTC_LDS", 0)
    rng = np.random.default_rng(77)
    T, labels, seq, width = _cases(rng, 96)[name]
    _check_exact(cuda, _logits(rng, "int", T, len(labels), 96), labels, seq, width)


def test_planted_path_is_recovered(cuda):
    """Logits built from a known path (+8 on its class at every frame, noise
    below 1 elsewhere): the spans are the planted runs. Independent of the
    restatement."""
    rng = np.random.default_rng(21)
    T, B, C = 60, 4, 96
    labels = [[5, 5, 9, 1], [7], list(rng.integers(0, 95, 12)), [3, 4, 4, 4, 2, 2]]
    seq = [60, 17, 52, 33]
    logits = rng.random((T, B, C)).astype(np.float32)
    runs = []
    for b, (l, L) in enumerate(zip(labels, seq)):
        ext = R.extended(l, C - 1)
        # run lengths: every symbol >= 1 frame, a blank between repeats >= 1, other blanks >= 0
        need = np.array([1 if (s % 2 == 1 or (0 < s < len(ext) - 1 and ext[s - 1] == ext[s + 1])) else 0
                         for s in range(len(ext))])
        extra = rng.multinomial(L - need.sum(), np.ones(len(ext)) / len(ext))
        states = np.repeat(np.arange(len(ext)), need + extra)
        assert len(states) == L
        logits[np.arange(L), b, ext[states]] += 8.0
        runs.append(R.spans(states, len(l)))
    fs, span, conf, logp, status = _align(cuda, logits, labels, seq)
    assert status.tolist() == [0] * B
    for b, l in enumerate(labels):
        np.testing.assert_array_equal(span[b, :len(l)], runs[b])
        assert np.all(span[b, len(l):] == -1)


@pytest.mark.parametrize("name", ["ragged", "boundary", "len200_workspace"])
def test_values_along_the_device_path(cuda, name):
    """path_logp and char_conf against float64 values computed from the
    device's own frame_state; a single path never beats the sum over paths."""
    from cnn_lstm_ctc_ocr_amd import kernels as K
    rng = np.random.default_rng(5)
    C = 96
    T, labels, seq, width = _cases(rng, C)[name]
    logits = _logits(rng, "gauss", T, len(labels), C)
    fs, span, conf, logp = _check_exact(cuda, logits, labels, seq, width)
    for b, (l, L) in enumerate(zip(labels, seq)):
        want_logp, want_conf = R.path_values(logits[:L, b], fs[b, :L], l)
        # the project's CTC tolerance (tests/test_gpu_ctc.py) plus an absolute floor
        np.testing.assert_allclose(logp[b], want_logp, rtol=1e-3, atol=1e-5)
        np.testing.assert_allclose(np.log(conf[b, :len(l)]), np.log(want_conf), rtol=1e-3, atol=1e-5)
    lab, ln = _dense(labels, width)
    loss, _, _ = K.ctc_loss(torch.from_numpy(logits).to(cuda), torch.from_numpy(lab).to(cuda),
                            torch.from_numpy(ln).to(cuda), torch.from_numpy(np.asarray(seq, np.int32)).to(cuda),
                            need_grad=False)
    loss = loss.cpu().numpy()
    assert np.all(logp <= -loss + 1e-4 * np.abs(loss))


def test_error_rows_are_flagged_like_the_loss(cuda):
    """The bad-row batch of tests/test_gpu_ctc.py (bad lengths, bad label
    values) and its infeasible batch: the status codes of ocrk_ctc_loss, void
    outputs for the flagged rows, the good row untouched."""
    from cnn_lstm_ctc_ocr_amd import _lib
    from cnn_lstm_ctc_ocr_amd import kernels as K
    K.status_word(cuda).zero_()
    rng = np.random.default_rng(5)
    T, B, C = 20, 5, 96
    logits_h = rng.standard_normal((T, B, C)).astype(np.float32)
    logits = torch.from_numpy(logits_h).to(cuda)
    lab = torch.tensor([[1, 2, 3], [1, 2, 3], [1, 95, 3], [4, -1, 3], [7, 8, 9]], dtype=torch.int32, device=cuda)
    ln = torch.tensor([3, 400, 3, 3, -2], dtype=torch.int32, device=cuda)
    seq = torch.full((B,), T, dtype=torch.int32, device=cuda)
    _, _, loss_status = K.ctc_loss(logits, lab, ln, seq, need_grad=False)
    assert K.read_status(cuda) == _lib.STATUS_CTC_BAD_LENGTH | _lib.STATUS_CTC_BAD_LABEL
    fs, span, conf, logp, status = [o.cpu().numpy() for o in K.ctc_align(logits, lab, ln, seq)]
    assert status.tolist() == loss_status.cpu().tolist() == [0, 2, 3, 3, 2]
    assert K.read_status(cuda) == _lib.STATUS_CTC_BAD_LENGTH | _lib.STATUS_CTC_BAD_LABEL
    assert np.all(fs[1:] == -1) and np.all(span[1:] == -1) and np.all(conf[1:] == 0)
    assert np.all(np.isneginf(logp[1:])) and np.isfinite(logp[0])
    want_fs, want_span = R.align_batch(logits_h[:, :1], [[1, 2, 3]], [T])
    np.testing.assert_array_equal(fs[:1], want_fs)
    np.testing.assert_array_equal(span[:1], want_span)
    # infeasible: [1, 1, 2] needs 4 frames; seq_len 0
    logits = torch.zeros(3, 3, 96, device=cuda)
    lab = torch.tensor([[1, 1, 2], [1, 2, 3], [0, 0, 0]], dtype=torch.int32, device=cuda)
    ln = torch.tensor([3, 3, 0], dtype=torch.int32, device=cuda)
    seq = torch.tensor([3, 3, 0], dtype=torch.int32, device=cuda)
    _, _, loss_status = K.ctc_loss(logits, lab, ln, seq, need_grad=False)
    fs, span, conf, logp, status = [o.cpu().numpy() for o in K.ctc_align(logits, lab, ln, seq)]
    assert status.tolist() == loss_status.cpu().tolist() == [1, 0, 1]
    assert K.read_status(cuda) == _lib.STATUS_CTC_INFEASIBLE
    assert np.all(fs[[0, 2]] == -1) and np.all(span[[0, 2]] == -1) and np.all(conf[[0, 2]] == 0)
    assert np.all(np.isneginf(logp[[0, 2]]))
    assert fs[1].tolist() == [1, 3, 5] and span[1].tolist() == [[0, 1], [1, 2], [2, 3]]


def test_greedy_decode_always_aligns_and_collapses_back(cuda):
    from cnn_lstm_ctc_ocr_amd import decode
    rng = np.random.default_rng(11)
    T, B, C = 125, 64, 96
    logits = np.maximum(np.round(rng.standard_normal((T, B, C)) * 2) / 2, 0).astype(np.float32)
    logits[:, :, 95] += (rng.random((T, B)) < 0.5) * 3.0              # frequent blanks
    seq = rng.integers(1, T + 1, B).astype(np.int32)
    lg, sq = torch.from_numpy(logits).to(cuda), torch.from_numpy(seq).to(cuda)
    out, out_len, _ = decode.ctc_greedy_decoder_raw(lg, sq)
    fs, span, conf, logp, status = [o.cpu().numpy() for o in decode.ctc_alignment(lg, out, out_len, sq)]
    assert span.shape == (B, T, 2)                                     # the decoder's dense width
    assert status.tolist() == [0] * B
    out, out_len = out.cpu().numpy(), out_len.cpu().numpy()
    for b in range(B):
        label = out[b, :out_len[b]].tolist()
        ext = R.extended(label, C - 1)
        assert np.all(fs[b, seq[b]:] == -1)
        assert R.collapse(ext[fs[b, :seq[b]]], C - 1) == label
        assert np.all(span[b, out_len[b]:] == -1)


# ---------------------------------------------------------------- the service
SIZES = (64, 64)


def _store(cuda, seed=0):
    """The store of tests/test_gpu_server.py."""
    from cnn_lstm_ctc_ocr_amd import ModelConfig, ParamStore
    vals = M.init_params(seed=seed, rnn_sizes=SIZES)
    for k in vals:
        if "lstm_cell/kernel" in k:
            vals[k] = (vals[k] * 20).astype(np.float32)
    return ParamStore(ModelConfig(rnn_sizes=SIZES, dtype=torch.float32), device=cuda, values=vals), vals


@pytest.fixture(scope="module")
def bucket_batch(cuda):
    """One 16-row bucket batch, the store, and the oracle's logits on it (computed once)."""
    from cnn_lstm_ctc_ocr_amd.server import Bucket, fill_batch
    store, vals = _store(cuda)
    rng = np.random.default_rng(1)
    b = Bucket(0.0, 16, (96, 128))
    for i, w in enumerate(rng.integers(97, 129, 13)):
        b.addImgToBucket("0", str(i), 0.0, rng.integers(0, 256, (32, int(w))).astype(np.uint8))
    _infos, batch, wd = fill_batch(*b.getBatch(now=1.0), 16)
    logits_ref, seq_ref = M.RefModel(vals, "lstm", SIZES).forward(G.preprocess(batch), wd, training=False)
    return store, batch, wd, logits_ref, seq_ref


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("decoder", ["greedy", "beam"])
def test_recognizer_detail(cuda, bucket_batch, decoder, graphs):
    from cnn_lstm_ctc_ocr_amd.mjsynth import out_charset
    from cnn_lstm_ctc_ocr_amd.server import Recognition, Recognizer
    store, batch, wd, logits_ref, seq_ref = bucket_batch
    texts = Recognizer(store, decoder=decoder, beam_width=16, graphs=graphs)(batch, wd)
    got = Recognizer(store, decoder=decoder, beam_width=16, graphs=graphs, detail=True)(batch, wd)
    assert len(got) == len(texts) == 16 and all(type(r) is Recognition for r in got)
    assert [r.text for r in got] == texts
    labels = [[out_charset.index(c) for c in t] for t in texts]
    loss_ref, _ = G.ctc_loss(logits_ref, labels, seq_ref)
    for r, w, loss in zip(got, wd, loss_ref):
        assert r.confidence > 0
        print(f"{decoder} graphs={graphs} {r.text!r}: log confidence {math.log(r.confidence):.5f} oracle {-loss:.5f}")
        np.testing.assert_allclose(math.log(r.confidence), -loss, rtol=1e-3)
        assert len(r.char_confidence) == len(r.char_px) == len(r.text)
        assert all(0 < c <= 1 for c in r.char_confidence)
        flat = [x for px in r.char_px for x in px]
        assert all(0 <= x <= w for x in flat) and flat == sorted(flat)


def test_service_delivers_recognitions(cuda):
    from cnn_lstm_ctc_ocr_amd.linepredictor import BatchLinePredictor
    from cnn_lstm_ctc_ocr_amd.server import LocalServer, Recognition, Recognizer
    store, _ = _store(cuda, seed=2)
    srv = LocalServer(Recognizer(store, detail=True), bucket_size=8, bucket_max_time=0.0)
    client = BatchLinePredictor(srv)
    rng = np.random.default_rng(3)
    crops = [rng.integers(0, 256, (32, int(w))).astype(np.uint8) for w in rng.integers(40, 300, 12)]
    stop = threading.Event()
    th = threading.Thread(target=srv.run, kwargs={"stop": stop.is_set, "idle_sleep": 0.001})
    th.start()
    try:
        got = client.predict_batch("page", crops, give_up_after=50000)
    finally:
        stop.set()
        th.join()
    plain = Recognizer(store)
    for i, c in enumerate(crops):
        r = got[i]
        assert type(r) is Recognition and len(r.char_px) == len(r.char_confidence) == len(r.text)
        assert all(0 <= x0 <= x1 <= c.shape[1] for x0, x1 in r.char_px)
        w = c.shape[1]
        x = np.zeros((1, 32, -(-w // 32) * 32, 1), np.uint8)
        x[0, :, :w, 0] = c
        assert plain(x, np.array([w], np.int32))[0] == r.text
