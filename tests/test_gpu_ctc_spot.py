"""ocrk_ctc_spot (the best placement of every keyword inside every row, scored
against the greedy path) against tests/ctc_spot_ref.py -- scores bytewise, spans
exactly -- and the keyword switch of the serving Recognizer."""
import numpy as np
import pytest
import torch

import ctc_spot_ref as R
from oracle import ref_model as M

pytestmark = pytest.mark.gpu

C = 96
NEG = np.float32(-np.inf)


def _logits(rng, kind, T, B, C):
    """The logits of tests/test_gpu_ctc_lexicon.py: ReLU'd small integers (exact ties everywhere) or Gaussian."""
    if kind == "int":
        return np.maximum(rng.integers(-3, 4, (T, B, C)), 0).astype(np.float32)
    return np.maximum(rng.standard_normal((T, B, C)) * 3, 0).astype(np.float32)


def _dense(rows, width, fill):
    d = np.full((len(rows), width), fill, np.int32)
    for i, w in enumerate(rows):
        d[i, :len(w)] = w
    return d


def _spot(cuda, logits, seq, kws, alts=None, width=None):
    """(score f32 [B, K], span i32 [B, K, 2], kw_status i32 [K]) of the device as NumPy arrays."""
    from cnn_lstm_ctc_ocr_amd import kernels as K
    width = max(len(k) for k in kws) if width is None else width
    dev = lambda a: torch.from_numpy(a).to(cuda)
    alt = None if alts is None else dev(_dense([a if a is not None else [-1] * len(k) for k, a in zip(kws, alts)],
                                               width, -1))
    out = K.ctc_spot(dev(logits), dev(np.asarray(seq, np.int32)), dev(_dense(kws, width, 0)), alt,
                     dev(np.array([len(k) for k in kws], np.int32)))
    return [o.cpu().numpy() for o in out]


def _same(got, want):
    """Scores bit for bit, spans exactly."""
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    np.testing.assert_array_equal(got[0].view(np.uint32), np.ascontiguousarray(want[0], np.float32).view(np.uint32))
    np.testing.assert_array_equal(got[1], want[1])


def _keyword(rng, n, C, repeats=0):
    """n classes, none equal to either of the two before it (so a planted repeat makes no second one), then
    `repeats` adjacent repeats planted from the front."""
    kw = [int(rng.integers(0, C - 1))]
    while len(kw) < n:
        c = int(rng.integers(0, C - 1))
        if c not in kw[-2:]:
            kw.append(c)
    for i in range(repeats):
        kw[2 * i + 1] = kw[2 * i]
    return kw


def _alternatives(rng, kws, C):
    """An alternative on about half the positions; every fourth keyword has none at all. Some overlap the
    neighbour's label on purpose (the blank is then needed between the two)."""
    alts = []
    for j, kw in enumerate(kws):
        if j % 4 == 3:
            alts.append(None)
            continue
        a = [int(rng.integers(0, C - 1)) if rng.random() < 0.5 else -1 for _ in kw]
        if len(kw) >= 2 and j % 3 == 0:
            a[1] = kw[0]
        alts.append(a)
    return alts


# ------------------------------------------------------------ small, tie-heavy
SMALL_SEQ = [12, 5, 0]


def _small_case(with_alts):
    rng = np.random.default_rng(5)
    logits = _logits(rng, "int", 12, 3, 5)
    kws = [_keyword(rng, n, 5) for n in (1, 1, 2, 2, 3, 3, 4, 5, 6, 7, 12)]
    kws += [[2, 2], [0, 0, 0], [1, 1, 3], [3, 1, 1, 0], [0, 1, 0, 1, 0], [1, 1, 1, 1, 1, 1], [2, 2, 2, 2, 2, 2, 2]]
    assert sorted({R.required_time(k) for k in kws} & {5, 6, 12, 13}) == [5, 6, 12, 13]    # both rows' edges
    return logits, kws, _alternatives(rng, kws, 5) if with_alts else None


@pytest.mark.parametrize("with_alts", [False, True])
def test_small_and_tie_heavy(cuda, with_alts):
    from cnn_lstm_ctc_ocr_amd import kernels as K
    K.status_word(cuda).zero_()
    logits, kws, alts = _small_case(with_alts)
    score, span, status = _spot(cuda, logits, SMALL_SEQ, kws, alts)
    want = R.spot_batch(logits, SMALL_SEQ, kws, alts)
    _same((score, span), want)
    assert status.tolist() == [0] * len(kws)
    assert np.all(np.isneginf(score[2])) and np.all(span[2] == -1)        # the row without frames
    assert np.isfinite(score[0]).sum() > np.isfinite(score[1]).sum() > 0
    assert np.all(score <= 0) and (score[0] == 0).any()
    assert K.read_status(cuda) == 0                                      # not fitting a row is an ordinary result


# --------------------------------------------------------------- serving shape
SERVING_SEQ = [125, 60, 33, 17]
WIDTH = 40                                                               # wider than every keyword


def _serving_keywords(rng):
    """65 keywords: a second chunk with one keyword. Adjacent slots share a wave's turn: (15, 16) and
    (16, 16) are paired, (16, 17) and (17, 15) meet as a paired-size and an unpaired keyword."""
    lens = [1, 2, 15, 16, 16, 16, 16, 17, 17, 15, 31, 32, 32, 32, 17, 17]
    lens += [int(n) for n in rng.integers(1, 17, 30)] + [int(n) for n in rng.integers(17, 33, 10)]
    lens += [int(n) for n in rng.integers(1, 33, 8)] + [5]
    kws = [_keyword(rng, n, C) for n in lens]
    kws[1] = [7, 7]                                                      # "aa"
    kws[12] = _keyword(rng, 32, C, repeats=1)                            # needs 33 frames: zero slack on row 2
    kws[13] = _keyword(rng, 32, C, repeats=2)                            # needs 34: one frame more than row 2 has
    kws[20] = _keyword(rng, 16, C, repeats=1)                            # needs 17: zero slack on row 3
    kws[21] = _keyword(rng, 16, C, repeats=2)                            # needs 18
    for j in (30, 40, 50):                                               # a repeat inside a random keyword
        if len(kws[j]) >= 2:
            kws[j][-1] = kws[j][-2]
    assert len(kws) == 65 and max(map(len, kws)) == 32 < WIDTH
    assert [R.required_time(kws[j]) for j in (12, 13, 20, 21)] == [33, 34, 17, 18]
    return kws


_cache = {}


def _serving(cuda, kind, with_alts):
    """The case's inputs, the helper's answer and the device's, computed once."""
    key = (kind, with_alts)
    if key not in _cache:
        rng = np.random.default_rng(11)
        kws = _serving_keywords(rng)
        alts = _alternatives(rng, kws, C) if with_alts else None
        if alts is not None:                                             # the zero-slack keywords keep their need
            for j in (12, 13, 20, 21):
                alts[j] = None
        logits = _logits(rng, kind, 125, 4, C)
        _cache[key] = (logits, kws, alts, R.spot_batch(logits, SERVING_SEQ, kws, alts),
                       _spot(cuda, logits, SERVING_SEQ, kws, alts, WIDTH))
    return _cache[key]


@pytest.mark.parametrize("with_alts", [False, True])
@pytest.mark.parametrize("kind", ["gauss", "int"])
def test_serving_shape(cuda, kind, with_alts):
    logits, kws, alts, want, (score, span, status) = _serving(cuda, kind, with_alts)
    _same((score, span), want)
    assert status.tolist() == [0] * 65
    need = np.array([R.required_time(k, None if alts is None else alts[j]) for j, k in enumerate(kws)])
    np.testing.assert_array_equal(np.isfinite(score), need[None, :] <= np.array(SERVING_SEQ)[:, None])
    assert np.isfinite(score[2, 12]) and span[2, 12].tolist() == [0, 33] and np.isneginf(score[2, 13])
    assert np.isfinite(score[3, 20]) and span[3, 20].tolist() == [0, 17] and np.isneginf(score[3, 21])
    assert np.all(np.isfinite(score[0])) and np.isfinite(score[0, 64])   # the second chunk's only keyword
    fin = np.isfinite(score)
    assert np.all(score[fin] <= 0) and np.all(span[fin][:, 0] >= 0) and np.all(span[~fin] == -1)
    assert np.all(span[fin][:, 1] - span[fin][:, 0] >= np.broadcast_to(need, score.shape)[fin])
    assert np.all(span[..., 1] <= np.array(SERVING_SEQ)[:, None])


@pytest.mark.parametrize("with_alts", [False, True])
def test_two_calls_are_bitwise_equal(cuda, with_alts):
    logits, kws, alts, _want, first = _serving(cuda, "int", with_alts)
    second = _spot(cuda, logits, SERVING_SEQ, kws, alts, WIDTH)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ LDS switch
@pytest.mark.parametrize("with_alts", [False, True])
def test_workspace_table_at_the_serving_shape(cuda, ocrk_opts, with_alts):
    """CTC_LDS = 0 sends a shape that fits LDS down the route that gathers from the workspace table: the same
    expressions in the same order, so the same bits."""
    logits, kws, alts, _want, lds = _serving(cuda, "gauss", with_alts)
    ocrk_opts("CTC_LDS", 0)
    ws = _spot(cuda, logits, SERVING_SEQ, kws, alts, WIDTH)
    for a, b in zip(lds, ws):
        assert a.tobytes() == b.tobytes()


def test_table_too_large_for_lds(cuda):
    """T = 300: 300 x 96 x 4 B = 115 KB > the 112 KB budget, so the table stays in the workspace. The same
    logits cut to T = 290 (111 KB) with the same lengths take the LDS route: equal bytes, and the helper's."""
    rng = np.random.default_rng(13)
    logits = _logits(rng, "gauss", 300, 2, C)
    seq = [290, 201]
    kws = [_keyword(rng, n, C) for n in (1, 3, 8, 16, 17, 32)] + [_keyword(rng, 9, C, repeats=2)]
    alts = _alternatives(rng, kws, C)
    ws = _spot(cuda, logits, seq, kws, alts)
    lds = _spot(cuda, np.ascontiguousarray(logits[:290]), seq, kws, alts)
    for a, b in zip(lds, ws):
        assert a.tobytes() == b.tobytes()
    _same(ws[:2], R.spot_batch(logits, seq, kws, alts))
    whole = _spot(cuda, logits, [300, 4000], kws, alts)                  # every frame; seq_len clamps to T
    _same(whole[:2], R.spot_batch(logits, [300, 300], kws, alts))


@pytest.mark.parametrize("lds", [1, 0])
def test_tail_frames_are_never_read(cuda, ocrk_opts, lds):
    logits, kws, alts, _want, clean = _serving(cuda, "gauss", True)
    ocrk_opts("CTC_LDS", lds)
    dirty = logits.copy()
    for b, n in enumerate(SERVING_SEQ):
        dirty[n:, b] = np.nan
    got = _spot(cuda, dirty, SERVING_SEQ, kws, alts, WIDTH)
    for a, b in zip(clean, got):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------ planted keywords
def _planted(text, T=30, first=3):
    """Logits [T, 2, C] whose argmax path reads `text` from frame `first` ('.' = blank), blank elsewhere."""
    from cnn_lstm_ctc_ocr_amd.mjsynth import out_charset
    assert len(out_charset) == C - 1
    rng = np.random.default_rng(17)
    logits = rng.random((T, 1, C)).astype(np.float32)
    path = [C - 1] * T
    for j, ch in enumerate(text):
        path[first + j] = C - 1 if ch == "." else out_charset.index(ch)
    logits[np.arange(T), 0, path] = 5.0
    return logits


def test_planted_keywords(cuda):
    from cnn_lstm_ctc_ocr_amd import decode
    logits = torch.from_numpy(np.concatenate([_planted("TTOTAAL..x"), _planted("tTOTAAL..x")], axis=1)).to(cuda)
    seq = torch.tensor([30, 30], dtype=torch.int32, device=cuda)
    score, span = decode.ctc_keyword_spotter(logits, seq, decode.KeywordSet(["TOTAL", "total", "TOTAL."]))
    score, span = score.cpu().numpy(), span.cpu().numpy()
    # row 0 reads ...TTOTAAL..x: TOTAL is on the argmax path, frames 3..9
    assert score[0, 0].tobytes() == np.float32(0).tobytes() and span[0, 0].tolist() == [3, 10]
    assert score[0, 1] < 0 and score[0, 2] < 0
    # row 1 reads ...tTOTAAL..x: the hit begins one frame later
    assert score[1, 0].tobytes() == np.float32(0).tobytes() and span[1, 0].tolist() == [4, 10]
    folded = decode.KeywordSet(["total"], case_insensitive=True)
    score, span = decode.ctc_keyword_spotter(logits, seq, folded)
    assert score.cpu().numpy().tobytes() == np.zeros((2, 1), np.float32).tobytes()
    # the documented looseness: the run "tT" of row 1 counts as one "t"
    assert span.cpu().numpy().tolist() == [[[3, 10]], [[3, 10]]]


# ------------------------------------------------------------ invalid keywords
def test_invalid_keywords(cuda):
    """Bad lengths, labels and alternatives: kw_status 2 / 3, -inf and (-1, -1) on every row, the status
    word's two bits, and the valid keywords of the same call untouched."""
    from cnn_lstm_ctc_ocr_amd import _lib
    from cnn_lstm_ctc_ocr_amd import kernels as K
    K.status_word(cuda).zero_()
    rng = np.random.default_rng(19)
    T, B, W = 40, 3, 36
    seq = [40, 21, 6]
    good = [_keyword(rng, n, C) for n in (3, 1, 16, 17, 6)]
    good_alts = _alternatives(rng, good, C)
    logits = _logits(rng, "gauss", T, B, C)
    lab = _dense(good, W, 0)
    alt = _dense([a if a is not None else [] for a in good_alts], W, -1)
    ln = [len(k) for k in good]
    # keywords 5..10: length 0, length 33, the blank as a label, a label -5, an alternative C, an alternative -2
    bad_lab = np.zeros((6, W), np.int32)
    bad_alt = np.full((6, W), -1, np.int32)
    bad_lab[0, :3] = bad_lab[1, :3] = [1, 2, 3]
    bad_lab[2, :3] = [1, C - 1, 3]
    bad_lab[3, :3] = [4, -5, 2]
    bad_lab[4, :3] = bad_lab[5, :3] = [4, 5, 6]
    bad_alt[4, 2] = C
    bad_alt[5, 0] = -2
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(cuda)
    lg, sq = torch.from_numpy(logits).to(cuda), dev(seq)
    score, span, status = [o.cpu().numpy() for o in K.ctc_spot(
        lg, sq, dev(np.concatenate([lab, bad_lab])), dev(np.concatenate([alt, bad_alt])),
        dev(ln + [0, 33, 3, 3, 3, 3]))]
    assert K.read_status(cuda, reset=False) == _lib.STATUS_CTC_BAD_LENGTH | _lib.STATUS_CTC_BAD_LABEL
    assert status.tolist() == [0] * 5 + [2, 2, 3, 3, 3, 3]
    assert np.all(np.isneginf(score[:, 5:])) and np.all(span[:, 5:] == -1)
    only_good = [o.cpu().numpy() for o in K.ctc_spot(lg, sq, dev(lab), dev(alt), dev(ln))]
    assert only_good[0].tobytes() == np.ascontiguousarray(score[:, :5]).tobytes()
    assert only_good[1].tobytes() == np.ascontiguousarray(span[:, :5]).tobytes()
    _same(only_good[:2], R.spot_batch(logits, seq, good, good_alts))
    assert np.all(np.isfinite(score[0, :5]))
    K.clear_status(cuda, _lib.STATUS_CTC_BAD_LENGTH | _lib.STATUS_CTC_BAD_LABEL)
    assert K.read_status(cuda) == 0


# --------------------------------------------------------------- bad arguments
def test_bad_arguments_launch_nothing(cuda):
    from cnn_lstm_ctc_ocr_amd import _lib
    from cnn_lstm_ctc_ocr_amd import kernels as K
    logits = torch.zeros(4, 2, C, device=cuda)
    seq = torch.full((2,), 4, dtype=torch.int32, device=cuda)
    lab = torch.zeros(3, 2, dtype=torch.int32, device=cuda)
    ln = torch.ones(3, dtype=torch.int32, device=cuda)
    with pytest.raises(TypeError):
        K.ctc_spot(logits.bfloat16(), seq, lab, None, ln)
    with pytest.raises(TypeError):
        K.ctc_spot(logits, seq, lab.long(), None, ln)
    with pytest.raises(TypeError):
        K.ctc_spot(logits, seq, lab, lab.long(), ln)
    with pytest.raises(ValueError):
        K.ctc_spot(logits, seq, lab, lab[:, :1].contiguous(), ln)
    with pytest.raises(ValueError):
        K.ctc_spot(logits, seq, lab, None, ln[:2])
    with pytest.raises(_lib.InvalidArgumentError, match="max_kw_len=256"):
        K.ctc_spot(logits, seq, torch.zeros(3, 256, dtype=torch.int32, device=cuda), None, ln)
    with pytest.raises(_lib.InvalidArgumentError, match="C=1"):
        K.ctc_spot(torch.zeros(4, 2, 1, device=cuda), seq, lab, None, ln)
    with pytest.raises(_lib.InvalidArgumentError, match="T=4097"):
        K.ctc_spot(torch.zeros(4097, 1, 2, device=cuda), seq[:1].contiguous(), lab, None, ln)
    # a short workspace: the error comes back and the outputs keep their bytes
    score = torch.full((2, 3), 7.0, device=cuda)
    span = torch.full((2, 3, 2), 7, dtype=torch.int32, device=cuda)
    nb = _lib.lib().ocrk_ctc_spot_workspace_size(4, 2, C, 3, 2)
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
    args = [_lib.ptr(logits), _lib.ptr(seq), 4, 2, C, _lib.ptr(lab), None, _lib.ptr(ln), 3, 2, _lib.ptr(score),
            _lib.ptr(span), None, None, _lib.ptr(ws), nb - 16, _lib.stream_ptr(cuda)]
    with pytest.raises(_lib.InvalidArgumentError, match="workspace too small"):
        _lib.call("ocrk_ctc_spot", *args)
    torch.cuda.synchronize()
    assert bool((score == 7).all()) and bool((span == 7).all())
    args[15] = nb                                                        # and with the workspace it asks for, it runs
    _lib.call("ocrk_ctc_spot", *args)
    assert bool((score == 0).all()) and span[:, :, 1].tolist() == [[1] * 3] * 2


# ---------------------------------------------------------------- the service
SIZES = (64, 64)
E2E_KEYWORDS = ["TOTAL", "gst", "a", "Change Due", "receipt no.", "ee", "x" * 32, "9.99"]


@pytest.fixture(scope="module")
def service(cuda):
    """The store of tests/test_gpu_server.py, 32 x 64 and 32 x 256 crops in one batch, and the eager
    logits of the batch."""
    from cnn_lstm_ctc_ocr_amd import ModelConfig, ParamStore
    from cnn_lstm_ctc_ocr_amd.config import INFER
    from cnn_lstm_ctc_ocr_amd.mjsynth import num_classes
    from cnn_lstm_ctc_ocr_amd.model import convnet_layers, rnn_layers
    vals = M.init_params(seed=0, rnn_sizes=SIZES)
    for k in vals:
        if "lstm_cell/kernel" in k:
            vals[k] = (vals[k] * 20).astype(np.float32)
    store = ParamStore(ModelConfig(rnn_sizes=SIZES, dtype=torch.float32), device=cuda, values=vals)
    rng = np.random.default_rng(23)
    widths = np.array([64, 256, 256, 64], np.int32)
    batch = np.zeros((4, 32, 256, 1), np.uint8)
    for b, w in enumerate(widths):
        batch[b, :, :w, 0] = rng.integers(0, 256, (32, int(w)))
    with torch.no_grad():
        feats, seq = convnet_layers(torch.from_numpy(batch).to(cuda), torch.from_numpy(widths).to(cuda), INFER, store)
        logits = rnn_layers(feats, seq, num_classes(), store).float().contiguous()
    return store, batch, widths, logits, seq.to(torch.int32).contiguous()


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("case_insensitive", [False, True])
def test_recognizer_with_keywords(cuda, service, graphs, case_insensitive):
    from cnn_lstm_ctc_ocr_amd import decode
    from cnn_lstm_ctc_ocr_amd import kernels as K
    from cnn_lstm_ctc_ocr_amd.server import KeywordHit, KeywordRecognition, Recognition, Recognizer
    store, batch, widths, logits, seq = service
    K.status_word(cuda).zero_()
    assert seq.tolist() == [29, 125, 125, 29]
    kset = decode.KeywordSet(E2E_KEYWORDS, case_insensitive)
    score, span = decode.ctc_keyword_spotter(logits, seq, kset)
    score, span = score.cpu().numpy(), span.cpu().numpy()
    assert np.isneginf(score[0, 6]) and np.isfinite(score[1, 6])         # 32 symbols do not fit 29 frames

    plain = Recognizer(store, graphs=graphs)(batch, widths)
    got = Recognizer(store, keywords=E2E_KEYWORDS, keyword_threshold=-1e30, case_insensitive=case_insensitive,
                     graphs=graphs)(batch, widths)
    assert len(got) == 4 and all(type(r) is KeywordRecognition and r.detail is None for r in got)
    assert [r.text for r in got] == plain
    for b, r in enumerate(got):
        ks = [k for k in range(len(E2E_KEYWORDS)) if np.isfinite(score[b, k])]
        ks.sort(key=lambda k: (-score[b, k], k))
        assert [h.keyword for h in r.hits] == [E2E_KEYWORDS[k] for k in ks]
        for h, k in zip(r.hits, ks):
            assert type(h) is KeywordHit and all(type(v) in (str, float, int) for v in h)
            assert np.float32(h.score).tobytes() == score[b, k].tobytes()
            assert (h.first_frame, h.end_frame) == tuple(span[b, k].tolist())
            assert (h.x0, h.x1) == decode.frames_to_px(h.first_frame, h.end_frame, widths[b])
            assert 0 <= h.x0 < h.x1 <= widths[b]
    # a higher threshold: the subset at or above it, in the same order
    thr = float(np.median(score[np.isfinite(score)]))
    some = Recognizer(store, keywords=kset, keyword_threshold=thr, graphs=graphs, detail=True)(batch, widths)
    detail = Recognizer(store, graphs=graphs, detail=True)(batch, widths)
    assert 0 < sum(len(r.hits) for r in some) < sum(len(r.hits) for r in got)
    for r, full, d in zip(some, got, detail):
        assert r.hits == tuple(h for h in full.hits if h.score >= thr)
        assert type(r.detail) is Recognition and r.detail == d and r.text == d.text == full.text
    assert K.read_status(cuda) == 0


def test_keyword_spotter_makes_no_host_sync(cuda, service):
    from cnn_lstm_ctc_ocr_amd import decode
    store, batch, widths, logits, seq = service
    kset = decode.KeywordSet(E2E_KEYWORDS, case_insensitive=True)
    decode.ctc_keyword_spotter(logits, seq, kset)                        # uploads the keywords' tensors
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        score, span = decode.ctc_keyword_spotter(logits, seq, kset)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(score.shape) == (4, 8) and score.dtype == torch.float32
    assert tuple(span.shape) == (4, 8, 2) and span.dtype == torch.int32
