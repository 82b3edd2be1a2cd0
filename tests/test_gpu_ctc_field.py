"""ocrk_ctc_field (the best-scoring string matching a character-class pattern
inside every row, scored against the greedy path) against tests/ctc_field_ref.py
-- scores bytewise, spans and texts exactly --, against ocrk_ctc_spot over an
enumerated language, and the fields switch of the serving Recognizer."""
import numpy as np
import pytest
import torch

import ctc_field_ref as F
from oracle import ref_model as M

pytestmark = pytest.mark.gpu

C = 96
DIGITS = list(range(52, 62))                                             # '0'..'9' in mjsynth.out_charset
DOT = 90                                                                 # '.'


def _logits(rng, kind, T, B, C):
    """The logits of tests/test_gpu_ctc_spot.py: ReLU'd small integers (exact ties everywhere) or Gaussian."""
    if kind == "int":
        return np.maximum(rng.integers(-3, 4, (T, B, C)), 0).astype(np.float32)
    return np.maximum(rng.standard_normal((T, B, C)) * 3, 0).astype(np.float32)


def _dense(patterns, width):
    """(pat_cls [P, width, 16] -1 padded, pat_opt [P, width], pat_len [P]) as int32 arrays."""
    cls = np.full((len(patterns), width, 16), -1, np.int32)
    opt = np.zeros((len(patterns), width), np.int32)
    for p, (c, o) in enumerate(patterns):
        for i, labels in enumerate(c):
            cls[p, i, :len(labels)] = labels
        opt[p, :len(o)] = o
    return cls, opt, np.array([len(c) for c, _ in patterns], np.int32)


def _field(cuda, logits, seq, patterns, width=None):
    """(score f32 [B, P], span i32 [B, P, 2], text i32 [B, P, width], pat_status i32 [P]) of the device."""
    from cnn_lstm_ctc_ocr_amd import kernels as K
    width = max(len(c) for c, _ in patterns) if width is None else width
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    cls, opt, ln = _dense(patterns, width)
    out = K.ctc_field(dev(logits), dev(np.asarray(seq, np.int32)), dev(cls), dev(opt), dev(ln))
    return [o.cpu().numpy() for o in out]


def _same(got, want):
    """Scores bit for bit, spans and texts exactly."""
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    for g, w in zip(got, want):
        assert g.shape == w.shape
    np.testing.assert_array_equal(got[0].view(np.uint32), np.ascontiguousarray(want[0], np.float32).view(np.uint32))
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])


def _pattern(rng, n, C, sizes=(1, 1, 1, 2, 3, 5, 10, 16), p_opt=0.35):
    """n positions: classes of the given sizes drawn at random, optional flags within the structure's limits."""
    cls = [sorted(int(l) for l in rng.choice(C - 1, int(rng.choice(sizes)), replace=False)) for _ in range(n)]
    opt, run = [], 0
    for i in range(n):
        o = int(i > 0 and run < 3 and rng.random() < p_opt)
        run = run + 1 if o else 0
        opt.append(o)
    return cls, opt


def _singletons(rng, n, C, repeats):
    """n mandatory one-label positions, no label equal to either of the two before it, then `repeats` adjacent
    repeats planted from the front: n + repeats frames are needed."""
    lab = [int(rng.integers(0, C - 1))]
    while len(lab) < n:
        c = int(rng.integers(0, C - 1))
        if c not in lab[-2:]:
            lab.append(c)
    for i in range(repeats):
        lab[2 * i + 1] = lab[2 * i]
    return [[l] for l in lab], [0] * n


# ------------------------------------------------------------ small, tie-heavy
SMALL_SEQ = [12, 5, 0]


def test_small_and_tie_heavy(cuda):
    from cnn_lstm_ctc_ocr_amd import kernels as K
    K.status_word(cuda).zero_()
    logits = _logits(np.random.default_rng(5), "int", 12, 3, 5)
    score, span, text, status = _field(cuda, logits, SMALL_SEQ, F.SMALL_PATTERNS)
    _same((score, span, text), F.field_batch(logits, SMALL_SEQ, F.SMALL_PATTERNS))
    assert status.tolist() == [0] * len(F.SMALL_PATTERNS)
    assert np.all(np.isneginf(score[2])) and np.all(span[2] == -1) and np.all(text[2] == -1)   # the row without frames
    assert np.all(np.isfinite(score[:2])) and np.all(score <= 0) and (score[0] == 0).any()
    assert K.read_status(cuda) == 0


# --------------------------------------------------------------- serving shape
SERVING_SEQ = [125, 60, 33, 17]
WIDTH = 18                                                               # wider than every pattern
N_PAT = 41                                                               # five workgroups of 8 and one pattern more


def _serving_patterns(rng):
    pats = [
        _singletons(rng, 16, C, 1),                                      # needs 17 frames: zero slack on row 3
        _singletons(rng, 16, C, 2),                                      # needs 18: one frame more than row 3 has
        ([sorted(int(l) for l in rng.choice(C - 1, 16, replace=False)) for _ in range(3)], [0, 0, 0]),
        ([DIGITS[1:]] + [DIGITS] * 3 + [[DOT]] + [DIGITS] * 2, [0, 1, 1, 1, 0, 0, 1]),     # an amount
        ([[3], [4, 5], [5, 6], [4, 7], [8], [9, 10], [3, 9]], [0, 1, 1, 1, 0, 1, 1]),      # 3 optionals, 2 trailing
        _pattern(rng, 16, C, p_opt=0.5),
        _pattern(rng, 16, C, sizes=(16,), p_opt=0.5),
        ([DIGITS] * 16, [0, 0] + [1, 1, 1, 0] * 3 + [1, 1]),
        ([[7]], [0]),
        ([[7], [7]], [0, 0]),                                            # "aa"
    ]
    lens = [int(n) for n in rng.integers(1, 5, 10)] + [int(n) for n in rng.integers(5, 9, 10)]
    lens += [int(n) for n in rng.integers(9, 17, 6)] + [int(n) for n in rng.integers(1, 17, 5)]
    pats += [_pattern(rng, n, C) for n in lens]
    assert len(pats) == N_PAT and max(len(c) for c, _ in pats) == 16 < WIDTH
    assert all(F.structure_ok(o) for _, o in pats)
    return pats


_cache = {}


def _serving(cuda, kind):
    """The case's inputs, the helper's answer and the device's, computed once."""
    if kind not in _cache:
        rng = np.random.default_rng(11)
        pats = _serving_patterns(rng)
        logits = _logits(rng, kind, 125, 4, C)
        _cache[kind] = (logits, pats, F.field_batch(logits, SERVING_SEQ, pats, WIDTH),
                        _field(cuda, logits, SERVING_SEQ, pats, WIDTH))
    return _cache[kind]


@pytest.mark.parametrize("kind", ["gauss", "int"])
def test_serving_shape(cuda, kind):
    logits, pats, want, (score, span, text, status) = _serving(cuda, kind)
    _same((score, span, text), want)
    assert status.tolist() == [0] * N_PAT
    assert np.isfinite(score[3, 0]) and span[3, 0].tolist() == [0, 17] and np.isneginf(score[3, 1])
    assert np.all(text[3, 0, :16] == [c[0] for c in pats[0][0]]) and np.all(text[3, 1] == -1)
    assert np.all(np.isfinite(score[0])) and np.isfinite(score[0, 40])   # the last workgroup's only pattern
    fin = np.isfinite(score)
    assert np.all(score[fin] <= 0) and np.all(span[fin][:, 0] >= 0) and np.all(span[~fin] == -1)
    assert np.all(text[~fin] == -1) and np.all(text[:, :, 16:] == -1)
    assert np.all(span[..., 1] <= np.array(SERVING_SEQ)[:, None])
    for p, (cls, opt) in enumerate(pats):                                # every label from its class
        for i, (c, o) in enumerate(zip(cls, opt)):
            got = text[:, p, i][fin[:, p]]
            assert np.all(np.isin(got, c + [-1] if o else c))
    optional = [text[:, p, i][fin[:, p]] for p, (_, opt) in enumerate(pats) for i, o in enumerate(opt) if o]
    assert any((t == -1).any() for t in optional) and any((t >= 0).any() for t in optional)   # left out, and taken


def test_two_calls_are_bitwise_equal(cuda):
    logits, pats, _want, first = _serving(cuda, "int")
    second = _field(cuda, logits, SERVING_SEQ, pats, WIDTH)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ LDS switch
def test_workspace_table_at_the_serving_shape(cuda, ocrk_opts):
    """CTC_LDS = 0 sends a shape that fits LDS down the route that gathers from the workspace table: the same
    expressions in the same order, so the same bits."""
    logits, pats, _want, lds = _serving(cuda, "gauss")
    ocrk_opts("CTC_LDS", 0)
    ws = _field(cuda, logits, SERVING_SEQ, pats, WIDTH)
    for a, b in zip(lds, ws):
        assert a.tobytes() == b.tobytes()


def test_table_too_large_for_lds(cuda):
    """T = 300: 300 x 96 x 4 B = 115 KB > the 112 KB budget, so the table stays in the workspace. The same
    logits cut to T = 290 (111 KB) with the same lengths take the LDS route: equal bytes, and the helper's."""
    rng = np.random.default_rng(13)
    logits = _logits(rng, "gauss", 300, 2, C)
    seq = [290, 201]
    pats = [_pattern(rng, n, C, sizes=(1, 2, 3)) for n in (1, 3, 4, 7, 16)] + [_serving_patterns(rng)[3]]
    ws = _field(cuda, logits, seq, pats)
    lds = _field(cuda, np.ascontiguousarray(logits[:290]), seq, pats)
    for a, b in zip(lds, ws):
        assert a.tobytes() == b.tobytes()
    _same(ws[:3], F.field_batch(logits, seq, pats))
    assert np.all(np.isfinite(ws[0]))


@pytest.mark.parametrize("lds", [1, 0])
def test_tail_frames_are_never_read(cuda, ocrk_opts, lds):
    logits, pats, _want, clean = _serving(cuda, "gauss")
    ocrk_opts("CTC_LDS", lds)
    dirty = logits.copy()
    for b, n in enumerate(SERVING_SEQ):
        dirty[n:, b] = np.nan
    got = _field(cuda, dirty, SERVING_SEQ, pats, WIDTH)
    for a, b in zip(clean, got):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------- against the existing kernel
def test_score_equals_the_spotter_over_the_language(cuda):
    """[1-9]\\d?\\.\\d: 990 strings through ocrk_ctc_spot, and their row-wise maximum, bytewise."""
    from cnn_lstm_ctc_ocr_amd import decode
    from cnn_lstm_ctc_ocr_amd import kernels as K
    fs = decode.FieldSet({"amount": r"[1-9]\d?\.\d"})
    (cls, opt), = fs.compiled
    strings = sorted(set(F.language(cls, opt)))
    assert len(strings) == 990
    logits = torch.from_numpy(_logits(np.random.default_rng(29), "gauss", 40, 2, C)).to(cuda)
    seq = torch.tensor([40, 23], dtype=torch.int32, device=cuda)
    lab = np.zeros((990, 4), np.int32)
    for i, s in enumerate(strings):
        lab[i, :len(s)] = s
    ln = torch.tensor([len(s) for s in strings], dtype=torch.int32, device=cuda)
    spot, _span, _status = K.ctc_spot(logits, seq, torch.from_numpy(lab).to(cuda), None, ln)
    score, span, text = decode.ctc_field_reader(logits, seq, fs)
    want = spot.max(dim=1).values.cpu().numpy()
    assert np.all(np.isfinite(want))
    assert score.cpu().numpy().tobytes() == want.reshape(2, 1).tobytes()
    # the text is one of the maximising strings
    spot = spot.cpu().numpy()
    for b, got in enumerate(text.cpu().numpy()[:, 0]):
        assert spot[b, strings.index(tuple(int(l) for l in got if l >= 0))] == want[b]


# --------------------------------------------------------------- planted lines
def _planted(line, T=30, first=3):
    """Logits [T, 1, C] whose argmax path reads `line` from frame `first` ('_' = blank), blank elsewhere: the
    construction of tests/test_gpu_ctc_spot.py."""
    from cnn_lstm_ctc_ocr_amd.mjsynth import out_charset
    assert len(out_charset) == C - 1
    rng = np.random.default_rng(17)
    logits = rng.random((T, 1, C)).astype(np.float32)
    path = [C - 1] * T
    for j, ch in enumerate(line):
        path[first + j] = C - 1 if ch == "_" else out_charset.index(ch)
    logits[np.arange(T), 0, path] = 5.0
    return logits


def test_planted_lines(cuda):
    from cnn_lstm_ctc_ocr_amd import decode
    lines = ["TOTAL_$1_12..50", "a12.5", "1_2_3_4_5.67"]
    logits = np.concatenate([_planted(l) for l in lines], axis=1)
    fs = decode.FieldSet({"amount": r"[1-9]\d{0,3}\.\d\d?"})
    seq = torch.full((3,), 30, dtype=torch.int32, device=cuda)
    score, span, text = [o.cpu().numpy() for o in decode.ctc_field_reader(torch.from_numpy(logits).to(cuda), seq, fs)]
    assert score.tobytes() == np.zeros((3, 1), np.float32).tobytes()     # exactly 0.0: on the argmax path
    assert fs.strings(text) == [["112.50"], ["12.5"], ["2345.67"]]
    assert span.tolist() == [[[10, 18]], [[4, 8]], [[5, 15]]]
    _same((score, span, text), F.field_batch(logits, [30] * 3, fs.compiled))


# ------------------------------------------------------------ invalid patterns
def test_invalid_patterns(cuda):
    """Bad lengths, structures and classes: pat_status 2 / 3, -inf, (-1, -1) and -1s on every row, the status
    word's two bits, and the valid patterns of the same call untouched."""
    from cnn_lstm_ctc_ocr_amd import _lib
    from cnn_lstm_ctc_ocr_amd import kernels as K
    K.status_word(cuda).zero_()
    rng = np.random.default_rng(19)
    T, B, W = 40, 3, 18
    seq = [40, 21, 6]
    good = [_pattern(rng, n, C) for n in (3, 1, 16, 9, 6)]
    logits = _logits(rng, "gauss", T, B, C)
    cls, opt, ln = _dense(good, W)
    # patterns 5..14: length 0; length 17; an optional position 0; four optionals in a row; the blank as a label;
    # a label -5; an unsorted class; a duplicate; an empty class; a label after the padding
    bad_cls = np.full((10, W, 16), -1, np.int32)
    bad_cls[:, :6, 0] = [1, 2, 3, 4, 5, 6]
    bad_opt = np.zeros((10, W), np.int32)
    bad_ln = [0, 17, 3, 6, 3, 3, 3, 3, 3, 3]
    bad_opt[2, 0] = 1
    bad_opt[3, 1:5] = 1
    bad_cls[4, 1, 1] = C - 1
    bad_cls[5, 2, 0] = -5
    bad_cls[6, 1, :3] = [7, 9, 8]
    bad_cls[7, 0, :3] = [7, 8, 8]
    bad_cls[8, 2, 0] = -1
    bad_cls[9, 1, :4] = [7, -1, 9, -1]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(cuda)
    lg, sq = torch.from_numpy(logits).to(cuda), dev(seq)
    score, span, text, status = [o.cpu().numpy() for o in K.ctc_field(
        lg, sq, dev(np.concatenate([cls, bad_cls])), dev(np.concatenate([opt, bad_opt])),
        dev(np.concatenate([ln, bad_ln])))]
    assert K.read_status(cuda, reset=False) == _lib.STATUS_CTC_BAD_LENGTH | _lib.STATUS_CTC_BAD_LABEL
    assert status.tolist() == [0] * 5 + [2, 2, 2, 2, 3, 3, 3, 3, 3, 3]
    assert np.all(np.isneginf(score[:, 5:])) and np.all(span[:, 5:] == -1) and np.all(text[:, 5:] == -1)
    only_good = [o.cpu().numpy() for o in K.ctc_field(lg, sq, dev(cls), dev(opt), dev(ln))]
    assert only_good[0].tobytes() == np.ascontiguousarray(score[:, :5]).tobytes()
    assert only_good[1].tobytes() == np.ascontiguousarray(span[:, :5]).tobytes()
    assert only_good[2].tobytes() == np.ascontiguousarray(text[:, :5]).tobytes()
    _same(only_good[:3], F.field_batch(logits, seq, good, W))
    assert np.all(np.isfinite(score[0, :5]))
    K.clear_status(cuda, _lib.STATUS_CTC_BAD_LENGTH | _lib.STATUS_CTC_BAD_LABEL)
    assert K.read_status(cuda) == 0


# --------------------------------------------------------------- bad arguments
def test_bad_arguments_launch_nothing(cuda):
    from cnn_lstm_ctc_ocr_amd import _lib
    from cnn_lstm_ctc_ocr_amd import kernels as K
    logits = torch.zeros(4, 2, C, device=cuda)
    seq = torch.full((2,), 4, dtype=torch.int32, device=cuda)
    cls = torch.full((3, 2, 16), -1, dtype=torch.int32, device=cuda)
    cls[:, :, 0] = 0
    opt = torch.zeros(3, 2, dtype=torch.int32, device=cuda)
    ln = torch.ones(3, dtype=torch.int32, device=cuda)
    with pytest.raises(TypeError):
        K.ctc_field(logits.bfloat16(), seq, cls, opt, ln)
    with pytest.raises(TypeError):
        K.ctc_field(logits, seq, cls.long(), opt, ln)
    with pytest.raises(TypeError):
        K.ctc_field(logits, seq, cls, opt.long(), ln)
    with pytest.raises(ValueError):
        K.ctc_field(logits, seq, cls[:, :, :8].contiguous(), opt, ln)
    with pytest.raises(ValueError):
        K.ctc_field(logits, seq, cls, opt[:, :1].contiguous(), ln)
    with pytest.raises(ValueError):
        K.ctc_field(logits, seq, cls, opt, ln[:2])
    with pytest.raises(_lib.InvalidArgumentError, match="max_pat_len=256"):
        K.ctc_field(logits, seq, torch.zeros(3, 256, 16, dtype=torch.int32, device=cuda),
                    torch.zeros(3, 256, dtype=torch.int32, device=cuda), ln)
    with pytest.raises(_lib.InvalidArgumentError, match="C=1"):
        K.ctc_field(torch.zeros(4, 2, 1, device=cuda), seq, cls, opt, ln)
    with pytest.raises(_lib.InvalidArgumentError, match="T=4097"):
        K.ctc_field(torch.zeros(4097, 1, 2, device=cuda), seq[:1].contiguous(), cls, opt, ln)
    # a short workspace: the error comes back and the outputs keep their bytes
    score = torch.full((2, 3), 7.0, device=cuda)
    span = torch.full((2, 3, 2), 7, dtype=torch.int32, device=cuda)
    text = torch.full((2, 3, 2), 7, dtype=torch.int32, device=cuda)
    nb = _lib.lib().ocrk_ctc_field_workspace_size(4, 2, C, 3, 2)
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
    args = [_lib.ptr(logits), _lib.ptr(seq), 4, 2, C, _lib.ptr(cls), _lib.ptr(opt), _lib.ptr(ln), 3, 2,
            _lib.ptr(score), _lib.ptr(span), _lib.ptr(text), None, None, _lib.ptr(ws), nb - 16, _lib.stream_ptr(cuda)]
    with pytest.raises(_lib.InvalidArgumentError, match="workspace too small"):
        _lib.call("ocrk_ctc_field", *args)
    torch.cuda.synchronize()
    assert bool((score == 7).all()) and bool((span == 7).all()) and bool((text == 7).all())
    args[16] = nb                                                        # and with the workspace it asks for, it runs
    _lib.call("ocrk_ctc_field", *args)
    assert bool((score == 0).all()) and span.tolist() == [[[0, 4]] * 3] * 2     # all ties: the hit extends
    assert text.tolist() == [[[0, -1]] * 3] * 2


# ---------------------------------------------------------------- the service
SIZES = (64, 64)
E2E_FIELDS = {"amount": r"[1-9]\d{0,3}\.\d{1,2}", "gst": r"\d\.\d\d", "word": "[a-p]{2,5}", "no": r"#\d{14}",
              "x": "x", "long": "y{16}"}
E2E_KEYWORDS = ["TOTAL", "gst", "a"]


@pytest.fixture(scope="module")
def service(cuda):
    """The store of tests/test_gpu_ctc_spot.py, 32 x 64 and 32 x 256 crops in one batch, and the eager logits
    of the batch."""
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
def test_recognizer_with_fields(cuda, service, graphs):
    from cnn_lstm_ctc_ocr_amd import decode
    from cnn_lstm_ctc_ocr_amd import kernels as K
    from cnn_lstm_ctc_ocr_amd.server import FieldHit, FieldRecognition, KeywordRecognition, Recognition, Recognizer
    store, batch, widths, logits, seq = service
    K.status_word(cuda).zero_()
    assert seq.tolist() == [29, 125, 125, 29]
    fset = decode.FieldSet(E2E_FIELDS)
    names = list(E2E_FIELDS)
    score, span, text = [o.cpu().numpy() for o in decode.ctc_field_reader(logits, seq, fset)]
    strings = fset.strings(text)
    assert np.isneginf(score[0, 5]) and np.isfinite(score[1, 5])         # 16 y and the 15 blanks between do not fit 29 frames

    plain = Recognizer(store, graphs=graphs)(batch, widths)
    got = Recognizer(store, fields=E2E_FIELDS, field_threshold=-1e30, graphs=graphs)(batch, widths)
    assert len(got) == 4 and all(type(r) is FieldRecognition and r.detail is None and r.hits == () for r in got)
    assert [r.text for r in got] == plain
    for b, r in enumerate(got):
        ps = [p for p in range(len(names)) if np.isfinite(score[b, p])]
        ps.sort(key=lambda p: (-score[b, p], p))
        assert [h.name for h in r.fields] == [names[p] for p in ps]
        for h, p in zip(r.fields, ps):
            assert type(h) is FieldHit and all(type(v) in (str, float, int) for v in h)
            assert h.text == strings[b][p] and len(h.text) >= 1
            assert np.float32(h.score).tobytes() == score[b, p].tobytes()
            assert (h.first_frame, h.end_frame) == tuple(span[b, p].tolist())
            assert (h.x0, h.x1) == decode.frames_to_px(h.first_frame, h.end_frame, widths[b])
            assert 0 <= h.x0 < h.x1 <= widths[b]
    # a higher threshold: the subset at or above it, in the same order; with keywords and detail it carries both
    thr = float(np.median(score[np.isfinite(score)]))
    both = Recognizer(store, fields=fset, field_threshold=thr, keywords=E2E_KEYWORDS, keyword_threshold=-1e30,
                      graphs=graphs, detail=True)(batch, widths)
    kw = Recognizer(store, keywords=E2E_KEYWORDS, keyword_threshold=-1e30, graphs=graphs, detail=True)(batch, widths)
    assert 0 < sum(len(r.fields) for r in both) < sum(len(r.fields) for r in got)
    for r, full, k in zip(both, got, kw):
        assert type(r) is FieldRecognition and type(k) is KeywordRecognition
        assert r.fields == tuple(h for h in full.fields if h.score >= thr)
        assert type(r.detail) is Recognition and r.detail == k.detail and r.text == k.text == full.text
        assert r.hits == k.hits and len(r.hits) >= 1
    assert K.read_status(cuda) == 0


def test_field_reader_makes_no_host_sync(cuda, service):
    from cnn_lstm_ctc_ocr_amd import decode
    store, batch, widths, logits, seq = service
    fset = decode.FieldSet(E2E_FIELDS)
    decode.ctc_field_reader(logits, seq, fset)                           # uploads the patterns' tensors
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        score, span, text = decode.ctc_field_reader(logits, seq, fset)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(score.shape) == (4, 6) and score.dtype == torch.float32
    assert tuple(span.shape) == (4, 6, 2) and span.dtype == torch.int32
    assert tuple(text.shape) == (4, 6, 16) and text.dtype == torch.int32
