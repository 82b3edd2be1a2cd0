"""ocrk_ctc_keyed_field (for every row and keyed field the jointly best placement
of one of the field's keywords, then a gap, then a string matching its pattern)
against tests/ctc_keyed_ref.py -- all five outputs, the two scores bytewise --, on
both table routes, and the keyed_fields switch of the serving Recognizer."""
import numpy as np
import pytest
import torch

import ctc_field_ref as F
import ctc_keyed_ref as KR
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


def _dense_patterns(patterns, width):
    cls = np.full((len(patterns), width, 16), -1, np.int32)
    opt = np.zeros((len(patterns), width), np.int32)
    for p, (c, o) in enumerate(patterns):
        for i, labels in enumerate(c):
            cls[p, i, :len(labels)] = labels
        opt[p, :len(o)] = o
    return cls, opt, np.array([len(c) for c, _ in patterns], np.int32)


def _dense_keywords(keywords, alts):
    width = max(len(w) for w in keywords)
    lab = np.zeros((len(keywords), width), np.int32)
    alt = None if alts is None else np.full((len(keywords), width), -1, np.int32)
    for k, w in enumerate(keywords):
        lab[k, :len(w)] = w
        if alts is not None:
            alt[k, :len(w)] = alts[k]
    return lab, alt, np.array([len(w) for w in keywords], np.int32)


def _keyed(cuda, logits, seq, keywords, alts, groups, patterns, gap_cost, width=None):
    """(score, span, kw_index, kw_score, text, kw_status, pat_status) of the device, as NumPy arrays."""
    from cnn_lstm_ctc_ocr_amd import kernels as K
    width = max(len(c) for c, _ in patterns) if width is None else width
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    lab, alt, ln = _dense_keywords(keywords, alts)
    cls, opt, pln = _dense_patterns(patterns, width)
    out = K.ctc_keyed_field(dev(logits), dev(np.asarray(seq, np.int32)), dev(lab), dev(alt), dev(ln),
                            dev(np.asarray(groups, np.int32)), dev(cls), dev(opt), dev(pln), gap_cost)
    return [o.cpu().numpy() for o in out]


def _same(got, want):
    """(score, span, kw_index, kw_score, text): the scores bit for bit, the rest exactly."""
    dtypes = (np.float32, np.int32, np.int32, np.float32, np.int32)
    for g, w, dt in zip(got, want, dtypes):
        assert g.dtype == dt and g.shape == w.shape
        if dt is np.float32:
            np.testing.assert_array_equal(g.view(np.uint32), np.ascontiguousarray(w, np.float32).view(np.uint32))
        else:
            np.testing.assert_array_equal(g, w)


def _consistent(got, seq):
    """What the definition promises of every result, whatever the logits."""
    score, span, kw_index, kw_score, text = got[:5]
    fin = np.isfinite(score)
    assert np.all(score[fin] <= 0) and np.all(kw_score[fin] <= 0) and np.all(score[fin] <= kw_score[fin])
    s = span[fin]
    L = np.broadcast_to(np.asarray(seq)[:, None], score.shape)[fin]
    assert np.all((0 <= s[:, 0]) & (s[:, 0] < s[:, 1]) & (s[:, 1] <= s[:, 2]) & (s[:, 2] < s[:, 3]) & (s[:, 3] <= L))
    assert np.all(kw_index[fin] >= 0)
    assert np.all(np.isneginf(score[~fin])) and np.all(span[~fin] == -1) and np.all(kw_index[~fin] == -1)
    assert np.all(np.isneginf(kw_score[~fin])) and np.all(text[~fin] == -1)


def _words(rng, C, lens):
    return [[int(l) for l in rng.integers(0, C - 1, n)] for n in lens]


def _alts(rng, C, keywords):
    """Per position an alternative label or -1 (sometimes the label itself, sometimes its neighbour's)."""
    return [[int(rng.integers(0, C - 1)) if rng.random() < 0.5 else -1 for _ in w] for w in keywords]


def _pattern(rng, n, C, sizes=(1, 1, 1, 2, 3, 5, 10, 16), p_opt=0.35):
    cls = [sorted(int(l) for l in rng.choice(C - 1, int(rng.choice(sizes)), replace=False)) for _ in range(n)]
    opt, run = [], 0
    for i in range(n):
        o = int(i > 0 and run < 3 and rng.random() < p_opt)
        run = run + 1 if o else 0
        opt.append(o)
    return cls, opt


# ------------------------------------------------------------ small, tie-heavy
SMALL_SEQ = [0, 1, 7, 12]
SMALL_GROUP_SIZES = [1, 2, 5, 1, 2, 5, 2, 1]                              # one group per pattern of SMALL_PATTERNS


@pytest.mark.parametrize("gap_cost", [0.0, 0.01])
@pytest.mark.parametrize("with_alts", [False, True])
@pytest.mark.parametrize("kind", ["gauss", "int"])
def test_small_and_tie_heavy(cuda, kind, with_alts, gap_cost):
    from cnn_lstm_ctc_ocr_amd import kernels as K
    K.status_word(cuda).zero_()
    rng = np.random.default_rng(5)
    logits = _logits(rng, kind, 12, 4, 5)
    groups = [a for a, n in enumerate(SMALL_GROUP_SIZES) for _ in range(n)]
    keywords = _words(rng, 5, rng.integers(1, 5, len(groups)))
    alts = _alts(rng, 5, keywords) if with_alts else None
    got = _keyed(cuda, logits, SMALL_SEQ, keywords, alts, groups, F.SMALL_PATTERNS, gap_cost)
    _same(got[:5], KR.keyed_batch(logits, SMALL_SEQ, keywords, alts, groups, F.SMALL_PATTERNS, gap_cost))
    _consistent(got, SMALL_SEQ)
    assert got[5].tolist() == [0] * len(keywords) and got[6].tolist() == [0] * len(F.SMALL_PATTERNS)
    assert np.all(np.isneginf(got[0][:2]))                               # no frames; one frame: no room for both
    assert np.isfinite(got[0][3]).sum() >= 6 and np.isfinite(got[0][2]).any()
    assert K.read_status(cuda) == 0


# ------------------------------------------------------------------ the limits
def _distinct(rng, n, C):
    """n labels, none equal to either of the two before it: the keyword needs exactly n frames."""
    lab = [int(rng.integers(0, C - 1))]
    while len(lab) < n:
        c = int(rng.integers(0, C - 1))
        if c not in lab[-2:]:
            lab.append(c)
    return lab


def test_the_limits(cuda):
    """A 32-symbol keyword beside a 16-symbol one (a wave that takes its two keywords one after the other) and
    pairs of short ones (a wave that takes both at once); waves whose longest pattern has 16, 8 and 4 positions
    (the three unrollings); three optional positions in a row and trailing optionals."""
    rng = np.random.default_rng(7)
    T, seq = 80, [80, 40]
    logits = _logits(rng, "gauss", T, 2, C)
    lens = [[16, 3, 5, 7], [8, 2, 6, 1], [4, 3, 1, 2]]                   # per wave of four 16-lane rows
    patterns = [_pattern(rng, n, C) for wave in lens for n in wave]
    patterns[3] = ([[3], [4, 5], [5, 6], [4, 7], [8], [9, 10], [3, 9]], [0, 1, 1, 1, 0, 1, 1])
    patterns[0] = ([[l] for l in _distinct(rng, 16, C)], [0] * 16)       # needs 16 frames
    keywords = [_distinct(rng, 32, C), _distinct(rng, 16, C), _distinct(rng, 16, C), _distinct(rng, 5, C)]
    groups = [0, 0, 1, 1]
    for a in range(2, 12):
        n = int(rng.integers(1, 4))
        keywords += _words(rng, C, rng.integers(1, 9, n))
        groups += [a] * n
    assert len(keywords) > 16                                            # more than one chunk of keywords
    for gap_cost in (0.0, 0.02):
        got = _keyed(cuda, logits, seq, keywords, None, groups, patterns, gap_cost)
        _same(got[:5], KR.keyed_batch(logits, seq, keywords, None, groups, patterns, gap_cost))
        _consistent(got, seq)
        assert np.all(np.isfinite(got[0][0])) and np.isfinite(got[0][1, 0])
        assert got[2][1, 0] == 1                                         # 32 + 16 frames do not fit the 40 of row 1
    alts = _alts(rng, C, keywords)
    got = _keyed(cuda, logits, seq, keywords, alts, groups, patterns, 0.02)
    _same(got[:5], KR.keyed_batch(logits, seq, keywords, alts, groups, patterns, 0.02))


# --------------------------------------------------------------- serving shape
SERVING_SEQ = [125, 60]
SERVING_COST = 0.02
WIDTH = 9                                                                # wider than every pattern


def _serving_fields(rng):
    patterns = [([DIGITS[1:]] + [DIGITS] * 3 + [[DOT]] + [DIGITS] * 2, [0, 1, 1, 1, 0, 0, 1]),     # an amount
                ([DIGITS, [DOT], DIGITS, DIGITS], [0, 0, 0, 0]),
                _pattern(rng, 5, C)]
    keywords = _words(rng, C, [5, 6, 3, 3, 7, 9, 2])
    return keywords, [0, 0, 0, 1, 1, 2, 2], patterns


_cache = {}


def _serving(cuda):
    """The case's inputs, the helper's answer and the device's, computed once."""
    if not _cache:
        rng = np.random.default_rng(11)
        keywords, groups, patterns = _serving_fields(rng)
        logits = _logits(rng, "gauss", 125, 2, C)
        _cache["x"] = (logits, keywords, groups, patterns,
                       KR.keyed_batch(logits, SERVING_SEQ, keywords, None, groups, patterns, SERVING_COST, WIDTH),
                       _keyed(cuda, logits, SERVING_SEQ, keywords, None, groups, patterns, SERVING_COST, WIDTH))
    return _cache["x"]


def test_serving_shape(cuda):
    logits, keywords, groups, patterns, want, got = _serving(cuda)
    _same(got[:5], want)
    _consistent(got, SERVING_SEQ)
    assert np.all(np.isfinite(got[0])) and np.all(got[4][:, :, 7:] == -1)
    assert np.all(np.asarray(groups)[got[2]] == np.arange(3)[None, :])   # every keyword from its field's group


def test_two_calls_are_bitwise_equal(cuda):
    logits, keywords, groups, patterns, _want, first = _serving(cuda)
    second = _keyed(cuda, logits, SERVING_SEQ, keywords, None, groups, patterns, SERVING_COST, WIDTH)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ LDS switch
def test_workspace_table_at_the_serving_shape(cuda, ocrk_opts):
    """CTC_LDS = 0 sends a shape that fits LDS down the route that gathers the emissions and the entry values
    from the workspace: the same expressions in the same order, so the same bits."""
    logits, keywords, groups, patterns, _want, lds = _serving(cuda)
    ocrk_opts("CTC_LDS", 0)
    ws = _keyed(cuda, logits, SERVING_SEQ, keywords, None, groups, patterns, SERVING_COST, WIDTH)
    for a, b in zip(lds, ws):
        assert a.tobytes() == b.tobytes()


def test_table_too_large_for_lds(cuda):
    """T = 300: 300 x 96 x 4 B = 115 KB > the 112 KB budget, so both tables stay in the workspace. The same
    logits cut to T = 290 with the same lengths: the keyword trail takes the LDS route (111 KB), the field
    lattice (290 x 104 x 4 B = 121 KB with its entry values) still the workspace. Equal bytes, and the helper's."""
    rng = np.random.default_rng(13)
    logits = _logits(rng, "gauss", 300, 2, C)
    seq = [290, 201]
    keywords, groups, patterns = _serving_fields(rng)
    ws = _keyed(cuda, logits, seq, keywords, None, groups, patterns, 0.01)
    cut = _keyed(cuda, np.ascontiguousarray(logits[:290]), seq, keywords, None, groups, patterns, 0.01)
    for a, b in zip(cut, ws):
        assert a.tobytes() == b.tobytes()
    _same(ws[:5], KR.keyed_batch(logits, seq, keywords, None, groups, patterns, 0.01))
    assert np.all(np.isfinite(ws[0]))


@pytest.mark.parametrize("lds", [1, 0])
def test_tail_frames_are_never_read(cuda, ocrk_opts, lds):
    logits, keywords, groups, patterns, _want, clean = _serving(cuda)
    ocrk_opts("CTC_LDS", lds)
    dirty = logits.copy()
    for b, n in enumerate(SERVING_SEQ):
        dirty[n:, b] = np.nan
    got = _keyed(cuda, dirty, SERVING_SEQ, keywords, None, groups, patterns, SERVING_COST, WIDTH)
    for a, b in zip(clean, got):
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- planted line
def _planted(line, T=40, first=3):
    """Logits [T, 1, C] whose argmax path reads `line` from frame `first` ('_' = blank), blank elsewhere: the
    construction of tests/test_gpu_ctc_field.py. Returns the logits and the path."""
    from cnn_lstm_ctc_ocr_amd.mjsynth import out_charset
    assert len(out_charset) == C - 1
    rng = np.random.default_rng(17)
    logits = rng.random((T, 1, C)).astype(np.float32)
    path = [C - 1] * T
    for j, ch in enumerate(line):
        path[first + j] = C - 1 if ch == "_" else out_charset.index(ch)
    logits[np.arange(T), 0, path] = 5.0
    return logits, path


def test_planted_line(cuda):
    """TOTAL 12.50 CASH 20.00 with the 2 of 12.50 read slightly worse than another character: the field reader
    alone returns 20.00; the keyed fields return the amount after their own keyword."""
    from cnn_lstm_ctc_ocr_amd import decode
    from cnn_lstm_ctc_ocr_amd.mjsynth import out_charset
    amount = r"[1-9]\d{0,3}\.\d{1,2}"
    logits, _path = _planted("TOTAL_12.50_CASH_20.0_0")
    logits[10, 0, out_charset.index("Z")] = 5.25                         # frame 10 is the 2 of 12.50: 0.25 behind
    lg = torch.from_numpy(logits).to(cuda)
    seq = torch.full((1,), 40, dtype=torch.int32, device=cuda)
    fs = decode.FieldSet({"amount": amount})
    score, span, text = [o.cpu().numpy() for o in decode.ctc_field_reader(lg, seq, fs)]
    assert fs.strings(text) == [["20.00"]] and score[0, 0] == 0 and span[0, 0].tolist() == [20, 26]
    keyed = decode.KeyedFieldSet({"total": (["TOTAL", "AMOUNT"], amount), "cash": (["CASH"], amount)})
    patterns = list(keyed.compiled)
    words = [[out_charset.index(ch) for ch in w] for w in keyed.keywords]
    for cost, strings, spans, scores in [
            # one blank frame of gap after either keyword; total pays the weakened 2 as well
            (0.05, ["12.50", "20.00"], [[3, 8, 9, 14], [15, 19, 20, 26]],
             [np.float32(-0.05) + np.float32(-0.25), np.float32(-0.05)]),
            (0.0, ["20.00", "20.00"], [[3, 8, 20, 26], [15, 19, 20, 26]], [0.0, 0.0])]:
        got = [o.cpu().numpy() for o in decode.ctc_keyed_field_reader(lg, seq, keyed, gap_cost=cost)]
        score, kw_index, kw_score, span, text = got
        assert keyed.strings(text) == [strings] and span[0].tolist() == spans
        assert np.all(span[0, :, 1] <= span[0, :, 2])
        assert score[0].tobytes() == np.asarray(scores, np.float32).tobytes()
        assert kw_index[0].tolist() == [0, 2] and kw_score[0].tolist() == [0.0, 0.0]
        _same((score, span, kw_index, kw_score, text),
              KR.keyed_batch(logits, [40], words, None, keyed.groups.tolist(), patterns, cost))


# -------------------------------------------------------------- invalid entries
def test_invalid_entries(cuda):
    """Bad keyword lengths, labels, alternatives and groups, bad patterns: flagged, never scored, never indexed;
    a field left without a valid keyword or pattern gives -inf on every row; the others are untouched."""
    from cnn_lstm_ctc_ocr_amd import _lib
    from cnn_lstm_ctc_ocr_amd import kernels as K
    K.status_word(cuda).zero_()
    rng = np.random.default_rng(19)
    T, seq, n_key = 40, [40, 21, 6], 6
    logits = _logits(rng, "gauss", T, 3, C)
    # fields: 0 and 1 sound; 2 with an invalid pattern; 3 with only invalid keywords; 4 with no keyword at all;
    # 5 sound, with invalid keywords beside its valid one
    patterns = [_pattern(rng, n, C) for n in (3, 1, 2, 4, 2, 5)]
    good = _words(rng, C, [3, 2, 4, 1, 2, 3])
    keywords = good + _words(rng, C, [3] * 8)
    groups = [0, 0, 1, 2, 5, 5] + [3, 3, 5, 5, 5, 0, 1, 1]
    lab, _none, ln = _dense_keywords(keywords, None)
    alt = np.full(lab.shape, -1, np.int32)
    ln[6], ln[7] = 0, 33                                                 # field 3's two keywords: bad lengths
    lab[8, 1] = C - 1                                                    # the blank as a label
    lab[9, 0] = -5
    alt[10, 2] = C                                                       # an alternative out of range
    lab[11] = 1 << 30                                                    # never an index
    groups[12], groups[13] = -1, n_key                                   # a group out of range
    cls, opt, pln = _dense_patterns(patterns, 6)
    pln[2] = 0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(cuda)
    out = [o.cpu().numpy() for o in K.ctc_keyed_field(torch.from_numpy(logits).to(cuda), dev(seq), dev(lab), dev(alt),
                                                      dev(ln), dev(groups), dev(cls), dev(opt), dev(pln), 0.01)]
    assert K.read_status(cuda, reset=False) == _lib.STATUS_CTC_BAD_LENGTH | _lib.STATUS_CTC_BAD_LABEL
    assert out[5].tolist() == [0] * 6 + [2, 2, 3, 3, 3, 3, 3, 3] and out[6].tolist() == [0, 0, 2, 0, 0, 0]
    ref_kw = good + [None] * 8
    ref_alts = [[-1] * len(w) for w in keywords]
    want = KR.keyed_batch(logits, seq, ref_kw, ref_alts, groups, patterns[:2] + [None] + patterns[3:], 0.01, 6)
    _same(out[:5], want)
    _consistent(out, seq)
    assert np.all(np.isneginf(out[0][:, 2:5])) and np.all(np.isfinite(out[0][0, [0, 1, 5]]))
    K.clear_status(cuda, _lib.STATUS_CTC_BAD_LENGTH | _lib.STATUS_CTC_BAD_LABEL)
    assert K.read_status(cuda) == 0


# --------------------------------------------------------------- bad arguments
def test_bad_arguments_launch_nothing(cuda):
    from cnn_lstm_ctc_ocr_amd import _lib
    from cnn_lstm_ctc_ocr_amd import kernels as K
    logits = torch.zeros(4, 2, C, device=cuda)
    seq = torch.full((2,), 4, dtype=torch.int32, device=cuda)
    kw = torch.zeros(2, 1, dtype=torch.int32, device=cuda)
    kln = torch.ones(2, dtype=torch.int32, device=cuda)
    grp = torch.tensor([0, 1], dtype=torch.int32, device=cuda)
    cls = torch.full((2, 2, 16), -1, dtype=torch.int32, device=cuda)
    cls[:, :, 0] = 1
    opt = torch.zeros(2, 2, dtype=torch.int32, device=cuda)
    pln = torch.ones(2, dtype=torch.int32, device=cuda)
    for bad in (-1e-3, float("nan")):
        with pytest.raises(_lib.InvalidArgumentError, match="gap_cost"):
            K.ctc_keyed_field(logits, seq, kw, None, kln, grp, cls, opt, pln, bad)
    with pytest.raises(TypeError):
        K.ctc_keyed_field(logits.bfloat16(), seq, kw, None, kln, grp, cls, opt, pln)
    with pytest.raises(TypeError):
        K.ctc_keyed_field(logits, seq, kw, None, kln, grp.long(), cls, opt, pln)
    with pytest.raises(ValueError):
        K.ctc_keyed_field(logits, seq, kw, None, kln, grp[:1], cls, opt, pln)
    with pytest.raises(ValueError):
        K.ctc_keyed_field(logits, seq, kw, None, kln, grp, cls[:, :, :8].contiguous(), opt, pln)
    # a short workspace and a null pointer: the error comes back and the outputs keep their bytes
    score = torch.full((2, 2), 7.0, device=cuda)
    span = torch.full((2, 2, 4), 7, dtype=torch.int32, device=cuda)
    kwi = torch.full((2, 2), 7, dtype=torch.int32, device=cuda)
    kws = torch.full((2, 2), 7.0, device=cuda)
    text = torch.full((2, 2, 2), 7, dtype=torch.int32, device=cuda)
    nb = _lib.lib().ocrk_ctc_keyed_field_workspace_size(4, 2, C, 2, 1, 2, 2)
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
    p = _lib.ptr
    args = [p(logits), p(seq), 4, 2, C, p(kw), None, p(kln), p(grp), 2, 1, p(cls), p(opt), p(pln), 2, 2, 0.0,
            p(score), p(span), p(kwi), p(kws), p(text), None, None, None, p(ws), nb - 16, _lib.stream_ptr(cuda)]
    with pytest.raises(_lib.InvalidArgumentError, match="workspace too small"):
        _lib.call("ocrk_ctc_keyed_field", *args)
    args[26] = nb
    for i in (0, 1, 5, 7, 8, 11, 12, 13, 17, 18, 19, 20, 21, 25):
        with pytest.raises(_lib.InvalidArgumentError, match="null pointer"):
            _lib.call("ocrk_ctc_keyed_field", *(args[:i] + [None] + args[i + 1:]))
    torch.cuda.synchronize()
    for o in (score, span, kwi, kws, text):
        assert bool((o == 7).all())
    _lib.call("ocrk_ctc_keyed_field", *args)                             # and with what it asks for, it runs
    # all ties: keyword label 0 on frame 0, the value (label 1) from frame 1, extended to the row's end
    assert bool((score == 0).all()) and span.tolist() == [[[0, 1, 1, 4]] * 2] * 2
    assert kwi.tolist() == [[0, 1]] * 2 and bool((kws == 0).all()) and text.tolist() == [[[1, -1]] * 2] * 2


# ---------------------------------------------------------------- the service
SIZES = (64, 64)
E2E_KEYED = {"total": (["TOTAL", "ttl", "a"], r"[1-9]\d{0,3}\.\d{1,2}"), "gst": (["gst", "b"], r"\d\.\d\d"),
             "word": (["x", "No."], "[a-p]{2,5}"), "long": (["receipt"], "y{16}")}
E2E_FIELDS = {"amount": r"[1-9]\d{0,3}\.\d{1,2}", "x": "x"}
E2E_KEYWORDS = ["TOTAL", "gst", "a"]
E2E_COST = 0.01


@pytest.fixture(scope="module")
def service(cuda):
    """The store of tests/test_gpu_ctc_field.py, 32 x 64 and 32 x 256 crops in one batch, and the eager logits
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


@pytest.fixture(scope="module")
def helper_hits(service):
    """The helper's answer on the read-back logits, computed once for the eager and the graphed run."""
    from cnn_lstm_ctc_ocr_amd import decode
    from cnn_lstm_ctc_ocr_amd.mjsynth import out_charset
    _store, _batch, _widths, logits, seq = service
    keyed = decode.KeyedFieldSet(E2E_KEYED)
    words = [[out_charset.index(ch) for ch in w] for w in keyed.keywords]
    return keyed, KR.keyed_batch(logits.cpu().numpy(), seq.cpu().numpy(), words, None, keyed.groups.tolist(),
                                 list(keyed.compiled), E2E_COST)


@pytest.mark.parametrize("graphs", [False, True])
def test_recognizer_with_keyed_fields(cuda, service, helper_hits, graphs):
    from cnn_lstm_ctc_ocr_amd import decode
    from cnn_lstm_ctc_ocr_amd import kernels as K
    from cnn_lstm_ctc_ocr_amd.server import FieldRecognition, KeyedHit, KeyedRecognition, Recognition, Recognizer
    store, batch, widths, logits, seq = service
    K.status_word(cuda).zero_()
    assert seq.tolist() == [29, 125, 125, 29]
    keyed, (score, span, kw_index, kw_score, text) = helper_hits
    names = list(E2E_KEYED)
    strings = keyed.strings(text)
    assert np.isneginf(score[0, 3]) and np.isfinite(score[1, 3])         # 7 + 31 frames do not fit 29

    # without keyed_fields: what it returns today
    plain = Recognizer(store, graphs=graphs)(batch, widths)
    assert all(type(t) is str for t in plain)
    fields_only = Recognizer(store, fields=E2E_FIELDS, field_threshold=-1e30, keywords=E2E_KEYWORDS,
                             keyword_threshold=-1e30, detail=True, graphs=graphs)(batch, widths)
    assert all(type(r) is FieldRecognition for r in fields_only)

    got = Recognizer(store, keyed_fields=E2E_KEYED, keyed_threshold=-1e30, keyed_gap_cost=E2E_COST,
                     graphs=graphs)(batch, widths)
    assert len(got) == 4 and all(type(r) is KeyedRecognition and r.detail is None for r in got)
    assert all(r.hits == () and r.fields == () for r in got) and [r.text for r in got] == plain
    for b, r in enumerate(got):
        ps = [p for p in range(len(names)) if np.isfinite(score[b, p])]
        ps.sort(key=lambda p: (-score[b, p], p))
        assert [h.name for h in r.keyed] == [names[p] for p in ps] and len(ps) >= 3
        for h, p in zip(r.keyed, ps):
            assert type(h) is KeyedHit and all(type(v) in (str, float, int) for v in h)
            assert h.text == strings[b][p] and len(h.text) >= 1
            assert h.keyword == keyed.keywords[kw_index[b, p]] and h.keyword in E2E_KEYED[h.name][0]
            assert np.float32(h.score).tobytes() == score[b, p].tobytes()
            assert np.float32(h.keyword_score).tobytes() == kw_score[b, p].tobytes()
            assert (h.kw_first_frame, h.kw_end_frame, h.first_frame, h.end_frame) == tuple(span[b, p].tolist())
            assert (h.kw_x0, h.kw_x1) == decode.frames_to_px(h.kw_first_frame, h.kw_end_frame, widths[b])
            assert (h.x0, h.x1) == decode.frames_to_px(h.first_frame, h.end_frame, widths[b])
            assert 0 <= h.kw_x0 < h.kw_x1 <= h.x0 < h.x1 <= widths[b]
    # a higher threshold: the subset at or above it, in the same order; with fields, keywords and detail it
    # carries all three as they come without keyed_fields
    thr = float(np.median(score[np.isfinite(score)]))
    every = Recognizer(store, keyed_fields=keyed, keyed_threshold=thr, keyed_gap_cost=E2E_COST, fields=E2E_FIELDS,
                       field_threshold=-1e30, keywords=E2E_KEYWORDS, keyword_threshold=-1e30, detail=True,
                       graphs=graphs)(batch, widths)
    assert 0 < sum(len(r.keyed) for r in every) < sum(len(r.keyed) for r in got)
    for r, full, f in zip(every, got, fields_only):
        assert type(r) is KeyedRecognition and r.keyed == tuple(h for h in full.keyed if h.score >= thr)
        assert type(r.detail) is Recognition and r.detail == f.detail and r.text == f.text == full.text
        assert r.hits == f.hits and r.fields == f.fields and len(r.hits) >= 1 and len(r.fields) >= 1
    assert K.read_status(cuda) == 0


def test_keyed_reader_makes_no_host_sync(cuda, service):
    from cnn_lstm_ctc_ocr_amd import decode
    store, batch, widths, logits, seq = service
    keyed = decode.KeyedFieldSet(E2E_KEYED, case_insensitive=True)
    decode.ctc_keyed_field_reader(logits, seq, keyed, E2E_COST)           # uploads the tensors
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        score, kw_index, kw_score, span, text = decode.ctc_keyed_field_reader(logits, seq, keyed, E2E_COST)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(score.shape) == (4, 4) and score.dtype == torch.float32
    assert tuple(kw_index.shape) == (4, 4) and kw_index.dtype == torch.int32
    assert tuple(kw_score.shape) == (4, 4) and kw_score.dtype == torch.float32
    assert tuple(span.shape) == (4, 4, 4) and span.dtype == torch.int32
    assert tuple(text.shape) == (4, 4, 16) and text.dtype == torch.int32
