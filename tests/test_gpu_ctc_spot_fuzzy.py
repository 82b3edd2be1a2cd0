"""ocrk_ctc_spot_fuzzy (the best path inside every row that spells every keyword
with at most its budget of edits) against tests/ctc_spot_fuzzy_ref.py -- scores
bytewise, spans and error counts exactly -- against the exact spotter where the
two must agree, and the keyword_errors switch of the serving Recognizer."""
import numpy as np
import pytest
import torch

import ctc_spot_fuzzy_ref as R
from oracle import ref_model as M

pytestmark = pytest.mark.gpu

C = 96
INF = float("inf")


def _dense(rows, width, fill):
    d = np.full((len(rows), width), fill, np.int32)
    for i, w in enumerate(rows):
        d[i, :len(w)] = w
    return d


def _tensors(cuda, kws, alts, width):
    dev = lambda a: torch.from_numpy(a).to(cuda)
    width = max(len(k) for k in kws) if width is None else width
    alt = None if alts is None else dev(_dense([a if a is not None else [-1] * len(k) for k, a in zip(kws, alts)],
                                               width, -1))
    return dev(_dense(kws, width, 0)), alt, dev(np.array([len(k) for k in kws], np.int32))


def _fuzzy(cuda, logits, seq, kws, alts, errs, cost, width=None):
    """(score f32 [B, K], span i32 [B, K, 2], errors i32 [B, K], kw_status i32 [K]) of the device as NumPy arrays."""
    from cnn_lstm_ctc_ocr_amd import kernels as K
    lab, alt, ln = _tensors(cuda, kws, alts, width)
    out = K.ctc_spot_fuzzy(torch.from_numpy(logits).to(cuda), torch.from_numpy(np.asarray(seq, np.int32)).to(cuda),
                           lab, alt, ln, torch.from_numpy(np.asarray(errs, np.int32)).to(cuda), cost)
    return [o.cpu().numpy() for o in out]


def _exact(cuda, logits, seq, kws, alts, width=None):
    from cnn_lstm_ctc_ocr_amd import kernels as K
    lab, alt, ln = _tensors(cuda, kws, alts, width)
    out = K.ctc_spot(torch.from_numpy(logits).to(cuda), torch.from_numpy(np.asarray(seq, np.int32)).to(cuda),
                     lab, alt, ln)
    return [o.cpu().numpy() for o in out]


def _same(got, want):
    """Scores bit for bit, spans and error counts exactly."""
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    for g, w in zip(got, want):
        assert g.shape == w.shape
    np.testing.assert_array_equal(got[0].view(np.uint32), np.ascontiguousarray(want[0], np.float32).view(np.uint32))
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])


def _keyword(rng, n, C, repeats=0):
    """n classes, none equal to either of the two before it, then `repeats` adjacent repeats from the front."""
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
    neighbour's label on purpose."""
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


def _budgets(kws, cycle):
    """Budgets from `cycle`, cut to what each keyword takes: adjacent keywords (a wave's pair) differ."""
    return [min(cycle[j % len(cycle)], R.max_budget(len(k))) for j, k in enumerate(kws)]


# ------------------------------------------------------------ small, tie-heavy
SMALL_T, SMALL_C = 12, 5
SMALL_SEQ = [12, 3, 0, 1, 12]                                # 3: below the workspace route's four-step read-ahead
SMALL_LENS = [5, 1, 2, 16, 17, 32, 3, 4, 2, 6, 7, 3, 9, 10, 4, 12, 3]


def _small_case(n_kw, with_alts):
    rng = np.random.default_rng(5)
    logits = (np.maximum(rng.integers(-3, 4, (SMALL_T, len(SMALL_SEQ), SMALL_C)), 0) / 4).astype(np.float32)
    kws = [_keyword(rng, n, SMALL_C, repeats=(j % 5 == 4)) for j, n in enumerate(SMALL_LENS)]
    kws[8] = [2, 2]
    kws = kws[:n_kw]
    return logits, kws, _alternatives(rng, kws, SMALL_C) if with_alts else None, _budgets(kws, (2, 1, 0, 2, 1))


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("cost", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("with_alts", [False, True])
@pytest.mark.parametrize("n_kw", [1, 17])
def test_small_and_tie_heavy(cuda, ocrk_opts, n_kw, with_alts, cost, lds):
    from cnn_lstm_ctc_ocr_amd import kernels as K
    K.status_word(cuda).zero_()
    ocrk_opts("CTC_LDS", lds)
    logits, kws, alts, errs = _small_case(n_kw, with_alts)
    if n_kw == 17:
        assert sorted(set(errs)) == [0, 1, 2] and any(a != b for a, b in zip(errs[0::2], errs[1::2]))
    score, span, errors, status = _fuzzy(cuda, logits, SMALL_SEQ, kws, alts, errs, cost)
    _same((score, span, errors), R.spot_batch(logits, SMALL_SEQ, kws, alts, errs, cost))
    assert status.tolist() == [0] * n_kw
    assert np.all(np.isneginf(score[2])) and np.all(span[2] == -1) and np.all(errors[2] == -1)
    fin = np.isfinite(score)
    assert fin[0].any() and np.all(errors[fin] >= 0) and np.all(errors[~fin] == -1)
    assert np.all(errors <= np.array(errs)[None, :])
    if n_kw == 17 and cost < 1:
        assert (errors == 1).any() and (errors == 2).any() and (errors == 0).any()
    assert K.read_status(cuda) == 0                          # no path is an ordinary result


# --------------------------------------------------------------- serving shape
SERVING_T, SERVING_B = 125, 64
WIDTH = 40                                                   # wider than every keyword
SERVING_LENS = [1, 2, 5, 9, 15, 16, 16, 17, 17, 32, 31, 6, 4]


def _serving_inputs():
    rng = np.random.default_rng(11)
    kws = [_keyword(rng, n, C) for n in SERVING_LENS]
    kws[3] = _keyword(rng, 9, C, repeats=2)
    alts = _alternatives(rng, kws, C)
    logits = np.maximum(rng.standard_normal((SERVING_T, SERVING_B, C)) * 3, 0).astype(np.float32)
    seq = [int(n) for n in rng.integers(1, SERVING_T + 1, SERVING_B)]
    seq[:6] = [125, 0, 3, 60, 33, 17]
    return logits, seq, kws, alts, _budgets(kws, (2, 0, 1, 2, 2, 1))


_cache = {}


def _serving(cuda, key):
    """The serving case's inputs and the device's answers, computed once: 'mixed' (budgets mixed, edit_cost
    0.25, with the helper's answer), 'b0' / 'b1' / 'b2' (every budget 0, at most 1, at most 2)."""
    if "inputs" not in _cache:
        _cache["inputs"] = _serving_inputs()
    logits, seq, kws, alts, errs = _cache["inputs"]
    if key not in _cache:
        if key == "mixed":
            _cache[key] = (_fuzzy(cuda, logits, seq, kws, alts, errs, 0.25, WIDTH),
                           R.spot_batch(logits, seq, kws, alts, errs, 0.25))
        else:
            cap = int(key[1])
            _cache[key] = _fuzzy(cuda, logits, seq, kws, alts, [min(cap, R.max_budget(len(k))) for k in kws], 0.25,
                                 WIDTH)
    return _cache[key]


def test_serving_shape(cuda):
    (score, span, errors, status), want = _serving(cuda, "mixed")
    logits, seq, kws, alts, errs = _cache["inputs"]
    assert sorted(set(errs)) == [0, 1, 2]
    _same((score, span, errors), want)
    assert status.tolist() == [0] * len(kws)
    fin = np.isfinite(score)
    assert fin[0].all() and not fin[1].any() and np.all(errors[~fin] == -1) and np.all(span[~fin] == -1)
    assert np.all(span[fin][:, 0] >= 0) and np.all(span[..., 1] <= np.array(seq)[:, None])
    assert (errors == 1).any() and (errors == 2).any()


def test_budget_zero_and_infinite_cost_are_the_exact_spotter(cuda):
    zero = _serving(cuda, "b0")
    logits, seq, kws, alts, errs = _cache["inputs"]
    exact = _exact(cuda, logits, seq, kws, alts, WIDTH)
    barred = _fuzzy(cuda, logits, seq, kws, alts, [R.max_budget(len(k)) for k in kws], INF, WIDTH)
    for got in (zero, barred):
        assert got[0].tobytes() == exact[0].tobytes() and got[1].tobytes() == exact[1].tobytes()
        np.testing.assert_array_equal(got[2], np.where(np.isfinite(exact[0]), 0, -1))
    assert np.isfinite(exact[0]).any() and np.isneginf(exact[0]).any()


def test_scores_grow_with_the_budget(cuda):
    s0, s1, s2 = (_serving(cuda, k)[0] for k in ("b0", "b1", "b2"))
    assert np.all(s2 >= s1) and np.all(s1 >= s0)
    assert (s1 > s0).any() and (s2 > s1).any()


def test_two_calls_are_bitwise_equal(cuda):
    first, _want = _serving(cuda, "mixed")
    logits, seq, kws, alts, errs = _cache["inputs"]
    second = _fuzzy(cuda, logits, seq, kws, alts, errs, 0.25, WIDTH)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


def test_workspace_table_at_the_serving_shape(cuda, ocrk_opts):
    """CTC_LDS = 0 sends a shape that fits LDS down the route that gathers from the workspace: the same
    expressions in the same order, so the same bits."""
    lds, _want = _serving(cuda, "mixed")
    logits, seq, kws, alts, errs = _cache["inputs"]
    ocrk_opts("CTC_LDS", 0)
    ws = _fuzzy(cuda, logits, seq, kws, alts, errs, 0.25, WIDTH)
    for a, b in zip(lds, ws):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("lds", [1, 0])
def test_tail_frames_are_never_read(cuda, ocrk_opts, lds):
    clean, _want = _serving(cuda, "mixed")
    logits, seq, kws, alts, errs = _cache["inputs"]
    ocrk_opts("CTC_LDS", lds)
    dirty = logits.copy()
    for b, n in enumerate(seq):
        dirty[n:, b] = np.nan
    got = _fuzzy(cuda, dirty, seq, kws, alts, errs, 0.25, WIDTH)
    for a, b in zip(clean, got):
        assert a.tobytes() == b.tobytes()


def test_table_too_large_for_lds(cuda):
    """T = 300: 300 x 96 x 4 B = 115 KB > the 112 KB budget, so the table stays in the workspace. The same
    logits cut to T = 280 (107.5 KB of table + 2.2 KB of (nb, a)) with the same lengths take the LDS route:
    equal bytes, and the helper's."""
    rng = np.random.default_rng(13)
    logits = np.maximum(rng.standard_normal((300, 2, C)) * 3, 0).astype(np.float32)
    seq = [280, 201]
    kws = [_keyword(rng, n, C) for n in (3, 8, 16, 17, 32)] + [_keyword(rng, 9, C, repeats=2)]
    alts = _alternatives(rng, kws, C)
    errs = _budgets(kws, (1, 2, 0, 2, 1, 2))
    ws = _fuzzy(cuda, logits, seq, kws, alts, errs, 0.5)
    lds = _fuzzy(cuda, np.ascontiguousarray(logits[:280]), seq, kws, alts, errs, 0.5)
    for a, b in zip(lds, ws):
        assert a.tobytes() == b.tobytes()
    _same(ws[:3], R.spot_batch(logits, seq, kws, alts, errs, 0.5))
    whole = _fuzzy(cuda, logits, [300, 4000], kws, alts, errs, 0.5)      # every frame; seq_len clamps to T
    full = _fuzzy(cuda, logits, [300, 300], kws, alts, errs, 0.5)
    for a, b in zip(whole, full):
        assert a.tobytes() == b.tobytes()
    assert np.all(np.isfinite(whole[0])) and np.all(whole[1][..., 1] <= 300)


# ------------------------------------------------------------ planted keywords
def _planted(text, T=30, first=3):
    """Logits [T, 1, C] whose argmax path reads `text` from frame `first` ('.' = blank), blank elsewhere."""
    from cnn_lstm_ctc_ocr_amd.mjsynth import out_charset
    assert len(out_charset) == C - 1
    rng = np.random.default_rng(17)
    logits = rng.random((T, 1, C)).astype(np.float32)
    path = [C - 1] * T
    for j, ch in enumerate(text):
        path[first + j] = C - 1 if ch == "." else out_charset.index(ch)
    logits[np.arange(T), 0, path] = 5.0
    return logits


def test_planted_lines(cuda):
    from cnn_lstm_ctc_ocr_amd import decode
    lines = ["T0TAL", "TOTL", "TO-TAL", "TOTAL", "T0TA1"]
    logits = torch.from_numpy(np.concatenate([_planted(s) for s in lines], axis=1)).to(cuda)
    seq = torch.full((len(lines),), 30, dtype=torch.int32, device=cuda)
    score, span, errors = decode.ctc_fuzzy_keyword_spotter(logits, seq, decode.FuzzyKeywordSet(["TOTAL"], 1))
    score, span, errors = score.cpu().numpy()[:, 0], span.cpu().numpy()[:, 0], errors.cpu().numpy()[:, 0]
    exact, espan = decode.ctc_keyword_spotter(logits, seq, decode.KeywordSet(["TOTAL"]))
    exact, espan = exact.cpu().numpy()[:, 0], espan.cpu().numpy()[:, 0]
    zero = np.float32(0).tobytes()
    for b, text in enumerate(lines[:3]):                     # one edit away: found at no cost, where it was planted
        assert score[b].tobytes() == zero and errors[b] == 1 and span[b].tolist() == [3, 3 + len(text)]
        assert exact[b] < 0
    assert score[3].tobytes() == zero and errors[3] == 0 and span[3].tolist() == espan[3].tolist() == [3, 8]
    assert exact[3].tobytes() == zero
    assert score[4] < 0                                      # two edits away with a budget of one
    two = decode.ctc_fuzzy_keyword_spotter(logits, seq, decode.FuzzyKeywordSet(["TOTAL"], 2))
    assert two[0][4, 0].item() == 0 and two[2][4, 0].item() == 2 and two[1][4, 0].tolist() == [3, 8]
    # an edit costs what it is said to cost
    half = decode.ctc_fuzzy_keyword_spotter(logits, seq, decode.FuzzyKeywordSet(["TOTAL"], 1), edit_cost=0.5)
    assert half[0][:4, 0].tolist() == [-0.5, -0.5, -0.5, 0.0] and half[2][:4, 0].tolist() == [1, 1, 1, 0]


# ------------------------------------------------- invalid keywords and budgets
def test_invalid_keywords_and_budgets(cuda):
    """Bad lengths, labels, alternatives and budgets: kw_status 2 / 3, -inf, (-1, -1) and -1 on every row, the
    status word's two bits, and the valid keywords of the same call untouched."""
    from cnn_lstm_ctc_ocr_amd import _lib
    from cnn_lstm_ctc_ocr_amd import kernels as K
    K.status_word(cuda).zero_()
    rng = np.random.default_rng(19)
    T, B, W = 40, 3, 36
    seq = [40, 21, 6]
    good = [_keyword(rng, n, C) for n in (3, 1, 16, 17, 6)]
    good_alts = _alternatives(rng, good, C)
    good_errs = [2, 0, 1, 2, 1]
    logits = np.maximum(rng.standard_normal((T, B, C)) * 3, 0).astype(np.float32)
    lab = _dense(good, W, 0)
    alt = _dense([a if a is not None else [] for a in good_alts], W, -1)
    ln = [len(k) for k in good]
    # keywords 5..11: length 0, length 33, the blank as a label, an alternative C; then budgets 3, -1, and 2 for
    # a keyword of 2 symbols
    bad_lab = np.zeros((7, W), np.int32)
    bad_alt = np.full((7, W), -1, np.int32)
    bad_lab[:, :3] = [1, 2, 3]
    bad_lab[2, :3] = [1, C - 1, 3]
    bad_alt[3, 2] = C
    bad_len = [0, 33, 3, 3, 3, 3, 2]
    bad_err = [0, 0, 1, 1, 3, -1, 2]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(cuda)
    lg, sq = torch.from_numpy(logits).to(cuda), dev(seq)
    score, span, errors, status = [o.cpu().numpy() for o in K.ctc_spot_fuzzy(
        lg, sq, dev(np.concatenate([lab, bad_lab])), dev(np.concatenate([alt, bad_alt])), dev(ln + bad_len),
        dev(good_errs + bad_err), 0.25)]
    assert K.read_status(cuda, reset=False) == _lib.STATUS_CTC_BAD_LENGTH | _lib.STATUS_CTC_BAD_LABEL
    assert status.tolist() == [0] * 5 + [2, 2, 3, 3, 2, 2, 2]
    assert np.all(np.isneginf(score[:, 5:])) and np.all(span[:, 5:] == -1) and np.all(errors[:, 5:] == -1)
    only_good = [o.cpu().numpy() for o in K.ctc_spot_fuzzy(lg, sq, dev(lab), dev(alt), dev(ln), dev(good_errs), 0.25)]
    for got, whole in zip(only_good, (score, span, errors)):
        assert got.tobytes() == np.ascontiguousarray(whole[:, :5]).tobytes()
    _same(only_good[:3], R.spot_batch(logits, seq, good, good_alts, good_errs, 0.25))
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
    err = torch.zeros(3, dtype=torch.int32, device=cuda)
    with pytest.raises(TypeError):
        K.ctc_spot_fuzzy(logits.bfloat16(), seq, lab, None, ln, err)
    with pytest.raises(TypeError):
        K.ctc_spot_fuzzy(logits, seq, lab, None, ln, err.long())
    with pytest.raises(ValueError):
        K.ctc_spot_fuzzy(logits, seq, lab, None, ln, err[:2])
    with pytest.raises(ValueError):
        K.ctc_spot_fuzzy(logits, seq, lab, lab[:, :1].contiguous(), ln, err)
    with pytest.raises(_lib.InvalidArgumentError, match="max_kw_len=256"):
        K.ctc_spot_fuzzy(logits, seq, torch.zeros(3, 256, dtype=torch.int32, device=cuda), None, ln, err)
    # a negative or NaN cost, a short workspace: the error comes back and the outputs keep their bytes
    score = torch.full((2, 3), 7.0, device=cuda)
    span = torch.full((2, 3, 2), 7, dtype=torch.int32, device=cuda)
    errors = torch.full((2, 3), 7, dtype=torch.int32, device=cuda)
    nb = _lib.lib().ocrk_ctc_spot_fuzzy_workspace_size(4, 2, C, 3, 2)
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda)

    def args(cost=0.0, ws_bytes=nb):
        return [_lib.ptr(logits), _lib.ptr(seq), 4, 2, C, _lib.ptr(lab), None, _lib.ptr(ln), _lib.ptr(err), 3, 2,
                cost, _lib.ptr(score), _lib.ptr(span), _lib.ptr(errors), None, None, _lib.ptr(ws), ws_bytes,
                _lib.stream_ptr(cuda)]

    for bad, match in ((args(cost=-1.0), "edit_cost"), (args(cost=float("nan")), "edit_cost"),
                       (args(ws_bytes=nb - 16), "workspace too small")):
        with pytest.raises(_lib.InvalidArgumentError, match=match):
            _lib.call("ocrk_ctc_spot_fuzzy", *bad)
    torch.cuda.synchronize()
    assert bool((score == 7).all()) and bool((span == 7).all()) and bool((errors == 7).all())
    _lib.call("ocrk_ctc_spot_fuzzy", *args())                # and with what it asks for, it runs
    assert bool((score == 0).all()) and span[:, :, 1].tolist() == [[1] * 3] * 2 and bool((errors == 0).all())


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
def test_recognizer_with_keyword_errors(cuda, service, graphs):
    from cnn_lstm_ctc_ocr_amd import decode
    from cnn_lstm_ctc_ocr_amd import kernels as K
    from cnn_lstm_ctc_ocr_amd.server import FuzzyKeywordHit, KeywordHit, KeywordRecognition, Recognizer
    store, batch, widths, logits, seq = service
    K.status_word(cuda).zero_()
    kset = decode.FuzzyKeywordSet(E2E_KEYWORDS, "auto", case_insensitive=True)
    assert kset.errors.tolist() == [1, 0, 0, 2, 2, 0, 2, 1]
    score, span, errors = (o.cpu().numpy() for o in decode.ctc_fuzzy_keyword_spotter(logits, seq, kset, 0.5))

    plain = Recognizer(store, graphs=graphs)(batch, widths)
    got = Recognizer(store, keywords=E2E_KEYWORDS, keyword_errors="auto", keyword_edit_cost=0.5,
                     keyword_threshold=-1e30, case_insensitive=True, graphs=graphs)(batch, widths)
    assert len(got) == 4 and all(type(r) is KeywordRecognition and r.detail is None for r in got)
    assert [r.text for r in got] == plain
    assert sum(len(r.hits) for r in got) > 0
    for b, r in enumerate(got):
        ks = [k for k in range(len(E2E_KEYWORDS)) if np.isfinite(score[b, k])]
        ks.sort(key=lambda k: (-score[b, k], errors[b, k], k))
        assert [h.keyword for h in r.hits] == [E2E_KEYWORDS[k] for k in ks]
        for h, k in zip(r.hits, ks):
            assert type(h) is FuzzyKeywordHit and all(type(v) in (str, float, int) for v in h)
            assert np.float32(h.score).tobytes() == score[b, k].tobytes() and h.errors == errors[b, k]
            assert (h.first_frame, h.end_frame) == tuple(span[b, k].tolist())
            assert (h.x0, h.x1) == decode.frames_to_px(h.first_frame, h.end_frame, widths[b])
    # the same set passed as a FuzzyKeywordSet; and without the new arguments the old types
    again = Recognizer(store, keywords=kset, keyword_edit_cost=0.5, keyword_threshold=-1e30, graphs=graphs)(batch,
                                                                                                           widths)
    assert again == got
    old = Recognizer(store, keywords=E2E_KEYWORDS, keyword_threshold=-1e30, graphs=graphs)(batch, widths)
    assert all(type(h) is KeywordHit for r in old for h in r.hits)
    assert K.read_status(cuda) == 0


def test_fuzzy_spotter_makes_no_host_sync(cuda, service):
    from cnn_lstm_ctc_ocr_amd import decode
    store, batch, widths, logits, seq = service
    kset = decode.FuzzyKeywordSet(E2E_KEYWORDS, "auto", case_insensitive=True)
    decode.ctc_fuzzy_keyword_spotter(logits, seq, kset)      # uploads the keywords' tensors
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        score, span, errors = decode.ctc_fuzzy_keyword_spotter(logits, seq, kset, 0.25)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(score.shape) == (4, 8) and score.dtype == torch.float32
    assert tuple(span.shape) == (4, 8, 2) and span.dtype == torch.int32
    assert tuple(errors.shape) == (4, 8) and errors.dtype == torch.int32
