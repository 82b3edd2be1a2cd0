"""ocrk_ctc_lexicon_score (log p(word | logits) of a word list for every row,
the best words and the lexicon's normaliser) against the float64 oracle's
ctc_loss_single, and the lexicon switch of the serving Recognizer."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import shard_records
from oracle import ref_graph as G

pytestmark = pytest.mark.gpu

C = 96
RTOL = 1e-3                                  # the bound tests/test_gpu_ctc.py holds ocrk_ctc_loss to against this oracle
FIX = os.path.join(os.path.dirname(__file__), "golden", "mjsynth_test_bucket.npz")


def _logits(rng, kind, T, B, C):
    """The logits of tests/test_gpu_ctc_align.py: ReLU'd small integers (exact ties everywhere) or Gaussian."""
    if kind == "int":
        return np.maximum(rng.integers(-3, 4, (T, B, C)), 0).astype(np.float32)
    return np.maximum(rng.standard_normal((T, B, C)) * 3, 0).astype(np.float32)


def _words(rng, lens):
    return [[int(c) for c in rng.integers(0, C - 1, n)] for n in lens]


def _dense(words, width=None):
    width = max([len(w) for w in words] + [1]) if width is None else width
    d = np.zeros((len(words), width), np.int32)
    for i, w in enumerate(words):
        d[i, :len(w)] = w
    return d, np.array([len(w) for w in words], np.int32)


def _score(cuda, logits, seq, words, top_k=1, width=None, need_scores=True):
    """(logp, top_idx, top_logp, log_norm, word_status) as NumPy arrays."""
    from cnn_lstm_ctc_ocr_amd import kernels as K
    lab, ln = _dense(words, width)
    out = K.ctc_lexicon_score(torch.from_numpy(logits).to(cuda), torch.from_numpy(np.asarray(seq, np.int32)).to(cuda),
                              torch.from_numpy(lab).to(cuda), torch.from_numpy(ln).to(cuda), top_k, need_scores)
    return [None if o is None else o.cpu().numpy() for o in out]


def _oracle(logits, seq, words):
    """float64 ln p(word | logits[:L, b]) [B, K]; -inf where ctc_required_time says the word does not fit."""
    T, B, _ = logits.shape
    want = np.full((B, len(words)), -np.inf)
    for b in range(B):
        L = min(max(int(seq[b]), 0), T)
        for k, w in enumerate(words):
            if L > 0 and G.ctc_required_time(w) <= L:
                want[b, k] = -G.ctc_loss_single(logits[:L, b], w, blank=C - 1)[0]
    return want


def _ragged_words(rng):
    """63 words: 60 of random lengths 0..12, some with adjacent repeats (one with zero slack against the
    7-frame row, one against the 12-frame row), and lengths 31 / 32 / 33 (S = 63 / 65 / 67, around one register)."""
    words = _words(rng, rng.integers(0, 13, 60))
    words[0] = []                                           # the empty word: all blanks
    words[7] = [3, 3, 9, 1, 1]                              # needs 5 + 2 = 7 frames
    words[8] = [1, 1, 2, 2, 3, 3, 4, 4]                     # needs 8 + 4 = 12 frames
    words[9] = [5, 5, 5]
    for i in (20, 21, 22):                                  # a repeat inside a random word
        if len(words[i]) >= 2:
            words[i][1] = words[i][0]
    return words + _words(rng, [31, 32, 33])


RAGGED_SEQ = [40, 40, 33, 25, 12, 7, 1, 0]


def _case(name):
    """name -> (logits [T, B, C], seq_len, words, label tensor width or None)."""
    rng = np.random.default_rng(0)
    if name in ("ragged_gauss", "ragged_int"):
        # a seed at which the ORACLE's top-2 gap exceeds twice the score tolerance on every row (checked on the
        # CPU, asserted in test_best_word_is_the_oracles): ReLU'd logits tie often on the one-frame row
        rng = np.random.default_rng(2)
        words = _ragged_words(rng)
        return _logits(rng, name[7:], 40, 8, C), RAGGED_SEQ, words, None
    if name == "four_registers":                            # S = 141 and S = 7 in one call
        return _logits(rng, "gauss", 150, 2, C), [150, 97], _words(rng, [70, 3]), None
    if name == "eight_registers":                           # S = 401; T C floats do not fit LDS either
        return _logits(rng, "gauss", 512, 1, C), [512], _words(rng, [200]), None
    if name == "table_in_workspace":                        # 512 x 96 x 4 B = 196 KB > the CU's LDS
        return _logits(rng, "gauss", 512, 1, C), [500], _words(rng, rng.integers(0, 13, 20)), None
    if name == "wide_label_tensor":                         # max_word_len 130, short words only
        return _logits(rng, "int", 30, 3, C), [30, 17, 4], _words(rng, rng.integers(0, 10, 9)), 130
    if name == "one_word":
        return _logits(rng, "gauss", 20, 3, C), [20, 9, 2], _words(rng, [4]), None
    if name == "chunks":                                    # more than one chunk of words per row, the last ragged
        return _logits(rng, "gauss", 12, 2, C), [12, 5], _words(rng, rng.integers(0, 9, 1025)), None
    raise KeyError(name)


CASES = ["ragged_gauss", "ragged_int", "four_registers", "eight_registers", "table_in_workspace",
         "wide_label_tensor", "one_word", "chunks"]
_cache = {}


def _run(cuda, name):
    """The case's inputs, the oracle's scores and the device's outputs at top_k = 5, computed once."""
    if name not in _cache:
        logits, seq, words, width = _case(name)
        _cache[name] = (logits, seq, words, width, _oracle(logits, seq, words),
                        _score(cuda, logits, seq, words, 5, width))
    return _cache[name]


@pytest.mark.parametrize("name", CASES)
def test_scores_match_the_oracle(cuda, name):
    from cnn_lstm_ctc_ocr_amd import kernels as K
    K.status_word(cuda).zero_()
    logits, seq, words, width, want, (logp, top_idx, top_logp, log_norm, status) = _run(cuda, name)
    assert logp.shape == want.shape and logp.dtype == np.float32
    assert status.tolist() == [0] * len(words)
    np.testing.assert_array_equal(np.isneginf(logp), np.isneginf(want))   # -inf iff the oracle says infeasible
    assert not np.any(np.isnan(logp)) and not np.any(np.isposinf(logp))
    fin = np.isfinite(want)
    assert fin.any()
    err = np.abs(logp[fin] - want[fin]) / np.abs(want[fin])
    print(f"{name}: {fin.sum()} finite / {fin.size} pairs, max relative error {err.max():.3e}")
    np.testing.assert_allclose(logp[fin], want[fin], rtol=RTOL)
    # infeasibility is an ordinary result here: no status bit
    assert K.read_status(cuda) == 0


@pytest.mark.parametrize("kind", ["gauss", "int"])
def test_ragged_rows(cuda, kind):
    """The row without frames: all -inf, nothing selected, log_norm -inf; the zero-slack repeats are scored."""
    logits, seq, words, width, want, (logp, top_idx, top_logp, log_norm, status) = _run(cuda, "ragged_" + kind)
    assert logp.shape == (8, 63) and seq[7] == 0
    assert np.all(np.isneginf(logp[7])) and np.all(top_idx[7] == -1) and np.all(np.isneginf(top_logp[7]))
    assert np.isneginf(log_norm[7]) and np.all(np.isfinite(log_norm[:7]))
    assert G.ctc_required_time(words[7]) == seq[5] == 7 and np.isfinite(logp[5, 7])
    assert G.ctc_required_time(words[8]) == seq[4] == 12 and np.isfinite(logp[4, 8]) and np.isneginf(logp[5, 8])
    assert np.isfinite(logp[6, 0]) and np.all(np.isfinite(logp[0]))      # one frame: the empty word fits
    assert np.all(np.isneginf(logp[3:, 60:])) and np.all(np.isfinite(logp[:2, 60:]))


def _select(logp_row, top_k):
    """(logp descending, index ascending) over the finite scores, padded with -1 / -inf."""
    idx = np.lexsort((np.arange(len(logp_row)), -logp_row))
    idx = idx[np.isfinite(logp_row[idx])][:top_k]
    pad = top_k - len(idx)
    return (np.concatenate([idx, np.full(pad, -1)]).astype(np.int32),
            np.concatenate([logp_row[idx], np.full(pad, -np.inf, np.float32)]).astype(np.float32))


@pytest.mark.parametrize("top_k", [1, 5, 32])
@pytest.mark.parametrize("name", CASES)
def test_selection_follows_the_device_scores(cuda, name, top_k):
    logits, seq, words, width = _case(name)
    logp, top_idx, top_logp, log_norm, _ = _score(cuda, logits, seq, words, top_k, width)
    assert top_idx.shape == top_logp.shape == (len(seq), top_k) and top_idx.dtype == np.int32
    for b in range(len(seq)):
        want_idx, want_logp = _select(logp[b], top_k)
        np.testing.assert_array_equal(top_idx[b], want_idx)
        assert top_logp[b].tobytes() == want_logp.tobytes()             # the stored scores, bit for bit
        fin = logp[b][np.isfinite(logp[b])].astype(np.float64)
        if len(fin):
            m = fin.max()
            np.testing.assert_allclose(log_norm[b], m + np.log(np.exp(fin - m).sum()), rtol=1e-5)
        else:
            assert np.isneginf(log_norm[b])
    # without the score array the same words are selected with the same scores
    none, idx2, logp2, norm2, _ = _score(cuda, logits, seq, words, top_k, width, need_scores=False)
    assert none is None
    assert idx2.tobytes() == top_idx.tobytes() and logp2.tobytes() == top_logp.tobytes()
    assert norm2.tobytes() == log_norm.tobytes()


@pytest.mark.parametrize("name", ["ragged_gauss", "ragged_int", "chunks", "table_in_workspace"])
def test_two_calls_are_bitwise_equal(cuda, name):
    logits, seq, words, width = _case(name)
    first = _score(cuda, logits, seq, words, 5, width)
    second = _score(cuda, logits, seq, words, 5, width)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


def test_workspace_table_at_a_small_shape(cuda, ocrk_opts):
    """CTC_LDS = 0 sends a shape that fits LDS down the route that gathers from the workspace table:
    the same expressions in the same order, so the same bits."""
    logits, seq, words, width, _want, lds = _run(cuda, "ragged_gauss")
    ocrk_opts("CTC_LDS", 0)
    ws = _score(cuda, logits, seq, words, 5, width)
    for a, b in zip(lds, ws):
        assert a.tobytes() == b.tobytes()


def test_equal_words_rank_by_index(cuda):
    rng = np.random.default_rng(3)
    words = _words(rng, rng.integers(1, 9, 20))
    words[17] = list(words[3])
    logits = _logits(rng, "gauss", 30, 4, C)
    logp, top_idx, top_logp, _, _ = _score(cuda, logits, [30, 30, 21, 16], words, 20)
    for b in range(4):
        assert np.isfinite(logp[b, 3]) and logp[b, 3].tobytes() == logp[b, 17].tobytes()
        order = top_idx[b].tolist()
        assert order.index(17) == order.index(3) + 1
        assert top_logp[b, order.index(3)] == top_logp[b, order.index(17)] == logp[b, 3]


def test_best_word_is_the_oracles(cuda):
    """The device's argmax equals the float64 oracle's on every row with a feasible word -- where the
    oracle's own top-2 gap exceeds twice the score tolerance, which the test asserts for each such row."""
    logits, seq, words, width, want, (logp, top_idx, top_logp, _, _) = _run(cuda, "ragged_gauss")
    rows = [b for b in range(len(seq)) if np.isfinite(want[b]).any()]
    assert rows == [0, 1, 2, 3, 4, 5, 6]
    for b in rows:
        order = np.argsort(-want[b], kind="stable")
        best, second = want[b, order[0]], want[b, order[1]]
        assert np.isfinite(second)
        print(f"row {b}: oracle best {best:.3f} (word {order[0]}), gap {best - second:.3f}, "
              f"2 x tolerance {2 * RTOL * abs(best):.3f}")
        assert best - second > 2 * RTOL * abs(best)
        assert top_idx[b, 0] == order[0]


def test_invalid_words(cuda):
    """Bad lengths and label values: word_status 2 / 3, -inf on every row, never selected, the other
    words' scores untouched, exactly the two status bits."""
    from cnn_lstm_ctc_ocr_amd import _lib
    from cnn_lstm_ctc_ocr_amd import kernels as K
    K.status_word(cuda).zero_()
    rng = np.random.default_rng(4)
    T, B, W = 25, 3, 6
    good = _words(rng, [3, 0, 6, 2, 5])
    logits_h = _logits(rng, "gauss", T, B, C)
    logits = torch.from_numpy(logits_h).to(cuda)
    seq = torch.tensor([25, 11, 6], dtype=torch.int32, device=cuda)
    lab, ln = _dense(good, W)
    # rows 5..8: word_len -1, word_len W + 1, the blank as a label, a label far out of range
    lab = np.concatenate([lab, [[1, 2, 3, 0, 0, 0], [1, 2, 3, 4, 5, 6], [1, C - 1, 3, 0, 0, 0], [4, 10 ** 6, 2, 0, 0, 0]]])
    lab = lab.astype(np.int32)
    ln = np.concatenate([ln, [-1, W + 1, 3, 3]]).astype(np.int32)
    logp, top_idx, top_logp, log_norm, status = [
        o.cpu().numpy() for o in K.ctc_lexicon_score(logits, seq, torch.from_numpy(lab).to(cuda),
                                                     torch.from_numpy(ln).to(cuda), top_k=9)]
    assert K.read_status(cuda, reset=False) == _lib.STATUS_CTC_BAD_LENGTH | _lib.STATUS_CTC_BAD_LABEL
    assert status.tolist() == [0, 0, 0, 0, 0, 2, 2, 3, 3]
    want = _oracle(logits_h, [25, 11, 6], good)
    assert np.all(np.isneginf(logp[:, 5:])) and np.all(np.isfinite(logp[0, :5]))
    np.testing.assert_array_equal(np.isneginf(logp[:, :5]), np.isneginf(want))
    assert not np.isin(top_idx, [5, 6, 7, 8]).any()
    assert sorted(top_idx[0, :5].tolist()) == [0, 1, 2, 3, 4] and np.all(top_idx[:, 5:] == -1)
    for b in range(B):
        want_idx, want_logp = _select(logp[b], 9)
        np.testing.assert_array_equal(top_idx[b], want_idx)
        assert top_logp[b].tobytes() == want_logp.tobytes()
    only_good = _score(cuda, logits_h, seq.cpu().numpy(), good, 9, W)
    assert only_good[0].tobytes() == np.ascontiguousarray(logp[:, :5]).tobytes()
    assert only_good[1].tobytes() == top_idx.tobytes() and only_good[3].tobytes() == log_norm.tobytes()
    np.testing.assert_allclose(logp[:, :5], want, rtol=RTOL)
    K.clear_status(cuda, _lib.STATUS_CTC_BAD_LENGTH | _lib.STATUS_CTC_BAD_LABEL)
    assert K.read_status(cuda) == 0


def test_bad_scalars_launch_nothing(cuda):
    from cnn_lstm_ctc_ocr_amd import _lib
    from cnn_lstm_ctc_ocr_amd import kernels as K
    logits = torch.zeros(4, 2, C, device=cuda)
    seq = torch.full((2,), 4, dtype=torch.int32, device=cuda)
    lab = torch.zeros(3, 2, dtype=torch.int32, device=cuda)
    ln = torch.ones(3, dtype=torch.int32, device=cuda)
    for top_k in (0, 33):
        with pytest.raises(_lib.InvalidArgumentError, match="top_k"):
            K.ctc_lexicon_score(logits, seq, lab, ln, top_k=top_k)
    with pytest.raises(TypeError):
        K.ctc_lexicon_score(logits.bfloat16(), seq, lab, ln)
    with pytest.raises(TypeError):
        K.ctc_lexicon_score(logits, seq, lab.long(), ln)


# ---------------------------------------------------------------- the service
@pytest.fixture(scope="module")
def serving(cuda):
    """A seed-0 fp32 LSTM 512/512 store (untrained), the golden bucket batch, a lexicon of its words
    plus 20 others of the shard, and the eager logits of the batch."""
    from cnn_lstm_ctc_ocr_amd import ModelConfig, ParamStore
    from cnn_lstm_ctc_ocr_amd.config import INFER
    from cnn_lstm_ctc_ocr_amd.decode import Lexicon
    from cnn_lstm_ctc_ocr_amd.mjsynth import num_classes, out_charset
    from cnn_lstm_ctc_ocr_amd.model import convnet_layers, rnn_layers
    with np.load(FIX, allow_pickle=False) as z:
        batch, widths, texts = z["x_u8"], z["widths"], [str(t) for t in z["texts"]]
    others = []
    for r in shard_records("test"):
        t = r["text"]
        if t and t not in texts and t not in others and all(ch in out_charset for ch in t):
            others.append(t)
        if len(others) == 20:
            break
    assert len(others) == 20
    lexicon = Lexicon(texts + others)
    store = ParamStore(ModelConfig(cell="lstm", rnn_sizes=(512, 512), dtype=torch.float32), device=cuda, seed=0)
    with torch.no_grad():
        feats, seq = convnet_layers(torch.from_numpy(batch).to(cuda), torch.from_numpy(widths).to(cuda), INFER, store)
        logits = rnn_layers(feats, seq, num_classes(), store).float().contiguous()
    return store, batch, widths, lexicon, logits, seq.to(torch.int32).contiguous()


@pytest.mark.parametrize("graphs", [False, True])
def test_recognizer_with_a_lexicon(cuda, serving, graphs):
    from cnn_lstm_ctc_ocr_amd import kernels as K
    from cnn_lstm_ctc_ocr_amd.server import LexiconRecognition, Recognizer
    store, batch, widths, lexicon, logits, seq = serving
    K.status_word(cuda).zero_()
    got = Recognizer(store, lexicon=lexicon, detail=True, lexicon_top=3, graphs=graphs)(batch, widths)
    texts = Recognizer(store, lexicon=list(lexicon.words), graphs=graphs)(batch, widths)
    assert len(got) == len(texts) == 8 and all(type(r) is LexiconRecognition for r in got)
    assert [r.text for r in got] == texts
    # the posterior of each chosen word from the loss kernel on the same logits
    lab_all, ln_all = lexicon.tensors(cuda)
    pick = torch.tensor([lexicon.words.index(r.text) for r in got], device=cuda)
    loss, _, _ = K.ctc_loss(logits, lab_all[pick].contiguous(), ln_all[pick].contiguous(), seq, need_grad=False)
    for r, w, nll in zip(got, widths, loss.cpu().tolist()):
        assert r.text in lexicon.words and r.text == r.alternatives[0][0]
        assert len(r.alternatives) == 3 and all(word in lexicon.words for word, _ in r.alternatives)
        print(f"graphs={graphs} {r.text!r}: log confidence {math.log(r.confidence):.4f} loss kernel {-nll:.4f} "
              f"posterior {r.lexicon_posterior:.4f}")
        np.testing.assert_allclose(math.log(r.confidence), -nll, rtol=RTOL)
        np.testing.assert_allclose(math.log(r.confidence), r.alternatives[0][1], rtol=1e-6)
        assert 0 < r.lexicon_posterior <= 1 + 1e-6
        for (w0, lp0), (w1, lp1) in zip(r.alternatives, r.alternatives[1:]):
            assert lp0 > lp1 or (lp0 == lp1 and lexicon.words.index(w0) < lexicon.words.index(w1))
        assert len(r.char_confidence) == len(r.char_px) == len(r.text)
        assert all(0 < c <= 1 for c in r.char_confidence)
        flat = [x for px in r.char_px for x in px]
        assert all(0 <= x <= w for x in flat) and flat == sorted(flat)
    assert K.read_status(cuda) == 0
    if graphs:
        eager = Recognizer(store, lexicon=lexicon, detail=True, lexicon_top=3)(batch, widths)
        assert got == eager
        # the captured forward carries no unconstrained decoder; labels() still has its own graph
        rec = Recognizer(store, lexicon=lexicon, graphs=True)
        assert rec(batch, widths) == texts
        assert [g.decoder for g in rec.graphs.values()] == [None]
        assert torch.equal(rec.labels(batch, widths), Recognizer(store).labels(batch, widths))
        assert sorted(str(g.decoder) for g in rec.graphs.values()) == ["None", "greedy"]


def test_lexicon_decoder_makes_no_host_sync(cuda, serving):
    from cnn_lstm_ctc_ocr_amd import decode
    store, batch, widths, lexicon, logits, seq = serving
    decode.ctc_lexicon_decoder(logits, seq, lexicon, 2)                  # uploads the lexicon's tensors
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        idx, logp, log_norm = decode.ctc_lexicon_decoder(logits, seq, lexicon, 2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(idx.shape) == tuple(logp.shape) == (8, 2) and idx.dtype == torch.int32
    assert tuple(log_norm.shape) == (8,) and bool((logp[:, 0] <= log_norm).all())
