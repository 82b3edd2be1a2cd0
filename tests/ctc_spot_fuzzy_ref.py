"""NumPy float32 restatement of ocrk_ctc_spot_fuzzy's recursion (include/ocrk.h):
the best path inside a row that spells a keyword with at most `err` edits
(substitution, insertion, deletion of an inner symbol), scored against the
greedy path, with the kernel's own candidate and tie order, so the device can
be compared bit for bit; and a backtrace of the best path's state sequence. A
test helper (tests/test_ctc_spot_fuzzy_ref.py pins it to an enumeration of
state paths). The recursion runs on all the rows of a batch at once."""
import numpy as np

from ctc_spot_ref import F32, NEG, MAX_LEN, relative, sets, emissions, skips

MAX_ERR = 2
# candidate codes of the backtrace (kind, layer and lane of the predecessor follow from them)
M_STAY, M_ONE, M_TWO, M_ENTRY, M_W0, M_W1, M_W2, M_DEL3, M_DEL4 = range(9)
W_STAY, W_M0, W_M1, W_M2, W_ENTRY, W_WILD = range(6)
W_NONE = -1                                                 # a wild state no candidate reached


def max_budget(n):
    """The largest budget a keyword of n symbols takes."""
    return min(MAX_ERR, n - 1)


def wild(rel):
    """(nb f32 [..., L], a [..., L]): the best non-blank rel of each frame and the lowest class attaining it."""
    nonblank = rel[..., :-1]
    return nonblank.max(axis=-1).astype(F32), nonblank.argmax(axis=-1)


def _shift(x, d, fill):
    """Lane s takes lane s - d; the lanes shifted in take `fill`."""
    out = np.full_like(x, fill)
    if d < x.shape[-1]:
        out[..., d:] = x[..., :x.shape[-1] - d]
    return out


def _take(b, bs, bc, mask, v, vs, code):
    """A later candidate replaces the current one only where strictly greater."""
    m = mask & (v > b)
    b[m], bs[m], bc[m] = v[m], vs[m], code


def spot_rows(rel, lengths, labels, alts=None, err=0, edit_cost=0.0, trace=False):
    """rel f32 [B, T, C] (frames at or past lengths[b] are not read: any value), lengths [B];
    labels: 1..32 classes in [0, C - 1); alts: per position a class or -1, or None;
    err in 0..min(2, n - 1); edit_cost a float32 >= 0, +inf allowed.
    Returns (score f32 [B], first [B], end [B], errors [B]): -inf, (-1, -1) and -1 where no
    path exists; with trace=True also, per row, the best path as a list over its frames
    first..end-1 of (kind 'M' or 'W', layer e, state s, candidate code), None without a path."""
    rel = np.asarray(rel)
    assert rel.dtype == np.float32 and rel.ndim == 3
    n = len(labels)
    assert 1 <= n <= MAX_LEN and 0 <= err <= max_budget(n)
    cost = F32(edit_cost)
    assert cost >= 0
    B, T, C = rel.shape
    lengths = np.clip(np.asarray(lengths, np.int64), 0, T)
    S = 2 * n - 1
    lane = np.arange(S)
    even, odd = lane % 2 == 0, lane % 2 == 1
    sset = sets(labels, alts)
    skip = skips(labels, alts)
    skip4 = np.zeros(S, bool)                                # deletion of symbol i - 1, symbols i - 2 and i adjacent
    for i in range(2, n):
        skip4[2 * i] = not (sset[i] & sset[i - 2])
    valid = np.arange(T)[None, :] < lengths[:, None]
    rel = np.where(valid[:, :, None], rel, F32(0)).astype(F32)
    nb, a = wild(rel)                                        # [B, T]
    a = np.where(valid, a, -1)
    # own[b, t, s]: a(t) is not in the set of even lane s (true on the blank lanes)
    own = np.ones((B, T, S), bool)
    for i, st in enumerate(sset):
        own[:, :, 2 * i] = ~np.isin(a, list(st))
    # prev[b, t, s]: a(t) is not in the set of the symbol before lane s, index (s - 1) >> 1 (s >= 1)
    prev = np.ones((B, T, S), bool)
    prev[:, :, 1:] = own[:, :, (lane[1:] - 1) // 2 * 2]
    em = np.stack([emissions(rel[b], labels, alts) for b in range(B)]) if B else np.zeros((0, T, S), F32)

    M = [np.full((B, S), NEG, F32) for _ in range(err + 1)]
    Ms = [np.full((B, S), -1, np.int64) for _ in range(err + 1)]
    W = [np.full((B, S), NEG, F32) for _ in range(err + 1)]   # W[0] stays empty
    Ws = [np.full((B, S), -1, np.int64) for _ in range(err + 1)]
    best = np.full(B, NEG, F32)
    first = np.full(B, -1, np.int64)
    end = np.full(B, -1, np.int64)
    errors = np.full(B, -1, np.int64)
    bkind = np.zeros(B, np.int64)                            # 0: the best ended on M, 1: on W
    tr = []                                                  # per frame: (codes of M[e], codes of W[e])
    all_s = np.ones((B, S), bool)
    for t in range(T):
        live = t < lengths                                   # rows past their length keep what they have
        if not live.any():
            break
        same = (a[:, t] == a[:, t - 1]) if t >= 1 else np.zeros(B, bool)
        own_prev = own[:, t - 1] if t >= 1 else np.ones((B, S), bool)
        prev_now = prev[:, t]
        nM, nMs, nW, nWs = list(M), list(Ms), list(W), list(Ws)
        cM, cW = [None] * (err + 1), [None] * (err + 1)
        for e in range(err + 1):
            b, bs = M[e].copy(), Ms[e].copy()                # 1 stay
            bc = np.full((B, S), M_STAY, np.int8)
            _take(b, bs, bc, all_s, _shift(M[e], 1, NEG), _shift(Ms[e], 1, -1), M_ONE)
            _take(b, bs, bc, skip[None, :] & all_s, _shift(M[e], 2, NEG), _shift(Ms[e], 2, -1), M_TWO)
            if e == 0:
                m = (lane == 0)[None, :] & (F32(0) > b)      # 4 entry
                b[m], bs[m], bc[m] = F32(0), t, M_ENTRY
            else:
                _take(b, bs, bc, odd[None, :] & all_s, W[e], Ws[e], M_W0)
                _take(b, bs, bc, odd[None, :] | ((even & (lane >= 2))[None, :] & own_prev),
                      _shift(W[e], 1, NEG), _shift(Ws[e], 1, -1), M_W1)
                _take(b, bs, bc, (even & (lane >= 2))[None, :] & own_prev,
                      _shift(W[e], 2, NEG), _shift(Ws[e], 2, -1), M_W2)
                _take(b, bs, bc, (even & (lane >= 4))[None, :] & all_s,
                      (_shift(M[e - 1], 3, NEG) - cost).astype(F32), _shift(Ms[e - 1], 3, -1), M_DEL3)
                _take(b, bs, bc, skip4[None, :] & all_s,
                      (_shift(M[e - 1], 4, NEG) - cost).astype(F32), _shift(Ms[e - 1], 4, -1), M_DEL4)
            nM[e], nMs[e], cM[e] = (b + em[:, t]).astype(F32), bs, bc
            if e == 0:
                continue
            b = np.where(same[:, None], W[e], NEG).astype(F32)   # 1 stay, while the frame's best class stays
            bs = np.where(same[:, None], Ws[e], -1)
            bc = np.where(same[:, None] & (W[e] > NEG), W_STAY, W_NONE).astype(np.int8)
            _take(b, bs, bc, odd[None, :] & all_s, (M[e - 1] - cost).astype(F32), Ms[e - 1], W_M0)
            _take(b, bs, bc, (even & (lane >= 1))[None, :] | (odd[None, :] & prev_now),
                  (_shift(M[e - 1], 1, NEG) - cost).astype(F32), _shift(Ms[e - 1], 1, -1), W_M1)
            _take(b, bs, bc, (even & (lane >= 2))[None, :] & prev_now,
                  (_shift(M[e - 1], 2, NEG) - cost).astype(F32), _shift(Ms[e - 1], 2, -1), W_M2)
            if e == 1:
                v = F32(0) - cost
                m = (lane == 0)[None, :] & (v > b)
                b[m], bs[m], bc[m] = v, t, W_ENTRY
            if e == 2 and t >= 1:
                _take(b, bs, bc, (lane >= 1)[None, :] & ~same[:, None],
                      (_shift(W[1], 1, NEG) - cost).astype(F32), _shift(Ws[1], 1, -1), W_WILD)
            nW[e], nWs[e], cW[e] = (b + nb[:, t, None]).astype(F32), bs, bc
        for e in range(err + 1):                             # rows past their length are frozen
            M[e] = np.where(live[:, None], nM[e], M[e])
            Ms[e] = np.where(live[:, None], nMs[e], Ms[e])
            W[e] = np.where(live[:, None], nW[e], W[e])
            Ws[e] = np.where(live[:, None], nWs[e], Ws[e])
        if trace:
            tr.append((cM, cW))
        for e in range(err + 1):
            for kind, V, St in ((0, M[e], Ms[e]), (1, W[e], Ws[e])):
                if kind == 1 and e == 0:
                    continue
                m = live & (V[:, S - 1] > best)
                best[m], first[m], end[m], errors[m], bkind[m] = V[m, S - 1], St[m, S - 1], t + 1, e, kind
    if not trace:
        return best, first, end, errors
    paths = []
    for b in range(B):
        if end[b] < 0:
            paths.append(None)
            continue
        kind, e, s, t = "MW"[bkind[b]], int(errors[b]), S - 1, int(end[b]) - 1
        path = []
        while True:
            code = int(tr[t][0 if kind == "M" else 1][e][b, s])
            path.append((kind, e, s, code))
            if kind == "M":
                if code == M_ENTRY:
                    break
                kind, e, s = {M_STAY: ("M", e, s), M_ONE: ("M", e, s - 1), M_TWO: ("M", e, s - 2),
                              M_W0: ("W", e, s), M_W1: ("W", e, s - 1), M_W2: ("W", e, s - 2),
                              M_DEL3: ("M", e - 1, s - 3), M_DEL4: ("M", e - 1, s - 4)}[code]
            else:
                assert code != W_NONE
                if code == W_ENTRY:
                    break
                kind, e, s = {W_STAY: ("W", e, s), W_M0: ("M", e - 1, s), W_M1: ("M", e - 1, s - 1),
                              W_M2: ("M", e - 1, s - 2), W_WILD: ("W", 1, s - 1)}[code]
            t -= 1
        assert t == first[b], (t, first[b])
        paths.append(path[::-1])
    return best, first, end, errors, paths


def spot(logits, labels, alts=None, err=0, edit_cost=0.0, trace=False):
    """One row: logits float32 [L, C] cut to its length (blank = C - 1). Returns (score float32,
    first, end, errors), with trace=True also the best path (see spot_rows)."""
    logits = np.asarray(logits)
    assert logits.dtype == np.float32
    L = logits.shape[0]
    if L == 0:
        return (NEG, -1, -1, -1, None) if trace else (NEG, -1, -1, -1)
    r = spot_rows(relative(logits)[None], [L], labels, alts, err, edit_cost, trace)
    out = (r[0][0], int(r[1][0]), int(r[2][0]), int(r[3][0]))
    return out + (r[4][0],) if trace else out


def labelling(logits, labels, alts, path, first):
    """The frame labelling of a traced path: the class each frame of the path reads (a matched
    symbol's better label, the blank, or a wild frame's best non-blank class), CTC-collapsed."""
    rel = relative(np.asarray(logits))
    C = rel.shape[1]
    _, a = wild(rel)
    frames = []
    for j, (kind, _e, s, _code) in enumerate(path):
        t = first + j
        if kind == "W":
            frames.append(int(a[t]))
        elif s % 2:
            frames.append(C - 1)
        else:
            i = s // 2
            l, alt = int(labels[i]), -1 if alts is None else int(alts[i])
            frames.append(alt if alt >= 0 and rel[t, alt] > rel[t, l] else l)
    out, last = [], None
    for c in frames:
        if c != last and c != C - 1:
            out.append(c)
        last = c
    return frames, out


def spot_batch(logits, seq_len, keywords, alts=None, errs=None, edit_cost=0.0):
    """Time-major float32 [T, B, C]; keywords: lists of classes; alts: None or one list (or None)
    per keyword; errs: one budget per keyword (None: all 0). Returns (score float32 [B, K], span
    int32 [B, K, 2], errors int32 [B, K])."""
    T, B, _ = logits.shape
    K = len(keywords)
    score = np.full((B, K), NEG, F32)
    span = np.full((B, K, 2), -1, np.int32)
    errors = np.full((B, K), -1, np.int32)
    L = np.clip(np.asarray(seq_len, np.int64), 0, T)
    valid = np.arange(T)[None, :] < L[:, None]
    lg = np.where(valid[:, :, None], np.transpose(logits, (1, 0, 2)), F32(0)).astype(F32)
    rel = relative(lg)
    for k, kw in enumerate(keywords):
        v, f, e, er = spot_rows(rel, L, kw, None if alts is None else alts[k], 0 if errs is None else int(errs[k]),
                                edit_cost)
        score[:, k], span[:, k, 0], span[:, k, 1], errors[:, k] = v, f, e, er
    return score, span, errors
