"""NumPy float32 restatement of ocrk_ctc_spot's recursion (include/ocrk.h): the
best placement of a keyword inside a row, free start and free end, scored
against the greedy path, with the kernel's own tie order, so the device can be
compared bit for bit. A test helper (tests/test_ctc_spot_ref.py pins it to
brute-force enumeration)."""
import numpy as np

F32 = np.float32
NEG = F32(-np.inf)
MAX_LEN = 32


def relative(logits):
    """rel[t][c] = logits[t][c] - max_c logits[t][c], one float32 subtraction."""
    logits = np.asarray(logits)
    assert logits.dtype == np.float32
    return (logits - logits.max(axis=-1, keepdims=True)).astype(F32)


def sets(labels, alts=None):
    """The symbol set {l_i, a_i} of each position."""
    alts = [-1] * len(labels) if alts is None else alts
    return [{int(l)} | ({int(a)} if a >= 0 else set()) for l, a in zip(labels, alts)]


def required_time(labels, alts=None):
    """n + the adjacent positions whose sets overlap (they need the blank between them)."""
    s = sets(labels, alts)
    return len(s) + sum(1 for p, q in zip(s, s[1:]) if p & q)


def emissions(rel, labels, alts=None):
    """e[t][s] float32 [L, S], S = 2 n - 1: even s symbol s / 2, odd s the blank C - 1."""
    L, C = rel.shape
    n = len(labels)
    e = np.empty((L, 2 * n - 1), F32)
    e[:, 1::2] = rel[:, C - 1:C]
    for i, l in enumerate(labels):
        e[:, 2 * i] = rel[:, int(l)]
        if alts is not None and alts[i] >= 0:
            e[:, 2 * i] = np.maximum(rel[:, int(l)], rel[:, int(alts[i])])
    return e


def skips(labels, alts=None):
    """skip[s]: state s may be entered from s - 2 (even s >= 2, disjoint symbol sets)."""
    s = sets(labels, alts)
    skip = np.zeros(2 * len(s) - 1, bool)
    for i in range(1, len(s)):
        skip[2 * i] = not (s[i] & s[i - 1])
    return skip


def spot(logits, labels, alts=None):
    """logits: float32 [L, C] (one row cut to its length; blank = C - 1); labels:
    1..32 classes in [0, C - 1); alts: per position a class or -1, or None.
    Returns (score float32, first, end): -inf and (-1, -1) where the keyword
    does not fit L frames."""
    logits = np.asarray(logits)
    assert logits.dtype == np.float32 and 1 <= len(labels) <= MAX_LEN
    L = logits.shape[0]
    if required_time(labels, alts) > L:
        return NEG, -1, -1
    e = emissions(relative(logits), labels, alts)
    skip = skips(labels, alts)
    S = e.shape[1]
    V = np.full(S, NEG, F32)
    st = np.full(S, -1, np.int64)
    best, first, end = NEG, -1, -1
    for t in range(L):
        b, bs = V.copy(), st.copy()                          # stay
        v1 = np.concatenate([[NEG], V[:-1]]).astype(F32)
        s1 = np.concatenate([[-1], st[:-1]])
        v2 = np.concatenate([[NEG, NEG], V[:-2]]).astype(F32)[:S]
        s2 = np.concatenate([[-1, -1], st[:-2]])[:S]
        m = v1 > b                                           # one back only if strictly greater
        b[m], bs[m] = v1[m], s1[m]
        m = skip & (v2 > b)                                  # then two back where allowed
        b[m], bs[m] = v2[m], s2[m]
        if F32(0) > b[0]:                                    # then entry, state 0 only
            b[0], bs[0] = F32(0), t
        V, st = (b + e[t]).astype(F32), bs                   # a single float32 add
        if V[S - 1] > best:
            best, first, end = V[S - 1], int(st[S - 1]), t + 1
    return best, first, end


def spot_batch(logits, seq_len, keywords, alts=None):
    """Time-major float32 [T, B, C]; keywords: lists of classes; alts: None or
    one list (or None) per keyword. Returns (score float32 [B, K], span int32
    [B, K, 2])."""
    T, B, _ = logits.shape
    score = np.full((B, len(keywords)), NEG, F32)
    span = np.full((B, len(keywords), 2), -1, np.int32)
    for b in range(B):
        L = min(max(int(seq_len[b]), 0), T)
        row = np.ascontiguousarray(logits[:L, b])
        for k, kw in enumerate(keywords):
            score[b, k], span[b, k, 0], span[b, k, 1] = spot(row, kw, None if alts is None else alts[k])
    return score, span
