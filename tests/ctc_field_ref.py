"""NumPy float32 restatement of ocrk_ctc_field's recursion (include/ocrk.h): the
best-scoring string matching a small character-class pattern, placed anywhere
inside a row, scored against the greedy path, with the kernel's own tie order,
so the device can be compared bit for bit. A test helper
(tests/test_ctc_field_ref.py pins it to enumeration through ctc_spot_ref.spot)."""
import itertools

import numpy as np

from ctc_spot_ref import relative

F32 = np.float32
NEG = F32(-np.inf)
MAX_LEN = 16
MAX_CLASS = 16
MAX_OPT_RUN = 3

# (classes, optional flags) over C = 5 (labels 0..3), shared by the host and the GPU tests
FULL = [0, 1, 2, 3]
SMALL_PATTERNS = [
    ([[0, 1, 3]], [0]),                                                  # one position of 3 labels
    ([[0, 1], [1, 2]], [0, 0]),                                          # two overlapping classes
    ([[0], [1, 2], [3]], [0, 1, 0]),                                     # mandatory, optional, mandatory
    ([[2], [0, 1], [1, 3], [0], [3]], [0, 1, 1, 1, 0]),                  # three optionals between two singletons
    ([[1], [0, 2]], [0, 1]),                                             # a trailing optional
    ([[2], [2]], [0, 0]),                                                # the repeat: needs its blank
    ([FULL, FULL, FULL, FULL], [0, 0, 1, 1]),                            # four full classes, two trailing optionals
    ([[1], [3]], [0, 0]),
]


def structure_ok(opt):
    """Position 0 mandatory, at most 3 consecutive optional positions, 1..16 positions."""
    if not 1 <= len(opt) <= MAX_LEN or opt[0]:
        return False
    run = 0
    for o in opt:
        run = run + 1 if o else 0
        if run > MAX_OPT_RUN:
            return False
    return True


def before(opt):
    """k[i]: the number of consecutive optional positions immediately before i."""
    k = []
    for i in range(len(opt)):
        r = 0
        while i - 1 - r >= 0 and opt[i - 1 - r]:
            r += 1
        k.append(r)
    return k


def end_positions(opt):
    """n - 1, then back through the trailing optional positions to the first mandatory one."""
    i = len(opt) - 1
    ends = [i]
    while opt[i]:
        i -= 1
        ends.append(i)
    return ends


def language(cls, opt):
    """Every label string the pattern matches (with repeats where classes overlap), in no particular order."""
    per = [[(l,) for l in c] + ([()] if o else []) for c, o in zip(cls, opt)]
    return [tuple(itertools.chain.from_iterable(pick)) for pick in itertools.product(*per)]


def field(logits, cls, opt):
    """logits: float32 [L, C] (one row cut to its length; blank = C - 1); cls: per
    position 1..16 strictly ascending classes in [0, C - 1); opt: per position a
    flag. Returns (score float32, first, end, text): text has the chosen class
    per position, -1 for an absent one; -inf, -1, -1 and all -1 where no
    matching string fits L frames."""
    logits = np.asarray(logits)
    n = len(cls)
    assert logits.dtype == np.float32 and len(opt) == n and structure_ok(opt)
    L, C = logits.shape
    for c in cls:
        assert 1 <= len(c) <= MAX_CLASS and all(0 <= l < C - 1 for l in c)
        assert all(a < b for a, b in zip(c, c[1:]))
    rel = relative(logits) if L else logits
    k = before(opt)
    ends = end_positions(opt)
    # per position i the states in the recursion's own order: index 0 the blank after i, index 1 + j the label
    # cls[i][j]. np.argmax returns the FIRST of equal maxima: the scan in which a later candidate replaces the
    # current one only if strictly greater.
    lab = [np.array([C - 1] + list(c)) for c in cls]
    V = [np.full(len(l), NEG, F32) for l in lab]
    start = [np.full(len(l), -1, np.int64) for l in lab]
    chosen = [np.full((len(l), n), -1, np.int64) for l in lab]
    best, first, end, text = NEG, -1, -1, (-1,) * n
    for t in range(L):
        nV, nstart, nchosen = [v.copy() for v in V], [s.copy() for s in start], [c.copy() for c in chosen]
        for i in range(n):
            s = int(np.argmax(V[i]))                         # the blank after i: itself, then i's labels
            nV[i][0] = V[i][s] + rel[t, C - 1]
            nstart[i][0], nchosen[i][0] = start[i][s], chosen[i][s]
            m = len(cls[i])
            b = V[i][1:].copy()                              # stay
            src = [(i, 1 + j) for j in range(m)]
            for q in range(i - 1, max(i - 2 - k[i], -1), -1):   # predecessors, nearest first
                cand = np.where(lab[q][None, :] == lab[i][1:, None], NEG, V[q][None, :])   # not the same label twice
                s = np.argmax(cand, axis=1)
                v = cand[np.arange(m), s]
                for j in np.nonzero(v > b)[0]:
                    b[j], src[j] = v[j], (q, int(s[j]))
            nV[i][1:] = b + rel[t, lab[i][1:]]               # a single float32 add
            for j, (q, s) in enumerate(src):
                nstart[i][1 + j], nchosen[i][1 + j] = start[q][s], chosen[q][s]
                if i == 0 and F32(0) > b[j]:                 # the free start
                    nV[i][1 + j] = F32(0) + rel[t, lab[i][1 + j]]
                    nstart[i][1 + j], nchosen[i][1 + j] = t, -1
                nchosen[i][1 + j, i] = lab[i][1 + j]
        V, start, chosen = nV, nstart, nchosen
        for i in ends:
            for j in np.nonzero(V[i][1:] >= best)[0]:
                v, s = V[i][1 + j], int(start[i][1 + j])
                if v > best or (v == best and np.isfinite(best) and s == first):
                    best, first, end, text = v, s, t + 1, tuple(int(x) for x in chosen[i][1 + j])
    return best, first, end, text


def field_batch(logits, seq_len, patterns, width=None):
    """Time-major float32 [T, B, C]; patterns: (cls, opt) pairs. Returns (score
    float32 [B, P], span int32 [B, P, 2], text int32 [B, P, width])."""
    T, B, _ = logits.shape
    width = max(len(c) for c, _ in patterns) if width is None else width
    score = np.full((B, len(patterns)), NEG, F32)
    span = np.full((B, len(patterns), 2), -1, np.int32)
    text = np.full((B, len(patterns), width), -1, np.int32)
    for b in range(B):
        L = min(max(int(seq_len[b]), 0), T)
        row = np.ascontiguousarray(logits[:L, b])
        for p, (cls, opt) in enumerate(patterns):
            score[b, p], span[b, p, 0], span[b, p, 1], lab = field(row, cls, opt)
            text[b, p, :len(lab)] = lab
    return score, span, text
