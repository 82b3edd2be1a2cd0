"""NumPy float32 restatement of ocrk_ctc_align's recursion (include/ocrk.h): the
best single path of a label through the raw logits, with the kernel's own
tie-breaking, so the device path can be compared bit for bit. A test helper
(tests/test_ctc_align_ref.py pins it to brute-force path enumeration)."""
import numpy as np

F32 = np.float32
NEG = F32(-np.inf)


def extended(label, blank):
    """l' = [blank, l0, blank, l1, ..., blank]."""
    ext = [blank]
    for c in label:
        ext += [int(c), blank]
    return np.array(ext, np.int64)


def required_time(label):
    label = list(label)
    return len(label) + sum(1 for a, b in zip(label, label[1:]) if a == b)


def feasible(label, L):
    return L >= 1 and required_time(label) <= L


def best_path(logits, label):
    """logits: float32 [L, C] (one sequence cut to its length, L >= 1, blank =
    C - 1); label: feasible list of classes. Returns (states int [L], score
    float32): the extended-state index per frame and the float32 sum of the
    raw logits along the path, accumulated as the recursion does."""
    logits = np.asarray(logits)
    assert logits.dtype == np.float32
    L, C = logits.shape
    ext = extended(label, C - 1)
    S = len(ext)
    s_idx = np.arange(S)
    skip = np.zeros(S, bool)
    skip[3:] = (s_idx[3:] % 2 == 1) & (ext[3:] != ext[1:-2])
    V = np.full(S, NEG, F32)
    V[0] = logits[0, ext[0]]
    if S > 1:
        V[1] = logits[0, ext[1]]
    bp = np.zeros((L, S), np.int8)
    for t in range(1, L):
        best = V.copy()
        a1 = np.concatenate([[NEG], V[:-1]]).astype(F32)
        a2 = np.concatenate([[NEG, NEG], V[:-2]]).astype(F32)[:S]
        a2[~skip] = NEG
        m1 = a1 > best                       # one back only if strictly greater
        best[m1] = a1[m1]
        m2 = a2 > best                       # then two back only if allowed and strictly greater
        best[m2] = a2[m2]
        bp[t, m1] = 1
        bp[t, m2] = 2
        V = (best + logits[t, ext]).astype(F32)          # a single float32 add
    s = S - 1
    if S >= 2 and V[S - 2] > V[S - 1]:
        s = S - 2
    score = V[s]
    states = np.zeros(L, np.int64)
    for t in range(L - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    return states, score


def spans(states, n):
    """(first, last + 1) frame of each of the n label symbols (state 2 i + 1)."""
    out = np.full((n, 2), -1, np.int64)
    for i in range(n):
        (ts,) = np.nonzero(np.asarray(states) == 2 * i + 1)
        if len(ts):
            out[i] = (ts[0], ts[-1] + 1)
            assert len(ts) == ts[-1] + 1 - ts[0]          # contiguous
    return out


def collapse(classes, blank):
    """CTC collapse of a frame-class sequence: merge repeats, drop blanks."""
    out, prev = [], None
    for c in classes:
        c = int(c)
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def align_batch(logits, labels, seq_len):
    """Batched form over time-major float32 [T, B, C]: (frame_state int [B, T]
    with -1 past each length, span int [B, Lmax, 2] with -1 past each label)."""
    T, B, C = logits.shape
    Lmax = max([len(l) for l in labels] + [0])
    fs = np.full((B, T), -1, np.int64)
    sp = np.full((B, Lmax, 2), -1, np.int64)
    for b in range(B):
        L = min(max(int(seq_len[b]), 0), T)
        st, _ = best_path(np.ascontiguousarray(logits[:L, b]), labels[b])
        fs[b, :L] = st
        sp[b, :len(labels[b])] = spans(st, len(labels[b]))
    return fs, sp


def path_values(logits, states, label):
    """float64 values along a given state path: (path_logp, char_conf [n])."""
    x = np.asarray(logits, np.float64)
    L, C = x.shape
    m = x.max(axis=1, keepdims=True)
    logsm = x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))
    ext = extended(label, C - 1)
    states = np.asarray(states)
    logp = logsm[np.arange(L), ext[states]].sum()
    conf = np.zeros(len(label))
    for i, c in enumerate(label):
        conf[i] = np.exp(logsm[states == 2 * i + 1, int(c)].max())
    return logp, conf
