"""NumPy float32 restatement of ocrk_ctc_keyed_field's definition (include/ocrk.h):
the jointly best placement of one keyword of a group, then a gap, then a string
matching a pattern, scored against the greedy path, with the kernel's own tie
order, so the device can be compared bit for bit. A test helper
(tests/test_ctc_keyed_ref.py pins it to ctc_field_ref.field and to brute-force
enumeration)."""
import numpy as np

import ctc_field_ref as FR
from ctc_spot_ref import emissions, relative, skips

F32 = np.float32
NEG = F32(-np.inf)
NO_GAP = (NEG, -1, -1, -1)


def trail(rel, labels, alts=None):
    """Step 1. K[t] = (V[t][S - 1], its start) per frame: the keyword's best placement ending
    exactly at frame t + 1, from ocrk_ctc_spot's recursion (ctc_spot_ref.spot's loop)."""
    L = rel.shape[0]
    if L == 0:
        return []
    e = emissions(rel, labels, alts)
    skip = skips(labels, alts)
    S = e.shape[1]
    V = np.full(S, NEG, F32)
    st = np.full(S, -1, np.int64)
    out = []
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
        out.append((V[S - 1], int(st[S - 1])))
    return out


def gap_state(trails, L, gap_cost):
    """Step 2. G[t] = (value, keyword index, keyword first, keyword end): what a field entering
    position 0 at frame t inherits. trails: {keyword index: trail}, visited in ascending index."""
    cost = F32(gap_cost)
    G = [NO_GAP] * L
    for t in range(1, L):
        v, k, f, e = G[t - 1]
        cur = (F32(v - cost), k, f, e) if k >= 0 else NO_GAP    # the carry: one float32 subtraction
        for kk in sorted(trails):
            kv, ks = trails[kk][t - 1]
            if kv > cur[0]:                                  # only if strictly greater
                cur = (kv, kk, ks, t)
        G[t] = cur
    return G


def field_with_entry(rel, cls, opt, entry):
    """Step 3. ctc_field_ref.field's recursion on rel [L, C], position 0 entered at frame t with
    entry[t] (float32) instead of float32 0. Returns (score, first, end, text)."""
    n = len(cls)
    assert len(opt) == n and FR.structure_ok(opt)
    L, C = rel.shape
    k = FR.before(opt)
    ends = FR.end_positions(opt)
    lab = [np.array([C - 1] + list(c)) for c in cls]
    V = [np.full(len(l), NEG, F32) for l in lab]
    start = [np.full(len(l), -1, np.int64) for l in lab]
    chosen = [np.full((len(l), n), -1, np.int64) for l in lab]
    best, first, end, text = NEG, -1, -1, (-1,) * n
    for t in range(L):
        ent = F32(entry[t])
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
                if i == 0 and ent > b[j]:                    # the entry: 0 in ocrk_ctc_field, G[t] here
                    nV[i][1 + j] = ent + rel[t, lab[i][1 + j]]
                    nstart[i][1 + j], nchosen[i][1 + j] = t, -1
                nchosen[i][1 + j, i] = lab[i][1 + j]
        V, start, chosen = nV, nstart, nchosen
        for i in ends:
            for j in np.nonzero(V[i][1:] >= best)[0]:
                v, s = V[i][1 + j], int(start[i][1 + j])
                if v > best or (v == best and np.isfinite(best) and s == first):
                    best, first, end, text = v, s, t + 1, tuple(int(x) for x in chosen[i][1 + j])
    return best, first, end, text


def keyed(row_logits, keywords, alts, cls, opt, gap_cost):
    """row_logits: float32 [L, C] (one row cut to its length; blank = C - 1); keywords: the
    group's label lists, as {index into the flat list: labels} or a list (indices 0..); alts: the
    same shape of alternatives (-1 for none), or None; cls, opt: the pattern. Returns (score
    float32, (kw_first, kw_end, first, end), kw_index, kw_score float32, text); -inf, -1s, -1, -inf
    and -1s where no keyword-then-string path fits L frames."""
    row_logits = np.asarray(row_logits)
    assert row_logits.dtype == np.float32
    if not isinstance(keywords, dict):
        alts = None if alts is None else dict(enumerate(alts))
        keywords = dict(enumerate(keywords))
    L = row_logits.shape[0]
    n = len(cls)
    rel = relative(row_logits) if L else row_logits
    trails = {k: trail(rel, w, None if alts is None else alts[k]) for k, w in keywords.items()}
    G = gap_state(trails, L, gap_cost)
    score, first, end, text = field_with_entry(rel, cls, opt, [g[0] for g in G])
    if first < 0:
        return NEG, (-1, -1, -1, -1), -1, NEG, (-1,) * n
    _v, k, kf, ke = G[first]
    return score, (kf, ke, first, end), k, trails[k][ke - 1][0], text


def keyed_batch(logits, seq_len, keywords, alts, groups, patterns, gap_cost, width=None):
    """Time-major float32 [T, B, C]; keywords: the flat list of label lists (None for one the
    device is to treat as invalid); alts: None or one list per keyword; groups: the keyed field of
    each keyword; patterns: one (cls, opt) pair per keyed field, or None for an invalid one.
    Returns (score f32 [B, P], span i32 [B, P, 4], kw_index i32 [B, P], kw_score f32 [B, P],
    text i32 [B, P, width])."""
    T, B, _ = logits.shape
    P = len(patterns)
    width = max(len(p[0]) for p in patterns if p is not None) if width is None else width
    score = np.full((B, P), NEG, F32)
    span = np.full((B, P, 4), -1, np.int32)
    kw_index = np.full((B, P), -1, np.int32)
    kw_score = np.full((B, P), NEG, F32)
    text = np.full((B, P, width), -1, np.int32)
    for b in range(B):
        L = min(max(int(seq_len[b]), 0), T)
        row = np.ascontiguousarray(logits[:L, b])
        for a, pat in enumerate(patterns):
            group = {k: w for k, (w, g) in enumerate(zip(keywords, groups)) if g == a and w is not None}
            if pat is None or not group:
                continue
            galts = None if alts is None else {k: alts[k] for k in group}
            score[b, a], span[b, a], kw_index[b, a], kw_score[b, a], lab = keyed(row, group, galts, *pat, gap_cost)
            text[b, a, :len(lab)] = lab
    return score, span, kw_index, kw_score, text
