"""TF-named CTC decoders and edit distance on device tensors.

Mirrors the tf.nn / tf calls the reference makes on the hot path:
  * ctc_greedy_decoder       -- src/weinman/validate.py:85-90
  * ctc_beam_search_decoder  -- src/weinman/test.py:84-88 (beam 128),
                                src/weinman/client.py:227-231 (merge_repeated=False)
  * edit_distance            -- src/weinman/test.py:90 (normalize=False)
ctc_alignment (with frame_center_px / frames_to_px) has no tf counterpart: it
places a decoded string's characters on the frames, for server.Recognition.
Lexicon / ctc_lexicon_decoder have none either: they score a closed word list
against the logits (what src/extract_fields and src/accuracy_measure do on the
host with fuzzy matches of the decoded string), for server.LexiconRecognition.
KeywordSet / ctc_keyword_spotter find keywords inside a line on the same logits
(src/extract_fields/extractor.py's fuzzy regexes), for server.KeywordRecognition.
FuzzyKeywordSet / ctc_fuzzy_keyword_spotter find them with up to two edits each
(extractor.py's FuzzyRegexExtractor(maxerr=(len + 1) / 5)), for
server.FuzzyKeywordHit.
FieldSet / ctc_field_reader read the best string matching a small character-class
pattern out of a line on the same logits (extractor.py's amount, GST and receipt
number regexes over the 1-best string), for server.FieldRecognition.
KeyedFieldSet / ctc_keyed_field_reader pair the two on the lattice: the string
matching a pattern that follows one of a field's keywords (extractor.py's
KWDetector / KWExtractor pairing), for server.KeyedRecognition.
Sparse outputs are returned dense, -1 padded (what sparse_tensor_to_dense(-1)
gives the reference, validate.py:91-92), plus per-row lengths.
"""
import numpy as np
import torch

from . import kernels as K
from . import mjsynth

MAX_WORD_LEN = 255                                          # the CTC kernels' label limit
MAX_KEYWORD_LEN = 32                                        # ocrk_ctc_spot: 2 n - 1 states on the 64 lanes of a wave
MAX_FIELD_LEN = 16                                          # ocrk_ctc_field: positions of a pattern,
MAX_FIELD_CLASS = 16                                        # characters of a class (one per lane of a 16-lane row),
MAX_FIELD_OPTIONAL = 3                                      # and optional positions in a row


def _f32(logits):
    return (logits if logits.dtype == torch.float32 else logits.float()).contiguous()


def ctc_greedy_decoder(inputs, sequence_length, merge_repeated=True):
    """Returns ([dense i64 [B, max_len]], neg_sum_logits [B, 1]) like
    tf.nn.ctc_greedy_decoder's (decoded, neg_sum_logits)."""
    out, out_len, neg = K.ctc_greedy_decode(_f32(inputs), sequence_length.to(torch.int32).contiguous(),
                                            merge_repeated)
    width = int(out_len.max().item()) if out_len.numel() else 0
    return [out[:, :width]], neg.unsqueeze(1)


def ctc_greedy_decoder_raw(inputs, sequence_length, merge_repeated=True):
    """The same decode without the host sync for the output width: (out i64
    [B, T] (labels then -1), out_len i32 [B], neg_sum_logits f32 [B])."""
    return K.ctc_greedy_decode(_f32(inputs), sequence_length.to(torch.int32).contiguous(), merge_repeated)


def ctc_beam_search_decoder(inputs, sequence_length, beam_width=100, top_paths=1, merge_repeated=True):
    """Returns (decoded, log_probability): decoded is a list of top_paths
    dense i64 [B, max_len_k] tensors (-1 padded), log_probability f32
    [B, top_paths]."""
    out, out_len, logp = K.ctc_beam_decode(_f32(inputs), sequence_length.to(torch.int32).contiguous(),
                                           beam_width, top_paths, merge_repeated)
    widths = out_len.max(dim=1).values.tolist() if out_len.numel() else [0] * top_paths
    return [out[k, :, :int(widths[k])] for k in range(top_paths)], logp


def ctc_beam_search_decoder_raw(inputs, sequence_length, beam_width=100, top_paths=1, merge_repeated=True):
    """Same search without the host sync for the output width: (out
    [top_paths, B, T], out_len [top_paths, B], log_probability)."""
    return K.ctc_beam_decode(_f32(inputs), sequence_length.to(torch.int32).contiguous(), beam_width,
                             top_paths, merge_repeated)


def _masked_labels(labels, label_length):
    """Dense i32 labels with every position at or past its row's length set to
    0: the decoders pad with -1, which must never reach a kernel as a label."""
    lab = labels.to(torch.int32)
    if lab.dim() == 1:
        lab = lab.reshape(lab.shape[0], 0)
    ln = label_length.to(torch.int32).contiguous()
    pos = torch.arange(lab.shape[1], device=lab.device, dtype=torch.int32)
    return torch.where(pos[None, :] < ln[:, None], lab, torch.zeros_like(lab)).contiguous(), ln


def ctc_alignment(inputs, labels, label_length, sequence_length):
    """The best single path of each row's label through its logits (no
    reference counterpart: what src/processing needs to place and filter the
    recognised characters). inputs [T, B, C]; labels dense [B, W] as either
    decoder returns them (-1 padded, any integer dtype) with label_length [B];
    sequence_length [B]. Returns (frame_state i32 [B, T] extended-state index
    per frame, -1 past the sequence; span i32 [B, W, 2] (first, end) frames of
    each character; char_conf f32 [B, W]; path_logp f32 [B]; status i32 [B],
    0 = aligned, else the ctc_loss codes and all outputs void)."""
    lab, ln = _masked_labels(labels, label_length)
    return K.ctc_align(_f32(inputs), lab, ln, sequence_length.to(torch.int32).contiguous())


class Lexicon:
    """An ordered closed vocabulary: strings over mjsynth.out_charset, encoded
    once (mjsynth.encode) and kept as dense int32 labels + lengths per device.
    ValueError for an empty list, an empty string, a character outside the
    charset, a duplicate, or a word over 255 characters. Pickles as its plain
    list of strings (the device tensors are rebuilt where it lands)."""

    def __init__(self, words):
        words = list(words)
        if not words:
            raise ValueError("Lexicon: the word list is empty")
        seen = set()
        encoded = []
        for i, w in enumerate(words):
            if not isinstance(w, str):
                raise ValueError(f"Lexicon: entry {i} is {type(w).__name__}, not a string")
            if not w:
                raise ValueError(f"Lexicon: entry {i} is the empty string")
            if len(w) > MAX_WORD_LEN:
                raise ValueError(f"Lexicon: entry {i} has {len(w)} characters (at most {MAX_WORD_LEN})")
            if w in seen:
                raise ValueError(f"Lexicon: duplicate word {w!r} (entry {i})")
            seen.add(w)
            try:
                encoded.append(mjsynth.encode(w))
            except ValueError:
                bad = next(ch for ch in w if ch not in mjsynth.out_charset)
                raise ValueError(f"Lexicon: {w!r} (entry {i}) has the character {bad!r} outside the charset") from None
        self.words = tuple(words)
        self.lengths = np.array([len(e) for e in encoded], np.int32)
        self.labels = np.zeros((len(encoded), int(self.lengths.max())), np.int32)
        for i, e in enumerate(encoded):
            self.labels[i, :len(e)] = e
        self._device = {}

    def __len__(self):
        return len(self.words)

    def __reduce__(self):
        return (Lexicon, (list(self.words),))

    def tensors(self, device):
        """(labels i32 [n, max_len], lengths i32 [n]) on `device`, uploaded once per device."""
        key = str(torch.device(device))
        t = self._device.get(key)
        if t is None:
            t = self._device[key] = (torch.from_numpy(self.labels).to(device),
                                     torch.from_numpy(self.lengths).to(device))
        return t


def ctc_lexicon_decoder(inputs, sequence_length, lexicon, top_k=1):
    """The top_k words of `lexicon` for each row of inputs [T, B, C] by
    log p(word | inputs[:sequence_length[b], b]) (the CTC sum over all paths,
    -ctc_loss), ties to the earlier word. Returns (index i32 [B, top_k] into
    lexicon.words, -1 where fewer than top_k words fit the row; log_probability
    f32 [B, top_k], -inf there; log_norm f32 [B], the log-sum-exp over the whole
    lexicon: exp(log_probability - log_norm) is the posterior within it).
    Device tensors, no host sync."""
    lab, ln = lexicon.tensors(inputs.device)
    _logp, idx, logp, log_norm, _status = K.ctc_lexicon_score(
        _f32(inputs), sequence_length.to(torch.int32).contiguous(), lab, ln, top_k, need_scores=False)
    return idx, logp, log_norm


class KeywordSet:
    """An ordered list of keywords to find INSIDE recognised lines: strings over
    mjsynth.out_charset, encoded once and kept as dense int32 labels,
    alternatives and lengths per device. case_insensitive: the alternative of
    an ASCII letter is its other case (other characters have none), and
    duplicates are judged after case folding. ValueError for an empty list, an
    empty string, a character outside the charset, a duplicate, or a keyword
    over 32 characters (one lattice state per lane of a wave). Pickles as its
    arguments (the device tensors are rebuilt where it lands)."""

    def __init__(self, keywords, case_insensitive=False):
        keywords = list(keywords)
        if not keywords:
            raise ValueError("KeywordSet: the keyword list is empty")
        self.case_insensitive = bool(case_insensitive)
        seen = set()
        encoded = []
        for i, w in enumerate(keywords):
            if not isinstance(w, str):
                raise ValueError(f"KeywordSet: entry {i} is {type(w).__name__}, not a string")
            if not w:
                raise ValueError(f"KeywordSet: entry {i} is the empty string")
            if len(w) > MAX_KEYWORD_LEN:
                raise ValueError(f"KeywordSet: entry {i} has {len(w)} characters (at most {MAX_KEYWORD_LEN})")
            key = w.lower() if self.case_insensitive else w
            if key in seen:
                raise ValueError(f"KeywordSet: duplicate keyword {w!r} (entry {i})")
            seen.add(key)
            try:
                encoded.append(mjsynth.encode(w))
            except ValueError:
                bad = next(ch for ch in w if ch not in mjsynth.out_charset)
                raise ValueError(f"KeywordSet: {w!r} (entry {i}) has the character {bad!r} outside the "
                                 "charset") from None
        self.keywords = tuple(keywords)
        self.lengths = np.array([len(e) for e in encoded], np.int32)
        self.labels = np.zeros((len(encoded), int(self.lengths.max())), np.int32)
        self.alternatives = np.full(self.labels.shape, -1, np.int32)
        for i, (w, e) in enumerate(zip(keywords, encoded)):
            self.labels[i, :len(e)] = e
            if self.case_insensitive:
                self.alternatives[i, :len(e)] = [mjsynth.out_charset.index(ch.swapcase())
                                                 if ch.isascii() and ch.isalpha() else -1 for ch in w]
        self._device = {}

    def __len__(self):
        return len(self.keywords)

    def __reduce__(self):
        return (KeywordSet, (list(self.keywords), self.case_insensitive))

    def tensors(self, device):
        """(labels i32 [n, max_len], alternatives i32 [n, max_len] or None when case-sensitive,
        lengths i32 [n]) on `device`, uploaded once per device."""
        key = str(torch.device(device))
        t = self._device.get(key)
        if t is None:
            t = self._device[key] = (torch.from_numpy(self.labels).to(device),
                                     torch.from_numpy(self.alternatives).to(device) if self.case_insensitive else None,
                                     torch.from_numpy(self.lengths).to(device))
        return t


def ctc_keyword_spotter(inputs, sequence_length, keywords):
    """Where each keyword of `keywords` (a KeywordSet) reads best inside each
    row of inputs [T, B, C], on the first sequence_length[b] frames, free start
    and free end (ocrk_ctc_spot; no reference graph op: what
    src/extract_fields/extractor.py does on the host with fuzzy regexes over the
    decoded string). Returns (score f32 [B, K]: ln of p(the best path spelling
    the keyword on frames [first, end)) / p(the greedy path on those frames),
    <= 0 and 0 when the greedy path spells it; span i32 [B, K, 2]: (first, end),
    for frames_to_px). A keyword that does not fit the row has -inf and
    (-1, -1). With case_insensitive keywords a run of one position may switch
    between the two cases ("tT" reads as one "t"). Device tensors, no host sync."""
    lab, alt, ln = keywords.tensors(inputs.device)
    score, span, _status = K.ctc_spot(_f32(inputs), sequence_length.to(torch.int32).contiguous(), lab, alt, ln)
    return score, span


MAX_KEYWORD_ERRORS = 2                                      # ocrk_ctc_spot_fuzzy: layers of the lattice in registers


class FuzzyKeywordSet(KeywordSet):
    """A KeywordSet whose keywords may be found with edits: max_errors is the
    number of substituted, inserted or deleted symbols allowed per keyword, one
    int for all, one per keyword, or "auto": min(2, (len + 1) // 5), the
    reference's FuzzyRegexExtractor(maxerr=(len + 1) / 5) capped at the
    kernel's two. ValueError for a budget outside 0..min(2, len - 1) (and
    KeywordSet's own). Pickles as its arguments."""

    def __init__(self, keywords, max_errors="auto", case_insensitive=False):
        super().__init__(keywords, case_insensitive)
        lengths = [int(n) for n in self.lengths]
        if isinstance(max_errors, str):
            if max_errors != "auto":
                raise ValueError(f"FuzzyKeywordSet: max_errors is 'auto', an int or one int per keyword, "
                                 f"not {max_errors!r}")
            budgets = [min(MAX_KEYWORD_ERRORS, (n + 1) // 5) for n in lengths]
        elif isinstance(max_errors, (int, np.integer)) and not isinstance(max_errors, bool):
            budgets = [int(max_errors)] * len(lengths)
        else:
            try:
                budgets = list(max_errors)
            except TypeError:
                raise ValueError(f"FuzzyKeywordSet: max_errors is 'auto', an int or one int per keyword, "
                                 f"not {type(max_errors).__name__}") from None
            if len(budgets) != len(lengths):
                raise ValueError(f"FuzzyKeywordSet: {len(budgets)} budgets for {len(lengths)} keywords")
            for i, e in enumerate(budgets):
                if isinstance(e, bool) or not isinstance(e, (int, np.integer)):
                    raise ValueError(f"FuzzyKeywordSet: the budget of entry {i} is {type(e).__name__}, not an int")
            budgets = [int(e) for e in budgets]
        for i, (e, n) in enumerate(zip(budgets, lengths)):
            if not 0 <= e <= min(MAX_KEYWORD_ERRORS, n - 1):
                raise ValueError(f"FuzzyKeywordSet: {self.keywords[i]!r} (entry {i}) takes 0.."
                                 f"{min(MAX_KEYWORD_ERRORS, n - 1)} errors, not {e}")
        self.max_errors = max_errors if isinstance(max_errors, str) else tuple(budgets)
        self.errors = np.array(budgets, np.int32)

    def __reduce__(self):
        arg = self.max_errors if isinstance(self.max_errors, str) else list(self.max_errors)
        return (FuzzyKeywordSet, (list(self.keywords), arg, self.case_insensitive))

    def fuzzy_tensors(self, device):
        """KeywordSet.tensors(device) and the budgets i32 [n] on `device`, uploaded once per device."""
        key = "errors:" + str(torch.device(device))
        t = self._device.get(key)
        if t is None:
            t = self._device[key] = torch.from_numpy(self.errors).to(device)
        return self.tensors(device) + (t,)


def ctc_fuzzy_keyword_spotter(inputs, sequence_length, keywords, edit_cost=0.0):
    """ctc_keyword_spotter with edits: where each keyword of `keywords` (a
    FuzzyKeywordSet) reads best inside each row of inputs [T, B, C] when up to
    its budget of symbols may be substituted, inserted or (inside the keyword)
    deleted (ocrk_ctc_spot_fuzzy; src/extract_fields/extractor.py's
    FuzzyRegexExtractor, on the lattice instead of the decoded string). A
    substituted or inserted symbol reads as the frames' best non-blank class
    and costs nothing beyond edit_cost (>= 0, a log likelihood ratio charged
    once per edit). Returns (score f32 [B, K], <= 0 and 0 when the greedy path
    spells the keyword within its budget and edit_cost is 0; span i32 [B, K, 2];
    errors i32 [B, K]: the edits the best path used, -1 with -inf and (-1, -1)
    where there is no path). Device tensors, no host sync."""
    if not isinstance(keywords, FuzzyKeywordSet):
        raise TypeError(f"ctc_fuzzy_keyword_spotter takes a FuzzyKeywordSet, not {type(keywords).__name__}")
    edit_cost = float(edit_cost)
    if not edit_cost >= 0:
        raise ValueError(f"ctc_fuzzy_keyword_spotter: edit_cost is at least 0 (got {edit_cost})")
    lab, alt, ln, err = keywords.fuzzy_tensors(inputs.device)
    score, span, errors, _status = K.ctc_spot_fuzzy(_f32(inputs), sequence_length.to(torch.int32).contiguous(), lab,
                                                    alt, ln, err, edit_cost)
    return score, span, errors


_FIELD_SPECIAL ="\\[]{}?.*+()|^$"                          # literals only when escaped
_FIELD_UNSUPPORTED = ".*+()|^$"                             # what a regular expression has and a field pattern lacks


def _field_char(name, pattern, ch):
    if ch not in mjsynth.out_charset:
        raise ValueError(f"FieldSet: {name!r}: {pattern!r} has the character {ch!r} outside the charset")
    return ch


def _field_escape(name, pattern, i):
    """The characters of the escape whose backslash is pattern[i], and the index after it."""
    if i + 1 >= len(pattern):
        raise ValueError(f"FieldSet: {name!r}: {pattern!r} ends in a backslash")
    ch = pattern[i + 1]
    if ch == "d":
        return "0123456789", i + 2
    if ch in _FIELD_SPECIAL or ch == "-":                    # \- for a hyphen inside a class that is no range
        return _field_char(name, pattern, ch), i + 2
    raise ValueError(f"FieldSet: {name!r}: unsupported escape \\{ch} in {pattern!r}")


def _field_class(name, pattern, i):
    """The characters of the class whose '[' is pattern[i], and the index after its ']'."""
    chars = []
    i += 1
    if i < len(pattern) and pattern[i] == "^":
        raise ValueError(f"FieldSet: {name!r}: unsupported negated class in {pattern!r}")
    while True:
        if i >= len(pattern):
            raise ValueError(f"FieldSet: {name!r}: unterminated class in {pattern!r}")
        ch = pattern[i]
        if ch == "]":
            break
        if ch == "\\":
            item, i = _field_escape(name, pattern, i)
        elif ch in _FIELD_SPECIAL:
            raise ValueError(f"FieldSet: {name!r}: {ch!r} inside a class of {pattern!r} is written \\{ch}")
        else:
            item, i = _field_char(name, pattern, ch), i + 1
        if len(item) == 1 and i + 1 < len(pattern) and pattern[i] == "-" and pattern[i + 1] != "]":
            if pattern[i + 1] == "\\":
                hi, i = _field_escape(name, pattern, i + 1)
            elif pattern[i + 1] in _FIELD_SPECIAL:
                raise ValueError(f"FieldSet: {name!r}: {pattern[i + 1]!r} inside a class of {pattern!r} is "
                                 f"written \\{pattern[i + 1]}")
            else:
                hi, i = _field_char(name, pattern, pattern[i + 1]), i + 2
            if len(hi) != 1 or ord(hi) < ord(item):
                raise ValueError(f"FieldSet: {name!r}: bad range {item}-{hi} in {pattern!r}")
            item = "".join(_field_char(name, pattern, chr(c)) for c in range(ord(item), ord(hi) + 1))
        chars.extend(item)
    if not chars:
        raise ValueError(f"FieldSet: {name!r}: empty class in {pattern!r}")
    return "".join(chars), i + 1


def _field_quantifier(name, pattern, i):
    """(m, n, index after) of the quantifier at pattern[i]; (1, 1, i) where there is none."""
    if i < len(pattern) and pattern[i] == "?":
        return 0, 1, i + 1
    if i >= len(pattern) or pattern[i] != "{":
        return 1, 1, i
    j = pattern.find("}", i)
    body = pattern[i + 1:j] if j >= 0 else ""
    parts = body.split(",")
    if j < 0 or len(parts) > 2 or not all(p.isascii() and p.isdigit() for p in parts):
        raise ValueError(f"FieldSet: {name!r}: bad quantifier in {pattern!r} ({{m}} or {{m,n}})")
    m, n = int(parts[0]), int(parts[-1])
    if not m <= n or n - m > MAX_FIELD_OPTIONAL:
        raise ValueError(f"FieldSet: {name!r}: quantifier {{{body}}} in {pattern!r} needs m <= n <= m + "
                         f"{MAX_FIELD_OPTIONAL}")
    return m, n, j + 1


def compile_field(name, pattern):
    """A field pattern as (classes, optional): per position the sorted labels of its class and
    whether the position may be absent. The grammar is deliberately small: a literal character of
    mjsynth.out_charset (the characters \\ [ ] { } ? . * + ( ) | ^ $ only when escaped with a
    backslash), \\d, a class [...] of characters, ranges and escapes without negation, each followed
    by nothing, ?, {m} or {m,n} with n - m <= 3 (m mandatory copies, then n - m optional ones).
    ValueError for anything else, naming the pattern."""
    if not isinstance(pattern, str):
        raise ValueError(f"FieldSet: {name!r} is {type(pattern).__name__}, not a string")
    classes, optional = [], []
    i = 0
    while i < len(pattern):
        ch = pattern[i]
        if ch == "\\":
            chars, i = _field_escape(name, pattern, i)
        elif ch == "[":
            chars, i = _field_class(name, pattern, i)
        elif ch in _FIELD_UNSUPPORTED:
            raise ValueError(f"FieldSet: {name!r}: unsupported {ch!r} in {pattern!r} (escape it for the character)")
        elif ch in _FIELD_SPECIAL:
            raise ValueError(f"FieldSet: {name!r}: stray {ch!r} in {pattern!r} (escape it for the character)")
        else:
            chars, i = _field_char(name, pattern, ch), i + 1
        labels = sorted({mjsynth.out_charset.index(c) for c in chars})
        if len(labels) > MAX_FIELD_CLASS:
            raise ValueError(f"FieldSet: {name!r}: a class of {pattern!r} has {len(labels)} characters "
                             f"(at most {MAX_FIELD_CLASS})")
        m, n, i = _field_quantifier(name, pattern, i)
        classes += [labels] * n
        optional += [False] * m + [True] * (n - m)
    if not 1 <= len(classes) <= MAX_FIELD_LEN:
        raise ValueError(f"FieldSet: {name!r}: {pattern!r} has {len(classes)} positions (1..{MAX_FIELD_LEN})")
    if optional[0]:
        raise ValueError(f"FieldSet: {name!r}: {pattern!r} begins with an optional position")
    run = 0
    for o in optional:
        run = run + 1 if o else 0
        if run > MAX_FIELD_OPTIONAL:
            raise ValueError(f"FieldSet: {name!r}: {pattern!r} has more than {MAX_FIELD_OPTIONAL} optional "
                             "positions in a row")
    return classes, optional


class FieldSet:
    """Named field patterns to read out of recognised lines (amounts, GST, receipt
    numbers: what src/extract_fields/extractor.py reads with regular expressions
    over the decoded string): a mapping name -> pattern in compile_field's
    grammar, compiled once and kept as dense int32 classes, optional flags and
    lengths per device. ValueError for an empty mapping or a pattern outside the
    grammar or its limits (16 positions, 16 characters per class, a mandatory
    first position, at most 3 optional positions in a row). Pickles as its
    mapping (the device tensors are rebuilt where it lands)."""

    def __init__(self, patterns):
        if not hasattr(patterns, "items"):
            raise TypeError(f"FieldSet: patterns is a mapping name -> pattern, not {type(patterns).__name__}")
        patterns = dict(patterns)
        if not patterns:
            raise ValueError("FieldSet: the pattern mapping is empty")
        for name in patterns:
            if not isinstance(name, str):
                raise ValueError(f"FieldSet: the name {name!r} is {type(name).__name__}, not a string")
        self.patterns = patterns
        self.names = tuple(patterns)
        self.compiled = tuple(compile_field(name, pat) for name, pat in patterns.items())
        self.lengths = np.array([len(c) for c, _ in self.compiled], np.int32)
        width = int(self.lengths.max())
        self.classes = np.full((len(self.compiled), width, MAX_FIELD_CLASS), -1, np.int32)
        self.optional = np.zeros((len(self.compiled), width), np.int32)
        for p, (cls, opt) in enumerate(self.compiled):
            for i, labels in enumerate(cls):
                self.classes[p, i, :len(labels)] = labels
            self.optional[p, :len(opt)] = opt
        self._device = {}

    def __len__(self):
        return len(self.names)

    def __reduce__(self):
        return (FieldSet, (dict(self.patterns),))

    def tensors(self, device):
        """(classes i32 [n, max_len, 16], optional i32 [n, max_len], lengths i32 [n]) on `device`,
        uploaded once per device."""
        key = str(torch.device(device))
        t = self._device.get(key)
        if t is None:
            t = self._device[key] = (torch.from_numpy(self.classes).to(device),
                                     torch.from_numpy(self.optional).to(device),
                                     torch.from_numpy(self.lengths).to(device))
        return t

    def strings(self, text):
        """The string of each row of `text` (int labels [..., max_len], -1 = absent), as a nested list."""
        text = np.asarray(text)
        flat = ["".join(mjsynth.out_charset[l] for l in row if l >= 0) for row in text.reshape(-1, text.shape[-1])]
        return np.array(flat, dtype=object).reshape(text.shape[:-1]).tolist()


def ctc_field_reader(inputs, sequence_length, fields):
    """The best-scoring string matching each pattern of `fields` (a FieldSet)
    inside each row of inputs [T, B, C], on the first sequence_length[b] frames,
    placed anywhere (ocrk_ctc_field; no reference graph op: what
    src/extract_fields/extractor.py does on the host with regular expressions
    over the 1-best string, where one digit misread as its runner-up silently
    changes an amount). Returns (score f32 [B, P]: ln of p(the best path
    spelling a matching string on frames [first, end)) / p(the greedy path on
    those frames), <= 0 and 0 when the greedy path spells one; span i32
    [B, P, 2]: (first, end), for frames_to_px; text i32 [B, P, max_len]: the
    label chosen at each position, -1 for an absent one: FieldSet.strings turns
    it into strings). A pattern that fits the row nowhere has -inf, (-1, -1) and
    -1s. Device tensors, no host sync."""
    cls, opt, ln = fields.tensors(inputs.device)
    score, span, text, _status = K.ctc_field(_f32(inputs), sequence_length.to(torch.int32).contiguous(), cls, opt, ln)
    return score, span, text


class KeyedFieldSet:
    """Named keyed fields to read out of recognised lines: a mapping name ->
    (keywords, pattern), "the string matching `pattern` that follows one of
    `keywords` on the line" (what src/extract_fields/extractor.py's KWDetector /
    KWExtractor pair produces: {'total': [...], 'gst': [...]}), e.g.
    {"total": (["total", "amount", "ttl"], r"[1-9]\\d{0,3}\\.\\d{1,2}")}.
    Each field's keywords are validated and encoded as a KeywordSet does (its
    ValueErrors, its 32-character limit, case_insensitive's alternatives;
    duplicates are judged within a field, so two fields may share a keyword) and
    its pattern goes through compile_field. Kept as one flat keyword list with
    each keyword's field index, and dense int32 tensors per device. ValueError
    for an empty mapping, a value that is not a (keywords, pattern) pair, or
    anything KeywordSet or compile_field refuses. Pickles as its arguments."""

    def __init__(self, mapping, case_insensitive=False):
        if not hasattr(mapping, "items"):
            raise TypeError("KeyedFieldSet: mapping is a mapping name -> (keywords, pattern), "
                            f"not {type(mapping).__name__}")
        mapping = dict(mapping)
        if not mapping:
            raise ValueError("KeyedFieldSet: the mapping is empty")
        self.case_insensitive = bool(case_insensitive)
        sets, compiled, clean = [], [], {}
        for name, value in mapping.items():
            if not isinstance(name, str):
                raise ValueError(f"KeyedFieldSet: the name {name!r} is {type(name).__name__}, not a string")
            if isinstance(value, str) or not hasattr(value, "__len__") or len(value) != 2:
                raise ValueError(f"KeyedFieldSet: {name!r} maps to a pair (keywords, pattern)")
            keywords, pattern = value
            if isinstance(keywords, str) or not hasattr(keywords, "__iter__"):
                raise ValueError(f"KeyedFieldSet: {name!r}: keywords is a sequence of strings, "
                                 f"not {type(keywords).__name__}")
            try:
                sets.append(KeywordSet(keywords, self.case_insensitive))
            except ValueError as e:
                raise ValueError(f"KeyedFieldSet: {name!r}: {e}") from None
            compiled.append(compile_field(name, pattern))
            clean[name] = (list(sets[-1].keywords), pattern)
        self.mapping = clean
        self.names = tuple(clean)
        self.compiled = tuple(compiled)
        self.keywords = tuple(w for s in sets for w in s.keywords)             # the flat list kw_index points into
        self.groups = np.concatenate([np.full(len(s), a, np.int32) for a, s in enumerate(sets)])
        self.kw_lengths = np.concatenate([s.lengths for s in sets])
        self.labels = np.zeros((len(self.keywords), int(self.kw_lengths.max())), np.int32)
        self.alternatives = np.full(self.labels.shape, -1, np.int32)
        k = 0
        for s in sets:
            self.labels[k:k + len(s), :s.labels.shape[1]] = s.labels
            self.alternatives[k:k + len(s), :s.labels.shape[1]] = s.alternatives
            k += len(s)
        self.lengths = np.array([len(c) for c, _ in self.compiled], np.int32)
        width = int(self.lengths.max())
        self.classes = np.full((len(self.compiled), width, MAX_FIELD_CLASS), -1, np.int32)
        self.optional = np.zeros((len(self.compiled), width), np.int32)
        for p, (cls, opt) in enumerate(self.compiled):
            for i, labels in enumerate(cls):
                self.classes[p, i, :len(labels)] = labels
            self.optional[p, :len(opt)] = opt
        self._device = {}

    def __len__(self):
        return len(self.names)

    def __reduce__(self):
        return (KeyedFieldSet, ({n: (list(k), p) for n, (k, p) in self.mapping.items()}, self.case_insensitive))

    def tensors(self, device):
        """(labels i32 [K, max_kw], alternatives i32 [K, max_kw] or None when case-sensitive, keyword
        lengths i32 [K], groups i32 [K], classes i32 [n, max_len, 16], optional i32 [n, max_len], pattern
        lengths i32 [n]) on `device`, uploaded once per device."""
        key = str(torch.device(device))
        t = self._device.get(key)
        if t is None:
            up = lambda a: torch.from_numpy(a).to(device)                    # noqa: E731
            t = self._device[key] = (up(self.labels), up(self.alternatives) if self.case_insensitive else None,
                                     up(self.kw_lengths), up(self.groups), up(self.classes), up(self.optional),
                                     up(self.lengths))
        return t

    strings = FieldSet.strings


def ctc_keyed_field_reader(inputs, sequence_length, keyed, gap_cost=0.0):
    """For each keyed field of `keyed` (a KeyedFieldSet) and each row of inputs
    [T, B, C], on the first sequence_length[b] frames: the jointly best placement
    of one of the field's keywords, then a gap, then a string matching its
    pattern (ocrk_ctc_keyed_field: the keyword / value pairing of
    src/extract_fields/extractor.py, made on the lattice, where "the amount after
    TOTAL" can still be told from "the amount after CASH"). gap_cost >= 0, nats
    per frame between keyword and value: 0 leaves the gap free, a positive value
    prefers the value nearest its keyword. Returns (score f32 [B, P]: <= 0, and 0
    when the greedy path spells a keyword and later a matching string; kw_index
    i32 [B, P]: into keyed.keywords; kw_score f32 [B, P]: the keyword placement's
    own score; span i32 [B, P, 4]: (kw_first, kw_end, first, end) frames, for
    frames_to_px; text i32 [B, P, max_len]: the label chosen at each position,
    -1 for an absent one: keyed.strings turns it into strings). A field with no
    keyword-then-value path in the row has -inf, -1, -inf, -1s and -1s. Device
    tensors, no host sync."""
    lab, alt, ln, grp, cls, opt, pln = keyed.tensors(inputs.device)
    score, span, kw_index, kw_score, text, _ks, _ps = K.ctc_keyed_field(
        _f32(inputs), sequence_length.to(torch.int32).contiguous(), lab, alt, ln, grp, cls, opt, pln, gap_cost)
    return score, kw_index, kw_score, span, text


# Where a frame sits in the crop (src/weinman/model.py:134-163), in input-column
# indices (column c spans c - 0.5 .. c + 0.5). The 3x3 convolutions are 'same'
# except conv1, which is 'valid' and trims one column per side: its column j is
# centred on input column j + 1. pool2 (width 2, stride 2) makes column p from
# conv columns 2p, 2p + 1: centre 2p + 1.5. pool4 and pool6 are width-2,
# stride-1 windows, each moving the centre half a column of its input, i.e. one
# input column: pool4 column q sits at 2q + 2.5 and pool6 column t, the frame,
# at 2t + 3.5 (pool8 pools rows only). Frames are 2 input columns apart, so
# frame t owns 2t + 2.5 .. 2t + 4.5. Cross-check with model.py:152-163's
# T = floor((W - 2) / 2) - 2: for even W the last centre is W - 4.5, the mirror
# of the first (3.5) about the crop's middle (W - 1) / 2; W = 256 gives 3.5 and 251.5.
def frame_center_px(t):
    """Input column on which frame t's pooling footprint is centred."""
    return 2.0 * t + 3.5


def frames_to_px(first, end, width):
    """Input-column extent (x0, x1) of the frames [first, end), clipped to
    [0, width]. Scalars give floats; NumPy arrays (broadcast) give arrays."""
    x0 = np.clip(2.0 * np.asarray(first) + 2.5, 0.0, width)
    x1 = np.clip(2.0 * np.asarray(end) + 2.5, 0.0, width)
    if x0.ndim == 0 and x1.ndim == 0:
        return float(x0), float(x1)
    return x0, x1


def edit_distance(hypothesis, hypothesis_len, truth, truth_len, totals=None):
    """tf.edit_distance(normalize=False) row by row: f32 [B]."""
    hyp = hypothesis.to(torch.int64).contiguous()
    lab = truth.to(torch.int32).contiguous()
    if lab.dim() == 1:
        lab = lab.reshape(lab.shape[0], 0)
    return K.edit_distance(hyp, hypothesis_len.to(torch.int32).contiguous(), lab,
                           truth_len.to(torch.int32).contiguous(), totals)
