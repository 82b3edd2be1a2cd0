"""Drop-in for the width-bucketed recognise service of src/processing/server.py
(Bucket, LocalServer) on the libocrk GPU path.

Semantics kept from the reference:
  * 31 buckets, width ranges (w, w+32] for w = 32, 64, ..., 992 (server.py:63-64);
    a crop is zero-padded (uint8 0, i.e. -0.5 after preprocessing) on the right
    to the bucket's upper width (server.py:29-34);
  * a bucket releases a batch when it holds MORE than batchsize crops or its
    oldest crop waited longer than maxtime (server.py:45);
  * a short batch is topped up with zero crops whose width is widths[0]
    (server.py:123-128); their results are dropped (clientid '-1');
  * one result per crop: (imgid, text) on the client's output queue, text =
    validate._get_string of the -1-filtered labels (server.py:130-141).
Known reference edge cases, reproduced unless fixed deliberately:
  * a crop exactly 32 px wide fits no (w, w+32] bucket; the reference's
    assert(success_count == 1) fails (server.py:114). Here addImage raises
    ValueError; LocalServer(accept_narrow=True) adds a (0, 32] bucket.
  * a 3-channel crop: the reference keeps channel 1 and drops the channel
    axis (server.py:33-35); here channel 1 is kept WITH the axis so the batch
    stays [bs, 32, W, 1].
The model step runs on the GPU: convnet_layers(INFER) -> rnn_layers ->
ctc_greedy_decoder (server.py:83-89), or the beam-search decoder when the
service is built with decoder="beam" (BASELINE config C5, beam 16).
"""
import math
import queue
import time
from collections.abc import Mapping, Sequence
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib, decode, validate
from . import kernels as K
from .config import INFER
from .model import convnet_layers, rnn_layers
from .mjsynth import num_classes

BUCKET_STEP = 32
BUCKET_MAX_WIDTH = 1000


class Bucket:
    """server.py:17-57."""

    def __init__(self, maxtime, batchsize, widthrange):
        self.maxtime = maxtime
        self.batchsize = batchsize
        self.widthrange = widthrange
        self.imgs = []
        self.widths = []
        self.infos = []
        self.oldesttime = None

    def addImgToBucket(self, clientid, imgid, imgtime, img):
        w = img.shape[1]
        if not (self.widthrange[0] < w <= self.widthrange[1]):
            return False
        img = np.asarray(img)
        if img.ndim == 3:
            img = img[:, :, 1:2] if img.shape[2] > 1 else img
        else:
            img = img[:, :, None]
        padded = np.zeros((img.shape[0], self.widthrange[1], 1), np.uint8)
        padded[:, :w] = img
        self.imgs.append(padded)
        self.widths.append(w)
        self.infos.append((clientid, imgid))
        if self.oldesttime is None or imgtime < self.oldesttime:
            self.oldesttime = imgtime
        return True

    def getBatch(self, now=None):
        if not self.imgs:
            return None
        now = time.time() if now is None else now
        if len(self.imgs) > self.batchsize or (now - self.oldesttime) > self.maxtime:
            batch = np.stack(self.imgs[:self.batchsize])
            widths = np.array(self.widths[:self.batchsize], np.int32)
            infos = self.infos[:self.batchsize]
            del self.imgs[:self.batchsize], self.widths[:self.batchsize], self.infos[:self.batchsize]
            self.oldesttime = now          # as the reference (server.py:52)
            return infos, batch, widths
        return None


def fill_batch(infos, batch, widths, bucket_size):
    """server.py:123-128: top a short batch up with zero crops of width widths[0]."""
    n = batch.shape[0]
    if n >= bucket_size:
        return infos, batch, widths
    extra = bucket_size - n
    batch = np.concatenate([batch, np.zeros((extra,) + batch.shape[1:], batch.dtype)])
    widths = np.concatenate([widths, np.full(extra, widths[0], np.int32)])
    return list(infos) + [("-1", "0")] * extra, batch, widths


def _keyword_set(keywords, case_insensitive, who):
    """keywords as a decode.KeywordSet (or None): a KeywordSet as it is, a sequence of strings encoded."""
    if keywords is None or isinstance(keywords, decode.KeywordSet):
        return keywords
    if isinstance(keywords, str) or not isinstance(keywords, Sequence):
        raise TypeError(f"{who}: keywords is a decode.KeywordSet or a sequence of strings, "
                        f"not {type(keywords).__name__}")
    return decode.KeywordSet(keywords, case_insensitive)


def _fuzzy_keyword_set(keywords, errors, who):
    """The keyword set of keywords= with keyword_errors=: without keyword_errors the set as it is (a
    decode.FuzzyKeywordSet keeps its own budgets); with them a decode.FuzzyKeywordSet of the same keywords."""
    if errors is None:
        return keywords
    if keywords is None:
        raise ValueError(f"{who}: keyword_errors needs keywords")
    if isinstance(keywords, decode.FuzzyKeywordSet):
        raise ValueError(f"{who}: the decode.FuzzyKeywordSet has its budgets already; leave keyword_errors out")
    return decode.FuzzyKeywordSet(list(keywords.keywords), errors, keywords.case_insensitive)


def _keyword_edit_cost(value, fuzzy, who):
    value = float(value)
    if not value >= 0:                                       # NaN refused too; +inf allows no edit at all
        raise ValueError(f"{who}: keyword_edit_cost is a log likelihood ratio per edit, at least 0 (got {value})")
    if value and not fuzzy:
        raise ValueError(f"{who}: keyword_edit_cost needs keyword_errors or a decode.FuzzyKeywordSet")
    return value


def _keyword_threshold(value, who):
    value = float(value)
    if not value <= 0:                                       # a score is a log likelihood ratio <= 0 (NaN refused too)
        raise ValueError(f"{who}: keyword_threshold is a log likelihood ratio, at most 0 (got {value})")
    return value


def _field_set(fields, who):
    """fields as a decode.FieldSet (or None): a FieldSet as it is, a mapping name -> pattern compiled."""
    if fields is None or isinstance(fields, decode.FieldSet):
        return fields
    if not isinstance(fields, Mapping):
        raise TypeError(f"{who}: fields is a decode.FieldSet or a mapping name -> pattern, "
                        f"not {type(fields).__name__}")
    return decode.FieldSet(fields)


def _field_threshold(value, who):
    value = float(value)
    if not value <= 0:
        raise ValueError(f"{who}: field_threshold is a log likelihood ratio, at most 0 (got {value})")
    return value


def _keyed_set(keyed, case_insensitive, who):
    """keyed_fields as a decode.KeyedFieldSet (or None): a KeyedFieldSet as it is, a mapping
    name -> (keywords, pattern) encoded with case_insensitive."""
    if keyed is None or isinstance(keyed, decode.KeyedFieldSet):
        return keyed
    if not isinstance(keyed, Mapping):
        raise TypeError(f"{who}: keyed_fields is a decode.KeyedFieldSet or a mapping name -> (keywords, pattern), "
                        f"not {type(keyed).__name__}")
    return decode.KeyedFieldSet(keyed, case_insensitive)


def _keyed_threshold(value, who):
    value = float(value)
    if not value <= 0:
        raise ValueError(f"{who}: keyed_threshold is a log likelihood ratio, at most 0 (got {value})")
    return value


def _keyed_gap_cost(value, who):
    value = float(value)
    if not 0 <= value < math.inf:                            # NaN refused too
        raise ValueError(f"{who}: keyed_gap_cost is in nats per frame, at least 0 and finite (got {value})")
    return value


def _checked_batch(batch):
    if batch.dtype != torch.uint8 or batch.dim() != 4:
        raise TypeError(f"Recognizer: a batch tensor is uint8 [bs, 32, W, 1], not {batch.dtype} {list(batch.shape)}")
    return batch


def _checked_widths(widths):
    if widths.dtype != torch.int32 or widths.dim() != 1:
        raise TypeError(f"Recognizer: a widths tensor is int32 [bs], not {widths.dtype} {list(widths.shape)}")
    return widths


def _device_batch(batch, dev):
    """The batch on the recogniser's device: a tensor (page.page_crops's views) as it is, NumPy uploaded."""
    if isinstance(batch, torch.Tensor):
        return _checked_batch(batch).to(dev, non_blocking=True).contiguous()
    return torch.from_numpy(np.ascontiguousarray(batch, dtype=np.uint8)).to(dev, non_blocking=True)


def _device_widths(widths, dev):
    if isinstance(widths, torch.Tensor):
        return _checked_widths(widths).to(dev, non_blocking=True).contiguous()
    return torch.from_numpy(np.asarray(widths, np.int32)).to(dev, non_blocking=True)


def _host_widths(widths):
    """widths as float64 NumPy for the pixel extents of results that are read back anyway."""
    if isinstance(widths, torch.Tensor):
        widths = widths.cpu().numpy()
    return np.asarray(widths, np.float64)


class PageLines(NamedTuple):
    """What Recognizer.page returns."""
    results: list                                  # per box what __call__ returns for its crop; None if skipped
    skipped: list                                  # page.PagePlan.skipped: (box index, "empty" | "narrow" | "wide")


class Recognition(NamedTuple):
    """What Recognizer(detail=True) returns per crop (a plain tuple of built-in
    values: it crosses ReplicaPool's and a Manager's queues pickled)."""
    text: str
    confidence: float                              # posterior of the string: exp(-ctc_loss(text | logits))
    char_confidence: Tuple[float, ...]             # per character: its best softmax probability inside its span
    char_px: Tuple[Tuple[float, float], ...]       # per character: (x0, x1) input columns, within [0, width]


class LexiconRecognition(NamedTuple):
    """What Recognizer(lexicon=..., detail=True) returns per crop (built-in values only,
    like Recognition). A crop no word of the lexicon fits (too narrow for all of them) has
    text "", confidence and posterior 0.0 and empty tuples."""
    text: str                                      # the lexicon's best word for the crop
    confidence: float                              # exp(-ctc_loss(text | logits)), Recognition.confidence's meaning
    lexicon_posterior: float                       # p(text) / sum of p(word) over the lexicon
    alternatives: Tuple[Tuple[str, float], ...]    # up to lexicon_top (word, log p), best first; [0] is text
    char_confidence: Tuple[float, ...]             # as Recognition, from the alignment of text
    char_px: Tuple[Tuple[float, float], ...]


class KeywordHit(NamedTuple):
    """One keyword found inside a crop (Recognizer(keywords=...)): built-in values only."""
    keyword: str
    score: float                                   # ln p(best path spelling it there) / p(greedy path there), <= 0
    first_frame: int                               # the first frame of the first symbol
    end_frame: int                                 # one past the last frame of the last symbol
    x0: float                                      # decode.frames_to_px(first_frame, end_frame, width)
    x1: float


class FuzzyKeywordHit(NamedTuple):
    """One keyword found inside a crop with edits allowed (Recognizer(keywords=..., keyword_errors=...)):
    KeywordHit's fields, then the edits of the best path. Built-in values only."""
    keyword: str
    score: float                                   # ln p(best path spelling it within its budget) / p(greedy path)
    first_frame: int
    end_frame: int
    x0: float
    x1: float
    errors: int                                    # substituted, inserted or deleted symbols of that path


class KeywordRecognition(NamedTuple):
    """What Recognizer(keywords=...) returns per crop (built-in values only, like Recognition)."""
    text: str                                      # the string the same recogniser returns without keywords
    detail: Optional[Recognition]                  # the Recognition with detail=True, else None
    hits: Tuple[KeywordHit, ...]                   # score >= keyword_threshold; best first, then by keyword index


class FieldHit(NamedTuple):
    """One field read out of a crop (Recognizer(fields=...)): built-in values only."""
    name: str
    text: str                                      # the best-scoring string matching the field's pattern
    score: float                                   # ln p(best path spelling it there) / p(greedy path there), <= 0
    first_frame: int                               # the first frame of the first symbol
    end_frame: int                                 # one past the last frame of the last symbol
    x0: float                                      # decode.frames_to_px(first_frame, end_frame, width)
    x1: float


class FieldRecognition(NamedTuple):
    """What Recognizer(fields=...) returns per crop (built-in values only, like Recognition)."""
    text: str                                      # the string the same recogniser returns without fields
    detail: Optional[Recognition]                  # the Recognition with detail=True, else None
    hits: Tuple[KeywordHit, ...]                   # as KeywordRecognition.hits when keywords are given too, else ()
    fields: Tuple[FieldHit, ...]                   # score >= field_threshold; best first, then by pattern order


class KeyedHit(NamedTuple):
    """One keyed field read out of a crop (Recognizer(keyed_fields=...)): built-in values only."""
    name: str
    keyword: str                                   # the keyword of the field's group the value was found after
    text: str                                      # the best-scoring string matching the field's pattern after it
    score: float                                   # ln p(best keyword-gap-value path) / p(greedy path there), <= 0
    keyword_score: float                           # the keyword placement's own score, <= 0
    kw_first_frame: int                            # the keyword's frames: first of its first symbol,
    kw_end_frame: int                              # one past the last of its last symbol (<= first_frame)
    kw_x0: float                                   # decode.frames_to_px(kw_first_frame, kw_end_frame, width)
    kw_x1: float
    first_frame: int                               # the value's frames
    end_frame: int
    x0: float                                      # decode.frames_to_px(first_frame, end_frame, width)
    x1: float


class KeyedRecognition(NamedTuple):
    """What Recognizer(keyed_fields=...) returns per crop (built-in values only, like Recognition)."""
    text: str                                      # the string the same recogniser returns without keyed_fields
    detail: Optional[Recognition]                  # the Recognition with detail=True, else None
    hits: Tuple[KeywordHit, ...]                   # as KeywordRecognition.hits when keywords are given too, else ()
    fields: Tuple[FieldHit, ...]                   # as FieldRecognition.fields when fields are given too, else ()
    keyed: Tuple[KeyedHit, ...]                    # score >= keyed_threshold; best first, then in field order


class Recognizer:
    """The per-batch model step of LocalServer.run (server.py:80-89, 132-138):
    uint8 [bs, 32, W, 1] + widths -> one string per crop. Holds the variables
    (a ParamStore) on one GPU.

    Serving precision: the reference serves in float32, and only a float32
    store gives the reference's strings (greedy and beam decodes are identical
    to the oracle's on the golden MJSynth batch; bf16 differs, CER 0.034 greedy /
    0.022 beam-16 there -- bench.py's cer_vs_ref). A bf16 store is refused
    unless allow_bf16=True states that approximate strings are acceptable.

    detail=True: __call__ returns a Recognition per crop instead of a string --
    the same text, its posterior, and each character's confidence and pixel
    extent from the forced alignment of the decoded labels to the same logits
    (decode.ctc_alignment; two more launches per batch, none when False).

    lexicon (a decode.Lexicon or a sequence of strings): closed-vocabulary
    recognition. __call__ returns each crop's most probable lexicon word by
    log p(word | logits) (decode.ctc_lexicon_decoder; "" where no word fits the
    crop) and the unconstrained decoder is not launched; with detail=True a
    LexiconRecognition with the best lexicon_top words.

    keywords (a decode.KeywordSet or a sequence of strings, then encoded with
    case_insensitive): keyword spotting inside the line. __call__ returns a
    KeywordRecognition per crop: the text (and the Recognition with
    detail=True) exactly as without keywords, and a KeywordHit for every
    keyword whose score (decode.ctc_keyword_spotter on the same forward's
    logits: the log likelihood ratio of its best placement against the greedy
    path, <= 0) reaches keyword_threshold (default ln 0.5), with its frames
    and pixel columns. One more entry call per batch (two launches), none
    without keywords. Not combined with lexicon.

    keyword_errors ("auto", an int or one int per keyword; or keywords given
    as a decode.FuzzyKeywordSet): the keywords are found with up to that many
    substituted, inserted or deleted symbols each, keyword_edit_cost (>= 0)
    off the score per edit (decode.ctc_fuzzy_keyword_spotter in place of the
    exact spotter: the same number of launches). The hits of
    KeywordRecognition, FieldRecognition and KeyedRecognition are then
    FuzzyKeywordHit, KeywordHit's fields plus errors, ordered by score
    descending, then errors ascending, then keyword index. The keywords of
    keyed_fields stay exact.

    fields (a decode.FieldSet or a mapping name -> pattern): field reading
    inside the line. __call__ returns a FieldRecognition per crop: text and
    detail exactly as without fields, hits as with keywords alone (() without
    keywords), and a FieldHit for every pattern whose best matching string
    (decode.ctc_field_reader on the same forward's logits) scores at least
    field_threshold (default ln 0.5), with its frames and pixel columns. One
    more entry call per batch (two launches), none without fields. Not
    combined with lexicon.

    keyed_fields (a decode.KeyedFieldSet or a mapping name -> (keywords,
    pattern), then encoded with case_insensitive): a value read after its
    keyword, "the amount after TOTAL". __call__ returns a KeyedRecognition per
    crop: text, detail, hits and fields exactly as without keyed_fields (() for
    what was not asked for), and a KeyedHit for every keyed field whose jointly
    best keyword-gap-value placement (decode.ctc_keyed_field_reader on the same
    forward's logits, with keyed_gap_cost nats per frame of gap) scores at
    least keyed_threshold (default ln 0.5). One more entry call per batch (four
    launches), none without keyed_fields. Not combined with lexicon.

    Wherever a batch and its widths are taken as NumPy arrays, a uint8 device
    tensor [bs, 32, W, 1] and an int32 device tensor [bs] are taken too and read
    where they lie (page() feeds the crops of a whole page this way)."""

    def __init__(self, store, decoder="greedy", beam_width=16, merge_repeated=True, allow_bf16=False,
                 graphs=False, detail=False, lexicon=None, lexicon_top=1, keywords=None,
                 keyword_threshold=math.log(0.5), case_insensitive=False, fields=None,
                 field_threshold=math.log(0.5), keyed_fields=None, keyed_threshold=math.log(0.5),
                 keyed_gap_cost=0.0, keyword_errors=None, keyword_edit_cost=0.0):
        if decoder not in ("greedy", "beam"):
            raise ValueError("decoder is 'greedy' or 'beam'")
        if store.cfg.dtype != torch.float32 and not allow_bf16:
            raise ValueError(f"Recognizer: a {store.cfg.dtype} store does not reproduce the reference's strings "
                             "(float32 does); pass allow_bf16=True to serve approximate decodes")
        self.store = store
        self.decoder = decoder
        self.beam_width = beam_width
        self.merge_repeated = merge_repeated
        self.graphs = {} if graphs else None      # batch shape (+ "logits": no decoder) -> infer.InferGraph
        self.detail = bool(detail)
        if lexicon is not None and not isinstance(lexicon, decode.Lexicon):
            if isinstance(lexicon, str) or not isinstance(lexicon, Sequence):
                raise TypeError("Recognizer: lexicon is a decode.Lexicon or a sequence of strings, "
                                f"not {type(lexicon).__name__}")
            lexicon = decode.Lexicon(lexicon)
        if not 1 <= int(lexicon_top) <= 32:
            raise ValueError("Recognizer: lexicon_top is 1..32")
        self.lexicon = lexicon
        self.lexicon_top = int(lexicon_top)
        self.keywords = _fuzzy_keyword_set(_keyword_set(keywords, case_insensitive, "Recognizer"), keyword_errors,
                                           "Recognizer")
        self.fuzzy_keywords = isinstance(self.keywords, decode.FuzzyKeywordSet)
        self.keyword_edit_cost = _keyword_edit_cost(keyword_edit_cost, self.fuzzy_keywords, "Recognizer")
        if self.keywords is not None and lexicon is not None:
            raise ValueError("Recognizer: keywords and lexicon are two different questions; pass one of them")
        self.keyword_threshold = _keyword_threshold(keyword_threshold, "Recognizer")
        self.fields = _field_set(fields, "Recognizer")
        if self.fields is not None and lexicon is not None:
            raise ValueError("Recognizer: fields and lexicon are two different questions; pass one of them")
        self.field_threshold = _field_threshold(field_threshold, "Recognizer")
        self.keyed_fields = _keyed_set(keyed_fields, case_insensitive, "Recognizer")
        if self.keyed_fields is not None and lexicon is not None:
            raise ValueError("Recognizer: keyed_fields and lexicon are two different questions; pass one of them")
        self.keyed_threshold = _keyed_threshold(keyed_threshold, "Recognizer")
        self.keyed_gap_cost = _keyed_gap_cost(keyed_gap_cost, "Recognizer")

    def _graphed(self, batch, widths, decoded=True):
        """decoded=False: the forward alone (the lexicon path launches no unconstrained decoder)."""
        shape = tuple(batch.shape)
        key = shape if decoded else shape + ("logits",)
        g = self.graphs.get(key)
        if g is None or g.version != self.store.version:
            from .infer import InferGraph
            g = self.graphs[key] = InferGraph(self.store, batch=shape[0], width=shape[2],
                                              decoder="greedy" if decoded and self.decoder == "greedy" else None,
                                              merge_repeated=self.merge_repeated)
        if not isinstance(batch, torch.Tensor):
            batch = torch.from_numpy(np.ascontiguousarray(batch, dtype=np.uint8))
        if not isinstance(widths, torch.Tensor):
            widths = torch.from_numpy(np.asarray(widths, np.int32))
        return g.run(_checked_batch(batch), _checked_widths(widths))

    def labels(self, batch, widths):
        """Dense int64 [bs, max_len] (-1 padded) device tensor. graphs=True: the
        forward of each (bs, W) bucket shape is captured once (infer.InferGraph)
        and replayed per batch."""
        dev = self.store.device
        if self.graphs is not None:
            g = self._graphed(batch, widths)
            if self.decoder == "greedy":
                width = int(g.decoded_len.max().item()) if g.decoded_len.numel() else 0
                return g.decoded[:, :width].clone()
            out, _ = decode.ctc_beam_search_decoder(g.logits, g.seq_len, self.beam_width, 1, self.merge_repeated)
            return out[0]
        with torch.no_grad():
            image = _device_batch(batch, dev)
            width = _device_widths(widths, dev)
            features, seq_len = convnet_layers(image, width, INFER, self.store)
            logits = rnn_layers(features, seq_len, num_classes(), self.store)
            if self.decoder == "greedy":
                return validate._get_output(logits, seq_len, self.merge_repeated)[0]
            out, _ = decode.ctc_beam_search_decoder(logits, seq_len, self.beam_width, 1, self.merge_repeated)
            return out[0]

    def _decoded(self, batch, widths):
        """(logits [T, bs, C], seq_len [bs], out i64 [bs, T] (labels then -1),
        out_len i32 [bs]): the launches of labels(), keeping what the alignment needs."""
        dev = self.store.device
        if self.graphs is not None:
            g = self._graphed(batch, widths)
            logits, seq_len = g.logits, g.seq_len
            if self.decoder == "greedy":
                return logits, seq_len, g.decoded, g.decoded_len
        else:
            with torch.no_grad():
                image = _device_batch(batch, dev)
                width = _device_widths(widths, dev)
                features, seq_len = convnet_layers(image, width, INFER, self.store)
                logits = rnn_layers(features, seq_len, num_classes(), self.store)
            if self.decoder == "greedy":
                out, out_len, _ = decode.ctc_greedy_decoder_raw(logits, seq_len, self.merge_repeated)
                return logits, seq_len, out, out_len
        out, out_len, _ = decode.ctc_beam_search_decoder_raw(logits, seq_len, self.beam_width, 1, self.merge_repeated)
        return logits, seq_len, out[0], out_len[0]

    def recognitions(self, batch, widths):
        """One Recognition per crop. A row whose decode cannot be aligned (only
        a greedy decode with merge_repeated=False can be infeasible: 'aa' read
        from two adjacent frames) keeps its text with confidence 0.0, zero
        character confidences and (0.0, 0.0) extents; the CTC bits such a row
        sets in the device status word are cleared here."""
        return self._recognitions(*self._decoded(batch, widths), widths)

    def _recognitions(self, logits, seq_len, out, out_len, widths):
        with torch.no_grad():
            n_max = int(out_len.max().item()) if out_len.numel() else 0
            lab, ln = decode._masked_labels(out[:, :n_max], out_len)
            logits = decode._f32(logits)
            seq = seq_len.to(torch.int32).contiguous()
            _fs, span, conf, _logp, status = K.ctc_align(logits, lab, ln, seq)
            loss, _, _ = K.ctc_loss(logits, lab, ln, seq, need_grad=False)
            # two read-backs (one per dtype), then whole-array host work: a crop costs no per-character NumPy call
            ints = torch.cat([lab, span.reshape(lab.shape[0], -1), ln[:, None], status[:, None]], dim=1).cpu().numpy()
            flts = torch.cat([conf, loss[:, None]], dim=1).cpu().numpy()
        lab, span = ints[:, :n_max], ints[:, n_max:3 * n_max].reshape(-1, n_max, 2)
        ln, status = ints[:, -2].tolist(), ints[:, -1].tolist()
        if any(status):
            K.clear_status(self.store.device, _lib.STATUS_CTC)
        x0, x1 = decode.frames_to_px(span[:, :, 0], span[:, :, 1], _host_widths(widths)[:, None])
        px = np.stack([x0, x1], axis=2).tolist()
        conf, loss, lab = flts[:, :n_max].tolist(), flts[:, -1].tolist(), lab.tolist()
        res = []
        for b, n in enumerate(ln):
            text = validate._get_string(lab[b][:n])
            if status[b] != 0:
                res.append(Recognition(text, 0.0, (0.0,) * n, ((0.0, 0.0),) * n))
                continue
            res.append(Recognition(text, math.exp(-loss[b]), tuple(conf[b][:n]), tuple(map(tuple, px[b][:n]))))
        return res

    def _lexicon_top(self, batch, widths, top_k):
        """(logits f32 [T, bs, C], seq_len i32 [bs], index [bs, top_k], log p [bs, top_k], log_norm [bs]):
        the forward (the replayed graph's, with graphs=True) and the lexicon scoring on its logits."""
        if self.graphs is not None:
            g = self._graphed(batch, widths, decoded=False)
            logits, seq_len = g.logits, g.seq_len
        else:
            dev = self.store.device
            with torch.no_grad():
                image = _device_batch(batch, dev)
                width = _device_widths(widths, dev)
                features, seq_len = convnet_layers(image, width, INFER, self.store)
                logits = rnn_layers(features, seq_len, num_classes(), self.store)
        with torch.no_grad():
            logits = decode._f32(logits)
            seq = seq_len.to(torch.int32).contiguous()
            idx, logp, log_norm = decode.ctc_lexicon_decoder(logits, seq, self.lexicon, top_k)
        return logits, seq, idx, logp, log_norm

    def lexicon_words(self, batch, widths):
        """The most probable lexicon word per crop ("" where no word fits the crop's frames)."""
        idx = self._lexicon_top(batch, widths, 1)[2]
        words = self.lexicon.words
        return [words[i] if i >= 0 else "" for i in idx[:, 0].tolist()]

    def lexicon_recognitions(self, batch, widths):
        """One LexiconRecognition per crop: the lexicon_top best words, and the best one
        aligned to the logits as recognitions() aligns the decoded string."""
        logits, seq, idx, logp, log_norm = self._lexicon_top(batch, widths, self.lexicon_top)
        k = self.lexicon_top
        with torch.no_grad():
            lab_all, ln_all = self.lexicon.tensors(logits.device)
            found = idx[:, 0] >= 0
            best = idx[:, 0].clamp(min=0).long()
            lab = lab_all[best].contiguous()
            ln = torch.where(found, ln_all[best], torch.zeros_like(ln_all[best])).contiguous()
            _fs, span, conf, _logp, status = K.ctc_align(logits, lab, ln, seq)
            n_max = lab.shape[1]
            ints = torch.cat([idx, span.reshape(lab.shape[0], -1), ln[:, None], status[:, None]], dim=1).cpu().numpy()
            flts = torch.cat([logp, log_norm[:, None], conf], dim=1).cpu().numpy()
        idx, span = ints[:, :k].tolist(), ints[:, k:k + 2 * n_max].reshape(-1, n_max, 2)
        ln, status = ints[:, -2].tolist(), ints[:, -1].tolist()
        if any(status):                                     # a row without a word and without frames (seq_len 0)
            K.clear_status(self.store.device, _lib.STATUS_CTC)
        x0, x1 = decode.frames_to_px(span[:, :, 0], span[:, :, 1], _host_widths(widths)[:, None])
        px = np.stack([x0, x1], axis=2).tolist()
        logp, log_norm, conf = flts[:, :k].tolist(), flts[:, k].tolist(), flts[:, k + 1:].tolist()
        words = self.lexicon.words
        res = []
        for b, n in enumerate(ln):
            if idx[b][0] < 0:
                res.append(LexiconRecognition("", 0.0, 0.0, (), (), ()))
                continue
            alts = tuple((words[i], lp) for i, lp in zip(idx[b], logp[b]) if i >= 0)
            if status[b] != 0:
                cc, cp = (0.0,) * n, ((0.0, 0.0),) * n
            else:
                cc, cp = tuple(conf[b][:n]), tuple(map(tuple, px[b][:n]))
            res.append(LexiconRecognition(words[idx[b][0]], math.exp(logp[b][0]), math.exp(logp[b][0] - log_norm[b]),
                                          alts, cc, cp))
        return res

    def keyword_recognitions(self, batch, widths):
        """One KeywordRecognition per crop: the decode of labels() / recognitions(), and the spotting
        launch on the same forward's logits (the replayed graph's, with graphs=True). A keyword that
        does not fit a crop's frames has no place and is never a hit."""
        return self._keyword_recognitions(*self._decoded(batch, widths), widths)

    def _texts(self, logits, seq_len, out, out_len, widths):
        """(texts, details) of a decoded batch: the Recognitions with detail=True, else None per crop."""
        if self.detail:
            details = self._recognitions(logits, seq_len, out, out_len, widths)
            return [d.text for d in details], details
        rows, lens = out.cpu().numpy(), out_len.cpu().tolist()           # labels then -1: the first out_len count
        return [validate._get_string(row[:n]) for row, n in zip(rows, lens)], [None] * len(widths)

    def _keyword_recognitions(self, logits, seq_len, out, out_len, widths):
        if self.fuzzy_keywords:
            return self._fuzzy_keyword_recognitions(logits, seq_len, out, out_len, widths)
        with torch.no_grad():
            score, span = decode.ctc_keyword_spotter(logits, seq_len, self.keywords)
        texts, details = self._texts(logits, seq_len, out, out_len, widths)
        score, span = score.cpu().numpy(), span.cpu().numpy()
        # whole-array host work on the hits alone: by crop, then score descending, then keyword index
        bs, ks = np.nonzero((score >= self.keyword_threshold) & (span[:, :, 0] >= 0))
        order = np.lexsort((ks, -score[bs, ks], bs))
        bs, ks = bs[order], ks[order]
        first, end = span[bs, ks, 0], span[bs, ks, 1]
        x0, x1 = decode.frames_to_px(first, end, _host_widths(widths)[bs])
        words = self.keywords.keywords
        hits = [[] for _ in texts]
        for b, k, s, f, e, a0, a1 in zip(bs.tolist(), ks.tolist(), score[bs, ks].tolist(), first.tolist(),
                                         end.tolist(), np.atleast_1d(x0).tolist(), np.atleast_1d(x1).tolist()):
            hits[b].append(KeywordHit(words[k], s, f, e, a0, a1))
        return [KeywordRecognition(text, d, tuple(h)) for text, d, h in zip(texts, details, hits)]

    def _fuzzy_keyword_recognitions(self, logits, seq_len, out, out_len, widths):
        """_keyword_recognitions with the error-tolerant spotter: FuzzyKeywordHits, by score descending, then
        errors ascending, then keyword index."""
        with torch.no_grad():
            score, span, errors = decode.ctc_fuzzy_keyword_spotter(logits, seq_len, self.keywords,
                                                                   self.keyword_edit_cost)
        texts, details = self._texts(logits, seq_len, out, out_len, widths)
        score, span, errors = score.cpu().numpy(), span.cpu().numpy(), errors.cpu().numpy()
        bs, ks = np.nonzero((score >= self.keyword_threshold) & (span[:, :, 0] >= 0))
        order = np.lexsort((ks, errors[bs, ks], -score[bs, ks], bs))
        bs, ks = bs[order], ks[order]
        first, end = span[bs, ks, 0], span[bs, ks, 1]
        x0, x1 = decode.frames_to_px(first, end, _host_widths(widths)[bs])
        words = self.keywords.keywords
        hits = [[] for _ in texts]
        for b, k, s, f, e, a0, a1, n in zip(bs.tolist(), ks.tolist(), score[bs, ks].tolist(), first.tolist(),
                                            end.tolist(), np.atleast_1d(x0).tolist(), np.atleast_1d(x1).tolist(),
                                            errors[bs, ks].tolist()):
            hits[b].append(FuzzyKeywordHit(words[k], s, f, e, a0, a1, n))
        return [KeywordRecognition(text, d, tuple(h)) for text, d, h in zip(texts, details, hits)]

    def field_recognitions(self, batch, widths):
        """One FieldRecognition per crop: what keyword_recognitions() (with keywords) or labels() /
        recognitions() give, and the field-reading launch on the same forward's logits (the replayed
        graph's, with graphs=True). A pattern that fits a crop's frames nowhere is never a hit."""
        return self._field_recognitions(self._decoded(batch, widths), widths)

    def _field_recognitions(self, decoded, widths):
        logits, seq_len = decoded[0], decoded[1]
        with torch.no_grad():
            score, span, text = decode.ctc_field_reader(logits, seq_len, self.fields)
        if self.keywords is not None:
            base = [(r.text, r.detail, r.hits) for r in self._keyword_recognitions(*decoded, widths)]
        else:
            base = [(t, d, ()) for t, d in zip(*self._texts(*decoded, widths))]
        score, span, text = score.cpu().numpy(), span.cpu().numpy(), text.cpu().numpy()
        # whole-array host work on the hits alone: by crop, then score descending, then pattern order
        bs, ps = np.nonzero((score >= self.field_threshold) & (span[:, :, 0] >= 0))
        order = np.lexsort((ps, -score[bs, ps], bs))
        bs, ps = bs[order], ps[order]
        first, end = span[bs, ps, 0], span[bs, ps, 1]
        x0, x1 = decode.frames_to_px(first, end, _host_widths(widths)[bs])
        strings = self.fields.strings(text[bs, ps]) if len(bs) else []
        names = self.fields.names
        found = [[] for _ in base]
        for b, p, w, s, f, e, a0, a1 in zip(bs.tolist(), ps.tolist(), strings, score[bs, ps].tolist(), first.tolist(),
                                            end.tolist(), np.atleast_1d(x0).tolist(), np.atleast_1d(x1).tolist()):
            found[b].append(FieldHit(names[p], w, s, f, e, a0, a1))
        return [FieldRecognition(t, d, h, tuple(f)) for (t, d, h), f in zip(base, found)]

    def keyed_recognitions(self, batch, widths):
        """One KeyedRecognition per crop: what field_recognitions() (with fields), keyword_recognitions()
        (with keywords) or labels() / recognitions() give, and the keyed-field entry on the same forward's
        logits (the replayed graph's, with graphs=True). A keyed field with no keyword-then-value path in
        a crop's frames is never a hit."""
        decoded = self._decoded(batch, widths)
        logits, seq_len = decoded[0], decoded[1]
        with torch.no_grad():
            score, kw_index, kw_score, span, text = decode.ctc_keyed_field_reader(logits, seq_len, self.keyed_fields,
                                                                                  self.keyed_gap_cost)
        if self.fields is not None:
            base = [(r.text, r.detail, r.hits, r.fields) for r in self._field_recognitions(decoded, widths)]
        elif self.keywords is not None:
            base = [(r.text, r.detail, r.hits, ()) for r in self._keyword_recognitions(*decoded, widths)]
        else:
            base = [(t, d, (), ()) for t, d in zip(*self._texts(*decoded, widths))]
        score, kw_index, kw_score = score.cpu().numpy(), kw_index.cpu().numpy(), kw_score.cpu().numpy()
        span, text = span.cpu().numpy(), text.cpu().numpy()
        # whole-array host work on the hits alone: by crop, then score descending, then field order
        bs, ps = np.nonzero((score >= self.keyed_threshold) & (span[:, :, 2] >= 0))
        order = np.lexsort((ps, -score[bs, ps], bs))
        bs, ps = bs[order], ps[order]
        sp = span[bs, ps]
        w = _host_widths(widths)[bs]
        k0, k1 = decode.frames_to_px(sp[:, 0], sp[:, 1], w)
        x0, x1 = decode.frames_to_px(sp[:, 2], sp[:, 3], w)
        strings = self.keyed_fields.strings(text[bs, ps]) if len(bs) else []
        names, words = self.keyed_fields.names, self.keyed_fields.keywords
        found = [[] for _ in base]
        for b, p, k, t, s, ks, fr, a0, a1, c0, c1 in zip(
                bs.tolist(), ps.tolist(), kw_index[bs, ps].tolist(), strings, score[bs, ps].tolist(),
                kw_score[bs, ps].tolist(), sp.tolist(), np.atleast_1d(k0).tolist(), np.atleast_1d(k1).tolist(),
                np.atleast_1d(x0).tolist(), np.atleast_1d(x1).tolist()):
            found[b].append(KeyedHit(names[p], words[k], t, s, ks, fr[0], fr[1], a0, a1, fr[2], fr[3], c0, c1))
        return [KeyedRecognition(t, d, h, f, tuple(k)) for (t, d, h, f), k in zip(base, found)]

    def __call__(self, batch, widths):
        if self.keyed_fields is not None:
            return self.keyed_recognitions(batch, widths)
        if self.fields is not None:
            return self.field_recognitions(batch, widths)
        if self.keywords is not None:
            return self.keyword_recognitions(batch, widths)
        if self.lexicon is not None:
            return self.lexicon_recognitions(batch, widths) if self.detail else self.lexicon_words(batch, widths)
        if self.detail:
            return self.recognitions(batch, widths)
        return validate.decode_strings(self.labels(batch, widths))

    def page(self, page, boxes, normalize=True, bucket_size=16, accept_narrow=False, pad=1):
        """Read a page from its line boxes (pagepredictor.py:274, 319-328, then the bucketing of
        LocalServer): page is uint8 or float32 [H, W] (NumPy, uploaded once, or a device tensor),
        boxes integers [n, 4] of (y0, x0, y1, x1). page.plan_page buckets the boxes, page.page_crops
        cuts, resizes and pads every crop on the device in one launch, and each batch is recognised
        where it lies. Returns PageLines(results, skipped): results[i] is what __call__ returns for
        the crop of box i, None for a box the plan skipped."""
        from . import page as P
        plan = P.plan_page(boxes, tuple(page.shape), bucket_size, accept_narrow, pad)
        results = [None] * plan.n_boxes
        crops = P.page_crops(page, plan, normalize, device=self.store.device)
        for (batch, widths), planned in zip(crops, plan.batches):
            for res, box in zip(self(batch, widths), planned.boxes.tolist()):
                if box >= 0:                                 # a top-up row's result is dropped
                    results[box] = res
        return PageLines(results, plan.skipped)


class LocalServer:
    """server.py:59-145. `recognizer` is a Recognizer (or any callable
    (batch, widths) -> list of strings, or of Recognition tuples with
    Recognizer(detail=True): results are forwarded as they are); queues come from `manager` (a
    multiprocessing Manager, or None for in-process queue.Queue)."""

    def __init__(self, recognizer, manager=None, bucket_size=16, bucket_max_time=1.0, accept_narrow=False):
        self.client_inputs = {}
        self.client_outputs = {}
        self.recognizer = recognizer
        self.manager = manager
        self.bucket_size = bucket_size
        self.buckets = [Bucket(bucket_max_time, bucket_size, (w, w + BUCKET_STEP))
                        for w in range(BUCKET_STEP, BUCKET_MAX_WIDTH, BUCKET_STEP)]
        if accept_narrow:
            self.buckets.insert(0, Bucket(bucket_max_time, bucket_size, (0, BUCKET_STEP)))
        self.maxclientid = 0
        self.batches_run = 0
        self._inflight = {}                # batch id -> infos (asynchronous recognizers)
        self._next_batch = 0

    def _queue(self):
        return self.manager.Queue() if self.manager is not None else queue.Queue()

    def register(self):
        clientid = str(self.maxclientid)
        self.maxclientid += 1
        self.client_inputs[clientid] = self._queue()
        self.client_outputs[clientid] = self._queue()
        return clientid, self.client_inputs[clientid], self.client_outputs[clientid]

    def addImage(self, clientid, imgid, imgtime, img):
        hits = sum(b.addImgToBucket(clientid, imgid, imgtime, img) for b in self.buckets)
        if hits != 1:                                   # server.py:114 assert(success_count == 1)
            raise ValueError(f"crop of width {img.shape[1]} fits {hits} buckets (needs exactly 1)")

    def poll_inputs(self, idle_sleep=0.0):
        got = False
        for clientid, q in list(self.client_inputs.items()):
            try:
                imgid, imgtime, img = q.get(block=False)
            except queue.Empty:
                if idle_sleep:
                    time.sleep(idle_sleep)
                continue
            self.addImage(clientid, imgid, imgtime, img)
            got = True
        return got

    def _deliver(self, infos, texts):
        for (clientid, imgid), txt in zip(infos, texts):
            if clientid == "-1":
                continue
            self.client_outputs[clientid].put((imgid, txt), block=False)

    def flush_buckets(self, now=None):
        """Run every bucket that is ready; returns the number of batches run
        (submitted, for an asynchronous recognizer such as ReplicaPool)."""
        n = 0
        for bi, bucket in enumerate(self.buckets):
            b = bucket.getBatch(now)
            if b is None:
                continue
            infos, batch, widths = fill_batch(*b, self.bucket_size)
            if hasattr(self.recognizer, "submit"):
                bid = self._next_batch
                self._next_batch += 1
                self._inflight[bid] = infos
                self.recognizer.submit(bi, bid, batch, widths)
            else:
                self._deliver(infos, self.recognizer(batch, widths))
            n += 1
        self.batches_run += n
        self.collect()
        return n

    def collect(self, block=False):
        """Forward the results an asynchronous recognizer has finished
        (block=True: wait until every submitted batch is back)."""
        if not hasattr(self.recognizer, "poll"):
            return 0
        n = 0
        while self._inflight:
            done = self.recognizer.poll(block=block)
            if not done:
                break
            for bid, texts in done:
                self._deliver(self._inflight.pop(bid), texts)
                n += 1
        return n

    def run(self, states=None, logger=None, stop=None, idle_sleep=0.1):
        """server.py:94-145 main loop; returns when `stop()` is true."""
        if states is not None:
            states["server_started"] = True
        if logger is not None:
            logger.info("server started, waiting image ...")
        while stop is None or not stop():
            try:
                self.poll_inputs(idle_sleep)
                self.flush_buckets()
                self.collect()
            except Exception:
                if logger is None:
                    raise
                logger.exception("SERVER ERROR")


# ------------------------------------------------------- multi-GPU replicas
def _replica_main(rank, device, make_recognizer, inq, outq):
    """Worker process of a ReplicaPool: one recognizer on one device; batches
    in, ("result", batch id, texts) out, until a None item arrives. The
    replica's GPU is made the CURRENT device before anything else, so every
    per-device launch setting of libocrk (kernel LDS limits, CU counts, the
    persistent kernels' co-residency checks) is taken on that GPU and the
    process never initialises cuda:0 by accident."""
    try:
        if isinstance(device, (str, torch.device)) and str(device).startswith("cuda"):
            torch.cuda.set_device(torch.device(device))
        rec = make_recognizer(device)
    except BaseException as e:                       # reported to the pool, which raises
        outq.put(("init_error", rank, f"{type(e).__name__}: {e}"))
        return
    outq.put(("ready", rank, None))
    while True:
        item = inq.get()
        if item is None:
            break
        bid, batch, widths = item
        try:
            outq.put(("result", bid, list(rec(batch, widths))))
        except Exception as e:                        # reported to the server, which raises
            outq.put(("error", bid, f"{type(e).__name__}: {e}"))
    outq.put(("exit", rank, None))


def gpu_recognizer(cfg=None, checkpoint=None, seed=0, decoder="greedy", beam_width=16, allow_bf16=False,
                   detail=False, lexicon=None, lexicon_top=1, keywords=None, keyword_threshold=math.log(0.5),
                   case_insensitive=False, fields=None, field_threshold=math.log(0.5), keyed_fields=None,
                   keyed_threshold=math.log(0.5), keyed_gap_cost=0.0, keyword_errors=None, keyword_edit_cost=0.0):
    """A make_recognizer for ReplicaPool: a Recognizer whose ParamStore is
    built on the replica's device (restored from a TF1 checkpoint, or the
    reference initialisers with `seed`). Picklable (spawn); a lexicon or a
    keyword list travels as its plain list of strings, field patterns as their plain
    mapping, keyed fields as their plain mapping too, and they are encoded in the replica."""
    return _GpuRecognizerFactory(cfg, checkpoint, seed, decoder, beam_width, allow_bf16, detail, lexicon, lexicon_top,
                                 keywords, keyword_threshold, case_insensitive, fields, field_threshold, keyed_fields,
                                 keyed_threshold, keyed_gap_cost, keyword_errors, keyword_edit_cost)


class _GpuRecognizerFactory:
    def __init__(self, cfg, checkpoint, seed, decoder, beam_width, allow_bf16=False, detail=False, lexicon=None,
                 lexicon_top=1, keywords=None, keyword_threshold=math.log(0.5), case_insensitive=False,
                 fields=None, field_threshold=math.log(0.5), keyed_fields=None, keyed_threshold=math.log(0.5),
                 keyed_gap_cost=0.0, keyword_errors=None, keyword_edit_cost=0.0):
        self.cfg, self.checkpoint, self.seed, self.decoder, self.beam_width = cfg, checkpoint, seed, decoder, beam_width
        self.allow_bf16, self.detail = allow_bf16, detail
        if lexicon is not None:                             # checked here, in the parent; pickled as strings
            lexicon = list(decode.Lexicon(lexicon).words if not isinstance(lexicon, decode.Lexicon) else lexicon.words)
        self.lexicon, self.lexicon_top = lexicon, lexicon_top
        kws = _fuzzy_keyword_set(_keyword_set(keywords, case_insensitive, "gpu_recognizer"), keyword_errors,
                                 "gpu_recognizer")                           # checked here too; pickled as strings
        fuzzy = isinstance(kws, decode.FuzzyKeywordSet)                      # and as its budgets
        self.keyword_errors = [int(e) for e in kws.errors] if fuzzy else None
        self.keyword_edit_cost = _keyword_edit_cost(keyword_edit_cost, fuzzy, "gpu_recognizer")
        if kws is not None and lexicon is not None:
            raise ValueError("gpu_recognizer: keywords and lexicon are two different questions; pass one of them")
        self.keywords = None if kws is None else list(kws.keywords)
        self.case_insensitive = bool(case_insensitive) if kws is None else kws.case_insensitive
        self.keyword_threshold = _keyword_threshold(keyword_threshold, "gpu_recognizer")
        fset = _field_set(fields, "gpu_recognizer")                          # and the patterns; pickled as a mapping
        if fset is not None and lexicon is not None:
            raise ValueError("gpu_recognizer: fields and lexicon are two different questions; pass one of them")
        self.fields = None if fset is None else dict(fset.patterns)
        self.field_threshold = _field_threshold(field_threshold, "gpu_recognizer")
        kset = _keyed_set(keyed_fields, self.case_insensitive, "gpu_recognizer")   # pickled as a mapping
        if kset is not None and lexicon is not None:
            raise ValueError("gpu_recognizer: keyed_fields and lexicon are two different questions; pass one of them")
        self.keyed_fields = None if kset is None else {n: (list(k), p) for n, (k, p) in kset.mapping.items()}
        self.keyed_case_insensitive = self.case_insensitive if kset is None else kset.case_insensitive
        self.keyed_threshold = _keyed_threshold(keyed_threshold, "gpu_recognizer")
        self.keyed_gap_cost = _keyed_gap_cost(keyed_gap_cost, "gpu_recognizer")

    def __call__(self, device):
        from .config import ModelConfig
        from .params import ParamStore
        store = ParamStore(self.cfg or ModelConfig(dtype=torch.float32), device=device, seed=self.seed)
        if self.checkpoint:
            from . import checkpoint as ckpt
            ckpt.restore(store, self.checkpoint)
        return Recognizer(store, decoder=self.decoder, beam_width=self.beam_width, allow_bf16=self.allow_bf16,
                          detail=self.detail, lexicon=self.lexicon, lexicon_top=self.lexicon_top,
                          keywords=self.keywords, keyword_threshold=self.keyword_threshold,
                          case_insensitive=self.case_insensitive, fields=self.fields,
                          field_threshold=self.field_threshold,
                          keyed_fields=None if self.keyed_fields is None else decode.KeyedFieldSet(
                              self.keyed_fields, self.keyed_case_insensitive),
                          keyed_threshold=self.keyed_threshold, keyed_gap_cost=self.keyed_gap_cost,
                          keyword_errors=self.keyword_errors, keyword_edit_cost=self.keyword_edit_cost)


class ReplicaError(RuntimeError):
    """A ReplicaPool worker failed to start, died, or raised on a batch."""


class ReplicaPool:
    """Data-parallel recognise step over several GPUs (inference and
    decode are replicas, no exchange), one worker PROCESS per device. The
    LocalServer stays the single bucketing front end (server.py:59-145, with
    the page workers as its clients, ocr-app.py:186-193); each ready batch is
    sent whole to replica (bucket index mod replicas), so a width bucket -- one
    input shape -- always lands on the same GPU. submit / poll make the
    LocalServer asynchronous: batches of different buckets run on their GPUs
    concurrently. `devices`: e.g. ["cuda:0", ..., "cuda:7"].

    Failures surface as ReplicaError naming the replica: a recognizer that
    cannot be built (reported by the worker), a worker process that dies
    (checked while waiting: its exit code), a batch that raised. The reference
    server instead logs and leaves its loop (server.py:144-145) and relies on
    the app's heartbeat watchdog to restart it (ocr-app.py:219-249)."""

    def __init__(self, devices, make_recognizer, start_method="spawn", timeout=600.0):
        import multiprocessing as mp
        ctx = mp.get_context(start_method)
        self.devices = list(devices)
        self.outq = ctx.Queue()
        self.inqs = [ctx.Queue() for _ in self.devices]
        self.procs = [ctx.Process(target=_replica_main, args=(r, d, make_recognizer, self.inqs[r], self.outq),
                                  daemon=True) for r, d in enumerate(self.devices)]
        self.assigned = {}                                   # batch id -> replica (in flight)
        self._pending = []                                   # results collected by a poll() that raised
        self._closed = False
        for pr in self.procs:
            pr.start()
        ready = set()
        deadline = time.time() + timeout
        while len(ready) < len(self.procs):
            msg = self._get(deadline)
            if msg is None:
                self._abort()
                raise ReplicaError(f"replicas {sorted(set(range(len(self.procs))) - ready)} not ready "
                                   f"after {timeout:.0f} s")
            tag, who, info = msg
            if tag == "ready":
                ready.add(who)
            elif tag == "init_error":
                self._abort()
                raise ReplicaError(f"replica {who} ({self.devices[who]}) failed to start: {info}")

    def _dead(self):
        """(rank, exit code) of the first worker that exited, if any."""
        for r, pr in enumerate(self.procs):
            if not pr.is_alive() and pr.exitcode is not None:
                return r, pr.exitcode
        return None

    def _get(self, deadline):
        """Next message, waiting in short slices while checking that every
        worker is alive (None at the deadline)."""
        while True:
            try:
                return self.outq.get(timeout=0.2)
            except queue.Empty:
                pass
            dead = self._dead()
            if dead is not None and not self._closed:
                try:                                         # a message it sent just before exiting
                    return self.outq.get_nowait()
                except queue.Empty:
                    pass
                self._abort()
                raise ReplicaError(f"replica {dead[0]} ({self.devices[dead[0]]}) died with exit code {dead[1]}; "
                                   f"{len(self.assigned)} batches in flight are lost")
            if deadline is not None and time.time() > deadline:
                return None

    def _abort(self):
        self._closed = True
        for pr in self.procs:
            if pr.is_alive():
                pr.terminate()

    def replica_of(self, bucket_index):
        return bucket_index % len(self.procs)

    def submit(self, bucket_index, batch_id, batch, widths):
        dead = self._dead()
        if dead is not None:
            self._abort()
            raise ReplicaError(f"replica {dead[0]} ({self.devices[dead[0]]}) died with exit code {dead[1]}")
        r = self.replica_of(bucket_index)
        self.assigned[batch_id] = r
        self.inqs[r].put((batch_id, np.ascontiguousarray(batch), np.asarray(widths, np.int32)))

    def _take(self, msg, out):
        """File a result into `out`; a batch error is returned (not raised) so
        poll() can keep the results it has already collected."""
        tag, bid, payload = msg
        if tag == "result":
            self.assigned.pop(bid, None)
            out.append((bid, payload))
        elif tag == "error":
            r = self.assigned.pop(bid, None)
            return ReplicaError(f"replica {r} failed on batch {bid}: {payload}")
        return None                                  # control messages ("ready", "exit") carry no batch

    def poll(self, block=False, timeout=600.0):
        """Finished (batch id, texts) pairs (block: wait for at least one).
        A batch that raised in its replica surfaces as ReplicaError; results
        collected by the same poll are not lost -- they are kept and returned
        by the next poll()."""
        out, err = [], None
        pending, self._pending = self._pending, []
        for m in pending:
            err = self._take(m, out) or err
        while err is None:
            try:
                msg = self.outq.get_nowait()
            except queue.Empty:
                if out or not block or not self.assigned:
                    return out
                msg = self._get(time.time() + timeout)
                if msg is None:
                    self._pending = [("result", bid, texts) for bid, texts in out]
                    raise ReplicaError(f"no result from the replicas within {timeout:.0f} s "
                                       f"({len(self.assigned)} batches in flight)")
            err = self._take(msg, out)
        self._pending = [("result", bid, texts) for bid, texts in out]
        raise err

    def close(self):
        self._closed = True
        for q in self.inqs:
            q.put(None)
        for pr in self.procs:
            pr.join(timeout=60)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def predict_signature(store, images, width, beam_width=128, top_paths=3, merge_repeated=False):
    """The serving signature src/weinman/client.py consumes (model 'clreceipt',
    inputs 'images' u8 [bs, 32, W, 1] and 'width' i32 [bs]; client.py:101-123):
    'output0' = beam log-probabilities [bs, top_paths], 'output1'..'output<top_paths>'
    = the decoded paths as dense int64 [bs, len] (-1 padded), from
    ctc_beam_search_decoder(beam_width=128, merge_repeated=False) (client.py:222-233)."""
    dev = store.device
    with torch.no_grad():
        image = torch.as_tensor(np.asarray(images, np.uint8)).to(dev)
        w = torch.as_tensor(np.asarray(width, np.int32)).to(dev)
        features, seq_len = convnet_layers(image, w, INFER, store)
        logits = rnn_layers(features, seq_len, num_classes(), store)
        paths, logp = decode.ctc_beam_search_decoder(logits, seq_len, beam_width, top_paths, merge_repeated)
    out = {"output0": logp.cpu().numpy()}
    for k, p in enumerate(paths, start=1):
        out[f"output{k}"] = p.cpu().numpy()
    return out
