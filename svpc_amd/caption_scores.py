"""Host compilation for Bleu_1…4, ROUGE_L and CIDEr of decoded captions on the device.

reference: src/train.py:278-331 (eval_language_metrics) runs densevid_eval/para-evaluate.py, whose scorers are the public caption
scorer's Bleu(4) (option ``closest``), Rouge (β = 1.2) and Cider() (n = 4, σ = 6); METEOR is out of scope.  That scorer is not part of the
reference checkout, so the published definitions (restated by tests/caption_scores_reference.py) are the specification.  The
scorers work on strings and the device sees ids, so the host compiles the strings once and the kernels (svpc_caption_tokens,
svpc_caption_score_counts, svpc_caption_score_accum) work on token ids:

- ``parse_sent`` (para-evaluate.py:26-29) replaces every character outside a-z / A-Z by a blank, lower-cases and splits.  The
  substitution is per character, so a paragraph's token list is the concatenation of ``parse_sent(word)`` over its words: a word may
  give no token (``"1/2"``), one, or several (``"stir-fry"``);
- a word is ``idx2word[id]`` below V and the video's ``oov_word_dict`` entry from V on, after ``encode("ascii", "ignore")``;
- a token is an id 1 … 65534 of one lexicon (reference tokens, vocabulary-word tokens, copied-word tokens as videos are planned); an
  n-gram is the exact 64-bit key of its ≤ 4 ids in 16-bit fields — no hash collisions to reason about;
- ``ReferenceCorpus`` keeps on the device: the CSR vocabulary id → tokens, every reference's tokens (16-bit), the open-addressing table
  gram key → idf (``gram_hash`` below is the one hash, also stated in include/svpc_hip.h) and the table exp(−δ² / 72); per reference its
  length and its four CIDEr norms are computed here in float64;
- ``corpus.plan(videos)`` packs a batch's tables into one device buffer (one upload, none for a recurring batch): the reference slots of
  these videos and the CSR of each video's copied words → tokens.
"""
from __future__ import annotations

import math
import re

import numpy as np
import torch

from .caption_plan import CAP_COPIED, Bounded, GroupTables, PackedTables, PlanCompiler, RowTables, copied_words, vocabulary
from .ingredients import ascii_word

CAP_TOKENS = 1024           # tokens of a hypothesis and of a reference: both sit in the workgroup's LDS
CAP_REFS = 4
CAP_LEXICON = 65534         # token ids 1 … 65534: four 16-bit fields make an exact 64-bit gram key
VID_COLS = 12               # n_ref, corpus index, X, oov0, ref_off[4], ref_len[4]
SIGMA = 6.0
HASH_MUL = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


def parse_sent(s):
    """densevid_eval/para-evaluate.py:26-29"""
    return re.sub("[^a-zA-Z]", " ", s).strip().lower().split()


def gram_key(ids):
    """≤ 4 token ids → the 64-bit key (first token in the lowest field, absent fields 0)"""
    k = 0
    for j, t in enumerate(ids):
        k |= int(t) << (16 * j)
    return k


def gram_hash(key):
    """the table's hash, on both sides: h = key · 0x9E3779B97F4A7C15 mod 2⁶⁴, then h ^ (h >> 32); the slot is its low bits"""
    h = (key * HASH_MUL) & _M64
    return h ^ (h >> 32)


def _gram_counts(tok, n):
    c = {}
    for i in range(len(tok) - n + 1):
        k = gram_key(tok[i:i + n])
        c[k] = c.get(k, 0) + 1
    return c


class ScorePlan(PackedTables):
    """A batch's device tables: [ref_norm (N, 4, 4) float64 | vid (N, 12) | oov_off | oov_tok] int32 in one buffer; ``vid_off(steps)``
    adds the (N + 1,) table of the videos' first rows for a decode's (S_b) structure, cached."""

    def __init__(self, corpus, compiled, device):
        self.corpus = corpus
        self.n_vid = len(compiled)
        self.index = [c["index"] for c in compiled]
        self.max_expansion = [max(corpus.voc_expansion, c["expansion"]) for c in compiled]
        norms = np.zeros((self.n_vid, CAP_REFS, 4), dtype=np.float64)
        vid, oov_off, oov_tok = [], [], []
        for b, c in enumerate(compiled):
            i = c["index"]
            refs = corpus.ref_slots[i] if i >= 0 else []          # (a reference-free plan: n_ref = 0, index −1)
            row = [len(refs), i, len(c["tokens"]), len(oov_off)] + [0] * (VID_COLS - 4)
            for r, (off, n, nrm) in enumerate(refs):
                row[4 + r], row[8 + r] = off, n
                norms[b, r] = nrm
            vid += row
            for t in c["tokens"]:
                oov_off.append(len(oov_tok))
                oov_tok += t
            oov_off.append(len(oov_tok))
        super().__init__(dict(ref_norm=norms, vid=np.array(vid, dtype=np.int32), oov_off=np.array(oov_off, dtype=np.int32),
                              oov_tok=np.array(oov_tok + [0], dtype=np.int32)), device)        # (the float64 section comes first)
        self._offs = RowTables()
        self._groups = GroupTables()

    def vid_off(self, steps):
        return self._offs.table(steps, self.device, self.n_vid)

    def groups(self, steps, k, scope):
        """consensus selection's group tables of a decode's (S_b) structure with K candidates, cached → (table, G)"""
        return self._groups.table(steps, k, scope, self.device, self.n_vid)

    def check_cap(self, steps, lt):
        """ValueError when a video's hypothesis could exceed 1,024 tokens: S_b · (Lt − 1) · (longest expansion of a word)"""
        for b, s in enumerate(steps):
            if int(s) * (int(lt) - 1) * self.max_expansion[b] > CAP_TOKENS:
                raise ValueError("video %d: %d captions of %d words of up to %d tokens could exceed %d hypothesis tokens"
                                 % (b, s, int(lt) - 1, self.max_expansion[b], CAP_TOKENS))


class ReferenceCorpus(PlanCompiler):
    """Built once per evaluation set: ``idx2word`` (a list, or a dict id → word covering 0 … V − 1), ``references`` (video key → 1 … 4
    reference paragraph strings — a single string counts as one — as ``import_ground_truths`` holds them; the documents of CIDEr's idf are
    the videos of this whole set), the device the tables live on.  ``table_capacity``: slots of the gram table (a power of two above the
    number of grams; default: at most half full).

    ``plan(videos)``: one dict per video with ``key`` (a key of ``references``) and ``oov_word_dict`` (word → extended id) → the batch's
    ScorePlan.  ``compile_video(video)``: one video's host tables; ValueError for a key outside the reference set, copied ids outside
    V … V + 127 or used twice."""

    def __init__(self, idx2word, references, device="cuda", table_capacity=None):
        super().__init__(device)
        self._free_videos, self._free_plans = Bounded(4096), Bounded(32)
        idx2word = vocabulary(idx2word)
        if not len(references):
            raise ValueError("no references")
        self.V = len(idx2word)
        self._tok = {}                      # token string → id 1 …
        self.keys = list(references)
        self.index_of = {k: i for i, k in enumerate(self.keys)}
        self.n_docs = len(self.keys)
        self.log_docs = math.log(float(self.n_docs))
        # references first, then the vocabulary words
        self.ref_tokens = []                # per video, per reference: its token ids
        for k in self.keys:
            paras = references[k]
            paras = [paras] if isinstance(paras, str) else list(paras)
            if not 1 <= len(paras) <= CAP_REFS:
                raise ValueError("video %r: 1 … %d references, got %d" % (k, CAP_REFS, len(paras)))
            toks = []
            for p in paras:
                t = [self._token_id(w) for w in parse_sent(p)]
                if not t:
                    raise ValueError("video %r: a reference without a token" % (k,))
                if len(t) > CAP_TOKENS:
                    raise ValueError("video %r: a reference of %d tokens (at most %d)" % (k, len(t), CAP_TOKENS))
                toks.append(t)
            self.ref_tokens.append(toks)
        self.voc_tokens = [[self._token_id(w) for w in parse_sent(ascii_word(s))] for s in idx2word]
        self.voc_expansion = max(1, max(len(t) for t in self.voc_tokens))
        # document frequencies and idf over the videos of the whole set
        df = {}
        for toks in self.ref_tokens:
            seen = set()
            for t in toks:
                for n in range(1, 5):
                    seen.update(_gram_counts(t, n))
            for g in seen:
                df[g] = df.get(g, 0) + 1
        self.df = df
        self.idf = {g: self.log_docs - math.log(max(1.0, float(c))) for g, c in df.items()}
        # per reference: offset into the token array, length, the four norms
        flat, self.ref_slots, self.min_ref_len = [], [], []
        for toks in self.ref_tokens:
            slots = []
            for t in toks:
                nrm = [math.sqrt(sum((float(c) * self.idf[g]) ** 2 for g, c in _gram_counts(t, n).items())) for n in range(1, 5)]
                slots.append((len(flat), len(t), nrm))
                flat += t
            self.ref_slots.append(slots)
            self.min_ref_len.append(min(len(t) for t in toks))
        self.n_ref_tok = len(flat)
        # the gram → idf table
        need = len(df) + 1
        cap = 2
        while cap < (need if table_capacity is not None else 2 * need):
            cap *= 2
        if table_capacity is not None:
            if table_capacity & (table_capacity - 1) or table_capacity < need:
                raise ValueError("table_capacity must be a power of two above the %d grams, got %r" % (len(df), table_capacity))
            cap = int(table_capacity)
        self.table_capacity = cap
        self.table_keys = np.zeros(cap, dtype=np.uint64)
        self.table_idf = np.zeros(cap, dtype=np.float64)
        self.longest_probe = 0
        keys_py = [0] * cap
        for g, v in self.idf.items():
            slot, n = gram_hash(g) & (cap - 1), 1
            while keys_py[slot]:
                slot, n = (slot + 1) & (cap - 1), n + 1
            keys_py[slot] = g
            self.table_keys[slot] = g
            self.table_idf[slot] = v
            self.longest_probe = max(self.longest_probe, n)
        self.gauss_host = np.array([math.exp(-(d * d) / (2 * SIGMA ** 2)) for d in range(CAP_TOKENS)], dtype=np.float64)
        voc_off = np.zeros(self.V + 1, dtype=np.int32)
        voc_off[1:] = np.cumsum([len(t) for t in self.voc_tokens])
        voc_tok = np.array([x for t in self.voc_tokens for x in t] + [0], dtype=np.int32)
        self.voc_off = torch.from_numpy(voc_off).to(self.device)
        self.voc_tok = torch.from_numpy(voc_tok).to(self.device)
        self.ref_tok = torch.from_numpy(np.array(flat, dtype=np.uint16).view(np.int16).copy()).to(self.device)
        self.tab_key = torch.from_numpy(self.table_keys.view(np.int64).copy()).to(self.device)
        self.tab_idf = torch.from_numpy(self.table_idf.copy()).to(self.device)
        self.gauss = torch.from_numpy(self.gauss_host.copy()).to(self.device)

    def _token_id(self, w):
        i = self._tok.get(w)
        if i is None:
            if len(self._tok) >= CAP_LEXICON:
                raise ValueError("the token lexicon is full (%d tokens)" % CAP_LEXICON)
            i = self._tok[w] = len(self._tok) + 1
        return i

    @property
    def n_tokens(self):
        return len(self._tok)

    def token_strings(self):
        """→ id → token string (index 0 unused)"""
        out = [None] * (len(self._tok) + 1)
        for w, i in self._tok.items():
            out[i] = w
        return out

    def probe(self, key):
        """host-side walk of the device table as the kernel walks it → (idf, slots visited); idf None for an absent gram"""
        cap = self.table_capacity
        slot = gram_hash(int(key)) & (cap - 1)
        for n in range(1, cap + 1):
            k = int(self.table_keys[slot])
            if k == int(key):
                return float(self.table_idf[slot]), n
            if k == 0:
                return None, n
            slot = (slot + 1) & (cap - 1)
        return None, cap

    @staticmethod
    def video_key(video):
        return (video["key"], tuple(sorted((video.get("oov_word_dict") or {}).items())))

    def _compile(self, video):
        if video["key"] not in self.index_of:
            raise ValueError("video %r is not in the reference set" % (video["key"],))
        return dict(self._copied(video), index=self.index_of[video["key"]])

    def _copied(self, video):
        tokens = copied_words(video.get("oov_word_dict"), self.V, lambda w: [self._token_id(t) for t in parse_sent(ascii_word(w))],
                              missing=[])                                 # (an id no word of the video spells gives no token)
        return dict(tokens=tokens, expansion=max([1] + [len(t) for t in tokens]))

    def _plan(self, compiled):
        return ScorePlan(self, compiled, self.device)

    def plan(self, videos, references=True):
        """``references=False``: the plan of videos that have no references — the same packed layout with n_ref = 0 and index −1, any
        ``key`` (or none) accepted — for consensus selection, where this corpus only supplies the vocabulary and the
        idf.  Cached apart from the plans with references."""
        if references:
            return super().plan(videos)
        if not len(videos):
            raise ValueError("no videos to plan")
        keys = tuple(tuple(sorted((v.get("oov_word_dict") or {}).items())) for v in videos)
        p = self._free_plans.get(keys)
        if p is None:
            compiled = []
            for v, k in zip(videos, keys):
                c = self._free_videos.get(k)
                if c is None:
                    c = self._free_videos.put(k, dict(self._copied(v), index=-1))
                compiled.append(c)
            p = self._free_plans.put(keys, self._plan(compiled))
        return p


def bleu_from_totals(correct, guess, testlen, reflen):
    """[Bleu_1 … Bleu_4] from integer totals (Bleu(4), option ``closest``: tiny = 1e-15, small = 1e-9)"""
    tiny, small = 1e-15, 1e-9
    ratio = (testlen + tiny) / (reflen + small)
    out, b = [], 1.0
    for n in range(4):
        b *= (correct[n] + tiny) / (guess[n] + small)
        v = b ** (1.0 / (n + 1))
        if ratio < 1:
            v *= math.exp(1 - 1 / ratio)
        out.append(v)
    return out
