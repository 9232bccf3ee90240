"""What the host compilers of the caption metrics share (DESIGN §11.4–11.6): ``ingredients`` and ``caption_scores`` turn strings into id
tables once, pack a batch's tables into one device buffer and cache everything that recurs, so an ``update`` uploads nothing and can be
captured.  One statement each of

- ``Bounded``: the caches' bound (a dict emptied before the insertion that would outgrow it);
- ``PackedTables``: named numpy sections → one int32 buffer, one upload; ``section`` / ``ptr`` / ``size`` by name;
- ``RowTables``: the cached table of a decode's (S_b) structure — the videos' first rows, optionally (video, step) of every row;
- ``GroupTables``: the cached tables of consensus selection's groups per (S_b structure, K, scope);
- ``vocabulary`` and ``copied_words``: the rules for ``idx2word`` and for a video's ``oov_word_dict`` (ids V … V + 127, each once);
- ``PlanCompiler``: per-video compilation and per-batch plans, both cached by key.
"""
from __future__ import annotations

import numpy as np
import torch

CAP_COPIED = 128            # copied (OOV) words of one video, ids V … V + 127: four 32-bit words per predicate


class Bounded(dict):
    """a cache of at most ``limit`` + 1 entries: ``put`` empties it first when it already holds more than ``limit``"""

    def __init__(self, limit):
        super().__init__()
        self.limit = limit

    def put(self, key, value):
        if len(self) > self.limit:
            self.clear()
        self[key] = value
        return value


class PackedTables:
    """``parts`` (name → numpy array, in order) as one int32 device buffer ``buf``, made by one upload; ``sections``: name → (offset,
    size) in int32 words.  A uint32 section is viewed as int32, another integer one converted; a float64 section is viewed as int32 pairs
    and must start on an 8-byte boundary."""

    def __init__(self, parts, device):
        self.device = device
        self.sections, flat, o = {}, [], 0
        for name, a in parts.items():
            if a.dtype == np.float64:
                if o % 2:
                    raise ValueError("the float64 section %r would start at the odd int32 offset %d" % (name, o))
                a32 = a.reshape(-1).view(np.int32)
            else:
                a32 = a.view(np.int32) if a.dtype == np.uint32 else a.astype(np.int32)
            self.sections[name] = (o, a32.size)
            flat.append(a32)
            o += a32.size
        self.buf = torch.from_numpy(np.concatenate(flat)).to(device)          # the batch's one upload

    def section(self, name):
        """a section of the packed buffer as an int32 view (tests; the kernels take ``ptr(name)``)"""
        o, n = self.sections[name]
        return self.buf[o:o + n]

    def ptr(self, name):
        return self.buf.data_ptr() + 4 * self.sections[name][0]

    def size(self, name):
        return self.sections[name][1]


class RowTables(Bounded):
    """(S_b) structure → its int32 device table [vid_off (N + 1)], with ``rows`` followed by (video, step) of every row (2 T): uploaded
    once per structure and device, so a recurring structure uploads nothing."""

    def __init__(self, rows=False):
        super().__init__(32)
        self.rows = rows

    def table(self, steps, device, n_vid=None):
        """``n_vid``: the number of videos ``steps`` must describe (ValueError otherwise, and for a negative count)"""
        steps = tuple(int(s) for s in steps)
        if n_vid is not None and (len(steps) != n_vid or any(s < 0 for s in steps)):
            raise ValueError("the plan holds %d video(s), got the row counts %r" % (n_vid, list(steps)))
        key = (steps, str(device))
        t = self.get(key)
        if t is None:
            off = [0]
            for s in steps:
                off.append(off[-1] + s)
            vs = [x for b, s in enumerate(steps) for i in range(s) for x in (b, i)] if self.rows else []
            t = self.put(key, torch.tensor(off + vs, dtype=torch.int32, device=device))
        return t


class GroupTables(Bounded):
    """((S_b) structure, K, scope) → the int32 device table of consensus selection's groups: [streams (G · K, 4) = first
    clean row, rows, row stride, video of stream g · K + k | grp_off (G + 1) first sentence of every group].  The clean rows are those of
    the (T, K, Lt) decode taken as T · K rows, so candidate k of sentence t is row t · K + k.  ``paragraph``: one group per video,
    candidate k is row k of each of its sentences in order; ``sentence``: one group per sentence.  Uploaded once per key and device."""

    def __init__(self):
        super().__init__(32)

    def table(self, steps, k, scope, device, n_vid=None):
        """→ (table, G); ValueError for row counts that do not describe ``n_vid`` videos"""
        steps, k = tuple(int(s) for s in steps), int(k)
        if n_vid is not None and (len(steps) != n_vid or any(s < 0 for s in steps)):
            raise ValueError("the plan holds %d video(s), got the row counts %r" % (n_vid, list(steps)))
        key = (steps, k, scope, str(device))
        t = self.get(key)
        if t is None:
            streams, off, row0 = [], [0], 0
            for b, s in enumerate(steps):
                if scope == "paragraph":
                    for c in range(k):
                        streams += [row0 * k + c, s, k, b]
                    off.append(row0 + s)
                else:
                    for r in range(row0, row0 + s):
                        for c in range(k):
                            streams += [r * k + c, 1, k, b]
                        off.append(r + 1)
                row0 += s
            t = self.put(key, (torch.tensor(streams + off, dtype=torch.int32, device=device), len(off) - 1))
        return t


def vocabulary(idx2word):
    """``idx2word`` (a list, or a dict id → word covering 0 … V − 1) → the list of the V ≥ 1 words"""
    if isinstance(idx2word, dict):
        if sorted(idx2word) != list(range(len(idx2word))):
            raise ValueError("idx2word must cover the ids 0 … V − 1")
        idx2word = [idx2word[i] for i in range(len(idx2word))]
    if not len(idx2word):
        raise ValueError("an empty vocabulary")
    return idx2word


def copied_words(oov_word_dict, V, word, missing=None):
    """A video's ``oov_word_dict`` (word → extended id) → [``word(w)`` of id V + x for x < X], X = the highest id in use − V + 1 and
    ``missing`` for an id no word of the video spells.  ValueError for an id outside V … V + 127, not integral, or used twice; the
    caller's ``word`` runs item by item between these checks and may raise its own."""
    oov = {}
    for w, i in (oov_word_dict or {}).items():
        if isinstance(i, bool) or int(i) != i or not V <= int(i) < V + CAP_COPIED:
            raise ValueError("copied word %r: its id %r is outside V … V + %d (at most %d copied words per video)"
                             % (w, i, CAP_COPIED - 1, CAP_COPIED))
        if int(i) in oov:
            raise ValueError("copied id %d is used twice" % int(i))
        oov[int(i)] = word(w)
    X = max(oov) - V + 1 if oov else 0
    return [oov.get(V + x, missing) for x in range(X)]


class PlanCompiler:
    """Base of ``IngredientLexicon`` and ``ReferenceCorpus``: ``compile_video(video)`` caches a video's host tables per
    ``video_key(video)`` (bounded at 4096), ``plan(videos)`` the batch's plan per tuple of video keys (bounded at 32), so a recurring
    batch uploads nothing.  A subclass supplies ``video_key``, ``_compile(video)`` and ``_plan(compiled)``."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._videos = Bounded(4096)
        self._plans = Bounded(32)

    def compile_video(self, video):
        key = self.video_key(video)
        c = self._videos.get(key)
        if c is None:
            c = self._videos.put(key, self._compile(video))
        return c

    def plan(self, videos):
        if not len(videos):
            raise ValueError("no videos to plan")
        key = tuple(self.video_key(v) for v in videos)
        p = self._plans.get(key)
        if p is None:
            p = self._plans.put(key, self._plan([self.compile_video(v) for v in videos]))
        return p
