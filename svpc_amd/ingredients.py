"""Host compilation for the ingredient-prediction recall / precision / F1 on the device.

reference: src/calculate_ingredient_f1.py:6-30 (extract_ingredients), :32-59 (calculate_ingredient_f1), :61-73
(construct_ingredient_dict: the global set A of ingredient strings).  The reference's rule is a string rule — ``ingredient in sentence`` is
a substring test, so ``oil`` is found inside ``boil`` — and the device sees ids.  The host therefore compiles strings into bit tables
once, and the kernel (svpc_caption_ingredients) matches ids against them:

- a caption word is the string of its id (``idx2word`` below V, the video's ``oov_word_dict`` from V on) after
  ``encode("ascii", "ignore")``; a word that ends up empty or contains a blank is a ValueError;
- listed ingredient I[e] with t = I[e].split(" ") is mentioned iff at some position p — k = 1: t[0] occurs inside w[p]; k ≥ 2: w[p] ends
  with t[0], w[p + j] == t[j] for the middle j and w[p + k − 1] starts with t[k − 1] (= ``I[e] in " ".join(w)`` for such words);
- every pattern token is a predicate (*contains t*, *ends with t*, *equals t*, *starts with t*); ``IngredientLexicon`` keeps one row of a
  (P, ⌈V / 32⌉) device bitmap per distinct predicate (bit i: vocabulary word i satisfies it), grown as videos are planned, and the V-bit
  map of the vocabulary words in A;
- ``lexicon.plan(videos)`` packs a batch's tables into one device buffer (one upload, none for a recurring batch): per video the CSR of
  ingredient → pattern tokens (predicate row + the predicate evaluated on the video's ≤ 128 copied words), the ids equal to a whole
  listed ingredient, the copied words in A, and per ground-truth step the mask of listed ingredients, the ids of its extra words and the
  length of its list (an extra word no id of the video spells can never be matched: it only counts in the length).
"""
from __future__ import annotations

import numpy as np
import torch

from .caption_plan import CAP_COPIED, PackedTables, PlanCompiler, RowTables, copied_words, vocabulary

CAP_INGREDIENTS = 64        # E_b: one bit of the 64-bit mask per listed ingredient
CAP_TOKENS = 128            # pattern tokens of one video
CONTAINS, ENDS, EQUALS, STARTS = 0, 1, 2, 3
VID_COLS = 8                # ing0, E, X, eq0, n_eq, gt0, n_gt, (unused)


def ascii_word(s):
    return s.encode("ascii", "ignore").decode("ascii")


def _caption_word(s, what):
    w = ascii_word(s)
    if w == "" or " " in w:
        raise ValueError("%s %r is empty or contains a blank after encode('ascii', 'ignore')" % (what, s))
    return w


def pattern(ingredient):
    """an ingredient string → its pattern tokens [(predicate kind, token string)]"""
    if ingredient == "":
        raise ValueError("an empty ingredient string matches every caption: refused")
    t = ingredient.split(" ")
    if len(t) == 1:
        return [(CONTAINS, t[0])]
    return [(ENDS, t[0])] + [(EQUALS, x) for x in t[1:-1]] + [(STARTS, t[-1])]


def holds(kind, t, word):
    """predicate (kind, t) on a word, by direct string test"""
    if kind == CONTAINS:
        return t in word
    if kind == ENDS:
        return word.endswith(t)
    if kind == EQUALS:
        return word == t
    return word.startswith(t)


def _mentioned(pat, words):
    k = len(pat)
    return any(all(holds(kind, t, words[p + j]) for j, (kind, t) in enumerate(pat)) for p in range(len(words) - k + 1))


def _bits(flags, n_words):
    out = np.zeros(n_words, dtype=np.uint32)
    for i, f in enumerate(flags):
        if f:
            out[i >> 5] |= np.uint32(1 << (i & 31))
    return out


def masks_to_names(masks, ingredients):
    """(S_b,) masks of one video (a tensor, an array or a list of ints) → per step the names of the listed ingredients mentioned"""
    vals = masks.tolist() if hasattr(masks, "tolist") else list(masks)
    return [[ing for e, ing in enumerate(ingredients) if (int(m) >> e) & 1] for m in vals]


class IngredientPlan(PackedTables):
    """A batch's device tables (see the module docstring); ``rows(steps)`` adds the row → (video, step) table of a decode's (S_b)
    structure, cached, so a recurring structure uploads nothing."""

    def __init__(self, lexicon, compiled, device):
        self.lexicon = lexicon
        self.n_vid = len(compiled)
        self.ingredients = [c["ingredients"] for c in compiled]
        self.gt_steps = [len(c["gt"]) if c["gt"] is not None else None for c in compiled]
        self.has_gt = all(g is not None for g in self.gt_steps)
        vid, ing_tok, tok_row, tok_oov, eq_ids, oov_a = [], [], [], [], [], []
        gt_mask, gt_len, gx_off, gx_ids = [], [], [0], []
        for c in compiled:
            base = len(tok_row)
            vid += [len(ing_tok), len(c["ingredients"]), c["X"], len(eq_ids), len(c["eq_ids"]), len(gt_len), len(c["gt"] or ()), 0]
            ing_tok += [base + o for o in c["ing_off"]]
            tok_row += c["tok_row"]
            tok_oov.append(c["tok_oov"].reshape(-1))
            eq_ids += c["eq_ids"]
            oov_a.append(c["oov_a"])
            for mask, extra, n in c["gt"] or ():
                gt_mask += [mask & 0xFFFFFFFF, mask >> 32]
                gt_len.append(n)
                gx_ids += extra
                gx_off.append(len(gx_ids))
        parts = dict(vid=np.array(vid, dtype=np.int64), ing_tok=np.array(ing_tok, dtype=np.int64), tok_row=np.array(tok_row, dtype=np.int64),
                     tok_oov=np.concatenate(tok_oov) if tok_oov else np.zeros(0, np.uint32), eq_ids=np.array(eq_ids, dtype=np.int64),
                     oov_a=np.concatenate(oov_a) if oov_a else np.zeros(0, np.uint32), gt_mask=np.array(gt_mask, dtype=np.uint32),
                     gt_len=np.array(gt_len, dtype=np.int64), gx_off=np.array(gx_off, dtype=np.int64), gx_ids=np.array(gx_ids, dtype=np.int64))
        super().__init__(parts, device)
        self._rows = RowTables(rows=True)

    def default_steps(self):
        if not self.has_gt:
            raise ValueError("steps are required: the plan has no ground-truth sentences to take the videos' step counts from")
        return list(self.gt_steps)

    def rows(self, steps):
        """[vid_off (N + 1) | (video, step) of every row (2 T)] int32 on the device for the videos' row counts ``steps``"""
        return self._rows.table(steps, self.device, self.n_vid)


class IngredientLexicon(PlanCompiler):
    """Built once per vocabulary: ``idx2word`` (a list, or a dict id → word covering 0 … V − 1), ``all_ingredients`` (the global set A),
    the device the tables live on.  ``table`` is the (capacity, ⌈V / 32⌉) int32 predicate bitmap (``n_rows`` rows in use), ``a_bits`` the
    (⌈V / 32⌉,) map of the vocabulary words in A.

    ``plan(videos)``: one dict per video with ``ingredients`` (raw strings, duplicates kept), ``oov_word_dict`` (word → extended id) and
    optionally ``gt_sentences`` (and ``key``, any hashable that names the video; default: its content) → the batch's IngredientPlan.
    ``compile_video(video)``: one video's host tables; ValueError for an empty ingredient, a copied word that is empty or holds a blank,
    copied ids outside V … V + 127 or used twice, more than 64 ingredients or 128 pattern tokens."""

    def __init__(self, idx2word, all_ingredients, device="cuda"):
        super().__init__(device)
        self.words = [_caption_word(w, "vocabulary word") for w in vocabulary(idx2word)]
        self.V = len(self.words)
        self.W = (self.V + 31) // 32
        self.A = frozenset(all_ingredients)
        self._ids_of = {}
        for i, w in enumerate(self.words):
            self._ids_of.setdefault(w, []).append(i)
        self.a_bits_host = _bits([w in self.A for w in self.words], self.W)
        self.a_bits = torch.from_numpy(self.a_bits_host.view(np.int32).copy()).to(self.device)
        self._pred = {}                     # (kind, token) → row
        self.host_rows = []                 # row → (W,) uint32
        self.table = torch.zeros(256, self.W, dtype=torch.int32, device=self.device)
        self._uploaded = 0
        self._retired = []                  # outgrown tables stay allocated: a captured update may still read its (unchanged) rows

    @property
    def n_rows(self):
        return len(self.host_rows)

    def predicates(self):
        """→ [(kind, token)] in row order"""
        return sorted(self._pred, key=self._pred.get)

    def row_of(self, kind, t):
        r = self._pred.get((kind, t))
        if r is None:
            r = self._pred[(kind, t)] = len(self.host_rows)
            self.host_rows.append(_bits([holds(kind, t, w) for w in self.words], self.W))
        return r

    def _sync(self):
        n = len(self.host_rows)
        if n == self._uploaded:
            return
        if n > self.table.shape[0]:
            grown = torch.zeros(max(n, 2 * self.table.shape[0]), self.W, dtype=torch.int32, device=self.device)
            grown[:self._uploaded].copy_(self.table[:self._uploaded])
            self._retired.append(self.table)
            self.table = grown
        new = np.stack(self.host_rows[self._uploaded:n]).view(np.int32)
        self.table[self._uploaded:n].copy_(torch.from_numpy(new))
        self._uploaded = n

    @staticmethod
    def video_key(video):
        if "key" in video:
            return video["key"]
        gt = video.get("gt_sentences")
        return (tuple(video["ingredients"]), tuple(sorted((video.get("oov_word_dict") or {}).items())), None if gt is None else tuple(gt))

    def _compile(self, video):
        ingredients = list(video["ingredients"])
        if len(ingredients) > CAP_INGREDIENTS:
            raise ValueError("a video holds at most %d ingredients (one mask bit each), got %d" % (CAP_INGREDIENTS, len(ingredients)))
        copied = copied_words(video.get("oov_word_dict"), self.V, lambda w: _caption_word(w, "copied word"))  # (None: an id no word spells)
        pats = [pattern(ing) for ing in ingredients]
        if sum(len(p) for p in pats) > CAP_TOKENS:
            raise ValueError("a video holds at most %d pattern tokens, got %d" % (CAP_TOKENS, sum(len(p) for p in pats)))
        ing_off, tok_row, tok_oov = [0], [], []
        for p in pats:
            for kind, t in p:
                tok_row.append(self.row_of(kind, t))
                tok_oov.append(_bits([w is not None and holds(kind, t, w) for w in copied], CAP_COPIED // 32))
            ing_off.append(len(tok_row))

        def ids_of(s):
            return self._ids_of.get(s, []) + [self.V + x for x, w in enumerate(copied) if w == s]
        whole = set(ingredients)
        eq_ids = sorted({i for s in whole for i in ids_of(s)})
        gt = None
        if video.get("gt_sentences") is not None:
            gt = []
            for s in video["gt_sentences"]:
                words = s.split(" ")
                mask = sum(1 << e for e, p in enumerate(pats) if _mentioned(p, words))
                extra = [w for w in words if w not in whole and w in self.A]
                gt.append((mask, sorted({i for w in extra for i in ids_of(w)}), bin(mask).count("1") + len(extra)))
        return dict(ingredients=ingredients, X=len(copied), copied=copied, ing_off=ing_off, tok_row=tok_row,
                    tok_oov=np.stack(tok_oov) if tok_oov else np.zeros((0, CAP_COPIED // 32), np.uint32), eq_ids=eq_ids,
                    oov_a=_bits([w is not None and w in self.A for w in copied], CAP_COPIED // 32), gt=gt)

    def _plan(self, compiled):
        self._sync()
        return IngredientPlan(self, compiled, self.device)
