"""Pure-Python restatement of Bleu_1…4, ROUGE_L and CIDEr of decoded captions (svpc_amd/csrc/caption_scores.hip).

String level, ``collections.Counter`` only; shares no code with the product.  The definitions are the published ones as the public
caption scorer implements them (Bleu(4) with option ``closest``, Rouge with β = 1.2, the ``Cider()`` class with n = 4, σ = 6), applied the
way densevid_eval/para-evaluate.py applies them (:26-29 parse_sent, :71-84 the hypothesis paragraph, :112-125 evaluate_para):

- ``parse_sent(s)`` = ``re.sub('[^a-zA-Z]', ' ', s).strip().lower().split()``; a video's hypothesis is ``parse_sent`` of its submitted
  sentences, each followed by ``". "``; a reference is ``parse_sent`` of an annotation paragraph;
- a submitted sentence is the blank-joined words of a clean caption (tests/caption_metrics_reference.py, run collapse on); a word is
  ``idx2word[id]`` below V and the video's ``oov_word_dict`` entry from V on, after ``encode("ascii", "ignore")``;
- n-grams run over the whole paragraph, across sentence boundaries.
"""
import math
import re
from collections import Counter

from caption_metrics_reference import clean_caption

TINY, SMALL = 1e-15, 1e-9
BETA, SIGMA, N_MAX = 1.2, 6.0, 4


def parse_sent(sent):
    return re.sub("[^a-zA-Z]", " ", sent).strip().lower().split()


def ascii_word(s):
    return s.encode("ascii", "ignore").decode("ascii")


def sentence_words(clean_ids, idx2word, oov_word_dict):
    V = len(idx2word)
    inv = {int(v): k for k, v in (oov_word_dict or {}).items()}
    return [ascii_word(idx2word[i] if 0 <= i < V else inv[i]) for i in clean_ids]


def hypothesis_paragraph(id_rows, idx2word, oov_word_dict):
    """a video's decoded id rows → the paragraph string para-evaluate.py builds from the submitted sentences"""
    para = ""
    for row in id_rows:
        para += " ".join(sentence_words(clean_caption(row), idx2word, oov_word_dict)) + ". "
    return para


def hypothesis_tokens(id_rows, idx2word, oov_word_dict):
    return parse_sent(hypothesis_paragraph(id_rows, idx2word, oov_word_dict))


def hypothesis_tokens_per_word(id_rows, idx2word, oov_word_dict):
    """the same token list word by word (the substitution is per character): what the device does"""
    out = []
    for row in id_rows:
        for w in sentence_words(clean_caption(row), idx2word, oov_word_dict):
            out += parse_sent(w)
    return out


def grams(tokens, n):
    return Counter(tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1))


# ---------------------------------------------------------------------------------------------------- Bleu
def bleu_counts(h, refs):
    """→ (correct_1..4, guess_1..4, testlen, reflen) of one video"""
    correct, guess = [], []
    for n in range(1, N_MAX + 1):
        ch = grams(h, n)
        cr = [grams(r, n) for r in refs]
        correct.append(sum(min(c, max(x[g] for x in cr)) for g, c in ch.items()))
        guess.append(max(0, len(h) - n + 1))
    reflen = min((abs(len(r) - len(h)), len(r)) for r in refs)[1]
    return correct, guess, len(h), reflen


def bleu_from_counts(correct, guess, testlen, reflen):
    """→ [Bleu_1 … Bleu_4] from totals (of a corpus or of one video)"""
    out, b = [], 1.0
    ratio = (testlen + TINY) / (reflen + SMALL)
    for n in range(N_MAX):
        b *= (correct[n] + TINY) / (guess[n] + SMALL)
        v = b ** (1.0 / (n + 1))
        if ratio < 1:
            v *= math.exp(1 - 1 / ratio)
        out.append(v)
    return out


# ---------------------------------------------------------------------------------------------------- ROUGE_L
def lcs(a, b):
    """textbook dynamic programme"""
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[-1]


def rouge_l(h, refs):
    """→ (score, the largest lcs)"""
    ls = [lcs(r, h) for r in refs]
    p = max(l / max(len(h), 1) for l in ls)
    q = max(l / len(r) for l, r in zip(ls, refs))
    score = (1 + BETA ** 2) * p * q / (q + BETA ** 2 * p) if p != 0 and q != 0 else 0.0
    return score, max(ls)


# ---------------------------------------------------------------------------------------------------- CIDEr
class CiderCorpus:
    """document frequencies over the whole reference set: ``references`` = per video its list of reference token lists"""

    def __init__(self, references):
        self.n_docs = len(references)
        self.ref_len = math.log(float(self.n_docs))
        self.df = Counter()
        for refs in references:
            seen = set()
            for r in refs:
                for n in range(1, N_MAX + 1):
                    seen.update(grams(r, n))
            for g in seen:
                self.df[g] += 1

    def idf(self, g):
        return self.ref_len - math.log(max(1.0, self.df.get(g, 0)))

    def vec(self, tokens):
        """→ (vec_1..4 dicts, norm_1..4, length = number of bigrams)"""
        vecs, norms, length = [], [], 0
        for n in range(1, N_MAX + 1):
            v = {g: float(c) * self.idf(g) for g, c in grams(tokens, n).items()}
            vecs.append(v)
            norms.append(math.sqrt(sum(x * x for x in v.values())))
            if n == 2:
                length = sum(grams(tokens, n).values())
        return vecs, norms, length

    def score(self, h, refs):
        vh, nh, lh = self.vec(h)
        total = [0.0] * N_MAX
        for r in refs:
            vr, nr, lr = self.vec(r)
            delta = float(lh - lr)
            for n in range(N_MAX):
                val = 0.0
                for g, x in vh[n].items():
                    y = vr[n].get(g, 0.0)
                    val += min(x, y) * y
                if nh[n] != 0 and nr[n] != 0:
                    val /= nh[n] * nr[n]
                val *= math.exp(-(delta ** 2) / (2 * SIGMA ** 2))
                total[n] += val
        return 10.0 * (sum(total) / N_MAX) / len(refs)


# ---------------------------------------------------------------------------------------------------- a video, an epoch
def video_scores(h, refs, cider):
    """→ (the 11 integer counts: correct_1..4, guess_1..4, testlen, reflen, lcs; the 6 scores: Bleu_1..4, ROUGE_L, CIDEr)"""
    correct, guess, testlen, reflen = bleu_counts(h, refs)
    rouge, best = rouge_l(h, refs)
    return (correct + guess + [testlen, reflen, best],
            bleu_from_counts(correct, guess, testlen, reflen) + [rouge, cider.score(h, refs)])


def corpus_result(hyps, references, missing="skip"):
    """``hyps``: video index → hypothesis token list (a dict, or a list of (index, tokens) pairs when videos repeat); ``references``:
    per video of the WHOLE reference set its reference token lists → (the result dict of CaptionScores.result(), per-update rows)."""
    cider = CiderCorpus(references)
    pairs = list(hyps.items()) if isinstance(hyps, dict) else list(hyps)
    if missing == "empty":
        seen = {i for i, _ in pairs}
        pairs = pairs + [(i, []) for i in range(len(references)) if i not in seen]
    rows = [video_scores(h, references[i], cider) for i, h in pairs]
    tot = [sum(r[0][k] for r in rows) for k in range(10)]
    nv = len(rows)
    bleu = bleu_from_counts(tot[0:4], tot[4:8], tot[8], tot[9]) if nv else [0.0] * 4
    res = {"Bleu_%d" % (n + 1): bleu[n] for n in range(N_MAX)}
    res.update(ROUGE_L=sum(r[1][4] for r in rows) / nv if nv else 0.0, CIDEr=sum(r[1][5] for r in rows) / nv if nv else 0.0,
               num_videos=nv, testlen=tot[8], reflen=tot[9], correct=tot[0:4], guess=tot[4:8])
    return res, rows
