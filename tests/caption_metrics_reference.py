"""Pure-Python restatement of the caption clean-up and the repetition / diversity counters (svpc_amd/csrc/caption.hip).

Id level: a word is its id; an id ≥ V is a copied OOV word of its video and is its own word.

- clean caption of an id row (recursive_caption_dataset.py:472-500 then src/translate.py:27-42): the ids without PAD and IGNORE, without
  the first of those, up to (not including) the first EOS, runs of one id collapsed to one;
- repetition words (densevid_eval/evaluateRepetition.py:79-87): the clean caption without a final ``period_id`` and without any
  ``comma_id``;
- per video, n = 1 … 4: total_n n-grams (n consecutive repetition words of one caption), distinct_n different ones;
  re_n = (total_n − distinct_n) / total_n, div_n = distinct_n / total_1 (0 for an empty denominator);
- epoch result: the means over the videos and the caption statistics.
"""
from svpc_amd.synthetic import EOS, IGNORE, PAD

COUNT_COLS = ("total_1", "total_2", "total_3", "total_4", "distinct_1", "distinct_2", "distinct_3", "distinct_4",
              "n_sen", "n_words", "n_empty", "n_copied")


def clean_caption(row, pad=PAD, eos=EOS, ignore=IGNORE, remove_dup=True):
    """one id row (a list of ints) → the clean caption (a list of ints)"""
    raw = [int(v) for v in row if v != pad and v != ignore]
    words = []
    for v in raw[1:]:
        if v == eos:
            break
        words.append(v)
    if not remove_dup:
        return words
    out = []
    for v in words:
        if not out or out[-1] != v:
            out.append(v)
    return out


def clean_rows(rows, lt=None, pad=PAD, eos=EOS, ignore=IGNORE, remove_dup=True):
    """rows of ids → (the clean captions left-aligned in ``lt``-wide PAD-filled rows, their lengths)"""
    out, lens = [], []
    for row in rows:
        c = clean_caption(row, pad, eos, ignore, remove_dup)
        n = lt if lt is not None else len(row)
        out.append(c + [pad] * (n - len(c)))
        lens.append(len(c))
    return out, lens


def repetition_words(clean, period_id=None, comma_id=None):
    w = list(clean)
    if period_id is not None and w and w[-1] == period_id:
        w = w[:-1]
    if comma_id is not None:
        w = [v for v in w if v != comma_id]
    return w


def video_counts(cleans, V, period_id=None, comma_id=None):
    """the clean captions of one video → the 12 counts of COUNT_COLS"""
    grams = [set() for _ in range(4)]
    total = [0] * 4
    for c in cleans:
        w = repetition_words(c, period_id, comma_id)
        for n in range(1, 5):
            for i in range(len(w) - n + 1):
                grams[n - 1].add(tuple(w[i:i + n]))
                total[n - 1] += 1
    return total + [len(g) for g in grams] + [len(cleans), sum(len(c) for c in cleans), sum(1 for c in cleans if not c),
                                              sum(1 for c in cleans for v in c if v >= V)]


def ratios(counts):
    """one video's counts → (re_1..4, div_1..4)"""
    re_ = [(counts[n] - counts[4 + n]) / counts[n] if counts[n] else 0.0 for n in range(4)]
    div = [counts[4 + n] / counts[0] if counts[0] else 0.0 for n in range(4)]
    return re_, div


def epoch_result(videos, V, period_id=None, comma_id=None, pad=PAD, eos=EOS, ignore=IGNORE, remove_dup=True):
    """``videos``: per video its id rows (lists of lists) → (the result dict of DecodeMetrics.result(), the per-video count rows)"""
    rows, vocab = [], set()
    sums = [0.0] * 8
    for vid in videos:
        cleans = [clean_caption(r, pad, eos, ignore, remove_dup) for r in vid]
        c = video_counts(cleans, V, period_id, comma_id)
        rows.append(c)
        re_, div = ratios(c)
        for n in range(4):
            sums[n] += re_[n]
            sums[4 + n] += div[n]
        vocab.update(v for cl in cleans for v in cl if 0 <= v < V)
    nv = len(rows)
    res = {}
    for n in range(4):
        res["re%d" % (n + 1)] = sums[n] / nv if nv else 0.0
        res["div%d" % (n + 1)] = sums[4 + n] / nv if nv else 0.0
    num_sen = sum(c[8] for c in rows)
    num_words = sum(c[9] for c in rows)
    res.update(num_videos=nv, num_sen=num_sen, num_words=num_words, avg_sen_len=num_words / num_sen if num_sen else 0.0,
               num_empty=sum(c[10] for c in rows), num_copied=sum(c[11] for c in rows), vocab_size=len(vocab))
    return res, rows
