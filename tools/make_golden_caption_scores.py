"""Write tests/golden/caption_scores.json: seeded hypothesis id rows for the 100 validation videos, their reference paragraphs, and what
the Python restatement of Bleu_1…4 / ROUGE_L / CIDEr (tests/caption_scores_reference.py) makes of them.

    python tools/make_golden_caption_scores.py --reference <path to the reference checkout> [--out tests/golden/caption_scores.json]

Only data is recorded, no reference text:
- references: every paragraph of densevid_eval/yc2_data/yc2_split_val_anet_format_para.json; for ten videos a second reference, the same
  paragraph with words dropped and replaced (one of them two tokens shorter than the first, for the closest-length tie);
- sentences: the per-step sentences of the same 100 videos (bosselut_split_yc2_val_anet_format.json);
- vocabulary: the 951 words of cache/yc2_word2idx.json; a video's OOV dictionary: the words of its sentences outside the vocabulary, ids
  V, V + 1, … in order of appearance;
- one id row per sentence: BOS, the sentence's words corrupted (a word is dropped with probability 0.1, replaced by a random vocabulary
  word with 0.12, and repeated after its successor with 0.08), cut to Lt − 2 words, EOS, then PAD fill (beam style) or junk with further
  EOS (greedy style).  Lt = 22, and 64 for four videos of at most eight sentences.  One video's rows are all empty, one video's hold a
  single one-token word, one video's are its sentences minus one word (the tie);
- per video the restatement's 11 counts and 6 scores, and the corpus result for ``missing="skip"`` and, with the last batch left out,
  ``missing="empty"``.
The scores are pinned to the published definitions as the restatement states them, not to outputs of the third-party scorer,
which is not part of the reference checkout.  No video is drawn again or left out; the coverage the tests rely on is asserted here.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import caption_scores_reference as cs  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, N_SPECIAL, PAD, UNK  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "caption_scores.json"))
    ap.add_argument("--seed", type=int, default=2019)
    a = ap.parse_args(argv)
    word2idx = json.load(open(os.path.join(a.reference, "cache", "yc2_word2idx.json")))
    V = len(word2idx)
    words = [None] * V
    for w, i in word2idx.items():
        words[i] = w
    assert all(w is not None for w in words) and words[PAD] == "[PAD]" and words[EOS] == "[EOS]" and words[BOS] == "[BOS]"
    data = os.path.join(a.reference, "densevid_eval", "yc2_data")
    paras = json.load(open(os.path.join(data, "yc2_split_val_anet_format_para.json")))
    steps = json.load(open(os.path.join(data, "bosselut_split_yc2_val_anet_format.json")))
    keys = list(paras)
    assert len(keys) == 100 and set(keys) == set(steps)
    rng = np.random.default_rng(a.seed)
    plain = list(range(N_SPECIAL, V))

    def corrupt_words(ws, p_drop, p_rep, p_dup):
        out, pending = [], None
        for w in ws:
            u = rng.random()
            if u < p_drop:
                continue
            if u < p_drop + p_rep:
                w = words[plain[int(rng.integers(0, len(plain)))]]
            out.append(w)
            if pending is not None:
                out.append(pending)
                pending = None
            if p_drop + p_rep <= u < p_drop + p_rep + p_dup:
                pending = w
        return out

    # ---- the Lt = 64 batch: four videos of at most eight sentences; special videos: empty, one token, the tie
    short = [k for k in keys if len(steps[k]["sentences"]) <= 8][:4]
    assert len(short) == 4
    rest = [k for k in keys if k not in short]
    k_empty, k_one = rest[5], rest[11]

    def tie_ok(k):
        sents = [s.split() for s in steps[k]["sentences"]]
        flat = [w for s in sents for w in s]
        return (all(w in word2idx and len(cs.parse_sent(w)) == 1 for w in flat) and all(len(s) <= 20 for s in sents)
                and all(x != y for s in sents for x, y in zip(s, s[1:])) and len(sents[0]) >= 4 and k not in (k_empty, k_one))
    k_tie = next(k for k in rest if tie_ok(k))
    second = [k for k in rest if k not in (k_empty, k_one, k_tie)][::9][:9] + [k_tie]
    references = {}
    for k in keys:
        references[k] = [paras[k]]
        if k == k_tie:
            ws = paras[k].split()
            references[k].append(" ".join(ws[:1] + ws[3:]))                       # two tokens shorter
        elif k in second:
            references[k].append(" ".join(corrupt_words(paras[k].split(), 0.1, 0.15, 0.0)))

    def video(k, lt):
        sents = [s.split() for s in steps[k]["sentences"]]
        oov = {}
        for s in sents:
            for w in s:
                if w not in word2idx and w not in oov:
                    oov[w] = V + len(oov)
        greedy_style = bool(rng.integers(0, 2))
        rows = []
        for si, s in enumerate(sents):
            if k == k_empty:
                body = []
            elif k == k_one:
                body = ["pan"] if si == 1 else []
            elif k == k_tie:
                body = s[:1] + s[2:] if si == 0 else s
            else:
                body = corrupt_words(s, 0.1, 0.12, 0.08)
            ids = [word2idx[w] if w in word2idx else oov[w] for w in body][:lt - 2]
            row = [BOS] + ids + [EOS]
            while len(row) < lt:
                row.append(int(rng.choice([EOS, UNK, plain[0], PAD])) if greedy_style else PAD)
            rows.append(row[:lt])
        return dict(key=k, oov=oov, ids=rows)

    sizes = [8] * 12
    blocks, o = [], 0
    for n in sizes:
        blocks.append(dict(lt=22, videos=[video(k, 22) for k in rest[o:o + n]]))
        o += n
    assert o == len(rest) == 96
    blocks.append(dict(lt=64, videos=[video(k, 64) for k in short]))

    # ---- the restatement on every video
    ref_tokens = [[cs.parse_sent(p) for p in references[k]] for k in keys]
    index = {k: i for i, k in enumerate(keys)}
    hyps, n_vid = {}, 0
    for b in blocks:
        for v in b["videos"]:
            h = cs.hypothesis_tokens(v["ids"], words, v["oov"])
            assert h == cs.hypothesis_tokens_per_word(v["ids"], words, v["oov"]), v["key"]
            assert len(v["ids"]) * (b["lt"] - 1) * 2 <= 1024
            assert index[v["key"]] not in hyps
            hyps[index[v["key"]]] = h
            n_vid += 1
    assert n_vid == 100 and sorted(hyps) == list(range(100))                    # no video drawn again or left out
    res, rows = cs.corpus_result(hyps, ref_tokens)
    by_index = {i: r for (i, _), r in zip(hyps.items(), rows)}
    for b in blocks:
        for v in b["videos"]:
            v["counts"], v["scores"] = by_index[index[v["key"]]]
    part = {i: h for i, h in hyps.items() if keys[i] not in short}
    res_empty, _ = cs.corpus_result(part, ref_tokens, missing="empty")

    # ---- what makes the fixture worth having
    assert all(c > 0 for c in res["correct"]), res
    clipped, zero_used, multi_used, ties = 0, False, False, 0
    for i, h in hyps.items():
        refs = ref_tokens[i]
        for n in range(1, 5):
            ch = cs.grams(h, n)
            cr = [cs.grams(r, n) for r in refs]
            clipped += sum(1 for g, c in ch.items() if c > max(x[g] for x in cr) > 0)
        if len(refs) > 1:
            d = sorted((abs(len(r) - len(h)), len(r)) for r in refs)
            ties += d[0][0] == d[1][0] and d[0][1] != d[1][1]
    for b in blocks:
        for v in b["videos"]:
            inv = {i: w for w, i in v["oov"].items()}
            for row in v["ids"]:
                for w in cs.sentence_words(cs.clean_caption(row), words, v["oov"]):
                    n = len(cs.parse_sent(w))
                    zero_used |= n == 0
                    multi_used |= n >= 2
            assert all(i >= V for i in inv)
    lens = sorted(len(h) for h in hyps.values())
    assert clipped >= 50, clipped
    assert lens[0] == 0 and 1 in lens, lens[:3]
    assert zero_used and multi_used, (zero_used, multi_used)
    assert ties >= 1, ties
    assert any(x >= V for b in blocks for v in b["videos"] for r in v["ids"] for x in r)
    out = dict(about="tools/make_golden_caption_scores.py: seeded hypothesis id rows of the validation videos, their reference paragraphs and "
                     "the restatement's Bleu / ROUGE_L / CIDEr counts and scores", seed=a.seed, V=V, pad=PAD, eos=EOS, bos=BOS, unk=UNK,
               idx2word=words, keys=keys, references=references, sentences={k: steps[k]["sentences"] for k in keys}, batches=blocks,
               corpus=res, corpus_missing_empty=res_empty, clipped_grams=int(clipped), length_ties=int(ties),
               special=dict(empty=k_empty, one_token=k_one, tie=k_tie, second_reference=second))
    with open(a.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("%s: %d batches, %d videos, correct %r of guess %r, %d clipped grams, %d tie(s), %d bytes"
          % (a.out, len(blocks), n_vid, res["correct"], res["guess"], clipped, ties, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
