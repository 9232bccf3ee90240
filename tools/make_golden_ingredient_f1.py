"""Write tests/golden/ingredient_f1.json: seeded id captions for the 100 validation recipes and what the REFERENCE's own
``extract_ingredients`` / ``calculate_ingredient_f1`` make of them.

    python tools/make_golden_ingredient_f1.py --reference <path to the reference checkout> [--out tests/golden/ingredient_f1.json]

Only inputs and results are recorded, no reference text:
- ``extract_ingredients``, ``calculate_ingredient_f1`` and ``construct_ingredient_dict`` (src/calculate_ingredient_f1.py) are taken out of
  their file with ``ast`` (the file imports tqdm), ``convert_ids_to_sentence`` and ``remove_dup`` as tools/make_golden_caption_metrics.py
  takes them; the generated sentence is ``remove_dup(convert_ids_to_sentence(row, oov))`` after ``encode("ascii", "ignore")``
  (src/translate.py:82-84);
- vocabulary: the 951 words of cache/yc2_word2idx.json; the global ingredient strings: what ``construct_ingredient_dict`` collects; the
  recipes: every one of densevid_eval/yc2_data/bosselut_split_yc2_val_anet_format.json with its ingredient list and sentences; a
  recipe's OOV dictionary: its ingredient tokens (lower-cased, split on blanks) outside the vocabulary, ids V, V + 1, … in order of
  appearance (clip_ingredient_to_feature's numbering);
- one id row per ground-truth sentence: BOS, 0 … Lt − 1 words, EOS, then PAD fill (beam style) or junk with further EOS (greedy style).
  ≈45 % of the words come from the recipe's ingredient tokens (whole ingredients in order, or single tokens), ≈10 % are vocabulary words
  that merely contain / end with / start with an ingredient token (``boil`` for ``oil``), the rest come from the vocabulary and the
  recipe's copied words; a word repeats the one before it with probability 0.2, so the run collapse interacts with the patterns;
- per recipe: the id rows, the reference's step lists for the generated and the ground-truth sentences; per batch of recipes: recall /
  precision / f1 as ``calculate_ingredient_f1`` printed them and the three totals (counted from the reference's step lists; their ratios
  are asserted equal to the printed values).
No caption is drawn again or left out: the reference scores every one, and the token-level rule (tests/ingredient_f1_reference.py)
must reproduce every step list — asserted here, with the coverage the tests rely on.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ingredient_f1_reference as ref_rule  # noqa: E402
from caption_metrics_reference import clean_caption  # noqa: E402
from make_golden_caption_metrics import function_from  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, IGNORE, N_SPECIAL, PAD, UNK  # noqa: E402


def whole_word_listed(ingredients, words):
    """the rule an id-level whole-word matcher would apply (what the fixture must tell apart from the reference's)"""
    out = []
    for e, ing in enumerate(ingredients):
        t = ing.split(" ")
        if any(words[p:p + len(t)] == t for p in range(len(words) - len(t) + 1)):
            out.append(e)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ingredient_f1.json"))
    ap.add_argument("--seed", type=int, default=2019)
    a = ap.parse_args(argv)
    src = os.path.join(a.reference, "src", "calculate_ingredient_f1.py")
    extract = function_from(src, "extract_ingredients")
    calc = function_from(src, "calculate_ingredient_f1")
    calc.__globals__["extract_ingredients"] = extract
    construct = function_from(src, "construct_ingredient_dict")
    construct.__globals__.update(os=os, json=json)
    remove_dup = function_from(os.path.join(a.reference, "src", "translate.py"), "remove_dup")
    to_sentence = function_from(os.path.join(a.reference, "src", "rtransformer", "recursive_caption_dataset.py"),
                                "convert_ids_to_sentence", inside_class="RecursiveCaptionDataset")
    cwd = os.getcwd()
    os.chdir(a.reference)
    try:
        A = construct()
    finally:
        os.chdir(cwd)
    word2idx = json.load(open(os.path.join(a.reference, "cache", "yc2_word2idx.json")))
    V = len(word2idx)
    words = [None] * V
    for w, i in word2idx.items():
        words[i] = w
    assert all(w is not None for w in words) and words[PAD] == "[PAD]" and words[EOS] == "[EOS]" and words[BOS] == "[BOS]"
    idx2word = {i: w for i, w in enumerate(words)}
    stub = type("Stub", (), dict(idx2word=idx2word, PAD=PAD, IGNORE=IGNORE, EOS_TOKEN=words[EOS]))()
    val = json.load(open(os.path.join(a.reference, "densevid_eval", "yc2_data", "bosselut_split_yc2_val_anet_format.json")))
    rng = np.random.default_rng(a.seed)
    plain = list(range(N_SPECIAL, V))

    def recipe(rid, ann, lt):
        ingredients, sentences = list(ann["ingredients"]), list(ann["sentences"])
        oov = {}
        for ing in ingredients:
            for t in ing.lower().split():
                if t not in word2idx and t not in oov:
                    oov[t] = V + len(oov)
        to_id = lambda t: word2idx[t] if t in word2idx else oov.get(t)            # noqa: E731
        ing_ids = [[to_id(t) for t in ing.split(" ")] for ing in ingredients]
        ing_ids = [x for x in ing_ids if all(i is not None for i in x)]
        toks = sorted({t for ing in ingredients for t in ing.split(" ") if t})
        near = sorted({word2idx[w] for w in words[N_SPECIAL:] for t in toks if t in w and w != t})   # `boil` for `oil`
        greedy_style = bool(rng.integers(0, 2))
        rows = []
        for _ in sentences:
            n = int(rng.integers(0, lt))
            body = []
            while len(body) < n:
                u = rng.random()
                if body and u < 0.2:
                    body.append(body[-1])
                elif u < 0.5 and ing_ids:
                    body += ing_ids[int(rng.integers(0, len(ing_ids)))]
                elif u < 0.65 and ing_ids:
                    x = ing_ids[int(rng.integers(0, len(ing_ids)))]
                    body.append(x[int(rng.integers(0, len(x)))])
                elif u < 0.75 and near:
                    body.append(near[int(rng.integers(0, len(near)))])
                elif u < 0.8 and oov:
                    body.append(V + int(rng.integers(0, len(oov))))
                elif u < 0.83:
                    body.append(int(rng.choice([PAD, UNK, BOS])))
                else:
                    body.append(plain[int(rng.integers(0, len(plain)))])
            row = [BOS] + body[:n] + [EOS]
            while len(row) < lt:
                row.append(int(rng.choice([EOS, UNK, plain[0], PAD])) if greedy_style else PAD)
            rows.append(row[:lt])
        gen = [remove_dup(to_sentence(stub, row, oov)).encode("ascii", "ignore").decode("ascii") for row in rows]
        return dict(id=rid, ingredients=ingredients, gt_sentences=sentences, oov=oov, ids=rows, gen_sentences=gen)

    rids = list(val)
    assert len(rids) == 100
    sizes = [8] * 12 + [4]
    blocks, o = [], 0
    for bi, n in enumerate(sizes):
        lt = 64 if bi == len(sizes) - 1 else 22
        vids = [recipe(r, val[r], lt) for r in rids[o:o + n]]
        o += n
        rd = {"gt": {v["id"]: {"ingredients": v["ingredients"], "sentences": v["gt_sentences"]} for v in vids},
              "model": {v["id"]: {"ingredients": v["ingredients"], "sentences": v["gen_sentences"]} for v in vids}}
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            calc(rd, A)                                   # (fills step_ingredients in place, prints the three ratios)
        printed = {}
        for line in out.getvalue().splitlines():
            for k in ("recall", "precision", "f1"):
                if line.startswith(k + ":"):
                    printed[k] = float(line.split(":")[1])
        tot = [0, 0, 0]
        for v in vids:
            v["gen_lists"] = rd["model"][v["id"]]["step_ingredients"]
            v["gt_lists"] = rd["gt"][v["id"]]["step_ingredients"]
            for g, t in zip(v["gen_lists"], v["gt_lists"]):
                tot[0] += sum(1 for x in g if x in t)
                tot[1] += len(t)
                tot[2] += len(g)
            del v["gen_sentences"]
        assert printed["recall"] == tot[0] / tot[1] and printed["precision"] == tot[0] / tot[2], (printed, tot)
        blocks.append(dict(lt=lt, videos=vids, recall=printed["recall"], precision=printed["precision"], f1=printed["f1"],
                           n_correct=tot[0], n_recall=tot[1], n_precision=tot[2]))
    assert o == 100

    # ---- what the fixture must contain, and the token-level rule on every caption
    n_cap = differs = 0
    ks, has_dup, has_copied, has_empty, has_repeat = set(), False, False, False, False
    for b in blocks:
        for v in b["videos"]:
            video = dict(ingredients=v["ingredients"], oov_word_dict=v["oov"], gt_sentences=v["gt_sentences"])
            r = ref_rule.video_result(v["ids"], video, words, A)
            assert r["gen"] == v["gen_lists"] and r["gt"] == v["gt_lists"], v["id"]
            has_dup |= len(set(v["ingredients"])) < len(v["ingredients"])
            ks |= {len(i.split(" ")) for i in v["ingredients"]}
            for row, lst, m in zip(v["ids"], v["gen_lists"], r["masks"]):
                n_cap += 1
                cw = ref_rule.caption_words(clean_caption(row), words, v["oov"])
                got = [e for e in range(len(v["ingredients"])) if (m >> e) & 1]
                differs += got != whole_word_listed(v["ingredients"], cw)
                has_copied |= any(x >= V for x in row)
                has_empty |= not cw
                extra = lst[len(got):]
                has_repeat |= len(set(extra)) < len(extra)
    assert n_cap == sum(len(v["sentences"]) for v in val.values()) == 798, n_cap
    assert differs >= 20, differs
    assert ks >= {2, 3, 4} and has_dup and has_copied and has_empty and has_repeat, (ks, has_dup, has_copied, has_empty, has_repeat)
    res = dict(about="tools/make_golden_ingredient_f1.py: seeded id captions of the validation recipes and the reference's own step lists "
                     "and recall / precision / f1", seed=a.seed, V=V, pad=PAD, eos=EOS, bos=BOS, unk=UNK, ignore=IGNORE, idx2word=words,
               all_ingredients=sorted(A), captions=n_cap, substring_differs_from_whole_word=int(differs), batches=blocks)
    with open(a.out, "w") as f:
        json.dump(res, f, separators=(",", ":"))
    print("%s: %d batches, %d recipes, %d captions, %d differ from whole-word matching, %d bytes"
          % (a.out, len(blocks), 100, n_cap, differs, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
