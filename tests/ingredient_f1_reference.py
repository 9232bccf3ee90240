"""Pure-Python restatement of the ingredient-prediction recall / precision / F1 (svpc_amd/csrc/ingredient.hip).

reference: src/calculate_ingredient_f1.py:6-30 (extract_ingredients: ``ingredient in sentence`` — a substring test — for the recipe's
listed ingredients, then ``word in all_ingredient_dict`` for every other word), :32-59 (calculate_ingredient_f1: the three totals over the
zip of the generated and ground-truth steps).  Token level: a caption is a word list, never a joined string.

- a word is the string of its id (``idx2word`` below V, the video's ``oov_word_dict`` from V on) after ``encode("ascii", "ignore")``;
- listed ingredient ``I[e]``, t = I[e].split(" "), is mentioned iff some position p has: k = 1: t[0] occurs inside w[p]; k ≥ 2: w[p] ends
  with t[0], w[p + j] == t[j] for the middle j, w[p + k − 1] starts with t[k − 1];
- extra words: every position whose word equals no whole string of I and is in the global set A (a word twice counts twice);
- a step's list = the mentioned listed ingredients (list order, duplicates kept) + the extra words (caption order);
- precision_total += len(gen list), recall_total += len(gt list), correct += #{x in gen list : x in gt list}, over the zip of a video's
  generated and ground-truth steps; the ratios are 0 where the reference would divide by zero.
"""
from caption_metrics_reference import clean_caption


def ascii_word(s):
    return s.encode("ascii", "ignore").decode("ascii")


def caption_words(clean_ids, idx2word, oov_word_dict):
    """a clean caption's ids → its word strings"""
    V = len(idx2word)
    inv = {int(v): k for k, v in (oov_word_dict or {}).items()}
    return [ascii_word(idx2word[i] if 0 <= i < V else inv[i]) for i in clean_ids]


def mentioned(ingredient, words):
    t = ingredient.split(" ")
    k, n = len(t), len(words)
    if k == 1:
        return any(t[0] in w for w in words)
    for p in range(n - k + 1):
        if words[p].endswith(t[0]) and words[p + k - 1].startswith(t[k - 1]) and all(words[p + j] == t[j] for j in range(1, k - 1)):
            return True
    return False


def step_list(words, ingredients, all_ingredients):
    """one step's word list → (its ingredient list, the indices e of the listed ingredients mentioned, the extra words)"""
    listed = [e for e, ing in enumerate(ingredients) if mentioned(ing, words)]
    whole = set(ingredients)
    extra = [w for w in words if w not in whole and w in all_ingredients]
    return [ingredients[e] for e in listed] + extra, listed, extra


def step_counts(gen_list, gt_list):
    """→ (correct, len(gen list), len(gt list)) of one zipped step"""
    return sum(1 for x in gen_list if x in gt_list), len(gen_list), len(gt_list)


def ratios(n_correct, n_recall, n_precision):
    recall = n_correct / n_recall if n_recall else 0.0
    precision = n_correct / n_precision if n_precision else 0.0
    f1 = 2 * recall * precision / (recall + precision) if recall + precision else 0.0
    return recall, precision, f1


def video_result(id_rows, video, idx2word, all_ingredients, remove_dup=True):
    """``id_rows``: a video's decoded id rows; ``video``: dict(ingredients, oov_word_dict, gt_sentences) →
    dict(gen lists, gt lists, masks (ints, bit e = listed ingredient e mentioned), n_extra, counts (correct, gen, gt) over the zip)"""
    ingredients = video["ingredients"]
    gen, masks, n_extra = [], [], []
    for row in id_rows:
        words = caption_words(clean_caption(row, remove_dup=remove_dup), idx2word, video.get("oov_word_dict"))
        lst, listed, extra = step_list(words, ingredients, all_ingredients)
        gen.append(lst)
        masks.append(sum(1 << e for e in listed))
        n_extra.append(len(extra))
    gt = [step_list(s.split(" "), ingredients, all_ingredients)[0] for s in video.get("gt_sentences") or ()]
    c = [0, 0, 0]
    for a, b in zip(gen, gt):
        for i, v in enumerate(step_counts(a, b)):
            c[i] += v
    return dict(gen=gen, gt=gt, masks=masks, n_extra=n_extra, counts=c)


def epoch_result(batches, idx2word, all_ingredients, remove_dup=True):
    """``batches``: lists of (id_rows, video) pairs → (the result dict of IngredientF1.result(), the per-video results)"""
    tot, per = [0, 0, 0], []
    for batch in batches:
        for rows, video in batch:
            r = video_result(rows, video, idx2word, all_ingredients, remove_dup)
            per.append(r)
            for i in range(3):
                tot[i] += r["counts"][i]
    recall, precision, f1 = ratios(tot[0], tot[2], tot[1])
    return dict(recall=recall, precision=precision, f1=f1, n_correct=tot[0], n_recall=tot[2], n_precision=tot[1]), per
