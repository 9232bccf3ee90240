"""Ingredient-prediction recall / precision / F1 without a GPU: the Python restatement (tests/ingredient_f1_reference.py) against the
fixture recorded from the reference's own functions (tests/golden/ingredient_f1.json, tools/make_golden_ingredient_f1.py); the bit tables
``svpc_amd.ingredients`` compiles, bit by bit against direct string tests, and — walked id by id the way the kernel walks them — against
the restatement; hand-built edges; every host check; the no-CPU-fallback rule; the C-ABI declaration."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import ingredient_f1_reference as ir  # noqa: E402
from caption_metrics_reference import clean_caption, clean_rows  # noqa: E402
from svpc_amd import _lib, ingredients as ing, ops  # noqa: E402
from svpc_amd.ingredients import IngredientLexicon  # noqa: E402
from svpc_amd.metrics import IngredientF1  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, PAD  # noqa: E402

GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "ingredient_f1.json")))
WORDS, A, V = GOLD["idx2word"], set(GOLD["all_ingredients"]), GOLD["V"]


def _video(v):
    return dict(ingredients=v["ingredients"], oov_word_dict=v["oov"], gt_sentences=v["gt_sentences"])


def _bit(row, i):
    return (int(row[i >> 5]) >> (i & 31)) & 1


def _u32(t):
    return t.numpy().view(np.uint32)


def walk_plan(plan, rows, steps, lt):
    """The kernel's walk over the packed tables, in Python on ids alone: → (masks, extra counts, (T, 3) row counts)."""
    lex = plan.lexicon
    table, a_bits = _u32(lex.table), _u32(lex.a_bits)
    sec = {k: plan.section(k).numpy() for k in plan.sections}
    tok_oov, oov_a, gt_mask = (sec[k].view(np.uint32) for k in ("tok_oov", "oov_a", "gt_mask"))
    rv = plan.rows(steps).numpy()
    N = plan.n_vid
    assert rv[:N + 1].tolist() == np.cumsum([0] + list(steps)).tolist()
    clean, lens = clean_rows(rows, lt)
    masks, extras, counts = [], [], []
    for r, (cw, n) in enumerate(zip(clean, lens)):
        b, s = int(rv[N + 1 + 2 * r]), int(rv[N + 2 + 2 * r])
        ing0, E, X, eq0, n_eq, gt0, n_gt, _ = (int(x) for x in sec["vid"][8 * b:8 * b + 8])
        w = cw[:n]

        def pred(j, word):
            if 0 <= word < lex.V:
                row = int(sec["tok_row"][j])
                assert 0 <= row < lex.n_rows
                return _bit(table[row], word)
            x = word - lex.V
            return _bit(tok_oov[4 * j:4 * j + 4], x) if 0 <= x < X else 0
        mask = 0
        for e in range(E):
            t0, t1 = int(sec["ing_tok"][ing0 + e]), int(sec["ing_tok"][ing0 + e + 1])
            if t1 > t0 and any(all(pred(t0 + j, w[p + j]) for j in range(t1 - t0)) for p in range(n - (t1 - t0) + 1)):
                mask |= 1 << e
        eq = set(sec["eq_ids"][eq0:eq0 + n_eq].tolist())

        def in_a(word):
            if 0 <= word < lex.V:
                return _bit(a_bits, word)
            x = word - lex.V
            return _bit(oov_a[4 * b:4 * b + 4], x) if 0 <= x < X else 0
        extra = [x for x in w if x not in eq and in_a(x)]
        c = [0, 0, 0]
        if s < n_gt:
            g = gt0 + s
            gm = int(gt_mask[2 * g]) | (int(gt_mask[2 * g + 1]) << 32)
            gx = set(sec["gx_ids"][int(sec["gx_off"][g]):int(sec["gx_off"][g + 1])].tolist())
            c = [bin(mask & gm).count("1") + sum(1 for x in extra if x in gx), bin(mask).count("1") + len(extra), int(sec["gt_len"][g])]
        masks.append(mask)
        extras.append(len(extra))
        counts.append(c)
    return masks, extras, counts


# ------------------------------------------------------------------------------------------------ 1. fixture and restatement
def test_fixture_covers_the_rule():
    assert (GOLD["pad"], GOLD["eos"], GOLD["bos"]) == (PAD, EOS, BOS) and V == 951 == len(WORDS)
    vids = [v for b in GOLD["batches"] for v in b["videos"]]
    assert len(vids) == 100 and {b["lt"] for b in GOLD["batches"]} == {22, 64}
    rows = [r for v in vids for r in v["ids"]]
    assert len(rows) == GOLD["captions"] == 798 and GOLD["substring_differs_from_whole_word"] >= 20
    assert {len(i.split(" ")) for v in vids for i in v["ingredients"]} >= {1, 2, 3, 4}
    assert sum(1 for v in vids if len(set(v["ingredients"])) < len(v["ingredients"])) >= 1
    assert any(x >= V for r in rows for x in r)
    assert any(not clean_caption(r) for r in rows)
    with_eos = [r for r in rows if EOS in r]
    assert any(r[-1] == PAD for r in with_eos) and any(EOS in r[r.index(EOS) + 1:] for r in with_eos)        # both fill styles
    assert {len(clean_caption(r)) for r in rows if len(r) == 22} >= set(range(0, 15))


def test_restatement_equals_the_reference():
    differs = 0
    for b in GOLD["batches"]:
        res, per = ir.epoch_result([[(v["ids"], _video(v)) for v in b["videos"]]], WORDS, A)
        for v, r in zip(b["videos"], per):
            assert r["gen"] == v["gen_lists"], v["id"]
            assert r["gt"] == v["gt_lists"], v["id"]
            for row, m in zip(v["ids"], r["masks"]):
                cw = ir.caption_words(clean_caption(row), WORDS, v["oov"])
                whole = sum(1 << e for e, i in enumerate(v["ingredients"])
                            if any(cw[p:p + len(i.split(" "))] == i.split(" ") for p in range(len(cw))))
                differs += whole != m
        assert (res["n_correct"], res["n_recall"], res["n_precision"]) == (b["n_correct"], b["n_recall"], b["n_precision"])
        for k in ("recall", "precision", "f1"):
            assert abs(res[k] - b[k]) <= 1e-12, (k, res[k], b[k])
    assert differs == GOLD["substring_differs_from_whole_word"] >= 20


# ------------------------------------------------------------------------------------------------ 2. the compiled tables
def test_predicate_tables_equal_direct_string_tests():
    lex = IngredientLexicon(WORDS, A, device="cpu")
    plans = [lex.plan([_video(v) for v in b["videos"]]) for b in GOLD["batches"]]
    preds = lex.predicates()
    assert len(preds) == lex.n_rows > 100 and {k for k, _ in preds} == {ing.CONTAINS, ing.ENDS, ing.EQUALS, ing.STARTS}
    table = _u32(lex.table)
    direct = {ing.CONTAINS: lambda t, w: w.find(t) >= 0, ing.ENDS: lambda t, w: w[len(w) - len(t):] == t and len(t) <= len(w),
              ing.EQUALS: lambda t, w: w == t, ing.STARTS: lambda t, w: w[:len(t)] == t}
    for row, (kind, t) in enumerate(preds):
        for i, w in enumerate(WORDS):
            assert _bit(table[row], i) == int(direct[kind](t, w)), (kind, t, w)
        assert not table[row][-1] >> (V - 32 * (lex.W - 1)) if V % 32 else True       # no bit past the vocabulary
    a_bits = _u32(lex.a_bits)
    assert [_bit(a_bits, i) for i in range(V)] == [int(w in A) for w in WORDS]
    # per video: the token CSR, the predicates on the copied words, the whole-ingredient ids, the copied words in A
    for b, plan in zip(GOLD["batches"], plans):
        sec = {k: plan.section(k).numpy() for k in plan.sections}
        for n, v in enumerate(b["videos"]):
            ing0, E, X, eq0, n_eq, gt0, n_gt, _ = (int(x) for x in sec["vid"][8 * n:8 * n + 8])
            assert E == len(v["ingredients"]) and X == len(v["oov"]) and n_gt == len(v["gt_sentences"])
            inv = {i: w for w, i in v["oov"].items()}
            for e, name in enumerate(v["ingredients"]):
                t0, t1 = int(sec["ing_tok"][ing0 + e]), int(sec["ing_tok"][ing0 + e + 1])
                toks = name.split(" ")
                assert t1 - t0 == len(toks)
                for j, t in enumerate(toks):
                    kind = ing.CONTAINS if len(toks) == 1 else ing.ENDS if j == 0 else ing.STARTS if j == len(toks) - 1 else ing.EQUALS
                    assert preds[int(sec["tok_row"][t0 + j])] == (kind, t)
                    bits = sec["tok_oov"].view(np.uint32)[4 * (t0 + j):4 * (t0 + j) + 4]
                    assert [_bit(bits, x) for x in range(128)] == [int(x < X and direct[kind](t, inv[V + x])) for x in range(128)]
            universe = {i: w for i, w in enumerate(WORDS)}
            universe.update(inv)
            assert sec["eq_ids"][eq0:eq0 + n_eq].tolist() == sorted(i for i, w in universe.items() if w in set(v["ingredients"]))
            assert [_bit(sec["oov_a"].view(np.uint32)[4 * n:4 * n + 4], x) for x in range(128)] == [int(x < X and inv[V + x] in A)
                                                                                                   for x in range(128)]
            for s, lst in enumerate(v["gt_lists"]):
                assert int(sec["gt_len"][gt0 + s]) == len(lst)


def test_table_walk_equals_the_restatement_on_the_fixture():
    lex = IngredientLexicon(WORDS, A, device="cpu")
    for b in GOLD["batches"]:
        plan = lex.plan([_video(v) for v in b["videos"]])
        assert lex.plan([_video(v) for v in b["videos"]]) is plan                    # cached: a recurring batch uploads nothing
        steps = [len(v["ids"]) for v in b["videos"]]
        masks, extras, counts = walk_plan(plan, [r for v in b["videos"] for r in v["ids"]], steps, b["lt"])
        assert plan.rows(steps) is plan.rows(steps)
        _, per = ir.epoch_result([[(v["ids"], _video(v)) for v in b["videos"]]], WORDS, A)
        assert masks == [m for r in per for m in r["masks"]]
        assert extras == [x for r in per for x in r["n_extra"]]
        assert [sum(c[i] for c in counts) for i in range(3)] == [b["n_correct"], b["n_precision"], b["n_recall"]]
        o = 0
        for v, r in zip(b["videos"], per):
            n = len(v["ids"])
            assert [sum(c[i] for c in counts[o:o + n]) for i in range(3)] == r["counts"]
            assert ing.masks_to_names(masks[o:o + n], v["ingredients"]) == [lst[:len(lst) - x] for lst, x in zip(r["gen"], r["n_extra"])]
            o += n


# ------------------------------------------------------------------------------------------------ 3. hand-built edges
EDGE_WORDS = ["[PAD]", "[CLS]", "[SEP]", "[VID]", "[BOS]", "[EOS]", "[UNK]", "add", "oil", "boil", "olive", "the", "pan", "olives", "red",
              "wine", "vinegar", "salt", "onions", "winery", "soy", "sauce", "to", "unsalted"]
EDGE_A = {"oil", "olive oil", "salt", "pan", "red wine vinegar", "sauce", "mirin", "xo", "soy sauce"}


def _ids(sentence, oov=None):
    w2i = {w: i for i, w in enumerate(EDGE_WORDS)}
    w2i.update(oov or {})
    body = [w2i[w] for w in sentence.split(" ")] if sentence else []
    return ([BOS] + body + [EOS] + [PAD] * 22)[:22]


def _edge(video, sentences):
    """restatement and table walk of one video's captions → (names per step, extra counts, counts)"""
    lex = IngredientLexicon(EDGE_WORDS, EDGE_A, device="cpu")
    rows = [_ids(s, video.get("oov_word_dict")) for s in sentences]
    r = ir.video_result(rows, video, EDGE_WORDS, EDGE_A)
    plan = lex.plan([video])
    masks, extras, counts = walk_plan(plan, rows, [len(rows)], 22)
    assert masks == r["masks"] and extras == r["n_extra"]
    assert [sum(c[i] for c in counts) for i in range(3)] == r["counts"]
    # the reference's own statement of the rule on the joined string
    for row, lst in zip(rows, r["gen"]):
        s = " ".join(ir.caption_words(clean_caption(row), EDGE_WORDS, video.get("oov_word_dict")))
        ref = [i for i in video["ingredients"] if i in s] + [w for w in s.split(" ") if w not in video["ingredients"] and w in EDGE_A]
        assert lst == ref, (s, lst, ref)
    return ing.masks_to_names(masks, video["ingredients"]), extras, r["counts"]


def test_edges():
    # oil inside boil: a substring, not a word; `salt` inside `unsalted`
    names, extra, _ = _edge(dict(ingredients=["oil", "salt"], gt_sentences=["add oil"]), ["boil the pan", "add unsalted olives"])
    assert names == [["oil"], ["salt"]] and extra == [1, 0]                       # (`pan` is an extra word; `boil` is not in A)
    # a pattern at the caption's last position, and one that would need a word past it
    names, _, _ = _edge(dict(ingredients=["olive oil", "red wine vinegar"], gt_sentences=[]), ["add olive oil", "add red wine", "olive"])
    assert names == [["olive oil"], [], []]
    # k >= 2 has substring ends too: `boil olives` does not hold `olive oil`, `olive oil` is inside `olive boil`? no — the first word must
    # END with `olive` and the last START with `oil`
    names, _, _ = _edge(dict(ingredients=["olive oil", "wine"], gt_sentences=[]), ["olive boil", "olives oil", "olive oil", "the winery"])
    assert names == [[], [], ["olive oil"], ["wine"]]
    # a duplicate ingredient counts twice, in both lists
    names, _, c = _edge(dict(ingredients=["salt", "oil", "salt"], gt_sentences=["add salt to the pan"]), ["add salt"])
    assert names == [["salt", "salt"]] and c == [2, 2, 3]
    # an empty caption; more generated steps than ground truth (the zip) and fewer
    names, extra, c = _edge(dict(ingredients=["oil"], gt_sentences=["add oil"]), ["", "add oil", "add oil"])
    assert names == [[], ["oil"], ["oil"]] and c == [0, 0, 1]
    _, _, c = _edge(dict(ingredients=["oil"], gt_sentences=["add oil", "add salt", "boil"]), ["add oil"])
    assert c == [1, 1, 1]
    # k = 4
    names, _, _ = _edge(dict(ingredients=["red wine vinegar sauce"], gt_sentences=[]),
                        ["add red wine vinegar sauce to the pan", "add red wine sauce", "red wine vinegar", "unsalted red wine vinegar sauce"])
    assert names == [["red wine vinegar sauce"], [], [], ["red wine vinegar sauce"]]
    # a copied word as first and as last pattern token, as a k = 1 pattern, as an extra word and as a whole listed ingredient
    oov = {"mirin": len(EDGE_WORDS), "xo": len(EDGE_WORDS) + 1, "oxo": len(EDGE_WORDS) + 2}
    names, extra, c = _edge(dict(ingredients=["mirin sauce", "soy mirin", "xo"], oov_word_dict=oov, gt_sentences=["add mirin sauce", "xo mirin"]),
                            ["add mirin sauce", "soy mirin oxo", "mirin mirin xo"])
    assert names == [["mirin sauce"], ["soy mirin", "xo"], ["xo"]] and extra == [2, 1, 1]       # `mirin` is in A and not a whole ingredient
    assert c == [3 + 2, 3 + 3, 3 + 2]                                             # (the third caption has no ground-truth step)
    # repeated extra words count twice; a ground-truth extra word outside the video's words only counts in the length
    _, extra, c = _edge(dict(ingredients=["oil"], gt_sentences=["pan sauce mirin"]), ["pan the pan sauce"])
    assert extra == [3] and c == [3, 3, 3]
    # run collapse first: `olive olive oil` is `olive oil`
    names, _, _ = _edge(dict(ingredients=["olive oil"], gt_sentences=[]), ["olive olive oil oil"])
    assert names == [["olive oil"]]


def test_ratios_are_zero_where_the_reference_divides_by_zero():
    assert ir.ratios(0, 0, 0) == (0.0, 0.0, 0.0) and ir.ratios(0, 3, 0) == (0.0, 0.0, 0.0) and ir.ratios(0, 3, 2) == (0.0, 0.0, 0.0)
    from svpc_amd.metrics import compute_total_f1
    assert compute_total_f1(0, 0, 0) == dict(recall=0, precision=0, f1=0)


# ------------------------------------------------------------------------------------------------ 4. host checks
def test_value_errors():
    lex = IngredientLexicon(EDGE_WORDS, EDGE_A, device="cpu")
    n = len(EDGE_WORDS)
    with pytest.raises(ValueError):
        IngredientLexicon(["a", "café", "é"], EDGE_A, device="cpu")               # a word that is empty after ascii / ignore
    with pytest.raises(ValueError):
        IngredientLexicon(["a", "b c"], EDGE_A, device="cpu")                                # a blank inside a word
    with pytest.raises(ValueError):
        IngredientLexicon([], EDGE_A, device="cpu")
    with pytest.raises(ValueError):
        IngredientLexicon({0: "a", 2: "b"}, EDGE_A, device="cpu")
    with pytest.raises(ValueError):
        lex.plan([dict(ingredients=["oil", ""])])                                            # an empty ingredient string
    with pytest.raises(ValueError):
        lex.plan([dict(ingredients=["oil"], oov_word_dict={"é": n})])                   # a copied word empty after ascii
    with pytest.raises(ValueError):
        lex.plan([dict(ingredients=["oil"], oov_word_dict={"a b": n})])
    with pytest.raises(ValueError):
        lex.plan([dict(ingredients=["oil"], oov_word_dict={"a": n - 1})])                    # a copied id inside the vocabulary
    with pytest.raises(ValueError):
        lex.plan([dict(ingredients=["oil"], oov_word_dict={"a": n + 128})])                  # the 129th copied word
    with pytest.raises(ValueError):
        lex.plan([dict(ingredients=["oil"], oov_word_dict={"a": n, "b": n})])
    with pytest.raises(ValueError):
        lex.plan([dict(ingredients=["i%d" % i for i in range(65)])])                         # 65 ingredients
    with pytest.raises(ValueError):
        lex.plan([dict(ingredients=["a b c"] * 43)])                                         # 129 pattern tokens
    with pytest.raises(ValueError):
        lex.plan([])
    lex.plan([dict(ingredients=["i%d" % i for i in range(64)], oov_word_dict={"w%d" % i: n + i for i in range(128)})])      # at the caps
    lex.plan([dict(ingredients=["a b"] * 64)])
    plan = lex.plan([dict(ingredients=["oil"], gt_sentences=["add oil", "boil"]), dict(ingredients=["salt"], gt_sentences=["salt"])])
    words, ln = torch.zeros(3, 22, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.caption_ingredients(torch.zeros(3, 65, dtype=torch.int32), ln, plan)             # Lt > 64
    with pytest.raises(ValueError):
        ops.caption_ingredients(words.to(torch.int64), ln, plan)
    with pytest.raises(ValueError):
        ops.caption_ingredients(words, ln.to(torch.int64), plan)
    with pytest.raises(ValueError):
        ops.caption_ingredients(words, ln, plan, steps=[2, 2])                               # rows do not add up
    with pytest.raises(ValueError):
        ops.caption_ingredients(words, ln, plan, steps=[3])                                  # one count per video
    with pytest.raises(ValueError):
        ops.caption_ingredients(words, ln, plan, acc=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.caption_ingredients(words, ln, plan, acc=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.caption_ingredients(words, ln, lex.plan([dict(ingredients=["oil"])]))            # no ground truth: steps are required
    with pytest.raises(ValueError):
        plan.rows([1, -1])


def test_no_cpu_fallback():
    lex = IngredientLexicon(EDGE_WORDS, EDGE_A, device="cpu")
    with pytest.raises(_lib.SvpcKernelError):
        IngredientF1(lex)
    plan = lex.plan([dict(ingredients=["oil"], gt_sentences=["add oil"])])
    with pytest.raises(_lib.SvpcKernelError):
        ops.caption_ingredients(torch.zeros(1, 22, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), plan)


def test_lexicon_table_grows_and_keeps_its_rows():
    lex = IngredientLexicon(EDGE_WORDS, EDGE_A, device="cpu")
    lex.plan([dict(ingredients=["oil", "olive oil"])])
    first = _u32(lex.table)[:lex.n_rows].copy()
    k = lex.n_rows
    lex.plan([dict(ingredients=["x%d y%d" % (i, i) for i in range(60)]) for _ in range(1)])
    for j in range(6):
        lex.plan([dict(ingredients=["z%d_%d" % (j, i) for i in range(60)])])
    assert lex.n_rows == k + 120 + 360 > 256 and lex.table.shape[0] >= lex.n_rows and len(lex._retired) >= 1
    assert (_u32(lex.table)[:k] == first).all()
    assert lex.row_of(ing.CONTAINS, "oil") == 0 and lex.n_rows == k + 480                  # a known predicate is not added again


def test_symbol_declared_and_exported():
    decls = _lib.declarations()
    lib = _lib.load()
    assert "svpc_caption_ingredients" in decls and len(decls["svpc_caption_ingredients"][1]) == 28
    assert hasattr(lib, "svpc_caption_ingredients")
    assert lib.svpc_abi_version() == 2
