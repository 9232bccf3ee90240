"""Ingredient-prediction recall / precision / F1 on the MI355X: svpc_caption_ingredients against the fixture recorded from the reference's
own functions (tests/golden/ingredient_f1.json) and the Python restatement (tests/ingredient_f1_reference.py); IngredientF1 (several
updates, determinism, ``clean=``, graph capture); and end to end on the outputs of the greedy, beam, n-best and sampling decodes."""
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
from helpers import as_views as _views, build_model, host_rows as _host_rows  # noqa: E402
from svpc_amd import ops, synthetic as syn  # noqa: E402
from svpc_amd.ingredients import IngredientLexicon, masks_to_names  # noqa: E402
from svpc_amd.metrics import DecodeMetrics, IngredientF1  # noqa: E402
from svpc_amd.synthetic import EOS, IGNORE, PAD  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = type("O", (), {"cuda": True})
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "ingredient_f1.json")))
WORDS, A, V = GOLD["idx2word"], set(GOLD["all_ingredients"]), GOLD["V"]


def _video(v):
    return dict(ingredients=v["ingredients"], oov_word_dict=v["oov"], gt_sentences=v["gt_sentences"])


def _same(got, ref):
    for k in ("n_correct", "n_recall", "n_precision"):
        assert got[k] == ref[k], (k, got, ref)
    for k in ("recall", "precision", "f1"):
        assert abs(got[k] - ref[k]) <= 1e-12, (k, got[k], ref[k])


@pytest.fixture(scope="module")
def lexicon():
    return IngredientLexicon(WORDS, A, device=DEV)


# ------------------------------------------------------------------------------------------------ 1. the kernel against the fixture
@pytest.mark.parametrize("lt", [22, 64])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_kernel_equals_the_fixture(lexicon, lt, dtype):
    blocks = [b for b in GOLD["batches"] if b["lt"] == lt]
    assert blocks
    for b in blocks:
        plan = lexicon.plan([_video(v) for v in b["videos"]])
        steps = [len(v["ids"]) for v in b["videos"]]
        ids = torch.tensor([r for v in b["videos"] for r in v["ids"]], dtype=dtype, device=DEV)
        words, ln = ops.clean_captions(ids, PAD, EOS, IGNORE, True)
        acc = torch.zeros(3, dtype=torch.int64, device=DEV)
        masks, extra, row_counts, vid_counts = ops.caption_ingredients(words, ln, plan, acc, steps=steps)
        assert masks.dtype == torch.int64 and extra.dtype == torch.int32 and tuple(row_counts.shape) == (len(ids), 3)
        masks, extra, row_counts, vid_counts = masks.cpu().tolist(), extra.cpu().tolist(), row_counts.cpu().tolist(), vid_counts.cpu().tolist()
        o = 0
        for n, v in enumerate(b["videos"]):
            tot = [0, 0, 0]
            for s, (gen, gt) in enumerate(zip(v["gen_lists"], v["gt_lists"])):
                names = masks_to_names([masks[o + s]], v["ingredients"])[0]
                assert names == gen[:len(names)] and extra[o + s] == len(gen) - len(names), (v["id"], s)
                ref = list(ir.step_counts(gen, gt))
                assert row_counts[o + s] == ref, (v["id"], s, row_counts[o + s], ref)
                tot = [x + y for x, y in zip(tot, ref)]
            assert vid_counts[n] == tot
            o += len(v["ids"])
        assert acc.cpu().tolist() == [b["n_correct"], b["n_precision"], b["n_recall"]]
        # steps default to the ground-truth step counts; acc=None accumulates nothing
        m2 = ops.caption_ingredients(words, ln, plan)[0]
        assert m2.cpu().tolist() == masks


def test_kernel_on_row_k_of_3d_ids(lexicon):
    b = GOLD["batches"][0]
    plan = lexicon.plan([_video(v) for v in b["videos"]])
    rows = [r for v in b["videos"] for r in v["ids"]]
    steps = [len(v["ids"]) for v in b["videos"]]
    rng = np.random.default_rng(4)
    junk = rng.integers(0, V, size=(len(rows), 22)).tolist()
    ids = torch.tensor([[j, r, j] for r, j in zip(rows, junk)], dtype=torch.int64, device=DEV)          # (T, 3, Lt): row 1 is the fixture's
    words, ln = ops.clean_captions(ids, PAD, EOS, IGNORE, True, row=1)
    acc = torch.zeros(3, dtype=torch.int64, device=DEV)
    ops.caption_ingredients(words, ln, plan, acc, steps=steps)
    assert acc.cpu().tolist() == [b["n_correct"], b["n_precision"], b["n_recall"]]
    f = IngredientF1(lexicon)
    views, o = [], 0
    for s in steps:
        views.append(ids[o:o + s])
        o += s
    f.update(views, plan, row=1)
    assert f.acc.cpu().tolist() == acc.cpu().tolist()
    with pytest.raises(ValueError):
        f.update(views, plan, row=3)


def test_kernel_without_ground_truth_and_ragged_steps(lexicon):
    """fewer / more generated steps than ground-truth steps (the zip), and a plan without ground truth: masks only"""
    b = GOLD["batches"][1]
    vids = b["videos"][:3]
    rows = [v["ids"][:2] for v in vids[:1]] + [v["ids"] + v["ids"][:2] for v in vids[1:2]] + [v["ids"] for v in vids[2:]]
    plan = lexicon.plan([_video(v) for v in vids])
    ids = torch.tensor([r for v in rows for r in v], dtype=torch.int64, device=DEV)
    words, ln = ops.clean_captions(ids, PAD, EOS)
    acc = torch.zeros(3, dtype=torch.int64, device=DEV)
    masks, extra, _, vid_counts = ops.caption_ingredients(words, ln, plan, acc, steps=[len(r) for r in rows])
    ref, per = ir.epoch_result([[(r, _video(v)) for r, v in zip(rows, vids)]], WORDS, A)
    assert vid_counts.cpu().tolist() == [r["counts"] for r in per]
    assert acc.cpu().tolist() == [ref["n_correct"], ref["n_precision"], ref["n_recall"]]
    assert masks.cpu().tolist() == [m for r in per for m in r["masks"]] and extra.cpu().tolist() == [x for r in per for x in r["n_extra"]]
    bare = lexicon.plan([dict(ingredients=v["ingredients"], oov_word_dict=v["oov"]) for v in vids])
    m2, e2, rc, _ = ops.caption_ingredients(words, ln, bare, acc, steps=[len(r) for r in rows])
    assert m2.cpu().tolist() == masks.cpu().tolist() and e2.cpu().tolist() == extra.cpu().tolist() and int(rc.abs().sum()) == 0
    assert acc.cpu().tolist() == [ref["n_correct"], ref["n_precision"], ref["n_recall"]]            # nothing was added
    with pytest.raises(ValueError):
        IngredientF1(lexicon).update(_views(rows, 22), bare)


def test_ids_outside_the_video_universe_match_nothing(lexicon):
    """an id that is neither a vocabulary word nor a copied word of its video (another video's copied id, a negative id) is a word that
    satisfies no predicate and is not in A: it separates its neighbours like any word"""
    b = GOLD["batches"][4]
    vids = b["videos"]
    plan = lexicon.plan([_video(v) for v in vids])
    rng = np.random.default_rng(9)
    far, neg = V + 127, -7
    rows, ref_videos = [], []
    for v in vids:
        vr = [[(far if u < 0.1 else neg if u < 0.2 else x) if p > 0 and x not in (PAD, EOS) else x
               for p, (x, u) in enumerate(zip(r, rng.random(len(r))))] for r in v["ids"]]
        rows.append(vr)
        oov = dict(v["oov"])
        oov.update({"~far~": far, "~neg~": neg})
        ref_videos.append(dict(ingredients=v["ingredients"], oov_word_dict=oov, gt_sentences=v["gt_sentences"]))
    assert all(far not in v["oov"].values() for v in vids)
    ids = torch.tensor([r for v in rows for r in v], dtype=torch.int64, device=DEV)
    words, ln = ops.clean_captions(ids, PAD, EOS)
    acc = torch.zeros(3, dtype=torch.int64, device=DEV)
    masks, extra, _, vid_counts = ops.caption_ingredients(words, ln, plan, acc)
    ref, per = ir.epoch_result([list(zip(rows, ref_videos))], WORDS, A)
    assert masks.cpu().tolist() == [m for r in per for m in r["masks"]] and extra.cpu().tolist() == [x for r in per for x in r["n_extra"]]
    assert vid_counts.cpu().tolist() == [r["counts"] for r in per]
    assert acc.cpu().tolist() == [ref["n_correct"], ref["n_precision"], ref["n_recall"]]


# ------------------------------------------------------------------------------------------------ 2. IngredientF1
def test_ingredient_f1_against_the_restatement(lexicon):
    blocks = [b for b in GOLD["batches"] if b["lt"] == 22][:5]
    seq = blocks + blocks[:2]                                       # recurring batches: their plans are cached
    f = IngredientF1(lexicon)
    for b in seq:
        plan = lexicon.plan([_video(v) for v in b["videos"]])
        counts = f.update(_views([v["ids"] for v in b["videos"]], 22), plan)
        assert counts is f.last_counts and f.last_masks.shape[0] == sum(len(v["ids"]) for v in b["videos"])
        _, per = ir.epoch_result([[(v["ids"], _video(v)) for v in b["videos"]]], WORDS, A)
        assert counts.cpu().tolist() == [r["counts"] for r in per]
    ref, _ = ir.epoch_result([[(v["ids"], _video(v)) for v in b["videos"]] for b in seq], WORDS, A)
    got = f.result()
    _same(got, ref)
    # the reference's printed numbers of one batch
    g = IngredientF1(lexicon)
    g.update(_views([v["ids"] for v in blocks[0]["videos"]], 22), lexicon.plan([_video(v) for v in blocks[0]["videos"]]))
    one = g.result()
    for k in ("recall", "precision", "f1"):
        assert abs(one[k] - blocks[0][k]) <= 1e-12
    # the same sequence again: the same bits; int32 ids in separate tensors: one copy, the same result
    f2, f3 = IngredientF1(lexicon), IngredientF1(lexicon)
    for b in seq:
        plan = lexicon.plan([_video(v) for v in b["videos"]])
        f2.update(_views([v["ids"] for v in b["videos"]], 22), plan)
        f3.update([torch.tensor(v["ids"], dtype=torch.int32, device=DEV) for v in b["videos"]], plan)
    assert torch.equal(f.acc, f2.acc) and f2.result() == got and torch.equal(f.acc, f3.acc)
    f.reset()
    assert f.result() == dict(recall=0, precision=0, f1=0, n_correct=0, n_recall=0, n_precision=0) and f.last_masks is None


def test_clean_argument_shares_one_clean_up(lexicon):
    b = GOLD["batches"][2]
    plan = lexicon.plan([_video(v) for v in b["videos"]])
    views = _views([v["ids"] for v in b["videos"]], 22)
    f, g = IngredientF1(lexicon), IngredientF1(lexicon)
    f.update(views, plan)
    ids, steps = ops.stack_captions(views)
    clean = ops.clean_captions(ids, PAD, EOS, IGNORE, True)
    g.update(views, plan, clean=clean)
    assert torch.equal(f.acc, g.acc) and torch.equal(f.last_masks, g.last_masks) and torch.equal(f.last_counts, g.last_counts)
    dm, h = DecodeMetrics(V, DEV), IngredientF1(lexicon)            # beside DecodeMetrics: its clean-up serves both counters
    assert dm.last_clean is None
    dm.update(views)
    h.update(views, plan, clean=dm.last_clean)
    assert torch.equal(dm.last_clean[0], clean[0]) and torch.equal(dm.last_clean[1], clean[1])
    assert torch.equal(f.acc, h.acc) and torch.equal(f.last_masks, h.last_masks)
    assert f.result() == g.result() and f.result()["n_correct"] == b["n_correct"]
    with pytest.raises(ValueError):
        g.update(views, plan, clean=(clean[0][:-1], clean[1][:-1]))


def test_update_captured(lexicon):
    from svpc_amd.graph import capturing
    # three batches of one (S_b) structure and one plan: the same recipes, three different decodes
    b = GOLD["batches"][3]
    vids = b["videos"]
    plan = lexicon.plan([_video(v) for v in vids])
    steps = [len(v["ids"]) for v in vids]
    base = [r for v in vids for r in v["ids"]]
    rng = np.random.default_rng(6)
    offs = np.cumsum([0] + steps)

    def shuffled():                                                # the captions of every video in another order (a video's copied ids
        return [base[offs[n] + int(i)] for n, s in enumerate(steps) for i in rng.permutation(s)]       # mean nothing in another video)
    three = [base, shuffled(), shuffled()]
    eager = IngredientF1(lexicon)
    for rows in three:
        buf = torch.tensor(rows, dtype=torch.int64, device=DEV)
        eager.update(list(torch.split(buf, steps)), plan)
    f = IngredientF1(lexicon)
    static = torch.tensor(three[0], dtype=torch.int64, device=DEV)
    views, o = [], 0
    for s in steps:
        views.append(static[o:o + s])
        o += s
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        f.update(views, plan)                                       # eager: caches the row table of this structure
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capturing(graph, stream=stream):
        f.update(views, plan)
    for rows in three[1:]:
        static.copy_(torch.tensor(rows, dtype=torch.int64, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        o, vr = 0, []
        for s in steps:
            vr.append(rows[o:o + s])
            o += s
        _, per = ir.epoch_result([[(r, _video(v)) for r, v in zip(vr, vids)]], WORDS, A)
        assert f.last_counts.cpu().tolist() == [r["counts"] for r in per]
    assert torch.equal(f.acc, eager.acc)
    assert f.result() == eager.result() and f.result()["n_precision"] > 0


# ------------------------------------------------------------------------------------------------ 3. end to end
@pytest.mark.parametrize("case", ["tiny", "c1"])
def test_ingredient_f1_end_to_end(golden_dir, case):
    from svpc_amd.translator import Translator
    z, cfg, batch, model = build_model(case, "vivt", golden_dir, DEV)
    Vm = cfg.vocab_size
    i2w = ["w%d" % i for i in range(Vm)]
    # ingredient names from the batch's ingr_id_dict (extended ids → words); ground truth: sentences over the same words
    videos, names_all = [], set()
    rng = np.random.default_rng(12)
    for d, oov, n_steps in zip(batch["ingr_id_dict"], batch["oov_word_dict"], batch["batch_step_num"]):
        inv = {int(v): k for k, v in oov.items()}
        names = [" ".join(i2w[i] if i < Vm else inv[i] for i in d[e]) for e in sorted(d)]
        names_all.update(names)
        pool = [t for n in names for t in n.split(" ")] + [i2w[int(i)] for i in rng.integers(7, Vm, size=6)]
        gt = [" ".join(pool[int(i)] for i in rng.integers(0, len(pool), size=int(rng.integers(1, 9)))) for _ in range(int(n_steps))]
        videos.append(dict(ingredients=names, oov_word_dict=oov, gt_sentences=gt))
    all_ingredients = names_all | {i2w[int(i)] for i in rng.integers(7, Vm, size=Vm // 3)}
    lex = IngredientLexicon(i2w, all_ingredients, device=DEV)
    plan = lex.plan(videos)
    tr = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model)
    before, _ = tr.translate_batch(syn.translate_inputs(batch))
    before = [d.clone() for d in before]
    f = IngredientF1(lex)
    seen = []

    greedy, _ = tr.translate_batch(syn.translate_inputs(batch))
    f.update(greedy, plan)
    seen.append(_host_rows(greedy))
    for a, b in zip(before, greedy):                                # the decode itself is untouched by a live IngredientF1
        assert torch.equal(a, b)
    for b, d in enumerate(greedy):
        np.testing.assert_array_equal(d.cpu().numpy(), z["decode/%d" % b])
    beam, _, _ = tr.translate_batch_beam(syn.translate_inputs(batch), 2)
    f.update(beam, plan)
    seen.append(_host_rows(beam))
    nbest = tr.translate_batch_nbest(syn.translate_inputs(batch), 2, 2)[0]
    assert nbest[0].dim() == 3
    counts = f.update(nbest, plan, row=1)
    seen.append(_host_rows(nbest, 1))
    _, per = ir.epoch_result([list(zip(seen[-1], videos))], i2w, all_ingredients)
    assert counts.cpu().tolist() == [r["counts"] for r in per]
    samples = tr.translate_batch_sample(syn.translate_inputs(batch), 2, seed=17)[0]
    f.update(samples, plan, row=1)
    seen.append(_host_rows(samples, 1))

    ref, _ = ir.epoch_result([list(zip(rows, videos)) for rows in seen], i2w, all_ingredients)
    got = f.result()
    _same(got, ref)
    assert got["n_recall"] > 0

    # Translator.caption_ingredients: int64 views of one buffer; the names from the masks equal the restatement's lists
    mask_list, extra_list = tr.caption_ingredients(samples, plan, row=1)
    assert mask_list[0].dtype == torch.int64 and extra_list[0].dtype == torch.int64 and mask_list[0]._base is mask_list[-1]._base
    _, per = ir.epoch_result([list(zip(seen[-1], videos))], i2w, all_ingredients)
    for m, x, r, v in zip(mask_list, extra_list, per, videos):
        assert m.cpu().tolist() == r["masks"] and x.cpu().tolist() == r["n_extra"]
        assert masks_to_names(m, v["ingredients"]) == [lst[:len(lst) - k] for lst, k in zip(r["gen"], r["n_extra"])]
