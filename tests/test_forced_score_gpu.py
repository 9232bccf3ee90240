"""Forced decoding on the MI355X: svpc_force_inputs / svpc_force_score / svpc_force_finish against the restatement
(tests/forced_score_reference.py) on seeded random rows, exactly; ``Translator.score_captions`` against the CPU restatement built on the
oracle's decoder blocks (gold labels, the decoder's own n-best rows, sampled rows); against the decodes' own scores; copied words,
``unk="skip"``, determinism, graph replay, ``metrics.ForcedScores``, ``consensus(weights="posterior")``; and the bf16x3 deviation.

Bounds.  Kernel against the restatement: everything equal, cum bit for bit (the step score is computed in fp64 and rounded once on both
sides, the sum runs in fp32 in position order on both sides).  Translator against the restatement (fp32): cum and step within rtol
1e-4 / atol 1e-6 (``test_beam_gpu._compare``'s bound for translator scores), len / finished / n_scored exactly, rank exactly wherever the
restatement's gap — the distance in step score from the target to its nearer neighbour in the decoder's order — exceeds 1e-4; at most
5 % of a fixture's ranked positions (its three caption sources together) may fall under that gap, asserted on the restatement alone.
bf16x3: see ``BOUND_X3``."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import forced_score_reference as fr  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import ops, synthetic as syn  # noqa: E402
from svpc_amd.ops_common import Idx  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, IGNORE, PAD, UNK  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = type("O", (), {"cuda": True})
GAP = 1e-4
SAMPLE_SEED = 2            # a seed whose samples never pick PAD as a word on any fixture (see ``_sources``)
REPORT_DIR = os.environ.get("SVPC_REPORT_DIR") or os.path.join(ROOT, "reports")
# bf16x3 at the config-1 shape: the worst |cum − fp32 CPU restatement| measured over the three caption sources of ("c1", "v") and
# ("c1", "vivt") on the MI355X was MEASURED_X3 (profiles/forced_score_parity.json); the assertion is at twice that, the margin for
# the split-product rounding varying with the caption.
MEASURED_X3 = 0.001529693603515625        # ("c1", "vivt"), n-best rows; cum there is about −160
BOUND_X3 = 2.0 * MEASURED_X3


# ------------------------------------------------------------------------------------------------ 1. the kernels
#        C,  Lt,  T,  K, id dtype          (R = T·K caption rows, R·(Lt − 1) score rows: 1, and counts that are no multiple of the 4 per workgroup)
SHAPES = [(7, 2, 1, 1, torch.int64), (64, 22, 3, 3, torch.int32), (65, 64, 2, 1, torch.int64), (951, 22, 2, 16, torch.int32),
          (1025, 22, 3, 3, torch.int64), (4097, 6, 5, 1, torch.int32)]


def _random_case(rng, C, Lt, R, logits, adversarial):
    """score rows, captions and column counts: mixed C_r in one launch; captions that end at position 1, never end, are all PAD, stop at
    IGNORE; targets at UNK, at C_r, below 0; (adversarial) rows of few distinct values and zero probabilities"""
    row_c = np.array([C if r % 3 == 0 else int(rng.integers(max(UNK + 1, C // 2), C + 1)) for r in range(R)])
    if adversarial:
        vals = np.array([0.0, 0.125, 0.25, 0.5] if not logits else [-3.0, -1.0, 0.0, 2.0], np.float32)
        s = vals[rng.integers(0, len(vals), size=(R * Lt, C))]
    else:
        s = (rng.random((R * Lt, C)) ** 4).astype(np.float32) if not logits else rng.standard_normal((R * Lt, C)).astype(np.float32) * 3
    s[:, UNK] = 1.0 if not logits else 50.0            # UNK would win every comparison were it a candidate
    ids = np.zeros((R, Lt), np.int64)
    ids[:, 0] = BOS
    for r in range(R):
        c = int(row_c[r])
        words = rng.integers(1, c, size=Lt - 1)
        words[words == EOS] = 1
        kind = r % 6
        n = int(rng.integers(0, Lt - 1))               # words before the end
        if kind == 0:
            row = list(words)                                          # never ends
        elif kind == 1:
            row = [EOS] + [PAD] * (Lt - 2)                             # ends at position 1
        elif kind == 2:
            row = [PAD] * (Lt - 1)                                     # all PAD
        elif kind == 3:
            row = list(words[:n]) + [IGNORE] * (Lt - 1 - n)
        else:
            row = list(words[:n]) + [EOS] + [PAD] * (Lt - 2 - n)
            if n:                                                      # a non-candidate target somewhere before the end
                row[int(rng.integers(0, n))] = [UNK, c, -7, c + 3][int(rng.integers(0, 4))]
        ids[r, 1:] = row[:Lt - 1]
    return s, ids, row_c


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("C,Lt,T,K,dtype", SHAPES)
def test_kernels_equal_the_restatement(C, Lt, T, K, dtype, logits):
    rng = np.random.default_rng(1000 * C + Lt + logits)
    R = T * K
    for adversarial in (False, True):
        s, ids, row_c = _random_case(rng, C, Lt, R, logits, adversarial)
        sd = torch.from_numpy(s).to(DEV)
        idd = torch.from_numpy(ids).to(DEV).to(dtype).view(T, K, Lt)
        V = max(UNK + 1, C - 2)                        # text vocabulary: the last two columns are copied words
        text, mask, tgt, ln, fin = ops.force_inputs(idd if K > 1 else idd[:, 0], V, UNK, EOS, PAD, IGNORE)
        for rule in ("bar", "skip"):
            ref = fr.score_rows(s, ids, row_c, logits, rule)
            got = ops.force_score(sd, Idx(row_c.tolist()), tgt, ln, logits, UNK, rule)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(ln.cpu().numpy(), ref["len"])
            np.testing.assert_array_equal(fin.cpu().numpy(), ref["finished"])
            np.testing.assert_array_equal(got["n_scored"].cpu().numpy(), ref["n_scored"])
            np.testing.assert_array_equal(got["rank"].cpu().numpy(), ref["rank"])
            np.testing.assert_array_equal(got["top"].cpu().numpy(), ref["top"])
            for k in ("step", "top_step", "cum"):                      # bit for bit (−inf included)
                np.testing.assert_array_equal(got[k].cpu().numpy().view(np.int32), ref[k].astype(np.float32).view(np.int32), err_msg=k)
        # the model side: ids inside the text vocabulary up to the end, UNK for the others, PAD and mask 0 after it
        t_h, m_h = text.cpu().numpy(), mask.cpu().numpy()
        for r in range(R):
            n = int(ref["len"][r])
            want = [w if 0 <= w < V else UNK for w in ids[r, :n + 1]]
            assert t_h[r, :n + 1].tolist() == want and (t_h[r, n + 1:] == PAD).all()
            assert (m_h[r, :n + 1] == 1).all() and (m_h[r, n + 1:] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. the translator
def _cpu(batch):
    return {k: ([t.cpu() for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor) else
                (v.cpu() if isinstance(v, torch.Tensor) else v)) for k, v in batch.items()}


def _reference(cfg, model, batch, captions, rule="bar"):
    P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    c = _cpu(batch)
    return fr.forced_decode(P, cfg, c["input_ids_list"], c["video_features_list"], c["input_masks_list"], c["ingr_input_ids"],
                            c["ingr_sep_masks"], c["batch_step_num"], c["ingr_id_dict"], c["oov_word_dict"],
                            [x.cpu().numpy() for x in captions], rule)


def _translator(cfg, model, **kw):
    from svpc_amd.translator import Translator
    return Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, **kw)


def _sources(tr, batch):
    """the three caption sources: the fixture's gold labels (K = 1), the decoder's n-best rows and sampled rows (K = 4)"""
    gold = tr.gold_captions(batch["input_labels_list"], batch["batch_step_num"])
    nbest = tr.translate_batch_nbest(syn.translate_inputs(batch), 4, 4)
    sample = tr.translate_batch_sample(syn.translate_inputs(batch), num_samples=4, seed=SAMPLE_SEED)
    # PAD is a column like any other to the decoder, and a row that picks it goes on; to forced scoring a PAD ends the caption.  The
    # decodes' own scores and lengths can only be met on rows without such a pick, so the seed is one that has none
    for dec, _, _, ln in (nbest, sample):
        ids, n = torch.cat(list(dec)), torch.cat(list(ln)).unsqueeze(-1)
        pos = torch.arange(ids.shape[-1], device=ids.device).view(1, 1, -1)
        assert not bool(((ids == PAD) & (pos >= 1) & (pos <= n)).any()), "a decoded row picked PAD as a word: choose another seed"
    return dict(gold=(gold, None, None), nbest=(nbest[0], nbest[2], nbest[3]), sample=(sample[0], sample[2], sample[3]))


def _against(got, ref, what):
    """one call's namespace against the restatement's per-video dicts → (ranked positions, those under the gap)"""
    ranked = under = 0
    for b, r in enumerate(ref):
        cum, step = got.score_list[b].cpu().numpy(), got.step_list[b].cpu().numpy()
        shape = r["cum"].shape
        assert cum.shape == shape and got.score_list[b].dtype == torch.float32 and got.rank_list[b].dtype == torch.int32
        for k, v in (("cum", cum), ("step", step)):
            fin = np.isfinite(r[k])
            print("%s video %d: max |%s - ref| = %.3e" % (what, b, k, float(np.abs(v[fin].astype(np.float64) - r[k][fin]).max(initial=0.0))))
        np.testing.assert_allclose(cum, r["cum"], rtol=1e-4, atol=1e-6, err_msg=what)
        np.testing.assert_allclose(step, r["step"], rtol=1e-4, atol=1e-6, err_msg=what)
        np.testing.assert_allclose(got.top_step_list[b].cpu().numpy(), r["top_step"], rtol=1e-4, atol=1e-6, err_msg=what)
        np.testing.assert_array_equal(got.length_list[b].cpu().numpy(), r["len"])
        np.testing.assert_array_equal(got.finished_list[b].cpu().numpy(), r["finished"])
        np.testing.assert_array_equal(got.n_scored_list[b].cpu().numpy(), r["n_scored"])
        rank = got.rank_list[b].cpu().numpy()
        clear = ~(r["gap"] <= GAP)
        np.testing.assert_array_equal(rank[clear], r["rank"][clear], err_msg=what)
        np.testing.assert_array_equal(rank < 0, r["rank"] < 0)
        ranked += int((r["rank"] >= 0).sum())
        under += int(((r["rank"] >= 0) & ~clear).sum())
    return ranked, under


@pytest.mark.parametrize("incremental", [True, False])
@pytest.mark.parametrize("case,mt", [("tiny", "v"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")])
def test_translator_against_the_cpu_restatement(golden_dir, case, mt, incremental):
    z, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    src = _sources(_translator(cfg, model), batch)                     # (the decodes that make the captions are incremental)
    tr = _translator(cfg, model, incremental=incremental)
    ranked = under = 0
    for name, (dec, _, _) in src.items():
        got = tr.score_captions(syn.translate_inputs(batch), dec)
        a, b = _against(got, _reference(cfg, model, batch, dec), "%s %s %s" % (case, mt, name))
        ranked, under = ranked + a, under + b
    print("%s %s: %d of %d ranked positions under the gap" % (case, mt, under, ranked))
    assert ranked > 0 and under <= 0.05 * ranked


@pytest.mark.parametrize("case,mt", [("tiny", "v"), ("tiny", "vi"), ("tiny", "viv"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")])
def test_scores_of_the_decoder_s_own_rows(golden_dir, case, mt):
    """what the decodes report about their rows is what forced scoring says of them"""
    z, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    tr = _translator(cfg, model)
    src = _sources(tr, batch)
    for name in ("nbest", "sample"):
        dec, sc, ln = src[name]
        got = tr.score_captions(syn.translate_inputs(batch), dec)
        for b in range(len(dec)):
            np.testing.assert_allclose(got.score_list[b].cpu().numpy(), sc[b].cpu().numpy(), rtol=1e-4, atol=1e-6, err_msg=name)
            np.testing.assert_array_equal(got.length_list[b].cpu().numpy(), ln[b].cpu().numpy())
    greedy, _ = tr.translate_batch(syn.translate_inputs(batch))
    got = tr.score_captions(syn.translate_inputs(batch), greedy)
    for b, d in enumerate(greedy):
        assert tuple(got.score_list[b].shape) == (d.shape[0], 1)
        rank, step, top_step = (x[b][:, 0].cpu().numpy() for x in (got.rank_list, got.step_list, got.top_step_list))
        ids = d.cpu().numpy()
        for s in range(ids.shape[0]):
            hit = np.nonzero(ids[s, 1:] == EOS)[0]
            n = int(hit[0]) + 1 if len(hit) else ids.shape[1] - 1      # positions 1 … n: through the first EOS
            assert int(got.length_list[b][s, 0]) == n
            ok = (rank[s, :n] == 0) | (top_step[s, :n] - step[s, :n] <= 1e-4)
            assert ok.all(), (b, s, rank[s, :n], top_step[s, :n] - step[s, :n])


def _oov_batch(golden_dir):
    _, cfg, _, model = build_model("tiny", "vivt", golden_dir, DEV)
    return cfg, model, syn.make_batch(cfg, n_videos=3, max_steps=3, n_ingr=[3, 2, 3], n_oov=[2, 0, 3], seed=77, device=DEV)


def test_copied_words_and_skip(golden_dir):
    """extended ids ≥ V in the captions (columns of the copy distribution), a column past C_r and UNK as targets, both rules"""
    cfg, model, batch = _oov_batch(golden_dir)
    tr = _translator(cfg, model)
    gold = tr.gold_captions(batch["input_labels_list"], batch["batch_step_num"])
    V = cfg.vocab_size
    assert any(bool((g >= V).any()) for g in gold)
    gold[1][0, 2] = V                                                  # video 1 has no copied word: column V is past its C_r
    gold[0][1, 1] = UNK
    gold[2][0, 1] = V + 1                                              # a copied word of video 2
    for rule in ("bar", "skip"):
        got = tr.score_captions(syn.translate_inputs(batch), gold, unk=rule)
        ref = _reference(cfg, model, batch, gold, rule)
        _against(got, ref, "oov " + rule)
        cum = torch.cat([c.reshape(-1) for c in got.score_list]).cpu().numpy()
        assert np.isinf(cum).sum() == (2 if rule == "bar" else 0)
    assert int(got.rank_list[2][0, 0, 0]) >= 0


def test_deterministic_and_graph_replay(golden_dir):
    z, cfg, batch, model = build_model("c1", "vivt", golden_dir, DEV)
    eager, graphed = _translator(cfg, model), _translator(cfg, model, graph=True)
    a = eager.translate_batch_sample(syn.translate_inputs(batch), num_samples=3, seed=1)[0]
    b = eager.translate_batch_sample(syn.translate_inputs(batch), num_samples=3, seed=2)[0]
    assert not all(torch.equal(x, y) for x, y in zip(a, b))
    keys = ("cum", "length", "finished", "n_scored", "step", "rank", "top", "top_step")

    def bits(r):
        return [getattr(r, k).clone() for k in keys]
    ea, eb = bits(eager.score_captions(syn.translate_inputs(batch), a)), bits(eager.score_captions(syn.translate_inputs(batch), b))
    again = bits(eager.score_captions(syn.translate_inputs(batch), a))
    assert all(torch.equal(x, y) for x, y in zip(ea, again))           # the same input: the same bits
    assert not torch.equal(ea[0], eb[0])
    for dec, want in ((a, ea), (b, eb), (a, ea)):                      # capture with a, replay with b's captions, then a's again
        got = bits(graphed.score_captions(syn.translate_inputs(batch), dec))
        assert all(torch.equal(x, y) for x, y in zip(want, got))
    assert len(graphed._preps) == 1 and next(iter(graphed._preps.values())).graphs


def test_forced_scores_metric(golden_dir):
    from svpc_amd.metrics import ForcedScores
    cfg, model, batch = _oov_batch(golden_dir)
    tr = _translator(cfg, model)
    gold = tr.gold_captions(batch["input_labels_list"], batch["batch_step_num"])
    gold[0][1, 1] = UNK                                                # one caption at −inf
    sample = tr.translate_batch_sample(syn.translate_inputs(batch), num_samples=4, seed=3)[0]
    fs = ForcedScores(DEV)
    cum, ns, fin, rank = [], [], [], []
    for dec in (gold, sample):
        r = tr.score_captions(syn.translate_inputs(batch), dec)
        fs.update(r)
        cum.append(r.cum.cpu().numpy().reshape(-1).astype(np.float64)); ns.append(r.n_scored.cpu().numpy().reshape(-1))
        fin.append(r.finished.cpu().numpy().reshape(-1)); rank.append(r.rank.cpu().numpy().reshape(-1))
    cum, ns, fin, rank = (np.concatenate(x) for x in (cum, ns, fin, rank))
    res = fs.compute()
    ok, rk = np.isfinite(cum), rank[rank >= 0]
    assert res["captions"] == len(cum) and res["tokens"] == int(ns.sum()) and (~ok).sum() == 1
    assert abs(res["score_sum"] - cum[ok].sum()) <= 1e-9 * abs(cum[ok].sum())
    assert abs(res["ppl"] - np.exp(-cum[ok].sum() / ns[ok].sum())) <= 1e-9 * res["ppl"]
    assert res["inf_share"] == (~ok).sum() / len(cum) and res["finished_share"] == fin.sum() / len(cum)
    assert res["top1"] == (rk == 0).sum() / len(rk) and abs(res["mean_rank"] - rk.mean()) <= 1e-12 * rk.mean()
    fs.reset()
    assert fs.compute()["captions"] == 0


def test_consensus_with_forced_scores_as_posterior_weights(golden_dir):
    """candidates pooled from two decodes have no score of their own: ``score_captions`` gives them one, ``consensus`` takes it"""
    import consensus_reference as cr
    from test_consensus_gpu import SPECIAL, Case
    z, cfg, batch, model = build_model("c1", "vivt", golden_dir, DEV)
    Vm, N = cfg.vocab_size, len(batch["batch_step_num"])
    i2w = SPECIAL + ["".join(chr(97 + (i // 26 ** k) % 26) for k in range(3)) for i in range(7, Vm)]
    refs, videos = {}, []
    for b in range(N):
        inv = {int(v): k for k, v in batch["oov_word_dict"][b].items()}
        sents = []
        for s in range(int(batch["batch_step_num"][b])):
            lab = batch["input_labels_list"][s][b].cpu().tolist()
            sents.append(" ".join(i2w[x] if x < Vm else inv[x] for x in lab if x not in (IGNORE, EOS, PAD)))
        refs["vid%d" % b] = [" ".join(sents)]
        videos.append(dict(oov=batch["oov_word_dict"][b]))
    c = Case(i2w, refs)
    plan = c.plan(videos)
    tr = _translator(cfg, model)
    two = [tr.translate_batch_sample(syn.translate_inputs(batch), num_samples=2, seed=s)[0] for s in (7, 8)]
    pooled = [torch.cat([x, y], 1) for x, y in zip(*two)]              # (S_b, 4, Lt)
    scored = tr.score_captions(syn.translate_inputs(batch), pooled)
    got = tr.consensus(pooled, plan, scores=scored.score_list, scope="sentence", weights="posterior")
    rows = [d.cpu().tolist() for d in pooled]
    cands = [[[rows[b][s][k] for s in range(len(rows[b]))] for k in range(4)] for b in range(N)]
    ref = c.reference(videos, cands, "sentence", "CIDEr", [x.cpu().tolist() for x in scored.score_list])
    g = 0
    for b in range(N):
        for s in range(len(rows[b])):
            E, p = ref[g][1], int(got.pick_list[b][s])
            assert E[p] >= max(E) - cr.MARGIN * max(1.0, abs(max(E)))
            if not cr.under_margin(E):
                assert p == cr.pick_of(E)
            np.testing.assert_allclose(got.expected_list[b][s].cpu().numpy(), E, rtol=1e-9, atol=1e-12)
            g += 1


# ------------------------------------------------------------------------------------------------ 3. bf16x3
@pytest.mark.parametrize("mt", ["v", "vivt"])
def test_bf16x3_deviation_at_config_1(golden_dir, mt):
    """the same translator cases at the config-1 shape under the headline arithmetic: |cum − fp32 CPU restatement| ≤ BOUND_X3"""
    z, cfg, batch, model = build_model("c1", mt, golden_dir, DEV)
    src = _sources(_translator(cfg, model), batch)                     # the captions: made once, in fp32
    refs = {name: _reference(cfg, model, batch, dec) for name, (dec, _, _) in src.items()}
    ops.set_precision("bf16x3")
    try:
        _, _, _, model_x3 = build_model("c1", mt, golden_dir, DEV)    # (the same weights; its weight store gets the mode's lo plane)
        tr = _translator(cfg, model_x3)
        got = {name: [x.cpu().numpy() for x in tr.score_captions(syn.translate_inputs(batch), dec).score_list] for name, (dec, _, _) in src.items()}
        torch.cuda.synchronize()
    finally:
        ops.set_precision("fp32")
    worst = {}
    for name, ref in refs.items():
        dev = 0.0
        for g, r in zip(got[name], ref):
            fin = np.isfinite(r["cum"])
            np.testing.assert_array_equal(np.isfinite(g), fin)
            dev = max([dev] + np.abs(g[fin].astype(np.float64) - r["cum"][fin]).tolist())
        worst[name] = dev
    print("bf16x3 c1 %s: worst |cum - restatement| = %s" % (mt, json.dumps(worst)))
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "forced_score_parity_%s.json" % mt), "w") as f:
        json.dump(dict(case="c1", mt=mt, precision="bf16x3", worst_abs_cum_deviation=worst, bound=BOUND_X3), f, indent=1)
    assert max(worst.values()) <= BOUND_X3, worst
