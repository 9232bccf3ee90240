"""Truncated sampling on the MI355X (min-p, locally typical, epsilon and eta): the kernel (svpc_sample_step_trunc) against
tests/truncation_reference.py::trunc_select on the same fp32 tables, its draws against the truncated softmax, all stages off against
svpc_sample_step bit for bit, and Translator.translate_batch_sample with the four keywords end to end — against the CPU ``trunc_decode``
(fp32), eagerly and replayed, and through the callers that forward their keywords to it.  The tables, settings and (case, setting)
pairs live in the reference module; tests/test_truncation_host.py asserts on the reference alone what these tests rely on."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import sampling_reference as sr  # noqa: E402
import truncation_reference as trr  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import ops, synthetic as syn  # noqa: E402
from svpc_amd.ops_common import Idx  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, IGNORE, PAD, UNK  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = type("O", (), {"cuda": True})
SPECIAL = ["[PAD]", "[CLS]", "[SEP]", "[VID]", "[BOS]", "[EOS]", "[UNK]"]


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _run_kernel(tb, pos, Lt, logits, st, trunc, plain=False):
    s, row_c, row_x, cum, fin, length = tb
    n = s.shape[0]
    cum_d, fin_d, len_d = (torch.from_numpy(x.copy()).to(DEV) for x in (cum, fin, length))
    text = torch.full((n, Lt), -7, dtype=torch.int32, device=DEV)
    ext = torch.full((n, Lt), -7, dtype=torch.int32, device=DEV)
    seed_d = torch.tensor([st["seed"]], dtype=torch.int64, device=DEV)
    args = (torch.from_numpy(s).to(DEV), Idx(row_c.tolist()), Idx(row_x.tolist()), pos, logits, UNK, EOS, PAD, cum_d, fin_d, len_d, text,
            ext, seed_d)
    kw = dict(temp=st["t"], topk=st["k"], topp=st["q"], min_length=st["m"])
    if plain:
        nx_ext, nx_mod = ops.sample_step(*args, **kw)
        kept = torch.zeros(n, dtype=torch.int32, device=DEV)
    else:
        nx_ext, nx_mod, kept = ops.sample_step_trunc(*args, **kw, **trunc)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (nx_ext, nx_mod, cum_d, fin_d, len_d, text, ext, kept)]


def _check_step(out, ref, tb, pos):
    """every row equal to the reference (picks, model ids, cum bit for bit, finished, length, kept) unless its set, top-p or Gumbel
    margin is within KERNEL_TIE → the number of such rows that differ"""
    s, row_c, row_x, cum, fin, length = tb
    nx_ext, nx_mod, cum_d, fin_d, len_d, text, ext, kept = out
    picks, r_cum, r_fin, r_len, mg, r_kept, _ = ref
    r_mod = sr.model_ids(picks, fin.astype(bool), row_c, row_x)
    ok = (nx_ext == picks) & (nx_mod == r_mod) & (cum_d.view(np.int32) == r_cum.view(np.int32)) & (fin_d.astype(bool) == r_fin) \
        & (len_d == r_len) & (kept == r_kept)
    near = trr.flagged_rows(ref, fin)
    bad = np.nonzero(~ok)[0]
    for i in bad:
        assert near[i], ("row %d differs without a near-tie" % i, int(nx_ext[i]), int(picks[i]), int(kept[i]), int(r_kept[i]), mg[i].tolist())
    assert np.all(kept[fin.astype(bool)] == 0)
    np.testing.assert_array_equal(text[:, pos + 1], nx_mod)
    np.testing.assert_array_equal(ext[:, pos + 1], nx_ext)
    keep = np.ones(text.shape[1], bool)
    keep[pos + 1] = False
    assert np.all(text[:, keep] == -7) and np.all(ext[:, keep] == -7)
    return int(near.sum())


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_sample_step_trunc_equals_trunc_select(R, logits):
    counted = rows = 0
    for tb, st, trunc, ref in trr.kernel_cases(R, logits):
        out = _run_kernel(tb, trr.KERNEL_POS, trr.KERNEL_LT, logits, st, trunc)
        counted += _check_step(out, ref, tb, trr.KERNEL_POS)
        rows += tb[0].shape[0]
    print("R = %d, logits = %s: %d of %d rows within %g of a cut or a Gumbel tie" % (R, logits, counted, rows, trr.KERNEL_TIE))
    assert counted <= rows // 200, (counted, rows)


def test_sample_step_trunc_wide_rows():
    """rows of 1,025 … 4,096 columns (the wide kernel variant), both score modes: no row may differ"""
    for logits, tb, st, trunc, ref in trr.wide_cases():
        out = _run_kernel(tb, 3, 8, logits, st, trunc)
        assert _check_step(out, ref, tb, 3) == 0
        ok = (out[0] == ref[0]) & (out[7] == ref[5]) & (out[2].view(np.int32) == ref[1].view(np.int32))
        assert ok.all(), (trunc, np.nonzero(~ok)[0].tolist())


@pytest.mark.parametrize("logits", [False, True])
def test_all_stages_off_is_sample_step(logits):
    """svpc_sample_step_trunc with the four stages off ≡ svpc_sample_step bit for bit, on the kernel tables and on wide rows"""
    rng = np.random.default_rng(77 + logits)
    for R, cmax_hi in ((3, 700), (2, 4097)):
        for adversarial in (False, True):
            tb = trr.tables(rng, 29 if cmax_hi == 700 else 6, R, logits, adversarial, cmax_hi=cmax_hi)
            for k, q, t in trr.BASE + [(0, 0.0, 0.7)]:
                st = dict(k=k, q=q, t=t, m=0, seed=int(rng.integers(0, 1 << 63)))
                a = _run_kernel(tb, 4, 9, logits, st, trr.OFF)
                b = _run_kernel(tb, 4, 9, logits, st, None, plain=True)
                for x, y in zip(a[:7], b[:7]):
                    np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32))
                live = ~tb[4].astype(bool) & np.isfinite(a[2])        # (a live row without candidates ends with cum −inf)
                assert np.all(a[7][~live] == 0) and np.all(a[7][live] >= 1)


RULES = [dict(min_p=0.07), dict(typical_p=0.9), dict(typical_p=0.37), dict(epsilon_cutoff=0.04), dict(eta_cutoff=0.04),
         dict(min_p=0.07, typical_p=0.9, epsilon_cutoff=3e-3, eta_cutoff=3e-3)]


@pytest.mark.parametrize("trunc", RULES, ids=[",".join("%s=%s" % i for i in d.items()) for d in RULES])
def test_sample_step_trunc_distribution(trunc):
    """one row of 40 columns repeated over 24,576 rows of one launch, every row drawing with its own counter: no draw outside the kept
    set, the counts against the truncated softmax, kept the same in every row"""
    rng = np.random.default_rng(23)
    C, n = 40, 24576
    row = rng.dirichlet(np.ones(C) * 0.6).astype(np.float32)
    row[UNK] = 0.2
    tb = (np.tile(row, (n, 1)), np.full(n, C), np.zeros(n, np.int64), np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32))
    out = _run_kernel(tb, 2, 6, False, dict(k=0, q=0.0, t=1.3, m=0, seed=977), trunc)
    target = trr.target_distribution(row, C, False, 2, temp=1.3, **trunc)
    counts = np.bincount(out[0], minlength=C)
    assert counts[target == 0].sum() == 0, "a draw outside the kept set"
    assert np.all(out[7] == int((target > 0).sum()))
    stat, dof = sr.chi_square(counts, target)
    assert dof >= 2 and stat < sr.chi_square_bound(dof), (stat, dof)


# ------------------------------------------------------------------------------------------------ 2. the translator
def _cpu(batch):
    return {k: ([t.cpu() for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor) else
                (v.cpu() if isinstance(v, torch.Tensor) else v)) for k, v in batch.items()}


def _ref(cfg, model, batch, R, seed, **kw):
    P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    c = _cpu(batch)
    return trr.trunc_decode(P, cfg, c["input_ids_list"], c["video_features_list"], c["input_masks_list"], c["ingr_input_ids"],
                            c["ingr_sep_masks"], c["batch_step_num"], c["ingr_id_dict"], c["oov_word_dict"], R, seed, **kw)


def _well_formed(dec, cums, lens, batch, R, Lt):
    assert len(dec) == len(batch["batch_step_num"])
    for d, c, ln, S_b in zip(dec, cums, lens, batch["batch_step_num"]):
        assert d.dtype == torch.int64 and c.dtype == torch.float32 and ln.dtype == torch.int64
        assert tuple(d.shape) == (S_b, R, Lt) and tuple(c.shape) == (S_b, R) and tuple(ln.shape) == (S_b, R)
        d, ln = d.cpu(), ln.cpu()
        for s_ in range(S_b):
            for j in range(R):
                y, L = d[s_, j].tolist(), int(ln[s_, j])
                assert y[0] == BOS and 1 <= L <= Lt - 1
                assert EOS not in y[1:L] and all(v == PAD for v in y[L + 1:]), (y, L)
                assert y[L] == EOS or L == Lt - 1 or y[L] == PAD, (y, L)
                assert UNK not in y[1:L + 1], y


def _translator(cfg, model, **kw):
    from svpc_amd.translator import Translator
    return Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, **kw)


@pytest.mark.parametrize("case,mt,trunc", trr.DECODE_PAIRS, ids=["%s-%s-%s" % (c, m, ",".join("%s=%s" % i for i in k.items()))
                                                                  for c, m, k in trr.DECODE_PAIRS])
def test_truncated_samples_against_the_cpu_reference(golden_dir, case, mt, trunc):
    """ids and lengths equal ``trunc_decode``'s and cum is within rtol 1e-4 — except samples with an undecided step (the pick margin at
    δ = 1e-4, or a Gumbel / top-p gap within 1e-4), which are counted"""
    _, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    R, seed = trr.DECODE_R, trr.DECODE_SEED
    tr = _translator(cfg, model)
    dec, _, cums, lens = tr.translate_batch_sample(syn.translate_inputs(batch), R, seed=seed, **trunc)
    assert int(tr.last_sample_seed) == seed
    _well_formed(dec, cums, lens, batch, R, cfg.max_t_len)
    r_ids, r_cum, r_len, r_mg, r_und, r_kept = _ref(cfg, model, batch, R, seed, delta=trr.DECODE_DELTA, **trunc)
    kept = tr.last_sample_kept.cpu().numpy().T.reshape(-1, R, cfg.max_t_len - 1)          # (T, R, Lt − 1)
    counted = total = t0 = 0
    for d, c, ln, ri, rc, rl, rm, ru, rk in zip(dec, cums, lens, r_ids, r_cum, r_len, r_mg, r_und, r_kept):
        d, c, ln = d.cpu(), c.cpu().numpy(), ln.cpu().numpy()
        for s_ in range(d.shape[0]):
            for j in range(d.shape[1]):
                total += 1
                if torch.equal(d[s_, j], ri[s_, j]):
                    np.testing.assert_allclose(c[s_, j], rc[s_, j], rtol=1e-4, atol=1e-6)
                    assert ln[s_, j] == rl[s_, j]
                    continue
                assert ru[s_, j] > 0 or rm[s_, j] <= trr.DECODE_DELTA, ("ids differ on a decided sample", d[s_, j].tolist(), ri[s_, j].tolist())
                counted += 1
        t0 += d.shape[0]
    assert kept.shape[0] == t0 and kept.min() >= 0 and kept.max() <= max(cfg.vocab_size + len(o) for o in batch["oov_word_dict"])
    print("%s %s %s: %d of %d samples undecided and different" % (case, mt, trunc, counted, total))
    assert counted <= max(1, total // 20), (counted, total)


@pytest.mark.parametrize("case,mt,trunc", trr.MEMBER_PAIRS, ids=["%s-%s-%d" % (c, m, len(k)) for c, m, k in trr.MEMBER_PAIRS])
def test_truncated_samples_lie_in_the_loosened_set(golden_dir, case, mt, trunc):
    """typical sampling on c1 vivt leaves too many undecided steps for an id comparison: every drawn word, replayed along the GPU's own
    prefix through the oracle, must lie in the loosened set (δ = 1e-3)"""
    _, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    R, seed = trr.DECODE_R, trr.DECODE_SEED
    tr = _translator(cfg, model)
    dec, _, cums, lens = tr.translate_batch_sample(syn.translate_inputs(batch), R, seed=seed, **trunc)
    _well_formed(dec, cums, lens, batch, R, cfg.max_t_len)
    ref = _ref(cfg, model, batch, R, seed, delta=trr.MEMBER_DELTA, forced=[d.cpu() for d in dec], **trunc)
    outside = sum(int(u.sum()) for u in ref[4])
    assert outside == 0, outside
    for d, c, ri, rc in zip(dec, cums, ref[0], ref[1]):             # the replay followed the GPU's ids, so its cum is the GPU's
        assert torch.equal(d.cpu(), ri)
        np.testing.assert_allclose(c.cpu().numpy(), rc, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("case,mt", [("tiny", "vivt"), ("c1", "v")])
def test_truncated_eager_and_replayed(golden_dir, case, mt):
    """eager ≡ graph-replayed bit for bit under a fixed seed; a second setting gets a second plan; everything off is the plain decode"""
    _, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    kw = dict(random_sampling_temp=1.5, random_sampling_topp=0.95, typical_p=0.9, eta_cutoff=3e-3)
    eager, graphed = _translator(cfg, model), _translator(cfg, model, graph=True)
    e = eager.translate_batch_sample(syn.translate_inputs(batch), 4, seed=99, **kw)
    ek = eager.last_sample_kept.clone()
    for it in range(3):                                  # capture, then replay
        g = graphed.translate_batch_sample(syn.translate_inputs(batch), 4, seed=99, **kw)
        for k in (0, 2, 3):
            for a, b in zip(e[k], g[k]):
                assert torch.equal(a, b)
        assert torch.equal(graphed.last_sample_kept, ek)
    assert len(graphed._preps) == 1 and next(iter(graphed._preps.values())).graphs
    graphed.translate_batch_sample(syn.translate_inputs(batch), 4, seed=99, **dict(kw, typical_p=0.37))
    assert len(graphed._preps) == 2
    # everything off: the plain decode's plan, launches and ids
    plain = eager.translate_batch_sample(syn.translate_inputs(batch), 4, seed=99, random_sampling_temp=1.5, random_sampling_topp=0.95)
    n = len(eager._preps)
    off = eager.translate_batch_sample(syn.translate_inputs(batch), 4, seed=99, random_sampling_temp=1.5, random_sampling_topp=0.95,
                                       min_p=0.0, typical_p=1.0, epsilon_cutoff=0, eta_cutoff=0.0)
    assert len(eager._preps) == n and eager.last_sample_kept is None
    for k in (0, 2, 3):
        for a, b in zip(plain[k], off[k]):
            assert torch.equal(a, b)
    assert any(not torch.equal(a, b) for a, b in zip(plain[0], e[0])), "truncation changed nothing"


def test_truncation_through_consensus_and_self_critical(golden_dir):
    """the callers that forward their keywords to the sampler take the new ones: finite outputs on tiny vivt"""
    from svpc_amd import scst
    from svpc_amd.caption_scores import ReferenceCorpus
    _, cfg, batch, model = build_model("tiny", "vivt", golden_dir, DEV)
    Vm = cfg.vocab_size
    i2w = SPECIAL + ["".join(chr(97 + (i // 26 ** k) % 26) for k in range(3)) for i in range(7, Vm)]
    refs, videos = {}, []
    for b in range(len(batch["batch_step_num"])):
        inv = {int(v): k for k, v in batch["oov_word_dict"][b].items()}
        sents = []
        for s in range(int(batch["batch_step_num"][b])):
            lab = batch["input_labels_list"][s][b].cpu().tolist()
            sents.append(" ".join(i2w[x] if x < Vm else inv[x] for x in lab if x not in (IGNORE, EOS, PAD)))
        refs["vid%d" % b] = [" ".join(sents)]
        videos.append(dict(key="vid%d" % b, oov_word_dict=batch["oov_word_dict"][b]))
    corpus = ReferenceCorpus(i2w, refs, device=DEV)
    tr = _translator(cfg, model)
    plan = corpus.plan([dict(oov_word_dict=v["oov_word_dict"]) for v in videos], references=False)
    got, oov, picks = tr.translate_batch_consensus(syn.translate_inputs(batch), plan, source="sample", num_candidates=3, seed=17,
                                                   typical_p=0.9)
    assert tr.last_sample_kept is not None and int(tr.last_sample_kept.max()) >= 1
    for b, S_b in enumerate(batch["batch_step_num"]):
        assert tuple(got[b].shape) == (S_b, cfg.max_t_len) and int(picks[b].min()) >= 0 and int(picks[b].max()) < 3
    r = scst.SelfCritical(tr, corpus).step(syn.translate_inputs(batch), videos, num_samples=3, seed=17, eta_cutoff=3e-3)
    assert torch.isfinite(r.loss).all() and torch.isfinite(r.reward).all() and torch.isfinite(r.cum).all()
    with pytest.raises(TypeError):
        tr.translate_batch_stochastic(syn.translate_inputs(batch), 2, typical_p=0.9)
