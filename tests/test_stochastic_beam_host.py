"""Stochastic beam search without a GPU: the argument checks of Translator.translate_batch_stochastic / ops.check_stochastic_beam /
ops.stochastic_beam_step, the exported symbol, and tests/stochastic_beam_reference.py alone — the facts that follow from the definition,
dead rows, fewer than W candidates, a two-row anchor worked by hand, the without-replacement law of its draws on a hand-built tree, and
the margins of every fixed input the GPU tests use."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import sampling_reference as sr  # noqa: E402
import stochastic_beam_cases as sbc  # noqa: E402
import stochastic_beam_reference as sbr  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import _lib, ops, synthetic as syn  # noqa: E402
from svpc_amd.synthetic import EOS, PAD, UNK  # noqa: E402

O = type("O", (), {"cuda": False})


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.fixture(scope="module")
def tiny(golden_dir):
    _, cfg, batch, model = build_model("tiny", "vivt", golden_dir, "cpu")
    return cfg, batch, model


def _tr(tiny, **kw):
    from svpc_amd.translator import Translator
    cfg, _, model = tiny
    return Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, **kw)


BAD = [
    dict(beam_size=0), dict(beam_size=9), dict(beam_size=2.0), dict(beam_size=True),
    dict(random_sampling_temp=0.0), dict(random_sampling_temp=-1.0), dict(random_sampling_temp=float("inf")),
    dict(random_sampling_temp=float("nan")), dict(random_sampling_temp="hot"),
    dict(min_length=-1), dict(min_length=6), dict(min_length=1.0),
    dict(seed=-1), dict(seed=1 << 63), dict(seed=1.5), dict(seed="7"), dict(seed=True),
]


@pytest.mark.parametrize("kw", BAD, ids=[",".join("%s=%r" % i for i in d.items()) for d in BAD])
def test_bad_arguments_raise_value_error(tiny, kw):
    cfg, batch, _ = tiny
    assert cfg.max_t_len == 6
    with pytest.raises(ValueError):
        _tr(tiny).translate_batch_stochastic(syn.translate_inputs(batch), **kw)


def test_bad_opt_attribute_raises_value_error(tiny):
    tr = _tr(tiny)
    tr.opt.random_sampling_temp = -2.0
    with pytest.raises(ValueError):
        tr.translate_batch_stochastic(syn.translate_inputs(tiny[1]), 2)
    tr.opt.random_sampling_temp = 1.0
    tr.opt.beam_size = 11
    with pytest.raises(ValueError):
        tr.translate_batch_stochastic(syn.translate_inputs(tiny[1]))


def test_rows_wider_than_4096_columns_raise_value_error(tiny):
    cfg, batch, _ = tiny
    inputs = list(syn.translate_inputs(batch))
    inputs[8] = [dict(d) for d in inputs[8]]
    inputs[8][0] = {"w%d" % i: cfg.vocab_size + i for i in range(4097 - cfg.vocab_size)}      # C = V + X = 4097
    with pytest.raises(ValueError, match="4096"):
        _tr(tiny).translate_batch_stochastic(inputs, 2)


@pytest.mark.parametrize("kw", [dict(random_sampling_topk=5), dict(random_sampling_topp=0.9), dict(block_ngram_repeat=2),
                                dict(length_penalty_name="avg"), dict(n_best=2), dict(num_samples=2), dict(random_sampling_tmp=0.5)])
def test_any_other_keyword_raises_type_error(tiny, kw):
    with pytest.raises(TypeError):
        _tr(tiny).translate_batch_stochastic(syn.translate_inputs(tiny[1]), 2, **kw)


def test_non_incremental_raises_not_implemented(tiny):
    with pytest.raises(NotImplementedError):
        _tr(tiny, incremental=False).translate_batch_stochastic(syn.translate_inputs(tiny[1]), 2, seed=3)


def test_no_cpu_fallback(tiny):
    with pytest.raises(_lib.SvpcKernelError):
        _tr(tiny).translate_batch_stochastic(syn.translate_inputs(tiny[1]), 2, seed=3)
    R, C, Lt = 4, 12, 6
    toks = [[torch.zeros(R, Lt, dtype=torch.int32) for _ in range(3)] for _ in range(2)]
    with pytest.raises(_lib.SvpcKernelError):
        ops.stochastic_beam_step(torch.rand(R, C), [C] * R, [0] * R, 2, 0, False, UNK, EOS, PAD, torch.zeros(R), torch.zeros(R, dtype=torch.float64),
                                 torch.zeros(R, dtype=torch.float64), torch.zeros(R, dtype=torch.int32), torch.zeros(R, dtype=torch.int32),
                                 toks[0], toks[1], Lt, torch.zeros(1, dtype=torch.int64))


def test_consensus_names_the_new_source(tiny):
    with pytest.raises(ValueError, match="stochastic"):
        _tr(tiny).translate_batch_consensus(syn.translate_inputs(tiny[1]), None, source="nope")


def test_check_stochastic_beam_normalises():
    c = ops.check_stochastic_beam(22, 4, np.int64(5), 4096, 0.7, 4)
    assert c == dict(beam_size=4, random_sampling_temp=0.7, min_length=4, seed=5)
    assert ops.check_stochastic_beam(22, 1)["seed"] is None
    assert ops.check_stochastic_beam(22, 8, seed=(1 << 63) - 1)["seed"] == (1 << 63) - 1
    for bad in (dict(beam_size=0), dict(beam_size=9), dict(beam_size=3, random_sampling_temp=float("nan")), dict(beam_size=3, min_length=22),
                dict(beam_size=3, seed=1 << 63), dict(beam_size=3, max_cols=4097)):
        with pytest.raises(ValueError):
            ops.check_stochastic_beam(22, **bad)


def test_opt_attributes_are_read_and_the_setting_is_part_of_the_plan_key(tiny, monkeypatch):
    seen = []
    tr = _tr(tiny)
    tr.opt.random_sampling_temp = 0.25
    tr.opt.min_length = 2
    tr.opt.beam_size = 3
    tr.opt.seed = 2019                            # (the reference's training seed: not read)
    monkeypatch.setattr(tr, "_translate", lambda *a, **kw: seen.append(kw["decode"]))
    tr.translate_batch_stochastic(syn.translate_inputs(tiny[1]))
    tr.translate_batch_stochastic(syn.translate_inputs(tiny[1]), 4, seed=7, random_sampling_temp=2.0, min_length=0)
    a, b = seen
    assert (a.kind, a.width, a.stochastic, a.seed, a.n_best) == ("beam", 3, (0.25, 2), None, 3)
    assert (b.kind, b.width, b.stochastic, b.seed, b.n_best) == ("beam", 4, (2.0, 0), 7, 4)
    assert a.key != b.key and not a.ranked and ("stochastic", 0.25, 2) in a.key
    from svpc_amd.translator import BEAM, Decode
    assert Decode(BEAM, 3).key != a.key and Decode(BEAM, 3, n_best=3).key != a.key


def test_symbol_is_declared_and_exported():
    ret, args = _lib.declarations()["svpc_beam_step_gumbel"]
    assert ret is ctypes.c_int and len(args) == 32 and args.count(ctypes.c_double) == 1
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "svpc_beam_step_gumbel")
    assert _lib.load().svpc_abi_version() == 2


# ------------------------------------------------------------------------------------------------ the reference alone
def _drive(W, T, C, steps, logits, seed, temp=1.0, min_length=0, rng=None, detail=None):
    """``steps`` selection steps over fresh random score rows → (ids (T·W, steps + 1), final state, per-step (before, after) states)"""
    rng = rng or np.random.default_rng(seed)
    cum, phi, G, fin, ln = sbr.initial_state(T, W)
    ids = np.full((T * W, steps + 1), PAD, np.int64)
    ids[:, 0] = syn.BOS
    trail = []
    for i in range(steps):
        s = (rng.standard_normal((T * W, C)) * 2).astype(np.float32) if logits else rng.dirichlet(np.ones(C) * 0.3, size=T * W).astype(np.float32)
        o = sbr.stochastic_beam_select(s, [C] * (T * W), [0] * (T * W), W, i, logits, cum, phi, G, fin, ln, seed, temp, min_length,
                                       detail=detail)
        trail.append((G.copy(), fin.copy(), o))
        ids = ids[o["parent"]].copy()
        ids[:, i + 1] = o["ext"]
        cum, phi, G, fin, ln = o["cum"], o["phi"], o["G"], o["finished"], o["length"]
    return ids, (cum, phi, G, fin, ln), trail


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("W", [1, 2, 3, 5, 8])
def test_facts_that_follow_from_the_definition(W, logits):
    T, C, steps = 6, 14, 5
    detail = []
    ids, (cum, phi, G, fin, ln), trail = _drive(W, T, C, steps, logits, 77 + W, temp=0.8, min_length=2, detail=detail)
    for t in range(T):
        rows = [tuple(ids[t * W + h]) for h in range(W) if G[t * W + h] > -np.inf]
        assert len(set(rows)) == len(rows) >= 1                 # the finite-G rows are pairwise different captions
        assert not any(EOS in r[1:3] for r in rows)             # the min length bars EOS at positions 1 and 2
    for G_before, _, o in trail:
        assert np.all(o["G"] <= G_before[o["parent"]])          # G never increases from parent to child …
        Gs = o["G"].reshape(T, W)
        assert np.all(Gs[:, 1:] <= Gs[:, :-1])                  # … nor from row j to row j + 1 (dead rows, −inf, last)
        live = o["G"] > -np.inf
        assert np.all(o["phi"][live] <= 1e-12) and np.all(np.isinf(o["cum"][~live])) and np.all(o["finished"][~live])
    assert detail
    for r, cols, g, gt in detail:                               # exp(−G̃) − exp(−g) is the same for all short-listed children
        d = np.exp(-gt) - np.exp(-g)
        assert np.allclose(d, d[0], rtol=1e-9, atol=1e-9 * np.exp(-g).max()), (r, d)
        assert np.all(np.diff(gt) <= 0) and np.all(np.diff(g) <= 0)       # G̃ is non-decreasing in g within a row
    r, cols, g, gt = detail[0]
    assert gt[0] == 0.0                                          # the arg-max child carries its parent's G exactly (row 0 starts at 0)


def test_width_one_is_the_sampling_reference():
    rng = np.random.default_rng(8)
    T, C = 40, 30
    for logits in (False, True):
        s = (rng.standard_normal((T, C)) * 2).astype(np.float32) if logits else rng.dirichlet(np.ones(C) * 0.4, size=T).astype(np.float32)
        cum, phi, G, fin, ln = sbr.initial_state(T, 1)
        o = sbr.stochastic_beam_select(s, [C] * T, [0] * T, 1, 3, logits, cum, phi, G, fin, ln, 4242, 0.7, 0)
        picks, s_cum, s_fin, s_len, _ = sr.sample_select(s, [C] * T, [0] * T, 3, logits, cum, fin, ln, 4242, temp=0.7)
        np.testing.assert_array_equal(o["ext"], picks)
        np.testing.assert_array_equal(o["cum"].view(np.int32), s_cum.view(np.int32))
        np.testing.assert_array_equal(o["finished"], s_fin)
        np.testing.assert_array_equal(o["length"], s_len)


def test_dead_rows_and_fewer_than_w_candidates():
    W, C = 4, 9
    s = np.zeros((W, C), np.float32)
    s[:, UNK] = 0.9
    s[0, 7], s[0, 8] = 0.6, 0.4                     # the first step: row 0 alone offers two candidates for four slots
    cum, phi, G, fin, ln = sbr.initial_state(1, W)
    o = sbr.stochastic_beam_select(s, [C] * W, [0] * W, W, 0, False, cum, phi, G, fin, ln, 5)
    assert sorted(o["ext"][:2].tolist()) == [7, 8] and o["ext"][2:].tolist() == [PAD, PAD]
    assert o["parent"].tolist() == [0, 0, 2, 3] and o["finished"].tolist() == [False, False, True, True]
    assert np.all(np.isinf(o["G"][2:])) and np.all(np.isinf(o["phi"][2:])) and np.all(np.isinf(o["cum"][2:])) and o["length"].tolist() == [1] * 4
    assert o["G"][0] == 0.0 and o["G"][1] < 0.0
    np.testing.assert_allclose(np.exp(o["phi"][:2]).sum(), 1.0, rtol=1e-12)
    # the next step: row 0 has no candidate (an empty K0), row 1 only EOS, rows 2 and 3 are dead and offer nothing
    s2 = np.zeros((W, C), np.float32)
    s2[:, UNK] = 0.9
    s2[1, EOS] = 1.0
    s2[2:, 7] = 1.0
    o2 = sbr.stochastic_beam_select(s2, [C] * W, [0] * W, W, 1, False, o["cum"], o["phi"], o["G"], o["finished"], o["length"], 5)
    assert o2["ext"].tolist() == [EOS, PAD, PAD, PAD] and o2["parent"].tolist() == [1, 1, 2, 3]
    assert o2["G"][0] == o["G"][1] and o2["phi"][0] == o["phi"][1] and o2["cum"][0] == o["cum"][1]       # step score log 1 = 0
    assert o2["finished"].all() and np.all(np.isinf(o2["G"][1:]))
    # … and with the min length barring EOS nothing is left at all
    o3 = sbr.stochastic_beam_select(s2, [C] * W, [0] * W, W, 1, False, o["cum"], o["phi"], o["G"], o["finished"], o["length"], 5, min_length=2)
    assert np.all(np.isinf(o3["G"])) and o3["ext"].tolist() == [PAD] * 4 and o3["parent"].tolist() == [0, 1, 2, 3]
    # a finished row with finite G carries itself, whatever its score row holds
    o4 = sbr.stochastic_beam_select(s2, [C] * W, [0] * W, W, 2, False, o2["cum"], o2["phi"], o2["G"], o2["finished"], o2["length"], 5)
    assert o4["ext"].tolist() == [PAD] * 4 and o4["G"][0] == o2["G"][0] and o4["length"][0] == 2 and o4["length"][1:].tolist() == [3, 3, 3]


def test_two_row_anchor_worked_by_hand():
    """W = 2, τ = 1, position p = 3: row 0 live (cum −1, phi −1, G −0.5) over p(EOS) = p(8) = 0.25, p(7) = 0.5; row 1 finished with
    G = −0.7.  Every number below is formed here with ``math`` and the hash alone."""
    C, seed, pos = 9, 31337, 2
    s = np.zeros((2, C), np.float32)
    s[0, EOS], s[0, UNK], s[0, 7], s[0, 8] = 0.25, 0.9, 0.5, 0.25
    s[1, 7] = 1.0                                  # (a finished row's scores are not read)
    cum = np.array([-1.0, -2.0], np.float32)
    phi, G = np.array([-1.0, -1.5]), np.array([-0.5, -0.7])
    o = sbr.stochastic_beam_select(s, [C, C], [0, 0], 2, pos, False, cum, phi, G, np.array([False, True]), np.array([2, 2]), seed)
    step = {c: float(np.float32(math.log(p))) for c, p in ((EOS, 0.25), (7, 0.5), (8, 0.25))}     # fp64 log, rounded once to fp32; z = s / 1
    m = max(step.values())
    L = m + math.log(sum(math.exp(z - m) for z in step.values()))                                  # ≈ 0: the three sum to one
    assert abs(L) < 1e-7
    g, phi_c = {}, {}
    for c, z in step.items():
        u = (sr.hash32(seed, pos, 0 * 4096 + c) + 0.5) / 4294967296.0
        phi_c[c] = -1.0 + (z - L)
        g[c] = phi_c[c] - math.log(-math.log(u))
    first, second = sorted(g, key=lambda c: -g[c])[:2]
    v = -0.5 - g[second] + math.log1p(-math.exp(g[second] - g[first]))
    gt_second = -0.5 - max(v, 0.0) - math.log1p(math.exp(-abs(v)))
    cands = sorted([(-0.5, g[first], first, 0), (gt_second, g[second], second, 0), (-0.7, -0.7, PAD, 1)], key=lambda c: (-c[0], -c[1]))[:2]
    assert cands[0][2] == first and o["G"][0] == -0.5            # the arg-max child carries G_h exactly
    for k, (gt, _, col, h) in enumerate(cands):
        assert o["ext"][k] == col and o["parent"][k] == h
        assert abs(o["G"][k] - gt) < 1e-12
        if h == 0:
            assert abs(o["phi"][k] - phi_c[col]) < 1e-12 and abs(o["phi"][k] - (-1.0 + math.log(float(s[0, col])))) < 1e-7
            assert o["cum"][k] == np.float32(np.float32(-1.0) + np.float32(step[col])) and o["length"][k] == 3
            assert o["finished"][k] == (col == EOS)
        else:
            assert o["phi"][k] == -1.5 and o["cum"][k] == np.float32(-2.0) and o["length"][k] == 2 and o["finished"][k]
    assert gt_second < -0.5 and o["G"][1] <= o["G"][0]


def test_draws_are_without_replacement_on_a_hand_built_tree():
    """A two-pick tree over the words a = 7, b = 8 and EOS with fixed probability rows, W = 2, driven through ``stochastic_beam_select``
    over 2,000 consecutive seeds: the ordered pair (row 0, row 1) against P(x)·P(y) / (1 − P(x)) over whole sequences (every cell
    expects ≥ 5), and row 0 alone against P — both under the project's 1e-5 chi-square tail."""
    C, a, b, N = 9, 7, 8, 2000
    first = {a: 0.4, b: 0.35, EOS: 0.25}
    second = {a: {a: 0.3, b: 0.3, EOS: 0.4}, b: {a: 0.35, b: 0.25, EOS: 0.4}}
    seqs = {(EOS, PAD): first[EOS]}
    for x in (a, b):
        for y in (a, b, EOS):
            seqs[(x, y)] = first[x] * second[x][y]
    names = sorted(seqs)
    P = np.array([seqs[k] for k in names])
    assert abs(P.sum() - 1.0) < 1e-12
    pair_p = np.array([[P[i] * P[j] / (1.0 - P[i]) if i != j else 0.0 for j in range(len(P))] for i in range(len(P))])
    assert abs(pair_p.sum() - 1.0) < 1e-12 and N * pair_p[pair_p > 0].min() >= 5

    def row(d):
        r = np.zeros(C, np.float32)
        r[UNK] = 0.7
        for c, p in d.items():
            r[c] = p
        return r
    pairs = np.zeros((len(P), len(P)))
    for seed in range(N):
        cum, phi, G, fin, ln = sbr.initial_state(1, 2)
        s = np.stack([row(first), row(first)])
        o = sbr.stochastic_beam_select(s, [C, C], [0, 0], 2, 0, False, cum, phi, G, fin, ln, seed)
        w1 = o["ext"].copy()
        s = np.stack([row(second.get(int(w), first)) for w in w1])
        o2 = sbr.stochastic_beam_select(s, [C, C], [0, 0], 2, 1, False, o["cum"], o["phi"], o["G"], o["finished"], o["length"], seed)
        got = [(int(w1[p]), int(e)) for p, e in zip(o2["parent"], o2["ext"])]
        assert np.all(np.isfinite(o2["G"])) and got[0] != got[1]
        for k in (0, 1):                           # phi is the log-probability of the row's whole sequence
            assert abs(o2["phi"][k] - math.log(seqs[got[k]])) < 1e-6
        pairs[names.index(got[0]), names.index(got[1])] += 1
    stat, dof = sr.chi_square(pairs.reshape(-1), pair_p.reshape(-1))
    assert dof == len(P) * (len(P) - 1) - 1 and stat < sr.chi_square_bound(dof), (stat, dof)
    stat, dof = sr.chi_square(pairs.sum(1), P)
    assert dof == len(P) - 1 and stat < sr.chi_square_bound(dof), (stat, dof)


# ------------------------------------------------------------------------------------------------ the margins of the GPU tests' inputs
@pytest.mark.parametrize("W", sbc.WIDTHS)
def test_kernel_cases_have_margins_above_the_noise(W):
    seen = 0
    for key in sbc.case_list():
        if key[0] != W:
            continue
        m = sbc.reference(*key)["margin"]
        assert m.min() >= sbc.MARGIN, (key, float(m.min()))
        seen += 1
    assert seen == 2 * len(sbc.COLS)


def test_case_list_covers_every_value():
    cl = sbc.case_list()
    assert {k[0] for k in cl} == set(sbc.WIDTHS) and {k[2] for k in cl} == set(sbc.COLS) and {k[3] for k in cl} == set(sbc.TEMPS)
    assert {k[4] for k in cl} == set(sbc.SENTENCES) and {bool(k[5]) for k in cl} == {False, True} and {k[1] for k in cl} == {False, True}
    assert (8, True, 4096, sbc.TEMPS[(5 + 5) % 3], 257, sbc.POS + 2 if (5 + 1) % 2 else 0) in cl
    c = sbc.make_case(8, False, 7, *[k for k in cl if k[0] == 8 and not k[1] and k[2] == 7][0][3:])
    assert c["scores"].shape[1] == 10 and not c["finished"][0] and c["finished"][1:8].all()     # C = 7 at W = 8: fewer than W candidates


@pytest.mark.parametrize("case,mt", sbc.TRANSLATOR_CASES)
def test_translator_cases_have_margins_above_the_score_noise(golden_dir, case, mt):
    """the decodes the GPU test compares with the CPU restatement: every selection is decided by more than DECODE_MARGIN, far above
    what fp32 score rows computed in another order can move (the project's 1e-4 rule), and so above MARGIN"""
    _, cfg, batch, model = build_model(case, mt, golden_dir, "cpu")
    for W in sbc.TRANSLATOR_WIDTHS:
        ref = sbc.translator_reference(case, mt, W, cfg, model, batch)
        assert min(float(m.min()) for m in ref[5]) >= sbc.DECODE_MARGIN >= sbc.MARGIN, (W, [m.tolist() for m in ref[5]])
