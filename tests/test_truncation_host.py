"""Truncated sampling without a GPU: the argument checks of ops.check_truncation / Translator.translate_batch_sample, the keyword and
``opt`` plumbing into the ``Decode``, the truncation rules of tests/truncation_reference.py on hand-built rows with known kept sets, a
chi-square check that its draws follow the truncated softmax, and — on the reference alone — the conditions tests/test_truncation_gpu.py
relies on: how many rows of its tables sit within the tie bound of a cut, and that its (case, setting) pairs have no undecided step."""
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
from svpc_amd.synthetic import UNK  # noqa: E402

O = type("O", (), {"cuda": False})
NAMES = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


# ------------------------------------------------------------------------------------------------ argument checks and plumbing
@pytest.fixture(scope="module")
def tiny(golden_dir):
    _, cfg, batch, model = build_model("tiny", "vivt", golden_dir, "cpu")
    return cfg, batch, model


def _tr(tiny, **kw):
    from svpc_amd.translator import Translator
    cfg, _, model = tiny
    return Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, **kw)


BAD = [dict([(n, v)]) for n in NAMES for v in (-0.1, 1.5, float("nan"), float("inf"), "0.5", None, True, [0.5])] + \
      [dict(min_p=1.0), dict(epsilon_cutoff=1.0), dict(eta_cutoff=1.0), dict(min_p=1), dict(typical_p=1.0000001)]


@pytest.mark.parametrize("kw", BAD, ids=[",".join("%s=%r" % i for i in d.items()) for d in BAD])
def test_bad_arguments_raise_value_error(tiny, kw):
    with pytest.raises(ValueError):
        ops.check_truncation(**kw)
    with pytest.raises(ValueError):
        _tr(tiny).translate_batch_sample(syn.translate_inputs(tiny[1]), **kw)


def test_check_truncation_normalises():
    assert ops.check_truncation() == dict(min_p=0.0, typical_p=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
    c = ops.check_truncation(np.float32(0.25), 1.0, 0, np.float64(3e-3))
    assert c == dict(min_p=0.25, typical_p=0.0, epsilon_cutoff=0.0, eta_cutoff=3e-3) and all(type(v) is float for v in c.values())
    assert ops.check_truncation(typical_p=1)["typical_p"] == 0.0 and ops.check_truncation(typical_p=0.999)["typical_p"] == 0.999
    # the sampling settings are what they were
    assert ops.check_sampling(22, 3, 0.7, -1, 1.0, 4, seed=5) == dict(num_samples=3, random_sampling_temp=0.7, random_sampling_topk=0,
                                                                      random_sampling_topp=1.0, min_length=4, seed=5)


def _decode_of(tr, monkeypatch, *a, **kw):
    seen = {}

    def fake(*a_, **kw_):
        seen.update(kw_)
        raise StopIteration
    monkeypatch.setattr(tr, "_translate", fake)
    with pytest.raises(StopIteration):
        tr.translate_batch_sample(*a, **kw)
    return seen["decode"]


def test_keywords_and_opt_attributes_reach_the_decode(tiny, monkeypatch):
    tr = _tr(tiny)
    inputs = syn.translate_inputs(tiny[1])
    plain = _decode_of(tr, monkeypatch, inputs, 2, random_sampling_topk=3)
    assert plain.truncation is None and plain.sampling == (1.0, 3, 0.0, 0)
    off = _decode_of(tr, monkeypatch, inputs, 2, random_sampling_topk=3, min_p=0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0)
    assert off.truncation is None and off.key == plain.key
    d = _decode_of(tr, monkeypatch, inputs, 2, random_sampling_topk=3, typical_p=0.9, eta_cutoff=3e-3)
    assert d.truncation == (0.0, 0.9, 0.0, 3e-3) and d.sampling == plain.sampling and (d.kind, d.width, d.n_best) == ("sample", 2, 2)
    assert d.key != plain.key and d.key[:len(plain.key)] == plain.key
    d2 = _decode_of(tr, monkeypatch, inputs, 2, random_sampling_topk=3, typical_p=0.37, eta_cutoff=3e-3)
    assert d2.key != d.key
    # ``opt`` supplies them, keywords override
    tr.opt.min_p = 0.07
    tr.opt.typical_p = 0.2
    d = _decode_of(tr, monkeypatch, inputs, 2, typical_p=0.95)
    assert d.truncation == (0.07, 0.95, 0.0, 0.0) and d.sampling == (1.0, 0, 0.0, 0)
    tr.opt.eta_cutoff = 2.0
    with pytest.raises(ValueError):
        tr.translate_batch_sample(inputs, 2)


def test_unknown_keywords_still_raise_type_error(tiny):
    inputs = syn.translate_inputs(tiny[1])
    with pytest.raises(TypeError):
        _tr(tiny).translate_batch_sample(inputs, typical=0.9)
    with pytest.raises(TypeError):
        _tr(tiny).translate_batch_sample(inputs, min_p=0.1, top_a=0.2)
    for n in NAMES:                                        # stochastic beam search keeps rejecting them
        with pytest.raises(TypeError):
            _tr(tiny).translate_batch_stochastic(inputs, 2, **{n: 0.1})


def test_unlikelihood_sequence_step_forwards_the_keywords(tiny, monkeypatch):
    """the one caller that filtered its sampling keywords admits the new ones, and still refuses unknown ones"""
    from svpc_amd import unlikelihood as ul
    tr = _tr(tiny)
    seen = {}

    def fake(inputs, **kw):
        seen.update(kw)
        raise StopIteration
    monkeypatch.setattr(tr, "translate_batch_sample", fake)
    step = ul.Unlikelihood(tr)
    with pytest.raises(StopIteration):
        step.sequence_step(syn.translate_inputs(tiny[1]), source="sample", seed=3, random_sampling_temp=0.8, typical_p=0.9, eta_cutoff=3e-3)
    assert seen == dict(num_samples=1, seed=3, random_sampling_temp=0.8, typical_p=0.9, eta_cutoff=3e-3)
    with pytest.raises(TypeError):
        step.sequence_step(syn.translate_inputs(tiny[1]), source="sample", typical=0.9)


# ------------------------------------------------------------------------------------------------ the rules on hand-built rows
def _kept(p, temp=1.0, **trunc):
    p = np.asarray(p, np.float32)
    f = sr.filtered(p, len(p), False, 2, temp)
    return trr.truncate(f[0], f[1], **trunc)[0].tolist()


#              c: 0     1    2    3    4     5     6(UNK) 7     8     9
P = np.array([0.05, 0.3, 0.2, 0.1, 0.15, 0.1, 0.9, 0.05, 0.05, 0.0], np.float32)
ALL = [1, 2, 4, 3, 5, 0, 7, 8]


def test_all_off_is_the_identity():
    f = sr.filtered(P, len(P), False, 2)
    k, z, mg = trr.truncate(f[0], f[1])
    assert k.tolist() == ALL and np.array_equal(z, f[1]) and mg == np.inf
    k, z, mg = trr.truncate(f[0], f[1], min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
    assert k.tolist() == ALL and np.array_equal(z, f[1])


def test_min_p_on_a_hand_built_row():
    assert _kept(P, min_p=1e-300) == ALL                                 # a → 0 keeps all
    assert _kept(P, min_p=0.4) == [1, 2, 4]                              # w = p / 0.3: 0.2 → 0.67, 0.15 → 0.5, 0.1 → 0.33
    assert _kept(P, min_p=0.6) == [1, 2]
    assert _kept(P, min_p=0.999) == [1]                                  # the first column always stays
    assert _kept(P, min_p=0.4, temp=2.0) == [1, 2, 4, 3, 5, 0, 7, 8]     # w = sqrt(p / 0.3): 0.05 → 0.408
    assert _kept([0.2, 0.2, 0.2, 0.1], min_p=0.9) == [0, 1, 2]           # columns tied with the first have w = 1


def test_typical_on_hand_built_rows():
    u = np.full(12, 0.05, np.float32)
    u[UNK] = 0.9
    every = [c for c in range(12) if c != UNK]
    for m in (0.01, 0.37, 0.9, 0.999):                                    # a uniform row: every d is equal, they stay together
        assert _kept(u, typical_p=m) == every
    # a mode of 0.4 over ten columns of 0.06: H = 2.05; −ln q is 0.92 for the mode (d = 1.14) and 2.81 for the others (d = 0.76), so the
    # ten come first and hold 0.6 of the mass: the mode is dropped up to m = 0.6
    row = np.array([0.4] + [0.06] * 10, np.float32)
    row = np.insert(row, UNK, 0.9)
    tail = [c for c in range(1, 12) if c != UNK]
    assert _kept(row, typical_p=0.5) == tail and _kept(row, typical_p=0.59) == tail
    assert _kept(row, typical_p=0.7) == [0] + tail
    # the row above: H = 1.887; d is smallest for 0.15 (−ln q = 1.897), then 0.2, then the 0.1 pair, then 0.3, then the three 0.05
    assert _kept(P, typical_p=0.1) == [4]
    assert _kept(P, typical_p=0.3) == [2, 4]
    assert _kept(P, typical_p=0.5) == [2, 4, 3, 5]                        # the tied 0.1 columns enter together: 0.35 → 0.55
    assert _kept(P, typical_p=0.8) == [1, 2, 4, 3, 5]
    assert _kept(P, typical_p=0.9) == ALL                                 # … and so do the three 0.05 columns
    assert _kept(P, typical_p=1.0) == ALL and _kept(P, typical_p=0.0) == ALL


def test_epsilon_and_eta_on_hand_built_rows():
    assert _kept(P, epsilon_cutoff=0.06) == [1, 2, 4, 3, 5]
    assert _kept(P, epsilon_cutoff=0.25) == [1]
    assert _kept(P, epsilon_cutoff=0.9) == [1]                            # nothing reaches ε: the first column stays
    # eta: thr = min(η, √η·exp(−H)), exp(−H) = exp(−1.887) = 0.1515
    assert _kept(P, eta_cutoff=0.06) == [1, 2, 4, 3, 5, 0, 7, 8]          # √0.06 · 0.1515 = 0.037 < 0.05
    assert _kept(P, eta_cutoff=0.25) == [1, 2, 4, 3, 5]                   # 0.5 · 0.1515 = 0.076
    assert _kept(P, eta_cutoff=0.9) == [1, 2, 4]                          # 0.949 · 0.1515 = 0.144
    assert _kept(P, eta_cutoff=1e-4) == ALL                               # η itself is the smaller bound: 1e-4 < 1e-2 · 0.1515
    rng = np.random.default_rng(4)
    for _ in range(50):                                                   # at the same parameter eta's set ⊇ epsilon's
        row = rng.dirichlet(np.ones(30) * rng.choice([0.1, 0.5, 2.0])).astype(np.float32)
        par = float(rng.choice([3e-3, 0.02, 0.04, 0.2]))
        assert set(_kept(row, epsilon_cutoff=par)) <= set(_kept(row, eta_cutoff=par))


def test_stages_run_in_order_on_renormalised_survivors():
    # min-p 0.4 leaves {0.3, 0.2, 0.15}: q = 0.46, 0.31, 0.23.  ε = 0.25 then drops 0.15, which ε = 0.25 alone (q = 0.3, 0.2, …) would not
    # reach either — but ε = 0.17 keeps 0.2 (q = 0.2 of the full row) only with the renormalisation … and 0.15 (q = 0.23 ≥ 0.17) too
    assert _kept(P, min_p=0.4, epsilon_cutoff=0.25) == [1, 2]
    assert _kept(P, epsilon_cutoff=0.17) == [1, 2] and _kept(P, min_p=0.4, epsilon_cutoff=0.17) == [1, 2, 4]
    # typical first drops the mode, epsilon and eta then keep the new first column
    row = np.insert(np.array([0.4] + [0.06] * 10, np.float32), UNK, 0.9)
    assert _kept(row, typical_p=0.5, epsilon_cutoff=0.5) == [1]
    assert _kept(row, typical_p=0.5, eta_cutoff=0.5) == [c for c in range(1, 12) if c != UNK]      # thr = √0.5 · 0.1 = 0.07 < 0.1


SETTINGS = [dict(logits=False, temp=1.0, trunc=dict(typical_p=0.9)),
            dict(logits=False, temp=1.3, trunc=dict(min_p=0.07, eta_cutoff=0.04)),
            dict(logits=True, temp=0.7, topk=12, trunc=dict(typical_p=0.37, epsilon_cutoff=3e-3))]


@pytest.mark.parametrize("st", range(len(SETTINGS)))
def test_reference_draws_follow_the_truncated_softmax(st):
    st = SETTINGS[st]
    rng = np.random.default_rng(17)
    C, n_rows = 24, 1000
    row = (rng.standard_normal(C) * 1.5).astype(np.float32) if st["logits"] else rng.dirichlet(np.ones(C) * 0.7).astype(np.float32)
    row[UNK] = 5.0 if st["logits"] else 0.3
    kw = dict(temp=st["temp"], topk=st.get("topk", 0))
    target = trr.target_distribution(row, C, st["logits"], 2, **kw, **st["trunc"])
    assert 2 < (target > 0).sum() < C - 1
    counts = np.zeros(C)
    for seed in range(12):
        out = trr.trunc_select(np.tile(row, (n_rows, 1)), [C] * n_rows, [0] * n_rows, 2, st["logits"], np.zeros(n_rows, np.float32),
                               np.zeros(n_rows, bool), np.zeros(n_rows, np.int64), seed * 7919, **kw, **st["trunc"])
        counts += np.bincount(out[0], minlength=C)
        assert np.all(out[5] == (target > 0).sum())
    assert counts[target == 0].sum() == 0, "a draw outside the kept set"
    stat, dof = sr.chi_square(counts, target)
    assert dof >= 2 and stat < sr.chi_square_bound(dof), (stat, dof)


def test_all_off_select_is_sample_select():
    rng = np.random.default_rng(9)
    for logits in (False, True):
        s, row_c, row_x, cum, fin, length = trr.tables(rng, 7, 2, logits, False, cmax_hi=120)
        for k, q, t in trr.BASE:
            a = sr.sample_select(s, row_c, row_x, 3, logits, cum, fin.astype(bool), length, 41, temp=t, topk=k, topp=q)
            b = trr.trunc_select(s, row_c, row_x, 3, logits, cum, fin.astype(bool), length, 41, temp=t, topk=k, topp=q)
            for x, y in zip(a[:4], b[:4]):
                np.testing.assert_array_equal(x, y)
            np.testing.assert_array_equal(a[4], b[4][:, :3])


# ------------------------------------------------------------------------------------------------ what the GPU tests rely on
@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("R", [1, 3, 8])
def test_kernel_tables_leave_the_tie_allowance_to_rounding(R, logits):
    """the reference alone flags at most rows // 400 of the kernel test's rows (its allowance is rows // 200), and every setting truncates"""
    flagged = rows = 0
    cut = {}
    for tb, st, trunc, ref in trr.kernel_cases(R, logits):
        flagged += int(trr.flagged_rows(ref, tb[4]).sum())
        rows += tb[0].shape[0]
        plain = trr.trunc_select(tb[0], tb[1], tb[2], trr.KERNEL_POS, logits, tb[3], tb[4].astype(bool), tb[5], st["seed"], temp=st["t"],
                                 topk=st["k"], topp=st["q"], min_length=st["m"])
        assert np.all(ref[5] <= plain[5]) and np.all((ref[5] > 0) == (plain[5] > 0))
        key = tuple(sorted(trunc.items()))
        cut[key] = cut.get(key, 0) + int((ref[5] < plain[5]).sum())
    assert rows == 29 * R * 2 * len(trr.TRUNC) * len(trr.BASE)
    assert flagged <= rows // 400, (flagged, rows)
    assert all(v > 0 for v in cut.values()), cut              # every setting drops columns of some row: none of them is vacuous


def test_wide_tables_have_no_near_tie():
    for logits, tb, st, trunc, ref in trr.wide_cases():
        assert int(trr.flagged_rows(ref, tb[4]).sum()) == 0
        assert tb[1].min() >= 1025 and tb[1].max() == 4096 and tb[0].shape[0] == 24


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    cache = {}

    def get(case, mt):
        if (case, mt) not in cache:
            _, cfg, batch, model = build_model(case, mt, golden_dir, "cpu")
            model.eval()
            cache[case, mt] = (cfg, batch, {k: v.detach().clone() for k, v in model.state_dict().items()})
        return cache[case, mt]
    return get


@pytest.mark.parametrize("case,mt,trunc", trr.DECODE_PAIRS, ids=["%s-%s-%s" % (c, m, ",".join("%s=%s" % i for i in k.items()))
                                                                  for c, m, k in trr.DECODE_PAIRS])
def test_decode_pairs_have_no_undecided_step(fixtures, case, mt, trunc):
    """the (case, setting) pairs whose ids the GPU test compares: the reference alone counts no undecided step, so the GPU test's
    allowance is left for real rounding; and the truncation is not vacuous there"""
    cfg, b, P = fixtures(case, mt)
    r = trr.trunc_decode(P, cfg, b["input_ids_list"], b["video_features_list"], b["input_masks_list"], b["ingr_input_ids"],
                         b["ingr_sep_masks"], b["batch_step_num"], b["ingr_id_dict"], b["oov_word_dict"], trr.DECODE_R, trr.DECODE_SEED,
                         delta=trr.DECODE_DELTA, **trunc)
    assert sum(int(u.sum()) for u in r[4]) == 0
    assert all(float(m.min()) > trr.DECODE_DELTA for m in r[3])
    width = max(cfg.vocab_size + len(o) for o in b["oov_word_dict"])
    kept = np.concatenate([k.ravel() for k in r[5]])
    assert 0 < kept[kept > 0].mean() < 0.9 * (width - 1)
    # the replay of a decode along its own ids finds every word inside the loosened set
    f = trr.trunc_decode(P, cfg, b["input_ids_list"], b["video_features_list"], b["input_masks_list"], b["ingr_input_ids"],
                         b["ingr_sep_masks"], b["batch_step_num"], b["ingr_id_dict"], b["oov_word_dict"], trr.DECODE_R, trr.DECODE_SEED,
                         delta=trr.MEMBER_DELTA, forced=r[0], **trunc)
    assert sum(int(u.sum()) for u in f[4]) == 0
    assert all(torch.equal(x, y) for x, y in zip(f[0], r[0]))
