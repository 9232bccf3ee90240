"""Random-sampling decoding without a GPU: the Python port of the counter-based hash against known answers of the C++ function, the
argument checks of Translator.translate_batch_sample / ops.check_sampling, and the selection rule of tests/sampling_reference.py (top-k,
top-p, min length, temperature) on hand-built rows, with a chi-square check that its draws follow the filtered softmax."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import sampling_reference as sr  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import ops, synthetic as syn  # noqa: E402
from svpc_amd.synthetic import EOS, PAD, UNK  # noqa: E402

O = type("O", (), {"cuda": False})

# (seed, site, idx, svpc_hash32(seed, site, idx)): printed once by a host-only build of svpc_amd/csrc/common.h
HASH_KAT = [
    (0, 0, 0, 33350994), (0, 0, 1, 2767685996), (0, 0, 4095, 1718766457), (0, 0, 12579766, 1402174845), (0, 0, 4294967303, 2353839235),
    (0, 1, 0, 83415710), (0, 20, 4095, 179298301), (1, 0, 0, 2672842292), (1, 1, 0, 1136996714), (1, 1, 1, 83415710),
    (1, 20, 4294967303, 2425772240), (2019, 0, 0, 3897537647), (2019, 1, 12579766, 3952043450), (2019, 20, 1, 1048242462),
    (81985529216486895, 0, 4095, 2808710536), (81985529216486895, 1, 12579766, 14258433), (81985529216486895, 20, 4294967303, 1329158819),
    (9223372036854775807, 0, 0, 2189224271), (9223372036854775807, 1, 4095, 767952369), (9223372036854775807, 20, 12579766, 511668141),
]
MIX_KAT = [(0, 0), (1, 1753845952), (3735928559, 3861431939), (4294967295, 1734902346)]


def test_hash_port_matches_the_cpp_function():
    for x, y in MIX_KAT:
        assert sr.mix32(x) == y
    for seed, site, idx, h in HASH_KAT:
        assert sr.hash32(seed, site, idx) == h
        assert int(sr.hash32_np(seed, site, [idx])[0]) == h


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
    dict(num_samples=0), dict(num_samples=9), dict(num_samples=2.0), dict(num_samples=True),
    dict(random_sampling_temp=0.0), dict(random_sampling_temp=-1.0), dict(random_sampling_temp=float("inf")),
    dict(random_sampling_temp=float("nan")), dict(random_sampling_temp="hot"),
    dict(random_sampling_topk=-2), dict(random_sampling_topk=1.5),
    dict(random_sampling_topp=-0.1), dict(random_sampling_topp=1.5), dict(random_sampling_topp=float("nan")),
    dict(min_length=-1), dict(min_length=6), dict(min_length=1.0),
    dict(seed=-1), dict(seed=1 << 63), dict(seed=1.5), dict(seed="7"), dict(seed=True),
]


@pytest.mark.parametrize("kw", BAD, ids=[",".join("%s=%r" % i for i in d.items()) for d in BAD])
def test_bad_arguments_raise_value_error(tiny, kw):
    cfg, batch, _ = tiny
    assert cfg.max_t_len == 6
    with pytest.raises(ValueError):
        _tr(tiny).translate_batch_sample(syn.translate_inputs(batch), **kw)


def test_bad_opt_attribute_raises_value_error(tiny):
    tr = _tr(tiny)
    tr.opt.random_sampling_topp = 2.0
    with pytest.raises(ValueError):
        tr.translate_batch_sample(syn.translate_inputs(tiny[1]))
    with pytest.raises(ValueError):                              # (a keyword overrides the attribute; the bad one is then unread)
        tr.translate_batch_sample(syn.translate_inputs(tiny[1]), random_sampling_topk=-5, random_sampling_topp=0.5)


def test_rows_wider_than_4096_columns_raise_value_error(tiny):
    cfg, batch, _ = tiny
    inputs = list(syn.translate_inputs(batch))
    inputs[8] = [dict(d) for d in inputs[8]]
    inputs[8][0] = {"w%d" % i: cfg.vocab_size + i for i in range(4097 - cfg.vocab_size)}      # C = V + X = 4097
    with pytest.raises(ValueError, match="4096"):
        _tr(tiny).translate_batch_sample(inputs)


def test_unknown_keyword_raises_type_error(tiny):
    with pytest.raises(TypeError):
        _tr(tiny).translate_batch_sample(syn.translate_inputs(tiny[1]), beam_size=2)
    with pytest.raises(TypeError):
        _tr(tiny).translate_batch_sample(syn.translate_inputs(tiny[1]), random_sampling_tmp=0.5)


def test_non_incremental_raises_not_implemented(tiny):
    with pytest.raises(NotImplementedError):
        _tr(tiny, incremental=False).translate_batch_sample(syn.translate_inputs(tiny[1]), 2, seed=3)


def test_check_sampling_normalises():
    c = ops.check_sampling(22, 3, 0.7, -1, 1.0, 4, seed=np.int64(5), max_cols=4096)
    assert c == dict(num_samples=3, random_sampling_temp=0.7, random_sampling_topk=0, random_sampling_topp=1.0, min_length=4, seed=5)
    assert ops.check_sampling(22)["seed"] is None
    assert ops.check_sampling(22, seed=(1 << 63) - 1)["seed"] == (1 << 63) - 1


def test_opt_attributes_are_read_and_seed_is_not(tiny, monkeypatch):
    """``opt`` supplies the sampling settings (keywords override them); ``opt.seed`` (the reference's training seed) is not read"""
    seen = {}
    tr = _tr(tiny)
    tr.opt.random_sampling_temp = 0.25
    tr.opt.random_sampling_topk = 7
    tr.opt.seed = 2019

    def fake(*a, **kw):
        seen.update(kw)
        raise StopIteration
    monkeypatch.setattr(tr, "_translate", fake)
    with pytest.raises(StopIteration):
        tr.translate_batch_sample(syn.translate_inputs(tiny[1]), 2, random_sampling_topk=3)
    d = seen["decode"]
    assert (d.kind, d.width, d.sampling, d.n_best) == ("sample", 2, (0.25, 3, 0.0, 0), 2) and d.seed is None


# ------------------------------------------------------------------------------------------------ the selection rule
def _row(C, logits, rng):
    return (rng.standard_normal(C) * 2).astype(np.float32) if logits else (rng.random(C) ** 3).astype(np.float32)


@pytest.mark.parametrize("logits", [False, True])
def test_topk_one_is_argmax(logits):
    rng = np.random.default_rng(3 + logits)
    R, C = 64, 300
    s = np.stack([_row(C, logits, rng) for _ in range(R)])
    s[:, UNK] = 60.0                              # never a candidate
    s[5, 40] = s[5, 41] = s[5].max() + 1.0        # a tie: the lower column
    for seed, temp, topp in ((0, 1.0, 0.0), (9, 0.3, 0.5), (1 << 40, 4.0, 0.95)):
        picks, cum, fin, ln, _ = sr.sample_select(s, [C] * R, [0] * R, 3, logits, np.zeros(R, np.float32), np.zeros(R, bool),
                                                  np.zeros(R, np.int64), seed, temp=temp, topk=1, topp=topp)
        masked = s.copy()
        masked[:, UNK] = -np.inf
        np.testing.assert_array_equal(picks, masked.argmax(1))
        assert picks[5] == 40 and np.all(ln == 4)
        st = np.stack([sr.step_scores(row, logits) for row in s])
        np.testing.assert_array_equal(cum, st[np.arange(R), picks])


def test_kept_sets_on_hand_built_rows():
    #           c: 0     1    2    3    4     5(EOS) 6(UNK) 7     8     9
    p = np.array([0.05, 0.3, 0.2, 0.1, 0.15, 0.1, 0.9, 0.05, 0.05, 0.0], np.float32)
    C = len(p)

    def kept(**kw):
        return sr.filtered(p, C, False, 2, **kw)[0].tolist()
    assert kept() == [1, 2, 4, 3, 5, 0, 7, 8]                    # ≻ order; UNK and the zero column are not candidates
    assert kept(topk=4) == [1, 2, 4, 3]                          # the 0.1 tie keeps the lower column
    assert kept(topk=100) == kept() and kept(topk=0) == kept()
    assert kept(topp=0.1) == [1]                                 # always at least the first column
    assert kept(topp=0.6) == [1, 2, 4]                           # 0.3 + 0.2 < 0.6 ≤ 0.3 + 0.2 + 0.15
    assert kept(topk=4, topp=0.9) == [1, 2, 4, 3]                # the mass of K1 (0.75) is W
    assert kept(topk=4, topp=0.7) == [1, 2, 4]                   # 0.7 · 0.75 = 0.525: 0.3 + 0.2 < 0.525 ≤ 0.3 + 0.2 + 0.15
    assert kept(topp=1.0) == kept() and kept(topp=0.0) == kept()
    assert kept(min_length=3) == [1, 2, 4, 3, 0, 7, 8]           # p = 3 ≤ m: no EOS
    assert kept(min_length=2) == kept() and kept(min_length=1) == kept()
    # temperature flattens or sharpens the top-p mass: at τ = 0.25 the first column alone holds > 60 %
    assert kept(topp=0.6, temp=0.25) == [1]
    assert kept(topp=0.6, temp=4.0) == [1, 2, 4, 3, 5]
    assert sr.filtered(np.zeros(C, np.float32), C, False, 0) is None


def test_finished_and_empty_rows():
    R, C = 4, 12
    s = np.full((R, C), 0.1, np.float32)
    s[2] = 0.0                                    # every probability zero: K0 empty
    s[3, :] = 0.0
    s[3, EOS] = 1.0                               # only EOS, barred by the min length: K0 empty
    cum = np.array([-1.0, -2.0, -3.0, -4.0], np.float32)
    fin = np.array([True, False, False, False])
    ln = np.array([2, 0, 0, 0])
    picks, c, f, l_, _ = sr.sample_select(s, [C] * R, [0] * R, 4, False, cum, fin, ln, 11, min_length=5)
    assert picks.tolist() == [PAD, picks[1], PAD, PAD] and picks[1] not in (UNK, EOS, PAD)
    assert c[0] == -1.0 and c[2] == -np.inf and c[3] == -np.inf and c[1] == np.float32(-2.0) + sr.step_scores(s[1], False)[0]
    assert f.tolist() == [True, False, True, True] and l_.tolist() == [2, 5, 5, 5]


SETTINGS = [
    dict(logits=False, temp=1.0, topk=0, topp=0.0),
    dict(logits=False, temp=0.5, topk=5, topp=0.0),
    dict(logits=False, temp=2.0, topk=0, topp=0.8),
    dict(logits=True, temp=1.0, topk=6, topp=0.9),
    dict(logits=True, temp=0.7, topk=0, topp=0.0),
]


@pytest.mark.parametrize("st", SETTINGS, ids=["%s" % ",".join("%s=%s" % i for i in d.items()) for d in SETTINGS])
def test_reference_draws_follow_the_filtered_softmax(st):
    """one row drawn under 24 fixed seeds × 1,000 rows (every row its own counter) — the counts against softmax(z) over K2"""
    rng = np.random.default_rng(17)
    C = 24
    row = (rng.standard_normal(C) * 1.5).astype(np.float32) if st["logits"] else rng.dirichlet(np.ones(C) * 0.7).astype(np.float32)
    row[UNK] = 5.0 if st["logits"] else 0.3
    kw = dict(temp=st["temp"], topk=st["topk"], topp=st["topp"])
    target = sr.target_distribution(row, C, st["logits"], 2, **kw)
    counts = np.zeros(C)
    n_rows = 1000
    for seed in range(24):
        picks = sr.sample_select(np.tile(row, (n_rows, 1)), [C] * n_rows, [0] * n_rows, 2, st["logits"], np.zeros(n_rows, np.float32),
                                 np.zeros(n_rows, bool), np.zeros(n_rows, np.int64), seed * 7919, **kw)[0]
        counts += np.bincount(picks, minlength=C)
    assert counts[target == 0].sum() == 0, "a draw outside K2"
    stat, dof = sr.chi_square(counts, target)
    assert dof >= 2 and stat < sr.chi_square_bound(dof), (stat, dof)
