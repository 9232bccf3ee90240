"""Ensemble decoding without a GPU: the rule (tests/ensemble_reference.py::combine) and its properties, every host-side refusal of
``ops.ensemble_combine`` and ``EnsembleTranslator``, the header's declaration, and the loud failure on CPU tensors."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import ensemble_reference as er  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import _lib, ops  # noqa: E402
from svpc_amd.ensemble import AGREE, EnsembleTranslator  # noqa: E402
from svpc_amd.synthetic import UNK  # noqa: E402

O = type("O", (), {"cuda": False})


def _probs(rng, n, C, zeros=True):
    p = rng.dirichlet(np.ones(C) * 0.5, size=n).astype(np.float32)
    if zeros:
        p[rng.random((n, C)) < 0.1] = 0.0
    return p


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_copies_under_prob_return_the_member_bit_for_bit(M):
    rng = np.random.default_rng(M)
    p = _probs(rng, 9, 77)
    p[0, :5] = [1e-45, 3e-41, 1.1754944e-38, 0.0, 1.0]          # denormals, the smallest normal, the ends
    p[1, 3] = -0.25                                              # a negative entry counts as 0
    out = er.combine([p] * M, [77] * 9, rule="prob")
    np.testing.assert_array_equal(out.view(np.int32), np.where(p > 0, p, 0).astype(np.float32).view(np.int32))
    w = [0.0] * M
    w[M - 1] = 2.5                                               # one member at (normalised) weight 1 among different members
    others = [_probs(rng, 9, 77) for _ in range(M - 1)]
    out = er.combine(others + [p], [77] * 9, weights=w, rule="prob")
    np.testing.assert_array_equal(out, np.where(p > 0, p, 0).astype(np.float32))


def test_mean_of_normalised_members_is_normalised():
    rng = np.random.default_rng(3)
    C = 200
    logit = [rng.standard_normal((6, C)).astype(np.float32) * 3 for _ in range(3)]
    w = er.normalise((0.5, 0.3, 0.2), 3)
    # (before the rounding to fp32: the fp64 rows)
    acc = np.zeros((6, C))
    for m, l in enumerate(logit):
        z = l.astype(np.float64)
        z[:, UNK] = -np.inf
        e = np.exp(z - z.max(1, keepdims=True))
        acc += w[m] * e / e.sum(1, keepdims=True)
    np.testing.assert_allclose(acc.sum(1), 1.0, rtol=0, atol=1e-12)
    out = er.combine(logit, [C] * 6, weights=(0.5, 0.3, 0.2), rule="prob", logits=True)
    np.testing.assert_array_max_ulp(out, acc.astype(np.float32), maxulp=1)
    assert np.all(out[:, UNK] == 0)
    np.testing.assert_allclose(out.astype(np.float64).sum(1), 1.0, rtol=0, atol=C * 2.0 ** -25)


@pytest.mark.parametrize("logits", [False, True])
def test_logprob_is_at_most_prob_under_equal_weights(logits):
    rng = np.random.default_rng(5)
    C = 150
    mats = [(rng.standard_normal((7, C)).astype(np.float32) * 2) if logits else _probs(rng, 7, C) for _ in range(4)]
    a = er.combine(mats, [C] * 7, rule="prob", logits=logits).astype(np.float64)
    g = er.combine(mats, [C] * 7, rule="logprob", logits=logits).astype(np.float64)
    assert np.all(g <= a * (1 + 2.0 ** -22) + 1e-45)             # AM–GM, up to the two roundings to fp32
    if not logits:                                                # 0 as soon as one member has p = 0
        zero = np.any(np.stack(mats) <= 0, axis=0)
        assert np.all(g[zero] == 0) and np.all(g[~zero] > 0)


@pytest.mark.parametrize("rule", er.RULES)
@pytest.mark.parametrize("logits", [False, True])
def test_a_zero_weight_member_changes_nothing(rule, logits):
    rng = np.random.default_rng(7)
    C = 90
    mats = [(rng.standard_normal((5, C)).astype(np.float32)) if logits else _probs(rng, 5, C) for _ in range(2)]
    dead = np.full((5, C), -np.inf if logits else 0.0, np.float32)
    ref = er.combine(mats, [C] * 5, weights=(0.6, 0.4), rule=rule, logits=logits)
    out = er.combine([mats[0], dead, mats[1]], [C] * 5, weights=(0.6, 0.0, 0.4), rule=rule, logits=logits)
    np.testing.assert_array_equal(out.view(np.int32), ref.view(np.int32))
    assert np.all(np.isfinite(out))


def test_ragged_rows_padding_and_rows_per():
    rng = np.random.default_rng(11)
    mats = [_probs(rng, 10, 40) for _ in range(2)]
    out = er.combine(mats, [17, 40], rule="prob", rows_per=5, ld_out=44)
    assert out.shape == (10, 44) and np.all(out[:5, 17:] == 0) and np.all(out[:, 40:] == 0) and np.any(out[5:, 17:40] > 0)
    dead = er.combine([np.full((2, 8), -np.inf, np.float32), np.zeros((2, 8), np.float32)], [8, 8], rule="prob", logits=True)
    assert np.all(dead[:, UNK] == 0) and np.all(dead[:, np.arange(8) != UNK] == np.float32(0.5 / 7))   # a dead member row contributes 0


# ------------------------------------------------------------------------------------------------ the binding's refusals
def _two(n=4, C=12):
    return [torch.rand(n, C), torch.rand(n, C)]


def test_header_declares_the_entry_point():
    ret, args = _lib.declarations()["svpc_ensemble_combine"]
    assert len(args) == 14
    assert _lib.load().svpc_abi_version() == 2


def test_ensemble_combine_fails_loudly_on_cpu_tensors():
    with pytest.raises(_lib.SvpcKernelError):
        ops.ensemble_combine(_two(), [12] * 4, weights=None, rule="prob", logits=False, unk=UNK)


@pytest.mark.parametrize("bad", ["dtype", "dim", "stride", "rows", "device", "n_weights", "empty", "nine", "negative", "nan", "zero",
                                 "rule", "rows_per", "row_c", "cols"])
def test_ensemble_combine_value_errors(bad):
    ms, kw = _two(), dict(weights=None, rule="prob", logits=False, unk=UNK)
    row_c = [12] * 4
    if bad == "dtype":
        ms[1] = ms[1].double()
    elif bad == "dim":
        ms[1] = ms[1].view(-1)
    elif bad == "stride":
        ms[1] = torch.rand(12, 4).t()
    elif bad == "rows":
        ms[1] = torch.rand(5, 12)
    elif bad == "device":
        ms[1] = torch.empty(4, 12, device="meta")
    elif bad == "n_weights":
        kw["weights"] = (1.0, 1.0, 1.0)
    elif bad == "empty":
        ms = []
    elif bad == "nine":
        ms = [torch.rand(4, 12) for _ in range(9)]
    elif bad == "negative":
        kw["weights"] = (1.5, -0.5)
    elif bad == "nan":
        kw["weights"] = (float("nan"), 1.0)
    elif bad == "zero":
        kw["weights"] = (0.0, 0.0)
    elif bad == "rule":
        kw["rule"] = "geometric"
    elif bad == "rows_per":
        kw["rows_per"] = 0
    elif bad == "row_c":
        row_c = [12] * 3
    elif bad == "cols":
        row_c = [13] * 4
    with pytest.raises(ValueError):
        ops.ensemble_combine(ms, row_c, **kw)


def test_weights_are_normalised_in_member_order():
    assert ops.ensemble_weights(None, 4) == [0.25] * 4
    assert ops.ensemble_weights((1, 0), 2) == [1.0, 0.0]
    assert ops.ensemble_weights((0.5, 0.3, 0.2), 3) == er.normalise((0.5, 0.3, 0.2), 3).tolist()
    with pytest.raises(ValueError):
        ops.ensemble_weights((float("inf"), 1.0), 2)


# ------------------------------------------------------------------------------------------------ the translator's refusals
@pytest.fixture(scope="module")
def tiny(golden_dir):
    _, cfg, batch, model = build_model("tiny", "vivt", golden_dir, "cpu")
    return cfg, model


def _ens(cfg, models, cfgs=None, **kw):
    cfgs = cfgs or [cfg] * len(models)
    return EnsembleTranslator(O(), [{"model_cfg": c, "model": m.state_dict()} for c, m in zip(cfgs, models)], models, **kw)


def test_ensemble_translator_is_a_translator(tiny):
    from svpc_amd.translator import Translator
    cfg, model = tiny
    other = copy.deepcopy(model)
    tr = _ens(cfg, [model, other], weights=(3, 1), combine="logprob")
    assert isinstance(tr, Translator) and tr.model is model and tr._members() == [model, other]
    assert tr.weights == [0.75, 0.25] and tr.combine == "logprob" and tr.incremental and not tr.two_streams
    assert Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model)._members() == [model]
    with pytest.raises(ValueError):
        tr.two_streams = True
    tr.two_streams = False
    with pytest.raises(TypeError):
        EnsembleTranslator(O(), [{"model_cfg": cfg, "model": model.state_dict()}], [model], incremental=False)


@pytest.mark.parametrize("field", AGREE)
def test_members_must_agree(tiny, field):
    cfg, model = tiny
    other_cfg = copy.copy(cfg)
    v = getattr(cfg, field)
    setattr(other_cfg, field, "video" if field == "model_mode" else v + 1)
    with pytest.raises(ValueError, match=field):
        _ens(cfg, [model, copy.deepcopy(model)], cfgs=[cfg, other_cfg])


@pytest.mark.parametrize("bad", ["empty", "nine", "weights", "n_weights", "combine", "device", "checkpoints"])
def test_ensemble_translator_value_errors(tiny, bad):
    cfg, model = tiny
    models, kw, cfgs = [model, copy.deepcopy(model)], {}, None
    if bad == "empty":
        models = []
    elif bad == "nine":
        models = [model] * 9
    elif bad == "weights":
        kw["weights"] = (1.0, -1.0)
    elif bad == "n_weights":
        kw["weights"] = (1.0,)
    elif bad == "combine":
        kw["combine"] = "mean"
    elif bad == "device":
        models[1] = copy.deepcopy(model).to("meta")
    elif bad == "checkpoints":
        cfgs = [cfg]
    with pytest.raises(ValueError):
        _ens(cfg, models, cfgs=cfgs, **kw)
