"""Contrastive decoding without a GPU: the rule (tests/contrast_decode_reference.py::combine) and its properties, one hand-computed
example, every host-side refusal of ``ops.contrast_combine`` and of ``ContrastTranslator``'s constructor (all before any device work),
the header's declaration and the library's export."""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import contrast_decode_reference as cr  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import _lib, ops  # noqa: E402
from svpc_amd.contrast_decode import ContrastTranslator  # noqa: E402
from svpc_amd.ensemble import AGREE, EnsembleTranslator  # noqa: E402
from svpc_amd.synthetic import UNK  # noqa: E402
from svpc_amd.translator import Translator  # noqa: E402

O = type("O", (), {"cuda": False})
COEF = [(1.5, 0.5, 0.1), (1.0, 1.0, 0.1), (1.0, 0.0, 0.0), (2.0, 1.0, 1.0), (1.5, 0.5, 1e-6)]


def _scores(rng, n, C, logits):
    if logits:
        s = (rng.standard_normal((n, C)) * 3).astype(np.float32)
        s[rng.random((n, C)) < 0.05] = -np.inf
        return s
    p = rng.dirichlet(np.ones(C) * 0.5, size=n).astype(np.float32)
    p[rng.random((n, C)) < 0.1] = 0.0
    return p


def _logp(raw, logits):
    """fp64 log-probabilities of whole rows, UNK left out (−inf)"""
    raw = raw.astype(np.float64).copy()
    raw[:, UNK] = -np.inf if logits else 0.0
    with np.errstate(divide="ignore"):
        if not logits:
            return np.log(np.where(raw > 0, raw, 0.0))
        mx = raw.max(1, keepdims=True)
        return raw - (mx + np.log(np.exp(raw - mx).sum(1, keepdims=True)))


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("we,wa,alpha", COEF)
def test_rows_are_distributions_over_the_head(we, wa, alpha, logits):
    rng = np.random.default_rng(int(we * 10 + wa * 100 + logits))
    C = 120
    e, a = _scores(rng, 9, C, logits), _scores(rng, 9, C, logits)
    out, mask = cr.combine(e, a, [C] * 9, we, wa, alpha, logits)
    assert out.shape == mask.shape == (9, C) and out.dtype == np.float32 and np.all(np.isfinite(out))
    assert np.all(out[~mask] == 0) and np.all(out[:, UNK] == 0) and not mask[:, UNK].any()
    assert mask.any(1).all()
    np.testing.assert_allclose(out.astype(np.float64).sum(1), 1.0, rtol=0, atol=1e-6)
    le = _logp(e, logits)                                          # the head, restated: within log α of the expert's top
    with np.errstate(invalid="ignore"):
        d = le - le.max(1, keepdims=True)
    clear = np.abs(d - cr.log_alpha(alpha)) > 1e-9 if alpha > 0 else np.ones_like(mask)
    want = np.isfinite(le) & (d >= cr.log_alpha(alpha))
    assert np.all(mask[clear] == want[clear])
    if alpha == 1.0:                                               # only the columns tied at the top
        top = np.where(np.arange(C) == UNK, -np.inf, e.astype(np.float64)).max(1, keepdims=True)
        np.testing.assert_array_equal(mask, (e == top) & (np.arange(C) != UNK))


@pytest.mark.parametrize("logits", [False, True])
def test_a_head_of_one_column_is_exactly_one(logits):
    rng = np.random.default_rng(2)
    C = 50
    e, a = _scores(rng, 4, C, logits), _scores(rng, 4, C, logits)
    e[:, 17] = 30.0 if logits else 0.99                            # far above everything else: alone within α = 0.5 of itself
    for we, wa in ((1.5, 0.5), (1.0, 1.0), (3.0, 2.0)):
        out, mask = cr.combine(e, a, [C] * 4, we, wa, 0.5, logits)
        assert np.all(mask.sum(1) == 1) and np.all(mask[:, 17])
        np.testing.assert_array_equal(out[:, 17].view(np.int32), np.ones(4, np.float32).view(np.int32))
        assert np.all(out[:, np.arange(C) != 17] == 0)


def test_no_amateur_and_no_threshold_is_the_expert_renormalised():
    """wa = 0, α = 0 → p_e / Σ_{c ≠ UNK} p_e; the amateur matrix is never read (NaN everywhere does not matter)"""
    rng = np.random.default_rng(3)
    C = 80
    e = _scores(rng, 6, C, False)
    e[:, UNK] = 0.4
    out, mask = cr.combine(e, np.full((6, C), np.nan, np.float32), [C] * 6, 1.0, 0.0, 0.0, False)
    p = np.where(e > 0, e, 0).astype(np.float64)
    p[:, UNK] = 0
    np.testing.assert_allclose(out, p / p.sum(1, keepdims=True), rtol=1e-6, atol=0)
    np.testing.assert_array_equal(mask, p > 0)
    out_none, _ = cr.combine(e, None, [C] * 6, 1.0, 0.0, 0.0, False)
    np.testing.assert_array_equal(out_none.view(np.int32), out.view(np.int32))
    lg = _scores(rng, 6, C, True)                                  # logits mode: softmax without UNK
    out, mask = cr.combine(lg, None, [C] * 6, 1.0, 0.0, 0.0, True)
    np.testing.assert_allclose(out, np.exp(_logp(lg, True)), rtol=1e-6, atol=0)


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("we,wa", [(1.5, 0.5), (2.0, 1.0), (1.0, 0.0)])
def test_an_amateur_equal_to_the_expert_returns_the_expert_over_the_head(we, wa, logits):
    """we − wa = 1 and a = e: s = log p_e on the head (p_e > 1e-30 there), so out is the expert renormalised over the head"""
    rng = np.random.default_rng(4)
    C = 90
    e = _scores(rng, 7, C, logits)
    out, mask = cr.combine(e, e.copy(), [C] * 7, we, wa, 0.1, logits)
    p = np.where(mask, np.exp(_logp(e, logits)), 0.0)
    np.testing.assert_allclose(out, p / p.sum(1, keepdims=True), rtol=1e-6, atol=0)


def test_a_column_the_amateur_gives_zero_gets_the_floor():
    C = 10
    e = np.full((1, C), 0.1, np.float32)
    a = np.full((1, C), 0.1, np.float32)
    a[0, 3] = 0.0                                                  # log 0 = −inf → L0, not +inf in the score
    a[0, 4] = 1e-38                                                # below the floor too
    out, mask = cr.combine(e, a, [C], 1.5, 0.5, 0.1, False)
    assert np.all(np.isfinite(out)) and mask[0, np.arange(C) != UNK].all()
    u = np.full(C, 0.1 ** 1.5 / 0.1 ** 0.5)
    u[[3, 4]] = 0.1 ** 1.5 / 1e-30 ** 0.5
    u[UNK] = 0
    np.testing.assert_allclose(out[0], u / u.sum(), rtol=1e-6)
    assert out[0, 3] == out[0, 4] and out[0, 3] > 0.49


@pytest.mark.parametrize("logits", [False, True])
def test_dead_rows(logits):
    rng = np.random.default_rng(6)
    C = 40
    dead = np.full((1, C), -np.inf if logits else 0.0, np.float32)
    dead[0, UNK] = 50.0 if logits else 1.0                         # a finite UNK does not revive the row
    live = _scores(rng, 1, C, logits)
    out, mask = cr.combine(dead, live, [C], 1.5, 0.5, 0.1, logits)               # dead expert row: zeros
    assert np.all(out == 0) and not mask.any()
    out, mask = cr.combine(live, dead, [C], 1.5, 0.5, 0.1, logits)               # dead amateur row: finite, the expert over its head
    assert np.all(np.isfinite(out)) and mask.any()
    _, ref_mask = cr.combine(live, None, [C], 1.5, 0.0, 0.1, logits)           # (the head is the expert's alone)
    np.testing.assert_array_equal(mask, ref_mask)
    p = np.where(mask, np.exp(1.5 * _logp(live, logits)), 0.0)                  # (every la = L0: a constant that cancels)
    np.testing.assert_allclose(out, p / p.sum(1, keepdims=True), rtol=1e-6, atol=0)


@pytest.mark.parametrize("logits", [False, True])
def test_a_huge_unk_value_leaks_nowhere(logits):
    rng = np.random.default_rng(7)
    C = 60
    e, a = _scores(rng, 5, C, logits), _scores(rng, 5, C, logits)
    e2, a2 = e.copy(), a.copy()
    e2[:, UNK], a2[:, UNK] = (80.0, -80.0) if logits else (1.0, 0.0)
    e[:, UNK], a[:, UNK] = (-np.inf, 3.0) if logits else (0.0, 0.5)
    for we, wa, alpha in COEF:
        o1, m1 = cr.combine(e, a, [C] * 5, we, wa, alpha, logits)
        o2, m2 = cr.combine(e2, a2, [C] * 5, we, wa, alpha, logits)
        np.testing.assert_array_equal(o1.view(np.int32), o2.view(np.int32))
        np.testing.assert_array_equal(m1, m2)
        assert np.all(o1[:, UNK] == 0)


def test_ragged_rows_padding_and_rows_per():
    rng = np.random.default_rng(8)
    e, a = _scores(rng, 10, 40, False), _scores(rng, 10, 40, False)
    out, mask = cr.combine(e, a, [17, 40], 1.5, 0.5, 0.0, rows_per=5, ld_out=44)
    assert out.shape == mask.shape == (10, 44)
    assert np.all(out[:5, 17:] == 0) and np.all(out[:, 40:] == 0) and np.any(out[5:, 17:40] > 0) and not mask[:, 40:].any()
    short, _ = cr.combine(e[:5, :17], a[:5, :17], [17] * 5, 1.5, 0.5, 0.0)
    np.testing.assert_array_equal(out[:5, :17].view(np.int32), short.view(np.int32))


def test_head_margin_is_the_distance_to_the_threshold():
    e = np.array([[0.5, 0.05 * (1 + 1e-6), 0.01, 0.2, 0.0, 0.0, 0.9, 0.0]], np.float32)
    _, mask, margin = cr.combine(e, e, [8], 1.5, 0.5, 0.1, return_margin=True)
    assert mask[0].tolist() == [True, True, False, True, False, False, False, False]
    assert abs(margin[0] - math.log(float(e[0, 1]) / 0.05)) < 1e-7 and margin[0] < 1e-5
    _, _, margin = cr.combine(e, e, [8], 1.5, 0.5, 0.0, return_margin=True)       # α = 0: no threshold to be near
    assert margin[0] == np.inf


def test_hand_computed_example():
    """2 × 6, probability mode, UNK = column 2, we = 1.5, wa = 0.5, α = 0.5; every entry a power of two, so the scores are multiples of
    ln 2 / 2.  Row 0: top 0.5, head {0, 1, 5} (0.25 = α·top is inside); s = 1.5·ln p_e − 0.5·max(ln p_a, L0):
    column 0: 1.5·(−ln 2) − 0.5·(−2 ln 2) = −0.5 ln 2; column 1: 1.5·(−2 ln 2) − 0.5·(−ln 2) = −2.5 ln 2;
    column 5 (amateur 0 → the floor 1e-30): −3 ln 2 − 0.5·L0 → weight 2^−3·1e15.
    Row 1: top 0.5, head {1, 3}: column 1: −0.5 ln 2, column 3: 1.5·(−2 ln 2) − 0.5·(−2 ln 2) = −2 ln 2."""
    e = np.array([[0.5, 0.25, 1.0, 0.125, 0.0, 0.25], [0.0, 0.5, 0.0, 0.25, 0.125, 0.125]], np.float32)
    a = np.array([[0.25, 0.5, 0.5, 0.125, 0.25, 0.0], [0.5, 0.25, 0.5, 0.25, 0.5, 0.0]], np.float32)
    out, mask = cr.combine(e, a, [6, 6], 1.5, 0.5, 0.5, False, unk=2)
    assert mask.tolist() == [[True, True, False, False, False, True], [False, True, False, True, False, False]]
    u0 = np.array([2 ** -0.5, 2 ** -2.5, 0, 0, 0, 2 ** -3 * 1e15])
    u1 = np.array([0, 2 ** -0.5, 0, 2 ** -2.0, 0, 0])
    np.testing.assert_allclose(out[0], u0 / u0.sum(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(out[1], u1 / u1.sum(), rtol=1e-6, atol=0)
    assert out[0, 5] == 1.0 and 0 < out[0, 0] < 1e-14              # the floored column takes the row


# ------------------------------------------------------------------------------------------------ the binding's refusals
def test_header_declares_the_entry_point_and_the_library_exports_it():
    ret, args = _lib.declarations()["svpc_contrast_combine"]
    assert len(args) == 17
    lib = _lib.load()
    assert lib.svpc_abi_version() == 2
    assert hasattr(lib, "svpc_contrast_combine") and hasattr(lib, "svpc_ensemble_combine")


def test_contrast_combine_fails_loudly_on_cpu_tensors():
    with pytest.raises(_lib.SvpcKernelError):
        ops.contrast_combine(torch.rand(4, 12), torch.rand(4, 12), [12] * 4, expert_weight=1.5, amateur_weight=0.5, alpha=0.1,
                             logits=False, unk=UNK)


@pytest.mark.parametrize("bad", ["dtype", "dim", "stride", "rows", "device", "rows_per", "row_c", "cols", "cols_amateur", "we_zero",
                                 "we_negative", "we_inf", "we_nan", "wa_negative", "wa_inf", "wa_nan", "alpha_negative", "alpha_above",
                                 "alpha_nan", "not_a_tensor"])
def test_contrast_combine_value_errors(bad):
    e, a = torch.rand(4, 12), torch.rand(4, 12)
    kw = dict(expert_weight=1.5, amateur_weight=0.5, alpha=0.1, logits=False, unk=UNK)
    row_c = [12] * 4
    if bad == "dtype":
        a = a.double()
    elif bad == "dim":
        e = e.view(-1)
    elif bad == "stride":
        a = torch.rand(12, 4).t()
    elif bad == "rows":
        a = torch.rand(5, 12)
    elif bad == "device":
        a = torch.empty(4, 12, device="meta")
    elif bad == "rows_per":
        kw["rows_per"] = 0
    elif bad == "row_c":
        row_c = [12] * 3
    elif bad == "cols":
        row_c = [13] * 4
    elif bad == "cols_amateur":
        a = torch.rand(4, 11)
    elif bad == "not_a_tensor":
        a = None
    elif bad.startswith("we_"):
        kw["expert_weight"] = {"zero": 0.0, "negative": -1.0, "inf": math.inf, "nan": math.nan}[bad[3:]]
    elif bad.startswith("wa_"):
        kw["amateur_weight"] = {"negative": -0.5, "inf": math.inf, "nan": math.nan}[bad[3:]]
    elif bad.startswith("alpha_"):
        kw["alpha"] = {"negative": -0.1, "above": 1.5, "nan": math.nan}[bad[6:]]
    with pytest.raises(ValueError):
        ops.contrast_combine(e, a, row_c, **kw)


def test_coefficients_as_the_kernel_takes_them():
    assert ops.contrast_coefficients(1.5, 0.5, 0.1) == (1.5, 0.5, 0.1, math.log(0.1))
    assert ops.contrast_coefficients(1, 0, 0) == (1.0, 0.0, 0.0, -math.inf)
    assert ops.contrast_coefficients(2, 1, 1)[3] == 0.0


# ------------------------------------------------------------------------------------------------ the translator's refusals
@pytest.fixture(scope="module")
def tiny(golden_dir):
    _, cfg, batch, model = build_model("tiny", "vivt", golden_dir, "cpu")
    return cfg, model


def _ck(cfg, model):
    return {"model_cfg": cfg, "model": model.state_dict()}


def test_contrast_translator_is_an_ensemble_of_two(tiny):
    cfg, model = tiny
    other = copy.deepcopy(model)
    tr = ContrastTranslator(O(), _ck(cfg, model), model, _ck(cfg, other), other)
    assert isinstance(tr, EnsembleTranslator) and isinstance(tr, Translator)
    assert tr.model is model and tr._members() == [model, other] and tr.separate_amateur
    assert (tr.beta, tr.alpha, tr.expert_weight, tr.amateur_weight) == (0.5, 0.1, 1.5, 0.5)
    assert tr.incremental and not tr.two_streams and not tr.graph
    with pytest.raises(ValueError, match="two_streams"):
        tr.two_streams = True
    with pytest.raises(NotImplementedError, match="not offered for an ensemble"):
        tr.translate_batch_contrastive(None)
    with pytest.raises(TypeError):
        ContrastTranslator(O(), _ck(cfg, model), model, _ck(cfg, other), other, incremental=False)
    li = ContrastTranslator(O(), _ck(cfg, model), model, _ck(cfg, other), other, beta=1, expert_weight=1, alpha=0)       # Li et al.
    assert (li.expert_weight, li.amateur_weight, li.alpha) == (1.0, 1.0, 0.0)


def test_the_expert_as_its_own_amateur(tiny):
    cfg, model = tiny
    tr = ContrastTranslator(O(), _ck(cfg, model), model, amateur_video="zero", beta=1.0)
    assert tr._members() == [model, model] and not tr.separate_amateur and tr.expert_weight == 2.0
    feats = torch.rand(6, 5)
    assert tr._member_features(0, feats) is feats
    z = tr._member_features(1, feats)
    assert z.shape == feats.shape and z.dtype == feats.dtype and not z.any() and tr._member_features(1, torch.rand(6, 5)) is z
    assert tr._member_features(1, torch.rand(7, 5)) is not z       # one cached buffer per shape
    seen = []

    def noisy(f):
        seen.append(f)
        return f + 1.0
    tr = ContrastTranslator(O(), _ck(cfg, model), model, amateur_features=noisy)
    assert torch.equal(tr._member_features(1, feats), feats + 1.0) and seen[0] is feats and tr._member_features(0, feats) is feats
    tr = ContrastTranslator(O(), _ck(cfg, model), model, amateur_video="zero", amateur_features=noisy)     # the callable sees the zeros
    assert torch.equal(tr._member_features(1, feats), torch.ones_like(feats))


@pytest.mark.parametrize("field", AGREE)
def test_the_amateur_must_agree_with_the_expert(tiny, field):
    cfg, model = tiny
    other_cfg = copy.copy(cfg)
    v = getattr(cfg, field)
    setattr(other_cfg, field, "video" if field == "model_mode" else v + 1)
    other = copy.deepcopy(model)
    with pytest.raises(ValueError, match=field):
        ContrastTranslator(O(), _ck(cfg, model), model, _ck(other_cfg, other), other)


@pytest.mark.parametrize("bad", ["checkpoint_only", "model_only", "same_video", "amateur_video", "features", "beta_negative", "beta_nan",
                                 "beta_inf", "beta_none", "alpha_negative", "alpha_above", "alpha_nan", "expert_weight_zero",
                                 "expert_weight_negative", "expert_weight_nan", "device"])
def test_contrast_translator_value_errors(tiny, bad):
    cfg, model = tiny
    other = copy.deepcopy(model)
    args, kw = [_ck(cfg, model), model, _ck(cfg, other), other], {}
    if bad == "checkpoint_only":
        args[3] = None
    elif bad == "model_only":
        args[2] = None
    elif bad == "same_video":                                      # no separate amateur, no degraded view: identical distributions
        args = args[:2]
    elif bad == "amateur_video":
        kw["amateur_video"] = "blur"
    elif bad == "features":
        kw["amateur_features"] = 0.5
    elif bad.startswith("beta_"):
        kw["beta"] = {"negative": -0.5, "nan": math.nan, "inf": math.inf, "none": None}[bad[5:]]
    elif bad.startswith("alpha_"):
        kw["alpha"] = {"negative": -0.1, "above": 1.01, "nan": math.nan}[bad[6:]]
    elif bad.startswith("expert_weight_"):
        kw["expert_weight"] = {"zero": 0.0, "negative": -1.0, "nan": math.nan}[bad[14:]]
    elif bad == "device":
        args[3] = other.to("meta")
    with pytest.raises(ValueError):
        ContrastTranslator(O(), *args, **kw)
