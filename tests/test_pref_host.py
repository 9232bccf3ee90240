"""Preference optimisation without a GPU: the restatement (tests/pref_reference.py) against torch float64 autograd of the
written objective, hand-built videos with known pairs (the ln 2 case among them), the exactly-zero cases, every host check, no CPU
fallback, the argument rules of ``PreferenceOptimization.step`` that need no device, the exported symbol, and the conditions on the fixed
inputs the GPU tests run on."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pref_cases as pc  # noqa: E402
import pref_reference as pr  # noqa: E402
import scst_reference as sr  # noqa: E402
from svpc_amd import _lib, mrt, ops, prefopt  # noqa: E402
from svpc_amd.synthetic import UNK  # noqa: E402

f32 = np.float32
LN2 = math.log(2.0)


def _one_video(cum, cost, ref=None, length=None, w=None, beta=1.0, gamma=0.0, eps=0.0, lb=0.0, rho=1.0, kind="sigmoid", pairs="all"):
    cum = np.asarray(cum, f32).reshape(1, -1)
    K = cum.shape[1]
    length = np.full((1, K), 2) if length is None else np.asarray(length).reshape(1, K)
    ref = None if ref is None else np.asarray(ref, f32).reshape(1, K)
    return pr.groups(cum, length, np.zeros((1, K), np.int32), [cost], [0, 1], w, ref, beta, gamma, eps, lb, rho, kind, pairs)


# ------------------------------------------------------------------------------------------------ the restatement alone
def test_hand_built_videos():
    # DPO, K = 2: cum = (−1, −3), ref = (−2, −2): u = (1, −1); candidate 0 is preferred: d = 2, β = 1/2: h = 1, ℓ = ln(1 + e⁻¹)
    r = _one_video([-1.0, -3.0], [0.0, 1.0], ref=[-2.0, -2.0], beta=0.5)
    assert r["u"].tolist() == [[1.0, -1.0]] and r["reward"].tolist() == [[0.5, -0.5]] and r["pos"].tolist() == [[0, 1]]
    assert r["pair"][0].tolist() == [[False, True], [False, False]] and r["n_pairs"][0] == 1 and r["n_correct"][0] == 1
    assert r["pref"][0] == pytest.approx(math.log1p(math.exp(-1.0)), rel=1e-15) and r["margin"][0] == 1.0
    D = -0.5 / (1.0 + math.e)                                              # β·(−σ(−1))
    assert r["G"][0] == pytest.approx([D, -D], rel=1e-14) and r["w_eff64"][0] == pytest.approx([-D, D], rel=1e-14)
    assert r["loss"] == f32(math.log1p(math.exp(-1.0))) and r["loss"].dtype == np.float32
    # the other preference: candidate 1 is preferred, d = −2: not correct, ℓ = ln(1 + e)
    r = _one_video([-1.0, -3.0], [1.0, 0.0], ref=[-2.0, -2.0], beta=0.5)
    assert r["pair"][0].tolist() == [[False, False], [True, False]] and r["n_correct"][0] == 0 and r["margin"][0] == -1.0
    assert r["pref"][0] == pytest.approx(math.log1p(math.e), rel=1e-15)
    # the reference equal to the policy: u = 0, pref = ln 2, nothing counted as correct, D = −β/2
    r = _one_video([-1.0, -3.0, -2.0], [0.3, 0.1, 0.2], ref=[-1.0, -3.0, -2.0], beta=0.1)
    assert not r["u"].any() and r["n_pairs"][0] == 3 and r["n_correct"][0] == 0 and r["margin"][0] == 0
    assert r["pref"][0] == pytest.approx(LN2, rel=1e-15)
    assert r["G"][0] == pytest.approx([0.1 / 3.0, -0.1 / 3.0, 0.0], abs=1e-17)      # the order is 1, 2, 0; the middle one: one pair as i, one as j
    # cDPO: ε moves ℓ and D; at h = 0 ℓ stays ln 2 and D = β(ε − 1/2)·… = −β(1 − 2ε)/2
    r = _one_video([-1.0, -3.0], [0.0, 1.0], ref=[-1.0, -3.0], beta=2.0, eps=0.1)
    assert r["pref"][0] == pytest.approx(LN2, rel=1e-15) and r["G"][0] == pytest.approx([-0.8, 0.8], rel=1e-14)
    # SimPO: no reference, β = 2, γ = 1/2, length-normalised: n = (2, 4): u = (−0.5, −0.75), h = 0
    r = _one_video([-1.0, -3.0], [0.0, 1.0], length=[2, 4], beta=2.0, gamma=0.5, lb=1.0)
    assert r["u"].tolist() == [[-0.5, -0.75]] and r["h"][0, 0, 1] == 0.0 and r["pref"][0] == pytest.approx(LN2, rel=1e-15)
    assert r["w_eff64"][0] == pytest.approx([0.5, -0.25], rel=1e-14)        # G = ∓1 spread over n = 2 and 4 words
    # hinge: h = β·d − γ = 2·0.25 − 0.5 = 0, ℓ = 1, D = −β; a pair far on the right side is idle
    r = _one_video([-1.0, -3.0], [0.0, 1.0], length=[2, 4], beta=2.0, gamma=0.5, lb=1.0, kind="hinge")
    assert r["pref"][0] == 1.0 and r["G"].tolist() == [[-2.0, 2.0]]
    r = _one_video([-1.0, -9.0], [0.0, 1.0], beta=2.0, kind="hinge")
    assert r["pref"][0] == 0.0 and not r["G"].any() and r["n_correct"][0] == 1 and r["loss"] == 0
    # ipo: d = 2, β = 1/2: (2 − 1)² = 1, D = 2
    r = _one_video([-1.0, -3.0], [0.0, 1.0], ref=[-2.0, -2.0], beta=0.5, kind="ipo")
    assert r["pref"][0] == 1.0 and r["G"].tolist() == [[2.0, -2.0]]
    # extremes: of four candidates only best against worst; a tie (1, 2) forms no pair under "all"
    r = _one_video([-1.0, -2.0, -3.0, -4.0], [0.5, 0.2, 0.2, 0.9], pairs="extremes")
    assert r["pos"].tolist() == [[2, 0, 1, 3]] and r["n_pairs"][0] == 1 and r["pair"][0, 1, 3]
    r = _one_video([-1.0, -2.0, -3.0, -4.0], [0.5, 0.2, 0.2, 0.9])
    assert r["n_pairs"][0] == 5 and not r["pair"][0, 1, 2] and not r["pair"][0, 2, 1]
    # invalid candidates: a reference-barred one and a nan cost stand in no pair; with likelihood weights: −Σ w·cum joins the loss
    r = _one_video([-1.0, -2.0, -3.0, -4.0], [0.5, float("nan"), 0.2, 0.9], ref=[-1.0, -1.0, -float("inf"), -1.0], w=np.full((1, 4), 0.5, f32))
    assert r["valid"].tolist() == [[1, 0, 0, 1]] and r["n_pairs"][0] == 1 and r["u"][0, 1] == 0 and r["u"][0, 2] == 0
    assert r["G"][0, 1] == 0 and r["G"][0, 2] == 0 and float(r["total"]) == pytest.approx(5.0 + r["pref"][0], rel=1e-15)


CASES = [(11, [3, 1, 2, 2], 4), (12, [1], 1), (13, [2, 0, 3], 3), (14, [20], 16), (15, [2] * 9, 2)]
SETTINGS = [(True, 0.1, 0.0, 0.0, 0.0, 1.0, "sigmoid", "all"), (True, 2.0, 0.0, 0.1, 0.0, 0.7, "sigmoid", "extremes"),
            (False, 2.0, 0.5, 0.0, 1.0, 1.0, "sigmoid", "all"), (True, 0.1, 0.5, 0.0, 1.0, 2.0, "hinge", "all"),
            (True, 0.5, 0.0, 0.0, 0.0, 1.0, "ipo", "all"), (False, 50.0, 0.0, 0.0, 0.0, 1.0, "sigmoid", "all")]


@pytest.mark.parametrize("with_ref,beta,gamma,eps,lb,rho,kind,pairs", SETTINGS)
@pytest.mark.parametrize("seed,steps,K", CASES)
def test_restatement_against_autograd(seed, steps, K, with_ref, beta, gamma, eps, lb, rho, kind, pairs):
    """a cost tie, a barred candidate, a reference-barred candidate, a non-finite cost and a video with no valid candidate are all in
    ``group_case``"""
    c = pc.group_case(seed, steps, K)
    ref = c["ref_cum"] if with_ref else None
    r = pr.groups(c["cum"], c["length"], c["barred"], c["cost"], c["vid_off"], c["w"], ref, beta, gamma, eps, lb, rho, kind, pairs)
    if seed == 11:
        assert not r["valid"][-1].any() and r["pref"][-1] == 0 and r["n_pairs"][-1] == 0                 # no valid candidate
        assert not r["valid"][0, 1] and not r["valid"][1, K - 1] and not r["valid"][2, 0]               # barred; +inf; nan
        assert bool(r["valid"][0, K - 2]) == (not with_ref)                                              # the reference-barred candidate
        assert r["valid"][1, 0] and r["valid"][1, 1] and not r["pair"][1, 0, 1] and not r["pair"][1, 1, 0]   # the tie forms no pair
    assert not r["G"][r["valid"] == 0].any() and not r["u"][r["valid"] == 0].any()
    assert (r["n_pairs"] <= 1).all() or pairs == "all"
    assert all(abs(r["G"][b].sum()) <= 1e-14 * (1.0 + np.abs(r["G"][b]).max()) for b in range(len(steps)))      # every D enters once as i, once as j
    cum = torch.tensor(np.where(np.isfinite(c["cum"]), c["cum"], 0.0).astype(np.float64), requires_grad=True)
    total = pr.objective_torch(cum, c["length"], c["barred"], c["cost"], c["vid_off"], c["w"], ref, beta, gamma, eps, lb, rho, kind, pairs)
    total.backward()
    tot = float(total.detach())
    assert abs(tot - float(r["total"])) <= 1e-12 * max(1.0, abs(tot))
    g = cum.grad.numpy()
    live = c["barred"] == 0
    scale = 1.0 + np.abs(r["G"]).max()
    assert np.abs(g[live] + r["w_eff64"][live]).max() <= 1e-13 * scale                                  # ∂loss / ∂cum = −w_eff
    assert not g[~live].any()                                               # a barred caption takes no part (seq_nll's backward zeroes its rows)


def _nll(c):
    """−Σ w·cum over the captions that are not barred, ``scst_reference.seq_nll``'s sum"""
    total = np.float64(0.0)
    for w, cu, b in zip(c["w"].reshape(-1), c["cum"].reshape(-1), c["barred"].reshape(-1)):
        if not b:
            total += np.float64(w) * np.float64(cu)
    return np.float32(-total)


def test_exact_identities():
    """ρ = 0, K = 1 and equal costs: G is exactly 0 (w_eff is w, bit for bit); an absent reference is an all-zero one; the reference equal to
    the policy gives u = 0, pref = ln 2 in every video with a pair and nothing counted correct"""
    for seed, steps, K in CASES:
        c = pc.group_case(seed, steps, K)
        args = (c["cum"], c["length"], c["barred"])
        r = pr.groups(*args, c["cost"], c["vid_off"], c["w"], c["ref_cum"], 2.0, 0.5, 0.1, 1.0, 0.0, "sigmoid", "all")          # ρ = 0
        assert not r["G"].any() and np.array_equal(r["w_eff"].view(np.int32), c["w"].view(np.int32))
        assert r["loss"].view(np.int32) == _nll(c).view(np.int32)
        flat = np.where(np.isfinite(c["cost"]), -1.25, c["cost"])
        r = pr.groups(*args, flat, c["vid_off"], c["w"], c["ref_cum"], 2.0, 0.0, 0.0, 1.0, 3.0, "ipo", "all")                  # equal costs
        assert not r["G"].any() and not r["pair"].any() and not r["pref"].any() and not r["n_pairs"].any()
        assert np.array_equal(r["w_eff"].view(np.int32), c["w"].view(np.int32))
        if K == 1:
            r = pr.groups(*args, c["cost"], c["vid_off"], c["w"], c["ref_cum"], 2.0, 0.5, 0.0, 1.0, 3.0, "hinge", "all")
            assert not r["G"].any() and not r["n_pairs"].any() and np.array_equal(r["w_eff"].view(np.int32), c["w"].view(np.int32))
        a = pr.groups(*args, c["cost"], c["vid_off"], c["w"], None, 2.0, 0.5, 0.1, 1.0, 1.0, "sigmoid", "all")
        z = pr.groups(*args, c["cost"], c["vid_off"], c["w"], np.zeros_like(c["cum"]), 2.0, 0.5, 0.1, 1.0, 1.0, "sigmoid", "all")
        for k in ("pref", "reward", "margin", "w_eff64", "total"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(z[k])), k
        own = np.where(c["barred"] == 1, f32(-1.0), c["cum"]).astype(f32)       # (a barred caption's own cum is −inf: the candidate is invalid anyway)
        r = pr.groups(*args, c["cost"], c["vid_off"], None, own, 0.1, 0.0, 0.0, 0.0, 1.0, "sigmoid", "all")
        assert not r["u"].any() and not r["n_correct"].any()
        assert all(r["pref"][b] == pytest.approx(LN2, rel=1e-15) for b in range(len(steps)) if r["n_pairs"][b])
        assert K == 1 or r["n_pairs"].any()


def test_fixed_gpu_inputs_meet_their_conditions():
    """conditions on the seeded kernel-level inputs, asserted on the restatement alone, fed the restatement's own cum — every case of
    ``pref_cases.KERNEL_CASES``, none left out: no hinge argument 1 − h lies within 1e-9 of 0 and no d within 1e-9 of 0 (the active set or
    ``n_correct`` could flip), every pref[b] (of a video with a pair) of the hinge and ipo cases is at least 1e-3·(β·max|u| + 1)
    (``pref_reference.pref_conditioning``), and the special rows and videos are what the case builders say"""
    seen = dict(active=False, idle=False, correct=False, wrong=False, refbar=False, large=False)
    for seed, C, Lt, K, steps, logits, wide, with_ref, lb, beta, gamma, eps, kind, pairs in pc.KERNEL_CASES:
        c = pc.score_case(seed, C, Lt, K, steps, logits, wide)
        nl = sr.seq_nll(c["scores"][:, :C], c["ids"], c["row_c"], c["w"], logits)
        assert sorted(np.nonzero(nl["barred"])[0].tolist()) == sorted(c["bar_rows"])
        ref = c["ref_cum"] if with_ref else None
        r = pr.groups(nl["cum"], nl["len"], nl["barred"], c["cost"], c["vid_off"], c["w"], ref, beta, gamma, eps, lb, 1.0, kind, pairs)
        assert pr.min_d_distance(r) > pc.D_MARGIN, (seed, pr.min_d_distance(r))
        if kind == "hinge":
            assert pr.min_hinge_distance(r) > pc.HINGE_MARGIN, (seed, pr.min_hinge_distance(r))
            h = r["h"][r["pair"]]
            seen["active"] |= bool((h < 1).any())
            seen["idle"] |= bool((h > 1).any())
        if kind in ("hinge", "ipo"):
            assert pr.pref_conditioning(r, beta) >= pc.PREF_CONDITION, (seed, pr.pref_conditioning(r, beta))
        d = r["d"][r["pair"]]
        seen["correct"] |= bool((d > 0).any())
        seen["wrong"] |= bool((d < 0).any())
        seen["large"] |= bool(d.size and beta == 50.0 and kind == "sigmoid" and (np.abs(beta * d) > 300).any())
        K_, N = K, len(steps)
        assert K_ == 1 or r["n_pairs"].any(), seed
        if N >= 2 and steps[-1]:
            assert not r["valid"][-1].any()
        if with_ref:
            for row in c["ref_bar_rows"]:
                t, k = divmod(row, K)
                b = int(np.searchsorted(np.asarray(c["vid_off"]), t, side="right")) - 1
                assert not r["valid"][b, k] and np.isfinite(c["cost"][b, k]) and not nl["barred"].reshape(-1, K)[t, k]
                seen["refbar"] = True
    assert all(seen.values()), seen


# ------------------------------------------------------------------------------------------------ the host checks
def test_every_value_error():
    cost = torch.zeros(3, 4, dtype=torch.float64)
    for k in (0, 17, -1, 2.0, True):
        with pytest.raises(ValueError):
            ops.check_pref(k=k)
    assert ops.check_pref(k=16)[0] == 16 and ops.check_pref(k=1)[0] == 1
    for bad in (cost.float(), cost[0], torch.zeros(3, 17, dtype=torch.float64), torch.zeros(3, 0, dtype=torch.float64), cost.tolist()):
        with pytest.raises(ValueError):
            ops.check_pref(cost=bad)
    for off, T in (([1, 2, 3, 4], 4), ([0, 2, 1, 4], 4), ([0, 5], 4), ([], 0)):
        with pytest.raises(ValueError):
            ops.check_pref(vid_off=off, n_sent=T)
    for v in (0.0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError):
            ops.check_pref(beta=v)
    for name in ("gamma", "length_beta", "pref_weight"):
        for v in (-1e-9, float("nan"), float("inf"), "1", True):
            with pytest.raises(ValueError):
                ops.check_pref(**{name: v})
        ops.check_pref(**{name: 0.0})
    for v in (-1e-9, 0.5, 1.0, float("nan"), "0.1", True):
        with pytest.raises(ValueError):
            ops.check_pref(label_smoothing=v)
    ops.check_pref(label_smoothing=0.49, loss_type="sigmoid")
    for kw in (dict(label_smoothing=0.1, loss_type="hinge"), dict(label_smoothing=0.1, loss_type="ipo"), dict(gamma=0.5, loss_type="ipo"),
               dict(loss_type="dpo"), dict(loss_type=0), dict(pairs="best"), dict(pairs=1), dict(source="greedy"), dict(utility="METEOR")):
        with pytest.raises(ValueError):
            ops.check_pref(**kw)
    ops.check_pref(gamma=0.5, loss_type="hinge")
    ref = torch.zeros(12, dtype=torch.float32)
    for bad, rows in ((ref.double(), 12), (ref[::2], 6), (ref.tolist(), 12)):
        with pytest.raises(ValueError):
            ops.check_pref(ref_cum=bad, rows=rows)
    with pytest.raises(ValueError):
        ops.check_pref(ref_cum=ref, rows=11)
    with pytest.raises(ValueError):
        ops.check_pref(ref_cum=ref, rows=12, device=torch.device("cuda:0"))
    assert ops.PREF_LOSS_TYPES == ("sigmoid", "hinge", "ipo") and ops.PREF_PAIRS == ("all", "extremes")
    assert ops.check_pref(k=4, source="stochastic", utility="CIDEr", loss_type="ipo", pairs="extremes") == (4, None, 5, 2, 1)


def test_no_cpu_fallback():
    with pytest.raises(_lib.SvpcKernelError):
        ops.check_pref(cost=torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(_lib.SvpcKernelError):
        ops.check_pref(ref_cum=torch.zeros(12, dtype=torch.float32), rows=12)
    R, Lt, C, K = 4, 3, 9, 2
    with pytest.raises(_lib.SvpcKernelError):
        ops.seq_pref(torch.rand(R * Lt, C), [C] * R, torch.zeros(R, Lt, dtype=torch.int32), torch.ones(R, dtype=torch.int32),
                     torch.zeros(1, K, dtype=torch.float64), [0, 2], None, None, False, UNK, 0.1, 0.0, 0.0, 0.0, 1.0, "sigmoid", "all")
    with pytest.raises(_lib.SvpcKernelError):
        prefopt.preference_loss(None, None, None, torch.zeros(1, K, dtype=torch.float64))


def test_step_argument_rules_without_a_device():
    model = torch.nn.Linear(1, 1)
    tr = SimpleNamespace(model=model)
    po = prefopt.PreferenceOptimization(tr, None, reference=tr)
    assert po.reference is tr and po.phase_events is None and isinstance(po, mrt.MinimumRisk)
    bad = [dict(source="greedy"), dict(utility="METEOR"), dict(num_candidates=17), dict(num_candidates=16, include_gold=True, input_labels_list=[]),
           dict(include_gold=True), dict(beta=0.0), dict(beta=-1.0), dict(gamma=-1.0), dict(label_smoothing=0.5), dict(loss_type="dpo"),
           dict(pairs="best"), dict(loss_type="hinge", label_smoothing=0.1), dict(loss_type="ipo", gamma=0.5), dict(pref_weight=-1.0),
           dict(length_beta=float("nan"))]
    model.eval()
    for kw in bad:
        with pytest.raises(ValueError):
            po.step(None, None, **kw)
    # the policy as its own reference must be in eval mode: in training mode the reference would see dropout
    model.train()
    with pytest.raises(ValueError, match="dropout"):
        po.step(None, None)
    assert model.training


def test_symbol_is_declared_and_exported():
    decls = _lib.declarations()
    assert "svpc_seq_pref_fwd" in decls and len(decls["svpc_seq_pref_fwd"][1]) == 35
    lib = _lib.load()
    assert hasattr(lib, "svpc_seq_pref_fwd") and lib.svpc_abi_version() == 2
    text = open(_lib.HEADER_PATH).read()
    assert "svpc_seq_pref_fwd" in text and "DESIGN 11.21" in text
