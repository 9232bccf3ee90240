"""Minimum-risk and ranking training without a GPU: the restatement (tests/risk_reference.py) against torch float64
autograd of the written objective, the exactly-zero cases, a literal hand-computed anchor, every host check, no CPU fallback, the exported
symbol, and the margins of the fixed inputs the GPU tests run on."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import risk_cases as rc  # noqa: E402
import risk_reference as rr  # noqa: E402
import scst_reference as sr  # noqa: E402
from svpc_amd import _lib, ops  # noqa: E402
from svpc_amd.synthetic import UNK  # noqa: E402

f32 = np.float32


# ------------------------------------------------------------------------------------------------ the restatement alone
def test_anchor():
    """one video, one sentence, K = 2: cum = (−1, −2), cost = (4, 1), α = ln 2, β = 0, λ = 1/4.  Q = (2/3, 1/3), risk = 3; the one pair is
    (i, j) = (1, 0) with h = 1 + λ = 5/4: active, rank = 5/4; G = ±(ρ_risk·ln 2·2/3 + ρ_rank)"""
    a = math.log(2.0)
    cum, ln, bar = np.array([[-1.0, -2.0]], f32), np.array([[2, 2]]), np.zeros((1, 2), np.int32)
    r = rr.groups(cum, ln, bar, [[4.0, 1.0]], [0, 1], None, a, 0.0, 0.25, 1.0, 2.0)
    assert r["valid"].tolist() == [[1, 1]] and r["pos"].tolist() == [[1, 0]]
    assert r["Q"][0] == pytest.approx([2.0 / 3.0, 1.0 / 3.0], rel=1e-15) and r["risk"][0] == pytest.approx(3.0, rel=1e-15)
    assert r["z"].tolist() == [[-1.0, -2.0]]
    assert r["pair"][0].tolist() == [[False, False], [True, False]] and r["active"][0].tolist() == [[False, False], [True, False]]
    assert r["hinge"][0, 1, 0] == 1.25 and r["rank"][0] == 1.25
    g = a * 2.0 / 3.0 + 2.0
    assert r["G"][0] == pytest.approx([g, -g], rel=1e-14)
    assert r["loss"] == f32(3.0 + 2.0 * 1.25) and r["loss"].dtype == np.float32
    np.testing.assert_array_equal(r["w_eff"], np.array([[-g, g]]).astype(f32))
    # with likelihood weights: −Σ w·cum = 0.5 + 0.5
    r = rr.groups(cum, ln, bar, [[4.0, 1.0]], [0, 1], np.array([[0.5, 0.25]], f32), a, 0.0, 0.25, 1.0, 2.0)
    assert r["loss"] == f32(6.5) and r["w_eff64"][0] == pytest.approx([0.5 - g, 0.25 + g], rel=1e-14)
    # length normalisation: n = 2, β = 1 halves z and the gradient; a larger margin than the gap still counts the position distance
    r = rr.groups(cum, ln, bar, [[4.0, 1.0]], [0, 1], None, 0.0, 1.0, 0.25, 1.0, 2.0)
    assert r["z"].tolist() == [[-0.5, -1.0]] and r["Q"].tolist() == [[0.5, 0.5]] and r["rank"][0] == 0.75
    assert r["G"].tolist() == [[2.0, -2.0]] and r["w_eff64"].tolist() == [[-1.0, 1.0]]
    # the worse candidate scored lower by more than the margin: the pair is not active
    r = rr.groups(np.array([[-5.0, -1.0]], f32), ln, bar, [[4.0, 1.0]], [0, 1], None, 0.0, 0.0, 0.25, 0.0, 1.0)
    assert r["hinge"][0, 1, 0] == -3.75 and not r["active"].any() and r["rank"][0] == 0 and not r["G"].any() and r["loss"] == 0


CASES = [(11, [3, 1, 2, 2], 4), (12, [1], 1), (13, [2, 0, 3], 3), (14, [20], 16), (15, [2] * 9, 2)]


@pytest.mark.parametrize("alpha,beta,margin,rho", [(5e-3, 0.0, 1e-3, (1.0, 0.0)), (2.0, 0.6, 0.5, (1.0, 2.0)), (0.7, 1.0, 0.05, (0.0, 1.0)),
                                                    (0.3, 0.6, 0.0, (0.5, 0.5))])
@pytest.mark.parametrize("seed,steps,K", CASES)
def test_restatement_against_autograd(seed, steps, K, alpha, beta, margin, rho):
    """a cost tie, a barred (invalid) candidate, a non-finite cost and a video with no valid candidate are all in ``group_case``"""
    c = rc.group_case(seed, steps, K)
    r = rr.groups(c["cum"], c["length"], c["barred"], c["cost"], c["vid_off"], c["w"], alpha, beta, margin, *rho)
    N = len(steps)
    if seed == 11:
        assert not r["valid"][-1].any() and r["risk"][-1] == 0 and r["rank"][-1] == 0                  # no valid candidate
        assert not r["valid"][0, 1] and not r["valid"][1, K - 1] and not r["valid"][2, 0]               # barred; +inf; nan
        assert r["valid"][1, 0] and r["valid"][1, 1] and c["cost"][1, 0] == c["cost"][1, 1]              # the tie …
        assert not r["pair"][1, 0, 1] and not r["pair"][1, 1, 0] and r["pos"][1, 1] == r["pos"][1, 0] + 1   # … forms no pair
    assert not r["Q"][r["valid"] == 0].any() and not r["G"][r["valid"] == 0].any()
    assert all(abs(r["Q"][b].sum() - 1.0) < 1e-14 for b in range(N) if r["valid"][b].any())
    cum = torch.tensor(np.where(np.isfinite(c["cum"]), c["cum"], 0.0).astype(np.float64), requires_grad=True)
    total = rr.objective_torch(cum, c["length"], c["barred"], c["cost"], c["vid_off"], c["w"], alpha, beta, margin, *rho)
    total.backward()
    tot = float(total.detach())
    assert abs(tot - float(r["total"])) <= 1e-12 * max(1.0, abs(tot))
    g = cum.grad.numpy()
    live = c["barred"] == 0
    scale = 1.0 + np.abs(r["G"]).max()
    assert np.abs(g[live] + r["w_eff64"][live]).max() <= 1e-13 * scale                                  # ∂loss / ∂cum = −w_eff
    assert not g[~live].any()                                               # a barred caption takes no part (seq_nll's backward zeroes its rows)


def test_exact_zero_cases():
    """K = 1, α = 0 and equal costs: G is exactly 0 (w_eff is w, bit for bit); without the weights the group terms vanish from the loss"""
    for seed, steps, K in CASES:
        c = rc.group_case(seed, steps, K)
        nll = sr_loss(c)
        r = rr.groups(c["cum"], c["length"], c["barred"], c["cost"], c["vid_off"], c["w"], 0.0, 0.6, 0.5, 1.0, 0.0)           # α = 0
        assert not r["G"].any() and np.array_equal(r["w_eff"].view(np.int32), c["w"].view(np.int32))
        flat = np.where(np.isfinite(c["cost"]), -1.25, c["cost"])
        r = rr.groups(c["cum"], c["length"], c["barred"], flat, c["vid_off"], c["w"], 2.0, 0.6, 0.5, 1.0, 3.0)               # equal costs
        assert not r["G"].any() and not r["pair"].any() and not r["rank"].any()
        assert np.array_equal(r["w_eff"].view(np.int32), c["w"].view(np.int32))
        r = rr.groups(c["cum"], c["length"], c["barred"], c["cost"], c["vid_off"], c["w"], 2.0, 0.6, 0.5, 0.0, 0.0)           # no weights
        assert not r["G"].any() and r["loss"].view(np.int32) == nll.view(np.int32)
        if K == 1:
            r = rr.groups(c["cum"], c["length"], c["barred"], c["cost"], c["vid_off"], c["w"], 2.0, 0.6, 0.5, 1.0, 3.0)
            assert not r["G"].any() and (r["Q"][r["valid"] == 1] == 1.0).all()


def sr_loss(c):
    """−Σ w·cum over the captions that are not barred, ``scst_reference.seq_nll``'s sum"""
    total = np.float64(0.0)
    for w, cu, b in zip(c["w"].reshape(-1), c["cum"].reshape(-1), c["barred"].reshape(-1)):
        if not b:
            total += np.float64(w) * np.float64(cu)
    return np.float32(-total)


def test_fixed_gpu_inputs_have_no_hinge_near_zero():
    """a condition on the seeded kernel-level inputs (no case is excluded): from the restatement, fed the restatement's own cum, no hinge
    argument lies within 1e-9 of 0, every video's rank term is large enough against its z for a relative bound of 1e-12 to mean something
    (``risk_reference.rank_conditioning``), every case with K ≥ 2 and a rank term has active and inactive pairs somewhere, and the special videos are
    what the case builder says"""
    seen_active = seen_idle = False
    for i, (C, Lt, K, steps, logits, wide, beta, alpha, margin) in enumerate(rc.KERNEL_CASES):
        c = rc.score_case(100 + i, C, Lt, K, steps, logits, wide)
        nl = sr.seq_nll(c["scores"][:, :C], c["ids"], c["row_c"], c["w"], logits)
        assert sorted(np.nonzero(nl["barred"])[0].tolist()) == sorted(c["bar_rows"])
        r = rr.groups(nl["cum"], nl["len"], nl["barred"], c["cost"], c["vid_off"], c["w"], alpha, beta, margin, 1.0, 1.0)
        assert rr.min_hinge_distance(r) > rc.HINGE_MARGIN, (i, rr.min_hinge_distance(r))
        assert rr.rank_conditioning(r) >= rc.RANK_CONDITION, (i, rr.rank_conditioning(r))
        seen_active |= bool(r["active"].any())
        seen_idle |= bool((r["pair"] & ~r["active"]).any())
        if len(steps) >= 2 and steps[-1]:
            assert not r["valid"][-1].any()
        if alpha == 40.0:
            zs = r["z"][r["valid"] == 1]
            assert alpha * (zs.max() - zs.min()) > 700.0
    assert seen_active and seen_idle


# ------------------------------------------------------------------------------------------------ the host checks
def test_every_value_error():
    cost = torch.zeros(3, 4, dtype=torch.float64)
    for k in (0, 17, -1, 2.0, True):
        with pytest.raises(ValueError):
            ops.check_risk(k=k)
    assert ops.check_risk(k=16)[0] == 16 and ops.check_risk(k=1)[0] == 1
    for bad in (cost.float(), cost[0], cost.unsqueeze(0), torch.zeros(3, 17, dtype=torch.float64), torch.zeros(3, 0, dtype=torch.float64),
                cost.tolist()):
        with pytest.raises(ValueError):
            ops.check_risk(cost=bad)
    with pytest.raises(ValueError):
        ops.check_risk(k=3, cost=cost)                                        # K is not the cost's column count
    for off, T in (([1, 2, 3, 4], 4), ([0, 2, 1, 4], 4), ([0, 1, 2, 3], 4), ([0, 5], 4), ([], 0)):
        with pytest.raises(ValueError):
            ops.check_risk(vid_off=off, n_sent=T)
    assert ops.check_risk(vid_off=[0, 2, 2, 4], n_sent=4)[1] == 3             # a video without sentences is allowed
    for name in ("alpha", "length_beta", "margin", "risk_weight", "rank_weight"):
        for v in (-1e-9, float("nan"), float("inf"), "1", True):
            with pytest.raises(ValueError):
                ops.check_risk(**{name: v})
        ops.check_risk(**{name: 0.0})
    with pytest.raises(ValueError):
        ops.check_risk(source="greedy")
    with pytest.raises(ValueError):
        ops.check_risk(utility="METEOR")
    assert ops.RISK_SOURCES == ("sample", "nbest", "diverse", "stochastic")
    assert ops.check_risk(k=4, source="stochastic", utility="CIDEr") == (4, None, 5)


def test_no_cpu_fallback():
    with pytest.raises(_lib.SvpcKernelError):
        ops.check_risk(cost=torch.zeros(3, 4, dtype=torch.float64))
    R, Lt, C, K = 4, 3, 9, 2
    with pytest.raises(_lib.SvpcKernelError):
        ops.seq_risk(torch.rand(R * Lt, C), [C] * R, torch.zeros(R, Lt, dtype=torch.int32), torch.ones(R, dtype=torch.int32),
                     torch.zeros(1, K, dtype=torch.float64), [0, 2], None, False, UNK, 1.0, 0.0, 0.1, 1.0, 0.0)
    from svpc_amd import mrt
    with pytest.raises(_lib.SvpcKernelError):
        mrt.risk_loss(None, None, None, torch.zeros(1, K, dtype=torch.float64))


def test_symbol_is_declared_and_exported():
    decls = _lib.declarations()
    assert "svpc_seq_risk_fwd" in decls and len(decls["svpc_seq_risk_fwd"][1]) == 31
    lib = _lib.load()
    assert hasattr(lib, "svpc_seq_risk_fwd") and lib.svpc_abi_version() == 2
    text = open(_lib.HEADER_PATH).read()
    assert "svpc_seq_risk_fwd" in text and "DESIGN 11.18" in text
