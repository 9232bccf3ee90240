"""Clipped policy-gradient training without a GPU: the restatement (tests/pg_reference.py) against torch float64 autograd of
the written objective, hand-built positions of every kind, ``group_advantage``'s rules and its exactly-zero cases, every host check, no CPU
fallback, the argument rules of ``PolicyOptimization`` that need no device, the exported symbols, and the conditions on the fixed inputs the
GPU tests run on."""
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

import pg_cases as gc  # noqa: E402
import pg_reference as pg  # noqa: E402
import scst_reference as sr  # noqa: E402
from svpc_amd import _lib, mrt, ops, policy  # noqa: E402
from svpc_amd.synthetic import UNK  # noqa: E402

f32 = np.float32


def _one_caption(step, A, old=None, ref=None, w=None, lo=0.2, hi=0.2, dual=0.0, beta=0.0, norm="none", length=None):
    """one video, one sentence, one candidate"""
    step = np.asarray(step, f32).reshape(1, -1)
    n = step.shape[1] if length is None else length
    cum = np.asarray([step[0, :n].astype(np.float64).sum()], f32)
    return pg.positions(step, [n], [0], cum, [[A]], [0, 1], None if w is None else np.asarray([w], f32),
                        None if old is None else np.asarray(old, f32).reshape(1, -1), None if ref is None else np.asarray(ref, f32).reshape(1, -1),
                        lo, hi, dual, beta, norm)


# ------------------------------------------------------------------------------------------------ the restatement alone
def test_hand_built_positions():
    L2 = math.log(2.0)
    # ρ = (1, 2, 1/2) exactly (float32 steps that differ by ln 2 would not give that: use steps whose difference is exact: 0 and ±ln 2 in float32)
    s = np.asarray([-1.0, -1.0, -1.0], f32)
    o = np.asarray([-1.0, f32(-1.0) - f32(L2), f32(-1.0) + f32(L2)], f32)
    rho = np.exp(s.astype(np.float64) - o.astype(np.float64))
    assert rho[0] == 1.0 and abs(rho[1] - 2.0) < 1e-6 and abs(rho[2] - 0.5) < 1e-6
    # A > 0: position 1 (ρ = 2 > 1.2) is clipped from above: sur = 1.2·A, no gradient; position 2 (ρ = 1/2): min takes ρ·A, active
    r = _one_caption(s, 2.0, old=o)
    assert r["active"][0, 0].tolist() == [True, False, True] and r["n_clip"][0, 0].tolist() == [1, 0]
    assert r["sur"][0, 0, 1] == pytest.approx(2.4, rel=1e-15) and r["sur"][0, 0, 2] == rho[2] * 2.0
    assert r["pos_w64"][0, 0].tolist() == [2.0, 0.0, rho[2] * 2.0]           # N·K = 1: pos_w = A·ρ·[active]
    assert r["ratio_max"][0, 0] == f32(rho[1]) and r["pg"][0, 0] == -(2.0 + 2.4 + rho[2] * 2.0)
    assert float(r["total"]) == pytest.approx(-(2.0 + 2.4 + rho[2] * 2.0), rel=1e-15) and r["loss"].dtype == np.float32
    # A < 0: position 2 (ρ = 1/2 < 0.8) is clipped from below; position 1 (ρ = 2) active without dual clip, clipped at c = 1.5 with it
    r = _one_caption(s, -2.0, old=o)
    assert r["active"][0, 0].tolist() == [True, True, False] and r["n_clip"][0, 0].tolist() == [0, 1]
    assert r["sur"][0, 0, 2] == pytest.approx(-1.6, rel=1e-15) and r["pos_w64"][0, 0, 1] == -2.0 * rho[1]
    r = _one_caption(s, -2.0, old=o, dual=1.5)
    assert r["active"][0, 0].tolist() == [True, False, False] and r["n_clip"][0, 0].tolist() == [1, 1] and r["sur"][0, 0, 1] == -3.0
    # A = 0: nothing, whatever ρ; sequence norm divides by N·K·n = 3; token norm by n_tok = 3
    r = _one_caption(s, 0.0, old=o)
    assert not r["pos_w64"].any() and not r["sur"][0, 0].any() and not r["active"].any() and r["total"] == 0
    a, b = _one_caption(s, 1.5, norm="sequence"), _one_caption(s, 1.5, norm="token")
    assert a["pos_w64"][0, 0].tolist() == [0.5] * 3 and b["pos_w64"][0, 0].tolist() == [0.5] * 3 and b["n_tok"] == 3
    assert (a["rho"][0, 0] == 1.0).all() and not a["n_clip"].any()          # no old_step: ρ is exactly 1
    # a ρ exactly on a bound is active: clip 0 / 0 with ρ = 1
    r = _one_caption(s, 1.0, old=s, lo=0.0, hi=0.0)
    assert r["active"].all() and not r["n_clip"].any()
    # the KL: ref = step gives exactly 0; δ = ln 2 (in float32): kl = 2 − ln 2 − 1, g = β(1 − 2) = −β
    r = _one_caption(s, 0.0, ref=s, beta=0.5)
    assert not r["klt"][0, 0].any() and not r["pos_w64"].any() and r["total"] == 0
    r = _one_caption(s[:1], 0.0, ref=[f32(-1.0) + f32(L2)], beta=0.5)
    d = float(f32(-1.0) + f32(L2)) + 1.0
    assert r["klt"][0, 0, 0] == pytest.approx(math.exp(d) - d - 1.0, rel=1e-14) and r["klt"][0, 0, 0] > 0
    assert r["pos_w64"][0, 0, 0] == pytest.approx(-0.5 * (1.0 - math.exp(d)), rel=1e-14)
    assert float(r["total"]) == pytest.approx(0.5 * r["klt"][0, 0, 0], rel=1e-15)
    # likelihood weights: pos_w = w + …, the loss gains −w·cum; past the caption's end 0; a −inf past the end changes nothing
    r = _one_caption(s, 2.0, old=[-1.0, -1.0, -np.inf], w=0.25, length=2)
    assert r["valid"][0, 0] == 1 and r["pos_w64"][0, 0].tolist() == [2.25, 2.25, 0.0] and float(r["total"]) == pytest.approx(0.5 - 4.0)
    # a −inf inside: the candidate is invalid: no policy term, the likelihood weight stays (it is the gradient of the −w·cum in the loss)
    r = _one_caption(s, 2.0, old=[-1.0, -np.inf, -1.0], w=0.25)
    assert r["valid"][0, 0] == 0 and r["pos_w64"][0, 0].tolist() == [0.25] * 3 and float(r["total"]) == 0.75 and r["n_tok"] == 0
    assert not r["pg"].any() and r["ratio_max"][0, 0] == 0


SETTINGS = [(True, True, "sequence", 0.2, 0.2, 0.0, 0.04), (True, False, "token", 0.2, 0.28, 0.0, 0.0), (True, True, "none", 0.2, 0.2, 3.0, 0.04),
            (False, True, "sequence", 0.2, 0.2, 0.0, 0.04), (False, False, "none", 0.2, 0.2, 0.0, 0.0), (True, False, "sequence", 0.0, 0.0, 3.0, 0.0)]
AUTOGRAD_CASES = [(300, 7, 2, 1, [1], False), (302, 65, 6, 2, [3, 1, 2], False), (303, 65, 6, 3, [3, 1, 2], True), (311, 65, 22, 3, [3, 0, 2], False),
                  (320, 7, 6, 16, [2, 1], True), (321, 7, 6, 3, [2] * 9, False)]


@pytest.mark.parametrize("with_old,with_ref,norm,lo,hi,dual,beta", SETTINGS)
@pytest.mark.parametrize("seed,C,Lt,K,steps,logits", AUTOGRAD_CASES)
def test_restatement_against_autograd(seed, C, Lt, K, steps, logits, with_old, with_ref, norm, lo, hi, dual, beta):
    """∂loss / ∂step = −pos_w on every caption that is not barred — the valid candidates' positions with the policy term, the others with
    the likelihood weight alone — and 0 on barred captions (the backward zeroes their rows)"""
    c = gc.score_case(seed, C, Lt, K, steps, logits, False, clip_zero=(lo == 0.0 and hi == 0.0))
    old, ref = (c["old_step"] if with_old else None), (c["ref_step"] if with_ref else None)
    own = c["own_step"]
    cum = sr.seq_nll(c["scores"][:, :C], c["ids"], c["row_c"], c["w"], logits)["cum"]
    r = pg.positions(own, c["len"], c["own_barred"], cum, c["adv"], c["vid_off"], c["w"], old, ref, lo, hi, dual, beta, norm)
    T = sum(steps)
    leaf = torch.tensor(np.where(np.isfinite(own), own, 0.0).astype(np.float64).reshape(T, K, Lt - 1), requires_grad=True)
    total = pg.objective_torch(leaf, c["len"], c["own_barred"], c["adv"], c["vid_off"], c["w"], old, ref, lo, hi, dual, beta, norm)
    total.backward()
    tot = float(total.detach())
    # (the restatement's likelihood term reads the float32 cum, the written objective sums the steps in float64: compare the policy term)
    alive = np.asarray(c["own_barred"]) == 0
    nll64 = sum(float(c["w"][row]) * float(own[row, :c["len"][row]].astype(np.float64).sum()) for row in np.nonzero(alive)[0])
    want = -nll64 + float(r["total"] + r["nll"])
    assert abs(tot - want) <= 1e-12 * max(1.0, abs(tot))
    g = leaf.grad.numpy()
    live = np.broadcast_to((np.asarray(c["own_barred"]).reshape(T, K) == 0)[:, :, None], g.shape)
    scale = 1.0 + r["gmax"] + float(np.abs(c["w"]).max())
    assert np.abs(g[live] + r["pos_w64"][live]).max() <= 1e-13 * scale
    assert not g[~live].any()
    valid_rows = r["valid"][r["row_vid"]] == 1                               # (T, K)
    assert not (r["pos_w64"] - np.asarray(c["w"], np.float64).reshape(T, K, 1) * (r["pos_w64"] != 0))[~valid_rows].any()
    assert (r["pg"][~valid_rows] == 0).all() and (r["kl"][~valid_rows] == 0).all() and not r["n_clip"][~valid_rows].any()


def test_exact_identities():
    """every advantage 0 and kl_beta 0: pos_w is row_w at the scored positions, bit for bit, and the loss is ``seq_nll``'s; no old_step,
    kl_beta 0, norm "none": pos_w = float32(A / (N·K)) + nothing else, no clip; ref_step = step: kl is exactly 0"""
    for seed, C, Lt, K, steps, logits in AUTOGRAD_CASES:
        c = gc.score_case(seed, C, Lt, K, steps, logits, False)
        nl = sr.seq_nll(c["scores"][:, :C], c["ids"], c["row_c"], c["w"], logits)
        N, T = len(steps), sum(steps)
        args = (c["own_step"], c["len"], c["own_barred"], nl["cum"])
        zero = np.where(np.isnan(c["adv"]), np.nan, 0.0)
        r = pg.positions(*args, zero, c["vid_off"], c["w"], None, c["ref_step"], 0.2, 0.2, 3.0, 0.0, "sequence")
        want = np.where(np.arange(Lt - 1)[None, :] < np.asarray(c["len"])[:, None], c["w"][:, None], f32(0.0)).astype(f32)
        assert np.array_equal(r["pos_w"].reshape(-1, Lt - 1).view(np.int32), want.view(np.int32))
        assert r["loss"].view(np.int32) == nl["loss"].view(np.int32)
        r = pg.positions(*args, c["adv"], c["vid_off"], None, None, None, 0.2, 0.2, 0.0, 0.0, "none")
        assert not r["n_clip"].any() and (r["rho"][r["scored"]] == 1.0).all()
        A = np.where(r["valid"] == 1, c["adv"], 0.0)[r["row_vid"]]           # (T, K)
        roww = (A / np.float64(N * K)).astype(f32)
        want = np.where(np.arange(Lt - 1)[None, None, :] < np.asarray(c["len"]).reshape(T, K, 1), roww[:, :, None], f32(0.0)).astype(f32)
        assert np.array_equal(r["pos_w"].view(np.int32), want.view(np.int32))
        r = pg.positions(*args, c["adv"], c["vid_off"], None, None, np.where(np.isfinite(c["own_step"]), c["own_step"], f32(0.0)),
                         0.2, 0.2, 0.0, 0.04, "token")
        assert not r["kl"].any() and (r["klt"][r["scored"]] == 0.0).all()


# ------------------------------------------------------------------------------------------------ the advantage rules
def test_group_advantage_rules():
    r = np.asarray([[1.0, 2.0, 4.0, np.nan], [0.5, 0.5, np.inf, 3.5]])
    a = pg.group_advantage(r, "center", 0.0)
    assert a[0].tolist() == [1.0 - 7.0 / 3.0, 2.0 - 7.0 / 3.0, 4.0 - 7.0 / 3.0, 0.0] and a[1].tolist() == [-1.0, -1.0, 0.0, 2.0]
    a = pg.group_advantage(r, "rloo", 0.0)
    assert a[0].tolist() == [1.0 - 3.0, 2.0 - 2.5, 4.0 - 1.5, 0.0] and a[1].tolist() == [0.5 - 2.0, 0.5 - 2.0, 0.0, 3.5 - 0.5]
    assert np.array_equal(a[0, :3], sr.advantages(r[:1, :3], "mean")[0])     # svpc_scst_weights' leave-one-out rule
    a = pg.group_advantage(r, "grpo", 0.0)
    sd = math.sqrt(((1 - 7 / 3) ** 2 + (2 - 7 / 3) ** 2 + (4 - 7 / 3) ** 2) / 3)
    assert a[0, :3] == pytest.approx([(1 - 7 / 3) / sd, (2 - 7 / 3) / sd, (4 - 7 / 3) / sd], rel=1e-14) and a[0, 3] == 0
    assert sum(a[0]) == pytest.approx(0.0, abs=1e-15) and np.mean(a[0, :3] ** 2) == pytest.approx(1.0, rel=1e-14)
    assert pg.group_advantage(r, "grpo", 1.0)[1, 3] == pytest.approx(2.0 / (math.sqrt(2.0) + 1.0), rel=1e-14)
    # exactly zero: K = 1; all rewards equal at K = 3; one finite reward; no finite reward
    for rule in pg.RULES:
        for rr in ([[0.7]], [[0.3, 0.3, 0.3]], [[np.nan, 1.5, np.inf]], [[np.nan, -np.inf, np.inf]], [[0.1 + 0.2, 0.1 + 0.2, np.nan, 0.1 + 0.2]]):
            a = pg.group_advantage(np.asarray(rr), rule, 1e-6)
            assert not a.any() and not np.signbit(a).any(), (rule, rr)


# ------------------------------------------------------------------------------------------------ conditions on the fixed inputs
def test_fixed_gpu_inputs_meet_their_conditions():
    """every case of ``pg_cases.KERNEL_CASES``, none left out: no ρ lies within 1e-5 (relative) of a bound that can switch it, except the
    positions set on a bound by construction, which are exactly on it; over the family every kind of position occurs; and the special
    rows are what the case builder says"""
    seen = dict(above=False, below=False, active_pos=False, active_neg=False, zero=False, dual=False)
    special = dict(inside=False, past=False, exact=False, barred=False, empty_video=False, nan_adv=False)
    for seed, C, Lt, K, steps, logits, wide, with_old, with_ref, norm, lo, hi, dual, beta in gc.KERNEL_CASES:
        c = gc.score_case(seed, C, Lt, K, steps, logits, wide, clip_zero=(lo == 0.0 and hi == 0.0))
        assert sorted(np.nonzero(c["own_barred"])[0].tolist()) == sorted(c["bar_rows"])
        cum = sr.seq_nll(c["scores"][:, :C], c["ids"], c["row_c"], c["w"], logits)["cum"]
        old, ref = (c["old_step"] if with_old else None), (c["ref_step"] if with_ref else None)
        r = pg.positions(c["own_step"], c["len"], c["own_barred"], cum, c["adv"], c["vid_off"], c["w"], old, ref, lo, hi, dual, beta, norm)
        exact = {(row // K, row % K, i) for row, i in c["exact"]} if with_old else set()
        assert pg.bound_distance(r, lo, hi, dual, exact) > gc.BOUND_MARGIN, (seed, pg.bound_distance(r, lo, hi, dual, exact))
        for t, k, i in exact:
            if r["scored"][t, k, i]:
                assert r["rho"][t, k, i] == 1.0 and (r["active"][t, k, i] or c["adv"][r["row_vid"][t], k] == 0)
                special["exact"] = True
        for key, v in pg.kinds(r, hi, dual).items():
            seen[key] |= v
        for nm, l, h, du, b in gc.ALT_SETTINGS:                               # the other settings every case also runs under
            a = pg.positions(c["own_step"], c["len"], c["own_barred"], cum, c["adv"], c["vid_off"], c["w"], old, ref, l, h, du,
                             b if with_ref else 0.0, nm)
            assert pg.bound_distance(a, l, h, du, exact) > gc.BOUND_MARGIN, (seed, nm, pg.bound_distance(a, l, h, du, exact))
        assert np.isfinite(r["pos_w64"]).all() and np.isfinite(r["total"])
        N = len(steps)
        for name, row, i in c["inf_inside"]:
            used = (name == "old_step" and with_old) or (name == "ref_step" and with_ref)
            t, k = divmod(row, K)
            b = int(r["row_vid"][t])
            assert i < c["len"][row] and not c["own_barred"][row]
            if used and np.isfinite(c["adv"][b, k]):
                assert not r["valid"][b, k]
                alone = pg.positions(c["own_step"], c["len"], c["own_barred"], cum, c["adv"], c["vid_off"], c["w"], None, None, lo, hi, dual, 0.0,
                                     norm)
                assert alone["valid"][b, k]                                  # … and only for it
                special["inside"] = True
        for name, row, i in c["inf_past"]:
            assert i >= c["len"][row]
            t, k = divmod(row, K)
            special["past"] |= bool(r["valid"][int(r["row_vid"][t]), k]) and (with_old or with_ref)
        special["barred"] |= bool(c["bar_rows"])
        special["empty_video"] |= bool(N >= 2 and steps[-1] and not r["valid"][-1].any())
        special["nan_adv"] |= bool(np.isnan(c["adv"]).any())
        assert r["n_tok"] == int(sum(c["len"][row] for row in range(len(c["len"])) if r["valid"][r["row_vid"][row // K], row % K]))
    assert all(seen.values()), seen
    assert all(special.values()), special


# ------------------------------------------------------------------------------------------------ the host checks
def test_every_value_error():
    adv = torch.zeros(3, 4, dtype=torch.float64)
    for k in (0, 17, -1, 2.0, True):
        with pytest.raises(ValueError):
            ops.check_pg(k=k)
    assert ops.check_pg(k=16)[0] == 16 and ops.check_pg(k=1)[0] == 1
    for bad in (adv.float(), adv[0], torch.zeros(3, 17, dtype=torch.float64), torch.zeros(3, 0, dtype=torch.float64), adv.tolist()):
        with pytest.raises(ValueError):
            ops.check_pg(adv=bad)
    for off, T in (([1, 2, 3, 4], 4), ([0, 2, 1, 4], 4), ([0, 5], 4), ([], 0)):
        with pytest.raises(ValueError):
            ops.check_pg(vid_off=off, n_sent=T)
    for v in (-1e-9, 1.0, 1.5, float("nan"), float("inf"), "0.2", True):
        with pytest.raises(ValueError):
            ops.check_pg(clip_lo=v)
    for name in ("clip_hi", "kl_beta", "eps"):
        for v in (-1e-9, float("nan"), float("inf"), "1", True):
            with pytest.raises(ValueError):
                ops.check_pg(**{name: v})
        ops.check_pg(**{name: 0.0})
    for v in (1.0, 0.5, -3.0, float("nan"), float("inf"), "3", True):
        with pytest.raises(ValueError):
            ops.check_pg(dual_clip=v)
    ops.check_pg(clip_lo=0.0, clip_hi=5.0, dual_clip=0.0)
    ops.check_pg(clip_lo=0.999, dual_clip=1.0001, kl_beta=0.04, has_ref=True)
    for kw in (dict(norm="mean"), dict(norm=0), dict(advantage="zscore"), dict(advantage=1), dict(source="greedy"), dict(utility="METEOR"),
               dict(kl_beta=0.04, has_ref=False), dict(kl_beta=0.04, rows=6, lt=3)):
        with pytest.raises(ValueError):
            ops.check_pg(**kw)
    ops.check_pg(kl_beta=0.0, has_ref=False)
    st = torch.zeros(6, 2, dtype=torch.float32)
    for name in ("old_step", "ref_step"):
        for bad, rows in ((st.double(), 6), (st[::2], 3), (st[:, :1], 6), (st.tolist(), 6), (st, 5)):
            with pytest.raises(ValueError):
                ops.check_pg(rows=rows, lt=3, **{name: bad})
        with pytest.raises(ValueError):
            ops.check_pg(rows=6, lt=3, device=torch.device("cuda:0"), **{name: st})
    with pytest.raises(ValueError):
        ops.check_pg(adv=adv, device=torch.device("cuda:0"))
    for bad in (adv.float(), adv[0], "grpo"):
        with pytest.raises(ValueError):
            ops.group_advantage(bad)
    with pytest.raises(ValueError):
        ops.group_advantage(torch.zeros(2, 17, dtype=torch.float64))
    assert ops.PG_NORMS == ("sequence", "token", "none") and ops.PG_ADVANTAGES == ("grpo", "center", "rloo")
    assert ops.check_pg(k=4, source="sample", utility="CIDEr", norm="token", advantage="rloo") == (4, None, 5, 1, 2)


def test_no_cpu_fallback():
    with pytest.raises(_lib.SvpcKernelError):
        ops.check_pg(adv=torch.zeros(3, 4, dtype=torch.float64))
    for name in ("old_step", "ref_step"):
        with pytest.raises(_lib.SvpcKernelError):
            ops.check_pg(rows=6, lt=3, **{name: torch.zeros(6, 2, dtype=torch.float32)})
    with pytest.raises(_lib.SvpcKernelError):
        ops.group_advantage(torch.zeros(3, 4, dtype=torch.float64))
    R, Lt, C, K = 4, 3, 9, 2
    with pytest.raises(_lib.SvpcKernelError):
        ops.seq_pg(torch.rand(R * Lt, C), [C] * R, torch.zeros(R, Lt, dtype=torch.int32), torch.ones(R, dtype=torch.int32),
                   torch.zeros(1, K, dtype=torch.float64), [0, 2], None, None, None, False, UNK)
    with pytest.raises(_lib.SvpcKernelError):
        policy.policy_loss(None, None, None, torch.zeros(1, K, dtype=torch.float64))


def test_argument_rules_without_a_device():
    model = torch.nn.Linear(1, 1)
    tr = SimpleNamespace(model=model)
    po = policy.PolicyOptimization(tr, None, reference=tr)
    assert po.reference is tr and po.phase_events is None and isinstance(po, mrt.MinimumRisk)
    bad = [dict(source="greedy"), dict(utility="METEOR"), dict(num_candidates=17), dict(num_candidates=0), dict(advantage="zscore"),
           dict(clip_lo=1.0), dict(clip_hi=-0.1), dict(dual_clip=1.0), dict(kl_beta=-1.0), dict(norm="mean"), dict(adv_eps=-1.0),
           dict(clip_lo=float("nan"))]
    model.eval()
    for kw in bad:
        with pytest.raises(ValueError):
            po.step(None, None, **kw)
    for kw in bad[:5]:
        with pytest.raises(ValueError):
            po.collect(None, None, **kw)
    with pytest.raises(ValueError, match="ref_step"):
        policy.PolicyOptimization(tr, None).step(None, None, kl_beta=0.04)     # a KL term without a reference
    ro = SimpleNamespace(ref_step=None, old_step=None, adv=None, dec_seq_list=None)
    with pytest.raises(ValueError, match="ref_step"):
        po.update(ro, None, kl_beta=0.04)
    with pytest.raises(TypeError):
        po.update(ro, None, beta=0.1)
    # the policy as its own reference must be in eval mode: in training mode the reference would see dropout
    model.train()
    with pytest.raises(ValueError, match="dropout"):
        po.step(None, None)
    with pytest.raises(ValueError, match="dropout"):
        po.collect(None, None)
    assert model.training


def test_symbols_are_declared_and_exported():
    decls = _lib.declarations()
    for name, n in (("svpc_seq_pg_fwd", 37), ("svpc_seq_pos_bwd", 16), ("svpc_group_advantage", 7)):
        assert name in decls and len(decls[name][1]) == n, name
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in ("svpc_seq_pg_fwd", "svpc_seq_pos_bwd", "svpc_group_advantage")) and lib.svpc_abi_version() == 2
    text = open(_lib.HEADER_PATH).read()
    assert "svpc_seq_pg_fwd" in text and "DESIGN 11.22" in text
