"""Contrastive (SimCTG) training without a GPU: the restatement (tests/simctg_reference.py) against torch autograd in fp64
and on hand-checked cases, its dot products against ``contrastive_reference.wave_dot``, every host check, no CPU fallback, the declared
and exported symbols, and the distances from the hinge's kinks of the inputs the GPU tests run on."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import contrastive_reference as cr  # noqa: E402
import simctg_cases as sc  # noqa: E402
import simctg_reference as sr  # noqa: E402
from svpc_amd import _lib, ops  # noqa: E402

f32 = np.float32


# ------------------------------------------------------------------------------------------------ the restatement alone
def test_gram_is_wave_dot():
    rng = np.random.default_rng(3)
    for D in (1, 32, 63, 64, 100, 768):
        H = rng.standard_normal((4, D)).astype(f32)
        G = sr.gram(H)
        for i in range(4):
            for j in range(4):
                assert G[i, j] == cr.wave_dot(H[i], H[j]), (D, i, j)


@pytest.mark.parametrize("rho", [0.3, 0.5, 1.0, 1.5, 2.0])
def test_restatement_against_autograd(rho):
    """loss and gradient of random captions against the textbook formula under torch autograd in fp64: the formula, the factor 2, the
    weights and the upstream factor"""
    rng = np.random.default_rng(int(rho * 10))
    lt, D, R, dl = 7, 24, 6, 2.5
    hidden = rng.standard_normal((R * lt, D)).astype(f32) + (rng.random((R * lt, 1)) * 1.5).astype(f32) * rng.standard_normal((1, D)).astype(f32)
    hidden[2 * lt + 1] = 0.0                                                   # a zero row
    length = np.array([6, 3, 4, 0, 1, 9])                                      # n = 1, n = 2, a length past the end
    v = np.array([0.3, -0.2, 0.7, 1.0, 0.5, 0.25], f32)
    ref = sr.seq_cl(hidden, length, v, rho, lt, dl=dl)
    assert ref["min_abs_m"][[0, 1, 4, 5]].min() > 1e-6      # clear of the kinks (caption 2's zero row: m = ρ − 1, at ρ = 1 exactly 0, inactive)
    h = torch.from_numpy(hidden).double().requires_grad_(True)
    total = torch.zeros((), dtype=torch.float64)
    for r in range(R):
        n = sr.tokens(length[r], lt)
        cl, sim = sr.cl_autograd(h[r * lt:r * lt + n], f32(rho))
        np.testing.assert_allclose(float(cl.detach()), ref["cl64"][r], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(float(sim), ref["sim64"][r], rtol=1e-12, atol=1e-15)
        total = total + float(v[r]) * cl
    (total * dl).backward()
    g = h.grad.numpy()
    np.testing.assert_allclose(ref["dh"], g, rtol=1e-9, atol=1e-12 * np.abs(g).max())
    assert abs(float(ref["loss"]) - float(total)) <= 2.0 ** -23 * abs(float(total)) + 1e-6 * float(np.abs(v * ref["cl"]).sum())
    assert not ref["dh"][2 * lt + 1].any() and not ref["dh"][3 * lt:4 * lt].any() and not ref["dh"][1 * lt + 4:2 * lt].any()
    assert ref["nact"][3] == 0 and ref["cl"][3] == 0 and ref["sim"][3] == 0
    assert ref["q"][3, 0] == cr.wave_dot(hidden[3 * lt], hidden[3 * lt]) and not ref["q"][3, 1:].any()
    assert 0 < ref["nact"].sum() < sum(n * (n - 1) for n in (sr.tokens(x, lt) for x in length)) or rho >= 1.5


def test_hand_checked_cases():
    lt, D = 4, 8
    a = np.zeros(D, f32); a[:4] = [1.0, 2.0, -1.0, 0.5]
    b = np.zeros(D, f32); b[4:] = [3.0, 1.0, 2.0, -2.0]
    pad = np.full((lt - 2, D), 7.0, f32)                                       # positions past the end: never read
    # two identical rows: c = 1, active for every ρ, cl = ρ, the gradient 0 since g ∥ u
    for rho in (0.001, 0.5, 1.0, 2.0):
        r = sr.seq_cl(np.vstack([a, a, pad]), [1], [1.0], rho, lt)
        assert r["nact"][0] == 2 and abs(r["cl64"][0] - float(f32(rho))) < 1e-15 and abs(r["sim64"][0] - 1.0) < 1e-15
        assert np.abs(r["dh"]).max() < 1e-15
    # disjoint support: c = 0 exactly; at ρ = 1 m = 0 exactly — inactive, no gradient; below 1 inactive, above 1 active with c constant
    for rho, act, cl in ((1.0, 0, 0.0), (0.5, 0, 0.0), (2.0, 2, 1.0)):
        r = sr.seq_cl(np.vstack([a, b, pad]), [1], [1.0], rho, lt)
        assert r["m"][0][0, 1] == rho - 1.0 and r["nact"][0] == act and r["cl64"][0] == cl and r["sim64"][0] == 0.0
        if act == 0:
            assert not r["dh"].any()
    # a zero row: cosine 0 with everything, its gradient exactly 0, and it moves no other row
    r = sr.seq_cl(np.vstack([a, np.zeros(D, f32), a + b, pad[:1]]), [2], [1.0], 2.0, lt)
    r2 = sr.seq_cl(np.vstack([a, a + b, pad]), [1], [1.0], 2.0, lt)
    assert r["nact"][0] == 6 and not r["dh"][1].any() and r["q"][0, 1] == 0.0
    np.testing.assert_allclose(r["dh"][[0, 2]] * 3.0, r2["dh"][[0, 1]], rtol=1e-12)      # (2 / (3·2) against 2 / (2·1))
    # n = 1: nothing to push apart
    r = sr.seq_cl(np.vstack([a, pad, pad[:1]]), [0], [1.0], 0.5, lt)
    assert r["cl"][0] == 0 and r["sim"][0] == 0 and r["nact"][0] == 0 and not r["dh"].any() and r["loss"] == 0 and r["q"][0, 0] > 0
    # n = 2 by hand: h0 = (1, 0), h1 = (1, 1): c = 1/√2; ρ = 0.5: m = c − 0.5, cl = m; d cl / d h0 = (u1 − c·u0) / |h0| = (0, 1/√2)
    h = np.zeros((2, D), f32); h[0, 0] = 1.0; h[1, 0] = 1.0; h[1, 1] = 1.0
    r = sr.seq_cl(np.vstack([h, pad]), [1], [1.0], 0.5, lt)
    c = 1.0 / math.sqrt(2.0)
    assert abs(r["cl64"][0] - (c - 0.5)) < 1e-15 and r["nact"][0] == 2
    np.testing.assert_allclose(r["dh"][0, :2], [0.0, c], atol=1e-15)
    np.testing.assert_allclose(r["dh"][1, :2], [c / 2, -c / 2], atol=1e-15)    # (u0 − c·u1) / |h1| = ((1, 0) − (½, ½)) / √2
    assert r["loss"] == f32(f32(c - 0.5))


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
@pytest.mark.parametrize("D", sc.DS)
@pytest.mark.parametrize("Lt", sc.LTS)
def test_fixed_inputs_keep_clear_of_the_kinks(D, Lt):
    """every pair that is not a constructed exact case has |m_ij| > 1e-9: the kernel's nact must match the restatement's exactly; the
    constructed ones are exact: m = 0 at ρ = 1, inactive"""
    for R in sc.RS:
        case = sc.kernel_case(D, Lt, R)
        assert R == 1 or (case["length"][6] < 0 and case["length"][7] > Lt - 1)
        for rho in sc.MARGINS:
            assert sc.kink_distance(D, Lt, R, rho) > 1e-9, (D, Lt, R, rho)
            ref = sc.reference(D, Lt, R, rho)
            if rho == 1.0:
                for (r, i, j) in case["exact"]:
                    assert ref["m"][r][i, j] == 0.0
        if R > 1 and Lt >= 5:                      # the margins see active and inactive pairs
            total = sum(m.shape[0] * (m.shape[0] - 1) for m in sc.reference(D, Lt, R, 0.5)["m"])
            assert 0 < sc.reference(D, Lt, R, 0.5)["nact"].sum() < total


@pytest.mark.parametrize("case,mt", sc.MODEL_CASES)
def test_model_margins_keep_clear_of_the_kinks(golden_dir, case, mt):
    """per fixture the margin is chosen so that the restatement alone shows no pair with |m_ij| <= 1e-4"""
    for K in sc.MODEL_KS:
        r = sc.model_reference(golden_dir, case, mt, K, False)
        assert r["min_abs_m"] > sc.KINK, (case, mt, K, r["min_abs_m"])
        assert np.isfinite(r["loss"]) and (r["cl"] > 0).any()


# ------------------------------------------------------------------------------------------------ the host checks
def test_value_errors():
    for m in (0.0, -0.5, 2.5, float("nan"), float("inf"), "0.5", None, True, 1e-60):
        with pytest.raises(ValueError):
            ops.check_simctg(margin=m) if m is not None else ops.seq_cl(torch.zeros(4, 3), torch.zeros(2, dtype=torch.int32), torch.zeros(2), m, 2)
    assert ops.check_simctg(margin=0.1) == float(f32(0.1)) and ops.check_simctg(margin=2) == 2.0
    for w in (-1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError):
            ops.check_simctg(cl_weight=w)
    ops.check_simctg(cl_weight=0)
    good = torch.zeros(3, 2)
    for kw in (dict(weights=torch.zeros(3, 3)), dict(cl_weights=torch.zeros(5)), dict(cl_weights=torch.zeros(3, 2, dtype=torch.int32)),
               dict(weights=[0.0] * 6), dict(cl_weights=None, weights=np.zeros((3, 2)))):
        with pytest.raises(ValueError):
            ops.check_simctg(**dict(dict(shape=(3, 2)), **kw))
    with pytest.raises(ValueError):
        ops.check_simctg(cl_weights=[0.0])                                      # (no shape yet: still a tensor)
    with pytest.raises(_lib.SvpcKernelError):
        ops.check_simctg(weights=good, cl_weights=good, shape=(3, 2))           # CPU tensors: no fallback
    h, ln, v = torch.zeros(12, 8), torch.zeros(2, dtype=torch.int32), torch.zeros(2)
    for args in ((h, ln, v, 0.5, 1), (h, ln, v, 0.5, 33), (h, ln, v, 0.5, 7), (h.double(), ln, v, 0.5, 6), (h, ln.long(), v, 0.5, 6),
                 (h, ln, v.double(), 0.5, 6), (h, ln, torch.zeros(3), 0.5, 6), (h.view(-1), ln, v, 0.5, 6), (h, ln, v, 0.5, 6.0),
                 (torch.zeros(64, 2000), ln, v, 0.5, 32)):
        with pytest.raises(ValueError):
            ops.seq_cl(*args)


def _bare_translator():
    from svpc_amd.translator import Translator
    tr = object.__new__(Translator)                                            # (the checks come before any use of the model)
    tr.max_t_len = 22
    return tr


def test_module_checks_on_the_host():
    from svpc_amd import simctg
    tr = _bare_translator()
    inputs = [None] * 11 + [[2, 1]]
    dec = [torch.zeros(2, 3, 22, dtype=torch.int64), torch.zeros(1, 3, 22, dtype=torch.int64)]
    w = torch.zeros(3, 3)
    for m in (0.0, 2.5, float("nan")):
        with pytest.raises(ValueError):
            simctg.contrastive_loss(tr, inputs, dec, w, w, margin=m)
    with pytest.raises(ValueError, match="step counts"):
        simctg.contrastive_loss(tr, [None] * 11 + [[1, 2]], dec, w, w)
    with pytest.raises(ValueError):
        simctg.contrastive_loss(tr, inputs, dec, torch.zeros(3, 2), w)
    with pytest.raises(ValueError):
        simctg.contrastive_loss(tr, inputs, dec, w, [0.0] * 9)
    with pytest.raises(ValueError):
        simctg.contrastive_loss(tr, inputs, dec, w, torch.zeros(3, 3, dtype=torch.int32))
    with pytest.raises(_lib.SvpcKernelError):                                  # CPU ids: no fallback
        simctg.contrastive_loss(tr, inputs, dec, w, w)
    step = simctg.SimCTG(tr)
    for kw in (dict(margin=0.0), dict(margin=3.0), dict(cl_weight=-1.0), dict(cl_weight=float("nan")), dict(cl_weight=float("inf"))):
        with pytest.raises(ValueError):
            step.step(inputs, [], **kw)
    with pytest.raises(TypeError):
        step.step(inputs, [], alpha=1.0)                                        # an unknown keyword


def test_no_cpu_fallback():
    h, ln, v = torch.zeros(12, 8), torch.zeros(2, dtype=torch.int32), torch.zeros(2)
    with pytest.raises(_lib.SvpcKernelError):
        ops.seq_cl(h, ln, v, 0.5, 6)
    with pytest.raises(_lib.SvpcKernelError):
        ops.check_simctg(row_v=v, rows=2)


def test_symbols_declared_and_exported():
    decls = _lib.declarations()
    lib = _lib.load()
    for name, n_args in (("svpc_seq_cl_fwd", 14), ("svpc_seq_cl_bwd", 12)):
        assert name in decls and len(decls[name][1]) == n_args and hasattr(lib, name), name
    import ctypes
    assert decls["svpc_seq_cl_fwd"][1][7] is ctypes.c_double and decls["svpc_seq_cl_bwd"][1][8] is ctypes.c_double       # the margin
    assert lib.svpc_abi_version() == 2
    from svpc_amd import scst, simctg
    assert callable(simctg.contrastive_loss) and hasattr(simctg.SimCTG, "step") and callable(scst.graded_pass)
    for fn in ("check_simctg", "seq_cl"):
        assert callable(getattr(ops, fn))


def test_per_caption_weights():
    w, v = sr.per_caption_weights([3, 0, 5, 1], 0.5)
    assert w.dtype == f32 and np.all(w == f32(1.0 / 9.0)) and np.all(v == f32(0.5 / 3.0))
    w, v = sr.per_caption_weights([0, 0], 2.0)
    assert np.all(w == 1.0) and np.all(v == 2.0)
