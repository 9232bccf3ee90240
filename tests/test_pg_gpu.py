"""Clipped policy-gradient training on the MI355X: svpc_seq_pg_fwd / svpc_seq_pos_bwd against ``ops.seq_nll`` (bit for bit
where the definition says so) and the restatement (tests/pg_reference.py) on the seeded inputs of tests/pg_cases.py; ``policy.policy_loss``
against ``scst.sequence_loss``; ``position_scores``; ``PolicyOptimization`` end to end for the four candidate sources, two updates on one
rollout, the policy as its own behaviour policy, and the bf16x3 deviation.

Bounds.  step / cum / barred, and with every advantage 0 and ``kl_beta`` = 0 the loss and dscores: ``seq_nll``'s bits.  valid, n_clip, n_tok:
exact.  pos_w: one fp32 ulp plus 1e-12·(|w| + max|g / den|) for the cancellation, against the restatement fed the kernel's own step bits
(``test_pref_gpu.py``'s rule for w_eff).  loss: one fp32 ulp.  pg / kl: 1e-12 relative plus 1e-15 per position (every term is a difference
of O(1) float64 values that carry an ulp or two each).  ratio_max: one fp32 ulp.  dscores: −pos_w / p at the target column, bit for bit
(probabilities); 1e-6 of the row's largest entry (logits: the log-sum-exp is re-derived here).  Condition on the inputs, asserted from the
restatement fed the kernel's step: no ρ within 1e-5 (relative) of a bound that can switch it, except those set exactly on it.  Measured
bounds: see ``MEASURED_SELF`` and ``MEASURED_X3``."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pg_cases as gc  # noqa: E402
import pg_reference as pg  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import ops, policy, scst, synthetic as syn  # noqa: E402
from svpc_amd.ops_common import Idx  # noqa: E402
from svpc_amd.synthetic import EOS, IGNORE, PAD, UNK  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPORT_DIR = os.environ.get("SVPC_REPORT_DIR") or os.path.join(ROOT, "reports")
NAMES = ("loss", "cum", "step", "barred", "pos_w", "pg", "kl", "n_clip", "ratio_max", "valid", "n_tok")


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def _np(out):
    return {k: v.detach().cpu().numpy() for k, v in zip(NAMES, out)}


def _check(got, ref, w, steps):
    """a kernel run (numpy) against the restatement fed the kernel's own step"""
    T, K = ref["pg"].shape
    np.testing.assert_array_equal(got["valid"], ref["valid"])
    np.testing.assert_array_equal(got["n_clip"].reshape(T, K, 2), ref["n_clip"])
    assert int(got["n_tok"][0]) == ref["n_tok"]
    for k in ("pg", "kl"):
        g, r = got[k].reshape(T, K), ref[k]
        assert np.isfinite(g).all(), k
        assert (np.abs(g - r) <= 1e-12 * np.abs(r) + 1e-15 * steps).all(), (k, float(np.abs(g - r).max()))
    rm, rr = got["ratio_max"].reshape(T, K).astype(np.float64), ref["ratio_max"].astype(np.float64)
    assert (np.abs(rm - rr) <= np.spacing(ref["ratio_max"])).all()
    want = ref["pos_w"].reshape(-1, steps)
    wcol = np.zeros(want.shape[0]) if w is None else np.abs(w.reshape(-1).astype(np.float64))
    tol = np.spacing(np.abs(want)).astype(np.float64) + 1e-12 * (wcol[:, None] + ref["gmax"])
    err = np.abs(got["pos_w"].reshape(-1, steps).astype(np.float64) - want.astype(np.float64))
    assert (err <= tol).all(), (float(err.max()), int(err.argmax()))
    assert not got["pos_w"].reshape(T, K, steps)[~ref["scored"] & (ref["pos_w64"] == 0)].any()
    assert abs(float(got["loss"]) - float(ref["total"])) <= _ulp32(ref["total"]), (float(got["loss"]), float(ref["total"]))


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("i", range(len(gc.KERNEL_CASES)))
def test_kernels(i):
    seed, C, Lt, K, steps, logits, wide, with_old, with_ref, norm, lo, hi, dual, beta = gc.KERNEL_CASES[i]
    c = gc.score_case(seed, C, Lt, K, steps, logits, wide, clip_zero=(lo == 0.0 and hi == 0.0))
    N, T, S = len(steps), sum(steps), Lt - 1
    R = T * K
    sd = torch.from_numpy(c["scores"]).to(DEV)                                # (under ``wide`` the rows are C + 5 floats apart)
    rcx = Idx(c["row_c"].tolist())
    wd = torch.from_numpy(c["w"]).to(DEV)
    adv = torch.from_numpy(c["adv"]).to(DEV)
    V = max(UNK + 1, C - 2)
    _, _, tgt, ln, _ = ops.force_inputs(torch.from_numpy(c["ids"]).to(DEV).view(T, K, Lt), V, UNK, EOS, PAD, IGNORE)
    lnh = ln.cpu().numpy()

    def nll(w):
        s = sd.detach().clone().requires_grad_(True)
        out = ops.seq_nll(s, rcx, tgt, ln, w, logits, UNK)
        out[0].backward()
        return out, s.grad

    base, d_base = nll(wd)
    step_dev = base[2].cpu().numpy()
    # the ρ set exactly on a bound: old_step is the kernel's own step there, bit for bit
    old_np = c["old_step"].copy()
    for r, p in c["exact"]:
        old_np[r, p] = step_dev[r, p]
    oldd = torch.from_numpy(old_np).to(DEV) if with_old else None
    refd = torch.from_numpy(c["ref_step"]).to(DEV) if with_ref else None

    def run(a=adv, old=oldd, ref=refd, w=wd, l=lo, h=hi, du=dual, b=beta, nm=norm):
        s = sd.detach().clone().requires_grad_(True)
        out = ops.seq_pg(s, rcx, tgt, ln, a, c["vid_off"], old, ref, w, logits, UNK, l, h, du, b, nm)
        assert out[0].requires_grad and not any(t.requires_grad for t in out[1:])
        out[0].backward()
        return out, s.grad

    def restate(got, a, old, ref, w, l, h, du, b, nm):
        return pg.positions(got["step"], lnh, got["barred"], got["cum"], a, c["vid_off"], w, old, ref, l, h, du, b, nm)

    # every advantage 0 and kl_beta 0: seq_nll's bits, the loss and the gradient included; pos_w is w at the scored positions
    zero, d_zero = run(a=torch.zeros_like(adv), b=0.0)
    for a, b in zip(zero[:4], base):
        assert _same(a, b)
    assert _same(d_zero, d_base) and not bool(zero[5].any()) and not bool(zero[7].any())
    scored = torch.arange(S, device=DEV)[None, :] < ln[:, None]
    assert _same(zero[4], torch.where(scored, wd[:, None].expand(R, S), torch.zeros((), device=DEV)).contiguous())
    # svpc_seq_pos_bwd with pos_w[r, :] = row_w[r] everywhere and dead = barred: svpc_seq_nll_bwd's bits
    flat = wd[:, None].expand(R, S).contiguous()
    dsc = torch.full(sd.shape, float("nan"), dtype=torch.float32, device=DEV)
    one = torch.ones((), dtype=torch.float32, device=DEV)
    ops._lib.call("seq_pos_bwd", ops._p(sd), sd.stride(0), ops._p(rcx.dev(sd.device)), int(max(c["row_c"])), ops._p(tgt), ops._p(ln),
                  ops._p(base[3]), ops._p(flat), ops._p(one), R, Lt, 1 if logits else 0, UNK, ops._p(dsc), dsc.shape[1], ops._stream())
    assert _same(dsc, d_base)
    # the full objective
    out, d = run()
    for a, b in zip(out[1:4], base[1:]):
        assert _same(a, b)
    got = _np(out)
    assert sorted(np.nonzero(got["barred"])[0].tolist()) == sorted(c["bar_rows"])
    ref = restate(got, c["adv"], old_np if with_old else None, c["ref_step"] if with_ref else None, c["w"], lo, hi, dual, beta, norm)
    exact = {(r // K, r % K, p) for r, p in c["exact"]} if with_old else set()
    assert pg.bound_distance(ref, lo, hi, dual, exact) > gc.BOUND_MARGIN                 # (condition on the seeded inputs)
    assert all(ref["rho"][e] == 1.0 for e in exact if ref["scored"][e])
    _check(got, ref, c["w"], S)
    assert with_old or not got["n_clip"].any()
    # dscores: −pos_w / p at the target column (probabilities: bit for bit), pos_w·(softmax without UNK − [c = y]) (logits)
    assert bool(torch.isfinite(d).all())
    live = (scored & (out[3] == 0)[:, None]).reshape(-1)                       # (R·S,) the positions with a gradient row
    rows = (torch.arange(R, device=DEV)[:, None] * Lt + torch.arange(S, device=DEV)[None, :]).reshape(-1)
    ycol = tgt[:, 1:].reshape(-1).long().clamp(0, sd.shape[1] - 1)
    pw = out[4].reshape(-1).double()
    expect = torch.zeros(sd.shape, dtype=torch.float64, device=DEV)
    if logits:
        keep = torch.arange(sd.shape[1], device=DEV)[None, :] < torch.from_numpy(c["row_c"]).to(DEV).repeat_interleave(S)[:, None]
        keep[:, UNK] = False
        z = sd[rows].double().masked_fill(~keep, float("-inf"))
        g = torch.softmax(z, 1)
        g[torch.arange(len(rows)), ycol] -= 1.0
        expect[rows[live]] = (g * pw[:, None])[live]
        scale = expect.abs().amax(1, keepdim=True)
        assert bool(((d.double() - expect).abs() <= 1e-6 * scale + 1e-30).all())
        assert not bool(d[expect.abs().amax(1) == 0].any())
    else:
        expect[rows[live], ycol[live]] = (-pw / sd[rows, ycol].double())[live]
        assert _same(d, expect.float())
    # no old_step, kl_beta 0, norm "none", no likelihood weights: seq_nll's gradient under row_w = fp32(A / (N·K)), nothing clipped
    rf, d_rf = run(old=None, ref=None, w=None, b=0.0, nm="none")
    a_rows = np.where(rf[9].cpu().numpy() == 1, c["adv"], 0.0)[ref["row_vid"]]  # (T, K): A of a valid candidate, 0 otherwise
    w3 = torch.from_numpy((a_rows / np.float64(N * K)).astype(np.float32).reshape(-1)).to(DEV)
    _, d_w3 = nll(w3)
    assert _same(d_rf, d_w3) and not bool(rf[7].any())
    assert bool((rf[8][rf[8] != 0] == 1.0).all())
    # ref_step equal to the pass's own step, bit for bit: kl is exactly 0
    own, _ = run(old=None, ref=torch.nan_to_num(out[2].clone(), neginf=0.0), b=0.04)
    assert not bool(own[6].any())
    # an absent old_step is ρ = 1 exactly: the bits of old_step = the pass's own step
    if with_old:
        a1, d1 = run(old=None)
        a2, d2 = run(old=torch.nan_to_num(out[2].clone(), neginf=0.0))
        assert all(_same(x, y) for x, y in zip(a1, a2)) and _same(d1, d2)
    # the other norms and clip settings on the same inputs, against the restatement
    for nm, l, h, du, b in gc.ALT_SETTINGS:
        if (nm, l, h, du, b) == (norm, lo, hi, dual, beta):
            continue
        b = b if with_ref else 0.0
        alt, _ = run(l=l, h=h, du=du, b=b, nm=nm)
        g2 = _np(alt)
        r2 = restate(g2, c["adv"], old_np if with_old else None, c["ref_step"] if with_ref else None, c["w"], l, h, du, b, nm)
        assert pg.bound_distance(r2, l, h, du, exact) > gc.BOUND_MARGIN
        _check(g2, r2, c["w"], S)
    # twice the same bits
    again, d_again = run()
    assert all(_same(a, b) for a, b in zip(out, again)) and _same(d, d_again)


@pytest.mark.parametrize("rule", pg.RULES)
def test_group_advantage(rule):
    rng = np.random.default_rng(5)
    for N, K in ((1, 1), (3, 2), (70, 3), (300, 16)):
        r = rng.standard_normal((N, K))
        if K >= 3:
            r[0, 1], r[N - 1, 0], r[N // 2, :] = np.nan, np.inf, 0.25
            r[1 % N, 1:] = -np.inf
        got = ops.group_advantage(torch.from_numpy(r).to(DEV), rule, 1e-6).cpu().numpy()
        want = pg.group_advantage(r, rule, 1e-6)
        assert np.array_equal(got == 0, want == 0) and not np.signbit(got[want == 0]).any()
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    for rr in ([[0.7]], [[0.3, 0.3, 0.3]], [[np.nan, 1.5, np.inf]], [[np.nan, -np.inf, np.inf]]):
        got = ops.group_advantage(torch.tensor(rr, dtype=torch.float64, device=DEV), rule)
        assert not bool(got.any())


def test_host_checks_on_the_device():
    C, Lt, K, steps = 9, 3, 2, [2, 1]
    c = gc.score_case(7, C, Lt, K, steps, False, False)
    sd = torch.from_numpy(c["scores"]).to(DEV)
    _, _, tgt, ln, _ = ops.force_inputs(torch.from_numpy(c["ids"]).to(DEV).view(3, K, Lt), C, UNK, EOS, PAD, IGNORE)
    adv = torch.from_numpy(c["adv"]).to(DEV)
    old = torch.from_numpy(c["old_step"]).to(DEV)
    tail = (None, False, UNK, 0.2, 0.2, 0.0, 0.0, "sequence")
    args = lambda a, off, o=old, rf=None, tl=tail: (sd, Idx(c["row_c"].tolist()), tgt, ln, a, off, o, rf) + tl  # noqa: E731
    for a, off in ((adv, [0, 3]), (adv, [0, 2, 4]), (adv[:, :1].contiguous(), [0, 2, 3]), (adv.float(), [0, 2, 3]), (adv, [0, 3, 2])):
        with pytest.raises(ValueError):
            ops.seq_pg(*args(a, off))
    for bad in (old.double(), old[:5], old.cpu(), torch.zeros(12, 2, dtype=torch.float32, device=DEV)[::2]):
        with pytest.raises(ValueError):
            ops.seq_pg(*args(adv, [0, 2, 3], o=bad))
        with pytest.raises(ValueError):
            ops.seq_pg(*args(adv, [0, 2, 3], rf=bad))
    for tl in (tail[:3] + (1.0,) + tail[4:], tail[:4] + (-0.1,) + tail[5:], tail[:5] + (1.0,) + tail[6:], tail[:6] + (0.04, "sequence"),
               tail[:7] + ("mean",)):
        with pytest.raises(ValueError):
            ops.seq_pg(*args(adv, [0, 2, 3], tl=tl))
    out = ops.seq_pg(*args(adv, [0, 2, 3]))
    assert len(out) == 11 and tuple(out[4].shape) == (6, 2) and tuple(out[9].shape) == (2, K) and tuple(out[7].shape) == (6, 2)
    ops.seq_pg(*args(adv, [0, 2, 3], o=old.view(3, K, 2), rf=old.view(-1), tl=tail[:6] + (0.04, "token")))       # (any contiguous shape)


# ------------------------------------------------------------------------------------------------ 2. the graded forced pass
def _translator(cfg, model, **kw):
    from svpc_amd.translator import Translator
    O = type("O", (), {"cuda": True})
    return Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, **kw)


def _weights(steps, K):
    T = sum(steps)
    w = [[(-1.0) ** (t + k) * (0.05 + 0.01 * ((3 * t + k) % 7)) for k in range(K)] for t in range(T)]
    return torch.tensor(w, dtype=torch.float32)


def _adv(N, K):
    """hand-set advantages of both signs, one exact zero (video 0, candidate K − 1 when K > 1)"""
    a = torch.tensor([[(-1.0) ** (b + k) * (0.4 + 0.3 * ((b + 2 * k) % 3)) for k in range(K)] for b in range(N)], dtype=torch.float64)
    if K > 1:
        a[0, K - 1] = 0.0
    return a


def _moved(step, seed, scale):
    """a frozen policy's step scores: the given ones moved by a seeded draw (the same offsets as the kernel cases use)"""
    rng = np.random.default_rng(seed)
    s = step.cpu().numpy().astype(np.float64)
    off = gc._offsets(rng, s.shape) if scale is None else rng.standard_normal(s.shape) * scale
    return torch.from_numpy(np.where(np.isfinite(s), s + off, s).astype(np.float32)).to(DEV)


def _candidates(tr, batch, K, seed=2):
    """the fixture's gold rows, then sampled rows of a fixed seed"""
    gold = tr.gold_captions(batch["input_labels_list"], batch["batch_step_num"])
    if K == 1:
        return [g.unsqueeze(1).contiguous() for g in gold]
    sample = tr.translate_batch_sample(syn.translate_inputs(batch), num_samples=4, seed=seed)[0]
    return [torch.cat([g.unsqueeze(1), s[:, :K - 1]], 1).contiguous() for g, s in zip(gold, sample)]


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


LOSS_KW = dict(clip_lo=0.2, clip_hi=0.28, dual_clip=3.0, kl_beta=0.04, norm="sequence")
CASES = [("tiny", "v"), ("tiny", "vi"), ("tiny", "viv"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")]


def _restate(r, adv, steps, w, old, ref, kw):
    Lt1 = r.step.shape[-1]
    flat = lambda t: None if t is None else t.cpu().numpy().reshape(-1, Lt1)  # noqa: E731
    return pg.positions(r.step.cpu().numpy().reshape(-1, Lt1), r.length.cpu().numpy().reshape(-1), r.barred.cpu().numpy().reshape(-1),
                        r.cum.cpu().numpy().reshape(-1), adv.cpu().numpy(), gc.vid_off(steps), None if w is None else w.cpu().numpy().reshape(-1),
                        flat(old), flat(ref), kw["clip_lo"], kw["clip_hi"], kw["dual_clip"], kw["kl_beta"], kw["norm"])


def _got(r):
    return dict(loss=r.loss.detach().cpu().numpy(), pos_w=r.pos_w.cpu().numpy(), pg=r.pg.cpu().numpy(), kl=r.kl.cpu().numpy(),
                n_clip=r.n_clip.cpu().numpy(), ratio_max=r.ratio_max.cpu().numpy(), valid=r.valid.cpu().numpy(), n_tok=r.n_tok.cpu().numpy())


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("case,mt", CASES)
def test_policy_loss_vs_sequence_loss(golden_dir, case, mt, K):
    z, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    tr = _translator(cfg, model)
    steps = [int(s) for s in batch["batch_step_num"]]
    N = len(steps)
    caps = _candidates(tr, batch, K)
    w, adv = _weights(steps, K).to(DEV), _adv(N, K).to(DEV)
    inputs = syn.translate_inputs(batch)
    before = [[t.clone() for t in inputs[0]], [t.clone() for t in inputs[2]]]
    own = policy.position_scores(tr, inputs, caps)
    old, ref = _moved(own, 11, None), _moved(own, 12, 0.3)
    model.zero_grad(set_to_none=True)
    r = policy.policy_loss(tr, inputs, caps, adv, old_step=old, ref_step=ref, weights=w, **LOSS_KW)
    r.loss.backward()
    ops.join_side()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before[0], inputs[0])) and all(torch.equal(a, b) for a, b in zip(before[1], inputs[2]))
    assert any(bool((t[:, cfg.max_v_len:] != PAD).any()) for t in inputs[0])
    g_full = _grads(model)
    assert len(g_full) > 20 and all(bool(torch.isfinite(g).all()) for g in g_full.values())

    def parent(weights):
        model.zero_grad(set_to_none=True)
        s = scst.sequence_loss(tr, syn.translate_inputs(batch), caps, weights)
        s.loss.backward()
        ops.join_side()
        torch.cuda.synchronize()
        return s, _grads(model)

    s0, _ = parent(w)
    assert _same(r.cum, s0.cum) and torch.equal(r.barred, s0.barred) and _same(r.step, s0.step) and torch.equal(r.length, s0.length)
    rs = _restate(r, adv, steps, w, old, ref, LOSS_KW)
    assert pg.bound_distance(rs, LOSS_KW["clip_lo"], LOSS_KW["clip_hi"], LOSS_KW["dual_clip"]) > gc.BOUND_MARGIN
    _check(_got(r), rs, w.cpu().numpy(), cfg.max_t_len - 1)
    assert rs["n_clip"].any() and rs["kl"].any()
    # on-policy, norm "none", no KL: the parameter gradients are the parent path's under row weights fp32(A / (N·K)), calibrated on the
    # parent path alone (``test_pref_gpu.py``'s procedure: a tensor two parent runs agree on in bits must come out in those bits, any
    # other within twice their difference; the atomically accumulated word-embedding gradient has a floor from the number format)
    model.zero_grad(set_to_none=True)
    q = policy.policy_loss(tr, syn.translate_inputs(batch), caps, adv, norm="none")
    q.loss.backward()
    ops.join_side()
    torch.cuda.synchronize()
    g_pg = _grads(model)
    a_valid = torch.where(q.valid == 1, adv, torch.zeros_like(adv))
    rows = torch.repeat_interleave(a_valid, torch.tensor(steps, device=DEV), 0) / float(N * K)  # (T, K) float64
    w3 = rows.float()
    assert not bool(q.n_clip.any()) and _same(q.pos_w, torch.where(torch.arange(cfg.max_t_len - 1, device=DEV) < q.length[:, :, None],
                                                                   w3[:, :, None], torch.zeros((), device=DEV)).contiguous())
    s1, g1 = parent(w3)
    s2, g2 = parent(w3)
    assert set(g1) == set(g2) == set(g_pg) and len(g1) > 20
    tol = {n: 2.0 * float((g1[n] - g2[n]).abs().max()) for n in g1}
    atomic = [n for n in g1 if n == "text_embeddings.word_embeddings.weight"]
    if atomic:
        runs = [g1, g2, parent(w3)[1], parent(w3)[1]]
        ids = torch.cat([c.reshape(-1) for c in caps])
        ids = torch.where(ids >= cfg.vocab_size, torch.full_like(ids, UNK), ids)
        m = int(torch.bincount(ids[ids != PAD]).max())
        for n in atomic:
            four = max(float((a[n] - b[n]).abs().max()) for i, a in enumerate(runs) for b in runs[i + 1:])
            tol[n] = max(2.0 * four, 2.0 * (m - 1) * 2.0 ** -24 * float(g1[n].abs().max()))
    for n in g1:
        if tol[n] == 0.0:
            assert _same(g_pg[n], g1[n]), n
        else:
            assert float((g_pg[n] - g1[n]).abs().max()) <= tol[n], (n, float((g_pg[n] - g1[n]).abs().max()), tol[n])


def test_position_scores(golden_dir):
    import test_ensemble_gpu as te
    z, cfg, batch, model = build_model("tiny", "vivt", golden_dir, DEV)
    tr = _translator(cfg, model)
    caps = _candidates(tr, batch, 3)
    other = te._other_model(golden_dir, "tiny", "vivt")
    T = sum(int(s) for s in batch["batch_step_num"])
    for scorer in (_translator(cfg, other), te._ensemble(cfg, [model, other])):
        inputs = syn.translate_inputs(batch)
        before = [[t.clone() for t in inputs[0]], [t.clone() for t in inputs[2]]]
        members = scorer._members()
        members[-1].train()
        try:
            got = policy.position_scores(scorer, inputs, caps)
            assert members[-1].training and not got.requires_grad           # the mode is restored; the pass ran without gradients …
        finally:
            members[-1].eval()
        assert all(torch.equal(a, b) for a, b in zip(before[0], inputs[0])) and all(torch.equal(a, b) for a, b in zip(before[1], inputs[2]))
        sc = scorer.score_captions(syn.translate_inputs(batch), caps)
        assert got.dtype == torch.float32 and tuple(got.shape) == (T, 3, cfg.max_t_len - 1)
        assert _same(got, sc.step) and got.data_ptr() != sc.step.data_ptr()    # … in eval mode: score_captions' bits, in a buffer of its own
    # with graph=True the pass's buffer belongs to the captured graph: the clone survives the next replay
    trg = _translator(cfg, other, graph=True)
    a = policy.position_scores(trg, syn.translate_inputs(batch), caps)
    keep = a.clone()
    caps2 = [torch.flip(c, [1]).contiguous() for c in caps]                    # (other captions in every row: the replay writes other scores)
    b = policy.position_scores(trg, syn.translate_inputs(batch), caps2)
    assert _same(a, keep) and not _same(a, b) and a.data_ptr() != b.data_ptr()


# ------------------------------------------------------------------------------------------------ 3. the step, end to end
#          source, K, decode keywords, reference, advantage, loss keywords
STEPS = [("sample", 3, dict(seed=17), "second", "grpo", dict(kl_beta=0.04)),                                                   # GRPO
         ("nbest", 3, {}, "ensemble", "center", dict(kl_beta=0.04, norm="none")),                                              # Dr. GRPO with a KL
         ("diverse", 4, dict(num_groups=2, diversity_strength=0.5), None, "rloo", dict(clip_hi=0.28, norm="token")),           # DAPO's loss
         ("stochastic", 3, dict(seed=17), "self", "grpo", dict(kl_beta=0.04, dual_clip=3.0))]
DEFAULTS = dict(clip_lo=0.2, clip_hi=0.2, dual_clip=0.0, kl_beta=0.0, norm="sequence")

# The policy as its own behaviour policy (eval mode, fp32, no optimiser step between): ρ = exp(step − old_step) compares the graded pass's
# and the forced pass's log-probability of the same positions — two code paths over the same parameters, so it is near 1 but need not be 1.
# The largest |ρ − 1| over ("tiny", "c1") × STEPS, measured on the MI355X (profiles/policy_parity.json); the assertion is at twice that.
MEASURED_SELF = 1.3351529560612363e-05                # ("c1", "sample": a few fp32 ulps of a step score; "tiny" 1.7e-6)


def _decoder_output(tr, batch, source, K, kw):
    inputs = syn.translate_inputs(batch)
    if source == "sample":
        return tr.translate_batch_sample(inputs, num_samples=K, **kw)[0]
    if source == "nbest":
        return tr.translate_batch_nbest(inputs, K, K)[0]
    if source == "diverse":
        return tr.translate_batch_diverse(inputs, K, kw["num_groups"], kw["diversity_strength"], K // kw["num_groups"])[0]
    return tr.translate_batch_stochastic(inputs, K, **kw)[0]


@pytest.mark.parametrize("source,K,kw,refkind,advantage,loss_kw", STEPS)
@pytest.mark.parametrize("case", ["tiny", "c1"])
def test_policy_step_end_to_end(golden_dir, case, source, K, kw, refkind, advantage, loss_kw):
    import test_ensemble_gpu as te
    import test_pref_gpu as tp
    from svpc_amd.graph import backward_all
    from svpc_amd.optim import FusedBertAdam
    z, cfg, batch, model = build_model(case, "vivt", golden_dir, DEV)
    tr = _translator(cfg, model)
    reference = None
    if refkind == "second":
        reference = _translator(cfg, te._other_model(golden_dir, case, "vivt"))
    elif refkind == "ensemble":
        reference = te._ensemble(cfg, [build_model(case, "vivt", golden_dir, DEV)[3], te._other_model(golden_dir, case, "vivt")])
    elif refkind == "self":
        reference = tr
    corpus, videos, _, _, _ = tp._corpus(cfg, batch)
    steps = [int(s) for s in batch["batch_step_num"]]
    N, T, S = len(steps), sum(steps), cfg.max_t_len - 1
    po = policy.PolicyOptimization(tr, corpus, reference=reference)
    opt = FusedBertAdam(list(model.named_parameters()), lr=1e-4, warmup=0.1, t_total=100, grad_clip=1.0)
    opt.zero_grad()
    inputs = syn.translate_inputs(batch)
    before = [[t.clone() for t in inputs[0]], [t.clone() for t in inputs[2]]]
    call = dict(num_candidates=K, source=source, advantage=advantage, **kw, **loss_kw)
    full = dict(DEFAULTS, **loss_kw)
    assert not model.training
    po.phase_events = []
    r = po.step(inputs, videos, **call)
    assert len(po.phase_events) == 7
    po.phase_events = None
    assert not model.training
    assert all(torch.equal(a, b) for a, b in zip(before[0], inputs[0])) and all(torch.equal(a, b) for a, b in zip(before[1], inputs[2]))
    # the candidates: the named decoder's output; the rewards: MinimumRisk's; the advantages: the restatement's of those rewards
    want = _decoder_output(tr, batch, source, K, kw)
    assert all(torch.equal(d, w_) for d, w_ in zip(r.dec_seq_list, want))
    plan = corpus.plan(list(videos))
    reward = torch.stack([tr.caption_scores(r.dec_seq_list, plan, row=k)[:, 5] for k in range(K)], 1)
    assert r.reward.dtype == torch.float64 and torch.equal(r.reward, reward)
    want_adv = pg.group_advantage(reward.cpu().numpy(), advantage, 1e-6)
    got_adv = r.adv.cpu().numpy()
    assert np.array_equal(got_adv == 0, want_adv == 0)
    np.testing.assert_allclose(got_adv, want_adv, rtol=1e-12, atol=0)
    # the behaviour policy's and the reference's step scores: score_captions' of the returned candidates
    assert _same(r.old_step, tr.score_captions(syn.translate_inputs(batch), r.dec_seq_list).step)
    if reference is None:
        assert r.ref_step is None
    else:
        assert _same(r.ref_step, reference.score_captions(syn.translate_inputs(batch), r.dec_seq_list).step)
    # the loss head: the restatement fed the step's own step scores and advantages
    rs = _restate(r, r.adv, steps, None, r.old_step, r.ref_step, full)
    dev1 = float(np.nanmax(np.abs(rs["rho"] - 1.0))) if rs["scored"].any() else 0.0
    print("self behaviour policy %s %s: largest |rho - 1| %.6e" % (case, source, dev1))
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "policy_self_%s_%s.json" % (case, source)), "w") as f:
        json.dump(dict(case=case, source=source, K=K, largest_abs_rho_minus_1=dev1, measured=MEASURED_SELF), f, indent=1)
    assert dev1 <= 2.0 * MEASURED_SELF, dev1
    assert pg.bound_distance(rs, full["clip_lo"], full["clip_hi"], full["dual_clip"]) > gc.BOUND_MARGIN and not rs["n_clip"].any()
    _check(_got(r), rs, None, S)
    assert tuple(r.pos_w.shape) == (T, K, S) and tuple(r.cum.shape) == (T, K) and tuple(r.n_clip.shape) == (T, K, 2)
    # the same call again: the same candidates, the same bits
    r2 = po.step(syn.translate_inputs(batch), videos, **call)
    assert all(torch.equal(a, b) for a, b in zip(r.dec_seq_list, r2.dec_seq_list))
    assert _same(r.loss, r2.loss) and _same(r.pos_w, r2.pos_w) and torch.equal(r.adv, r2.adv)
    # gradients: finite, not zero whenever some position has a weight; the optimizer steps
    backward_all(model, r.loss)
    ops.join_side()
    gsq = sum(float(p.grad.double().pow(2).sum()) for p in model.parameters() if p.grad is not None)
    # (beam candidates of an untrained model can all score the same reward: then every advantage is exactly 0)
    assert bool(r.pos_w.any()) or source in ("nbest", "diverse"), "every weight is zero: the gradient check below would be empty"
    assert np.isfinite(gsq) and (gsq > 0) == bool(r.pos_w.any()), gsq
    opt.step()
    # on_policy=True: no behaviour pass, ρ exactly 1
    r4 = po.step(syn.translate_inputs(batch), videos, on_policy=True, **call)
    assert r4.old_step is None and not bool(r4.n_clip.any()) and bool((r4.ratio_max[r4.ratio_max != 0] == 1.0).all())
    # train mode: dropout on, runs and stays finite; decode and the scoring passes ran in eval mode and the mode is restored.  The policy
    # as its own reference is refused in train mode.
    model.train()
    try:
        opt.zero_grad()
        if refkind == "self":
            with pytest.raises(ValueError):
                po.step(syn.translate_inputs(batch), videos, **call)
        else:
            r3 = po.step(syn.translate_inputs(batch), videos, **call)
            assert model.training
            backward_all(model, r3.loss)
            ops.join_side()
            opt.step()
            torch.cuda.synchronize()
            assert np.isfinite(float(r3.loss.detach()))
            assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    finally:
        model.eval()


@pytest.mark.parametrize("case", ["tiny", "c1"])
def test_two_updates_on_one_rollout(golden_dir, case):
    import test_ensemble_gpu as te
    import test_pref_gpu as tp
    from svpc_amd.graph import backward_all
    from svpc_amd.optim import FusedBertAdam
    z, cfg, batch, model = build_model(case, "vivt", golden_dir, DEV)
    tr = _translator(cfg, model)
    corpus, videos, _, _, _ = tp._corpus(cfg, batch)
    po = policy.PolicyOptimization(tr, corpus, reference=_translator(cfg, te._other_model(golden_dir, case, "vivt")))
    opt = FusedBertAdam(list(model.named_parameters()), lr=1e-3, grad_clip=1.0)              # (t_total = −1: a constant rate)
    ro = po.collect(syn.translate_inputs(batch), videos, num_candidates=3, source="sample", seed=17)
    assert bool(ro.adv.any())
    keep = [ro.old_step.clone(), ro.ref_step.clone(), ro.adv.clone()]
    devs = []
    for it in range(2):
        opt.zero_grad()
        r = po.update(ro, syn.translate_inputs(batch), kl_beta=0.04)
        backward_all(model, r.loss)
        ops.join_side()
        opt.step()
        torch.cuda.synchronize()
        assert np.isfinite(float(r.loss.detach()))
        live = r.ratio_max[r.ratio_max != 0]
        devs.append(float((live - 1.0).abs().max()))
    # the first update sees the behaviour policy itself (ρ within rounding of 1), the second the stepped policy: ρ ≠ 1 and a finite loss
    assert devs[0] <= 2.0 * MEASURED_SELF and devs[1] > 100.0 * max(devs[0], 1e-7), devs
    assert all(_same(a, b) for a, b in zip(keep[:2], (ro.old_step, ro.ref_step))) and torch.equal(keep[2], ro.adv)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_step_argument_rules(golden_dir):
    import test_pref_gpu as tp
    z, cfg, batch, model = build_model("tiny", "vivt", golden_dir, DEV)
    tr = _translator(cfg, model)
    corpus, videos, _, _, _ = tp._corpus(cfg, batch)
    po = policy.PolicyOptimization(tr, corpus)
    bad = [dict(source="greedy"), dict(utility="METEOR"), dict(num_candidates=17), dict(advantage="zscore"), dict(clip_lo=1.0),
           dict(source="nbest", seed=3), dict(source="diverse", num_candidates=3, num_groups=2), dict(kl_beta=0.04), dict(norm="mean")]
    for kw in bad:
        with pytest.raises(ValueError):
            po.step(syn.translate_inputs(batch), videos, **kw)
    with pytest.raises(TypeError):
        po.step(syn.translate_inputs(batch), videos, source="sample", no_such_keyword=1)
    assert not model.training


# ------------------------------------------------------------------------------------------------ 4. bf16x3
# bf16x3 at the config-1 shape against the fp32 restatement, measured on the MI355X over ("c1", "v") and ("c1", "vivt"), K = 3
# (profiles/policy_parity.json), DESIGN §11.18's procedure: the fp32 side is the CPU oracle's forced pass
# (``pg_reference.sequence_position_loss``): its step scores through the restatement give the loss and the weights per position, and the
# oracle's gradients under those weights are the reference gradients.  The assertion is at twice the measured worst.
MEASURED_X3 = dict(loss=2.0483742931878117e-06,              # ("c1", "vivt")
                   grad=0.15644380787866122,               # ("c1", "vivt"), step_wise_encoder.layer.1.attention.self.query.bias: small against the model's largest
                   grad_zero=0.0003131984878599307)       # ("c1", "vivt"): the zero-in-theory tensors, as a fraction of the model's largest gradient
BOUND_X3 = {k: 2.0 * v for k, v in MEASURED_X3.items()}


@pytest.mark.parametrize("mt", ["v", "vivt"])
def test_bf16x3_deviation_at_config_1(golden_dir, mt):
    import test_scst_gpu as ts
    K = 3
    z, cfg, batch, model = build_model("c1", mt, golden_dir, DEV)
    steps = [int(s) for s in batch["batch_step_num"]]
    N, S = len(steps), cfg.max_t_len - 1
    tr32 = _translator(cfg, model)
    caps = _candidates(tr32, batch, K)                                         # the captions and the frozen policies' scores: made once, in fp32
    own = policy.position_scores(tr32, syn.translate_inputs(batch), caps)
    old, ref = _moved(own, 11, None), _moved(own, 12, 0.3)
    w, adv = _weights(steps, K), _adv(N, K)
    # the fp32 restatement: the oracle's step scores → the restatement's loss and pos_w → the oracle's gradients under pos_w
    names = {n for n, _ in model.named_parameters()}
    P = {k: v.detach().cpu().clone().requires_grad_(k in names and v.is_floating_point()) for k, v in model.state_dict().items()}
    cb = ts._cpu(batch)
    args = (P, cfg, cb["input_ids_list"], cb["video_features_list"], cb["input_masks_list"], cb["ingr_input_ids"], cb["ingr_sep_masks"], steps,
            cb["ingr_id_dict"], cb["oov_word_dict"], [x.cpu().numpy() for x in caps])
    with torch.no_grad():
        _, step0, len0, bar0 = pg.sequence_position_loss(*args, None)
    cum0 = np.asarray([step0[r, :len0[r]].astype(np.float64).sum() for r in range(len(len0))], np.float32)
    rs = pg.positions(step0, len0, bar0, cum0, adv.numpy(), gc.vid_off(steps), w.numpy().reshape(-1), old.cpu().numpy().reshape(-1, S),
                      ref.cpu().numpy().reshape(-1, S), LOSS_KW["clip_lo"], LOSS_KW["clip_hi"], LOSS_KW["dual_clip"], LOSS_KW["kl_beta"],
                      LOSS_KW["norm"])
    surrogate, _, _, _ = pg.sequence_position_loss(*args, rs["pos_w"].reshape(-1, S))
    surrogate.backward()
    ref_grads = {n: (P[n].grad.clone() if P[n].grad is not None else None) for n in names}
    ref_loss = float(rs["total"])
    ops.set_precision("bf16x3")
    try:
        _, _, _, model_x3 = build_model("c1", mt, golden_dir, DEV)
        tr = _translator(cfg, model_x3)
        model_x3.zero_grad(set_to_none=True)
        r = policy.policy_loss(tr, syn.translate_inputs(batch), caps, adv.to(DEV), old_step=old, ref_step=ref, weights=w.to(DEV), **LOSS_KW)
        r.loss.backward()
        ops.join_side()
        torch.cuda.synchronize()
        loss = float(r.loss.detach())
        np.testing.assert_array_equal(r.barred.cpu().numpy().reshape(-1).astype(bool), np.asarray(bar0).astype(bool))
        gmax = max(float(g.abs().max()) for g in ref_grads.values() if g is not None)
        err, name, n, err0, name0 = ts._grad_errors(model_x3, ref_grads, mt, zero_scale=gmax)
    finally:
        ops.set_precision("fp32")
    rel = abs(loss - ref_loss) / abs(ref_loss)
    print("bf16x3 c1 %s: loss %.7g (restatement %.7g, rel %.3e); worst gradient error %.3e of its tensor's max (%s); zero in theory %.3e of the "
          "model's largest gradient (%s)" % (mt, loss, ref_loss, rel, err, name, err0, name0))
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "policy_parity_%s.json" % mt), "w") as f:
        json.dump(dict(case="c1", mt=mt, K=K, precision="bf16x3", loss=loss, restatement_loss=ref_loss, loss_rel_error=rel,
                       worst_grad_error=err, worst_grad_tensor=name, worst_zero_in_theory_error=err0, worst_zero_in_theory_tensor=name0,
                       tensors=n, bound=BOUND_X3, **LOSS_KW), f, indent=1)
    assert n > 20 and rel <= BOUND_X3["loss"] and err <= BOUND_X3["grad"] and err0 <= BOUND_X3["grad_zero"], (rel, err, name, err0, name0)
