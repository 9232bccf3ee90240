"""Preference optimisation on the MI355X: svpc_seq_pref_fwd against ``ops.seq_nll`` (bit for bit where the definition
says so) and the restatement (tests/pref_reference.py) on the seeded inputs of tests/pref_cases.py; ``prefopt.preference_loss`` against
``scst.sequence_loss`` — the parent path ``test_scst_gpu.py`` pins to the oracle —; ``reference_scores``; ``PreferenceOptimization.step``
end to end for the four candidate sources and the four kinds of reference; and the bf16x3 deviation.

Bounds.  cum / step / barred, and with ``pref_weight`` = 0 the loss and dscores: ``seq_nll``'s bits.  dscores: ``seq_nll``'s backward under
the returned w_eff, bit for bit.  valid, n_pairs, n_correct: exact.  pref / reward / margin: rtol 1e-12 of the restatement fed the kernel's
own cum.  w_eff: one fp32 ulp plus 1e-12·(|w| + max|G| / N) for the cancellation.  loss: one fp32 ulp.  Conditions on the inputs, asserted
from the restatement (tests/test_pref_host.py on its own cum, this file on the kernel's): no hinge argument 1 − h and no d lies within 1e-9
of 0 (the active set or n_correct could flip), and every hinge / ipo pref[b] is at least 1e-3·(β·max|u| + 1)
(``pref_reference.pref_conditioning``).  Model level: the parameter gradients of ``preference_loss`` against those of
``sequence_loss(weights=w_eff)``, compared and calibrated exactly as ``test_risk_gpu.test_risk_loss_vs_sequence_loss`` does.  Measured
bounds: see ``MEASURED_SELF`` and ``MEASURED_X3``."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import caption_scores_reference as cs  # noqa: E402
import pref_cases as pc  # noqa: E402
import pref_reference as pr  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import ops, prefopt, scst, synthetic as syn  # noqa: E402
from svpc_amd.ops_common import Idx  # noqa: E402
from svpc_amd.synthetic import EOS, IGNORE, PAD, UNK  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPORT_DIR = os.environ.get("SVPC_REPORT_DIR") or os.path.join(ROOT, "reports")
RHO = 0.7
LN2 = math.log(2.0)
NAMES = ("loss", "cum", "step", "barred", "pref", "reward", "valid", "n_pairs", "n_correct", "margin", "w_eff")


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def _check_groups(got, ref, w, N):
    """pref / reward / margin / valid / n_pairs / n_correct / w_eff / loss of a kernel run (numpy) against the restatement fed the kernel's
    own cum"""
    for k in ("valid", "n_pairs", "n_correct"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    for k in ("pref", "reward", "margin"):
        assert np.isfinite(got[k]).all(), k
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-12, atol=0, err_msg=k)
    assert not got["reward"][ref["valid"] == 0].any()
    gmax = float(np.abs(ref["G"]).max()) if ref["G"].size else 0.0
    want = ref["w_eff"].reshape(-1)
    tol = np.spacing(np.abs(want)).astype(np.float64) + 1e-12 * (np.abs(w.reshape(-1).astype(np.float64)) + gmax / max(N, 1))
    err = np.abs(got["w_eff"].reshape(-1).astype(np.float64) - want.astype(np.float64))
    assert (err <= tol).all(), (float(err.max()), int(err.argmax()))
    assert abs(float(got["loss"]) - float(ref["total"])) <= _ulp32(ref["total"]), (float(got["loss"]), float(ref["total"]))


def _conditions(ref, kind, beta):
    assert pr.min_d_distance(ref) > pc.D_MARGIN
    if kind == "hinge":
        assert pr.min_hinge_distance(ref) > pc.HINGE_MARGIN
    if kind in ("hinge", "ipo"):
        assert pr.pref_conditioning(ref, beta) >= pc.PREF_CONDITION


def _np(out):
    return {k: v.detach().cpu().numpy() for k, v in zip(NAMES, out)}


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("i", range(len(pc.KERNEL_CASES)))
def test_kernels(i):
    seed, C, Lt, K, steps, logits, wide, with_ref, lb, beta, gamma, eps, kind, pairs = pc.KERNEL_CASES[i]
    c = pc.score_case(seed, C, Lt, K, steps, logits, wide)
    N, T = len(steps), sum(steps)
    sd = torch.from_numpy(c["scores"]).to(DEV)                                # (under ``wide`` the rows are C + 5 floats apart)
    rcx = Idx(c["row_c"].tolist())
    wd = torch.from_numpy(c["w"]).to(DEV)
    cost = torch.from_numpy(c["cost"]).to(DEV)
    refd = torch.from_numpy(c["ref_cum"]).to(DEV) if with_ref else None
    V = max(UNK + 1, C - 2)
    _, _, tgt, ln, _ = ops.force_inputs(torch.from_numpy(c["ids"]).to(DEV).view(T, K, Lt), V, UNK, EOS, PAD, IGNORE)

    def nll(w):
        s = sd.detach().clone().requires_grad_(True)
        out = ops.seq_nll(s, rcx, tgt, ln, w, logits, UNK)
        out[0].backward()
        return out, s.grad

    def pref(rho=RHO, w=wd, cst=cost, ref=refd, b=beta, g=gamma, e=eps, kd=kind, pm=pairs):
        s = sd.detach().clone().requires_grad_(True)
        out = ops.seq_pref(s, rcx, tgt, ln, cst, c["vid_off"], ref, w, logits, UNK, b, g, e, lb, rho, kd, pm)
        assert out[0].requires_grad and not any(t.requires_grad for t in out[1:])
        out[0].backward()
        return out, s.grad

    base, d_base = nll(wd)
    # pref_weight = 0: seq_nll's bits, the loss and the gradient included; w_eff is w
    zero, d_zero = pref(rho=0.0)
    for a, b in zip(zero[:4], base):
        assert _same(a, b)
    assert _same(d_zero, d_base) and _same(zero[10], wd)
    # the full objective
    out, d = pref()
    for a, b in zip(out[1:4], base[1:]):
        assert _same(a, b)
    got = _np(out)
    assert sorted(np.nonzero(got["barred"])[0].tolist()) == sorted(c["bar_rows"])
    lnh = ln.cpu().numpy()
    ref = pr.groups(got["cum"], lnh, got["barred"], c["cost"], c["vid_off"], c["w"], c["ref_cum"] if with_ref else None, beta, gamma, eps, lb,
                    RHO, kind, pairs)
    _conditions(ref, kind, beta)                                            # (conditions on the seeded inputs)
    _check_groups(got, ref, c["w"], N)
    assert K == 1 or ref["n_pairs"].any()
    # dscores: seq_nll's backward under the returned w_eff, bit for bit
    under, d_under = nll(out[10])
    assert _same(d, d_under) and bool(torch.isfinite(d).all())
    # K = 1 or all costs equal: no pair, G exactly 0, w_eff = w bit for bit
    flat = torch.where(torch.isfinite(cost), torch.full_like(cost, -1.25), cost)
    ex, _ = pref(cst=flat)
    assert _same(ex[10], wd) and not bool(ex[7].any()) and not bool(ex[4].any()) and not bool(ex[8].any()) and not bool(ex[9].any())
    if K == 1:
        assert _same(out[10], wd) and not bool(out[7].any())
    # an absent ref_cum: the bits of an all-zero one
    none, d_none = pref(ref=None)
    zref, d_zref = pref(ref=torch.zeros(T * K, dtype=torch.float32, device=DEV))
    assert all(_same(a, b) for a, b in zip(none, zref)) and _same(d_none, d_zref)
    # the reference equal to the policy's own cum, bit for bit (sigmoid, γ = ε = 0): u = 0, pref = ln 2 in every video with a pair, nothing correct
    own, _ = pref(ref=out[1].clone(), g=0.0, e=0.0, kd="sigmoid", pm="all")
    assert not bool(own[5].any()) and not bool(own[8].any()) and not bool(own[9].any())
    p_own, n_own = own[4].cpu().numpy(), own[7].cpu().numpy()
    # (ln 2 up to the device's log1p, one ulp, and the rounding of at most 15 + 16 additions of equal terms: far inside 1e-14)
    assert (np.abs(p_own[n_own > 0] - LN2) <= 1e-14).all() and not p_own[n_own == 0].any() and (K == 1 or n_own.any())
    # twice the same bits
    again, d_again = pref()
    assert all(_same(a, b) for a, b in zip(out, again)) and _same(d, d_again)


def test_host_checks_on_the_device():
    C, Lt, K, steps = 9, 3, 2, [2, 1]
    c = pc.score_case(7, C, Lt, K, steps, False, False)
    sd = torch.from_numpy(c["scores"]).to(DEV)
    _, _, tgt, ln, _ = ops.force_inputs(torch.from_numpy(c["ids"]).to(DEV).view(3, K, Lt), C, UNK, EOS, PAD, IGNORE)
    cost = torch.from_numpy(c["cost"]).to(DEV)
    ref = torch.from_numpy(c["ref_cum"]).to(DEV)
    tail = (False, UNK, 0.1, 0.0, 0.0, 0.0, 1.0, "sigmoid", "all")
    args = lambda cst, off, rf=ref, tl=tail: (sd, Idx(c["row_c"].tolist()), tgt, ln, cst, off, rf, None) + tl  # noqa: E731
    for cst, off in ((cost, [0, 3]), (cost, [0, 2, 4]), (cost[:, :1].contiguous(), [0, 2, 3]), (cost.float(), [0, 2, 3]), (cost, [0, 3, 2])):
        with pytest.raises(ValueError):
            ops.seq_pref(*args(cst, off))
    for rf in (ref.double(), ref[:5], ref.cpu(), torch.zeros(12, dtype=torch.float32, device=DEV)[::2]):
        with pytest.raises(ValueError):
            ops.seq_pref(*args(cost, [0, 2, 3], rf=rf))
    for tl in ((False, UNK, 0.0) + tail[3:], tail[:4] + (0.1, 0.0, 1.0, "hinge", "all"), tail[:3] + (0.5, 0.0, 0.0, 1.0, "ipo", "all"),
               tail[:7] + ("dpo", "all"), tail[:8] + ("best",), tail[:6] + (-1.0,) + tail[7:]):
        with pytest.raises(ValueError):
            ops.seq_pref(*args(cost, [0, 2, 3], tl=tl))
    out = ops.seq_pref(*args(cost, [0, 2, 3]))
    assert len(out) == 11 and tuple(out[10].shape) == (6,) and tuple(out[5].shape) == (2, K)
    ops.seq_pref(*args(cost, [0, 2, 3], rf=ref.view(3, K)))                 # (any contiguous shape of R elements)


# ------------------------------------------------------------------------------------------------ 2. the graded forced pass
def _translator(cfg, model, **kw):
    from svpc_amd.translator import Translator
    O = type("O", (), {"cuda": True})
    return Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, **kw)


def _weights(steps, K):
    T = sum(steps)
    w = [[(-1.0) ** (t + k) * (0.05 + 0.01 * ((3 * t + k) % 7)) for k in range(K)] for t in range(T)]
    return torch.tensor(w, dtype=torch.float32)


def _costs(N, K):
    """hand-set, distinct inside a video but for one tie (video 0: candidates 0 and K − 1)"""
    c = torch.tensor([[-(0.3 + 0.2 * ((b + 2 * k) % 3) + 0.01 * k) for k in range(K)] for b in range(N)], dtype=torch.float64)
    if K > 1:
        c[0, K - 1] = c[0, 0]
    return c


def _ref_cum(steps, K):
    """hand-set reference scores: between −1 and −2.5 per caption"""
    T = sum(steps)
    return torch.tensor([[-(1.0 + 0.37 * ((3 * t + k) % 5)) for k in range(K)] for t in range(T)], dtype=torch.float32)


def _candidates(tr, batch, K, seed=2):
    """the fixture's gold rows, then sampled rows of a fixed seed"""
    gold = tr.gold_captions(batch["input_labels_list"], batch["batch_step_num"])
    if K == 1:
        return [g.unsqueeze(1).contiguous() for g in gold]
    sample = tr.translate_batch_sample(syn.translate_inputs(batch), num_samples=4, seed=seed)[0]
    return [torch.cat([g.unsqueeze(1), s[:, :K - 1]], 1).contiguous() for g, s in zip(gold, sample)]


def _grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


LOSS_KW = dict(beta=0.1, gamma=0.0, label_smoothing=0.1, length_beta=0.0, pref_weight=1.0, loss_type="sigmoid", pairs="all")
CASES = [("tiny", "v"), ("tiny", "vi"), ("tiny", "viv"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")]


def _restate(r, cost, steps, w, ref_cum, kw):
    return pr.groups(r.cum.cpu().numpy(), r.length.cpu().numpy(), r.barred.cpu().numpy(), cost.cpu().numpy(), pc.vid_off(steps),
                     None if w is None else w.cpu().numpy(), None if ref_cum is None else ref_cum.cpu().numpy(), kw["beta"], kw["gamma"],
                     kw["label_smoothing"], kw["length_beta"], kw["pref_weight"], kw["loss_type"], kw["pairs"])


def _got(r):
    return dict(loss=r.loss.detach().cpu().numpy(), pref=r.pref.cpu().numpy(), reward=r.reward.cpu().numpy(), margin=r.margin.cpu().numpy(),
                valid=r.valid.cpu().numpy(), n_pairs=r.n_pairs.cpu().numpy(), n_correct=r.n_correct.cpu().numpy(), w_eff=r.w_eff.cpu().numpy())


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("case,mt", CASES)
def test_preference_loss_vs_sequence_loss(golden_dir, case, mt, K):
    z, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    tr = _translator(cfg, model)
    steps = [int(s) for s in batch["batch_step_num"]]
    N = len(steps)
    caps = _candidates(tr, batch, K)
    w, cost, ref_cum = _weights(steps, K).to(DEV), _costs(N, K).to(DEV), _ref_cum(steps, K).to(DEV)
    inputs = syn.translate_inputs(batch)
    before = [[t.clone() for t in inputs[0]], [t.clone() for t in inputs[2]]]
    model.zero_grad(set_to_none=True)
    r = prefopt.preference_loss(tr, inputs, caps, cost, ref_cum=ref_cum, weights=w, **LOSS_KW)
    r.loss.backward()
    ops.join_side()
    torch.cuda.synchronize()
    g_pref = _grads(model)
    assert all(torch.equal(a, b) for a, b in zip(before[0], inputs[0])) and all(torch.equal(a, b) for a, b in zip(before[1], inputs[2]))
    assert any(bool((t[:, cfg.max_v_len:] != PAD).any()) for t in inputs[0])

    def parent(weights):
        model.zero_grad(set_to_none=True)
        s = scst.sequence_loss(tr, syn.translate_inputs(batch), caps, weights)
        s.loss.backward()
        ops.join_side()
        torch.cuda.synchronize()
        return s, _grads(model)

    s1, g1 = parent(r.w_eff)
    s2, g2 = parent(r.w_eff)
    assert _same(r.cum, s1.cum) and torch.equal(r.barred, s1.barred) and _same(r.step, s1.step) and torch.equal(r.length, s1.length)
    ref = _restate(r, cost, steps, w, ref_cum, LOSS_KW)
    _conditions(ref, LOSS_KW["loss_type"], LOSS_KW["beta"])
    _check_groups(_got(r), ref, w.cpu().numpy(), N)
    assert K == 1 or (ref["G"] != 0).any()
    if K == 1:
        assert _same(r.w_eff, w)
    # the parameter gradients: those of the parent path under w_eff, calibrated on the parent path alone (never on the new code): two
    # parent runs; a tensor they agree on in bits must come out in those bits, any other within twice their difference.  One exception, for
    # a reason in the parent path itself: the text word-embedding table's gradient is accumulated with fp32 atomics, so its
    # bits change from run to run.  For that tensor the spread is taken over four parent runs and has a floor from the number format:
    # reordering a sum of m fp32 addends moves it by up to 2(m − 1)·2⁻²⁴·Σ|addends| ≥ 2(m − 1)·2⁻²⁴·|sum|, m the gathers of the most frequent word.
    assert set(g1) == set(g2) == set(g_pref) and len(g1) > 20
    spread = {n: float((g1[n] - g2[n]).abs().max()) for n in g1}
    atomic = [n for n in g1 if n == "text_embeddings.word_embeddings.weight"]
    tol = {n: 2.0 * spread[n] for n in g1}
    if atomic:
        runs = [g1, g2, parent(r.w_eff)[1], parent(r.w_eff)[1]]
        ids = torch.cat([c.reshape(-1) for c in caps])
        ids = torch.where(ids >= cfg.vocab_size, torch.full_like(ids, UNK), ids)
        m = int(torch.bincount(ids[ids != PAD]).max())
        for n in atomic:
            four = max(float((a[n] - b[n]).abs().max()) for i, a in enumerate(runs) for b in runs[i + 1:])
            tol[n] = max(2.0 * four, 2.0 * (m - 1) * 2.0 ** -24 * float(g1[n].abs().max()))
            print("    %s %s K=%d %s: spread over four parent runs %.3e, tolerance %.3e; preference_loss differs by %.3e"
                  % (case, mt, K, n, four, tol[n], float((g_pref[n] - g1[n]).abs().max())))
    for n in g1:
        if tol[n] == 0.0:
            assert _same(g_pref[n], g1[n]), n
        else:
            assert float((g_pref[n] - g1[n]).abs().max()) <= tol[n], (n, float((g_pref[n] - g1[n]).abs().max()), tol[n])


def test_reference_scores(golden_dir):
    import test_ensemble_gpu as te
    z, cfg, batch, model = build_model("tiny", "vivt", golden_dir, DEV)
    tr = _translator(cfg, model)
    caps = _candidates(tr, batch, 3)
    other = te._other_model(golden_dir, "tiny", "vivt")
    for reference in (_translator(cfg, other), te._ensemble(cfg, [model, other])):
        inputs = syn.translate_inputs(batch)
        before = [[t.clone() for t in inputs[0]], [t.clone() for t in inputs[2]]]
        members = reference._members()
        members[-1].train()
        try:
            got = prefopt.reference_scores(reference, inputs, caps)
            assert members[-1].training and not got.requires_grad           # the mode is restored; the pass ran without gradients …
        finally:
            members[-1].eval()
        assert all(torch.equal(a, b) for a, b in zip(before[0], inputs[0])) and all(torch.equal(a, b) for a, b in zip(before[1], inputs[2]))
        assert any(bool((t[:, cfg.max_v_len:] != PAD).any()) for t in inputs[0])
        sc = reference.score_captions(syn.translate_inputs(batch), caps)
        assert got.dtype == torch.float32 and tuple(got.shape) == (sum(int(s) for s in batch["batch_step_num"]), 3)
        assert _same(got, sc.cum) and got.data_ptr() != sc.cum.data_ptr()      # … in eval mode: score_captions' bits, in a buffer of its own
    # with graph=True the pass's buffer belongs to the captured graph: the clone survives the next replay
    trg = _translator(cfg, other, graph=True)
    a = prefopt.reference_scores(trg, syn.translate_inputs(batch), caps)
    keep = a.clone()
    caps2 = [torch.flip(c, [1]).contiguous() for c in caps]                    # (other captions in every row: the replay writes other scores)
    b = prefopt.reference_scores(trg, syn.translate_inputs(batch), caps2)
    assert _same(a, keep) and not _same(a, b) and a.data_ptr() != b.data_ptr()


# ------------------------------------------------------------------------------------------------ 3. the step, end to end
SPECIAL = ["[PAD]", "[CLS]", "[SEP]", "[VID]", "[BOS]", "[EOS]", "[UNK]"]


def _corpus(cfg, batch):
    """the idf corpus built from the fixture's labels, as tests/test_scst_gpu.py does"""
    from svpc_amd.caption_scores import ReferenceCorpus
    Vm = cfg.vocab_size
    i2w = SPECIAL + ["".join(chr(97 + (i // 26 ** k) % 26) for k in range(3)) for i in range(7, Vm)]
    refs, videos = {}, []
    for b in range(len(batch["batch_step_num"])):
        inv = {int(v): k for k, v in batch["oov_word_dict"][b].items()}
        sents = []
        for s in range(int(batch["batch_step_num"][b])):
            lab = batch["input_labels_list"][s][b].cpu().tolist()
            sents.append(" ".join(i2w[x] if x < Vm else inv[x] for x in lab if x not in (IGNORE, EOS, PAD)))
        refs["vid%d" % b] = [" ".join(sents)]
        videos.append(dict(key="vid%d" % b, oov_word_dict=batch["oov_word_dict"][b]))
    ref_tokens = [[cs.parse_sent(p) for p in refs[k]] for k in refs]
    return ReferenceCorpus(i2w, refs, device=DEV), videos, ref_tokens, cs.CiderCorpus(ref_tokens), i2w


#          source, K, decode keywords, include_gold, reference, loss keywords
STEPS = [("sample", 3, dict(seed=17), False, "second", dict(beta=0.1)),                                                        # DPO
         ("nbest", 3, {}, False, "ensemble", dict(beta=0.1, label_smoothing=0.1)),                                             # cDPO
         ("diverse", 4, dict(num_groups=2, diversity_strength=0.5), False, None, dict(beta=2.0, gamma=0.5, length_beta=1.0)),  # SimPO
         ("stochastic", 3, dict(seed=17), False, "self", dict(beta=0.1)),
         ("stochastic", 2, dict(seed=5), True, "second", dict(beta=0.5, loss_type="ipo", pairs="extremes"))]
DEFAULTS = dict(beta=0.1, gamma=0.0, label_smoothing=0.0, length_beta=0.0, pref_weight=1.0, loss_type="sigmoid", pairs="all")

# The policy as its own reference (eval mode, fp32, γ = ε = 0): u = cum − ref_cum is the difference between the graded pass's and the forced
# pass's log-probability of the same captions — two code paths over the same parameters, so it is small but need not be 0.  The largest |u|
# over ("tiny", "c1") × the "self" row of STEPS, measured on the MI355X (profiles/pref_parity.json); the assertion is at twice that.
MEASURED_SELF = 2.288818359375e-05                    # ("c1": a few fp32 ulps of the paragraph scores; "tiny" 4.8e-6)


def _decoder_output(tr, batch, source, K, kw):
    inputs = syn.translate_inputs(batch)
    if source == "sample":
        return tr.translate_batch_sample(inputs, num_samples=K, **kw)[0]
    if source == "nbest":
        return tr.translate_batch_nbest(inputs, K, K)[0]
    if source == "diverse":
        return tr.translate_batch_diverse(inputs, K, kw["num_groups"], kw["diversity_strength"], K // kw["num_groups"])[0]
    return tr.translate_batch_stochastic(inputs, K, **kw)[0]


@pytest.mark.parametrize("source,K,kw,gold,refkind,loss_kw", STEPS)
@pytest.mark.parametrize("case", ["tiny", "c1"])
def test_preference_step_end_to_end(golden_dir, case, source, K, kw, gold, refkind, loss_kw):
    import test_ensemble_gpu as te
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
    corpus, videos, ref_tokens, cider, i2w = _corpus(cfg, batch)
    steps = [int(s) for s in batch["batch_step_num"]]
    N, Kc = len(steps), K + (1 if gold else 0)
    po = prefopt.PreferenceOptimization(tr, corpus, reference=reference)
    opt = FusedBertAdam(list(model.named_parameters()), lr=1e-4, warmup=0.1, t_total=100, grad_clip=1.0)
    opt.zero_grad()
    inputs = syn.translate_inputs(batch)
    before = [[t.clone() for t in inputs[0]], [t.clone() for t in inputs[2]]]
    extra = dict(include_gold=True, input_labels_list=batch["input_labels_list"]) if gold else {}
    call = dict(num_candidates=K, source=source, **kw, **loss_kw, **extra)
    full = dict(DEFAULTS, **loss_kw)
    assert not model.training
    po.phase_events = []
    r = po.step(inputs, videos, **call)
    assert len(po.phase_events) == 5
    po.phase_events = None
    assert not model.training
    assert all(torch.equal(a, b) for a, b in zip(before[0], inputs[0])) and all(torch.equal(a, b) for a, b in zip(before[1], inputs[2]))
    # the candidates: the named decoder's output (and the gold rows behind them)
    want = _decoder_output(tr, batch, source, K, kw)
    assert all(tuple(d.shape) == (s, Kc, cfg.max_t_len) for d, s in zip(r.dec_seq_list, steps))
    assert all(torch.equal(d[:, :K], w_) for d, w_ in zip(r.dec_seq_list, want))
    if gold:
        g = tr.gold_captions(batch["input_labels_list"], batch["batch_step_num"])
        assert all(torch.equal(d[:, K], g_) for d, g_ in zip(r.dec_seq_list, g))
    # rewards: the restatement's CIDEr of the returned rows
    rows = [d.cpu().tolist() for d in r.dec_seq_list]
    reward = r.reward.cpu().numpy()
    assert r.reward.dtype == torch.float64 and reward.shape == (N, Kc)
    for b in range(N):
        for k in range(Kc):
            h = cs.hypothesis_tokens([rows[b][s][k] for s in range(steps[b])], i2w, batch["oov_word_dict"][b])
            wantr = cider.score(h, ref_tokens[b])
            assert abs(reward[b, k] - wantr) <= 1e-12 * max(1.0, abs(wantr)), (b, k, reward[b, k], wantr)
    # the reference's scores: score_captions' cum of the returned candidates
    if reference is None:
        assert r.ref_cum is None
    else:
        assert _same(r.ref_cum, reference.score_captions(syn.translate_inputs(batch), r.dec_seq_list).cum)
    # the group quantities: the restatement fed the step's own cum, reward and ref_cum
    length = tr.score_captions(syn.translate_inputs(batch), r.dec_seq_list).length
    ref = pr.groups(r.cum.cpu().numpy(), length.cpu().numpy(), r.barred.cpu().numpy(), -reward, pc.vid_off(steps), None,
                    None if r.ref_cum is None else r.ref_cum.cpu().numpy(), full["beta"], full["gamma"], full["label_smoothing"],
                    full["length_beta"], full["pref_weight"], full["loss_type"], full["pairs"])
    if refkind != "self":                                                   # (u is near 0 against the policy itself: its sign is rounding)
        _conditions(ref, full["loss_type"], full["beta"])
        np.testing.assert_array_equal(r.n_correct.cpu().numpy(), ref["n_correct"])
    np.testing.assert_array_equal(r.n_pairs.cpu().numpy(), ref["n_pairs"])
    np.testing.assert_array_equal(r.valid.cpu().numpy(), ref["valid"])
    np.testing.assert_allclose(r.pref.cpu().numpy(), ref["pref"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(r.implicit_reward.cpu().numpy(), ref["reward"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(r.margin.cpu().numpy(), ref["margin"], rtol=1e-12, atol=0)
    wantw = ref["w_eff"].reshape(-1)
    tol = np.spacing(np.abs(wantw)).astype(np.float64) + 1e-12 * float(np.abs(ref["G"]).max()) / N
    assert (np.abs(r.w_eff.cpu().numpy().reshape(-1).astype(np.float64) - wantw.astype(np.float64)) <= tol).all()
    assert abs(float(r.loss.detach()) - float(ref["total"])) <= _ulp32(ref["total"])
    assert tuple(r.cum.shape) == (sum(steps), Kc) and tuple(r.barred.shape) == (sum(steps), Kc) and tuple(r.w_eff.shape) == (sum(steps), Kc)
    if refkind == "self":
        u = float(np.abs(ref["u"]).max())
        dev = float(np.abs(ref["pref"][ref["n_pairs"] > 0] - LN2).max()) if ref["n_pairs"].any() else 0.0
        print("self reference %s: largest |u| %.6e, largest |pref − ln 2| %.3e" % (case, u, dev))
        os.makedirs(REPORT_DIR, exist_ok=True)
        with open(os.path.join(REPORT_DIR, "pref_self_%s.json" % case), "w") as f:
            json.dump(dict(case=case, source=source, K=K, largest_abs_u=u, largest_pref_minus_ln2=dev, measured=MEASURED_SELF), f, indent=1)
        # |ℓ(h) − ln 2| ≤ |h| (the sigmoid loss has slope at most 1 in h) and |h| = β·|u_i − u_j| ≤ 2β·max|u|
        assert u <= 2.0 * MEASURED_SELF and dev <= 2.0 * full["beta"] * 2.0 * MEASURED_SELF, (u, dev)
    # the same call again: the same candidates, the same bits
    r2 = po.step(syn.translate_inputs(batch), videos, **call)
    assert all(torch.equal(a, b) for a, b in zip(r.dec_seq_list, r2.dec_seq_list))
    assert _same(r.loss, r2.loss) and _same(r.cum, r2.cum) and _same(r.w_eff, r2.w_eff) and torch.equal(r.pref, r2.pref)
    # gradients: finite, not zero whenever some G is not; the optimizer steps
    backward_all(model, r.loss)
    ops.join_side()
    gsq = sum(float(p.grad.double().pow(2).sum()) for p in model.parameters() if p.grad is not None)
    # (beam candidates of an untrained model can all score the same reward: then no pair exists, w_eff = 0 and the gradient is exactly zero)
    assert np.abs(ref["G"]).max() > 0 or source in ("nbest", "diverse"), "every G is zero: the gradient check below would be empty"
    assert np.isfinite(gsq) and (gsq > 0) == bool(np.abs(ref["G"]).max() > 0), gsq
    opt.step()
    # train mode: dropout on, runs and stays finite; decode and reference ran in eval mode and the mode is restored.  The policy as its
    # own reference is refused in train mode.
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
            assert np.isfinite(float(r3.loss))
            assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    finally:
        model.eval()


def test_step_argument_rules(golden_dir):
    z, cfg, batch, model = build_model("tiny", "vivt", golden_dir, DEV)
    tr = _translator(cfg, model)
    corpus, videos, _, _, _ = _corpus(cfg, batch)
    po = prefopt.PreferenceOptimization(tr, corpus)
    bad = [dict(source="greedy"), dict(utility="METEOR"), dict(num_candidates=17), dict(num_candidates=16, include_gold=True,
           input_labels_list=batch["input_labels_list"]), dict(include_gold=True), dict(beta=0.0), dict(source="nbest", seed=3),
           dict(source="diverse", num_candidates=3, num_groups=2), dict(loss_type="ipo", gamma=0.5), dict(pairs="best")]
    for kw in bad:
        with pytest.raises(ValueError):
            po.step(syn.translate_inputs(batch), videos, **kw)
    with pytest.raises(TypeError):
        po.step(syn.translate_inputs(batch), videos, source="sample", no_such_keyword=1)
    assert not model.training


# ------------------------------------------------------------------------------------------------ 4. bf16x3
# bf16x3 at the config-1 shape against the fp32 restatement, measured on the MI355X over ("c1", "v") and ("c1", "vivt"), K = 3
# (profiles/pref_parity.json), DESIGN §11.18's procedure: the fp32 side is the CPU oracle's cum (``scst_reference.sequence_loss``) through
# the restatement — its loss, and as gradients those of the oracle's sequence loss under the restatement's w_eff.  The assertion is at twice
# the measured worst.
MEASURED_X3 = dict(loss=2.368616546724928e-06,               # ("c1", "vivt")
                   grad=0.19790290335782282,               # ("c1", "vivt"), step_wise_encoder.layer.1.attention.self.query.bias: small against the model's largest
                   grad_zero=0.0002981076734065759)       # ("c1", "vivt"): the zero-in-theory tensors, as a fraction of the model's largest gradient
BOUND_X3 = {k: 2.0 * v for k, v in MEASURED_X3.items()}


@pytest.mark.parametrize("mt", ["v", "vivt"])
def test_bf16x3_deviation_at_config_1(golden_dir, mt):
    import test_scst_gpu as ts
    K = 3
    z, cfg, batch, model = build_model("c1", mt, golden_dir, DEV)
    steps = [int(s) for s in batch["batch_step_num"]]
    N = len(steps)
    caps = _candidates(_translator(cfg, model), batch, K)                      # the captions: made once, in fp32
    w, cost, ref_cum = _weights(steps, K), _costs(N, K), _ref_cum(steps, K)
    # the fp32 restatement: the oracle's cum → the restatement's loss and w_eff → the oracle's gradients under w_eff
    _, _, cum0, bar0 = ts._reference(("pref0", mt, K), cfg, model, batch, caps, torch.zeros_like(w))
    length = _translator(cfg, model).score_captions(syn.translate_inputs(batch), caps).length.cpu().numpy()
    ref = pr.groups(np.where(bar0.reshape(-1, K), -np.inf, cum0.reshape(-1, K)).astype(np.float32), length, bar0.reshape(-1, K).astype(np.int32),
                    cost.numpy(), pc.vid_off(steps), w.numpy(), ref_cum.numpy(), LOSS_KW["beta"], LOSS_KW["gamma"], LOSS_KW["label_smoothing"],
                    LOSS_KW["length_beta"], LOSS_KW["pref_weight"], LOSS_KW["loss_type"], LOSS_KW["pairs"])
    _, ref_grads, _, ref_bar = ts._reference(("pref1", mt, K), cfg, model, batch, caps, torch.from_numpy(ref["w_eff"]))
    ref_loss = float(ref["total"])
    ops.set_precision("bf16x3")
    try:
        _, _, _, model_x3 = build_model("c1", mt, golden_dir, DEV)
        tr = _translator(cfg, model_x3)
        model_x3.zero_grad(set_to_none=True)
        r = prefopt.preference_loss(tr, syn.translate_inputs(batch), caps, cost.to(DEV), ref_cum=ref_cum.to(DEV), weights=w.to(DEV), **LOSS_KW)
        r.loss.backward()
        ops.join_side()
        torch.cuda.synchronize()
        loss = float(r.loss)
        np.testing.assert_array_equal(r.barred.cpu().numpy().reshape(-1).astype(bool), ref_bar.reshape(-1))
        gmax = max(float(g.abs().max()) for g in ref_grads.values() if g is not None)
        err, name, n, err0, name0 = ts._grad_errors(model_x3, ref_grads, mt, zero_scale=gmax)
    finally:
        ops.set_precision("fp32")
    rel = abs(loss - ref_loss) / abs(ref_loss)
    print("bf16x3 c1 %s: loss %.7g (restatement %.7g, rel %.3e); worst gradient error %.3e of its tensor's max (%s); zero in theory %.3e of the "
          "model's largest gradient (%s)" % (mt, loss, ref_loss, rel, err, name, err0, name0))
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "pref_parity_%s.json" % mt), "w") as f:
        json.dump(dict(case="c1", mt=mt, K=K, precision="bf16x3", loss=loss, restatement_loss=ref_loss, loss_rel_error=rel,
                       worst_grad_error=err, worst_grad_tensor=name, worst_zero_in_theory_error=err0, worst_zero_in_theory_tensor=name0,
                       tensors=n, bound=BOUND_X3, **LOSS_KW), f, indent=1)
    assert n > 20 and rel <= BOUND_X3["loss"] and err <= BOUND_X3["grad"] and err0 <= BOUND_X3["grad_zero"], (rel, err, name, err0, name0)
