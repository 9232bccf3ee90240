"""Unlikelihood training on the MI355X: svpc_ul_negatives / svpc_seq_ul_fwd / svpc_seq_ul_bwd against the restatement
(tests/unlikelihood_reference.py) on the fixed inputs of tests/unlikelihood_cases.py (whose margins tests/test_unlikelihood_host.py checks);
``unlikelihood.unlikelihood_loss`` — loss and every parameter gradient — against the CPU restatement built on the oracle's blocks under torch
autograd; the two steps end to end with the fused optimizer; and the bf16x3 deviation.

Bounds.  Negatives: every entry equal.  Kernels: step / cum / barred equal ``ops.seq_nll``'s bit for bit; ulstep / ul within rtol 1e-6 of the
fp64 value rounded to fp32 (their inputs are fp64 and rounded once; the clamp keeps 1 − p ≥ 1e-5, so the cancellation in 1 − p amplifies a
1e-15 error to at most 1e-10); dscores within rtol 1e-4 / atol 1e-6 (seq_nll's bar) and exactly 0 wherever the definition says 0; the loss
within one fp32 rounding of the fp64 sum plus what ul's 1e-6 allows (1e-6·Σ|u·ul|) and 1e-12 of Σ|terms| for a sum that cancels; with
u = 0 everything has ``ops.seq_nll``'s bits.  Model level (fp32): the graded pass's existing bars — loss ≤ 1e-4 relative, each gradient
≤ 2e-3 of its tensor's max magnitude, an absolute floor only for the tensors whose gradient is zero in exact arithmetic.  bf16x3: see
``BOUND_X3``."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import unlikelihood_cases as uc  # noqa: E402
import unlikelihood_reference as ur  # noqa: E402
from helpers import build_model  # noqa: E402
from test_scst_gpu import _corpus, _cpu, _grad_errors, _per_video, _translator  # noqa: E402  (the graded pass's model-level helpers)
from svpc_amd import _lib, ops, scst, synthetic as syn, unlikelihood as ul  # noqa: E402
from svpc_amd.ops_common import Idx  # noqa: E402
from svpc_amd.synthetic import EOS, IGNORE, PAD, UNK  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAMPLE_SEED = 2
REPORT_DIR = os.environ.get("SVPC_REPORT_DIR") or os.path.join(ROOT, "reports")
# bf16x3 at the config-1 shape against the fp32 CPU restatement, measured on the MI355X over ("c1", "v") and ("c1", "vivt") and both rules
# (profiles/unlikelihood_parity.json): the worst relative loss error and the worst gradient error as a fraction of its tensor's max
# magnitude.  The assertion is at twice the measured worst, as §11.10's.
MEASURED_X3 = dict(loss=1.978684441392872e-06,               # ("c1", "vivt"), token rule
                   grad=0.1812483746378685,                # ("c1", "v"), token rule, step_wise_encoder.layer.1.attention.self.key.weight: small against the model's largest
                   grad_zero=0.00024850613193832307)       # the zero-in-theory tensors, as a fraction of the model's largest gradient
BOUND_X3 = {k: 2.0 * v for k, v in MEASURED_X3.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ (a) the negatives
@pytest.mark.parametrize("Lt,K,steps", uc.NEGATIVE_SHAPES)
def test_negatives_equal_the_restatement(Lt, K, steps):
    ids, row_c, sf = uc.negatives_case(Lt, K, steps)
    R = ids.shape[0]
    _, _, tgt, ln, fin = ops.force_inputs(torch.from_numpy(ids).to(DEV).view(R // K, K, Lt), 9, UNK, EOS, PAD, IGNORE)
    rc = Idx(row_c.tolist())
    seen = 0
    for rule, n, scope in [("token", 4, "caption")] + [("ngram", n, s) for n in (1, 2, 4) for s in ("caption", "paragraph")]:
        want = ur.negatives(ids, row_c, rule, n, scope, sent_first=sf, K=K)
        got = ops.ul_negatives(tgt, ln, fin, rc, UNK, EOS, rule, n, scope, sent_first=sf, K=K)
        assert got[0].dtype == torch.int32 and tuple(got[0].shape) == want[0].shape
        for name, g, w_ in zip(("neg", "npen", "nrep"), got, want):
            np.testing.assert_array_equal(g.cpu().numpy(), w_, err_msg="%s %s n=%d %s" % (name, rule, n, scope))
        seen += int(want[1].sum())
    assert seen > 0 or Lt == 2


# ------------------------------------------------------------------------------------------------ (b) the loss kernels
def _close(got, ref):
    """rtol 1e-4 / atol 1e-6 (seq_nll's bar); exactly 0 wherever the definition says 0"""
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-6)
    assert not got[ref == 0].any()


def _upload(case):
    R, Lt, C = case["R"], case["Lt"], case["C"]
    sd = torch.from_numpy(case["scores"]).to(DEV)
    rc = Idx(case["row_c"].tolist())
    _, _, tgt, ln, _ = ops.force_inputs(torch.from_numpy(case["ids"]).to(DEV), max(UNK + 1, C - 2), UNK, EOS, PAD, IGNORE)
    return sd, rc, tgt, ln, torch.from_numpy(case["neg"]).to(DEV), torch.from_numpy(case["w"]).to(DEV), torch.from_numpy(case["u"]).to(DEV)


def _loss_bound(ref, w, u):
    keep = ref["barred"] == 0
    a = np.abs(w.astype(np.float64)[keep] * ref["cum"].astype(np.float64)[keep]).sum()
    b = np.abs(u.astype(np.float64)[keep] * ref["ul"].astype(np.float64)[keep]).sum()
    return 2.0 ** -23 * abs(float(ref["loss"])) + 1e-6 * b + 1e-12 * (a + b)


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("C,Lt,T,K", uc.KERNEL_SHAPES)
def test_kernels_equal_the_restatement(C, Lt, T, K, logits):
    case = uc.kernel_case(C, Lt, T * K, logits)
    R, dl = T * K, 2.5
    ref = ur.seq_ul(case["scores"], case["ids"], case["row_c"], case["neg"], case["w"], case["u"], logits, dl=dl)
    sd, rc, tgt, ln, neg, wd, ud = _upload(case)
    sd.requires_grad_(True)
    loss, cum, step, barred, ul_, ulstep = ops.seq_ul(sd, rc, tgt, ln, neg, wd, ud, logits, UNK)
    assert loss.requires_grad and not any(t.requires_grad for t in (cum, step, barred, ul_, ulstep))
    nll = ops.seq_nll(sd.detach(), rc, tgt, ln, wd, logits, UNK)
    for name, a, b in (("cum", cum, nll[1]), ("step", step, nll[2]), ("barred", barred, nll[3])):          # bit for bit (−inf included)
        assert torch.equal(_bits(a), _bits(b)), name
    np.testing.assert_array_equal(barred.cpu().numpy(), ref["barred"])
    for name, got, want in (("ulstep", ulstep, ref["ulstep64"].astype(np.float32)), ("ul", ul_, ref["ul"])):
        g = got.cpu().numpy()
        print("%s: worst relative error %.3e" % (name, float(np.max(np.abs(g - want) / np.maximum(np.abs(want), 1e-30)))))
        np.testing.assert_allclose(g, want, rtol=1e-6, atol=0, err_msg=name)
    assert not ulstep.cpu().numpy()[np.arange(Lt - 1)[None, :] >= ref["len"][:, None]].any()               # 0 past the end
    assert abs(loss.item() - float(ref["loss"])) <= _loss_bound(ref, case["w"], case["u"]), (loss.item(), ref["loss"])
    # the backward through autograd, an upstream factor of 2.5 …
    (loss * dl).backward()
    _close(sd.grad.cpu().numpy(), ref["dscores"])
    # … and the kernel alone into a wider buffer full of NaN: every element is written
    out = torch.full((R * Lt, C + 3), float("nan"), dtype=torch.float32, device=DEV)
    dld = torch.tensor([dl], dtype=torch.float32, device=DEV)
    s0 = sd.detach()
    _lib.call("seq_ul_bwd", s0.data_ptr(), s0.stride(0), rc.dev(s0.device).data_ptr(), int(case["row_c"].max()), tgt.data_ptr(), ln.data_ptr(),
              barred.data_ptr(), neg.data_ptr(), case["M"], wd.data_ptr(), ud.data_ptr(), dld.data_ptr(), R, Lt, 1 if logits else 0, UNK,
              out.data_ptr(), C + 3, ops._stream())
    torch.cuda.synchronize()
    _close(out.cpu().numpy(), np.pad(ref["dscores"], ((0, 0), (0, 3))))
    # u = 0: the loss, cum, step, barred and the gradient have ops.seq_nll's bits
    s1, s2 = (s0.clone().requires_grad_(True) for _ in range(2))
    a = ops.seq_ul(s1, rc, tgt, ln, neg, wd, torch.zeros_like(ud), logits, UNK)
    b = ops.seq_nll(s2, rc, tgt, ln, wd, logits, UNK)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a[:4], b))
    (a[0] * dl).backward()
    (b[0] * dl).backward()
    assert torch.equal(_bits(s1.grad), _bits(s2.grad))


def test_loss_is_deterministic_and_sums_many_rows():
    """more caption rows than the reduction has threads; twice the same bits"""
    case = uc.kernel_case(9, 3, 777, False)
    ref = ur.seq_ul(case["scores"], case["ids"], case["row_c"], case["neg"], case["w"], case["u"], False)
    sd, rc, tgt, ln, neg, wd, ud = _upload(case)
    a = ops.seq_ul(sd, rc, tgt, ln, neg, wd, ud, False, UNK)
    b = ops.seq_ul(sd, rc, tgt, ln, neg, wd, ud, False, UNK)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    assert abs(float(a[0]) - float(ref["loss"])) <= _loss_bound(ref, case["w"], case["u"])


# ------------------------------------------------------------------------------------------------ (c) the graded forced pass
def _weights(steps, K, flip=0):
    """hand-set, mixed signs, different on every row"""
    T = sum(steps)
    w = [[(-1.0) ** (t + k + flip) * (0.05 + 0.01 * ((3 * t + k + 2 * flip) % 7)) for k in range(K)] for t in range(T)]
    return torch.tensor(w, dtype=torch.float32)


def _candidates(tr, batch):
    """K = 3: the fixture's gold row, a sampled row of a fixed seed, and the gold row of the video's FIRST sentence in every sentence (a
    paragraph that repeats itself, whatever the model samples)"""
    gold = tr.gold_captions(batch["input_labels_list"], batch["batch_step_num"])
    sample = tr.translate_batch_sample(syn.translate_inputs(batch), num_samples=1, seed=SAMPLE_SEED)[0]
    return [torch.cat([g.unsqueeze(1), s[:, :1], g[:1].unsqueeze(1).expand(g.shape[0], 1, -1)], 1).contiguous() for g, s in zip(gold, sample)]


RULES = {"token": dict(rule="token"), "ngram": dict(rule="ngram", ngram=2, scope="paragraph")}
_REF = {}


def _reference(key, cfg, model, batch, caps, w, u, kw):
    """loss and parameter gradients of the CPU restatement (computed once per case, left unchanged)"""
    if key not in _REF:
        names = {n for n, _ in model.named_parameters()}
        P = {k: v.detach().cpu().clone().requires_grad_(k in names and v.is_floating_point()) for k, v in model.state_dict().items()}
        c = _cpu(batch)
        steps = [int(s) for s in c["batch_step_num"]]
        loss, uls, bars, npens, nreps = ur.sequence_loss(
            P, cfg, c["input_ids_list"], c["video_features_list"], c["input_masks_list"], c["ingr_input_ids"], c["ingr_sep_masks"], steps,
            c["ingr_id_dict"], c["oov_word_dict"], [x.cpu().numpy() for x in caps], [x.numpy() for x in _per_video(w, steps)],
            [x.numpy() for x in _per_video(u, steps)], **kw)
        loss.backward()
        _REF[key] = (float(loss.detach()), {n: (P[n].grad.clone() if P[n].grad is not None else None) for n in names},
                     torch.cat(uls).numpy(), np.concatenate(bars), np.concatenate(npens), np.concatenate(nreps))
    return _REF[key]


CASES = [("tiny", "v"), ("tiny", "vi"), ("tiny", "viv"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")]


@pytest.mark.parametrize("rule", ["token", "ngram"])
@pytest.mark.parametrize("case,mt", CASES)
def test_unlikelihood_loss_and_gradients_vs_restatement(golden_dir, case, mt, rule):
    z, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    tr = _translator(cfg, model)
    steps = [int(s) for s in batch["batch_step_num"]]
    caps = _candidates(tr, batch)
    w, u = _weights(steps, 3), _weights(steps, 3, flip=1)
    ref_loss, ref_grads, ref_ul, ref_bar, ref_npen, ref_nrep = _reference((case, mt, rule), cfg, model, batch, caps, w, u, RULES[rule])
    inputs = syn.translate_inputs(batch)
    before = [[t.clone() for t in inputs[0]], [t.clone() for t in inputs[2]]]
    model.zero_grad(set_to_none=True)
    r = ul.unlikelihood_loss(tr, inputs, caps, w.to(DEV), u.to(DEV), **RULES[rule])
    r.loss.backward()
    ops.join_side()
    torch.cuda.synchronize()
    # the caller's ids and masks are what they were (a training batch is reused)
    assert all(torch.equal(a, b) for a, b in zip(before[0], inputs[0])) and all(torch.equal(a, b) for a, b in zip(before[1], inputs[2]))
    np.testing.assert_array_equal(r.barred.cpu().numpy().astype(bool), ref_bar)
    np.testing.assert_array_equal(r.npen.cpu().numpy(), ref_npen)
    np.testing.assert_array_equal(r.nrep.cpu().numpy(), ref_nrep)
    assert ref_npen.sum() > 0 and (rule == "token" or ref_nrep.sum() > 0)
    print("%s %s %s: loss %.7g (restatement %.7g)" % (case, mt, rule, float(r.loss), ref_loss))
    assert abs(float(r.loss) - ref_loss) <= 1e-4 * abs(ref_loss), (float(r.loss), ref_loss)
    np.testing.assert_allclose(r.ul.cpu().numpy(), ref_ul, rtol=1e-4, atol=1e-6)
    # the likelihood half is sequence_loss's
    sl = scst.sequence_loss(tr, syn.translate_inputs(batch), caps, w.to(DEV))
    assert torch.equal(_bits(r.cum), _bits(sl.cum)) and torch.equal(r.barred, sl.barred) and torch.equal(r.length, sl.length)
    err, name, n, err0, name0 = _grad_errors(model, ref_grads, mt)
    print("%s %s %s: worst gradient error %.3e of its tensor's max (%s), %d tensors; zero in theory %.3e (%s)"
          % (case, mt, rule, err, name, n, err0, name0))
    assert n > 20 and err <= 2e-3 and err0 <= 2e-3, (err, name, err0, name0)


# ------------------------------------------------------------------------------------------------ the steps, end to end
def _decodes(tr, batch, sc, videos):
    """greedy, beam, sampling, sequence_loss and SelfCritical.step on the batch: what a call of the new steps must leave as it was"""
    out = [torch.cat([d.reshape(-1) for d in tr.translate_batch(syn.translate_inputs(batch))[0]]),
           torch.cat([d.reshape(-1) for d in tr.translate_batch_beam(syn.translate_inputs(batch), 2)[0]]),
           torch.cat([d.reshape(-1) for d in tr.translate_batch_sample(syn.translate_inputs(batch), num_samples=2, seed=5)[0]])]
    gold = [g.unsqueeze(1).contiguous() for g in tr.gold_captions(batch["input_labels_list"], batch["batch_step_num"])]
    T = sum(int(s) for s in batch["batch_step_num"])
    sl = scst.sequence_loss(tr, syn.translate_inputs(batch), gold, torch.full((T, 1), 0.25, device=DEV))
    s = sc.step(syn.translate_inputs(batch), videos, num_samples=2, baseline="mean", seed=9)
    return out + [sl.loss.detach(), sl.cum, s.loss.detach(), s.reward, s.cum]


@pytest.mark.parametrize("case", ["tiny", "c1"])
def test_steps_end_to_end(golden_dir, case):
    from svpc_amd.graph import backward_all
    from svpc_amd.optim import FusedBertAdam
    z, cfg, batch, model = build_model(case, "vivt", golden_dir, DEV)
    tr = _translator(cfg, model)
    corpus, videos = _corpus(cfg, batch)[:2]
    sc = scst.SelfCritical(tr, corpus)
    steps = [int(s) for s in batch["batch_step_num"]]
    T = sum(steps)
    step = ul.Unlikelihood(tr)
    before = _decodes(tr, batch, sc, videos)
    inputs = syn.translate_inputs(batch)
    kept = [[t.clone() for t in inputs[0]], [t.clone() for t in inputs[2]]]
    a = step.token_step(inputs, batch["input_labels_list"], alpha=0.5)
    b = step.sequence_step(inputs, alpha=1.0, ngram=1, scope="paragraph", source="sample", seed=17)
    g = step.sequence_step(inputs, alpha=1.0, ngram=2, scope="caption")
    assert all(torch.equal(x, y) for x, y in zip(kept[0], inputs[0])) and all(torch.equal(x, y) for x, y in zip(kept[1], inputs[2]))
    for t in (a.nll, a.ul, a.npen, a.barred, b.ul, b.npen, b.nrep, g.ul):
        assert tuple(t.shape) == (T, 1)
    assert all(tuple(d.shape) == (s, 1, cfg.max_t_len) for d, s in zip(b.dec_seq_list, steps))
    # the token step is the restatement's weights over the gold rows: w = 1 / n, u = α / n
    gold = tr.gold_captions(batch["input_labels_list"], batch["batch_step_num"])
    lens = scst.sequence_loss(tr, syn.translate_inputs(batch), [x.unsqueeze(1).contiguous() for x in gold], torch.zeros(T, 1, device=DEV)).length
    w_ref, u_ref = ur.per_token_weights(lens.cpu().numpy().reshape(-1), 0.5)
    r = ul.unlikelihood_loss(tr, syn.translate_inputs(batch), gold, torch.from_numpy(w_ref).to(DEV), torch.from_numpy(u_ref).to(DEV), rule="token")
    assert torch.equal(_bits(r.loss.detach()), _bits(a.loss.detach())) and torch.equal(r.ul, a.ul) and torch.equal(r.npen, a.npen)
    assert np.isfinite(float(a.loss)) and float(a.ul.sum()) > 0 and int(a.npen.sum()) > 0
    assert np.isfinite(float(b.loss)) and float(b.loss) >= 0
    # one seed twice: the same decode, the same loss
    b2 = step.sequence_step(syn.translate_inputs(batch), alpha=1.0, ngram=1, scope="paragraph", source="sample", seed=17)
    assert all(torch.equal(x, y) for x, y in zip(b.dec_seq_list, b2.dec_seq_list))
    assert torch.equal(_bits(b.loss.detach()), _bits(b2.loss.detach())) and torch.equal(b.nrep, b2.nrep)
    after = _decodes(tr, batch, sc, videos)
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    # train mode: dropout on; each step with a FusedBertAdam update, everything stays finite, the mode is restored
    opt = FusedBertAdam(list(model.named_parameters()), lr=1e-4, warmup=0.1, t_total=100, grad_clip=1.0)
    model.train()
    try:
        for run in (lambda: step.token_step(syn.translate_inputs(batch), batch["input_labels_list"], alpha=1.0),
                    lambda: step.sequence_step(syn.translate_inputs(batch), alpha=1.0, ngram=1, scope="paragraph", source="sample", seed=3),
                    lambda: step.sequence_step(syn.translate_inputs(batch), alpha=1.0, ngram=1)):
            opt.zero_grad()
            r = run()
            assert model.training
            backward_all(model, r.loss)
            ops.join_side()
            opt.step()
            torch.cuda.synchronize()
            assert np.isfinite(float(r.loss))
            assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    finally:
        model.eval()


# ------------------------------------------------------------------------------------------------ bf16x3
@pytest.mark.parametrize("rule", ["token", "ngram"])
@pytest.mark.parametrize("mt", ["v", "vivt"])
def test_bf16x3_deviation_at_config_1(golden_dir, mt, rule):
    """the config-1 model-level case under the headline arithmetic against the fp32 CPU restatement: the worst loss and gradient errors are
    recorded (reports/unlikelihood_parity_<mt>_<rule>.json; the committed copy is profiles/unlikelihood_parity.json) and held to BOUND_X3"""
    z, cfg, batch, model = build_model("c1", mt, golden_dir, DEV)
    steps = [int(s) for s in batch["batch_step_num"]]
    caps = _candidates(_translator(cfg, model), batch)                         # the captions: made once, in fp32
    w, u = _weights(steps, 3), _weights(steps, 3, flip=1)
    ref_loss, ref_grads, _, ref_bar, _, _ = _reference(("c1", mt, rule), cfg, model, batch, caps, w, u, RULES[rule])
    ops.set_precision("bf16x3")
    try:
        _, _, _, model_x3 = build_model("c1", mt, golden_dir, DEV)            # (the same weights; its weight store gets the mode's lo plane)
        tr = _translator(cfg, model_x3)
        model_x3.zero_grad(set_to_none=True)
        r = ul.unlikelihood_loss(tr, syn.translate_inputs(batch), caps, w.to(DEV), u.to(DEV), **RULES[rule])
        r.loss.backward()
        ops.join_side()
        torch.cuda.synchronize()
        loss = float(r.loss)
        np.testing.assert_array_equal(r.barred.cpu().numpy().astype(bool), ref_bar)
        gmax = max(float(g.abs().max()) for g in ref_grads.values() if g is not None)
        err, name, n, err0, name0 = _grad_errors(model_x3, ref_grads, mt, zero_scale=gmax)
    finally:
        ops.set_precision("fp32")
    rel = abs(loss - ref_loss) / abs(ref_loss)
    print("bf16x3 c1 %s %s: loss %.7g (restatement %.7g, rel %.3e); worst gradient error %.3e of its tensor's max (%s); zero in theory %.3e of "
          "the model's largest gradient (%s)" % (mt, rule, loss, ref_loss, rel, err, name, err0, name0))
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "unlikelihood_parity_%s_%s.json" % (mt, rule)), "w") as f:
        json.dump(dict(case="c1", mt=mt, rule=rule, K=3, precision="bf16x3", loss=loss, restatement_loss=ref_loss, loss_rel_error=rel,
                       worst_grad_error=err, worst_grad_tensor=name, worst_zero_in_theory_error=err0, worst_zero_in_theory_tensor=name0,
                       tensors=n, bound=BOUND_X3), f, indent=1)
    assert n > 20 and rel <= BOUND_X3["loss"] and err <= BOUND_X3["grad"] and err0 <= BOUND_X3["grad_zero"], (rel, err, name, err0, name0)
