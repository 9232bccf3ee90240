"""The self-critical training step on the MI355X: svpc_seq_nll_fwd / svpc_seq_nll_bwd / svpc_scst_weights against the
restatement (tests/scst_reference.py) on seeded random rows; ``scst.sequence_loss`` — loss and every parameter gradient — against the CPU
restatement built on the oracle's blocks under torch autograd; the sum over the K captions of a sentence; ``SelfCritical.step`` end to end
with the fused optimizer; and the bf16x3 deviation.

Bounds.  Kernels: step / cum equal ``ops.force_score``'s bit for bit; dscores within rtol 1e-4 / atol 1e-6 (``test_beam_gpu._compare``'s
bound) and exactly 0 wherever the definition says 0; the loss within one fp32 rounding of the fp64 sum (both sides sum fp64 products, in
different orders: 2⁻²³ relative, plus 1e-12 of Σ|terms| for a sum that cancels); weights and advantages bit for bit.  Model level (fp32):
``tests/test_model_gpu.py``'s — loss ≤ 1e-4 relative, each gradient ≤ 2e-3 of its tensor's max magnitude, an absolute floor only for the
tensors whose gradient is zero in exact arithmetic; cum within rtol 1e-4 / atol 1e-6 of ``score_captions``.  bf16x3: see ``BOUND_X3``."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import caption_scores_reference as cs  # noqa: E402
import scst_reference as sr  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import _lib, ops, scst, synthetic as syn  # noqa: E402
from svpc_amd.ops_common import Idx  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, IGNORE, PAD, UNK  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = type("O", (), {"cuda": True})
SAMPLE_SEED = 2
SPECIAL = ["[PAD]", "[CLS]", "[SEP]", "[VID]", "[BOS]", "[EOS]", "[UNK]"]
REPORT_DIR = os.environ.get("SVPC_REPORT_DIR") or os.path.join(ROOT, "reports")
# bf16x3 at the config-1 shape against the fp32 CPU restatement, measured on the MI355X over ("c1", "v") and ("c1", "vivt"), K = 3
# (profiles/scst_parity.json): the worst relative loss error and the worst gradient error as a fraction of its tensor's max magnitude.
# The assertion is at twice the measured worst, the margin for the split-product rounding varying with the caption.
MEASURED_X3 = dict(loss=2.3097070749019594e-06,              # ("c1", "vivt")
                   grad=0.1434393183641582,               # ("c1", "vivt"), step_wise_encoder.layer.1.attention.self.query.bias: small against the model's largest
                   grad_zero=0.00035380186107399303)        # the zero-in-theory tensors, as a fraction of the model's largest gradient
BOUND_X3 = {k: 2.0 * v for k, v in MEASURED_X3.items()}


# ------------------------------------------------------------------------------------------------ 1. the kernels
#        C,  Lt,  T,  K      (R = T·K caption rows; one score row, and row counts that are no multiple of the 4 per workgroup)
SHAPES = [(7, 2, 1, 1), (64, 22, 3, 3), (65, 6, 7, 1), (951, 22, 2, 16), (1025, 6, 3, 3), (4097, 6, 5, 1)]


def _random_case(rng, C, Lt, R, logits, zeros):
    """score rows, captions, column counts and weights: mixed C_r in one launch; captions that end at position 1, never end, are all PAD,
    stop at IGNORE; targets at column 0 … C_r − 1, at UNK, at C_r, below 0; weights negative and zero; (zeros) probabilities of 0"""
    row_c = np.array([C if r % 3 == 0 else int(rng.integers(max(UNK + 1, C // 2), C + 1)) for r in range(R)])
    if zeros:
        vals = np.array([0.0, 0.125, 0.25, 0.5] if not logits else [-3.0, -1.0, 0.0, 2.0], np.float32)
        s = vals[rng.integers(0, len(vals), size=(R * Lt, C))]
    else:
        s = (rng.random((R * Lt, C)) ** 4 + 1e-3).astype(np.float32) if not logits else rng.standard_normal((R * Lt, C)).astype(np.float32) * 3
    s[:, UNK] = 1.0 if not logits else 50.0            # UNK would dominate the softmax were it a candidate
    ids = np.zeros((R, Lt), np.int64)
    ids[:, 0] = BOS
    for r in range(R):
        c = int(row_c[r])
        words = rng.integers(0, c, size=Lt - 1)
        words[(words == EOS) | (words == PAD) | (words == UNK)] = 1
        if Lt > 2:
            words[0], words[-1] = c - 1, 0                                 # the last column; column 0 is PAD and ends the row there
        kind = r % 6
        n = int(rng.integers(0, Lt - 1))               # words before the end
        if kind == 0:
            row = list(words[:-1]) + [c - 1 if c - 1 != UNK else 1]        # never ends (C = 7: column 6 is UNK; the one-row case scores a candidate)
        elif kind == 1:
            row = [EOS] + [PAD] * (Lt - 2)                                 # ends at position 1
        elif kind == 2:
            row = [PAD] * (Lt - 1)                                         # all PAD
        elif kind == 3:
            row = list(words[:n]) + [IGNORE] * (Lt - 1 - n)
        else:
            row = list(words[:n]) + [EOS] + [PAD] * (Lt - 2 - n)
            if n and kind == 5:                                            # a non-candidate target somewhere before the end: barred
                row[int(rng.integers(0, n))] = [UNK, c, -7, c + 3][int(rng.integers(0, 4))]
        ids[r, 1:] = row[:Lt - 1]
    w = rng.standard_normal(R).astype(np.float32)
    if R > 1:
        w[rng.integers(0, R)] = 0.0
    return s, ids, row_c, w


def _close(got, ref):
    """rtol 1e-4 / atol 1e-6 (``test_beam_gpu._compare``'s bound); exactly 0 wherever the definition says 0"""
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-6)
    assert not got[ref == 0].any()


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("C,Lt,T,K", SHAPES)
def test_kernels_equal_the_restatement(C, Lt, T, K, logits):
    rng = np.random.default_rng(1000 * C + Lt + logits)
    R = T * K
    for zeros in (False, True):
        s, ids, row_c, w = _random_case(rng, C, Lt, R, logits, zeros)
        dl = 2.5
        ref = sr.seq_nll(s, ids, row_c, w, logits, dl=dl)
        sd = torch.from_numpy(s).to(DEV).requires_grad_(True)
        wd = torch.from_numpy(w).to(DEV)
        rc = Idx(row_c.tolist())
        V = max(UNK + 1, C - 2)
        _, _, tgt, ln, _ = ops.force_inputs(torch.from_numpy(ids).to(DEV).view(T, K, Lt), V, UNK, EOS, PAD, IGNORE)
        loss, cum, step, barred = ops.seq_nll(sd, rc, tgt, ln, wd, logits, UNK)
        assert loss.requires_grad and not (cum.requires_grad or step.requires_grad or barred.requires_grad)
        fs = ops.force_score(sd.detach(), rc, tgt, ln, logits, UNK, "bar")
        for k, t in (("step", step), ("cum", cum)):                        # bit for bit (−inf included)
            assert torch.equal(t.view(torch.int32), fs[k].view(torch.int32)), k
            np.testing.assert_array_equal(t.cpu().numpy().view(np.int32), ref[k].astype(np.float32).view(np.int32), err_msg=k)
        np.testing.assert_array_equal(barred.cpu().numpy(), ref["barred"])
        assert R < 18 or ref["barred"].any()                                # (the barred path is exercised)
        assert R > 1 or zeros or (not ref["barred"].any() and np.isfinite(ref["step"]).all() and ref["dscores"].any())   # (one row: a finite step)
        terms = np.abs(w.astype(np.float64)[ref["barred"] == 0] * ref["cum"].astype(np.float64)[ref["barred"] == 0]).sum()
        assert abs(loss.item() - float(ref["loss"])) <= 2.0 ** -23 * abs(float(ref["loss"])) + 1e-12 * terms, (loss.item(), ref["loss"])
        # the backward through autograd, an upstream factor of 2.5 …
        (loss * dl).backward()
        _close(sd.grad.cpu().numpy(), ref["dscores"])
        # … and the kernel alone into a buffer full of NaN: every element is written
        out = torch.full((R * Lt, C + 3), float("nan"), dtype=torch.float32, device=DEV)
        dld = torch.tensor([dl], dtype=torch.float32, device=DEV)
        _lib.call("seq_nll_bwd", sd.data_ptr(), sd.stride(0), rc.dev(sd.device).data_ptr(), int(row_c.max()), tgt.data_ptr(), ln.data_ptr(),
                  barred.data_ptr(), wd.data_ptr(), dld.data_ptr(), R, Lt, 1 if logits else 0, UNK, out.data_ptr(), C + 3, ops._stream())
        torch.cuda.synchronize()
        _close(out.cpu().numpy(), np.pad(ref["dscores"], ((0, 0), (0, 3))))


def test_loss_is_deterministic_and_sums_many_rows():
    """more caption rows than the reduction has threads; twice the same bits"""
    rng = np.random.default_rng(5)
    C, Lt, R = 9, 3, 777
    s, ids, row_c, w = _random_case(rng, C, Lt, R, False, False)
    ref = sr.seq_nll(s, ids, row_c, w, False)
    sd, wd = torch.from_numpy(s).to(DEV), torch.from_numpy(w).to(DEV)
    _, _, tgt, ln, _ = ops.force_inputs(torch.from_numpy(ids).to(DEV), C, UNK, EOS, PAD, IGNORE)
    a = ops.seq_nll(sd, Idx(row_c.tolist()), tgt, ln, wd, False, UNK)
    b = ops.seq_nll(sd, Idx(row_c.tolist()), tgt, ln, wd, False, UNK)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    keep = ref["barred"] == 0
    terms = np.abs(w.astype(np.float64)[keep] * ref["cum"].astype(np.float64)[keep]).sum()
    assert abs(float(a[0]) - float(ref["loss"])) <= 2.0 ** -23 * abs(float(ref["loss"])) + 1e-12 * terms


@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("baseline", ["none", "greedy", "mean"])
def test_scst_weights_bit_for_bit(K, baseline):
    if baseline == "mean" and K == 1:
        with pytest.raises(ValueError):
            ops.scst_weights(torch.zeros(2, 1, dtype=torch.float64, device=DEV), [0, 1], "mean")
        return
    rng = np.random.default_rng(10 * K + len(baseline))
    steps = [3, 0, 1, 5, 2]                                                    # a video without sentences: an advantage, no weight rows
    N = len(steps)
    r = rng.random((N, K)) * 3
    r[3] = r[3, 0]                                                             # an all-zero advantage under "mean"
    g = rng.random(N) * 3
    A = sr.advantages(r, baseline, g)
    w = sr.row_weights(A, steps)
    adv, wd = ops.scst_weights(torch.from_numpy(r).to(DEV), [b for b, s in enumerate(steps) for _ in range(s)], baseline,
                               torch.from_numpy(g).to(DEV) if baseline == "greedy" else None)
    assert adv.dtype == torch.float64 and wd.dtype == torch.float32 and tuple(wd.shape) == (sum(steps) * K,)
    np.testing.assert_array_equal(adv.cpu().numpy().view(np.int64), A.view(np.int64))
    np.testing.assert_array_equal(wd.cpu().numpy().view(np.int32), w.view(np.int32))
    assert (A < 0).any() or baseline == "none"


# ------------------------------------------------------------------------------------------------ 2. the graded forced pass
def _cpu(batch):
    return {k: ([t.cpu() for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor) else
                (v.cpu() if isinstance(v, torch.Tensor) else v)) for k, v in batch.items()}


def _translator(cfg, model, **kw):
    from svpc_amd.translator import Translator
    return Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, **kw)


def _weights(steps, K):
    """hand-set, mixed signs, different on every row"""
    T = sum(steps)
    w = [[(-1.0) ** (t + k) * (0.05 + 0.01 * ((3 * t + k) % 7)) for k in range(K)] for t in range(T)]
    return torch.tensor(w, dtype=torch.float32)


def _candidates(tr, batch, K):
    """the fixture's gold rows, then sampled rows of a fixed seed"""
    gold = tr.gold_captions(batch["input_labels_list"], batch["batch_step_num"])
    if K == 1:
        return [g.unsqueeze(1).contiguous() for g in gold]
    sample = tr.translate_batch_sample(syn.translate_inputs(batch), num_samples=4, seed=SAMPLE_SEED)[0]
    return [torch.cat([g.unsqueeze(1), s[:, :K - 1]], 1).contiguous() for g, s in zip(gold, sample)]


def _per_video(t, steps):
    out, o = [], 0
    for s in steps:
        out.append(t[o:o + s])
        o += s
    return out


_REF = {}


def _reference(key, cfg, model, batch, caps, w):
    """loss and parameter gradients of the CPU restatement (computed once per case, left unchanged)"""
    if key not in _REF:
        names = {n for n, _ in model.named_parameters()}
        P = {k: v.detach().cpu().clone().requires_grad_(k in names and v.is_floating_point()) for k, v in model.state_dict().items()}
        c = _cpu(batch)
        steps = [int(s) for s in c["batch_step_num"]]
        loss, cums, bars = sr.sequence_loss(P, cfg, c["input_ids_list"], c["video_features_list"], c["input_masks_list"], c["ingr_input_ids"],
                                            c["ingr_sep_masks"], steps, c["ingr_id_dict"], c["oov_word_dict"],
                                            [x.cpu().numpy() for x in caps], [x.numpy() for x in _per_video(w, steps)])
        loss.backward()
        _REF[key] = (float(loss), {n: (P[n].grad.clone() if P[n].grad is not None else None) for n in names},
                     torch.cat(cums).numpy(), np.concatenate(bars))
    return _REF[key]


def _zero_in_theory(name, mt):
    """key biases (softmax shift invariance), the pointer's ``Wing.bias`` (the same shift of every entity's score) and, with ONE memory
    row per sentence (``v``), the cross-attention's query / key projections (a softmax over a single key is the constant 1): both sides
    hold rounding noise there — ``tests/test_model_gpu.py``'s list"""
    return (name.endswith(".key.bias") or name == "Wing.bias" or
            (mt == "v" and ("dec_enc_attention.query" in name or "dec_enc_attention.key" in name)))


def _grad_errors(model, ref_grads, mt, zero_scale=None):
    """→ (worst error as a fraction of the tensor's max magnitude, its name, tensors compared, the worst error among the tensors that are
    zero in exact arithmetic and its name); a tensor the restatement gives no (or an exactly zero) gradient must come out absent or
    exactly zero, unless it is zero in exact arithmetic only.  The zero-in-theory tensors hold rounding noise on both sides: their error
    is taken against the tensor's max magnitude plus ``tests/test_model_gpu.py``'s absolute floor of 2e-3, or, with ``zero_scale``
    (bf16x3, whose backward rounds to bf16), as a fraction of the model's largest gradient."""
    worst, worst_zero, n = (0.0, ""), (0.0, ""), 0
    for name, p in model.named_parameters():
        rg = ref_grads[name]
        zt = _zero_in_theory(name, mt)
        if (rg is None or float(rg.abs().max()) == 0.0) and not zt:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        if p.grad is None and zt:
            continue
        assert p.grad is not None, name
        rg = torch.zeros_like(p.grad, device="cpu") if rg is None else rg
        diff = float((p.grad.detach().cpu() - rg).abs().max())
        scale = max(1e-6, float(rg.abs().max()))
        if zt:
            worst_zero = max(worst_zero, (diff / (zero_scale if zero_scale is not None else scale + 2e-3), name))
        else:
            worst = max(worst, (diff / scale, name))
        n += 1
    return worst[0], worst[1], n, worst_zero[0], worst_zero[1]


def _run(tr, batch, caps, w):
    model = tr.model
    model.zero_grad(set_to_none=True)
    r = scst.sequence_loss(tr, syn.translate_inputs(batch), caps, w.to(DEV))
    r.loss.backward()
    ops.join_side()
    torch.cuda.synchronize()
    return r


CASES = [("tiny", "v"), ("tiny", "vi"), ("tiny", "viv"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")]


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("case,mt", CASES)
def test_sequence_loss_and_gradients_vs_restatement(golden_dir, case, mt, K):
    z, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    tr = _translator(cfg, model)
    steps = [int(s) for s in batch["batch_step_num"]]
    caps = _candidates(tr, batch, K)
    w = _weights(steps, K)
    ref_loss, ref_grads, ref_cum, ref_bar = _reference((case, mt, K), cfg, model, batch, caps, w)
    inputs = syn.translate_inputs(batch)
    before = [[t.clone() for t in inputs[0]], [t.clone() for t in inputs[2]]]
    model.zero_grad(set_to_none=True)
    r = scst.sequence_loss(tr, inputs, caps, w.to(DEV))
    r.loss.backward()
    ops.join_side()
    torch.cuda.synchronize()
    # the caller's ids and masks are what they were (a training batch is reused)
    assert all(torch.equal(a, b) for a, b in zip(before[0], inputs[0])) and all(torch.equal(a, b) for a, b in zip(before[1], inputs[2]))
    assert any(bool((t[:, cfg.max_v_len:] != PAD).any()) for t in inputs[0])
    np.testing.assert_array_equal(r.barred.cpu().numpy().reshape(-1).astype(bool), ref_bar.reshape(-1))
    print("%s %s K=%d: loss %.7g (restatement %.7g)" % (case, mt, K, float(r.loss), ref_loss))
    assert abs(float(r.loss) - ref_loss) <= 1e-4 * abs(ref_loss), (float(r.loss), ref_loss)
    live = ~ref_bar.reshape(-1)
    np.testing.assert_allclose(r.cum.cpu().numpy().reshape(-1)[live], ref_cum.reshape(-1)[live], rtol=1e-4, atol=1e-6)
    sc = tr.score_captions(syn.translate_inputs(batch), caps)
    np.testing.assert_allclose(r.cum.cpu().numpy(), sc.cum.cpu().numpy(), rtol=1e-4, atol=1e-6)
    assert torch.equal(r.length, sc.length)
    err, name, n, err0, name0 = _grad_errors(model, ref_grads, mt)
    print("%s %s K=%d: worst gradient error %.3e of its tensor's max (%s), %d tensors; zero in theory %.3e (%s)" % (case, mt, K, err, name, n, err0, name0))
    assert n > 20 and err <= 2e-3 and err0 <= 2e-3, (err, name, err0, name0)
    # the re-simulation (the BiLSTM ``recipe_encoder`` and ``recipe_reasoner``) takes no part: its gradients are absent or zero
    idle = 0
    for pn, p in model.named_parameters():
        if pn.startswith(("recipe_reasoner.", "recipe_encoder.")):
            idle += 1
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, pn
    assert idle > 0 or mt != "vivt"


@pytest.mark.parametrize("case,mt", [("tiny", "v"), ("tiny", "vi"), ("tiny", "vivt"), ("c1", "vivt")])
def test_gradients_sum_over_the_k_captions_of_a_sentence(golden_dir, case, mt):
    """K = 3 with the same caption in all three slots and w = (a, a, a) gives the gradients of K = 1 with w = 3a: a dropped or
    overwritten sum over K (memory rows, bank, bank projection) shows here"""
    z, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    tr = _translator(cfg, model)
    steps = [int(s) for s in batch["batch_step_num"]]
    one = _candidates(tr, batch, 1)
    a = _weights(steps, 1)
    r1 = _run(tr, batch, one, 3.0 * a)
    g1 = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    r3 = _run(tr, batch, [c.expand(-1, 3, -1).contiguous() for c in one], a.expand(-1, 3).contiguous())
    assert abs(float(r3.loss) - float(r1.loss)) <= 1e-4 * abs(float(r1.loss))
    assert torch.equal(r3.cum[:, 0], r1.cum[:, 0]) and torch.equal(r3.cum[:, 2], r1.cum[:, 0])
    n = 0
    for name, p in model.named_parameters():
        if name not in g1:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        scale = float(g1[name].abs().max())
        if scale == 0.0:
            continue
        err = float((p.grad - g1[name]).abs().max()) / (max(1e-6, scale) + (2e-3 if _zero_in_theory(name, mt) else 0.0))
        assert err <= 2e-3, (name, err)
        n += 1
    assert n > 20


# ------------------------------------------------------------------------------------------------ 3. the step, end to end
def _corpus(cfg, batch):
    """the idf corpus built from the fixture's labels, as tests/test_consensus_gpu.py does; → (corpus, videos, reference token lists, CIDEr restatement, idx2word)"""
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


@pytest.mark.parametrize("baseline", ["greedy", "mean"])
@pytest.mark.parametrize("case", ["tiny", "c1"])
def test_self_critical_step_end_to_end(golden_dir, case, baseline):
    from svpc_amd.graph import backward_all
    from svpc_amd.optim import FusedBertAdam
    z, cfg, batch, model = build_model(case, "vivt", golden_dir, DEV)
    tr = _translator(cfg, model)
    corpus, videos, ref_tokens, cider, i2w = _corpus(cfg, batch)
    steps = [int(s) for s in batch["batch_step_num"]]
    N, K = len(steps), 3
    sc = scst.SelfCritical(tr, corpus)
    opt = FusedBertAdam(list(model.named_parameters()), lr=1e-4, warmup=0.1, t_total=100, grad_clip=1.0)
    opt.zero_grad()
    inputs = syn.translate_inputs(batch)
    before = [[t.clone() for t in inputs[0]], [t.clone() for t in inputs[2]]]
    r = sc.step(inputs, videos, num_samples=K, baseline=baseline, seed=17)
    assert all(torch.equal(a, b) for a, b in zip(before[0], inputs[0])) and all(torch.equal(a, b) for a, b in zip(before[1], inputs[2]))
    # rewards: the restatement's CIDEr of the returned rows
    rows = [d.cpu().tolist() for d in r.dec_seq_list]                          # [b][s][k]
    reward = r.reward.cpu().numpy()
    assert r.reward.dtype == torch.float64 and reward.shape == (N, K)
    for b in range(N):
        for k in range(K):
            h = cs.hypothesis_tokens([rows[b][s][k] for s in range(steps[b])], i2w, batch["oov_word_dict"][b])
            want = cider.score(h, ref_tokens[b])
            assert abs(reward[b, k] - want) <= 1e-12 * max(1.0, abs(want)), (b, k, reward[b, k], want)
    greedy = None
    if baseline == "greedy":
        g_rows = [d.cpu().tolist() for d in tr.translate_batch(syn.translate_inputs(batch))[0]]
        greedy = r.baseline.cpu().numpy()
        for b in range(N):
            want = cider.score(cs.hypothesis_tokens(g_rows[b], i2w, batch["oov_word_dict"][b]), ref_tokens[b])
            assert abs(greedy[b] - want) <= 1e-12 * max(1.0, abs(want))
    # advantages and weights: the restatement on the device's rewards, bit for bit
    A = sr.advantages(reward, baseline, greedy)
    np.testing.assert_array_equal(r.advantage.cpu().numpy().view(np.int64), A.view(np.int64))
    np.testing.assert_array_equal(r.weights.cpu().numpy().reshape(-1).view(np.int32), sr.row_weights(A, steps).view(np.int32))
    assert np.isfinite(float(r.loss)) and tuple(r.cum.shape) == (sum(steps), K) and tuple(r.barred.shape) == (sum(steps), K)
    # the same seed again: the same samples, the same loss
    r2 = sc.step(syn.translate_inputs(batch), videos, num_samples=K, baseline=baseline, seed=17)
    assert all(torch.equal(a, b) for a, b in zip(r.dec_seq_list, r2.dec_seq_list))
    assert torch.equal(r.loss.detach().view(torch.int32), r2.loss.detach().view(torch.int32)) and torch.equal(r.cum, r2.cum)
    # gradients: finite, not all zero where the advantages are not; the re-simulation's absent or zero — in the optimizer's arena too
    backward_all(model, r.loss)
    ops.join_side()
    gsq = sum(float(p.grad.double().pow(2).sum()) for p in model.parameters() if p.grad is not None)
    assert np.abs(A).max() > 0, "every advantage is zero: the gradient check below would be empty"
    assert np.isfinite(gsq) and gsq > 0, gsq
    idle = 0
    for pn, p in model.named_parameters():
        if pn.startswith(("recipe_reasoner.", "recipe_encoder.")):
            idle += 1
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, pn
    assert idle > 0
    opt.step()
    # train mode: dropout on, runs and stays finite; one more optimizer step
    model.train()
    try:
        opt.zero_grad()
        r3 = sc.step(syn.translate_inputs(batch), videos, num_samples=K, baseline=baseline, seed=17)
        assert model.training                                                  # (the decodes ran in eval mode; the mode is restored)
        backward_all(model, r3.loss)
        ops.join_side()
        opt.step()
        torch.cuda.synchronize()
        assert np.isfinite(float(r3.loss))
        assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    finally:
        model.eval()


# ------------------------------------------------------------------------------------------------ 4. bf16x3
@pytest.mark.parametrize("mt", ["v", "vivt"])
def test_bf16x3_deviation_at_config_1(golden_dir, mt):
    """the config-1 model-level case under the headline arithmetic against the fp32 CPU restatement: the worst loss and gradient errors
    are recorded (reports/scst_parity_<mt>.json; the committed copy is profiles/scst_parity.json) and held to BOUND_X3"""
    K = 3
    z, cfg, batch, model = build_model("c1", mt, golden_dir, DEV)
    steps = [int(s) for s in batch["batch_step_num"]]
    caps = _candidates(_translator(cfg, model), batch, K)                      # the captions: made once, in fp32
    w = _weights(steps, K)
    ref_loss, ref_grads, _, ref_bar = _reference(("c1", mt, K), cfg, model, batch, caps, w)
    ops.set_precision("bf16x3")
    try:
        _, _, _, model_x3 = build_model("c1", mt, golden_dir, DEV)            # (the same weights; its weight store gets the mode's lo plane)
        tr = _translator(cfg, model_x3)
        r = _run(tr, batch, caps, w)
        loss = float(r.loss)
        np.testing.assert_array_equal(r.barred.cpu().numpy().reshape(-1).astype(bool), ref_bar.reshape(-1))
        gmax = max(float(g.abs().max()) for g in ref_grads.values() if g is not None)
        err, name, n, err0, name0 = _grad_errors(model_x3, ref_grads, mt, zero_scale=gmax)
    finally:
        ops.set_precision("fp32")
    rel = abs(loss - ref_loss) / abs(ref_loss)
    print("bf16x3 c1 %s: loss %.7g (restatement %.7g, rel %.3e); worst gradient error %.3e of its tensor's max (%s); zero in theory %.3e of the "
          "model's largest gradient (%s)" % (mt, loss, ref_loss, rel, err, name, err0, name0))
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "scst_parity_%s.json" % mt), "w") as f:
        json.dump(dict(case="c1", mt=mt, K=K, precision="bf16x3", loss=loss, restatement_loss=ref_loss, loss_rel_error=rel,
                       worst_grad_error=err, worst_grad_tensor=name, worst_zero_in_theory_error=err0, worst_zero_in_theory_tensor=name0,
                       tensors=n, bound=BOUND_X3), f, indent=1)
    assert n > 20 and rel <= BOUND_X3["loss"] and err <= BOUND_X3["grad"] and err0 <= BOUND_X3["grad_zero"], (rel, err, name, err0, name0)
