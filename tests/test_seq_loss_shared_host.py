"""The host layer the sequence losses and their training steps share, without a GPU: the error texts and the order of the host checks
against the record taken before the bindings got a module of their own (tests/golden/seq_loss_errors.json), the re-exports under ``ops``,
the eval-mode context manager, the copies of the ids and masks, the rollout the candidate-set steps share, and the autograd plumbing of the
six score-matrix losses with a recorder in place of the kernel library (CPU tensors stand in for device tensors — only their address,
shape and stride are read)."""
import inspect
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import seq_loss_error_cases as ec  # noqa: E402
from svpc_amd import _lib, distill, mrt, ops, policy, prefopt, scst, seq_loss_ops as slo, unlikelihood  # noqa: E402
from svpc_amd.synthetic import UNK  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "seq_loss_errors.json")) as _f:
    RECORD = json.load(_f)
# Every name ``ops`` held before the split is still there, with two exceptions the test makes on purpose: the private helpers
# ``_risk_number`` and ``_pg_number``, two spellings of the one number check that is now ``seq_loss_ops._number``; nothing else used them.
RETIRED = {"_risk_number", "_pg_number"}


# ------------------------------------------------------------------------------------------------ error texts and re-exports
def test_every_wrong_call_raises_what_it_raised_before(monkeypatch):
    monkeypatch.setattr(_lib, "call", ec.refuse_launch)
    cases = ec.cases()
    assert sorted(n for n, _ in cases) == sorted(RECORD["errors"])
    wrong = {n: (ec.run(call), RECORD["errors"][n]) for n, call in cases if ec.run(call) != RECORD["errors"][n]}
    assert not wrong, wrong
    kinds = {v[0] for n, v in RECORD["errors"].items() if not n.startswith("seq_nll/row_w_")}
    assert kinds == {"ValueError", "SvpcKernelError"}                          # no case passes, none trips over its own arguments
    assert RECORD["errors"]["seq_nll/row_w_none"][0] == "AttributeError"       # (seq_nll alone takes its row_w for a tensor unasked)
    for fam in ec.FAMILIES:                                                    # every wrapper's name stands in its own messages only
        texts = [v[1] for n, v in RECORD["errors"].items() if n.startswith("seq_%s/" % fam)]
        assert any(t.startswith("seq_%s: " % fam) for t in texts)
        assert not any(t.startswith("seq_%s: " % other) for t in texts for other in ec.FAMILIES if other != fam)


def test_public_names_are_reexported_and_none_left_ops():
    assert slo.__all__ == sorted(set(slo.__all__), key=slo.__all__.index)
    public = [n for n in vars(slo) if not n.startswith("_") and getattr(vars(slo)[n], "__module__", slo.__name__) == slo.__name__
              and not inspect.ismodule(vars(slo)[n])]
    assert set(public) <= set(slo.__all__), set(public) - set(slo.__all__)
    for n in slo.__all__:
        assert getattr(ops, n) is getattr(slo, n), n
    for n in ("_SeqNll", "_SeqUl", "_SeqKd", "_SeqCl", "_SeqRisk", "_SeqPref", "_SeqPg"):
        assert getattr(ops, n) is getattr(slo, n), n
    missing = set(RECORD["ops_names"]) - set(dir(ops)) - RETIRED
    assert not missing, missing
    assert not RETIRED & set(dir(ops)) and not RETIRED & set(dir(slo))


# ------------------------------------------------------------------------------------------------ mode handling and inputs
class Counted(torch.nn.Module):
    """a model stand-in that counts the calls that walk its modules"""

    def __init__(self, training):
        super().__init__()
        self.inner = torch.nn.Linear(1, 1)
        torch.nn.Module.train(self, training)
        self.calls = []

    def train(self, mode=True):
        self.calls.append(("train", mode))
        return super().train(mode)

    def eval(self):
        self.calls.append(("eval",))
        return torch.nn.Module.train(self, False)

    def _stacked(self, tensors):
        return torch.stack(list(tensors))


def test_eval_mode_switches_and_restores_only_the_training_members():
    a, b = Counted(True), Counted(False)
    with scst.eval_mode([a, b]):
        assert not a.training and not a.inner.training and not b.training
    assert a.training and a.inner.training and not b.training
    assert a.calls == [("eval",), ("train", True)] and b.calls == []
    with pytest.raises(RuntimeError, match="inside"):
        with scst.eval_mode(iter([a, b])):
            assert not a.training
            raise RuntimeError("inside")
    assert a.training and not b.training and b.calls == [] and len(a.calls) == 4
    a.eval()
    del a.calls[:]
    with scst.eval_mode([a, b]):
        pass
    assert not a.training and a.calls == [] and b.calls == []                 # nothing to switch: nothing walked, nothing switched back
    assert not hasattr(distill, "_Eval") and not hasattr(distill, "_fresh")


def test_fresh_inputs_copies_the_ids_and_masks_only():
    model = Counted(False)
    inputs = [[torch.arange(6).view(2, 3) + 10 * s for s in range(2)], [torch.zeros(2, 3, 4)], [torch.ones(2, 3) * s for s in range(2)]]
    inputs += [object() for _ in range(9)]
    keep = [[t.clone() for t in inputs[0]], [t.clone() for t in inputs[2]]]
    out = scst.fresh_inputs(model, tuple(inputs))
    assert isinstance(out, list) and len(out) == 12
    for slot, want in ((0, keep[0]), (2, keep[1])):
        assert len(out[slot]) == len(want) and all(torch.equal(a, b) for a, b in zip(out[slot], want))
        assert all(a.data_ptr() != b.data_ptr() for a, b in zip(out[slot], inputs[slot]))
        for t in out[slot]:
            t.fill_(-7)
        assert all(torch.equal(a, b) for a, b in zip(inputs[slot], want))
    assert all(out[i] is inputs[i] for i in range(12) if i not in (0, 2))


def test_frozen_scores_is_what_both_frozen_passes_call():
    model, other = Counted(True), Counted(False)
    seen = {}

    def score_captions(inputs, caps):
        seen.update(training=model.training, grad=torch.is_grad_enabled(), inputs=inputs, caps=caps)
        return SimpleNamespace(cum=seen.setdefault("cum", torch.arange(4.0)), step=seen.setdefault("step", torch.arange(8.0)))
    scorer = SimpleNamespace(_members=lambda: [model, other], score_captions=score_captions)
    inputs = [[torch.zeros(2, 3)], None, [torch.ones(2, 3)]] + [None] * 9
    for fn, field in ((prefopt.reference_scores, "cum"), (policy.position_scores, "step")):
        got = fn(scorer, inputs, "caps")
        assert torch.equal(got, seen[field]) and got.data_ptr() != seen[field].data_ptr()
        assert seen["training"] is False and seen["grad"] is False and seen["caps"] == "caps" and model.training
        assert seen["inputs"][0][0].data_ptr() != inputs[0][0].data_ptr() and seen["inputs"][2][0].data_ptr() != inputs[2][0].data_ptr()
    assert other.calls == [] and model.calls == [("eval",), ("train", True)] * 2
    assert "frozen reference model" in prefopt.reference_scores.__doc__ and "frozen policy" in policy.position_scores.__doc__


def test_one_per_token_rule():
    p = SimpleNamespace(length=torch.tensor([3, 0, 4], dtype=torch.int32))
    w, u = unlikelihood.Unlikelihood._per_token(p, 0.5, True)
    seventh = torch.tensor(7.0, dtype=torch.float64)
    assert w.tolist() == [(1.0 / seventh).float().item()] * 3 and u.tolist() == [(0.5 / seventh).float().item()] * 3
    w0, u0 = unlikelihood.Unlikelihood._per_token(p, 0.5, False)
    assert w0.tolist() == [0.0] * 3 and torch.equal(u0, u) and w0.dtype == torch.float32
    dw, dv = distill.Distill._per_token(p, 0.25)
    assert torch.equal(dw, scst.per_token(p, 0.75)[0]) and torch.equal(dv, scst.per_token(p, 0.25)[0])
    assert dw.is_contiguous() and tuple(dw.shape) == (3,)
    empty = SimpleNamespace(length=torch.zeros(2, dtype=torch.int32))
    assert scst.per_token(empty, 2.0)[0].tolist() == [2.0, 2.0]              # n = max(1, Σ len)


# ------------------------------------------------------------------------------------------------ the shared rollout
class StubTranslator(object):
    """records what a step calls, in order; two videos of (2, 1) sentences, Lt = 3"""
    SAMPLING, TRUNCATION = (), ()

    def __init__(self, log, fail=False):
        self.log, self.fail, self.model, self.max_t_len = log, fail, Counted(True), 3

    def translate_batch_sample(self, inputs, num_samples=1, seed=None, **kw):
        self.log.append(("decode", self.model.training, num_samples, seed, inputs[0][0].data_ptr()))
        if self.fail:
            raise RuntimeError("the decode failed")
        return [torch.zeros(s, num_samples, 3, dtype=torch.int64) + k for k, s in enumerate((2, 1))], ["oov"], None, None

    def gold_captions(self, labels, steps):
        self.log.append(("gold", labels, list(steps)))
        return [torch.full((s, 3), 9, dtype=torch.int32) for s in (2, 1)]

    def caption_scores(self, dec, plan, row=0):
        self.log.append(("scores", row, tuple(dec[0].shape)))
        return torch.arange(12, dtype=torch.float64).view(2, 6) + 100 * row


class StubCorpus(object):
    def __init__(self, log):
        self.log = log

    def plan(self, videos):
        self.log.append(("plan", videos))
        return "plan"


@pytest.fixture
def rollout(monkeypatch):
    log = []

    class Event(object):
        def __init__(self, enable_timing=False):
            assert enable_timing

        def record(self):
            log.append("stamp")
    monkeypatch.setattr(torch.cuda, "Event", Event)
    ns = SimpleNamespace(loss=0, risk=torch.zeros(2), rank=1, Q=2, w_eff=3, cum=4, barred=5, pref=6, reward=7, n_pairs=8, n_correct=9, margin=10,
                         valid=11)
    monkeypatch.setattr(mrt, "risk_loss", lambda tr, inputs, dec, cost, **kw: log.append(("risk_loss", tuple(cost.shape), sorted(kw))) or ns)
    monkeypatch.setattr(prefopt, "preference_loss", lambda tr, inputs, dec, cost, **kw: log.append(("preference_loss", sorted(kw))) or ns)
    monkeypatch.setattr(prefopt, "reference_scores", lambda ref, inputs, dec: log.append(("reference_scores",)) or "ref_cum")
    monkeypatch.setattr(policy, "position_scores", lambda scorer, inputs, dec: log.append(("position_scores", scorer.name)) or "step")
    monkeypatch.setattr(policy, "policy_loss", lambda tr, inputs, dec, adv, **kw: log.append(("policy_loss", sorted(kw))) or SimpleNamespace())
    monkeypatch.setattr(ops, "group_advantage", lambda reward, rule, eps: log.append(("group_advantage", rule)) or "adv")
    return log


def _inputs():
    ids, masks = [torch.zeros(2, 4, dtype=torch.int64)], [torch.ones(2, 4)]
    return [ids, None, masks] + [None] * 8 + [[2, 1]]


def test_rollout_checks_arguments_before_anything_is_called(rollout):
    tr = StubTranslator(rollout)
    tr.name = "policy"
    for step in (mrt.MinimumRisk(tr, StubCorpus(rollout)), prefopt.PreferenceOptimization(tr, StubCorpus(rollout)),
                 policy.PolicyOptimization(tr, StubCorpus(rollout))):
        step.phase_events = []
        for kw in (dict(num_candidates=17), dict(source="greedy"), dict(utility="METEOR")):
            with pytest.raises(ValueError):
                step.step(_inputs(), ["v0", "v1"], **kw)
        if not isinstance(step, policy.PolicyOptimization):
            with pytest.raises(ValueError, match="input_labels_list"):
                step.step(_inputs(), ["v0", "v1"], include_gold=True)
            with pytest.raises(ValueError):
                step.step(_inputs(), ["v0", "v1"], num_candidates=16, include_gold=True, input_labels_list="labels")
            with pytest.raises(ValueError):
                step.step(_inputs(), ["v0", "v1"], alpha=-1.0, beta=-1.0)
        assert rollout == [] and step.phase_events == [] and tr.model.calls == [] and tr.model.training
    for cls in (prefopt.PreferenceOptimization, policy.PolicyOptimization):       # the policy as its own reference, in training mode
        with pytest.raises(ValueError, match="dropout"):
            cls(tr, StubCorpus(rollout), reference=tr).step(_inputs(), ["v0", "v1"])
    assert rollout == [] and tr.model.calls == []


def test_rollout_restores_the_mode_when_the_decode_raises(rollout):
    tr = StubTranslator(rollout, fail=True)
    step = mrt.MinimumRisk(tr, StubCorpus(rollout))
    step.phase_events = []
    with pytest.raises(RuntimeError, match="the decode failed"):
        step.step(_inputs(), ["v0", "v1"], source="sample", num_candidates=2)
    assert tr.model.training and tr.model.calls == [("eval",), ("train", True)]
    assert [e if e == "stamp" else e[:2] for e in rollout] == ["stamp", ("decode", False)] and len(step.phase_events) == 1


def test_rollout_of_the_three_steps(rollout):
    inputs = _inputs()
    tr = StubTranslator(rollout)
    tr.name = "policy"
    decode = ("decode", False, 2, 5)

    def short(log):
        return [e if e == "stamp" else (e[:4] if e[0] == "decode" else e) for e in log]
    # minimum risk with the gold captions: K + 1 candidates, the gold row last; 4 stamps
    step = mrt.MinimumRisk(tr, StubCorpus(rollout))
    step.phase_events = []
    r = step.step(inputs, ["v0", "v1"], num_candidates=2, source="sample", include_gold=True, input_labels_list="labels", seed=5, alpha=0.1)
    assert short(rollout) == ["stamp", decode, ("gold", "labels", [2, 1]), "stamp", ("plan", ["v0", "v1"]), ("scores", 0, (2, 3, 3)),
                              ("scores", 1, (2, 3, 3)), ("scores", 2, (2, 3, 3)), "stamp", ("risk_loss", (2, 3), ["alpha"]), "stamp"]
    assert len(step.phase_events) == 4 and tr.model.training and tr.model.calls == [("eval",), ("train", True)]
    assert rollout[1][4] != inputs[0][0].data_ptr()                              # the decode ran on a copy of the ids
    assert tuple(r.reward.shape) == (2, 3) and r.reward[:, 2].tolist() == [205.0, 211.0]    # (CIDEr is column 5)
    assert all(d.shape[1] == 3 and bool((d[:, 2] == 9).all()) and bool((d[:, :2] != 9).all()) for d in r.dec_seq_list)
    assert r.oov_word_dict == ["oov"]
    # preference optimisation with a reference: 5 stamps
    del rollout[:]
    step = prefopt.PreferenceOptimization(tr, StubCorpus(rollout), reference=SimpleNamespace(name="reference"))
    step.phase_events = []
    r = step.step(inputs, ["v0", "v1"], num_candidates=2, source="sample", seed=5, beta=0.2)
    assert short(rollout) == ["stamp", decode, "stamp", ("plan", ["v0", "v1"]), ("scores", 0, (2, 2, 3)), ("scores", 1, (2, 2, 3)), "stamp",
                              ("reference_scores",), "stamp", ("preference_loss", ["beta", "ref_cum"]), "stamp"]
    assert len(step.phase_events) == 5 and r.ref_cum == "ref_cum" and tuple(r.reward.shape) == (2, 2)
    # policy gradient: collect 5 stamps (the advantages before the third), update 2
    del rollout[:]
    step = policy.PolicyOptimization(tr, StubCorpus(rollout), reference=SimpleNamespace(name="reference"))
    step.phase_events = []
    ro = step.collect(inputs, ["v0", "v1"], num_candidates=2, source="sample", seed=5)
    assert short(rollout) == ["stamp", decode, "stamp", ("plan", ["v0", "v1"]), ("scores", 0, (2, 2, 3)), ("scores", 1, (2, 2, 3)),
                              ("group_advantage", "grpo"), "stamp", ("position_scores", "policy"), "stamp", ("position_scores", "reference"),
                              "stamp"]
    assert len(step.phase_events) == 5 and ro.adv == "adv" and ro.old_step == "step" and ro.ref_step == "step"
    step.update(ro, inputs, kl_beta=0.04)
    assert short(rollout)[-3:] == ["stamp", ("policy_loss", ["kl_beta", "old_step", "ref_step"]), "stamp"] and len(step.phase_events) == 7
    assert tr.model.training and tr.model.calls == [("eval",), ("train", True)] * 3
    assert mrt.MinimumRisk._stamp is scst.SelfCritical._stamp is scst.PhaseEvents._stamp


# ------------------------------------------------------------------------------------------------ the autograd plumbing
R, LT, C, K = 4, 3, 9, 2
TALL = 2                                             # score rows past R·Lt


def _forward_args(fam, scores):
    f32, i32, f64 = ec.f32, ec.i32, ec.f64
    rc, tgt, length, row_w = i32(R) + C, i32(R, LT), i32(R) + 1, f32(R)
    cost, off = f64(1, K), torch.tensor([0, 2], dtype=torch.int32)
    return {"nll": (scores, rc, tgt, length, row_w, 0, UNK, C),
            "ul": (scores, rc, tgt, length, i32(R, LT - 1, 1) - 1, row_w, f32(R), 0, UNK, C),
            "kd": (scores, rc, tgt, length, f32(R * LT + TALL, C), row_w, f32(R), 0, 1, UNK, C),
            "risk": (scores, rc, tgt, length, cost, off, row_w, 0, UNK, C, (5e-3, 0.0, 1e-3, 1.0, 0.0)),
            "pref": (scores, rc, tgt, length, cost, off, f32(R), row_w, 0, UNK, C, (0.1, 0.0, 0.0, 0.0, 1.0), (0, 0)),
            "pg": (scores, rc, tgt, length, cost, off, f32(R, LT - 1), None, row_w, 0, UNK, C, (0.2, 0.2, 0.0, 0.0), 0)}[fam]


# family → (class, forward kernel, outputs, backward kernel, where the backward's weights come from: forward inputs or outputs)
PLUMBING = {"nll": (slo._SeqNll, "seq_nll_fwd", 4, "seq_nll_bwd", {7: ("in", 4)}),
            "ul": (slo._SeqUl, "seq_ul_fwd", 6, "seq_ul_bwd", {9: ("in", 5), 10: ("in", 6), 7: ("in", 4)}),
            "kd": (slo._SeqKd, "seq_kd_fwd", 8, "seq_kd_bwd", {9: ("in", 5), 10: ("in", 6), 2: ("in", 4)}),
            "risk": (slo._SeqRisk, "seq_risk_fwd", 10, "seq_nll_bwd", {7: ("out", 9)}),
            "pref": (slo._SeqPref, "seq_pref_fwd", 11, "seq_nll_bwd", {7: ("out", 10)}),
            "pg": (slo._SeqPg, "seq_pg_fwd", 11, "seq_pos_bwd", {7: ("out", 4)})}


@pytest.mark.parametrize("fam", ec.FAMILIES)
def test_autograd_plumbing(fam, monkeypatch):
    cls, fwd, n_out, bwd, weights = PLUMBING[fam]
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)) or 0)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: real_empty(*a, **k).fill_(-1))      # (what nobody writes stays −1)
    decls = _lib.declarations()
    scores = torch.zeros(R * LT + TALL, C, requires_grad=True)
    args = _forward_args(fam, scores)
    n_in = len(inspect.signature(cls.forward).parameters) - 1
    assert len(args) == n_in
    out = cls.apply(*args)
    assert [c[0] for c in calls] == [fwd] and len(calls[0][1]) == len(decls["svpc_" + fwd][1]) and calls[0][1][-1] == 0
    assert len(out) == n_out and out[0].requires_grad and not any(o.requires_grad for o in out[1:])
    loss, cum, step, barred = out[:4]
    assert loss.dim() == 0 and tuple(cum.shape) == (R,) and tuple(step.shape) == (R, LT - 1) and barred.dtype == torch.int32
    assert all(o.data_ptr() in calls[0][1] for o in out)                         # every output is one of the launch's arguments
    del calls[:]
    out[0].backward()                                                            # (autograd itself refuses a wrong number of gradients)
    assert [c[0] for c in calls] == [bwd] and len(calls[0][1]) == len(decls["svpc_" + bwd][1]) and calls[0][1][-1] == 0
    got = calls[0][1]
    assert got[0] == scores.data_ptr() and got[1] == scores.stride(0) and got[-2] == C
    for pos, (side, i) in weights.items():
        assert got[pos] == (args if side == "in" else out)[i].data_ptr(), (pos, side, i)
    g = scores.grad
    assert tuple(g.shape) == tuple(scores.shape) and bool((g[R * LT:] == 0).all()) and bool((g[:R * LT] == -1).all())
    # a score matrix of exactly R·Lt rows: nothing to zero; no gradient for the loss: no launch, one None per forward input
    exact = torch.zeros(R * LT, C, requires_grad=True)
    args = _forward_args(fam, exact)
    if fam == "kd":
        args = args[:4] + (ec.f32(R * LT, C),) + args[5:]
    cls.apply(*args)[0].backward()
    assert bool((exact.grad == -1).all())
    del calls[:]
    none = cls.backward(SimpleNamespace(needs_input_grad=(True,) + (False,) * (n_in - 1)), None)
    assert none == (None,) * n_in and calls == []


def test_the_common_checks_and_the_backward_preamble_stand_once():
    text = {}
    for name in os.listdir(os.path.join(ROOT, "svpc_amd")):
        if name.endswith(".py"):
            with open(os.path.join(ROOT, "svpc_amd", name)) as f:
                text[name] = f.read()
    for needle in ("dscores[R * lt:].zero_()", ".clone().unbind(0))\n    dec_in[2]", "def _stamp(self)", "was = [m for m in"):
        assert sum(t.count(needle) for t in text.values()) == 1, needle
    # (``force_score``, a decoder binding that stays in ops.py, says the same of its own ``tgt``; ``ul_negatives`` has no score matrix)
    assert text["seq_loss_ops.py"].count("tgt must be a contiguous int32 (R, Lt >= 2) matrix on the scores' device") == 1
    assert text["seq_loss_ops.py"].count("%s: one column count per caption row") == 1
    for cls in (slo._SeqRisk, slo._SeqPref, slo._SeqPg):
        assert "backward" not in vars(cls) and cls.backward is slo._SeqNll.backward
