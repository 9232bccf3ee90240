"""Ensemble decoding on the MI355X: the combine kernel (svpc_ensemble_combine) against tests/ensemble_reference.py::combine, and
``EnsembleTranslator`` end to end — identical members and weights (1, 0) against the plain ``Translator`` bit for bit for every strategy,
two different members against the CPU ensemble decodes (fp32), forced scoring of the ensemble's own rows, graph replay and re-capture.

Bounds.  ``prob`` in probability mode has no transcendental and the kernel adds in the reference's order with separately rounded
products: ``assert_array_equal``.  Everywhere else the device's fp64 exp / log may differ from libm's in the last fp64 bits, and after the
single rounding to fp32 that is at most 1 fp32 ulp: ``assert_array_max_ulp(maxulp=1)``.  Decodes against the CPU reference follow
test_beam_gpu / test_sampling_gpu: ids and lengths exact, cum within rtol 1e-4 / atol 1e-6, a row may differ only where the reference's
own margin is ≤ 1e-4, and such rows are at most max(1, total // 20).  Member 1's parameters are drawn with seed 13: checked on the CPU
reference alone, greedy, beam 3 and sampling (R = 3, seed 5) have no decision with a margin ≤ 1e-4 under either rule and weight pair on
any of the four cases (0 rows; the smallest margin is 1.18e-4, beam 3 on c1 vivt under ``prob``)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import ensemble_reference as er  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import ops, synthetic as syn  # noqa: E402
from svpc_amd.model_shapes import parameter_shapes  # noqa: E402
from svpc_amd.ops_common import Idx  # noqa: E402
from svpc_amd.synthetic import EOS, UNK  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = type("O", (), {"cuda": True})
TIE = 1e-4
SETTINGS = [("prob", None), ("logprob", (0.7, 0.3))]


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _members(rng, n_rows, cmax, M, logits, lds, offset=False):
    """M member matrices (host float32 (n_rows, cmax) and their device copies with leading dimensions ``lds``): exact zeros, denormals
    and negative entries (probabilities); −inf logits, one member row entirely −inf; a huge UNK value that must not leak"""
    host, dev = [], []
    for m in range(M):
        if logits:
            s = (rng.standard_normal((n_rows, cmax)) * 3).astype(np.float32)
            s[rng.random((n_rows, cmax)) < 0.05] = -np.inf
            s[:, UNK] = 80.0
            if m == M - 1:
                s[n_rows // 2, :] = -np.inf
                s[n_rows // 2, UNK] = 80.0
        else:
            s = (rng.random((n_rows, cmax)) ** 4).astype(np.float32)
            s[rng.random((n_rows, cmax)) < 0.1] = 0.0
            s[rng.random((n_rows, cmax)) < 0.02] = 1e-40
            s[rng.random((n_rows, cmax)) < 0.01] = -0.5
            s[:, UNK] = 1.0
        buf = torch.full((n_rows * lds[m] + 1,), 7.0, dtype=torch.float32, device=DEV)
        d = buf[1:] if offset and m == 0 else buf[:-1]
        d = d.view(n_rows, lds[m])
        d[:, :cmax] = torch.from_numpy(s).to(DEV)
        host.append(s)
        dev.append(d)
    return host, dev


def _check(dev, host, row_c, weights, rule, logits, rows_per, exact):
    cmax = max(row_c)
    out = ops.ensemble_combine(dev, Idx(row_c), weights=weights, rule=rule, logits=logits, unk=UNK, rows_per=rows_per, max_cols=cmax)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    ref = er.combine(host, row_c, weights, rule, logits, UNK, rows_per, ld_out=cmax)
    assert out.shape == ref.shape == (host[0].shape[0], cmax) and np.all(np.isfinite(out))
    if exact:
        np.testing.assert_array_equal(out.view(np.int32), ref.view(np.int32))
    else:
        np.testing.assert_array_max_ulp(out, ref, maxulp=1)
    for r in range(out.shape[0]):
        assert np.all(out[r, row_c[r // rows_per]:] == 0)                    # padding columns: exactly 0
    if logits:
        assert np.all(out[:, UNK] == 0)                                       # the UNK column never leaks
    return out


def _weight_sets(M):
    return [None] + ([(0.5, 0.3, 0.2)] if M == 3 else []) + ([(1, 0), (0, 2)] if M == 2 else [])


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("rule", er.RULES)
@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_kernel_equals_combine(M, rule, logits):
    rng = np.random.default_rng(100 * M + 10 * logits + (rule == "prob"))
    exact = rule == "prob" and not logits
    for n_rows in (1, 21):                                  # 21: 7 sentences × 3 rows, more than one workgroup
        for rows_per in (1, 5):
            n_c = -(-n_rows // rows_per)
            row_c = [int(c) for c in rng.integers(16, 700, size=n_c)] if rows_per > 1 else \
                [int(c) for c in np.repeat(rng.integers(16, 700, size=-(-n_rows // 3)), 3)[:n_rows]]
            cmax = max(row_c)
            # leading dimensions: all equal to the output's modulo 4 (the 16-byte body), and differing ones with an odd one (scalar)
            for lds, offset in (([cmax + 4 * (m % 3) for m in range(M)], False), ([cmax + (0, 3, 8, 1, 4, 5, 12, 7)[m] for m in range(M)], False),
                                ([cmax] * M, True)):
                host, dev = _members(rng, n_rows, cmax, M, logits, lds, offset)
                for w in _weight_sets(M):
                    _check(dev, host, row_c, w, rule, logits, rows_per, exact)


def test_kernel_wide_rows():
    """rows of 4,096 columns, the widest the step kernels take; both rules and score modes"""
    rng = np.random.default_rng(9)
    row_c = [4096, 1025, 4096, 3000, 4095]
    for logits in (False, True):
        host, dev = _members(rng, 5, 4096, 3, logits, [4096, 4100, 4099])
        for rule in er.RULES:
            _check(dev, host, row_c, (0.5, 0.3, 0.2), rule, logits, 1, rule == "prob" and not logits)
        host, dev = _members(rng, 5, 4096, 3, logits, [4096, 4100, 4104])
        _check(dev, host, row_c, None, "prob", logits, 1, not logits)


def test_copies_and_unit_weight_return_the_member():
    """the two consequences the identity tests below rest on, on the device: M copies under ``prob`` in probability mode, and any
    members with one weight 1, give the member's matrix bit for bit"""
    rng = np.random.default_rng(4)
    host, dev = _members(rng, 21, 333, 2, False, [333, 336])
    want = np.where(host[0] > 0, host[0], 0).astype(np.float32)
    for M in (1, 2, 3, 8):
        out = ops.ensemble_combine([dev[0]] * M, Idx([333] * 21), weights=None, rule="prob", logits=False, unk=UNK)
        np.testing.assert_array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    out = ops.ensemble_combine(dev, Idx([333] * 21), weights=(1, 0), rule="prob", logits=False, unk=UNK)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    assert ops.ensemble_combine([d[:0] for d in dev], Idx([]), weights=None, rule="prob", logits=False, unk=UNK, max_cols=333).shape == (0, 333)


# ------------------------------------------------------------------------------------------------ 2. the translator: fixtures
_FIX = {}


def _other_params(cfg, mt, seed):
    return syn.draw_parameters([(n, torch.empty(s)) for n, s in parameter_shapes(cfg, mt).items()], seed=seed)


def _other_model(golden_dir, case, mt, seed=13):
    _, cfg, _, model = build_model(case, mt, golden_dir, DEV)
    missing, unexpected = model.load_state_dict(_other_params(cfg, mt, seed), strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing)
    return model


def _fixture(golden_dir, case, mt, copies=1):
    """built once per fixture and shared, never changed: cfg, batch, ``copies`` identical models and one different member (seed 13)"""
    f = _FIX.get((case, mt))
    if f is None:
        _, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
        f = _FIX[(case, mt)] = dict(cfg=cfg, batch=batch, same=[model], other=_other_model(golden_dir, case, mt), refs={})
    while len(f["same"]) < copies:
        f["same"].append(build_model(case, mt, golden_dir, DEV)[3])
    return f


def _single(cfg, model, **kw):
    from svpc_amd.translator import Translator
    return Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, **kw)


def _ensemble(cfg, models, **kw):
    from svpc_amd.ensemble import EnsembleTranslator
    return EnsembleTranslator(O(), [{"model_cfg": cfg, "model": m.state_dict()} for m in models], models, **kw)


def _phrases(batch):
    return [[[(11, 12)] for _ in range(int(s))] for s in batch["batch_step_num"]]


STRATEGIES = {
    "greedy": lambda tr, mi, b: tr.translate_batch(mi),
    "beam3": lambda tr, mi, b: tr.translate_batch_beam(mi, 3),
    "nbest": lambda tr, mi, b: tr.translate_batch_nbest(mi, 3, 3, block_ngram_repeat=2, min_length=2, length_penalty_name="avg"),
    "paragraph": lambda tr, mi, b: tr.translate_batch_nbest(mi, 3, 2, block_ngram_repeat=2, block_ngram_scope="paragraph"),
    "diverse": lambda tr, mi, b: tr.translate_batch_diverse(mi, 4, 2, 0.5),
    "constrained": lambda tr, mi, b: tr.translate_batch_constrained(mi, _phrases(b), 3),
    "sample": lambda tr, mi, b: tr.translate_batch_sample(mi, 3, seed=5, random_sampling_topk=10, random_sampling_topp=0.9),
    "stochastic": lambda tr, mi, b: tr.translate_batch_stochastic(mi, 3, seed=5),
}


def _tensors(result):
    """every per-video tensor list of a decode's result tuple (the OOV dictionary at index 1 left out), flattened"""
    return [t for k, lst in enumerate(result) if k != 1 for t in lst]


def _same(a, b, what):
    ta, tb = _tensors(a), _tensors(b)
    assert len(ta) == len(tb) and len(ta) > 0
    for x, y in zip(ta, tb):
        assert x.dtype == y.dtype and torch.equal(x, y), what


# ------------------------------------------------------------------------------------------------ 3. identity
def _identity(golden_dir, case, mt, graph, strategy):
    f = _fixture(golden_dir, case, mt, copies=3)
    cfg, batch = f["cfg"], f["batch"]
    run = STRATEGIES[strategy]
    want = run(_single(cfg, f["same"][0]), syn.translate_inputs(batch), batch)
    copies = _ensemble(cfg, f["same"][:3], graph=graph)
    unit = _ensemble(cfg, [f["same"][0], f["other"]], weights=(1, 0), graph=graph)
    for _ in range(2 if graph else 1):                       # (graph: the second call replays)
        _same(run(copies, syn.translate_inputs(batch), batch), want, "3 copies, %s" % strategy)
        _same(run(unit, syn.translate_inputs(batch), batch), want, "weights (1, 0), %s" % strategy)
    if graph:
        assert all(dp.graphs for dp in copies._preps.values()) and all(dp.graphs for dp in unit._preps.values())
    return copies, want


@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("case,mt", [("tiny", "vivt"), ("c1", "vivt")])
def test_identical_members_decode_what_one_model_decodes(golden_dir, case, mt, graph, strategy):
    copies, want = _identity(golden_dir, case, mt, graph, strategy)
    if strategy == "nbest":         # forced scoring of the ensemble's own n-best rows: the plain translator's, entry by entry
        f = _fixture(golden_dir, case, mt)
        a = copies.score_captions(syn.translate_inputs(f["batch"]), want[0])
        b = _single(f["cfg"], f["same"][0], graph=graph).score_captions(syn.translate_inputs(f["batch"]), want[0])
        assert sorted(vars(a)) == sorted(vars(b))
        for k, v in vars(b).items():
            for x, y in zip(getattr(a, k), v) if isinstance(v, list) else [(getattr(a, k), v)]:
                assert torch.equal(x, y), k


@pytest.mark.parametrize("strategy", ["beam3", "sample"])
def test_identical_members_in_bf16x3(golden_dir, strategy):
    """the members' matrices are identical whatever the arithmetic, so the identity holds in the headline precision too"""
    ops.set_precision("bf16x3")
    try:
        models = [build_model("c1", "vivt", golden_dir, DEV) for _ in range(3)]
        cfg, batch = models[0][1], models[0][2]
        run = STRATEGIES[strategy]
        want = run(_single(cfg, models[0][3]), syn.translate_inputs(batch), batch)
        _same(run(_ensemble(cfg, [m[3] for m in models]), syn.translate_inputs(batch), batch), want, strategy)
    finally:
        ops.set_precision("fp32")


# ------------------------------------------------------------------------------------------------ 4. two different members
def _reference(f, leg, rule, weights):
    """the CPU ensemble decode of one leg and setting: computed once, shared, never changed"""
    key = (leg, rule, weights)
    if key not in f["refs"]:
        cfg, batch = f["cfg"], f["batch"]
        Ps = [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in (f["same"][0], f["other"])]
        cpu = {k: ([t.cpu() for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor) else
                   (v.cpu() if isinstance(v, torch.Tensor) else v)) for k, v in batch.items()}
        args = (Ps, cfg, cpu["input_ids_list"], cpu["video_features_list"], cpu["input_masks_list"], cpu["ingr_input_ids"],
                cpu["ingr_sep_masks"], cpu["batch_step_num"], cpu["ingr_id_dict"], cpu["oov_word_dict"])
        if leg == "greedy":
            f["refs"][key] = er.ensemble_greedy(*args, weights=weights, rule=rule)
        elif leg == "beam3":
            f["refs"][key] = er.ensemble_beam_decode(*args, 3, weights=weights, rule=rule)
        else:
            f["refs"][key] = er.ensemble_sample_decode(*args, 3, 5, weights=weights, rule=rule)
    return f["refs"][key]


@pytest.mark.parametrize("leg", ["greedy", "beam3", "sample"])
@pytest.mark.parametrize("rule,weights", SETTINGS)
@pytest.mark.parametrize("case,mt", [("tiny", "v"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")])
def test_two_members_against_the_cpu_reference(golden_dir, case, mt, rule, weights, leg):
    f = _fixture(golden_dir, case, mt)
    cfg, batch = f["cfg"], f["batch"]
    tr = _ensemble(cfg, [f["same"][0], f["other"]], weights=weights, combine=rule)
    ref = _reference(f, leg, rule, weights)
    mi = syn.translate_inputs(batch)
    near = total = 0
    if leg == "greedy":
        dec, _ = tr.translate_batch(mi)
        for d, ri, rm in zip(dec, *ref):
            d = d.cpu()
            for s in range(ri.shape[0]):
                total += 1
                if not torch.equal(d[s], ri[s]):
                    assert float(rm[s].min()) <= TIE, ("ids differ without a near-tie", d[s].tolist(), ri[s].tolist(), float(rm[s].min()))
                    near += 1
    elif leg == "beam3":
        dec, _, scores = tr.translate_batch_beam(mi, 3)
        for d, sc, ri, rs, rm in zip(dec, scores, *ref):
            d, sc = d.cpu(), sc.cpu().numpy()
            for s in range(ri.shape[0]):
                total += 1
                if torch.equal(d[s], ri[s]):
                    np.testing.assert_allclose(sc[s], rs[s], rtol=1e-4, atol=1e-6)
                    continue
                assert float(rm[s].min()) <= TIE, ("ids differ without a near-tie", d[s].tolist(), ri[s].tolist(), float(rm[s].min()))
                near += 1
    else:
        dec, _, cums, lens = tr.translate_batch_sample(mi, 3, seed=5)
        for d, c, ln, ri, rc, rl, rm in zip(dec, cums, lens, *ref):
            d, c, ln = d.cpu(), c.cpu().numpy(), ln.cpu().numpy()
            for s in range(d.shape[0]):
                for j in range(d.shape[1]):
                    total += 1
                    if torch.equal(d[s, j], ri[s, j]):
                        np.testing.assert_allclose(c[s, j], rc[s, j], rtol=1e-4, atol=1e-6)
                        assert ln[s, j] == rl[s, j]
                        continue
                    assert rm[s, j] <= TIE, ("ids differ without a near-tie", d[s, j].tolist(), ri[s, j].tolist(), float(rm[s, j]))
                    near += 1
    print("%s %s %s %s: %d of %d rows decided within %.0e" % (case, mt, rule, leg, near, total, TIE))
    assert total > 0 and near <= max(1, total // 20), (near, total)


@pytest.mark.parametrize("rule,weights", SETTINGS)
@pytest.mark.parametrize("case,mt", [("tiny", "v"), ("tiny", "vivt"), ("c1", "vivt")])
def test_forced_scores_of_the_ensemble_s_own_rows(golden_dir, case, mt, rule, weights):
    """``score_captions`` of the two-member ensemble's beam-3 rows reproduces the beam's cum (test_forced_score_gpu's bound), its
    lengths and its finished flags"""
    f = _fixture(golden_dir, case, mt)
    tr = _ensemble(f["cfg"], [f["same"][0], f["other"]], weights=weights, combine=rule)
    dec, _, sc, ln = tr.translate_batch_nbest(syn.translate_inputs(f["batch"]), 3, 3)
    got = tr.score_captions(syn.translate_inputs(f["batch"]), dec)
    for b in range(len(dec)):
        np.testing.assert_allclose(got.score_list[b].cpu().numpy(), sc[b].cpu().numpy(), rtol=1e-4, atol=1e-6)
        np.testing.assert_array_equal(got.length_list[b].cpu().numpy(), ln[b].cpu().numpy())
        np.testing.assert_array_equal(got.finished_list[b].cpu().numpy().astype(bool), (dec[b][:, :, 1:] == EOS).any(-1).cpu().numpy())


# ------------------------------------------------------------------------------------------------ 5. graph replay
@pytest.mark.parametrize("case,mt", [("tiny", "vivt"), ("c1", "v")])
def test_graph_replay_and_recapture(golden_dir, case, mt):
    """replays equal the eager decode; after new parameters are loaded into member 1 ONLY the next call re-captures (the validity
    signature sees every member) and equals the eager decode of the new ensemble"""
    _, cfg, batch, m0 = build_model(case, mt, golden_dir, DEV)
    m1 = _other_model(golden_dir, case, mt)
    eager, graphed = _ensemble(cfg, [m0, m1]), _ensemble(cfg, [m0, m1], graph=True)
    legs = [STRATEGIES["beam3"], STRATEGIES["sample"]]

    def agree(times):
        for run in legs:
            want = run(eager, syn.translate_inputs(batch), batch)
            for _ in range(times):
                _same(run(graphed, syn.translate_inputs(batch), batch), want, "graph replay")
        return [t.clone() for run in legs for t in _tensors(run(eager, syn.translate_inputs(batch), batch))]

    before = agree(2)                                        # capture, then replay
    graphs = {k: next(iter(dp.graphs.values()))[0] for k, dp in graphed._preps.items()}
    assert len(graphs) == 2
    missing, unexpected = m1.load_state_dict(_other_params(cfg, mt, 14), strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing)
    after = agree(1)
    assert any(not torch.equal(a, b) for a, b in zip(before, after)), "the new member decodes what the old one did"
    for k, dp in graphed._preps.items():
        assert next(iter(dp.graphs.values()))[0] is not graphs[k], "member 1 changed and the graph was not re-captured"
