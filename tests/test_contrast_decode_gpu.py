"""Contrastive decoding on the MI355X: the combine kernel (svpc_contrast_combine) against tests/contrast_decode_reference.py::combine, and
``ContrastTranslator`` end to end — the same kernel on the same inputs as the two single ``Translator``s' matrices, β = 0 / α = 0 against
the plain ``Translator``, both amateurs against the CPU contrastive decodes (fp32), forced scoring of the translator's own rows, graph
replay and re-capture, and the rest of the decode surface.

Bounds.  Head membership is an exact maximum and one rounded product (or difference): ``out`` is exactly 0 wherever the reference's head
mask is false and in the padding, and a single-column head gives exactly 1.0.  Elsewhere the device's fp64 exp / log may differ from
libm's in the last fp64 bits, and after the single rounding to fp32 that is at most 1 fp32 ulp: ``assert_array_max_ulp(maxulp=1)``, the
bound the ensemble's transcendental legs meet.  Decodes against the CPU reference follow test_ensemble_gpu: ids and lengths exact, cum
within rtol 1e-4 / atol 1e-6, a row may differ only where the reference's own pick margin OR HEAD MARGIN (the smallest distance of any
column's log p_e to the head's threshold log α + log p_e,top, over the row's steps: such a column may legitimately flip) is ≤ 1e-4, and
such rows are at most max(1, total // 20).

The CPU reference alone over these settings (profiles/contrast_decode_parity.json; rows with a pick or head margin ≤ 1e-4 of the
rows decoded; the amateur's parameters are drawn with seed 13, as the ensemble's second member):
  tiny v     (β 0.5, seed-13 amateur): greedy 0/5, beam3 0/5, sample 0/15;   (β 1, zero-video self-amateur): 1/5, 0/5, 0/15
  tiny vivt  (β 0.5, seed-13 amateur): greedy 1/5, beam3 1/5, sample 0/15;   (β 1, zero-video self-amateur): 0/5, 0/5, 0/15
  c1 vivt    (β 0.5, seed-13 amateur): greedy 0/7, beam3 0/7, sample 1/21;   (β 1, zero-video self-amateur): 4/7, 0/7, 0/21
  c1 v       (β 0.5, seed-13 amateur): greedy 4/7, beam3 7/7, sample 13/21;  (β 1, zero-video self-amateur): 5/7, 7/7, 16/21
The smallest pick margin is 5.4e-7 (greedy, c1 vivt, self-amateur), the smallest head margin 1.8e-6 (sample, c1 v, seed-13 amateur).
On c1 v (``video`` mode, raw logits) the count is the EXPERT's: its ≈ 20 steps × several hundred logits put a column within 1e-4 of
log α below the top in most rows whatever the amateur — amateur seeds 13 … 23 were tried on the reference alone and leave 23 … 32 such
rows in all, none fewer than 23 (seed 22; all of them on c1 v) — so no seed brings the reference by itself under the cap there, and
the self-amateur has no seed to choose.  Seed 13 is kept.  These are rows that MAY differ; the test counts the rows that DO: on the
MI355X none differed in any of the 24 legs."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import contrast_decode_reference as cr  # noqa: E402
import ensemble_reference as er  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import ops, synthetic as syn  # noqa: E402
from svpc_amd.model_shapes import parameter_shapes  # noqa: E402
from svpc_amd.ops_common import Idx  # noqa: E402
from svpc_amd.synthetic import EOS, IGNORE, PAD, UNK  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = type("O", (), {"cuda": True})
TIE = 1e-4
COEF = [(1.5, 0.5, 0.1), (1.0, 1.0, 0.1), (1.0, 0.0, 0.0), (2.0, 1.0, 1.0), (1.5, 0.5, 1e-6)]
FIXTURES = [("tiny", "v"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")]
SETTINGS = {"separate": dict(beta=0.5, alpha=0.1), "self_zero": dict(beta=1.0, alpha=0.1, amateur_video="zero")}


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _pair(rng, n_rows, cmax, row_c, rows_per, logits, lds, offset=False):
    """(expert, amateur) host float32 (n_rows, cmax) matrices and their device copies with leading dimensions ``lds``, salted as
    test_ensemble_gpu._members salts its members — exact zeros, denormals and negative probabilities; −inf logits; a huge UNK value that
    must not leak —, with one dead amateur row (n_rows // 2), one dead expert row (the last, when there are ≥ 3 rows), a row whose head
    is a single column (row 0 for α ≥ 0.1) and a row with three columns exactly tied at the top (row 1, when there are ≥ 3 rows)"""
    host, dev = [], []
    for m in range(2):
        if logits:
            s = (rng.standard_normal((n_rows, cmax)) * 3).astype(np.float32)
            s[rng.random((n_rows, cmax)) < 0.05] = -np.inf
            s[:, UNK] = 80.0
        else:
            s = (rng.random((n_rows, cmax)) ** 4).astype(np.float32)
            s[rng.random((n_rows, cmax)) < 0.1] = 0.0
            s[rng.random((n_rows, cmax)) < 0.02] = 1e-40
            s[rng.random((n_rows, cmax)) < 0.01] = -0.5
            s[:, UNK] = 1.0
        if m == 1:
            s[n_rows // 2, :] = -np.inf if logits else 0.0
            s[n_rows // 2, UNK] = 80.0 if logits else 1.0
        else:
            if logits:
                s[0, 3] = 40.0                               # alone within log 0.1 of the top
            else:
                s[0, :] *= np.float32(0.05)
                s[0, 3] = 0.9
                s[0, UNK] = 1.0
            if n_rows >= 3:
                s[1, [2, 9, 12]] = 50.0 if logits else 1.0   # three columns exactly tied at the top (all rows have ≥ 16 columns)
                s[n_rows - 1, :] = -np.inf if logits else 0.0
                s[n_rows - 1, UNK] = 80.0 if logits else 1.0
        buf = torch.full((n_rows * lds[m] + 1,), 7.0, dtype=torch.float32, device=DEV)
        d = buf[1:] if offset and m == 0 else buf[:-1]
        d = d.view(n_rows, lds[m])
        d[:, :cmax] = torch.from_numpy(s).to(DEV)
        host.append(s)
        dev.append(d)
    return host, dev


def _check(dev, host, row_c, coef, logits, rows_per):
    we, wa, alpha = coef
    cmax = max(row_c)
    out = ops.contrast_combine(dev[0], dev[1], Idx(row_c), expert_weight=we, amateur_weight=wa, alpha=alpha, logits=logits, unk=UNK,
                               rows_per=rows_per, max_cols=cmax)
    torch.cuda.synchronize()
    assert out.shape == (host[0].shape[0], cmax) and out.is_contiguous()
    out = out.cpu().numpy()
    ref, mask = cr.combine(host[0], host[1], row_c, we, wa, alpha, logits, UNK, rows_per, ld_out=cmax)
    assert out.shape == ref.shape and np.all(np.isfinite(out))
    assert np.all(out[~mask] == 0) and not mask[:, UNK:UNK + 1].any()        # outside the head, UNK and the padding: exactly 0
    single = mask.sum(1) == 1
    assert np.all(out[single][mask[single]] == np.float32(1.0))              # a head of one column: exactly 1.0
    np.testing.assert_array_max_ulp(out, ref, maxulp=1)
    return out, mask


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("coef", COEF)
def test_kernel_equals_combine(coef, logits):
    rng = np.random.default_rng(int(coef[0] * 10 + coef[1] * 100 + coef[2] * 7) + 1000 * logits)
    for n_rows in (1, 21):                                  # 21: 7 sentences × 3 rows, more than one workgroup
        for rows_per in (1, 5):
            n_c = -(-n_rows // rows_per)
            row_c = [int(c) for c in rng.integers(16, 700, size=n_c)] if rows_per > 1 else \
                [int(c) for c in np.repeat(rng.integers(16, 700, size=-(-n_rows // 3)), 3)[:n_rows]]
            cmax = max(row_c)
            # leading dimensions: equal; odd and differing between expert, amateur and output; a 4-byte-offset base pointer
            for lds, offset in (([cmax, cmax], False), ([cmax + 3, cmax + 8], False), ([cmax + 5, cmax + 1], True)):
                host, dev = _pair(rng, n_rows, cmax, row_c, rows_per, logits, lds, offset)
                out, mask = _check(dev, host, row_c, coef, logits, rows_per)
                if coef[2] >= 0.1:
                    assert mask[0].sum() == 1 and out[0, 3] == 1.0
                if coef[2] == 1.0 and n_rows >= 3 and min(row_c) > 12:
                    assert mask[1].sum() == 3 and np.all(mask[1, [2, 9, 12]])
                if n_rows >= 3:
                    assert not mask[n_rows - 1].any()                        # the dead expert row
                    assert mask[n_rows // 2].any()                           # the dead amateur row still decodes


@pytest.mark.parametrize("logits", [False, True])
def test_kernel_wide_rows_and_a_row_of_one_column(logits):
    """rows of 4,096 columns, the widest the step kernels take; and rows of exactly one column"""
    rng = np.random.default_rng(9 + logits)
    row_c = [4096, 1025, 4096, 3000, 4095]
    host, dev = _pair(rng, 5, 4096, row_c, 1, logits, [4096, 4099])
    for coef in COEF:
        _check(dev, host, row_c, coef, logits, 1)
    host, dev = _pair(rng, 5, 4096, row_c, 1, logits, [4100, 4096], offset=True)
    _check(dev, host, row_c, COEF[0], logits, 1)
    one = np.array([[2.5 if logits else 0.3], [-np.inf if logits else 0.0], [-70.0 if logits else 1e-40]], np.float32)
    am = np.array([[0.1], [0.2], [-np.inf if logits else 0.0]], np.float32)
    for ld in (1, 3):
        d = [torch.full((3, ld), 7.0, device=DEV), torch.full((3, ld), 7.0, device=DEV)]
        d[0][:, :1], d[1][:, :1] = torch.from_numpy(one).to(DEV), torch.from_numpy(am).to(DEV)
        for coef in COEF:
            out, mask = _check(d, [one, am], [1, 1, 1], coef, logits, 1)
            assert out[:, 0].tolist() == [1.0, 0.0, 1.0]
    empty = ops.contrast_combine(dev[0][:0], dev[1][:0], Idx([]), expert_weight=1.5, amateur_weight=0.5, alpha=0.1, logits=logits,
                                 unk=UNK, max_cols=333)
    assert empty.shape == (0, 333)


# ------------------------------------------------------------------------------------------------ 2. the translator: fixtures
_FIX = {}


def _other_params(cfg, mt, seed):
    return syn.draw_parameters([(n, torch.empty(s)) for n, s in parameter_shapes(cfg, mt).items()], seed=seed)


def _other_model(golden_dir, case, mt, seed=13):
    """a second model of the fixture's shapes, drawn as tests/test_ensemble_gpu.py::_other_model draws the ensemble's second member"""
    _, cfg, _, model = build_model(case, mt, golden_dir, DEV)
    missing, unexpected = model.load_state_dict(_other_params(cfg, mt, seed), strict=False)
    assert not unexpected and all(k.endswith(".pe") for k in missing)
    return model


def _fixture(golden_dir, case, mt):
    """built once per fixture and shared, never changed: cfg, batch, the expert, the seed-13 amateur, and the CPU references"""
    f = _FIX.get((case, mt))
    if f is None:
        _, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
        f = _FIX[(case, mt)] = dict(cfg=cfg, batch=batch, expert=model, other=_other_model(golden_dir, case, mt), refs={})
    return f


def _ck(cfg, model):
    return {"model_cfg": cfg, "model": model.state_dict()}


def _single(cfg, model, **kw):
    from svpc_amd.translator import Translator
    return Translator(O(), _ck(cfg, model), model=model, **kw)


def _contrast(f, setting, **kw):
    from svpc_amd.contrast_decode import ContrastTranslator
    kw = dict(SETTINGS[setting], **kw)
    if setting == "separate":
        return ContrastTranslator(O(), _ck(f["cfg"], f["expert"]), f["expert"], _ck(f["cfg"], f["other"]), f["other"], **kw)
    return ContrastTranslator(O(), _ck(f["cfg"], f["expert"]), f["expert"], **kw)


def _zeroed(batch):
    b = dict(batch)
    b["video_features_list"] = [torch.zeros_like(t) for t in batch["video_features_list"]]
    return b


def _tensors(result):
    return [t for k, lst in enumerate(result) if k != 1 for t in lst]


def _same(a, b, what):
    ta, tb = _tensors(a), _tensors(b)
    assert len(ta) == len(tb) and len(ta) > 0
    for x, y in zip(ta, tb):
        assert x.dtype == y.dtype and torch.equal(x, y), what


def _cpu_args(f):
    cfg, batch = f["cfg"], f["batch"]
    cpu = {k: ([t.cpu() for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor) else
               (v.cpu() if isinstance(v, torch.Tensor) else v)) for k, v in batch.items()}
    return (cfg, cpu["input_ids_list"], cpu["video_features_list"], cpu["input_masks_list"], cpu["ingr_input_ids"],
            cpu["ingr_sep_masks"], cpu["batch_step_num"], cpu["ingr_id_dict"], cpu["oov_word_dict"])


def _params(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


# ------------------------------------------------------------------------------------------------ 3. same kernel, same inputs
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("case,mt", [("tiny", "v"), ("c1", "vivt")])
def test_teacher_scores_are_the_kernel_over_the_two_models_matrices(golden_dir, case, mt, setting):
    f = _fixture(golden_dir, case, mt)
    cfg, batch = f["cfg"], f["batch"]
    expert = _single(cfg, f["expert"])
    dec = expert.translate_batch_nbest(syn.translate_inputs(batch), 3, 2)[0]
    e = expert.teacher_scores(syn.translate_inputs(batch), dec)
    if setting == "separate":
        a = _single(cfg, f["other"]).teacher_scores(syn.translate_inputs(batch), dec)
    else:                                                   # the amateur is fed explicitly zeroed features
        a = expert.teacher_scores(syn.translate_inputs(_zeroed(batch)), dec)
    tr = _contrast(f, setting)
    got = tr.teacher_scores(syn.translate_inputs(batch), dec)
    assert e.logits == a.logits == (mt == "v") and got.logits is False and (got.T, got.K, got.Lt) == (e.T, e.K, e.Lt)
    want = ops.contrast_combine(e.scores, a.scores, e.cap_c, expert_weight=tr.expert_weight, amateur_weight=tr.amateur_weight,
                                alpha=tr.alpha, logits=e.logits, unk=UNK, rows_per=e.Lt, max_cols=e.max_cols)
    assert got.scores.shape == want.shape and torch.equal(got.scores, want)
    assert not torch.equal(e.scores, a.scores)
    rows = want.sum(1)                                      # every row a distribution over its head
    assert torch.allclose(rows, torch.ones_like(rows), rtol=0, atol=1e-5)


# ------------------------------------------------------------------------------------------------ 4. wa = 0, α = 0
@pytest.mark.parametrize("case,mt", FIXTURES)
def test_no_amateur_weight_and_no_threshold_decodes_what_the_expert_decodes(golden_dir, case, mt):
    """β = 0, α = 0: the step distribution is the expert's, renormalised without UNK, so greedy picks the expert's words; a row is
    excused only where the single model's own margin (the CPU greedy of the expert alone) is ≤ 1e-4"""
    f = _fixture(golden_dir, case, mt)
    cfg, batch = f["cfg"], f["batch"]
    want = _single(cfg, f["expert"]).translate_batch(syn.translate_inputs(batch))[0]
    _, margins = er.ensemble_greedy([_params(f["expert"])], *_cpu_args(f))
    for setting in sorted(SETTINGS):
        tr = _contrast(f, setting, beta=0.0, alpha=0.0)
        assert tr.expert_weight == 1.0 and tr.amateur_weight == 0.0
        got = tr.translate_batch(syn.translate_inputs(batch))[0]
        total = 0
        for d, w, mg in zip(got, want, margins):
            for s in range(w.shape[0]):
                total += 1
                if not torch.equal(d[s], w[s]):
                    assert float(np.nanmin(mg[s])) <= TIE, ("ids differ without a near-tie", setting, d[s].tolist(), w[s].tolist())
        assert total > 0


# ------------------------------------------------------------------------------------------------ 5. against the CPU decodes
def _zero(feats):
    return torch.zeros_like(feats)


def _reference(f, leg, setting):
    """the CPU contrastive decode of one leg and setting: computed once, shared, never changed"""
    key = (leg, setting)
    if key not in f["refs"]:
        kw = SETTINGS[setting]
        coef = (1.0 + kw["beta"], kw["beta"], kw["alpha"])
        Ps = [_params(f["expert"]), _params(f["other"] if setting == "separate" else f["expert"])]
        tf = (None, None) if setting == "separate" else (None, _zero)
        args = (Ps,) + _cpu_args(f)
        if leg == "greedy":
            f["refs"][key] = cr.contrast_greedy(*args, coef, tf)
        elif leg == "beam3":
            f["refs"][key] = cr.contrast_beam_decode(*args, 3, coef, tf)
        else:
            f["refs"][key] = cr.contrast_sample_decode(*args, 3, 5, coef, tf)
    return f["refs"][key]


@pytest.mark.parametrize("leg", ["greedy", "beam3", "sample"])
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("case,mt", FIXTURES)
def test_against_the_cpu_reference(golden_dir, case, mt, setting, leg):
    f = _fixture(golden_dir, case, mt)
    tr = _contrast(f, setting)
    ref = _reference(f, leg, setting)
    mi = syn.translate_inputs(f["batch"])
    near = total = 0

    def excused(pick_margin, head_margin, what):
        m = min(float(np.nanmin(pick_margin)), float(head_margin))
        assert m <= TIE, ("ids differ without a near-tie",) + what + (float(np.nanmin(pick_margin)), float(head_margin))

    if leg == "greedy":
        dec, _ = tr.translate_batch(mi)
        for d, ri, rm, rh in zip(dec, *ref):
            d = d.cpu()
            for s in range(ri.shape[0]):
                total += 1
                if not torch.equal(d[s], ri[s]):
                    excused(rm[s], rh[s], (d[s].tolist(), ri[s].tolist()))
                    near += 1
    elif leg == "beam3":
        dec, _, scores = tr.translate_batch_beam(mi, 3)
        for d, sc, ri, rs, rm, rh in zip(dec, scores, *ref):
            d, sc = d.cpu(), sc.cpu().numpy()
            for s in range(ri.shape[0]):
                total += 1
                if torch.equal(d[s], ri[s]) and (rh[s] > TIE or np.allclose(sc[s], rs[s], rtol=1e-4, atol=1e-6)):
                    np.testing.assert_allclose(sc[s], rs[s], rtol=1e-4, atol=1e-6)
                    continue
                excused(rm[s], rh[s], (d[s].tolist(), ri[s].tolist()))
                near += 1
    else:
        dec, _, cums, lens = tr.translate_batch_sample(mi, 3, seed=5)
        for d, c, ln, ri, rc, rl, rm, rh in zip(dec, cums, lens, *ref):
            d, c, ln = d.cpu(), c.cpu().numpy(), ln.cpu().numpy()
            for s in range(d.shape[0]):
                for j in range(d.shape[1]):
                    total += 1
                    if torch.equal(d[s, j], ri[s, j]) and (rh[s, j] > TIE or np.allclose(c[s, j], rc[s, j], rtol=1e-4, atol=1e-6)):
                        np.testing.assert_allclose(c[s, j], rc[s, j], rtol=1e-4, atol=1e-6)
                        assert ln[s, j] == rl[s, j]
                        continue
                    excused(np.asarray(rm[s, j]), rh[s, j], (d[s, j].tolist(), ri[s, j].tolist()))
                    near += 1
    print("%s %s %s %s: %d of %d rows differ, all decided within %.0e" % (case, mt, setting, leg, near, total, TIE))
    assert total > 0 and near <= max(1, total // 20), (near, total)


# ------------------------------------------------------------------------------------------------ 6. forced scoring
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("case,mt", [("tiny", "v"), ("tiny", "vivt"), ("c1", "vivt")])
def test_forced_scores_of_the_translator_s_own_rows(golden_dir, case, mt, setting):
    """``score_captions`` of the translator's beam-3 rows reproduces the beam's cum, its lengths and its finished flags"""
    f = _fixture(golden_dir, case, mt)
    tr = _contrast(f, setting)
    dec, _, sc, ln = tr.translate_batch_nbest(syn.translate_inputs(f["batch"]), 3, 3)
    got = tr.score_captions(syn.translate_inputs(f["batch"]), dec)
    for b in range(len(dec)):
        np.testing.assert_allclose(got.score_list[b].cpu().numpy(), sc[b].cpu().numpy(), rtol=1e-4, atol=1e-6)
        np.testing.assert_array_equal(got.length_list[b].cpu().numpy(), ln[b].cpu().numpy())
        np.testing.assert_array_equal(got.finished_list[b].cpu().numpy().astype(bool), (dec[b][:, :, 1:] == EOS).any(-1).cpu().numpy())


# ------------------------------------------------------------------------------------------------ 7. graph replay
STRATEGIES = {
    "beam3": lambda tr, mi, b: tr.translate_batch_beam(mi, 3),
    "sample": lambda tr, mi, b: tr.translate_batch_sample(mi, 3, seed=5, random_sampling_topk=10, random_sampling_topp=0.9),
}


def test_graph_replay_and_recapture(golden_dir):
    """replays equal the eager decode; after new parameters are loaded into the AMATEUR only, the next call re-captures (the validity
    signature sees both members) and equals the eager decode of the new pair; the self-amateur's graph replays its eager decode too"""
    from svpc_amd.contrast_decode import ContrastTranslator
    case, mt = "c1", "vivt"
    _, cfg, batch, m0 = build_model(case, mt, golden_dir, DEV)
    m1 = _other_model(golden_dir, case, mt)
    eager = ContrastTranslator(O(), _ck(cfg, m0), m0, _ck(cfg, m1), m1)
    graphed = ContrastTranslator(O(), _ck(cfg, m0), m0, _ck(cfg, m1), m1, graph=True)
    assert graphed._members() == [m0, m1]
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
    assert any(not torch.equal(a, b) for a, b in zip(before, after)), "the new amateur decodes what the old one did"
    for k, dp in graphed._preps.items():
        assert next(iter(dp.graphs.values()))[0] is not graphs[k], "the amateur changed and the graph was not re-captured"
    own = [ContrastTranslator(O(), _ck(cfg, m0), m0, amateur_video="zero", beta=1.0, graph=g) for g in (False, True)]
    want = legs[0](own[0], syn.translate_inputs(batch), batch)
    for _ in range(2):
        _same(legs[0](own[1], syn.translate_inputs(batch), batch), want, "self-amateur graph replay")
    assert all(dp.graphs for dp in own[1]._preps.values()) and len(own[1]._zero_feats) == 1


# ------------------------------------------------------------------------------------------------ 8. the rest of the surface
def test_self_amateur_in_bf16x3_replays_its_eager_decode(golden_dir):
    """beam 3 in the headline precision: the graph's replay equals the same translator's eager decode (no cross-precision claim)"""
    from svpc_amd.contrast_decode import ContrastTranslator
    ops.set_precision("bf16x3")
    try:
        _, cfg, batch, model = build_model("c1", "vivt", golden_dir, DEV)
        eager, graphed = [ContrastTranslator(O(), _ck(cfg, model), model, amateur_video="zero", beta=1.0, graph=g) for g in (False, True)]
        want = STRATEGIES["beam3"](eager, syn.translate_inputs(batch), batch)
        for _ in range(2):
            _same(STRATEGIES["beam3"](graphed, syn.translate_inputs(batch), batch), want, "bf16x3 replay")
    finally:
        ops.set_precision("fp32")


def _consensus_plan(cfg, batch):
    from svpc_amd.caption_scores import ReferenceCorpus
    Vm = cfg.vocab_size
    i2w = ["[PAD]", "[CLS]", "[SEP]", "[VID]", "[BOS]", "[EOS]", "[UNK]"] + \
        ["".join(chr(97 + (i // 26 ** k) % 26) for k in range(3)) for i in range(7, Vm)]
    refs = {}
    for b in range(len(batch["batch_step_num"])):            # the idf corpus: the synthetic labels as "training references"
        inv = {int(v): k for k, v in batch["oov_word_dict"][b].items()}
        sents = []
        for s in range(int(batch["batch_step_num"][b])):
            lab = batch["input_labels_list"][s][b].cpu().tolist()
            sents.append(" ".join(i2w[x] if x < Vm else inv[x] for x in lab if x not in (IGNORE, EOS, PAD)))
        refs["vid%d" % b] = [" ".join(sents)]
    return ReferenceCorpus(i2w, refs, device=DEV).plan([dict(oov_word_dict=d) for d in batch["oov_word_dict"]], references=False)


REST = {
    "nbest": lambda tr, mi, b, plan: tr.translate_batch_nbest(mi, 3, 3, block_ngram_repeat=2, min_length=2, length_penalty_name="avg"),
    "paragraph": lambda tr, mi, b, plan: tr.translate_batch_nbest(mi, 3, 2, block_ngram_repeat=2, block_ngram_scope="paragraph"),
    "diverse": lambda tr, mi, b, plan: tr.translate_batch_diverse(mi, 4, 2, 0.5),
    "constrained": lambda tr, mi, b, plan: tr.translate_batch_constrained(mi, [[[(11, 12)] for _ in range(int(s))] for s in b["batch_step_num"]], 3),
    "stochastic": lambda tr, mi, b, plan: tr.translate_batch_stochastic(mi, 3, seed=5),
    "consensus": lambda tr, mi, b, plan: tr.translate_batch_consensus(mi, plan, source="sample", num_candidates=3, seed=17),
}


@pytest.mark.parametrize("strategy", sorted(REST))
def test_every_other_strategy_runs(golden_dir, strategy):
    f = _fixture(golden_dir, "tiny", "vivt")
    cfg, batch = f["cfg"], f["batch"]
    plan = _consensus_plan(cfg, batch) if strategy == "consensus" else None
    for setting in sorted(SETTINGS):
        res = REST[strategy](_contrast(f, setting), syn.translate_inputs(batch), batch, plan)
        dec = res[0]
        assert len(dec) == len(batch["batch_step_num"])
        for b, d in enumerate(dec):
            C = cfg.vocab_size + len(batch["oov_word_dict"][b])
            assert d.dtype == torch.int64 and d.shape[0] == int(batch["batch_step_num"][b]) and d.shape[-1] == cfg.max_t_len
            assert int(d.min()) >= 0 and int(d.max()) < C and not bool((d == UNK).any())
        if strategy != "consensus":
            for sc in res[2]:                                # (the head may hold fewer words than the beam is wide: a lower-ranked row may be
                best = sc.reshape(sc.shape[0], -1)[:, 0]     #  an empty slot at −inf; the first row of every sentence is a caption)
                assert sc.dtype == torch.float32 and bool(torch.isfinite(best).all()) and not bool(torch.isnan(sc).any())
