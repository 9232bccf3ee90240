"""Knowledge distillation without a GPU: the restatement (tests/distill_reference.py) on the literal anchor, the clamp, a
logits row against torch autograd in the four flag combinations, unnormalised and empty teacher rows, Gibbs' inequality, every host check,
no CPU fallback, the exported symbols, and the margins of the fixed inputs the GPU tests run on."""
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

import distill_cases as dc  # noqa: E402
import distill_reference as dr  # noqa: E402
from svpc_amd import _lib, ops  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, PAD, UNK  # noqa: E402

f32 = np.float32


# ------------------------------------------------------------------------------------------------ the restatement alone
def _anchor():
    """C = 8, caption BOS 7 EOS, probabilities in both matrices"""
    assert (BOS, EOS, UNK, PAD) == (4, 5, 6, 0)
    s = np.zeros((3, 8), np.float32)
    t = np.zeros((3, 8), np.float32)
    s[0] = 0.125
    t[0, 7], t[0, 0], t[0, UNK] = 0.5, 0.5, 0.3
    for m in (s, t):
        m[1, [0, 1, 5, 7]] = 0.25
    return s, t, np.array([[BOS, 7, EOS]]), np.array([8])


def test_literal_anchor():
    s, t, ids, rc = _anchor()
    r = dr.seq_kd(s, t, ids, rc, np.array([0.0], f32), np.array([0.5], f32), False, False)
    assert r["kdstep"].dtype == np.float32 and r["kdstep"].tolist() == [[f32(math.log(8.0)), f32(math.log(4.0))]]
    assert r["hstep"].tolist() == [[f32(math.log(2.0)), f32(math.log(4.0))]]
    assert r["kd"][0] == f32(f32(math.log(8.0)) + f32(math.log(4.0))) and r["ent"][0] == f32(f32(math.log(2.0)) + f32(math.log(4.0)))
    assert r["barred"].tolist() == [0] and r["loss"] == f32(0.5 * float(r["kd"][0]))
    d = r["dscores"].copy()
    assert d[0, 7] == -2.0 and d[0, 0] == -2.0 and d[0, UNK] == 0.0
    assert all(d[1, c] == -0.5 for c in (0, 1, 5, 7))
    d[0, [0, 7]] = 0.0
    d[1, [0, 1, 5, 7]] = 0.0
    assert not d.any()


def test_clamp():
    """p = 0 (or under ε) where q > 0: the term is −q·log ε and the gradient zero; ε is 2^-100"""
    assert dr.LOG_EPS == -100.0 * math.log(2.0) == ops.KD_LOG_EPS
    s, t, ids, rc = _anchor()
    s[0, 0] = 0.0
    r = dr.seq_kd(s, t, ids, rc, np.array([0.0], f32), np.array([0.5], f32), False, False)
    assert r["kdstep64"][0, 0] == pytest.approx(0.5 * math.log(8.0) + 0.5 * 100.0 * math.log(2.0), rel=1e-15)
    assert r["dscores"][0, 0] == 0.0 and r["dscores"][0, 7] == -2.0
    for p, clamped in ((2.0 ** -101, True), (2.0 ** -99, False), (-1.0, True)):
        s[0, 0] = p
        r = dr.seq_kd(s, t, ids, rc, np.array([0.0], f32), np.array([0.5], f32), False, False)
        assert (r["dscores"][0, 0] == 0.0) == clamped, p
    # a barred caption: no loss, no gradient, whatever the teacher says
    for logits in (False, True):
        r = dr.seq_kd(s, t, np.array([[BOS, UNK, EOS]]), rc, np.array([1.0], f32), np.array([2.0], f32), logits, False)
        assert r["barred"].tolist() == [1] and r["loss"] == 0 and not r["dscores"].any()


def _autograd(rows, trows, ids, C, w, v, dl, logits, teacher_logits):
    """the fp64 formula under torch autograd: the teacher a constant, the clamp decided on the values"""
    z = torch.tensor(rows.astype(np.float64), requires_grad=True)
    tz = torch.tensor(trows.astype(np.float64))
    keep = torch.arange(C) != UNK
    loss = torch.zeros((), dtype=torch.float64)
    for i in range(ids.shape[1] - 1):
        ell = z[i] - torch.logsumexp(z[i][keep], 0) if logits else torch.log(z[i])
        q = torch.softmax(tz[i][keep], 0) if teacher_logits else torch.clamp(tz[i][keep], min=0.0)
        q = torch.nan_to_num(q, nan=0.0)
        lk = ell[keep]
        live = (q > 0) & (lk.detach() >= dr.LOG_EPS)
        dead = (q > 0) & ~live
        loss = loss - w * ell[int(ids[0, i + 1])] - v * (q[live] * lk[live]).sum() - v * q[dead].sum() * dr.LOG_EPS
    (loss * dl).backward()
    return float(loss.detach()), z.grad.numpy()


@pytest.mark.parametrize("logits,teacher_logits", dc.FLAGS)
def test_row_against_autograd(logits, teacher_logits):
    rng = np.random.default_rng(5 + 2 * int(logits) + int(teacher_logits))
    C, Lt = 11, 4
    rows = (rng.standard_normal((Lt, C)) * 2).astype(np.float32) if logits else (rng.random((Lt, C)) * 0.2 + 0.01).astype(np.float32)
    rows[:, UNK] = 30.0 if logits else 1.0
    trows = (rng.standard_normal((Lt, C)) * 2).astype(np.float32) if teacher_logits else (rng.random((Lt, C)) * 0.2).astype(np.float32)
    trows[:, UNK] = 40.0
    trows[1, 2] = -np.inf if teacher_logits else 0.0
    rows[0, 3] = -200.0 if logits else 0.0                                       # clamped under q > 0
    ids = np.array([[BOS, 7, 8, EOS]])
    w, v, dl = np.array([0.75], f32), np.array([-1.25], f32), 2.5
    r = dr.seq_kd(rows, trows, ids, np.array([C]), w, v, logits, teacher_logits, dl=dl)
    loss, grad = _autograd(rows, trows, ids, C, float(w[0]), float(v[0]), dl, logits, teacher_logits)
    g = r["dscores"]
    np.testing.assert_allclose(g[:3], np.nan_to_num(grad[:3]), rtol=1e-10, atol=1e-12)
    assert not g[3].any() and (not g[:, UNK].any() if logits else g[0, 3] == 0)            # the last row; UNK (logits); the clamped column
    assert abs(float(r["loss"]) - loss) <= 2.0 ** -22 * abs(loss)
    acc_k, acc_h = f32(0), f32(0)                                                # the running sums are float32, position by position
    for i in range(3):
        acc_k, acc_h = f32(acc_k + r["kdstep"][0, i]), f32(acc_h + r["hstep"][0, i])
    assert r["kd"][0] == acc_k and r["ent"][0] == acc_h


def test_logits_gradient_sums_to_zero():
    """Q′ = 1 and w = 0: Σ_c dz_c = 0 over the candidates"""
    rng = np.random.default_rng(9)
    C = 13
    rows = (rng.standard_normal((3, C)) * 2).astype(np.float32)
    q = rng.random((3, C))
    q[:, UNK] = 0.0
    q = (q / q.sum(1, keepdims=True)).astype(np.float32)
    r = dr.seq_kd(rows, q, np.array([[BOS, 7, EOS]]), np.array([C]), np.array([0.0], f32), np.array([1.0], f32), True, False)
    keep = np.arange(C) != UNK
    assert np.abs(r["dscores"][:2, keep].sum(1)).max() < 1e-6 and np.abs(r["dscores"][:2]).max() > 1e-3


def test_unnormalised_teacher():
    """Q = 0.7: the teacher is taken as it is — the cross-entropy scales with it and the logits gradient is 0.7·p − q"""
    C = 9
    rows = np.linspace(-1, 1, C, dtype=np.float32)[None].repeat(3, 0)
    q1 = np.full((3, C), 1.0 / (C - 1), np.float32)
    q1[:, UNK] = 0.0
    ids, rc, w, v = np.array([[BOS, 7, EOS]]), np.array([C]), np.array([0.0], f32), np.array([1.0], f32)
    a = dr.seq_kd(rows, q1, ids, rc, w, v, True, False)
    b = dr.seq_kd(rows, (q1 * f32(0.7)).astype(np.float32), ids, rc, w, v, True, False)
    np.testing.assert_allclose(b["kdstep64"], 0.7 * a["kdstep64"], rtol=1e-6)
    t = dr.row_terms(rows[0], q1[0] * f32(0.7), C, True, False)
    assert t["q"].sum() == pytest.approx(0.7, rel=1e-6)
    np.testing.assert_allclose(b["dscores"][0], t["q"].sum() * t["p"] - t["q"], rtol=1e-12)
    assert abs(b["dscores"][0].sum()) < 1e-12                                    # Σ (Q·p − q) = Q − Q


@pytest.mark.parametrize("logits", [False, True])
def test_empty_teacher_rows(logits):
    C = 9
    rng = np.random.default_rng(2)
    rows = (rng.random((3, C)) + 0.1).astype(np.float32)
    ids, rc, w, v = np.array([[BOS, 7, EOS]]), np.array([C]), np.array([0.5], f32), np.array([1.0], f32)
    nll = dr.seq_kd(rows, np.zeros((3, C), f32), ids, rc, w, np.array([0.0], f32), logits, False)
    for tq, tl in ((np.zeros((3, C), f32), False), (np.full((3, C), -np.inf, f32), True), (np.full((3, C), -1.0, f32), False)):
        tq[:, UNK] = 5.0
        r = dr.seq_kd(rows, tq, ids, rc, w, v, logits, tl)
        assert not r["kdstep"].any() and not r["hstep"].any() and r["kd"][0] == 0 and r["ent"][0] == 0
        assert np.array_equal(r["dscores"], nll["dscores"]) and r["loss"] == nll["loss"]


def test_gibbs():
    """kd >= ent on normalised rows, with equality for student = teacher"""
    rng = np.random.default_rng(4)
    C, Lt, R = 40, 6, 5
    def norm(m):
        m[:, UNK] = 0.0
        m = m / m.sum(1, keepdims=True)
        return m.astype(np.float32)
    p, q = norm(rng.random((R * Lt, C)) + 1e-3), norm(rng.random((R * Lt, C)) ** 3)
    ids = np.tile(np.array([[BOS, 7, 8, 9, 10, EOS]]), (R, 1))
    w = np.zeros(R, f32)
    r = dr.seq_kd(p, q, ids, np.full(R, C), w, np.ones(R, f32), False, False)
    assert (r["kdstep64"] >= r["hstep64"] - 1e-6).all() and (r["kdstep64"] > r["hstep64"] + 1e-3).any()
    same = dr.seq_kd(q + f32(0), q, ids, np.full(R, C), w, np.ones(R, f32), False, False)
    live = same["hstep64"] > 0
    np.testing.assert_allclose(same["kdstep64"][live], same["hstep64"][live], rtol=1e-12)
    # logits on both sides, the same row: kd = ent
    z = (rng.standard_normal((R * Lt, C)) * 2).astype(np.float32)
    both = dr.seq_kd(z, z, ids, np.full(R, C), w, np.ones(R, f32), True, True)
    np.testing.assert_allclose(both["kdstep64"], both["hstep64"], rtol=1e-12)
    keep = np.arange(C) != UNK
    assert np.abs(both["dscores"][:, keep]).max() < 1e-12


# ------------------------------------------------------------------------------------------------ the margins of the GPU tests' inputs
@pytest.mark.parametrize("logits,teacher_logits", dc.FLAGS)
@pytest.mark.parametrize("C,Lt,R", dc.KERNEL_SHAPES)
def test_fixed_inputs_keep_clear_of_the_clamp(C, Lt, R, logits, teacher_logits):
    case = dc.kernel_case(C, Lt, R, logits, teacher_logits)
    assert case["scores"].shape == (R * Lt, C + dc.PAD_S) and case["tq"].shape == (R * Lt, C + dc.PAD_T)
    ref = dr.seq_kd(case["scores"], case["tq"], case["ids"], case["row_c"], case["w"], case["v"], logits, teacher_logits)
    ell = ref["ell"]
    assert not (np.abs(ell - dr.LOG_EPS) <= math.log(2.0)).any() and np.isfinite(ell).all()
    for (r, i, c), want in [(e, True) for e in case["clamped"]] + [(e, False) for e in case["unclamped"]]:
        if i >= ref["len"][r]:
            continue
        t = dr.row_terms(case["scores"][r * Lt + i], case["tq"][r * Lt + i], int(case["row_c"][r]), logits, teacher_logits)
        assert t["q"][c] > 0 and bool(t["clamped"][c]) == want, (r, i, c, t["q"][c], t["ell"][c])
        if want:                                                                  # a clamped ℓ keeps its distance from log ε too
            raw = float(case["scores"][r * Lt + i, c])
            assert raw <= 0 or t["ell"][c] < dr.LOG_EPS - math.log(2.0)
    for r, i in case["dead"]:
        if i < ref["len"][r]:
            assert ref["kdstep"][r, i] == 0 and ref["hstep"][r, i] == 0
    if R >= 5:
        assert [e for e in case["clamped"] if e[1] < ref["len"][e[0]]] and [e for e in case["unclamped"] if e[1] < ref["len"][e[0]]]
        assert [e for e in case["dead"] if e[1] < ref["len"][e[0]]]
        assert np.isfinite(ref["kdstep"]).all() and np.isfinite(ref["hstep"]).all() and np.isfinite(ref["loss"])
    if R >= 9:
        assert ref["barred"].any() and not ref["barred"].all()


# ------------------------------------------------------------------------------------------------ host checks, no CPU fallback, symbols
def test_value_errors():
    ops.check_distill(alpha=0.0)
    ops.check_distill(alpha=1)
    for alpha in (-0.5, 1.5, float("inf"), float("nan"), "1", True, [1]):
        with pytest.raises(ValueError):
            ops.check_distill(alpha=alpha)
    dev = torch.device("cpu")
    for bad in (torch.zeros(12, 10, dtype=torch.float64), torch.zeros(12, 10, dtype=torch.int32), torch.zeros(11, 10), torch.zeros(13, 10),
                torch.zeros(12, 9), torch.zeros(12), torch.zeros(12, 20)[:, ::2], torch.zeros(10, 12).t(), [[0.0]]):
        with pytest.raises(ValueError):
            ops.check_distill(tq=bad, tq_rows=12, max_cols=10, device=dev)
    with pytest.raises(ValueError):                                         # a teacher matrix on another device than the scores
        ops.check_distill(tq=torch.zeros(12, 10), tq_rows=12, max_cols=10, device=torch.device("cuda:0"))
    for kw in (dict(row_w=torch.zeros(3)), dict(row_v=torch.zeros(3)), dict(row_w=torch.zeros(2, dtype=torch.float64)),
               dict(row_v=torch.zeros(2, 1)), dict(row_v=[0.0, 0.0])):
        with pytest.raises(ValueError):
            ops.check_distill(rows=2, device=dev, **kw)
    for kw in (dict(weights=torch.zeros(4, 2)), dict(kd_weights=torch.zeros(11)), dict(kd_weights=torch.zeros(4, 3, dtype=torch.int32)),
               dict(weights=[0.0] * 12)):
        with pytest.raises(ValueError):
            ops.check_distill(shape=(4, 3), **kw)
    tgt, ln = torch.zeros(2, 6, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    w, sc = torch.zeros(2), torch.zeros(12, 10)
    for args in ((sc, [10, 11], tgt, ln, sc, w, w), (sc[:11], [10, 10], tgt, ln, sc[:11], w, w), (sc, [10], tgt, ln, sc, w, w),
                 (sc, [10, 10], tgt, ln, sc.double(), w, w), (sc, [10, 10], tgt, ln, sc[:11], w, w), (sc, [10, 10], tgt, ln, sc[:, :9], w, w),
                 (sc, [10, 10], tgt, ln, sc, w, w.double()), (sc, [10, 10], tgt, ln, sc, w[:1], w), (sc, [10, 10], tgt, ln, sc, w, torch.zeros(2, 1)),
                 (sc, [10, 10], tgt, ln.long(), sc, w, w), (sc, [10, 10], tgt.long(), ln, sc, w, w)):
        with pytest.raises(ValueError):
            ops.seq_kd(*args, False, False, UNK)
    with pytest.raises(ValueError):
        ops.seq_kd(sc, [10, 10], tgt, ln, sc, w, w, False, False, UNK, max_cols=9)
    with pytest.raises(ValueError):
        ops.seq_kd(sc, [10, 10], tgt, ln, torch.zeros(12, 9), w, w, False, False, UNK, max_cols=10)   # tq narrower than max_cols


def _cfg(**over):
    base = dict(model_mode="vivt", vocab_size=100, max_t_len=22, max_v_len=12, max_i_len=30, video_feature_size=64, hidden_size=32,
                num_hidden_layers=2, num_attention_heads=4, word_vec_size=16)
    base.update(over)
    return SimpleNamespace(**base)


def _bare_translator(cfg=None, device="cpu"):
    from svpc_amd.translator import Translator
    tr = object.__new__(Translator)                                            # (the checks come before any use of the model)
    cfg = cfg or _cfg()
    tr.max_t_len = cfg.max_t_len
    tr.opt = SimpleNamespace()
    par = torch.zeros(1, device=device)
    tr.model = SimpleNamespace(config=cfg, parameters=lambda: iter([par]), training=False)
    return tr


def test_module_checks_on_the_host():
    from svpc_amd import distill as ds
    tr, te = _bare_translator(), _bare_translator(_cfg(hidden_size=64, num_hidden_layers=4, num_attention_heads=8, word_vec_size=32))
    ds.Distill(tr, te)                                                         # a smaller student is the point
    ds.Distill(tr, tr)                                                         # the teacher may be the student's own translator
    for f, val in (("model_mode", "video"), ("vocab_size", 101), ("max_t_len", 20), ("max_v_len", 13), ("max_i_len", 31),
                   ("video_feature_size", 128)):
        with pytest.raises(ValueError, match=f):
            ds.Distill(tr, _bare_translator(_cfg(**{f: val})))
        with pytest.raises(ValueError, match=f):
            ds.distillation_loss(tr, _bare_translator(_cfg(**{f: val})), [None] * 11 + [[2, 1]], [], torch.zeros(1), torch.zeros(1))
    with pytest.raises(ValueError, match="device"):
        ds.Distill(tr, _bare_translator(device="meta"))
    inputs = [None] * 11 + [[2, 1]]
    dec = [torch.zeros(2, 3, 22, dtype=torch.int64), torch.zeros(1, 3, 22, dtype=torch.int64)]
    w = torch.zeros(3, 3)
    with pytest.raises(ValueError, match="step counts"):
        ds.distillation_loss(tr, te, [None] * 11 + [[1, 2]], dec, w, w)
    for a, b in ((torch.zeros(3, 2), w), (w, torch.zeros(8)), (w, [0.0] * 9), (w, torch.zeros(3, 3, dtype=torch.int32)), (None, w)):
        with pytest.raises(ValueError):
            ds.distillation_loss(tr, te, inputs, dec, a, b)
    with pytest.raises(ValueError):                                            # captions of another length than the model's
        ds.distillation_loss(tr, te, inputs, [d[:, :, :20] for d in dec], w, w)
    with pytest.raises(_lib.SvpcKernelError):                                  # CPU ids: no fallback
        ds.distillation_loss(tr, te, inputs, dec, w, w)
    step = ds.Distill(tr, te)
    for kw in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(source="sample"), dict(source=None)):
        with pytest.raises(ValueError):
            step.sequence_step(inputs, **kw)
    with pytest.raises(TypeError):
        step.sequence_step(inputs, beam=4)                                     # an unknown keyword
    with pytest.raises(TypeError):
        step.sequence_step(inputs, source="greedy", beam_size=4)               # greedy takes no decoding keyword
    with pytest.raises(TypeError):
        step.sequence_step(inputs, random_sampling_temp=2.0)
    for alpha in (-1.0, 2.0, float("inf")):
        with pytest.raises(ValueError):
            step.word_step(inputs, [], alpha=alpha)


def test_no_cpu_fallback():
    tgt, ln = torch.zeros(2, 6, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    w, sc = torch.zeros(2), torch.zeros(12, 10)
    with pytest.raises(_lib.SvpcKernelError):
        ops.seq_kd(sc, [10, 10], tgt, ln, sc, w, w, False, False, UNK)
    with pytest.raises(_lib.SvpcKernelError):
        ops.check_distill(tq=sc, tq_rows=12, max_cols=10)
    with pytest.raises(_lib.SvpcKernelError):
        ops.check_distill(shape=(2, 1), kd_weights=torch.zeros(2))
    from svpc_amd.translator import Translator
    tr = _bare_translator()
    with pytest.raises(_lib.SvpcKernelError):
        Translator.teacher_scores(tr, [None] * 11 + [[1]], [torch.zeros(1, 22, dtype=torch.int64)])
    with pytest.raises(ValueError, match="step counts"):
        Translator.teacher_scores(tr, [None] * 11 + [[2]], [torch.zeros(1, 22, dtype=torch.int64)])


def test_symbols_declared_and_exported():
    decls = _lib.declarations()
    lib = _lib.load()
    for name, n_args in (("svpc_seq_kd_fwd", 24), ("svpc_seq_kd_bwd", 20)):
        assert name in decls and len(decls[name][1]) == n_args and hasattr(lib, name), name
    assert lib.svpc_abi_version() == 2
    from svpc_amd import distill as ds
    from svpc_amd.ensemble import EnsembleTranslator
    from svpc_amd.translator import Translator
    assert callable(ds.distillation_loss) and hasattr(ds.Distill, "word_step") and hasattr(ds.Distill, "sequence_step")
    assert callable(Translator.teacher_scores) and EnsembleTranslator.teacher_scores is Translator.teacher_scores
    for fn in ("check_distill", "seq_kd"):
        assert callable(getattr(ops, fn))
