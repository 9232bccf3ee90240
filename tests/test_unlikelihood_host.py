"""Unlikelihood training without a GPU: the restatement (tests/unlikelihood_reference.py) on literal anchors, the clamp, a
logits row against torch autograd, the negative rules on hand-built videos, the repeat-gram identity against ``DecodeMetrics``' counts,
every host check, no CPU fallback, the exported symbols, and the margins of the fixed inputs the GPU tests run on."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import caption_metrics_reference as cm  # noqa: E402
import unlikelihood_cases as uc  # noqa: E402
import unlikelihood_reference as ur  # noqa: E402
from svpc_amd import _lib, ops  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, IGNORE, PAD, UNK  # noqa: E402

f32 = np.float32


# ------------------------------------------------------------------------------------------------ the restatement alone
def _anchor_rows():
    """C = 8, caption BOS 7 7 EOS: p0(7) = 0.5, p1(7) = 0.25, p2(EOS) = 0.25, p2(7) = 0.5"""
    assert (BOS, EOS, UNK, PAD) == (4, 5, 6, 0)
    rows = np.full((4, 8), 0.03125, np.float32)
    rows[0, 7], rows[1, 7], rows[2, EOS], rows[2, 7] = 0.5, 0.25, 0.25, 0.5
    return rows, np.array([[BOS, 7, 7, EOS]]), np.array([8])


def test_anchor_token_rule():
    rows, ids, rc = _anchor_rows()
    neg, npen, nrep = ur.negatives(ids, rc, "token")
    assert neg.shape == (1, 3, 3) and neg[0, 2].tolist() == [7, -1, -1] and (neg[0, :2] == -1).all()      # only N(r, 2) = {7}
    assert npen.tolist() == [1] and nrep.tolist() == [0]
    r = ur.seq_ul(rows, ids, rc, neg, np.array([0.0], f32), np.array([0.5], f32), logits=False)
    assert r["loss"].dtype == np.float32 and r["loss"] == f32(0.5 * float(f32(math.log(2.0))))
    assert r["ulstep"].tolist() == [[0.0, 0.0, f32(math.log(2.0))]] and r["ul"][0] == f32(math.log(2.0))
    d = r["dscores"]
    assert d[2, 7] == 1.0
    d[2, 7] = 0.0
    assert not d.any()


def test_anchor_ngram_rule():
    rows, ids, rc = _anchor_rows()
    neg, npen, nrep = ur.negatives(ids, rc, "ngram", ngram=1)
    assert neg.shape == (1, 3, 1) and neg[0, :, 0].tolist() == [-1, 7, -1]                                  # only position 2 is penalised
    assert npen.tolist() == [1] and nrep.tolist() == [1]
    r = ur.seq_ul(rows, ids, rc, neg, np.array([0.0], f32), np.array([0.5], f32), logits=False)
    assert r["ulstep"][0, 1] == f32(math.log(4.0 / 3.0)) and r["ulstep"][0, 0] == 0 and r["ulstep"][0, 2] == 0
    d = r["dscores"]
    assert d[1, 7] == 0.5 / 0.75
    d[1, 7] = 0.0
    assert not d.any()
    # with a likelihood weight the two terms meet on the target column
    r = ur.seq_ul(rows, ids, rc, neg, np.array([0.25], f32), np.array([0.5], f32), logits=False)
    assert r["dscores"][1, 7] == -0.25 / 0.25 + 0.5 / 0.75 and r["dscores"][0, 7] == -0.25 / 0.5


def test_clamp():
    """p = 1: the term is −log ε and the gradient zero; 1 − p just under ε likewise; just over it: log1p and 1 / (1 − p)"""
    assert ur.EPS == 1e-5 == ops.UL_EPS == uc.EPS
    rows, ids, rc = _anchor_rows()
    neg = np.full((1, 3, 2), -1, np.int32)
    neg[0, 0] = [1, 2]
    neg[0, 1] = [3, 3]
    rows[0, 1], rows[0, 2] = 1.0, 1.0 - 2.0 ** -20
    rows[1, 3] = 1.0 - 2.0 ** -10
    r = ur.seq_ul(rows, ids, rc, neg, np.array([0.0], f32), np.array([2.0], f32), logits=False)
    assert r["ulstep64"][0, 0] == 2.0 * -math.log(1e-5) and not r["dscores"][0].any()
    assert r["ulstep64"][0, 1] == pytest.approx(2.0 * 10.0 * math.log(2.0), rel=1e-12)                     # listed twice: counted twice
    assert r["dscores"][1, 3] == 2.0 * 2.0 * 1024.0
    for logits in (False, True):                                            # a barred caption: no loss, no gradient, whatever it lists
        ids_b = np.array([[BOS, 7, UNK, EOS]])
        r = ur.seq_ul(rows, ids_b, rc, neg, np.array([1.0], f32), np.array([2.0], f32), logits=logits)
        assert r["barred"].tolist() == [1] and r["loss"] == 0 and not r["dscores"].any()


def test_logits_row_against_autograd():
    rng = np.random.default_rng(3)
    C, Lt = 11, 4
    rows = (rng.standard_normal((Lt, C)) * 2).astype(np.float32)
    rows[:, UNK] = 30.0
    ids = np.array([[BOS, 7, 8, EOS]])
    neg = np.array([[[1, 2, 2, UNK], [7, 9, -1, C], [8, 7, 3, 3]]], np.int32)       # twice, UNK, none, from C up; the target EOS is not listed
    w, u, dl = np.array([0.75], f32), np.array([-1.25], f32), 2.5
    r = ur.seq_ul(rows, ids, np.array([C]), neg, w, u, logits=True, dl=dl)
    z = torch.tensor(rows.astype(np.float64), requires_grad=True)
    keep = torch.arange(C) != UNK
    loss = torch.zeros((), dtype=torch.float64)
    for i in range(3):
        lp = z[i] - torch.logsumexp(z[i][keep], 0)
        loss = loss - float(w[0]) * lp[int(ids[0, i + 1])]
        for c in neg[0, i]:
            if 0 <= c < C and c != UNK:
                loss = loss - float(u[0]) * torch.log1p(-torch.exp(lp[int(c)]))
    (loss * dl).backward()
    g = r["dscores"]
    np.testing.assert_allclose(g, z.grad.numpy(), rtol=1e-10, atol=1e-12)
    assert np.abs(g[:3, keep.numpy()].sum(1)).max() < 1e-12 and not g[:, UNK].any() and not g[3].any()
    assert abs(float(r["loss"]) - float(loss.detach())) <= 2.0 ** -22 * abs(float(loss.detach()))
    # the running sums are float32, position by position
    acc = f32(0)
    for i in range(3):
        acc = f32(acc + r["ulstep"][0, i])
    assert r["ul"][0] == acc and r["ulstep"].dtype == np.float32


# ------------------------------------------------------------------------------------------------ the negative rules
def _video():
    """three sentences, K = 1: A = 7 8 9 7 8 (a bigram that repeats inside the caption), B = 8 9 1 (a bigram of A, and 9 1 that comes
    again in C), C = 9 1 7 8 EOS; Lt = 7"""
    return np.array([[BOS, 7, 8, 9, 7, 8, EOS],
                     [BOS, 8, 9, 1, EOS, PAD, PAD],
                     [BOS, 9, 1, 7, 8, EOS, PAD]])


def test_paragraph_scope_against_caption_scope():
    ids, rc = _video(), np.array([12, 12, 12])
    neg, npen, nrep = ur.negatives(ids, rc, "ngram", ngram=2, scope="caption")
    assert nrep.tolist() == [1, 0, 0] and npen.tolist() == [2, 0, 0]
    assert neg[0, :, 0].tolist() == [-1, -1, -1, 7, 8, -1] and (neg[1:] == -1).all()
    neg, npen, nrep = ur.negatives(ids, rc, "ngram", ngram=2, scope="paragraph", sent_first=[0, 0, 0], K=1)
    assert nrep.tolist() == [1, 1, 2]                                       # B: 8 9 (of A); C: 9 1 (of B) and 7 8 (of A); 1 7 is new
    assert neg[1, :, 0].tolist() == [8, 9, -1, -1, -1, -1] and neg[2, :, 0].tolist() == [9, 1, 7, 8, -1, -1]
    assert npen.tolist() == [2, 2, 4]
    # the second video starts at sentence 1: its sentences do not see sentence 0
    _, _, nrep2 = ur.negatives(ids, rc, "ngram", ngram=2, scope="paragraph", sent_first=[0, 1, 1], K=1)
    assert nrep2.tolist() == [1, 0, 1]


def test_a_gram_of_a_later_sentence_is_no_repeat():
    ids, rc = _video(), np.array([12, 12, 12])
    _, _, nrep = ur.negatives(ids, rc, "ngram", ngram=2, scope="paragraph", sent_first=[0, 0, 0], K=1)
    assert nrep[1] == 1                                                     # 9 1 also stands in the later C: B's copy is the first
    _, _, first = ur.negatives(ids[::-1].copy(), rc, "ngram", ngram=2, scope="paragraph", sent_first=[0, 0, 0], K=1)
    assert first.tolist() == [0, 1, 3]                                      # C first: nothing; B: 9 1; A: 7 8 (C's), 8 9 (B's), 7 8 again


def test_no_gram_spans_two_captions():
    # A ends with 7 8, B starts with 9: "8 9" across the boundary is no gram, so B's own "8 9" further on is its first occurrence
    ids = np.array([[BOS, 1, 7, 8, EOS, PAD], [BOS, 9, 2, 8, 9, EOS]])
    _, _, nrep = ur.negatives(ids, np.array([12, 12]), "ngram", ngram=2, scope="paragraph", sent_first=[0, 0], K=1)
    assert nrep.tolist() == [0, 0]
    # EOS is no word: "8 EOS" is no gram
    ids = np.array([[BOS, 8, EOS, PAD, PAD, PAD], [BOS, 2, 8, EOS, PAD, PAD]])
    _, _, nrep = ur.negatives(ids, np.array([12, 12]), "ngram", ngram=2, scope="paragraph", sent_first=[0, 0], K=1)
    assert nrep.tolist() == [0, 0]
    # K = 2: candidate row k looks at row k of the earlier sentences only
    ids = np.array([[BOS, 7, 8, EOS], [BOS, 1, 2, EOS], [BOS, 1, 2, EOS], [BOS, 1, 2, EOS]])
    _, _, nrep = ur.negatives(ids, np.full(4, 12), "ngram", ngram=2, scope="paragraph", sent_first=[0, 0], K=2)
    assert nrep.tolist() == [0, 0, 0, 1]


@pytest.mark.parametrize("Lt,K,steps", uc.NEGATIVE_SHAPES)
def test_repeat_grams_are_the_metrics_repeats(Lt, K, steps):
    """Σ nrep over a paragraph under paragraph scope = total_n − distinct_n of ``video_counts`` on the ``remove_dup=False`` clean captions,
    for rows whose only PAD / IGNORE lie after the end (every row the cases build)"""
    ids, rc, sf = uc.negatives_case(Lt, K, steps)
    checked = 0
    for n in (1, 2, 3, 4):
        _, _, nrep = ur.negatives(ids, rc, "ngram", ngram=n, scope="paragraph", sent_first=sf, K=K)
        o = 0
        for s in steps:
            for k in range(K):
                rows = [ids[(o + t) * K + k].tolist() for t in range(s)]
                counts = cm.video_counts([cm.clean_caption(r, remove_dup=False) for r in rows], 12)
                assert int(sum(nrep[(o + t) * K + k] for t in range(s))) == counts[n - 1] - counts[4 + n - 1], (n, o, k)
                checked += counts[n - 1] - counts[4 + n - 1]
            o += s
    assert checked > 0 or Lt == 2


def test_token_rule_by_hand():
    ids = np.array([[BOS, 7, 8, 7, UNK, 11, 8, EOS, PAD]])
    neg, npen, nrep = ur.negatives(ids, np.array([11]), "token")           # column 11 is from C_r up
    assert neg.shape == (1, 8, 8) and nrep.tolist() == [0]
    want = [[], [7], [8], [7, 8], [7, 8], [7], [7, 8]]                       # first occurrence order; the target, UNK and 11 left out
    for i, lst in enumerate(want):
        assert neg[0, i].tolist() == lst + [-1] * (8 - len(lst)), i
    assert (neg[0, 7] == -1).all() and npen.tolist() == [sum(len(x) for x in want)]


# ------------------------------------------------------------------------------------------------ the margins of the GPU tests' inputs
@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("C,Lt,T,K", uc.KERNEL_SHAPES)
def test_fixed_inputs_keep_clear_of_the_clamp(C, Lt, T, K, logits):
    case = uc.kernel_case(C, Lt, T * K, logits)
    assert case["neg"].shape == (T * K, Lt - 1, case["M"]) and 1 <= case["M"] <= 64
    ref = ur.seq_ul(case["scores"], case["ids"], case["row_c"], case["neg"], case["w"], case["u"], logits)
    q = ref["q"]
    assert not ((q >= 0.5 * ur.EPS) & (q <= 2.0 * ur.EPS)).any(), q[(q >= 0.5 * ur.EPS) & (q <= 2.0 * ur.EPS)]
    n_scored = int(ref["len"].sum())
    assert len(q) > 0 or n_scored == 0
    for r, i, c in case["clamped"] + case["near"]:
        if i >= ref["len"][r]:
            continue
        t = [x for x in ur.row_terms(case["scores"][r * Lt + i], [c], int(case["row_c"][r]), logits)]
        assert len(t) == 1 and t[0][3] == ((r, i, c) in case["clamped"]), (r, i, c, t)
    if T * K >= 9:
        scored = [(r, i, c) for r, i, c in case["clamped"] if i < ref["len"][r]]
        assert scored and (logits or [x for x in case["near"] if x[1] < ref["len"][x[0]]])
        assert ref["barred"].any() and not ref["barred"].all()


# ------------------------------------------------------------------------------------------------ host checks, no CPU fallback, symbols
def test_value_errors():
    assert ops.check_unlikelihood("token") == (0, 4, False) and ops.check_unlikelihood("ngram", 1, "paragraph", alpha=0.0) == (1, 1, True)
    for rule in ("word", None, 0):
        with pytest.raises(ValueError):
            ops.check_unlikelihood(rule)
    for n in (0, 5, -1, 2.0, True, "4"):
        with pytest.raises(ValueError):
            ops.check_unlikelihood("ngram", n)
    for scope in ("video", None, 1):
        with pytest.raises(ValueError):
            ops.check_unlikelihood("ngram", 4, scope)
    for alpha in (-0.5, float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError):
            ops.check_unlikelihood("token", alpha=alpha)
    with pytest.raises(ValueError):
        ops.check_unlikelihood(lt=66)                                       # Lt − 1 > 64
    assert ops.check_unlikelihood(lt=65, m=64)
    for m in (0, 65):
        with pytest.raises(ValueError):
            ops.check_unlikelihood(lt=6, m=m)
    dev = torch.device("cpu")
    for bad in (torch.zeros(2, 5, 3, dtype=torch.int64), torch.zeros(2, 5, dtype=torch.int32), torch.zeros(3, 5, 3, dtype=torch.int32),
                torch.zeros(2, 4, 3, dtype=torch.int32), torch.zeros(2, 5, 65, dtype=torch.int32), torch.zeros(2, 5, 0, dtype=torch.int32),
                torch.zeros(2, 5, 6, dtype=torch.int32)[:, :, ::2], [[[0]]]):
        with pytest.raises(ValueError):
            ops.check_unlikelihood(lt=6, neg=bad, rows=2, device=dev)
    with pytest.raises(ValueError):                                         # a table on another device than the scores
        ops.check_unlikelihood(lt=6, neg=torch.zeros(2, 5, 3, dtype=torch.int32), rows=2, device=torch.device("cuda:0"))
    for kw in (dict(row_w=torch.zeros(3)), dict(row_u=torch.zeros(3)), dict(row_w=torch.zeros(2, dtype=torch.float64)),
               dict(row_u=torch.zeros(2, 1)), dict(row_u=[0.0, 0.0])):
        with pytest.raises(ValueError):
            ops.check_unlikelihood(rows=2, device=dev, **kw)
    for kw in (dict(weights=torch.zeros(4, 2)), dict(ul_weights=torch.zeros(11)), dict(ul_weights=torch.zeros(4, 3, dtype=torch.int32)),
               dict(weights=[0.0] * 12)):
        with pytest.raises(ValueError):
            ops.check_unlikelihood(shape=(4, 3), **kw)
    tgt, ln = torch.zeros(2, 6, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    w, neg = torch.zeros(2), torch.zeros(2, 5, 5, dtype=torch.int32)
    sc = torch.zeros(12, 10)
    for args in ((sc, [10, 11], tgt, ln, neg, w, w), (sc[:11], [10, 10], tgt, ln, neg, w, w), (sc, [10], tgt, ln, neg, w, w),
                 (sc, [10, 10], tgt, ln, neg[:, :4], w, w), (sc, [10, 10], tgt, ln, neg, w, w.double()),
                 (sc, [10, 10], tgt, ln.long(), neg, w, w), (sc, [10, 10], tgt.long(), ln, neg, w, w)):
        with pytest.raises(ValueError):
            ops.seq_ul(*args, False, UNK)
    with pytest.raises(ValueError):
        ops.seq_ul(sc, [10, 10], tgt, ln, neg, w, w, False, UNK, max_cols=9)
    fin = torch.zeros(2, dtype=torch.int32)
    for kw in (dict(rule="word"), dict(rule="ngram", ngram=5), dict(rule="ngram", scope="video"),
               dict(rule="ngram", scope="paragraph"),                                                   # no sent_first
               dict(rule="ngram", scope="paragraph", sent_first=[0, 2], K=1),                           # a first sentence after its sentence
               dict(rule="ngram", scope="paragraph", sent_first=[0, 0], K=3),                           # K does not divide the rows
               dict(rule="ngram", scope="paragraph", sent_first=[0], K=1)):
        with pytest.raises(ValueError):
            ops.ul_negatives(tgt, ln, fin, [10, 10], UNK, EOS, **kw)
    with pytest.raises(ValueError):
        ops.ul_negatives(torch.zeros(2, 67, dtype=torch.int32), ln, fin, [10, 10], UNK, EOS, "token")    # Lt − 1 > 64
    with pytest.raises(ValueError):
        ops.ul_negatives(tgt, ln, fin, [10], UNK, EOS, "token")
    with pytest.raises(ValueError):
        ops.ul_negatives(tgt, ln, fin.long(), [10, 10], UNK, EOS, "token")


def _bare_translator():
    from svpc_amd.translator import Translator
    tr = object.__new__(Translator)                                            # (the checks come before any use of the model)
    tr.max_t_len = 22
    return tr


def test_module_checks_on_the_host():
    from svpc_amd import unlikelihood as ul
    tr = _bare_translator()
    inputs = [None] * 11 + [[2, 1]]
    dec = [torch.zeros(2, 3, 22, dtype=torch.int64), torch.zeros(1, 3, 22, dtype=torch.int64)]
    w = torch.zeros(3, 3)
    for kw in (dict(rule="word"), dict(rule="ngram", ngram=0), dict(rule="ngram", scope="video")):
        with pytest.raises(ValueError):
            ul.unlikelihood_loss(tr, inputs, dec, w, w, **kw)
    with pytest.raises(ValueError, match="step counts"):
        ul.unlikelihood_loss(tr, [None] * 11 + [[1, 2]], dec, w, w)
    with pytest.raises(ValueError):
        ul.unlikelihood_loss(tr, inputs, dec, torch.zeros(3, 2), w)
    with pytest.raises(ValueError):
        ul.unlikelihood_loss(tr, inputs, dec, w, [0.0] * 9)
    with pytest.raises(ValueError):
        ul.unlikelihood_loss(tr, inputs, dec, w, torch.zeros(3, 3, dtype=torch.int32))
    with pytest.raises(_lib.SvpcKernelError):                                  # CPU ids: no fallback
        ul.unlikelihood_loss(tr, inputs, dec, w, w)
    step = ul.Unlikelihood(tr)
    for kw in (dict(alpha=-1.0), dict(alpha=float("nan")), dict(ngram=5), dict(scope="video"), dict(source="beam")):
        with pytest.raises(ValueError):
            step.sequence_step(inputs, **kw)
    with pytest.raises(TypeError):
        step.sequence_step(inputs, source="sample", random_sampling_temperature=2.0)      # an unknown keyword
    with pytest.raises(TypeError):
        step.sequence_step(inputs, beam_size=4)
    for alpha in (-1.0, float("inf")):
        with pytest.raises(ValueError):
            step.token_step(inputs, [], alpha=alpha)


def test_no_cpu_fallback():
    tgt, ln, fin = torch.zeros(2, 6, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    w, neg = torch.zeros(2), torch.zeros(2, 5, 5, dtype=torch.int32)
    with pytest.raises(_lib.SvpcKernelError):
        ops.seq_ul(torch.zeros(12, 10), [10, 10], tgt, ln, neg, w, w, False, UNK)
    with pytest.raises(_lib.SvpcKernelError):
        ops.ul_negatives(tgt, ln, fin, [10, 10], UNK, EOS, "token")
    with pytest.raises(_lib.SvpcKernelError):
        ops.ul_negatives(tgt, ln, fin, [10, 10], UNK, EOS, "ngram", 2, "paragraph", sent_first=[0, 0], K=1)
    with pytest.raises(_lib.SvpcKernelError):
        ops.check_unlikelihood(lt=6, neg=neg, rows=2)
    with pytest.raises(_lib.SvpcKernelError):
        ops.check_unlikelihood(shape=(2, 1), ul_weights=torch.zeros(2))


def test_symbols_declared_and_exported():
    decls = _lib.declarations()
    lib = _lib.load()
    for name, n_args in (("svpc_ul_negatives", 16), ("svpc_seq_ul_fwd", 21), ("svpc_seq_ul_bwd", 19)):
        assert name in decls and len(decls[name][1]) == n_args and hasattr(lib, name), name
    assert lib.svpc_abi_version() == 2
    from svpc_amd import scst, unlikelihood as ul
    assert callable(ul.unlikelihood_loss) and hasattr(ul.Unlikelihood, "token_step") and hasattr(ul.Unlikelihood, "sequence_step")
    assert callable(scst.graded_pass) and callable(scst.sequence_loss)
    for fn in ("check_unlikelihood", "ul_negatives", "seq_ul"):
        assert callable(getattr(ops, fn))
