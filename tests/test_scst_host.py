"""The self-critical step without a GPU: the restatement (tests/scst_reference.py) on hand-built rows, the literal anchor, every host
check, no CPU fallback, the exported symbols."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import scst_reference as sr  # noqa: E402
from svpc_amd import _lib, ops  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, PAD, UNK  # noqa: E402

f32 = np.float32


def test_baselines():
    r = np.array([[0.5, 1.5, 1.0], [2.0, 2.0, 2.0]])
    assert np.array_equal(sr.advantages(r, "none"), r)
    assert np.array_equal(sr.advantages(r, "greedy", [1.0, 2.5]), [[-0.5, 0.5, 0.0], [-0.5, -0.5, -0.5]])      # a negative advantage
    A = sr.advantages(r, "mean")
    assert np.array_equal(A[0], [0.5 - 1.25, 1.5 - 0.75, 1.0 - 1.0]) and np.array_equal(A[1], [0.0, 0.0, 0.0])   # an all-zero advantage
    A2 = sr.advantages(np.array([[0.25, 1.0]]), "mean")                                                        # K = 2: the other sample
    assert np.array_equal(A2, [[-0.75, 0.75]])
    with pytest.raises(ValueError):
        sr.advantages(np.array([[0.25]]), "mean")                                                              # K = 1
    assert np.array_equal(sr.advantages(np.array([[0.25]]), "greedy", [0.75]), [[-0.5]])
    with pytest.raises(ValueError):
        sr.advantages(r, "median")


def test_row_weights_follow_the_rows():
    A = np.array([[1.0, -2.0], [0.5, 0.0], [3.0, 3.0]])
    w = sr.row_weights(A, [2, 0, 1])                                           # rows t·K + k; the video without sentences owns none
    assert w.dtype == np.float32 and w.tolist() == [f32(1 / 6), f32(-2 / 6), f32(1 / 6), f32(-2 / 6), f32(3 / 6), f32(3 / 6)]
    assert sr.row_weights(np.zeros((2, 3)), [1, 1]).tolist() == [0.0] * 6


def test_anchor_literal():
    """C = 8, p(7) = 0.5, p(EOS = 5) = 0.25: caption BOS 7 EOS, w = 0.5"""
    assert (BOS, EOS, UNK, PAD) == (4, 5, 6, 0)
    rows = np.array([[0.03125, 0.03125, 0.03125, 0.03125, 0.0625, 0.25, 0.0625, 0.5]] * 3, np.float32)
    r = sr.seq_nll(rows, [[BOS, 7, EOS]], [8], np.array([0.5], np.float32), logits=False)
    assert r["loss"].dtype == np.float32 and r["loss"] == f32(-0.5 * float(f32(f32(math.log(0.5)) + f32(math.log(0.25)))))
    assert r["barred"].tolist() == [0] and r["len"].tolist() == [2]
    d = r["dscores"]
    assert d[0, 7] == -1.0 and d[1, EOS] == -2.0
    d[0, 7] = d[1, EOS] = 0.0
    assert not d.any()


def test_barred_rows_add_nothing_and_never_make_nan():
    C, Lt = 10, 5
    rows = np.full((3 * Lt, C), 0.1, np.float32)
    rows[Lt + 1, 8] = 0.0                                                      # p(target) = 0 in the second caption
    ids = [[BOS, 7, 8, EOS, PAD], [BOS, 7, 8, EOS, PAD], [BOS, UNK, 8, EOS, PAD]]       # the third: a target that is no candidate
    w = np.array([0.25, 0.0, -1.0], np.float32)                                # (0 · −inf and w / 0 would both be NaN)
    r = sr.seq_nll(rows, ids, [C] * 3, w, logits=False)
    assert r["barred"].tolist() == [0, 1, 1]
    assert np.isfinite(r["loss"]) and r["loss"] == f32(-0.25 * float(r["cum"][0]))
    assert np.isfinite(r["dscores"]).all() and not r["dscores"][Lt:].any()
    assert r["dscores"][0, 7] == -0.25 / float(f32(0.1)) and not r["dscores"][3:Lt].any()      # rows past the end and the last row: 0
    for logits in (False, True):                                               # a negative and a zero weight
        r = sr.seq_nll(np.full((2 * Lt, C), 0.1, np.float32), ids[:1] * 2, [C] * 2, np.array([-0.5, 0.0], np.float32), logits=logits)
        assert r["barred"].tolist() == [0, 0] and r["loss"] == f32(0.5 * float(r["cum"][0])) and not r["dscores"][Lt:].any()
        if logits:                                                             # softmax without UNK − one-hot: rows sum to 0, UNK is 0
            g = r["dscores"][:3]
            assert np.abs(g.sum(1)).max() < 1e-12 and not g[:, UNK].any() and (g[0, 7] > 0)


def test_value_errors():
    ok = torch.zeros(4, 3, 22, dtype=torch.int64)
    for k in (0, 17, -1, 2.0, True, "4"):
        with pytest.raises(ValueError):
            ops.check_scst(num_samples=k)
    with pytest.raises(ValueError):
        ops.check_scst(num_samples=1, baseline="mean")
    assert ops.check_scst(num_samples=2, baseline="mean") == (2, 5, 2)
    assert ops.check_scst(num_samples=16, baseline="greedy", utility="Bleu_4") == (1, 3, 16)
    for kw in (dict(baseline="median"), dict(baseline=None), dict(utility="METEOR"), dict(utility=5)):
        with pytest.raises(ValueError):
            ops.check_scst(num_samples=4, **kw)
    for bad in (torch.zeros(4, 17, 22, dtype=torch.int64), torch.zeros(4, 0, 22, dtype=torch.int64),        # K outside 1 … 16
                torch.zeros(4, 3, 22, dtype=torch.float32), torch.zeros(4, 3, 22, dtype=torch.int16),        # dtype
                torch.zeros(4, 22, dtype=torch.int64), torch.zeros(2, 2, 3, 22, dtype=torch.int64),          # shape
                torch.zeros(4, 3, 1, dtype=torch.int64), [[[0] * 22]]):
        with pytest.raises(ValueError):
            ops.check_scst(bad)
    with pytest.raises(ValueError):
        ops.check_scst(ok, lt=21)
    with pytest.raises(ValueError, match="do not add up"):
        ops.check_scst(ok, lt=22, steps=[2, 1])                               # steps mismatch
    with pytest.raises(ValueError):
        ops.check_scst(ok, num_samples=4)                                      # K of the ids is not num_samples
    with pytest.raises(ValueError):
        ops.check_scst(torch.zeros(4, 1, 22, dtype=torch.int64), baseline="mean")
    for bad_w in (torch.zeros(4, 2), torch.zeros(11), torch.zeros(4, 3, dtype=torch.int32), [0.0] * 12):   # weights of the wrong shape
        with pytest.raises(ValueError):
            ops.check_scst(ok, weights=bad_w)
    with pytest.raises(ValueError):                                            # rewards: float64 (N, K)
        ops.scst_weights(torch.zeros(2, 3), [0, 1], "none")
    with pytest.raises(ValueError):                                            # the greedy baseline needs its rewards
        ops.scst_weights(torch.zeros(2, 3, dtype=torch.float64), [0, 1], "greedy")
    with pytest.raises(ValueError):
        ops.scst_weights(torch.zeros(2, 3, dtype=torch.float64), [0, 1], "greedy", torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.scst_weights(torch.zeros(2, 1, dtype=torch.float64), [0, 1], "mean")
    with pytest.raises(ValueError):                                            # a sentence of a video that is not there
        ops.scst_weights(torch.zeros(2, 3, dtype=torch.float64), [0, 2], "none")
    tgt, ln, w = torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2)
    with pytest.raises(ValueError):                                            # rows wider than the score matrix
        ops.seq_nll(torch.zeros(8, 10), [10, 11], tgt, ln, w, False, UNK)
    with pytest.raises(ValueError):                                            # … also when the caller names a smaller max_cols
        ops.seq_nll(torch.zeros(8, 10), [10, 11], tgt, ln, w, False, UNK, max_cols=10)
    with pytest.raises(ValueError):                                            # fewer score rows than R·Lt
        ops.seq_nll(torch.zeros(7, 10), [10, 10], tgt, ln, w, False, UNK)
    with pytest.raises(ValueError):                                            # one weight per caption row
        ops.seq_nll(torch.zeros(8, 10), [10, 10], tgt, ln, torch.zeros(3), False, UNK)
    with pytest.raises(ValueError):
        ops.seq_nll(torch.zeros(8, 10), [10, 10], tgt, ln, w.double(), False, UNK)
    with pytest.raises(ValueError):
        ops.seq_nll(torch.zeros(8, 10), [10], tgt, ln, w, False, UNK)


def test_sequence_loss_checks_on_the_host():
    from svpc_amd import scst
    from svpc_amd.translator import Translator
    tr = object.__new__(Translator)                                            # (the checks come before any use of the model)
    tr.max_t_len = 22
    inputs = [None] * 11 + [[2, 1]]
    dec = [torch.zeros(2, 3, 22, dtype=torch.int64), torch.zeros(1, 3, 22, dtype=torch.int64)]
    w = torch.zeros(3, 3)
    with pytest.raises(ValueError, match="step counts"):
        scst.sequence_loss(tr, [None] * 11 + [[1, 2]], dec, w)
    with pytest.raises(ValueError):
        scst.sequence_loss(tr, inputs, [d[:, :, :21] for d in dec], w)
    with pytest.raises(ValueError):
        scst.sequence_loss(tr, inputs, [d.repeat(1, 6, 1) for d in dec], torch.zeros(3, 18))       # K = 18
    with pytest.raises(ValueError):
        scst.sequence_loss(tr, inputs, dec, torch.zeros(3, 2))
    with pytest.raises(_lib.SvpcKernelError):                                  # CPU ids: no fallback
        scst.sequence_loss(tr, inputs, dec, w)
    sc = scst.SelfCritical(tr, None)
    for kw in (dict(num_samples=17), dict(num_samples=1, baseline="mean"), dict(baseline="best"), dict(utility="METEOR")):
        with pytest.raises(ValueError):
            sc.step(inputs, ["a", "b"], **kw)


def test_shared_key_rows_are_refused_under_grad():
    """K segments over the same memory rows would overwrite each other's dK / dV rows instead of summing them"""
    lt, nm, K = 4, 3, 2
    shared = ops.SeqInfo([r * lt for r in range(4)], [lt] * 4, [(r // K) * nm for r in range(4)], [nm] * 4)
    own = ops.SeqInfo.uniform(4, lt, nm)
    assert shared.shares_keys and not own.shares_keys
    q, kv = torch.zeros(16, 8), torch.zeros(6, 16, requires_grad=True)
    with pytest.raises(_lib.SvpcKernelError, match="share"):
        ops.attention(q, kv, (0, 0, 8), 8, 2, shared)


def test_no_cpu_fallback():
    tgt, ln, w = torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2)
    with pytest.raises(_lib.SvpcKernelError):
        ops.seq_nll(torch.zeros(8, 10), [10, 10], tgt, ln, w, False, UNK)
    with pytest.raises(_lib.SvpcKernelError):
        ops.scst_weights(torch.zeros(2, 3, dtype=torch.float64), [0, 1, 1], "mean")
    with pytest.raises(_lib.SvpcKernelError):
        ops.check_scst(torch.zeros(2, 3, 22, dtype=torch.int64))
    with pytest.raises(_lib.SvpcKernelError):
        ops.check_scst(weights=torch.zeros(6))


def test_symbols_declared_and_exported():
    decls = _lib.declarations()
    lib = _lib.load()
    for name, n_args in (("svpc_seq_nll_fwd", 16), ("svpc_seq_nll_bwd", 16), ("svpc_scst_weights", 10)):
        assert name in decls and len(decls[name][1]) == n_args and hasattr(lib, name), name
    assert lib.svpc_abi_version() == 2
    from svpc_amd import scst
    assert callable(scst.sequence_loss) and hasattr(scst.SelfCritical, "step")
    for fn in ("check_scst", "scst_weights", "seq_nll"):
        assert callable(getattr(ops, fn))
