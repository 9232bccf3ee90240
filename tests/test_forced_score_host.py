"""Forced decoding without a GPU: the restatement (tests/forced_score_reference.py) on hand-built score rows, the literal anchor,
``Translator.gold_captions`` against ``synthetic``'s label layout, every host check, no CPU fallback, the exported symbols."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import forced_score_reference as fr  # noqa: E402
from svpc_amd import _lib, ops, synthetic as syn  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, IGNORE, PAD, UNK  # noqa: E402

NINF = -np.inf
f32 = np.float32


def _rows(n, C, fill):
    return np.full((n, C), fill, np.float32)


def test_anchor_literal():
    """C = 8, p(7) = 0.5, p(EOS = 5) = 0.25: caption BOS 7 EOS"""
    assert (BOS, EOS, UNK, PAD) == (4, 5, 6, 0)
    rows = np.array([[0.03125, 0.03125, 0.03125, 0.03125, 0.0625, 0.25, 0.0625, 0.5]] * 3, np.float32)
    r = fr.score_caption(rows, [BOS, 7, EOS, PAD], 8, logits=False)
    assert r["cum"] == f32(f32(math.log(0.5)) + f32(math.log(0.25)))
    assert r["cum"].dtype == np.float32 and r["len"] == 2 and r["finished"] == 1 and r["n_scored"] == 2
    assert r["rank"].tolist() == [0, 1, -1] and r["top"].tolist() == [7, 7, -1]
    assert r["step"].tolist() == [f32(math.log(0.5)), f32(math.log(0.25)), 0.0]
    assert r["top_step"].tolist() == [f32(math.log(0.5)), f32(math.log(0.5)), 0.0]


@pytest.mark.parametrize("logits", [False, True])
def test_ends(logits):
    rng = np.random.default_rng(3 + logits)
    C, Lt = 12, 6
    rows = (rng.random((Lt, C)).astype(np.float32) + 0.01) if not logits else rng.standard_normal((Lt, C)).astype(np.float32)
    st = [fr.step_scores(rows[i], logits) for i in range(Lt)]
    # EOS ends the row and counts
    r = fr.score_caption(rows, [BOS, 8, 9, EOS, 10, 11], C, logits)
    assert (r["len"], r["finished"], r["n_scored"]) == (3, 1, 3)
    assert r["cum"] == f32(f32(st[0][8] + st[1][9]) + st[2][EOS])
    assert r["step"][3:].tolist() == [0.0, 0.0] and r["rank"][3:].tolist() == [-1, -1] and r["top"][3:].tolist() == [-1, -1]
    # PAD (and IGNORE) end the row and do not count; nothing after is looked at
    for stop in (PAD, IGNORE):
        r = fr.score_caption(rows, [BOS, 8, 9, stop, 10, EOS], C, logits)
        assert (r["len"], r["finished"], r["n_scored"]) == (2, 0, 2)
        assert r["cum"] == f32(st[0][8] + st[1][9])
    # no end at all
    r = fr.score_caption(rows, [BOS, 8, 9, 10, 11, 7], C, logits)
    assert (r["len"], r["finished"], r["n_scored"]) == (Lt - 1, 0, Lt - 1)
    # an all-PAD caption
    r = fr.score_caption(rows, [BOS, PAD, PAD, PAD, PAD, PAD], C, logits)
    assert (r["len"], r["finished"], r["n_scored"], float(r["cum"])) == (0, 0, 0, 0.0)
    # K = 1 through the batch form: (R·Lt, C) rows, two captions of different C
    both = fr.score_rows(np.concatenate([rows, rows]), [[BOS, 8, EOS, PAD, PAD, PAD], [BOS, 11, 9, EOS, PAD, PAD]], [12, 10], logits)
    assert both["len"].tolist() == [2, 3] and both["rank"].shape == (2, Lt - 1)
    assert both["rank"][1, 0] == -1 and both["step"][1, 0] == NINF             # column 11 is outside the second row's 10 columns
    if logits:                                                                 # the log-sum-exp runs over the row's own columns
        assert both["step"][1, 1] == fr.step_scores(rows[1][:10], True)[9]


@pytest.mark.parametrize("logits", [False, True])
def test_non_candidates_and_zero_probability(logits):
    C, Lt = 10, 5
    rows = _rows(Lt, C, 0.1) if not logits else _rows(Lt, C, 0.0)
    rows[:, UNK] = 0.9 if not logits else 9.0                                  # UNK would win every comparison were it a candidate
    rows[2, 8] = 0.0 if not logits else -5.0
    y = [BOS, UNK, C, 8, EOS]                                                  # target UNK, target >= C_r, p = 0 (pointer modes)
    bar = fr.score_caption(rows, y, C, logits, "bar")
    skip = fr.score_caption(rows, y, C, logits, "skip")
    assert bar["rank"].tolist()[:2] == [-1, -1] and skip["rank"].tolist()[:2] == [-1, -1]
    assert bar["step"][0] == NINF and bar["step"][1] == NINF and bar["cum"] == NINF and bar["n_scored"] == 4
    assert skip["step"][0] == 0.0 and skip["step"][1] == 0.0 and skip["n_scored"] == 2
    assert bar["top"][0] != UNK and bar["top"][0] == 0                         # equal values: the lower column first, UNK never
    assert bar["rank"][2] == C - 2                                             # the zero column is behind every other candidate
    if not logits:
        assert skip["step"][2] == NINF and skip["cum"] == NINF                 # p = 0 is −inf under both rules
    else:
        assert np.isfinite(skip["cum"])
        lse = math.log(8 * math.exp(0.0) + math.exp(-5.0))                     # UNK is not in the log-sum-exp
        assert abs(float(skip["step"][2]) - (-5.0 - lse)) < 1e-6
    neg = fr.score_caption(rows, [BOS, -7, EOS, PAD, PAD], C, logits, "skip")
    assert neg["rank"][0] == -1 and neg["n_scored"] == 1 and neg["finished"] == 1


def test_rank_ties_go_to_the_lower_column():
    C = 9
    rows = _rows(3, C, 0.125)
    rows[0, 3] = 0.25
    r = fr.score_caption(rows, [BOS, 8, EOS], C, False)
    # ahead of column 8: column 3 (higher) and the equal columns 0, 1, 2, 4, 5, 7 (UNK = 6 is no candidate)
    assert r["rank"][0] == 7 and r["top"][0] == 3
    r = fr.score_caption(rows, [BOS, 1, EOS], C, False)
    assert r["rank"][0] == 2                                                   # column 3, then the equal column 0


def test_gold_captions_follow_the_label_layout():
    from svpc_amd.translator import Translator
    cfg = syn.make_config(model_type="vivt", hidden_size=64, num_hidden_layers=1, num_attention_heads=2)
    batch = syn.make_batch(cfg, n_videos=3, max_steps=3, step_nums=[3, 1, 2], n_ingr=3, n_oov=[2, 0, 1], seed=5)
    tr = object.__new__(Translator)
    tr.max_v_len, tr.max_t_len = cfg.max_v_len, cfg.max_t_len
    gold = tr.gold_captions(batch["input_labels_list"], batch["batch_step_num"])
    ref = fr.gold_rows([t.numpy() for t in batch["input_labels_list"]], batch["batch_step_num"], cfg.max_v_len, cfg.max_t_len)
    assert [tuple(g.shape) for g in gold] == [(3, cfg.max_t_len), (1, cfg.max_t_len), (2, cfg.max_t_len)]
    saw_eos = saw_oov = False
    for g, r, ids in zip(gold, ref, range(3)):
        assert g.dtype == torch.int64
        np.testing.assert_array_equal(g.numpy(), r)
        assert (g[:, 0] == BOS).all() and not (g == IGNORE).any()
        saw_eos |= bool((g == EOS).any())
        saw_oov |= bool((g >= cfg.vocab_size).any())
    assert saw_eos
    # the captions are the text half of the inputs, with copied words as extended ids: BOS w_1 … w_n EOS, PAD after
    for b, S_b in enumerate(batch["batch_step_num"]):
        for s in range(S_b):
            text = batch["input_ids_list"][s][b][cfg.max_v_len:]
            n = int((gold[b][s] == EOS).nonzero()[0])
            known = gold[b][s][:n + 1] < cfg.vocab_size
            assert torch.equal(gold[b][s][:n + 1][known], text[:n + 1][known]) and (text[:n + 1][~known] == UNK).all()
            assert (gold[b][s][n + 1:] == PAD).all()
    assert ops.stack_captions(gold)[0].data_ptr() == gold[0].data_ptr()       # consecutive views of one buffer
    with pytest.raises(ValueError):
        tr.gold_captions(batch["input_labels_list"], [3, 1])


def test_value_errors():
    ok = torch.zeros(4, 3, 22, dtype=torch.int64)
    for bad in (torch.zeros(4, 17, 22, dtype=torch.int64), torch.zeros(4, 0, 22, dtype=torch.int64),        # K outside 1 … 16
                torch.zeros(4, 22, dtype=torch.float32), torch.zeros(4, 22, dtype=torch.int16),              # dtype
                torch.zeros(22, dtype=torch.int64), torch.zeros(2, 2, 3, 22, dtype=torch.int64),             # shape
                torch.zeros(4, 3, 1, dtype=torch.int64), [[0] * 22]):
        with pytest.raises(ValueError):
            ops.check_force(bad)
    with pytest.raises(ValueError):
        ops.check_force(ok, lt=21)                                             # Lt is not the model's
    with pytest.raises(ValueError):
        ops.check_force(ok, lt=22, steps=[2, 1])                               # structure / steps mismatch
    with pytest.raises(ValueError):
        ops.check_force(ok, lt=22, steps=[5, -1])
    for unk in ("drop", None, 0):
        with pytest.raises(ValueError):
            ops.check_force(ok, unk=unk)
    with pytest.raises(ValueError):
        ops.force_score(torch.zeros(8, 10), [10, 10], torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), False, UNK,
                        unk="drop")
    with pytest.raises(ValueError):                                            # rows wider than the score matrix
        ops.force_score(torch.zeros(8, 10), [10, 11], torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), False, UNK)
    with pytest.raises(ValueError):                                            # fewer score rows than R·Lt
        ops.force_score(torch.zeros(7, 10), [10, 10], torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), False, UNK)
    with pytest.raises(ValueError):                                            # one column count per caption row
        ops.force_score(torch.zeros(8, 10), [10], torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), False, UNK)
    with pytest.raises(ValueError):
        ops.force_inputs(ok, 5, UNK, EOS, PAD)                                 # UNK outside the vocabulary


def test_translator_checks_on_the_host():
    from svpc_amd.translator import Translator
    tr = object.__new__(Translator)                                            # (the checks come before any use of the model)
    tr.max_t_len = 22
    inputs = [None] * 11 + [[2, 1]]
    dec = [torch.zeros(2, 3, 22, dtype=torch.int64), torch.zeros(1, 3, 22, dtype=torch.int64)]
    with pytest.raises(ValueError):
        tr.score_captions(inputs, dec, unk="drop")
    with pytest.raises(ValueError):
        tr.score_captions(inputs, [d[:, :, :21] for d in dec])
    with pytest.raises(ValueError):
        tr.score_captions(inputs, [d.repeat(1, 6, 1) for d in dec])           # K = 18
    with pytest.raises(ValueError):
        tr.score_captions(inputs, [d.float() for d in dec])
    with pytest.raises(ValueError):
        tr.score_captions(inputs, [])
    with pytest.raises(ValueError, match="step counts"):                       # structure mismatch
        tr.score_captions([None] * 11 + [[1, 2]], dec)
    with pytest.raises(_lib.SvpcKernelError):                                  # CPU ids: no fallback
        tr.score_captions(inputs, dec)


def test_steps_mismatch_is_a_value_error():
    """ids on the CPU reach the device check first, so the structure check is exercised through ``check_force`` and the message"""
    with pytest.raises(ValueError, match="do not add up"):
        ops.check_force(torch.zeros(3, 22, dtype=torch.int32), lt=22, steps=[1, 1])


def test_no_cpu_fallback():
    ids = torch.zeros(2, 3, 22, dtype=torch.int64)
    with pytest.raises(_lib.SvpcKernelError):
        ops.check_force(ids)
    with pytest.raises(_lib.SvpcKernelError):
        ops.force_inputs(ids, 100, UNK, EOS, PAD)
    with pytest.raises(_lib.SvpcKernelError):
        ops.force_score(torch.zeros(8, 10), [10, 10], torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), False, UNK)
    with pytest.raises(_lib.SvpcKernelError):
        ops.force_accum(torch.zeros(2), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                        torch.zeros(2, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(9, dtype=torch.float64))
    from svpc_amd.metrics import ForcedScores
    with pytest.raises(_lib.SvpcKernelError):
        ForcedScores(device="cpu")


def test_symbols_declared_and_exported():
    decls = _lib.declarations()
    lib = _lib.load()
    for name, n_args in (("svpc_force_inputs", 15), ("svpc_force_score", 16), ("svpc_force_finish", 14), ("svpc_force_accum", 9)):
        assert name in decls and len(decls[name][1]) == n_args and hasattr(lib, name), name
    assert lib.svpc_abi_version() == 2
    from svpc_amd import metrics, translator
    assert hasattr(translator.Translator, "score_captions") and hasattr(translator.Translator, "gold_captions")
    assert translator.FORCE == "force" and hasattr(metrics, "ForcedScores")
    for fn in ("check_force", "force_inputs", "force_score", "force_accum"):
        assert callable(getattr(ops, fn))
