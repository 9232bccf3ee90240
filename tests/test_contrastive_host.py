"""Contrastive search without a GPU: the CPU reference (tests/contrastive_reference.py) against greedy where the rule reduces to it, the
penalty's effect, a hand-checked step, and every host-side refusal of the new entry points."""
import numpy as np
import pytest
import torch

import beam_reference as br
import contrastive_reference as cr
from svpc_amd import ops
from svpc_amd.synthetic import EOS, PAD, UNK

CASES = [("tiny", "v"), ("tiny", "vi"), ("tiny", "viv"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")]      # test_beam_gpu.CASES


@pytest.mark.parametrize("k,alpha", [(1, 0.6), (4, 0.0)])
@pytest.mark.parametrize("case,mt", CASES)
def test_reference_reduces_to_greedy(golden_dir, case, mt, k, alpha):
    """the candidate rows are in descending-p order and ties go to the lowest row: α = 0 and k = 1 pick what a width-1 beam picks"""
    z = np.load("%s/%s_%s.npz" % (golden_dir, case, mt))
    ids, cum, ln, pen, _, _ = cr.decode_case(golden_dir, case, mt, k, alpha)
    for b, d in enumerate(ids):
        g = br.greedy_equivalent(torch.from_numpy(z["decode/%d" % b]))
        np.testing.assert_array_equal(d.numpy(), g.numpy())
        assert np.all(cum[b] <= 0) and np.all(np.isfinite(cum[b]))
        for s in range(d.shape[0]):                      # len as translate_batch_nbest counts: the position of EOS, else Lt − 1
            hit = (g[s, 1:] == EOS).nonzero()
            assert ln[b][s] == (int(hit[0]) + 1 if len(hit) else d.shape[1] - 1)
            assert pen[b][s, 0] == 0 and np.all(pen[b][s, ln[b][s] + 1:] == 0)


@pytest.mark.parametrize("mt", ["v", "vi", "viv", "vivt"])
def test_the_penalty_changes_every_tiny_caption(golden_dir, mt):
    z = np.load("%s/tiny_%s.npz" % (golden_dir, mt))
    ids = cr.decode_case(golden_dir, "tiny", mt, 4, 0.6)[0]
    same = total = 0
    for b, d in enumerate(ids):
        g = br.greedy_equivalent(torch.from_numpy(z["decode/%d" % b]))
        same += int((d == g).all(1).sum()); total += d.shape[0]
    assert same == 0 and total > 0, (same, total)


def _hand_step(alpha):
    """two candidates, p = (0.5, 0.2); the history holds candidate 0's hidden state exactly, candidate 1's is orthogonal to it"""
    D, lt, k = 8, 4, 2
    st = cr.new_state(1, k, lt, D)
    h = np.zeros((2, D), np.float32); h[0, 0] = 2.0; h[1, 1] = 3.0
    st["cand_p"][:] = [0.5, 0.2]
    st["cand_s"][:] = np.log(np.array([0.5, 0.2])).astype(np.float32)
    st["ids"][0, 0] = 4; st["H"][0, 0] = h[0]; st["Hn"][0, 0] = 4.0
    scores = np.full((2, 9), 0.01, np.float32)
    return cr.select(scores, [9, 9], [0, 0], k, False, 1, h, np.array([3, 5]), st, alpha)


def test_hand_checked_step():
    st, o = _hand_step(0.6)          # 0.4·0.5 − 0.6·1 = −0.4 against 0.4·0.2 − 0 = 0.08
    np.testing.assert_allclose(o["score_all"], [-0.4, 0.08], atol=1e-15)
    assert o["winner"][0] == 1 and st["ids"][0, 1] == 5 and st["pen"][0, 1] == 0
    st, o = _hand_step(0.2)          # 0.8·0.5 − 0.2·1 = 0.2 against 0.8·0.2 = 0.16
    np.testing.assert_allclose(o["score_all"], [0.2, 0.16], atol=1e-15)
    assert o["winner"][0] == 0 and st["ids"][0, 1] == 3 and st["pen"][0, 1] == 1
    assert st["cum"][0] == np.float32(np.log(0.5)) and st["len"][0] == 1


def test_select_dead_finished_and_filters():
    D, lt, k = 4, 5, 3
    h = np.ones((6, D), np.float32)
    st = cr.new_state(2, k, lt, D)
    st["cand_p"][:] = [0.0, 0.0, 0.0, 0.3, 0.3, 0.0]            # sentence 0: nothing live; sentence 1: an exact tie, a dead row
    st["cand_s"][:] = [-np.inf] * 3 + [-1.0, -1.0, -np.inf]
    st["H"][:, 0] = 1.0; st["Hn"][:, 0] = D
    p = np.zeros((6, 12), np.float32)
    p[3, UNK] = 0.9; p[3, EOS] = 0.5; p[3, 7] = 0.25; p[3, 2] = 0.25            # only two allowed positive columns: a dead third child
    st2, o = cr.select(p, [12] * 6, [0] * 6, k, False, 1, h, np.array([1, 1, 1, 8, 9, 1]), st, 0.5, min_length=2)
    assert list(o["winner"]) == [-1, 0] and st2["fin"][0] and st2["cum"][0] == -np.inf and st2["ids"][0, 1] == PAD
    assert o["margin_sel"][1] == 0 and st2["ids"][1, 1] == 8
    assert list(o["ext"][3:]) == [2, 7, PAD] and list(st2["cand_p"][3:]) == [0.25, 0.25, 0.0] and list(o["parent"][3:]) == [3, 3, 3]
    assert list(o["ext"][:3]) == [PAD] * 3
    st3, o3 = cr.select(p, [12] * 6, [0] * 6, k, False, 2, h, np.array([1] * 6), st2, 0.5)
    assert o3["winner"][0] == -1 and st3["cum"][0] == -np.inf and np.all(st3["ids"][0, 2:] == PAD)      # a finished sentence changes nothing


def test_check_contrastive_refusals():
    ok = ops.check_contrastive(22, 4, 0.6, 0, 500)
    assert ok == dict(top_k=4, penalty_alpha=float(np.float32(0.6)), min_length=0)
    for bad in (True, 2.0, "3", 0, 9, None):
        with pytest.raises(ValueError):
            ops.check_contrastive(22, bad, 0.6)
    for bad in (True, "0.5", None, float("nan"), float("inf"), -0.1, 1.5):
        with pytest.raises(ValueError):
            ops.check_contrastive(22, 4, bad)
    for bad in (True, 1.5, -1, 22):
        with pytest.raises(ValueError):
            ops.check_contrastive(22, 4, 0.6, bad)
    with pytest.raises(ValueError):
        ops.check_contrastive(22, 4, 0.6, 0, 4097)
    assert ops.check_contrastive(22, 8, 1, 21, 4096)["penalty_alpha"] == 1.0


def _translator(cls, incremental=True):
    from types import SimpleNamespace
    tr = cls.__new__(cls)
    tr.incremental, tr.max_t_len, tr.opt = incremental, 22, SimpleNamespace()
    tr.model_config = SimpleNamespace(model_mode="video", vocab_size=100)
    return tr


def test_translator_contract_errors():
    from svpc_amd.ensemble import EnsembleTranslator
    from svpc_amd.translator import Translator
    inputs = [None] * 8 + [[{}]] + [None] * 3
    tr = _translator(Translator)
    with pytest.raises(TypeError):
        tr.translate_batch_contrastive(inputs, beam_size=4)
    for kw in (dict(top_k=0), dict(top_k=9), dict(top_k=True), dict(top_k=2.5), dict(penalty_alpha=1.01), dict(penalty_alpha=float("nan")),
               dict(penalty_alpha="x"), dict(min_length=22), dict(min_length=-1)):
        with pytest.raises(ValueError):
            tr.translate_batch_contrastive(inputs, **kw)
    tr.model_config.vocab_size = 4097
    with pytest.raises(ValueError):
        tr.translate_batch_contrastive(inputs)
    tr.model_config.vocab_size = 100
    tr.opt.top_k = 99                                   # the defaults come from opt and are checked alike
    with pytest.raises(ValueError):
        tr.translate_batch_contrastive(inputs)
    with pytest.raises(NotImplementedError):
        _translator(Translator, incremental=False).translate_batch_contrastive(inputs)
    with pytest.raises(NotImplementedError, match="hidden"):
        _translator(EnsembleTranslator).translate_batch_contrastive(inputs)


def test_decode_key_separates_alpha():
    from svpc_amd.translator import BEAM, Decode
    a = Decode(BEAM, 4, contrastive=(4, float(np.float32(0.6)), 0))
    b = Decode(BEAM, 4, contrastive=(4, float(np.float32(0.5)), 0))
    assert a.key != b.key and a.key != Decode(BEAM, 4).key and not a.ranked
    assert a.key == Decode(BEAM, 4, contrastive=(4, float(np.float32(0.6)), 0)).key


def test_library_exports_the_contrastive_step():
    from svpc_amd import _lib
    assert "svpc_contrastive_step" in _lib.declarations()
    lib = _lib.load()
    assert lib.svpc_abi_version() == 2 and hasattr(lib, "svpc_contrastive_step")


def test_cpu_tensors_are_refused():
    from svpc_amd._lib import SvpcKernelError
    T, k, lt, D = 2, 2, 5, 8
    R = T * k
    toks = [[torch.zeros(R, lt, dtype=torch.int32) for _ in range(3)] for _ in range(2)]
    args = dict(cand_p=torch.zeros(R), cand_score=torch.zeros(R), ids=torch.zeros(T, lt, dtype=torch.int32), cum=torch.zeros(T),
                length=torch.zeros(T, dtype=torch.int32), pen=torch.zeros(T, lt), finished=torch.zeros(T, dtype=torch.int32),
                hist=torch.zeros(T, lt, D), hist_n2=torch.zeros(T, lt, dtype=torch.float64))
    with pytest.raises(SvpcKernelError):
        ops.contrastive_step(torch.zeros(R, 16), [16] * R, [0] * R, k, 1, False, UNK, EOS, PAD, torch.zeros(R, D), toks_in=toks[0],
                             toks_out=toks[1], slot_rows=lt, alpha=0.5, **args)
    with pytest.raises(ValueError):                     # … after the host checks: a position outside the tables
        ops.contrastive_step(torch.zeros(R, 16), [16] * R, [0] * R, k, lt, False, UNK, EOS, PAD, torch.zeros(R, D), toks_in=toks[0],
                             toks_out=toks[1], slot_rows=lt, alpha=0.5, **args)
