"""Diverse (group) beam search without a GPU: the rule of tests/diverse_beam_reference.py on hand-built rows, its agreement with
``select_ctl`` (G = 1, and λ = 0 as G copies of a width-Bg search), the host-side checks of ops and Translator, and the kernel
library's new entry point.

The literal anchor (``test_anchor_two_groups_from_bos``), worked by hand: W = 2, G = 2 (Bg = 1), probabilities mode, position 0, so both
groups hold the BOS parent with cum = aug = 0, and the same row p(a) = 0.5, p(b) = 0.3, the rest smaller.  Group 0 picks a: cum = aug =
fp32(ln 0.5) = −0.6931.  Group 1 sees n(a) = 1:
  λ = 0    a: −0.6931 − 0   = −0.6931 > ln 0.3 = −1.2040 → a, cum = aug = fp32(ln 0.5);
  λ = 0.5  a: −0.6931 − 0.5 = −1.1931 > −1.2040         → still a, cum = fp32(ln 0.5), aug = fp32(fp32(ln 0.5) − 0.5);
  λ = 0.6  a: −0.6931 − 0.6 = −1.2931 < −1.2040         → b, cum = aug = fp32(ln 0.3)."""
import math
import types

import numpy as np
import pytest
import torch

import beam_controls_reference as bcr
import diverse_beam_reference as dbr
from svpc_amd import ops
from svpc_amd.synthetic import BOS, EOS, PAD, UNK

NEG = np.float32(-np.inf)
C = 12                                           # columns of the hand-made tables (UNK and EOS among them)
A, B_ = 9, 8                                     # the two words of the anchor


def _sel(p, W, G, lam, pos=0, cum=None, aug=None, fin=None, length=None, hist=None, **ctl):
    p = np.asarray(p, np.float32)
    R = p.shape[0]
    cum = dbr.start_scores(R // W, W, G) if cum is None else np.asarray(cum, np.float32)
    aug = cum.copy() if aug is None else np.asarray(aug, np.float32)
    fin = np.zeros(R, bool) if fin is None else np.asarray(fin, bool)
    length = np.zeros(R, np.int64) if length is None else np.asarray(length, np.int64)
    if hist is None:
        hist = np.full((R, pos + 1), 4, np.int64)
        hist[:, 0] = BOS
    return dbr.select_groups(p, [C] * R, [0] * R, W, G, False, cum, aug, fin, length, np.asarray(hist).reshape(R, -1), pos,
                             dbr.penalty_table(lam, W), **ctl)


def _row(first, second, n=1, pf=0.5, ps=0.3):
    p = np.full((n, C), 0.01, np.float32)
    p[:, first] = pf
    p[:, second] = ps
    return p


def test_anchor_two_groups_from_bos():
    ln5, ln3 = np.float32(math.log(0.5)), np.float32(math.log(np.float64(np.float32(0.3))))
    p = _row(A, B_, 2)
    par, ext, mod, cum, aug, fin, ln = _sel(p, 2, 2, 0.0)
    assert ext.tolist() == [A, A] and par.tolist() == [0, 1] and ln.tolist() == [1, 1]
    assert cum.tolist() == [ln5, ln5] and aug.tolist() == [ln5, ln5]
    par, ext, mod, cum, aug, fin, ln = _sel(p, 2, 2, 0.5)
    assert ext.tolist() == [A, A]
    assert cum.tolist() == [ln5, ln5] and aug.tolist() == [ln5, np.float32(ln5 - np.float32(0.5))]
    par, ext, mod, cum, aug, fin, ln = _sel(p, 2, 2, 0.6)
    assert ext.tolist() == [A, B_] and par.tolist() == [0, 1]
    assert cum.tolist() == [ln5, ln3] and aug.tolist() == [ln5, ln3]


def test_penalty_table_matches_the_product():
    for lam in (0.0, 0.1, 0.5, 0.6, 1e4, 3.3e-7):
        for W in (1, 4, 8):
            ref = dbr.penalty_table(lam, W)
            got = np.array(ops.diversity_table(lam, W), dtype=np.float64)
            assert got.astype(np.float32).view(np.int32).tolist() == ref.view(np.int32).tolist()
            assert np.array_equal(got, ref.astype(np.float64))          # (already fp32 values)


def test_finished_parents_carry_themselves_unpenalised_and_uncounted():
    # W = 2, G = 2, position 3.  Group 0's parent is finished (it carries PAD); group 1's parent ranks PAD first: were the carried PAD
    # counted, group 1 would pay for it
    p = _row(PAD, B_, 2)
    par, ext, mod, cum, aug, fin, ln = _sel(p, 2, 2, 10.0, pos=3, cum=[-1.0, -2.0], aug=[-1.5, -2.0], fin=[True, False], length=[2, 0])
    assert ext.tolist() == [PAD, PAD] and fin.tolist() == [True, False]
    assert cum[0] == np.float32(-1.0) and aug[0] == np.float32(-1.5) and ln.tolist() == [2, 4]
    assert aug[1] == np.float32(np.float32(-2.0) + np.float32(math.log(0.5)))          # no penalty paid
    # and a finished parent of a later group pays nothing for carrying PAD although group 0 picked PAD as a word
    par, ext, mod, cum, aug, fin, ln = _sel(p, 2, 2, 10.0, pos=3, cum=[-1.0, -2.0], aug=[-1.0, -2.5], fin=[False, True], length=[0, 3])
    assert ext.tolist() == [PAD, PAD] and fin.tolist() == [False, True] and aug[1] == np.float32(-2.5) and ln.tolist() == [4, 3]


def test_eos_is_counted():
    p = _row(EOS, B_, 2)
    _, ext, _, cum, aug, fin, _ = _sel(p, 2, 2, 0.6, pos=2, cum=[0.0, 0.0])
    assert ext.tolist() == [EOS, B_] and fin.tolist() == [True, False]
    _, ext, _, _, _, _, _ = _sel(p, 2, 2, 0.0, pos=2, cum=[0.0, 0.0])
    assert ext.tolist() == [EOS, EOS]


def test_fill_rows_when_a_group_has_fewer_than_bg_candidates():
    # W = 4, G = 2 (Bg = 2), rows of ONE column (column 0, p = 0.5), position 1.  Row 1 has used word 0 and unigram blocking bans it: group
    # 0 has one candidate, so its second slot is a fill row (parent the slot itself, PAD, −inf, finished, length p).  Group 1's two rows
    # both pick word 0 and pay pen[1]: group 0's live pick counts, its fill row does not
    p = np.full((4, 1), 0.5, np.float32)
    hist = np.array([[BOS, 7], [BOS, 0], [BOS, 7], [BOS, 7]], np.int64)
    cum = np.array([-1.0, -1.0, -1.0, -2.0], np.float32)
    out = dbr.select_groups(p, [1] * 4, [0] * 4, 4, 2, False, cum, cum.copy(), np.zeros(4, bool), np.ones(4, np.int64), hist, 1,
                            dbr.penalty_table(0.5, 4), block_ngram_repeat=1)
    par, ext, mod, cum2, aug2, fin, ln = out
    ln5 = np.float32(math.log(0.5))
    assert par.tolist() == [0, 1, 2, 3] and ext.tolist() == [0, PAD, 0, 0] and mod.tolist() == [0, PAD, 0, 0]
    assert fin.tolist() == [False, True, False, False] and ln.tolist() == [2, 2, 2, 2]
    assert cum2[1] == NEG and aug2[1] == NEG
    assert cum2[0] == np.float32(-1.0) + ln5 and aug2[0] == cum2[0]
    assert cum2[2] == np.float32(-1.0) + ln5 and aug2[2] == np.float32(np.float32(np.float32(-1.0) + ln5) - np.float32(0.5))
    assert aug2[3] == np.float32(np.float32(np.float32(-2.0) + ln5) - np.float32(0.5))


def test_ties_go_to_the_lower_flat_index():
    # W = 2, G = 1: both parents equal, two equal best columns: the order is (h 0, col lo), (h 0, col hi)
    p = _row(A, B_, 2, pf=0.4, ps=0.4)
    par, ext, *_ = _sel(p, 2, 1, 0.5, pos=2, cum=[-1.0, -1.0])
    assert par.tolist() == [0, 0] and ext.tolist() == [min(A, B_), max(A, B_)]
    # two groups, λ = 0: each picks the lower column of its own parent
    par, ext, *_ = _sel(p, 2, 2, 0.0, pos=2, cum=[-1.0, -1.0])
    assert par.tolist() == [0, 1] and ext.tolist() == [min(A, B_)] * 2
    # any λ > 0 breaks the tie for group 1 towards the other word
    par, ext, *_ = _sel(p, 2, 2, 1e-3, pos=2, cum=[-1.0, -1.0])
    assert ext.tolist() == [min(A, B_), max(A, B_)]


def test_groups_never_exchange_hypotheses():
    # W = 4, G = 2: group 1's parents are far better than group 0's; group 0 still keeps its own
    p = _row(A, B_, 4)
    par, ext, _, cum, aug, _, _ = _sel(p, 4, 2, 0.0, pos=2, cum=[-50.0, -60.0, -1.0, -2.0])
    assert par.tolist() == [0, 0, 2, 2] and ext.tolist() == [A, B_, A, B_]
    rng = np.random.default_rng(5)
    for _ in range(20):
        p = rng.random((6, C)).astype(np.float32)
        cum = (-rng.random(6) * 5).astype(np.float32)
        par, *_ = _sel(p, 6, 3, 0.7, pos=2, cum=cum)
        assert all(par[k] // 2 == k // 2 for k in range(6))


def test_min_length_and_ngram_bans_combined_with_a_penalty():
    # W = 2, G = 2, position 2 → p = 3.  The row ranks EOS first, A second, B_ third.  min_length 3 removes EOS: group 0 takes A, and group 1
    # — penalised on A — takes B_; with A also banned for group 1's parent by unigram blocking it takes B_ even at λ = 0
    p = np.full((2, C), 0.01, np.float32)
    p[:, EOS], p[:, A], p[:, B_] = 0.5, 0.3, 0.25
    hist = np.array([[BOS, 4, 4], [BOS, 4, 4]], np.int64)
    _, ext, *_ = _sel(p, 2, 2, 0.0, pos=2, cum=[0.0, 0.0], hist=hist)
    assert ext.tolist() == [EOS, EOS]
    _, ext, *_ = _sel(p, 2, 2, 0.0, pos=2, cum=[0.0, 0.0], hist=hist, min_length=3)
    assert ext.tolist() == [A, A]
    _, ext, _, cum, aug, _, _ = _sel(p, 2, 2, 0.5, pos=2, cum=[0.0, 0.0], hist=hist, min_length=3)
    assert ext.tolist() == [A, B_] and cum[1] == aug[1]
    hist[1, 2] = A
    _, ext, *_ = _sel(p, 2, 2, 0.0, pos=2, cum=[0.0, 0.0], hist=hist, min_length=3, block_ngram_repeat=1)
    assert ext.tolist() == [A, B_]
    # the ban and the penalty together: group 1's parent may not take B_ (banned) and pays for A → it takes A only while the penalty is small
    hist[1, 2] = B_
    _, ext, _, cum, aug, _, _ = _sel(p, 2, 2, 0.5, pos=2, cum=[0.0, 0.0], hist=hist, min_length=3, block_ngram_repeat=1)
    assert ext.tolist() == [A, A] and aug[1] == np.float32(np.float32(math.log(np.float64(np.float32(0.3)))) - np.float32(0.5))
    _, ext, *_ = _sel(p, 2, 2, 1e4, pos=2, cum=[0.0, 0.0], hist=hist, min_length=3, block_ngram_repeat=1)
    assert ext[1] not in (A, B_, EOS, UNK)


def _random_tables(rng, T, W, pos, logits):
    R = T * W
    Cs = np.repeat(rng.integers(UNK + 3, 40, size=T), W)
    s = rng.choice(np.array([0.0, 0.1, 0.2, 0.4], np.float32), size=(R, int(Cs.max()))) if rng.random() < 0.5 else rng.random((R, int(Cs.max()))).astype(np.float32)
    if logits:
        s = (s * 8 - 4).astype(np.float32)
    cum = (-rng.random(R) * 4).astype(np.float32)
    cum[rng.random(R) < 0.15] = -np.inf
    fin = rng.random(R) < 0.25
    length = np.where(fin, rng.integers(1, pos + 1, size=R), 0)
    hist = rng.integers(7, 11, size=(R, pos + 1))
    hist[:, 0] = BOS
    return s.astype(np.float32), Cs, np.zeros(R, np.int64), cum, fin, length, hist


CTLS = [dict(), dict(block_ngram_repeat=1), dict(min_length=5, block_ngram_repeat=2, exclusion_tokens=(8,)),
        dict(length_penalty_name="wu", length_penalty_alpha=0.9), dict(length_penalty_name="avg", min_length=5)]


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("ctl", range(len(CTLS)))
def test_one_group_equals_select_ctl(ctl, logits):
    c = dict(CTLS[ctl])
    lp = dbr.length_table(c.pop("length_penalty_name", "none"), c.pop("length_penalty_alpha", 0.0), 12)
    rng = np.random.default_rng(ctl * 2 + logits)
    for W in (1, 3, 4):
        s, Cs, Xs, cum, fin, length, hist = _random_tables(rng, 6, W, 4, logits)
        for _ in range(2):                          # step for step: the second step starts from the first's result
            ref = bcr.select_ctl(s, Cs, Xs, W, logits, cum, fin, length, hist, 4, lp=lp, **c)
            got = dbr.select_groups(s, Cs, Xs, W, 1, logits, cum, cum.copy(), fin, length, hist, 4, dbr.penalty_table(0.8, W), lp=lp, **c)
            for a, b in zip(ref, got[:4] + got[5:]):
                np.testing.assert_array_equal(np.asarray(a).view(np.int32) if np.asarray(a).dtype == np.float32 else a,
                                              np.asarray(b).view(np.int32) if np.asarray(b).dtype == np.float32 else b)
            np.testing.assert_array_equal(got[3].view(np.int32), got[4].view(np.int32))          # aug ≡ cum
            cum, fin, length = got[3], got[5], got[6]
            hist = hist[ref[0]]
            hist[:, 4] = np.where(ref[1] == PAD, 9, ref[1])


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("W,G", [(4, 2), (6, 3), (8, 4), (8, 2)])
def test_zero_strength_is_g_copies_of_the_narrow_search(W, G, logits):
    Bg = W // G
    rng = np.random.default_rng(W * 10 + G + logits)
    lp = dbr.length_table("wu", 0.6, 12)
    for ctl in (dict(), dict(block_ngram_repeat=1, min_length=5)):
        s, Cs, Xs, cum, fin, length, hist = _random_tables(rng, 5, W, 4, logits)
        got = dbr.select_groups(s, Cs, Xs, W, G, logits, cum, cum.copy(), fin, length, hist, 4, dbr.penalty_table(0.0, W), lp=lp, **ctl)
        for g in range(G):
            rows = np.array([t * W + g * Bg + j for t in range(5) for j in range(Bg)])
            ref = bcr.select_ctl(s[rows], Cs[rows], Xs[rows], Bg, logits, cum[rows], fin[rows], length[rows], hist[rows], 4, lp=lp, **ctl)
            np.testing.assert_array_equal(got[0][rows], rows[ref[0]])
            for a, b in zip(ref[1:], [got[1], got[2], got[3], got[5], got[6]]):
                a, b = np.asarray(a), np.asarray(b)[rows]
                np.testing.assert_array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b)
        # identical inputs in every group → identical copies
        s2, cum2, fin2, len2, hist2 = (np.concatenate([v.reshape(5, G, Bg, *v.shape[1:])[:, :1]] * G, 1).reshape(v.shape)
                                       for v in (s, cum, fin, length, hist))
        got = dbr.select_groups(s2, Cs, Xs, W, G, logits, cum2, cum2.copy(), fin2, len2, hist2, 4, dbr.penalty_table(0.0, W), lp=lp, **ctl)
        for v in got[1:]:
            v = np.asarray(v).reshape(5, G, Bg)
            for g in range(1, G):
                np.testing.assert_array_equal(v[:, g], v[:, 0])


# ------------------------------------------------------------------------------------------------ host-side checks
@pytest.mark.parametrize("bad", [dict(num_groups=1.0), dict(num_groups=2.5), dict(num_groups=True), dict(num_groups=3), dict(num_groups=0),
                                 dict(num_groups=-2), dict(num_groups=8), dict(beam=0), dict(beam=9), dict(beam=4.0),
                                 dict(diversity_strength=-0.1), dict(diversity_strength=float("inf")), dict(diversity_strength=float("nan")),
                                 dict(diversity_strength="0.5"), dict(diversity_strength=None), dict(diversity_strength=1e39),
                                 dict(n_best=0), dict(n_best=3), dict(n_best=1.0)])
def test_check_diverse_refuses(bad):
    kw = dict(beam=4, num_groups=2, diversity_strength=0.5, n_best=None)
    kw.update(bad)
    with pytest.raises(ValueError):
        ops.check_diverse(**kw)


def test_check_diverse_accepts_and_normalises():
    assert ops.check_diverse(4, 2, 0.5) == (4, 2, 0.5, 2)
    assert ops.check_diverse(8, 8, 0, 1) == (8, 8, 0.0, 1)
    assert ops.check_diverse(6, 3, 0.1, 1) == (6, 3, float(np.float32(0.1)), 1)
    assert ops.check_diverse(1, 1, 3) == (1, 1, 3.0, 1)


class _Opt(object):
    cuda = True


def _translator(**opt):
    from svpc_amd.translator import Translator
    tr = Translator.__new__(Translator)
    tr.incremental = True
    tr.opt = _Opt()
    for k, v in opt.items():
        setattr(tr.opt, k, v)
    tr.model_config = types.SimpleNamespace(max_t_len=22, vocab_size=951)
    return tr


def test_translator_refuses_before_device_work():
    inputs = [None] * 12
    tr = _translator()
    for bad in (dict(beam_size=4, num_groups=3), dict(beam_size=9, num_groups=1), dict(beam_size=4, num_groups=2, diversity_strength=-1.0),
                dict(beam_size=4, num_groups=2, n_best=3), dict(beam_size=4, num_groups=2, min_length=22),
                dict(beam_size=4, num_groups=2, block_ngram_repeat=2, block_ngram_scope="paragraph")):
        with pytest.raises(ValueError):
            tr.translate_batch_diverse(inputs, **bad)
    with pytest.raises(ValueError):                  # defaults come from opt
        _translator(beam_size=4, num_groups=3).translate_batch_diverse(inputs)
    with pytest.raises(ValueError):
        _translator(beam_size=4, num_groups=2, diversity_strength=float("nan")).translate_batch_diverse(inputs)
    with pytest.raises(TypeError):
        tr.translate_batch_diverse(inputs, 4, 2, 0.5, no_repeat_ngram_size=3)
    tr.incremental = False
    with pytest.raises(NotImplementedError):
        tr.translate_batch_diverse(inputs, 4, 2, 0.5)


def test_consensus_source_checks():
    tr = _translator()
    for kw in (dict(source="greedy"), dict(source="diverse", num_candidates=4, num_groups=3),
               dict(source="diverse", num_candidates=3, num_groups=2, beam_size=4),
               dict(source="diverse", num_candidates=4, num_groups=2, diversity_strength=-1.0)):
        with pytest.raises(ValueError):
            tr.translate_batch_consensus([None] * 12, None, **kw)


def test_the_decode_key_separates_settings():
    from svpc_amd.translator import BEAM, Decode
    plain = Decode(BEAM, 4, n_best=4)
    a = Decode(BEAM, 4, n_best=2, groups=(2, 0.5))
    b = Decode(BEAM, 4, n_best=1, groups=(2, 0.5))
    c = Decode(BEAM, 4, n_best=2, groups=(2, 0.25))
    d = Decode(BEAM, 4, n_best=1, groups=(4, 0.5))
    assert a.key == b.key and len({plain.key, a.key, c.key, d.key}) == 4
    assert plain.key == (BEAM, 4, None, True, None)            # (the plain decode's key is what it was)


def test_no_cpu_fallback():
    from svpc_amd import _lib
    R, lt, W = 4, 8, 2
    scores = torch.rand(R, 20)
    cum, aug = torch.zeros(R), torch.zeros(R)
    fin, length = torch.zeros(R, dtype=torch.int32), torch.zeros(R, dtype=torch.int32)
    toks = [[torch.zeros(R, lt, dtype=torch.int32) for _ in range(3)] for _ in range(2)]
    pen = torch.tensor(ops.diversity_table(0.5, W), dtype=torch.float32)
    with pytest.raises(_lib.SvpcKernelError):
        ops.beam_step_groups(scores, [20] * R, [0] * R, W, 2, 3, False, UNK, EOS, PAD, cum, aug, fin, length, toks[0], toks[1], lt, pen)
    for bad in (dict(aug=cum), dict(aug=torch.zeros(R, dtype=torch.float64)), dict(pen=pen[:1]), dict(pen=pen.double()), dict(groups=3),
                dict(length=None), dict(lp=torch.ones(3, dtype=torch.float64)), dict(min_length=8)):
        kw = dict(aug=aug, pen=pen, groups=2, length=length)
        extra = {k: bad[k] for k in bad if k not in kw}
        kw.update({k: bad[k] for k in bad if k in kw})
        with pytest.raises(ValueError):
            ops.beam_step_groups(scores, [20] * R, [0] * R, W, kw["groups"], 3, False, UNK, EOS, PAD, cum, kw["aug"], fin, kw["length"], toks[0],
                                 toks[1], lt, kw["pen"], **extra)


def test_library_exports_the_group_entry_point():
    from svpc_amd import _lib
    decl = _lib.declarations()
    assert "svpc_beam_step_groups" in decl
    assert len(decl["svpc_beam_step_groups"][1]) == len(decl["svpc_beam_step_ctl"][1]) + 3
    lib = _lib.load()
    assert lib.svpc_abi_version() == 2
    assert hasattr(lib, "svpc_beam_step_groups")
