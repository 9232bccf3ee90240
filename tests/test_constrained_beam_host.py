"""Lexically constrained beam search without a GPU: the rule of tests/constrained_beam_reference.py on hand-built rows, its
agreement with ``select_ctl`` when no sentence has a constraint, the candidate, tier and bank rules, the final order, the satisfaction
property, the host-side checks of ops and Translator, and the kernel library's two new entry points.

The literal allocation anchor (``test_anchor_allocation``), worked by hand: W = 2, probabilities mode, position 0, one live parent (row 0,
cum 0; row 1 starts at −inf), C = 8, p(a) = 0.5, p(b) = 0.3, p(c) = 0.05, constraint ((c,),).  The live parent's top-2 is {a, b}, its
forced column c: three live candidates, c in bank 1 (rank 0), a and b in bank 0 (ranks 0 and 1).  Ascending (rank, −bank): c, a, b → row 0
is c, cum fp32(ln 0.05), mask 1; row 1 is a, cum fp32(ln 0.5), mask 0.  The −inf row's two dead candidates come after the three live ones
and take no slot.  At the next step EOS is allowed for row 0 (mask full) and skipped for row 1."""
import math
import types

import numpy as np
import pytest
import torch

import beam_controls_reference as bcr
import constrained_beam_reference as cbr
from diverse_beam_reference import length_table
from svpc_amd import ops
from svpc_amd.synthetic import BOS, EOS, PAD, UNK

NEG = np.float32(-np.inf)
A, B_, C_ = 1, 2, 3                                # the anchor's words: ids below C = 8 that are no special id of the decoder
assert len({PAD, BOS, EOS, UNK} & {A, B_, C_}) == 0


def _ln(p):
    return np.float32(math.log(np.float64(np.float32(p))))


def _run(ws, ph):
    s = 0
    banks = []
    for w in ws:
        s = cbr.track(s, w, ph)
        banks.append(cbr.bank(s, ph))
    return s, banks


# ------------------------------------------------------------------------------------------------ the tracker
def test_tracker_anchors():
    ph = ((5, 6), (5,))
    s, banks = _run([5, 6, 5], ph)
    assert cbr.unpack(s) == (0b11, -1, 0) and banks == [1, 2, 3]
    s, banks = _run([5, 7], ph)
    assert s == 0 and banks == [1, 0]
    # in progress, the word is not the continuation but starts a phrase again
    s, banks = _run([5, 5], ph)
    assert cbr.unpack(s) == (0, 0, 1) and banks == [1, 1]
    # a finished phrase is not started again: the second 5 meets the unigram
    s, banks = _run([5, 6, 5, 6], ph)
    assert cbr.unpack(s) == (0b11, -1, 0) and banks == [1, 2, 3, 3]


def test_identical_phrases_are_met_one_after_the_other():
    ph = ((8,), (8,), (9, 8), (9, 8))
    s, banks = _run([8], ph)
    assert cbr.unpack(s)[0] == 0b0001 and banks == [1]
    s, banks = _run([8, 8], ph)
    assert cbr.unpack(s)[0] == 0b0011 and banks == [1, 2]
    s, banks = _run([9, 8, 9, 8], ph)
    assert cbr.unpack(s) == (0b1100, -1, 0) and banks == [1, 2, 3, 4]


def test_the_tracker_is_not_a_string_matcher():
    a, b = 8, 9
    s, _ = _run([a, a, b], ((a, a, b),))
    assert cbr.unpack(s)[0] == 1
    s, banks = _run([a, a, a, b], ((a, a, b),))      # the third a drops the progress and starts again at off 1: b does not complete
    assert cbr.unpack(s) == (0, -1, 0) and banks == [1, 2, 1, 0]
    assert cbr.contains([BOS, a, a, a, b], (a, a, b))


def test_state_packing_and_the_device_table():
    assert cbr.pack(0b101, 2, 3) == 0b101 | (3 << 4) | (3 << 8) and cbr.unpack(cbr.pack(0b101, 2, 3)) == (0b101, 2, 3)
    t = cbr.table([[(8, 9), (7,)], None, []])
    assert t.shape == (3, 4, 4) and t.dtype == np.int32
    assert t[0].tolist() == [[8, 9, -1, -1], [7, -1, -1, -1], [-1] * 4, [-1] * 4] and np.all(t[1:] == -1)
    got = ops.check_constraints([[[(8, 9), (7,)], None, []]], [3], [20], 12)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), t)


# ------------------------------------------------------------------------------------------------ the allocation
def _sel(p, W, cons, pos=0, cum=None, state=None, fin=None, length=None, hist=None, row_c=None, row_x=None, **ctl):
    p = np.asarray(p, np.float32)
    R, C = p.shape
    if cum is None:
        cum = np.zeros((R // W, W), np.float32); cum[:, 1:] = -np.inf
        cum = cum.reshape(-1)
    state = np.zeros(R, np.int64) if state is None else np.asarray(state)
    fin = np.zeros(R, bool) if fin is None else np.asarray(fin, bool)
    length = np.zeros(R, np.int64) if length is None else np.asarray(length, np.int64)
    if hist is None:
        hist = np.full((R, pos + 1), 4, np.int64)
        hist[:, 0] = BOS
    return cbr.select_cons(p, [C] * R if row_c is None else row_c, [0] * R if row_x is None else row_x, W, False, cum, state, fin, length,
                           np.asarray(hist).reshape(R, -1), pos, cons, **ctl)


def _anchor_rows(n=2):
    p = np.full((n, 8), 0.01, np.float32)
    p[:, A], p[:, B_], p[:, C_] = 0.5, 0.3, 0.05
    return p


def test_anchor_allocation():
    p = _anchor_rows()
    par, ext, mod, cum, st, fin, ln = _sel(p, 2, [[(C_,)]])
    assert par.tolist() == [0, 0] and ext.tolist() == [C_, A] and mod.tolist() == [C_, A]
    assert cum.tolist() == [_ln(0.05), _ln(0.5)] and st.tolist() == [1, 0] and ln.tolist() == [1, 1] and not fin.any()
    # the next step: EOS best everywhere; it is a candidate of row 0 only.  Bank 1: row 0's EOS (ln 0.05 + ln 0.9 = −3.10), its a and row
    # 1's forced c (both −3.69); bank 0: row 1's a (ln 0.5 + ln 0.5 = −1.39) and b — row 1 may not end, so it takes a
    p2 = _anchor_rows()
    p2[:, EOS] = 0.9
    hist = np.array([[BOS, C_], [BOS, A]], np.int64)
    par, ext, mod, cum2, st2, fin2, ln2 = _sel(p2, 2, [[(C_,)]], pos=1, cum=cum, state=st, hist=hist)
    assert par.tolist() == [0, 1] and ext.tolist() == [EOS, A] and fin2.tolist() == [True, False] and st2.tolist() == [1, 0]
    assert cum2[0] == np.float32(cum[0] + _ln(0.9)) and cum2[1] == np.float32(cum[1] + _ln(0.5))
    # W = 3 shows the order go on: bank 1's best, bank 0's best, then bank 1's second (row 0's a or row 1's c, whose sums differ in
    # rounding at most)
    p3, c3, s3 = _anchor_rows(3), np.array([cum[0], cum[1], NEG], np.float32), np.array([1, 0, 0])
    p3[:, EOS] = 0.9
    _, ext3, _, _, st3, _, _ = _sel(p3, 3, [[(C_,)]], pos=1, cum=c3, state=s3, hist=np.array([[BOS, C_], [BOS, A], [BOS, A]], np.int64))
    assert ext3[:2].tolist() == [EOS, A] and st3.tolist() == [1, 0, 1] and ext3[2] in (A, C_)
    # without the constraint the same rows pick a and b, and EOS for both at the next step
    par, ext, *_ = _sel(p, 2, [None])
    assert ext.tolist() == [A, B_]
    _, ext, *_ = _sel(p2, 2, [None], pos=1, cum=[-1.0, -1.0], hist=hist)
    assert ext.tolist() == [EOS, EOS]


def _random_tables(rng, T, W, pos, logits, C_hi=40):
    R = T * W
    Cs = np.repeat(rng.integers(UNK + 6, C_hi, size=T), W)
    s = (rng.choice(np.array([0.0, 0.1, 0.2, 0.4], np.float32), size=(R, int(Cs.max()))) if rng.random() < 0.5
         else rng.random((R, int(Cs.max()))).astype(np.float32))
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


def _bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("ctl", range(len(CTLS)))
def test_no_constraints_equals_select_ctl(ctl, logits):
    c = dict(CTLS[ctl])
    lp = length_table(c.pop("length_penalty_name", "none"), c.pop("length_penalty_alpha", 0.0), 12)
    rng = np.random.default_rng(ctl * 2 + logits)
    for W in (1, 3, 4):
        s, Cs, Xs, cum, fin, length, hist = _random_tables(rng, 6, W, 4, logits)
        state = np.zeros(6 * W, np.int64)
        for _ in range(2):                          # step for step: the second step starts from the first's result
            ref = bcr.select_ctl(s, Cs, Xs, W, logits, cum, fin, length, hist, 4, lp=lp, **c)
            got = cbr.select_cons(s, Cs, Xs, W, logits, cum, state, fin, length, hist, 4, [None] * 6, lp=lp, **c)
            for a, b in zip(ref, got[:4] + got[5:]):
                np.testing.assert_array_equal(_bits(a), _bits(b))
            assert not got[4].any()
            cum, fin, length = got[3], got[5], got[6]
            hist = hist[ref[0]]
            hist[:, 4] = np.where(ref[1] == PAD, 9, ref[1])


def test_candidate_rules():
    # a forced column that is also in the top-W appears once: W = 2, constraint (a,): rows a (bank 1), b (bank 0) — not a twice
    p = _anchor_rows()
    par, ext, _, cum, st, _, _ = _sel(p, 2, [[(A,)]])
    assert ext.tolist() == [A, B_] and st.tolist() == [1, 0] and cum.tolist() == [_ln(0.5), _ln(0.3)]
    # two unmet phrases with one first id force one column
    par, ext, _, _, st, _, _ = _sel(p, 2, [[(C_,), (C_, A)]])
    assert ext.tolist() == [C_, A] and st.tolist() == [1, 0]
    # a banned forced column is not added: unigram blocking, c already in the history
    hist = np.array([[BOS, C_], [BOS, C_]], np.int64)
    _, ext, *_ = _sel(p, 2, [[(C_,)]], pos=1, cum=[0.0, NEG], hist=hist, block_ngram_repeat=1)
    assert ext.tolist() == [A, B_]
    _, ext, *_ = _sel(p, 2, [[(C_,)]], pos=1, cum=[0.0, NEG], hist=hist)
    assert ext.tolist() == [C_, A]
    # … unless one of the gram's tokens is excluded from blocking
    _, ext, *_ = _sel(p, 2, [[(C_,)]], pos=1, cum=[0.0, NEG], hist=hist, block_ngram_repeat=1, exclusion_tokens=(C_,))
    assert ext.tolist() == [C_, A]
    # a forced column >= C_r, or UNK, is not added
    _, ext, _, _, st, _, _ = _sel(p, 2, [[(8,)]])
    assert ext.tolist() == [A, B_] and st.tolist() == [0, 0]
    _, ext, _, _, st, _, _ = _sel(p, 2, [[(UNK,)]])
    assert ext.tolist() == [A, B_] and st.tolist() == [0, 0]
    # a forced column with zero probability is not added (its child would be dead)
    p0 = _anchor_rows()
    p0[:, C_] = 0.0
    _, ext, _, cum, st, _, _ = _sel(p0, 2, [[(C_,)]])
    assert ext.tolist() == [A, B_] and st.tolist() == [0, 0] and np.all(np.isfinite(cum))
    # a forced column in the copied-word range: extended id kept, model id UNK
    _, ext, mod, _, st, _, _ = _sel(p, 2, [[(7,)]], row_x=[1, 1])
    assert ext.tolist() == [7, A] and mod.tolist() == [UNK, A] and st.tolist() == [1, 0]
    # a phrase in progress forces its continuation only
    _, ext, _, _, st, _, _ = _sel(p, 2, [[(B_, C_), (B_,)]], pos=1, cum=[-1.0, NEG], state=[cbr.pack(0, 0, 1), 0])
    assert ext.tolist() == [C_, B_] and cbr.unpack(st[0]) == (0b01, -1, 0)
    assert cbr.unpack(st[1]) == (0, 0, 1)           # (b is not the continuation: the progress is dropped and the LOWEST unmet phrase starting with b starts)


def test_dead_candidates_never_precede_a_live_one():
    # W = 3, position 0: rows 1 and 2 start at −inf — their dead candidates (key −inf in every bank) take no slot from the live parent's
    p = _anchor_rows(3)
    par, ext, _, cum, st, _, _ = _sel(p, 3, [[(C_,)]])
    assert par.tolist() == [0, 0, 0] and ext.tolist() == [C_, A, B_] and np.all(np.isfinite(cum))
    # a dead parent's child that would sit in a higher bank still comes after every live candidate
    p1 = np.full((2, 8), 0.0, np.float32)
    p1[0, A] = 0.5                                   # the live parent has ONE candidate of positive probability; its other columns are dead
    p1[1] = _anchor_rows(1)[0]
    par, ext, _, cum, st, _, _ = _sel(p1, 2, [[(C_,)]], pos=1, cum=[-1.0, NEG], hist=[[BOS, 4], [BOS, 4]])
    assert par[0] == 0 and ext[0] == A and st[0] == 0 and cum[0] == np.float32(-1.0) + _ln(0.5) and cum[1] == NEG
    assert par[1] == 1 and ext[1] == A               # (among the dead — every key −inf — the raw value decides: row 1's a, 0.5)
    rng = np.random.default_rng(3)
    for _ in range(30):
        s, Cs, Xs, cum, fin, length, hist = _random_tables(rng, 4, 4, 4, False)
        cons = [[(7, 8), (9,)], None, [(10,)], [(7,), (7,), (8, 9, 10)]]
        out = cbr.select_cons(s, Cs, Xs, 4, False, cum, np.zeros(16), fin, length, hist, 4, cons)
        live = np.isfinite(out[3]).reshape(4, 4)
        assert all(not (live[t, k + 1] and not live[t, k]) for t in range(4) for k in range(3))


def test_a_finished_parent_sits_in_the_bank_of_its_own_state():
    # W = 2: row 0 finished with the constraint met (bank 1), row 1 live and unmet.  Bank 1: the finished parent and row 1's forced child;
    # bank 0: row 1's top columns.  Order: bank 1 rank 0, bank 0 rank 0 → the better of bank 1 first
    p = _anchor_rows()
    par, ext, _, cum, st, fin, ln = _sel(p, 2, [[(C_,)]], pos=2, cum=[-9.0, -1.0], state=[1, 0], fin=[True, False], length=[2, 0])
    assert par.tolist() == [1, 1] and ext.tolist() == [C_, A] and st.tolist() == [1, 0]      # −1 + ln 0.05 = −4.0 beats −9 inside bank 1
    par, ext, _, cum, st, fin, ln = _sel(p, 2, [[(C_,)]], pos=2, cum=[-2.0, -1.0], state=[1, 0], fin=[True, False], length=[2, 0])
    assert par.tolist() == [0, 1] and ext.tolist() == [PAD, A] and st.tolist() == [1, 0] and fin.tolist() == [True, False]
    assert cum[0] == np.float32(-2.0) and ln.tolist() == [2, 3]
    # unmet and finished (it ended before the rule applied, or was given): bank 0, it competes with the top columns there
    par, ext, _, cum, st, fin, ln = _sel(p, 2, [[(C_,)]], pos=2, cum=[-0.1, -1.0], state=[0, 0], fin=[True, False], length=[2, 0])
    assert par.tolist() == [1, 0] and ext.tolist() == [C_, PAD] and st.tolist() == [1, 0]


def test_fill_rows():
    # rows of ONE column that unigram blocking bans: no candidate at all → fill rows with state 0
    p = np.full((2, 1), 0.5, np.float32)
    hist = np.array([[BOS, 0], [BOS, 0]], np.int64)
    par, ext, mod, cum, st, fin, ln = cbr.select_cons(p, [1, 1], [0, 0], 2, False, [-1.0, -2.0], [1, 1], [False, False], [0, 0], hist, 1,
                                                      [[(0,)]], block_ngram_repeat=1)
    assert par.tolist() == [0, 1] and ext.tolist() == [PAD, PAD] and mod.tolist() == [PAD, PAD] and st.tolist() == [0, 0]
    assert np.all(cum == NEG) and fin.all() and ln.tolist() == [2, 2]
    # one candidate, W = 2: the second row is a fill row
    hist[0, 1] = 7
    par, ext, _, cum, st, fin, ln = cbr.select_cons(p, [1, 1], [0, 0], 2, False, [-1.0, -2.0], [0, 1], [False, False], [0, 0], hist, 1,
                                                    [[(0,)]], block_ngram_repeat=1)
    assert par.tolist() == [0, 1] and ext.tolist() == [0, PAD] and st.tolist() == [1, 0] and fin.tolist() == [False, True]


def test_final_order():
    lp = length_table("avg", 0.0, 12)
    # popcount beats the key; −inf last whatever its state; equal popcount: the key, then the index
    cum = np.array([-1.0, -8.0, -np.inf, -3.0, -3.0], np.float32)
    state = [0b0001, 0b0011, 0b0111, 0b0100, cbr.pack(0b1000, 1, 2)]
    order, keys = cbr.final_order_cons(cum, [2, 4, 3, 3, 3], state, None)
    assert order == [1, 0, 3, 4, 2]
    order, keys = cbr.final_order_cons(cum, [2, 4, 3, 3, 1], state, lp)
    assert order == [1, 0, 3, 4, 2] and keys[4] == -3.0 and keys[3] == -1.0
    order, _ = cbr.final_order_cons(cum, [2, 4, 3, 1, 3], state, lp)
    assert order == [1, 0, 4, 3, 2]
    # all states equal: the n-best order
    order, _ = cbr.final_order_cons(cum, [2, 4, 3, 3, 3], [3] * 5, lp)
    assert order == bcr.final_order(cum, [2, 4, 3, 3, 3], lp)[0]


@pytest.mark.parametrize("W", [1, 2, 4])
def test_row_zero_meets_every_constraint(W):
    """the satisfaction property: Σ len ≤ Lt − 2, no control bans the phrase words, positive probabilities → row 0 of every sentence ends
    with the full mask and holds every phrase as a contiguous run"""
    Lt, T, C = 12, 4, 30
    rng = np.random.default_rng(W)
    cons = [[(7, 8, 9, 10), (11, 12, 13, 14), (15,), (16,)], [(20, 21), (20,)], None, [(9,), (9,), (9, 9, 9)]]
    R = T * W
    cum = np.zeros((T, W), np.float32); cum[:, 1:] = -np.inf
    cum, state, fin, length = cum.reshape(-1), np.zeros(R, np.int64), np.zeros(R, bool), np.zeros(R, np.int64)
    hist = np.full((R, Lt), PAD, np.int64); hist[:, 0] = BOS
    for i in range(Lt - 1):
        s = (rng.random((R, C)) * 0.9 + 0.001).astype(np.float32)
        s[:, EOS] = 0.95                            # EOS is every row's best column from the first step on
        par, ext, _, cum, state, fin, length = cbr.select_cons(s, [C] * R, [0] * R, W, False, cum, state, fin, length, hist, i, cons,
                                                               min_length=2, lp=length_table("wu", 0.7, Lt))
        hist = hist[par]
        hist[:, i + 1] = ext
    for t in range(T):
        r = t * W
        assert cbr.unpack(state[r])[0] == (1 << len(cons[t] or ())) - 1, (t, state[r])
        ids = hist[r].tolist()
        if t != 3:                                  # (sentence 3's phrases overlap: the run test is for distinct phrases)
            assert all(cbr.contains(ids, ph) for ph in cons[t] or ())
        assert ids.count(9) >= (5 if t == 3 else 0)
    if W == 1:                                      # (one row: it ends as soon as it may)
        assert fin.all() and length.tolist() == [11, 4, 3, 6]


# ------------------------------------------------------------------------------------------------ host-side checks
GOOD = [[[(7, 8), (9,)], None], [[]]]


@pytest.mark.parametrize("bad", [
    None, 5, "ab", [[None, None]], [[None, None], [None], [None]],                                    # nesting, video count
    [[None], [None]], [[None, None, None], [None]], [[None, 7], [None]], [[[7], None], [None]],       # sentence count, a phrase that is an id
    [[[(7,)] * 5, None], [None]],                                                                     # more than 4 phrases
    [[[()], None], [None]], [[[(7, 8, 9, 10, 11)], None], [None]],                                    # empty / longer than 4
    [[[(PAD,)], None], [None]], [[[(7, BOS)], None], [None]], [[[(EOS,)], None], [None]], [[[(UNK,)], None], [None]],
    [[[(20,)], None], [None]], [[[(-1,)], None], [None]], [[None, None], [[(22,)]]], [[[(7.5,)], None], [None]], [[[(True,)], None], [None]],
    [[[(7, 8, 9, 10), (7, 8, 9, 10), (7, 8, 9)], None], [None]],                                      # Σ len = 11 > Lt − 2 = 10
])
def test_check_constraints_refuses(bad):
    with pytest.raises(ValueError):
        ops.check_constraints(bad, [2, 1], [20, 22], 12)


def test_check_constraints_accepts():
    t = ops.check_constraints(GOOD, [2, 1], [20, 22], 12)
    assert tuple(t.shape) == (3, ops.CONS_MAX, ops.CONS_LEN) and t.dtype == torch.int32 and not t.is_cuda
    assert t[0].tolist() == [[7, 8, -1, -1], [9, -1, -1, -1], [-1] * 4, [-1] * 4] and bool((t[1:] == -1).all())
    t = ops.check_constraints([[None, None], [[(21,), [7, 8, 9, 10], torch.tensor([7, 8]), np.array([9, 9, 9])]]], [2, 1], [20, 22], 12)
    assert t[2].tolist() == [[21, -1, -1, -1], [7, 8, 9, 10], [7, 8, -1, -1], [9, 9, 9, -1]]          # Σ len = 10 = Lt − 2
    assert ops.CONS_MAX == 4 and ops.CONS_LEN == 4


class _Opt(object):
    cuda = True


def _translator(**opt):
    from svpc_amd.translator import Translator
    tr = Translator.__new__(Translator)
    tr.incremental = True
    tr.opt = _Opt()
    for k, v in opt.items():
        setattr(tr.opt, k, v)
    tr.model_config = types.SimpleNamespace(max_t_len=22, vocab_size=951, model_mode="full")
    return tr


def test_translator_refuses_before_device_work():
    inputs = [None] * 12
    tr = _translator()
    with pytest.raises(ValueError, match="paragraph"):
        tr.translate_batch_constrained(inputs, [], 4, block_ngram_repeat=2, block_ngram_scope="paragraph")
    for bad in (dict(beam_size=9), dict(beam_size=4, n_best=5), dict(beam_size=4, min_length=22)):
        with pytest.raises(ValueError):
            tr.translate_batch_constrained(inputs, [], **bad)
    with pytest.raises(TypeError):
        tr.translate_batch_constrained(inputs, [], 4, no_repeat_ngram_size=3)
    inputs[8], inputs[11] = [{"zest": 951}, {}], [2, 1]
    for bad in ([[None, None]], [[[(952,)], None], [None]], [[None, None], [[(951,)]]], [[[(EOS,)], None], [None]]):
        with pytest.raises(ValueError):
            tr.translate_batch_constrained(inputs, bad, 4)
    tr.incremental = False
    with pytest.raises(NotImplementedError):
        tr.translate_batch_constrained(inputs, [], 4)


def test_constraint_ids():
    from svpc_amd.translator import Translator
    w2i = {"olive": 30, "oil": 31, "salt": 32, "zest": 40}
    oov = {"zest": 951, "yuzu": 952}
    assert Translator.constraint_ids([["olive", "oil"], ["salt"]], w2i, oov) == [[30, 31], [32]]
    assert Translator.constraint_ids(["olive oil", "yuzu zest"], w2i, oov) == [[30, 31], [952, 951]]      # a copied word takes its copied id
    assert Translator.constraint_ids([], w2i, oov) == [] and Translator.constraint_ids(None, w2i, None) == []
    assert Translator.constraint_ids([["zest"]], w2i, {}) == [[40]]
    with pytest.raises(ValueError, match="saffron"):
        Translator.constraint_ids([["saffron"]], w2i, oov)


def test_the_decode_key_has_a_flag_only():
    from svpc_amd.translator import BEAM, Decode
    plain = Decode(BEAM, 4, n_best=4)
    a = Decode(BEAM, 4, n_best=4, cons=ops.check_constraints(GOOD, [2, 1], [20, 22], 12))
    b = Decode(BEAM, 4, n_best=2, cons=ops.check_constraints([[None, None], [None]], [2, 1], [20, 22], 12))
    assert a.key == b.key and a.key != plain.key and a.constrained and not plain.constrained
    assert plain.key == (BEAM, 4, None, True, None)            # (the plain decode's key is what it was)


def test_no_cpu_fallback():
    from svpc_amd import _lib
    R, lt, W = 4, 8, 2
    scores = torch.rand(R, 20)
    cum = torch.zeros(R)
    fin, length, cstate = (torch.zeros(R, dtype=torch.int32) for _ in range(3))
    toks = [[torch.zeros(R, lt, dtype=torch.int32) for _ in range(3)] for _ in range(2)]
    cons = torch.full((R // W, 4, 4), -1, dtype=torch.int32)
    with pytest.raises(_lib.SvpcKernelError):
        ops.beam_step_cons(scores, [20] * R, [0] * R, W, 3, False, UNK, EOS, PAD, cum, cstate, fin, length, toks[0], toks[1], lt, cons)
    with pytest.raises(_lib.SvpcKernelError):
        ops.beam_finalize_cons(cum, toks[0][1], W, W, cstate, length)
    for bad in (dict(cons=cons[:1]), dict(cons=cons.long()), dict(cons=cons[:, :3]), dict(cstate=cstate.long()), dict(cstate=cstate[:2]),
                dict(length=None), dict(lp=torch.ones(3, dtype=torch.float64)), dict(min_length=8)):
        kw = dict(cons=cons, cstate=cstate, length=length)
        extra = {k: bad[k] for k in bad if k not in kw}
        kw.update({k: bad[k] for k in bad if k in kw})
        with pytest.raises(ValueError):
            ops.beam_step_cons(scores, [20] * R, [0] * R, W, 3, False, UNK, EOS, PAD, cum, kw["cstate"], fin, kw["length"], toks[0], toks[1],
                               lt, kw["cons"], **extra)
    for bad in (dict(cstate=cstate.long()), dict(cstate=cstate[:2]), dict(n_best=3), dict(lp=torch.ones(3, dtype=torch.float64))):
        kw = dict(cstate=cstate, n_best=W, lp=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.beam_finalize_cons(cum, toks[0][1], W, kw["n_best"], kw["cstate"], length, kw["lp"])


def test_library_exports_the_constrained_entry_points():
    from svpc_amd import _lib
    decl = _lib.declarations()
    assert "svpc_beam_step_cons" in decl and "svpc_beam_finalize_cons" in decl
    assert len(decl["svpc_beam_step_cons"][1]) == len(decl["svpc_beam_step_ctl"][1]) + 2
    assert len(decl["svpc_beam_finalize_cons"][1]) == len(decl["svpc_beam_finalize_nbest"][1]) + 2
    lib = _lib.load()
    assert lib.svpc_abi_version() == 2
    assert hasattr(lib, "svpc_beam_step_cons") and hasattr(lib, "svpc_beam_finalize_cons")
