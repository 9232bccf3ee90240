"""The host checks the four selection steps share (ops.beam_step, beam_step_groups, beam_step_cons, stochastic_beam_step), without a GPU:
every one refuses the same bad shared arguments with ValueError, and a good call on CPU tensors gets past every check to the library's
door (SvpcKernelError: there is no CPU fallback).  R = 4 rows (T = 2 sentences of W = 2), Lt = 8, C = 20.

The control keywords ``block_ngram_repeat``, ``lp`` and ``exclusion`` are not part of ``stochastic_beam_step``'s signature (passing
them is a TypeError, tests/test_stochastic_beam_host.py), so those three cases run for the three functions that take them; ``min_length``
and everything positional run for all four."""
import pytest
import torch

from svpc_amd import _lib, ops
from svpc_amd.synthetic import EOS, PAD, UNK

R, LT, W, C = 4, 8, 2, 20
STEPS = ("beam_step", "beam_step_groups", "beam_step_cons", "stochastic_beam_step")
WITH_CONTROLS = STEPS[:3]


def _good():
    """the shared arguments of a good call, by name"""
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)      # noqa: E731
    return dict(scores=torch.rand(R, C), row_c=[C] * R, row_x=[0] * R, beam=W, pos=0, cum=torch.zeros(R), finished=i32(R), length=i32(R),
                toks_in=[i32(R, LT) for _ in range(3)], toks_out=[i32(R, LT) for _ in range(3)], slot_rows=LT, kw={})


def _call(fn, a):
    head = (a["scores"], a["row_c"], a["row_x"], a["beam"])
    mid = (a["pos"], False, UNK, EOS, PAD, a["cum"])
    tail = (a["toks_in"], a["toks_out"], a["slot_rows"])
    f64 = lambda: torch.zeros(R, dtype=torch.float64)                  # noqa: E731
    if fn == "beam_step":
        return ops.beam_step(*head, *mid, a["finished"], *tail, length=a["length"], **a["kw"])
    if fn == "beam_step_groups":
        return ops.beam_step_groups(*head, 2, *mid, torch.zeros(R), a["finished"], a["length"], *tail, torch.zeros(W), **a["kw"])
    if fn == "beam_step_cons":
        cons = torch.full((R // W, ops.CONS_MAX, ops.CONS_LEN), -1, dtype=torch.int32)
        return ops.beam_step_cons(*head, *mid, torch.zeros(R, dtype=torch.int32), a["finished"], a["length"], *tail, cons, **a["kw"])
    return ops.stochastic_beam_step(*head, *mid, f64(), f64(), a["finished"], a["length"], *tail, torch.zeros(1, dtype=torch.int64), **a["kw"])


def _strided(a):
    a["scores"] = torch.rand(R, 2 * C)[:, ::2]


def _noncontiguous_table(a):
    a["toks_out"][1] = torch.zeros(R, 2 * LT, dtype=torch.int32)[:, ::2]


def _set(key, value):
    def change(a):
        a[key] = value
    return change


def _kw(**kw):
    def change(a):
        a["kw"] = kw
    return change


def _table_dtype(a):
    a["toks_in"][2] = torch.zeros(R, LT, dtype=torch.int64)


BAD = {
    "beam=0": _set("beam", 0),
    "beam=9": _set("beam", 9),
    "scores-dtype": _set("scores", torch.rand(R, C, dtype=torch.float64)),
    "scores-column-stride": _strided,
    "cum-length": _set("cum", torch.zeros(R + 1)),
    "table-noncontiguous": _noncontiguous_table,
    "table-dtype": _table_dtype,
    "pos=Lt-1": _set("pos", LT - 1),
    "slot_rows<Lt": _set("slot_rows", LT - 1),
    "min_length=Lt": _kw(min_length=LT),
}
BAD_CONTROLS = {
    "block_ngram_repeat=Lt": _kw(block_ngram_repeat=LT),
    "lp-short": _kw(lp=torch.ones(LT - 1, dtype=torch.float64)),
    "exclusion-bits": _kw(exclusion=(torch.zeros(1, dtype=torch.int32), 33)),
}
CASES = [(fn, k, v) for fn in STEPS for k, v in BAD.items()] + [(fn, k, v) for fn in WITH_CONTROLS for k, v in BAD_CONTROLS.items()]


@pytest.mark.parametrize("fn,change", [(fn, v) for fn, _, v in CASES], ids=["%s-%s" % (fn, k) for fn, k, _ in CASES])
def test_shared_bad_argument_raises_value_error(fn, change):
    a = _good()
    change(a)
    with pytest.raises(ValueError):
        _call(fn, a)


@pytest.mark.parametrize("fn", STEPS)
def test_good_call_reaches_the_library(fn):
    with pytest.raises(_lib.SvpcKernelError):
        _call(fn, _good())


@pytest.mark.parametrize("fn", WITH_CONTROLS)
def test_good_controls_reach_the_library(fn):
    a = _good()
    a["kw"] = dict(min_length=LT - 1, block_ngram_repeat=LT - 1, lp=torch.ones(LT, dtype=torch.float64),
                   exclusion=(torch.zeros(1, dtype=torch.int32), 32))
    with pytest.raises(_lib.SvpcKernelError):
        _call(fn, a)
