"""The tail of a training step's backward pass: scheduling of the parameter-gradient kernels whose results nobody reads before the
optimizer (or the gradient all-reduce) — grouped weight gradients, bias column sums, reduction finalizers — and the join at the end of
backward.  Everything here launches on the current stream; the work is only *deferred*, so that ≈150 launches of 5–15 µs become a handful.

Four queues, flushed in this order at every join point (``flush_pending``: end of backward through an autograd callback, before a
gradient bucket is all-reduced, before the optimizer kernels):

  bf16 wgrads   dW += dzᵀ·x of the bf16-stream linears, one launch without split-K (their bias gradients ride along, or become column sums)
  fp32 wgrads   the same for fp32-storage linears, also flushed at ``GROUP_FLUSH_AT`` entries
  column sums   first stage of Σ_rows dz for bias gradients (into per-chunk partials), also flushed at 48 entries
  finalizers    out0 / out1 += column sums of a (groups × ncols) partial: the second stage of the above and of every LayerNorm-like tail

A queue is flushed before an entry is added whose target is already pending in it: two accumulations into one gradient stay ordered.
Every arena gradient that has been written is reported to ``GRAD_READY_HOOK`` (the data-parallel reducer counts these reports).

The backward functions of ``ops`` reach the queues through two routing helpers, ``bias_grad`` and ``defer_partials``.  Known asymmetry,
kept as it is: when ``defer_partials`` declines (not every target is an arena gradient), the eager fallbacks of ``_CrossAttnLn``,
``_PtrAttnGate`` and ``_SimHeads`` ``add_`` into the arena targets they do have WITHOUT reporting them ready, unlike every other
in-place write of an arena gradient (``_LayerNorm``'s fallback writes no arena target: it hands autograd two fresh tensors).

What this module needs from ``ops`` (``_ws``, ``_stream``, ``_dt``, ``_fast``, ``_colsum``, ``USE_P8W``, ``BWD_EXACT``, ``_RES_SINK``) it reads
through ``_ops()`` at call time, so a switch set on ``ops`` after import (tests/tools/bwd_ablation.py) is honoured.
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib

USE_GROUPED_WGRAD = os.environ.get("SVPC_NO_GROUPED_WGRAD", "") == ""
GROUP_BF16 = os.environ.get("SVPC_NO_GROUP_BF16", "") == ""      # also the bf16-stream wgrads (one launch, no split-K)
GROUP_FLUSH_AT = int(os.environ.get("SVPC_GROUP_FLUSH_AT", "16"))
# packed Q/K/V (432 tiles of 64²) and LSTM (576) weight gradients over K = 192 rows are pure latency as launches of their own
GROUP_MAX_TILES = int(os.environ.get("SVPC_GROUP_MAX_TILES", "1200"))
COLSUM_FLUSH_AT = 48

# ---- state: all of it
_WQ16 = []                 # pending bf16-stream wgrads (dz, x, wgrad, bgrad or None)
_WQ = []                   # pending fp32 wgrads (dz, x, wgrad, bgrad or None)
_CQ = []                   # pending first stages of bias-gradient column sums (x, partial)
_FQ = []                   # pending finalizers (partial, out0, out1 or None, groups, ncols, split)
_JOIN_QUEUED = [False]     # join_side is queued as the running backward pass's final callback
GRAD_READY_HOOK = None     # set by GradReducer: called with (data_ptr, numel, kind) of every arena gradient that has just been written
HOOKS_PAUSED = [0]         # > 0: gradient-ready notifications (pointer reports here, the reducer's post-accumulate hooks) are ignored
_OPS = []
# ----


def _ops():
    if not _OPS:
        from . import ops
        _OPS.append(ops)
    return _OPS[0]


class _WgradProblem(ctypes.Structure):
    _fields_ = [("dz", ctypes.c_void_p), ("x", ctypes.c_void_p), ("dw", ctypes.c_void_p), ("db", ctypes.c_void_p),
                ("n_out", ctypes.c_int), ("n_in", ctypes.c_int), ("rows", ctypes.c_int), ("ld_dz", ctypes.c_int),
                ("ld_x", ctypes.c_int), ("ld_dw", ctypes.c_int)]


class _FinalizeEntry(ctypes.Structure):
    _fields_ = [("partial", ctypes.c_void_p), ("out0", ctypes.c_void_p), ("out1", ctypes.c_void_p), ("groups", ctypes.c_int),
                ("ncols", ctypes.c_int), ("split", ctypes.c_int)]


class _ColsumEntry(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("partial", ctypes.c_void_p), ("dt", ctypes.c_int), ("ldx", ctypes.c_int), ("R", ctypes.c_int),
                ("C", ctypes.c_int)]


class hooks_paused:
    """``with ops.hooks_paused():`` — while a part of the step is warmed up / captured into a hipGraph (svpc_amd/clip_graphs.py) the
    data-parallel reducer must not count the parameter writes of that pass (nor issue a collective from inside a capture)."""

    def __enter__(self):
        HOOKS_PAUSED[0] += 1
        return self

    def __exit__(self, *exc):
        HOOKS_PAUSED[0] -= 1
        return False


def _ready(t, kind=None):
    if GRAD_READY_HOOK is not None and t is not None and not HOOKS_PAUSED[0]:
        GRAD_READY_HOOK(t.data_ptr(), t.numel(), kind)


def _queue_end_of_backward_join():
    if not _JOIN_QUEUED[0]:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(join_side)
            _JOIN_QUEUED[0] = True
        except RuntimeError:      # not inside a backward pass: the caller joins (optimizer / reducer do)
            pass


# ------------------------------------------------------------------------------------------------ grouped weight gradients
def _defer_wgrad16(dz, x, wgrad, bgrad=None):
    rows, n_out = dz.shape
    n_in = x.shape[1]
    if n_out % 8 or n_in % 8 or dz.stride(0) % 8 or x.stride(0) % 8 or wgrad.stride(0) % 4 or rows < 1:
        return False
    if (dz.data_ptr() | x.data_ptr()) % 16 or dz.stride(1) != 1 or x.stride(1) != 1 or not wgrad.is_contiguous():
        return False
    wp = wgrad.data_ptr()
    bp = bgrad.data_ptr() if bgrad is not None else -1
    if any(q[2].data_ptr() == wp or (q[3] is not None and q[3].data_ptr() == bp) for q in _WQ16) or \
            len(_WQ16) >= _lib.load().svpc_gemm_group_wgrad_max():
        flush_wgrads()
    _WQ16.append((dz, x, wgrad, bgrad))
    _queue_end_of_backward_join()
    return True


def defer_wgrad(dz, x, wgrad, bgrad):
    """Queue dW += dzᵀ·x (and db += Σ dz) for the grouped launch; False if this problem must be launched on its own."""
    o = _ops()
    if USE_GROUPED_WGRAD and GROUP_BF16 and o._fast() and wgrad is not None and dz.dtype == torch.bfloat16 and x.dtype == torch.bfloat16:
        return _defer_wgrad16(dz, x, wgrad, bgrad)
    if not (USE_GROUPED_WGRAD and o._fast() and wgrad is not None and dz.dtype == torch.float32 and x.dtype == torch.float32) or o.BWD_EXACT:
        return False
    rows, n_out = dz.shape
    n_in = x.shape[1]
    if rows < 1 or n_out % 4 or n_in % 4 or dz.stride(0) % 4 or x.stride(0) % 4 or wgrad.stride(0) % 4:      # any row count: k tail zero-sourced
        return False
    if (dz.data_ptr() | x.data_ptr()) % 16 or dz.stride(1) != 1 or x.stride(1) != 1 or not wgrad.is_contiguous():
        return False
    tiles = -(-n_out // 64) * -(-n_in // 64)
    if tiles > GROUP_MAX_TILES:   # a grid of its own fills the chip for long enough: nothing to gain from grouping
        return False
    wp = wgrad.data_ptr()
    if any(q[2].data_ptr() == wp for q in _WQ):
        flush_wgrads(bf16=False)  # two accumulations into one gradient stay ordered
    _WQ.append((dz, x, wgrad, bgrad))
    if len(_WQ) >= min(GROUP_FLUSH_AT, _lib.load().svpc_gemm_group_wgrad_max()):
        flush_wgrads(bf16=False)
    _queue_end_of_backward_join()
    return True


def _problem_table(queue):
    probs = (_WgradProblem * len(queue))()
    for i, (dz, x, wg, bg) in enumerate(queue):
        probs[i] = _WgradProblem(dz.data_ptr(), x.data_ptr(), wg.data_ptr(), bg.data_ptr() if bg is not None else None, dz.shape[1],
                                 x.shape[1], dz.shape[0], dz.stride(0), x.stride(0), wg.stride(0))
    return probs


def flush_wgrads(bf16=True):
    o = _ops()
    if _WQ16 and bf16:
        probs = _problem_table(_WQ16)
        ws = o._ws(_WQ16[0][0].device)
        # the 8-phase template with transposed fragment reads when every problem is at least 256 wide (gemm_p8w.hip: it also takes the
        # bias gradients from the dz tiles it stages), else the round-1 form with the column sums as a pass of their own
        p8w = o.USE_P8W and _lib.load().svpc_gemm_group_wgrad_bf16_p8_ok(ctypes.addressof(probs), len(_WQ16)) == 1
        done = list(_WQ16)
        del _WQ16[:]
        if not p8w:
            for i, (dz, x, wg, bg) in enumerate(done):
                if bg is not None:
                    probs[i].db = None
                    defer_colsum(dz, bg)
        _lib.call("gemm_group_wgrad_bf16_p8" if p8w else "gemm_group_wgrad_bf16_ws", ctypes.addressof(probs), len(done),
                  ws.data_ptr(), ws.numel() * 4, o._stream())
        for _, _, wg, bg in done:
            _ready(wg, "w")
            if bg is not None and p8w:
                _ready(bg, "b")
    if not _WQ:
        return
    probs = _problem_table(_WQ)
    _lib.call("gemm_group_wgrad", ctypes.addressof(probs), len(_WQ), o._stream())
    done = list(_WQ)
    del _WQ[:]
    for _, _, wg, bg in done:
        _ready(wg, "w")
        if bg is not None:
            _ready(bg, "b")


# ------------------------------------------------------------------------------------------------ column sums and finalizers
def defer_finalize(partial, groups, ncols, out0, out1=None, split=None):
    """out0/out1 (+)= column sums of ``partial`` (groups × ncols), later, together with every other pending tail"""
    tgt = (out0.data_ptr(), out1.data_ptr() if out1 is not None else 0)
    if any(q[1].data_ptr() in tgt or (q[2] is not None and q[2].data_ptr() in tgt) for q in _FQ):
        flush_finalizes()
    _FQ.append((partial, out0, out1, int(groups), int(ncols), int(ncols if split is None else split)))
    if len(_FQ) >= _lib.load().svpc_multi_finalize_max():
        flush_finalizes()
    _queue_end_of_backward_join()


def defer_colsum(x, out):
    """out += Σ_rows x, both stages deferred: the column sums of all pending tensors run as one launch, then the finalizes"""
    R, C = x.shape
    chunks = _lib.load().svpc_colsum_chunks(R)
    partial = torch.empty(chunks * C, dtype=torch.float32, device=x.device)
    if len(_CQ) >= COLSUM_FLUSH_AT:
        flush_finalizes()
    _CQ.append((x, partial))
    defer_finalize(partial, chunks, C, out)


def _flush_colsums():
    if not _CQ:
        return
    o = _ops()
    ents = (_ColsumEntry * len(_CQ))()
    for i, (x, partial) in enumerate(_CQ):
        ents[i] = _ColsumEntry(x.data_ptr(), partial.data_ptr(), o._dt(x), x.stride(0), x.shape[0], x.shape[1])
    _lib.call("multi_colsum", ctypes.addressof(ents), len(_CQ), o._stream())
    del _CQ[:]


def flush_finalizes():
    _flush_colsums()
    if not _FQ:
        return
    ents = (_FinalizeEntry * len(_FQ))()
    for i, (partial, o0, o1, g, nc, sp) in enumerate(_FQ):
        ents[i] = _FinalizeEntry(partial.data_ptr(), o0.data_ptr(), (o1 if o1 is not None else o0).data_ptr(), g, nc, sp)
    _lib.call("multi_finalize", ctypes.addressof(ents), len(_FQ), _ops()._stream())
    done = list(_FQ)
    del _FQ[:]
    for _, o0, o1, _, _, _ in done:
        _ready(o0, "b" if o1 is None else None)
        if o1 is not None:
            _ready(o1)


# ------------------------------------------------------------------------------------------------ routing helpers of the backward functions
def bias_grad(dz, target):
    """target (an arena vector) += Σ_rows dz: deferred when the grouped column sum takes dz's layout, else launched now"""
    M, N = dz.shape
    V = 8 if dz.dtype == torch.bfloat16 else 4
    if N % V == 0 and dz.stride(0) % V == 0 and dz.data_ptr() % 16 == 0 and M > 0:
        defer_colsum(dz, target)
    else:
        _ops()._colsum(dz, out=target.view(1, -1), accumulate=1)
        _ready(target, "b")


def defer_partials(partial, groups, ncols, out0, out1, split):
    """Per-group partials (groups × ncols) whose column sums go to two arena gradients (columns [0, split) to out0, the rest to out1):
    queued when both targets are arena gradients; False otherwise — the caller then reduces ``partial`` its own way, now."""
    if out0 is None or out1 is None:
        return False
    defer_finalize(partial, groups, ncols, out0, out1, split)
    return True


# ------------------------------------------------------------------------------------------------ join points
def flush_pending():
    """Launch every queued gradient tail (grouped wgrads, column sums, finalizers) on the current stream.  Safe at any point of a
    backward pass: parked residual gradients (``ops._RES_SINK``) are left alone — LayerNorm backwards legitimately keep one parked
    until the consuming projection's dgrad runs."""
    flush_wgrads()
    flush_finalizes()


def join_side():
    """End of a backward pass (autograd callback) / before the optimizer kernels: ``flush_pending`` + the leftover check of the
    residual-gradient hand-over.  NOT for use in the middle of backward (a gradient bucket released by a hook calls
    ``flush_pending``): a parked gradient is normal there.  (The name dates from when gradient kernels ran on side streams that were
    joined here; there is no other stream to wait for any more.)"""
    flush_pending()
    _JOIN_QUEUED[0] = False
    sink = _ops()._RES_SINK
    if sink:
        n_left = len(sink)
        sink.clear()
        raise _lib.SvpcKernelError("residual-gradient hand-over: %d parked gradient(s) were never absorbed by a projection's dgrad "
                                   "(layernorm(..., sink=True) without a consuming ops.linear)" % n_left)
