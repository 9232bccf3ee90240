"""HIP-backed primitives of the hot path: thin ``torch.autograd.Function`` wrappers over the C-ABI
(include/svpc_hip.h).  PyTorch supplies device memory, the current stream and autograd wiring; all arithmetic
runs in the gfx950 kernels of svpc_amd/csrc.  No CPU path exists: tensors must live on the MI355X.

Two groups of bindings have modules of their own and are re-exported here, so that every caller says ``ops.<name>``: the tail of
backward (grad_tail.py) and the sequence losses over the decoder's score matrix with their host checks (seq_loss_ops.py).

The pure-torch statement of every function here (same signatures) lives in tests/emul_ops.py and is what the
GPU tests compare against.
"""
from __future__ import annotations

import ctypes
import math
import numbers
import os
import struct

import torch

from . import _lib
from .ops_common import (ACT_GELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, FIdx, Function, Idx, SeqInfo, _c, _id_rows, _p, _row_vec,  # noqa: F401
                         _TorchFunction, as_idx)
# The tail of backward — deferred parameter-gradient work (grouped weight gradients, bias column sums, reduction finalizers), the
# gradient-ready notifications and the end-of-backward join — lives in grad_tail.py; its public names are re-exported here.
from .grad_tail import (HOOKS_PAUSED, _WgradProblem, _queue_end_of_backward_join, _ready, bias_grad, defer_colsum,  # noqa: F401
                        defer_finalize, defer_partials, defer_wgrad, flush_finalizes, flush_pending, flush_wgrads, hooks_paused, join_side)
# The sequence losses of the training objectives (SCST, unlikelihood, distillation, SimCTG, minimum risk, preference optimisation, clipped
# policy gradient) and their host checks live in seq_loss_ops.py, which reads what it needs from this module at call time.
from .seq_loss_ops import *  # noqa: F401,F403
from .seq_loss_ops import _SeqCl, _SeqKd, _SeqNll, _SeqPg, _SeqPref, _SeqRisk, _SeqUl  # noqa: F401

_WS = {}
_WS_BYTES = 256 << 20


_DEV_IDX = [None]


def _stream():
    """raw handle of PyTorch's current stream on the current device.  (torch.cuda.current_stream() builds a Stream object and
    resolves the device through three Python layers: 9 µs a call, ≈240 calls per eager step — the raw getter is ≈0.3 µs.)"""
    i = _DEV_IDX[0]
    if i is None or not _FAST_STREAM:
        return torch.cuda.current_stream().cuda_stream
    return torch._C._cuda_getCurrentRawStream(i)


_FAST_STREAM = os.environ.get("SVPC_SLOW_STREAM", "") == "" and hasattr(torch._C, "_cuda_getCurrentRawStream")


def _ws(device):
    """One scratch arena per (device, stream) (split-K slabs, reduction partials); ops on a stream use it one at a time."""
    key = (device.index if isinstance(device, torch.device) else str(device), _stream())
    w = _WS.get(key)
    if w is None:
        w = torch.empty(_WS_BYTES // 4, dtype=torch.float32, device=device)
        _WS[key] = w
    return w


P8W_BIAS = os.environ.get("SVPC_NO_P8W_BIAS", "") == ""      # bias gradients of the bf16-stream linears inside the grouped wgrad launch


def _need_gpu(t):
    if not t.is_cuda:
        raise _lib.SvpcKernelError("svpc_amd.ops: tensors must be on the GPU (no CPU fallback exists)")
    _DEV_IDX[0] = t.device.index          # (the device the following launches go to: see _stream)


def _rows2d(t):
    """2-D, unit inner stride (row stride may exceed the width: packed projection outputs are read in place)."""
    assert t.dim() == 2
    if t.stride(1) != 1 and t.shape[1] != 1:
        t = t.contiguous()
    if t.shape[1] == 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t


# ------------------------------------------------------------------------------------------------ RNG
class Rng:
    """Counter-based dropout / Gumbel generator: one 64-bit seed word in HBM (bumped on device every training
    step, so a captured graph draws fresh masks on every replay) + a per-call site id."""

    def __init__(self, device, seed=2019):
        self.device = torch.device(device)
        self.seed = torch.tensor([seed], dtype=torch.int64, device=device)
        self._site = 0

    def begin_step(self, defer=False):
        """a new seed for the step's dropout / Gumbel draws; defer=True: the caller's first launch is ``gather_cast_multi(…, rng=self)``,
        which advances the seed itself (one launch fewer)"""
        self._site = 0
        if not defer:
            _lib.call("bump_seed", _p(self.seed), _stream())

    def site(self):
        self._site += 1
        return self._site

    def mask(self, site, n, p, device):
        out = torch.empty(n, dtype=torch.float32, device=device)
        _lib.call("dropout_mask", _p(out), n, float(p), int(site), _p(self.seed), _stream())
        return out

    def attn_mask(self, site, n_rows, max_k, p, device):
        """keep mask of the attention-probability dropout, (n_rows, max_k), rows (sequence·H + head)·max_q + query"""
        out = torch.empty(n_rows, max_k, dtype=torch.float32, device=device)
        _lib.call("attn_dropout_mask", _p(out), n_rows, max_k, float(p), int(site), _p(self.seed), _stream())
        return out


_DEFAULT_RNG = {}


def make_rng(device, seed=2019):
    return Rng(device, seed)


def default_rng(device):
    key = str(device)
    if key not in _DEFAULT_RNG:
        _DEFAULT_RNG[key] = Rng(device)
    return _DEFAULT_RNG[key]


def _drop_args(drop):
    if drop is None or drop[0] <= 0.0:
        return 0.0, 0, None
    p, rng, site = drop
    return float(p), int(site), rng.seed


# ------------------------------------------------------------------------------------------------ GEMM
class KernelTimer:
    """Optional HIP-event bracket around launches of one kernel class (bench.py's roofline leg).  Events are
    recorded on the stream the kernel is launched on (PyTorch's current stream)."""

    def __init__(self, min_flops=0.0, select=None):
        self.min_flops = min_flops
        self.select = select  # optional predicate on (M, N, K, a_kc, b_kc, a_dt, b_dt, c_dt)
        self.records = []     # (work, start_event, end_event)

    def bracket(self, work, desc=None):
        if work < self.min_flops or (self.select is not None and not self.select(desc)):
            return None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.records.append((work, e0, e1, desc))
        return e0, e1

    def summary(self):
        torch.cuda.synchronize()
        ms = sum(e0.elapsed_time(e1) for _, e0, e1, _ in self.records)
        work = sum(w for w, _, _, _ in self.records)
        # algorithmic HBM bytes: every operand and the result once, in their storage types
        el = lambda d: 2 if d == 1 else 4      # (split = two bf16 planes = 4 bytes per element)
        nbytes = sum(M * K * el(a) + N * K * el(b) + M * N * el(c) for _, _, _, (M, N, K, _, _, a, b, c) in self.records)
        # an event pair around NOTHING still measures a few µs (record-to-record latency on the stream): calibrate and remove it,
        # so the per-launch average is comparable with the profiler's kernel durations
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(50)]
        for e0, e1 in pairs:
            e0.record(); e1.record()
        torch.cuda.synchronize()
        empty = sorted(e0.elapsed_time(e1) for e0, e1 in pairs)[len(pairs) // 2]
        net = max(ms - empty * len(self.records), 0.0)
        return dict(launches=len(self.records), work=work, ms=net, ms_raw=ms, event_overhead_ms=empty, bytes=nbytes)


GEMM_TIMER = None   # set by bench.py
ATTN_TIMER = None   # set by bench.py: {"select": predicate on (n_seq·H, max_q, max_k), "fwd": [(e0, e1, bytes)], "bwd": [...]} — HIP-event
                    # brackets around the attention launches of the clip encoder (the roofline north_star names)


def _attn_bracket(which, n_pairs, max_q, max_k, nbytes):
    t = ATTN_TIMER
    if t is None or not t["select"](n_pairs, max_q, max_k):
        return None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t[which].append((e0, e1, nbytes))
    e0.record()
    return e1

# Arithmetic type of the dense contractions:
#   "fp32"   — v_mfma_f32_32x32x2_f32, fp32 storage: bit-level parity mode (1/16 of the bf16 matrix rate);
#   "bf16"   — bf16 MFMA operands with fp32 accumulate, bf16 activation streams: the throughput mode the baseline names;
#   "bf16x3" — the ≤1e-4-parity throughput mode: every FORWARD contraction is a three-term split-bf16 product
#              (a_lo·b_hi + a_hi·b_lo + a_hi·b_hi on the bf16 matrix cores, fp32 accumulate: ≈2⁻¹⁷ per operand instead of 2⁻⁹), the
#              clip-encoder stream is stored as two bf16 planes per row (hi = bf16(v), lo = bf16(v - hi): the bytes of fp32), all
#              other activations as fp32; the BACKWARD runs the bf16 mode's kernels on the hi planes (gradients have bf16-mode
#              accuracy, the loss / probabilities / token ids have ≈fp32 accuracy).
_PRECISION = "fp32"


def set_precision(p):
    global _PRECISION
    assert p in ("fp32", "bf16", "bf16x3")
    _PRECISION = p


def get_precision():
    return _PRECISION


def _fast():
    """the bf16 matrix cores carry the contractions (either throughput mode)"""
    return _PRECISION != "fp32"


def is_x3():
    return _PRECISION == "bf16x3"


# ---- split tensors (bf16x3 mode).  A split activation is handed around as its HI plane: a bf16 view (R, W) with row stride ≥ 2W of
# a (R, 2W) buffer, tagged with ``_svpc_lo`` = the column offset of the lo plane.  To autograd it is an ordinary bf16 tensor (its
# gradient is a dense (R, W) bf16 tensor); the x3 forward kernels read hi + lo, the bf16 backward kernels read the view in place.
# The tag lives on the Python object: only tensors handed straight from one svpc op to the next carry it (every producer sets it);
# anything else (a torch view / cast / cat) silently drops to the hi plane — use ``to_f32`` to leave the split domain.
def lo_off(t):
    return getattr(t, "_svpc_lo", None)


def require_split_tag(t, who):
    """bf16x3 mode: a bf16 ACTIVATION reaching a forward op must carry its lo-plane tag.  A torch view / cast / detach / cat of a split
    tensor drops the tag silently, and the op would then compute a one-term bf16 product on the hi plane alone — outside the mode's
    ≤ 1e-4 contract with no error anywhere.  Fail instead (use ``to_f32`` to leave the split domain on purpose)."""
    if _PRECISION == "bf16x3" and t is not None and t.dtype == torch.bfloat16 and lo_off(t) is None:
        raise _lib.SvpcKernelError("%s: bf16 tensor without its lo-plane tag in bf16x3 mode (a torch view / cast / cat of a split "
                                   "tensor drops `_svpc_lo`; hand split tensors from op to op, or convert with ops.to_f32)" % who)


def new_split(rows, width, device):
    buf = torch.empty(rows, 2 * width, dtype=torch.bfloat16, device=device)
    hi = buf[:, :width]
    hi._svpc_lo = width
    return hi


def _lo_view(t):
    return torch.as_strided(t.detach(), t.shape, t.stride(), t.storage_offset() + t._svpc_lo)


def _rows_move(src, src_lo, idx, dst, dst_lo, R, W):
    """dst[r] = convert(src[idx ? idx[r] : r]) between storage kinds in one launch (svpc_rows_move; data movement)"""
    sk = 2 if src_lo is not None else _dt(src)
    dk = 2 if dst_lo is not None else _dt(dst)
    _lib.call("rows_move", _p(src), sk, src.stride(0), src_lo or 0, _p(idx), _p(dst), dk, dst.stride(0), dst_lo or 0, R, W, _stream())


class _ToF32(Function):
    @staticmethod
    def forward(ctx, t, lo):
        ctx.dt = t.dtype
        if t.dim() == 2 and t.is_cuda and t.stride(1) == 1:
            out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
            _rows_move(t, lo, None, out, None, t.shape[0], t.shape[1])
            return out
        out = t.float()
        if lo is not None:
            out += torch.as_strided(t, t.shape, t.stride(), t.storage_offset() + lo).float()
        return out

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dt), None


class _StreamAndF32(Function):
    """(alias of the stream tensor, its fp32 copy) as ONE node: the backward adds the two gradients and casts in one launch (two separate
    consumers cost a cast of the fp32 gradient, then autograd's add)."""

    @staticmethod
    def forward(ctx, t, lo):
        out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
        _rows_move(t, lo, None, out, None, t.shape[0], t.shape[1])
        ctx.set_materialize_grads(False)
        return t.view_as(t), out

    @staticmethod
    def backward(ctx, g_stream, g32):
        if g32 is None:
            return g_stream, None
        g32 = _c(g32)
        a = _c(g_stream) if g_stream is not None else None
        out = torch.empty(g32.shape, dtype=torch.bfloat16, device=g32.device)
        _lib.call("add_cast_bf16", _p(a), _p(g32), _p(out), g32.numel(), _stream())
        return out, None


def stream_and_f32(t):
    """(t, fp32 copy of t) for a bf16 / split 2-D stream tensor with two consumers (one per form); fp32 input: (t, t)"""
    if t.dtype == torch.float32:
        return t, t
    lo = lo_off(t)
    if not (t.dim() == 2 and t.is_cuda and t.stride(1) == 1):
        return t, to_f32(t)
    a, f = _StreamAndF32.apply(t, lo)
    if lo is not None:
        a._svpc_lo = lo
    return a, f


def to_f32(t):
    """fp32 copy of a bf16 / split tensor (hi + lo for a split one; data movement and one exact add)."""
    if t.dtype == torch.float32:
        return t
    return _ToF32.apply(t, lo_off(t))


class _ScatterRows(Function):
    """out (n_rows, W) = zeros with out[idx[r]] = src[r] (idx int64, distinct rows); backward gathers the rows back"""

    @staticmethod
    def forward(ctx, src, idx, n_rows, inv=None):
        ctx.save_for_backward(idx)
        if inv is not None and src.is_cuda and src.dtype == torch.float32:       # inv: padded row → packed row or -1 (one launch)
            src = _c(src)
            out = torch.empty(n_rows, src.shape[1], dtype=torch.float32, device=src.device)
            _lib.call("rows_expand", _p(src), _p(inv), _p(out), n_rows, src.shape[1], _stream())
            return out
        out = torch.zeros(n_rows, src.shape[1], dtype=src.dtype, device=src.device)
        out.index_copy_(0, idx, src)
        return out

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        return torch.index_select(g, 0, idx), None, None, None


def scatter_rows(src, idx, n_rows, inv=None):
    """rows of a packed tensor back into a padded layout (zeros elsewhere); data movement.  inv (int32, n_rows): the packed row of every
    padded row or -1 — with it the expansion is one launch"""
    return _ScatterRows.apply(src, idx, int(n_rows), inv)


def take_rows_f32(t, idx):
    """fp32 rows ``idx`` of a (possibly split / bf16) 2-D tensor."""
    lo = lo_off(t)
    if lo is None:
        return torch.index_select(t, 0, idx).float()
    return _TakeSplit.apply(t, idx, lo)[0]


def take_rows_f32_alias(t, idx):
    """(fp32 rows ``idx`` of ``t``, an alias of ``t``) for a stream tensor with exactly ONE other consumer: that consumer takes the alias,
    and the gradient of the gathered rows is added into the alias's gradient IN PLACE (one small scatter launch) instead of a zero-filled
    stream-sized tensor, an index_add and autograd's stream-sized sum.  Plain tensors: (rows, t)."""
    lo = lo_off(t)
    if (lo is None and t.dtype != torch.bfloat16) or not t.is_cuda or idx.dtype != torch.int32 or t.dim() != 2:
        return take_rows_f32(t, idx), t
    rows, alias = _TakeSplit.apply(t, idx, lo)
    if lo is not None:
        alias._svpc_lo = lo
    return rows, alias


class _TakeSplit(Function):
    @staticmethod
    def forward(ctx, t, idx, lo):
        ctx.save_for_backward(idx)
        ctx.shape, ctx.dt = t.shape, t.dtype
        ctx.set_materialize_grads(False)         # (an unused alias must reach backward as None, not as a stream-sized tensor of zeros)
        if t.is_cuda and idx.dtype == torch.int32 and t.stride(1) == 1:
            out = torch.empty(idx.numel(), t.shape[1], dtype=torch.float32, device=t.device)
            _rows_move(t, lo, idx, out, None, idx.numel(), t.shape[1])
        elif lo is not None:
            low = torch.as_strided(t, t.shape, t.stride(), t.storage_offset() + lo)
            out = torch.index_select(t, 0, idx).float() + torch.index_select(low, 0, idx).float()
        else:
            out = torch.index_select(t, 0, idx).float()
        return out, t.view_as(t)

    @staticmethod
    def backward(ctx, g, g_alias):
        idx, = ctx.saved_tensors
        if g is None:
            return g_alias, None, None
        if (g_alias is not None and g_alias.is_cuda and g_alias.dtype == torch.bfloat16 and g_alias.is_contiguous() and idx.dtype == torch.int32
                and tuple(g_alias.shape) == tuple(ctx.shape)):
            g = _c(g.float())
            _lib.call("scatter_add_rows_bf16", _p(g), _p(idx), _p(g_alias), g_alias.stride(0), idx.numel(), g.shape[1], _stream())
            return g_alias, None, None
        out = torch.zeros(ctx.shape, dtype=ctx.dt, device=g.device)
        out.index_add_(0, idx.long(), g.to(ctx.dt))
        if g_alias is not None:
            out = out + g_alias
        return out, None, None


# bf16 activation stream: in "bf16" precision the clip encoder and the decoder keep their activations (and their gradients) in
# HBM as bf16 — half the bytes for every LayerNorm / attention / GEMM operand; statistics, softmax, accumulation and all parameter
# gradients stay fp32.  Any row count qualifies (the direct-to-LDS GEMM clamps its M/N edges and zero-fills the K tail of the
# wgrad); feature dims must be multiples of 32.  Without the direct-to-LDS kernel only interior-only shapes do (multiples of 128).
BF16_STREAM = True
USE_GLDS = True        # direct-to-LDS GEMM for bf16 × bf16 interior shapes
USE_L32 = True         # direct-to-LDS GEMM for fp32 × fp32 operands (latency-bound text / step-level side)


def _dt(t):
    return 1 if t.dtype == torch.bfloat16 else 0


def bf16_stream_ok(rows, *dims):
    if not (_fast() and BF16_STREAM and rows > 0):
        return False
    if is_x3():          # the split stream's GEMM (gemm_p8x3.hip) walks 64-deep k-tiles
        return USE_GLDS and all(d % 64 == 0 for d in dims)
    if USE_GLDS:
        return all(d % 32 == 0 for d in dims)
    return rows % 128 == 0 and all(d % 128 == 0 for d in dims)


# ---- backward ablation switches (tests/tools/bwd_ablation.py; all False in the product): which part of the bf16 backward of the bf16x3
# mode moves a training trajectory away from the fp32 one?  BWD_EXACT: every contraction on fp32 storage that is NOT a three-term forward
# product (i.e. the dgrads / wgrads of the text / step-level side) runs on the exact f32 MFMA, ungrouped; ATTN_BWD_EXACT: attention on
# fp32 storage takes the exact fp32 backward kernel instead of the matrix-core one.  (The third switch is ``BF16_STREAM`` below: False
# keeps every activation — and so every gradient — in fp32 storage.)
BWD_EXACT = False
ATTN_BWD_EXACT = False


def _gemm(A, lda, a_kc, B, ldb, b_kc, C, M, N, K, Z=None, bias=None, act=ACT_NONE, p=0.0, site=0, seed=None, accumulate=0, R=None, G=None,
          x3=False):
    """C = epi(A·B) (+ R: an addend of C's type and layout, only on the bf16 direct-to-LDS path; other paths add it afterwards).
    G = (aux, act): C = (A·B) ⊙ act'(aux) — absorbed only by the bf16 direct-to-LDS path; returns whether it was applied.
    x3 (fp32 operands, bf16x3 mode, forward products): three-term split-bf16 products (svpc_gemm_l32_x3); shapes that kernel does
    not take (a k-strided operand with K % 32 != 0, K % 4 != 0) run on the exact f32 MFMA instead — never on one-term bf16."""
    ws = _ws(C.device)
    g_done = False
    ev = (GEMM_TIMER.bracket(2.0 * M * N * K, (M, N, K, a_kc, b_kc, _dt(A), _dt(B), _dt(C)))
          if GEMM_TIMER is not None else None)
    if ev:
        ev[0].record()
    if BWD_EXACT and not x3 and A.dtype == B.dtype == C.dtype == torch.float32:
        _lib.call("gemm_f32", _p(A), lda, a_kc, _p(B), ldb, b_kc, _p(C), C.stride(0), _p(Z), M, N, K, _p(bias), act, p, site,
                  _p(seed), accumulate, _p(ws), ws.numel() * 4, _stream())
    elif x3 and A.dtype == B.dtype == C.dtype == torch.float32:
        if (A.data_ptr() | B.data_ptr()) % 16 == 0 and _lib.load().svpc_gemm_l32_supported(a_kc, b_kc, lda, ldb, M, N, K) == 1:
            _lib.call("gemm_l32_x3", _p(A), lda, a_kc, _p(B), ldb, b_kc, _p(C), C.stride(0), _p(Z), None, M, N, K, _p(bias), act, p, site,
                      _p(seed), accumulate, _p(ws), ws.numel() * 4, _stream())
        else:
            _lib.call("gemm_f32", _p(A), lda, a_kc, _p(B), ldb, b_kc, _p(C), C.stride(0), _p(Z), M, N, K, _p(bias), act, p, site,
                      _p(seed), accumulate, _p(ws), ws.numel() * 4, _stream())
    elif (_fast() and USE_P8T and a_kc == 1 and b_kc == 0 and A.dtype == B.dtype == C.dtype == torch.bfloat16 and Z is None and bias is None
          and act == ACT_NONE and p <= 0.0 and not accumulate and (-(-M // 256)) * (-(-N // 256)) >= P8T_MIN_TILES
          and (A.data_ptr() | B.data_ptr() | C.data_ptr()) % 16 == 0
          and _lib.load().svpc_gemm_p8t_supported(lda, ldb, C.stride(0), M, N, K) == 1
          and (R is None or (R.dtype == torch.bfloat16 and R.shape == C.shape and R.stride() == C.stride() and R.data_ptr() % 16 == 0))
          and (G is None or (G[1] in (ACT_RELU, ACT_GELU) and G[0].dtype == torch.bfloat16 and G[0].shape == C.shape
                             and G[0].stride() == C.stride() and G[0].data_ptr() % 16 == 0))):
        # stream dgrad on the 8-phase template with the weight matrix read k-strided in place (gemm_p8t.hip)
        _lib.call("gemm_p8t", _p(A), lda, _p(B), ldb, _p(C), C.stride(0), _p(G[0]) if G is not None else None, int(G[1]) if G is not None else 0,
                  _p(R), M, N, K, _stream())
        R = None
        g_done = G is not None
    elif (_fast() and USE_S4T and a_kc == 1 and b_kc == 0 and A.dtype == B.dtype == C.dtype == torch.bfloat16 and Z is None and bias is None
          and act == ACT_NONE and p <= 0.0 and not accumulate and G is None and S4T_MIN_TILES <= (-(-M // 128)) * (-(-N // 128)) <= S4T_MAX_TILES
          and (A.data_ptr() | B.data_ptr() | C.data_ptr()) % 16 == 0
          and _lib.load().svpc_gemm_s4t_supported(lda, ldb, C.stride(0), M, N, K) == 1
          and (R is None or (R.dtype == torch.bfloat16 and R.shape == C.shape and R.stride() == C.stride() and R.data_ptr() % 16 == 0))):
        # small-M stream dgrad (the decoder's 4,224 / 576 rows) on 128² tiles with the weight matrix read k-strided in place (gemm_s4t.hip)
        _lib.call("gemm_s4t", _p(A), lda, _p(B), ldb, _p(C), C.stride(0), _p(R), M, N, K, _stream())
        R = None
    elif _fast() and USE_GLDS and A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16 and \
            (A.data_ptr() | B.data_ptr()) % 16 == 0 and _lib.load().svpc_gemm_glds_supported(a_kc, b_kc, lda, ldb, M, N, K) == 1:
        g_ok = G is not None and G[0].dtype == C.dtype and G[0].shape == C.shape and G[0].stride() == C.stride() and not accumulate
        _lib.call("gemm_glds_rg", _p(A), lda, a_kc, _p(B), ldb, b_kc, _p(C), _dt(C), C.stride(0), _p(Z), _p(R), _p(G[0]) if g_ok else None,
                  int(G[1]) if g_ok else 0, M, N, K, _p(bias), act, p, site, _p(seed), accumulate, _p(ws), ws.numel() * 4, _stream())
        R = None
        g_done = g_ok
    elif _fast() and USE_L32 and A.dtype == B.dtype == C.dtype == torch.float32 and \
            (A.data_ptr() | B.data_ptr()) % 16 == 0 and _lib.load().svpc_gemm_l32_preferred(a_kc, b_kc, lda, ldb, M, N, K) == 1:
        if R is not None and not (R.dtype == torch.float32 and R.is_contiguous() and R.shape == C.shape and C.is_contiguous()):
            Rk = None
        else:
            Rk, R = R, None       # absorbed by the epilogue
        g_ok = (G is not None and G[0].dtype == torch.float32 and G[0].shape == C.shape and G[0].is_contiguous() and C.is_contiguous()
                and Z is None and bias is None and act == ACT_NONE and p <= 0.0)
        if g_ok:                  # C = (A·B) ⊙ act'(aux) + R: the activation backward of the tensor this dgrad differentiates
            _lib.call("gemm_l32_rg", _p(A), lda, a_kc, _p(B), ldb, b_kc, _p(C), C.stride(0), _p(Rk), _p(G[0]), int(G[1]), M, N, K,
                      accumulate, _p(ws), ws.numel() * 4, _stream())
            g_done = True
        else:
            _lib.call("gemm_l32_r", _p(A), lda, a_kc, _p(B), ldb, b_kc, _p(C), C.stride(0), _p(Z), _p(Rk), M, N, K, _p(bias), act, p, site,
                      _p(seed), accumulate, _p(ws), ws.numel() * 4, _stream())
    elif _fast():
        dt = lambda t: 1 if t.dtype == torch.bfloat16 else 0
        _lib.call("gemm_mx", _p(A), dt(A), lda, a_kc, _p(B), dt(B), ldb, b_kc, _p(C), dt(C), C.stride(0), _p(Z), M, N, K, _p(bias),
                  act, p, site, _p(seed), accumulate, _p(ws), ws.numel() * 4, _stream())
    else:
        _lib.call("gemm_f32", _p(A), lda, a_kc, _p(B), ldb, b_kc, _p(C), C.stride(0), _p(Z), M, N, K, _p(bias), act, p, site,
                  _p(seed), accumulate, _p(ws), ws.numel() * 4, _stream())
    if R is not None:
        if G is not None and not g_done:
            raise _lib.SvpcKernelError("gemm: an activation-backward factor and an addend need the direct-to-LDS path")
        C.add_(R)
    if ev:
        ev[1].record()
    return g_done


def _colsum(x2d, idx=None, K=1, out=None, accumulate=0):
    R, Cc = x2d.shape
    if out is None:
        out = torch.empty(K, Cc, dtype=torch.float32, device=x2d.device)
        if R == 0:
            return out.zero_()
    if R == 0:
        return out
    ws = _ws(x2d.device)
    _lib.call("bucket_colsum_t", _p(x2d), _dt(x2d), x2d.stride(0), _p(idx), R, Cc, K, _p(out), accumulate, _p(ws), _stream())
    return out


# Direct-to-arena parameter gradients: once the optimizer has re-pointed ``p.grad`` into its contiguous arena (and marked
# the parameter), backward kernels accumulate weight / bias / gain gradients straight into that storage (GEMM epilogue
# ``accumulate``, reduction finalizers) instead of returning a tensor for autograd to add — no temporaries, no add kernels.


def _direct(p):
    if p is None or not p.is_leaf:
        return None
    g = getattr(p, "grad", None)
    return g if (g is not None and getattr(p, "_svpc_direct", False)) else None


def direct_grads(*params):
    """the arena gradients of ``params`` when every one of them is written in place (else None) — for ``linear(..., bgrad=(…))`` with a
    bias that is a sum of parameters"""
    gs = tuple(_direct(p) for p in params)
    return gs if all(g is not None for g in gs) else None


def _shadow(w):
    """bf16 shadow of parameter ``w`` (svpc_amd.optim.WeightStore), re-cast first if ``w`` changed behind the store's back.  A store
    built with the lo plane (bf16x3 mode) keeps it ``_svpc_lo`` elements behind the shadow; it is re-cast together with it."""
    s = getattr(w, "_svpc_bf16", None)
    if s is None:
        return None
    if w._version != w._svpc_bf16_ver:
        with torch.no_grad():
            s.copy_(w.detach())
            if lo_off(s) is not None:
                split_planes(w.detach(), s, _lo_view_flat(s))
        w._svpc_bf16_ver = w._version
    return s


def _lo_view_flat(s):
    """the lo plane of a weight-shadow view (same shape and strides, ``_svpc_lo`` elements further on in the store's buffer)"""
    return torch.as_strided(s, s.shape, s.stride(), s.storage_offset() + s._svpc_lo)


def split_planes(src, hi, lo):
    """hi ← bf16(src), lo ← bf16(src - hi) (weights leaving the fp32 master copy; data preparation, not on the step's hot path)"""
    with torch.no_grad():
        hi.copy_(src)
        lo.copy_(src - hi.float())


def _transient_split(w):
    """(hi, lo offset) planes of a weight that has no store (first step, tests): one 2·numel bf16 buffer"""
    buf = torch.empty(2, *w.shape, dtype=torch.bfloat16, device=w.device)
    split_planes(w.detach(), buf[0], buf[1])
    hi = buf[0]
    hi._svpc_lo = w.numel()
    return hi


# Residual-gradient hand-over.  In `y = LayerNorm(sub(h) + h)` the gradient of h has two parts: the LayerNorm's dh (residual path)
# and the dgrad of sub's first projection.  Autograd would add them with a separate kernel (≈30 per step on the bf16 streams);
# instead a LayerNorm called with sink=True parks its dh here, keyed by h's address, and returns no residual gradient, and the
# backward of the projection that consumes h adds the parked tensor in its dgrad epilogue (C = dz·W + R).  The caller promises
# that exactly one ops.linear consumes h and needs its input gradient; join_side() fails loudly if a parked gradient is left over.
USE_RES_SINK = os.environ.get("SVPC_RES_SINK", "1") != "0"
FUSE_ACT_BWD = os.environ.get("SVPC_FUSE_ACT_BWD", "1") != "0"      # activation backward inside the following projection's dgrad
FUSE_ACT_BWD_F32 = os.environ.get("SVPC_FUSE_ACT_BWD_F32", "1") != "0"      # … also for fp32-storage projections (step-wise encoder)
_RES_SINK = {}
SINK_STATS = [0, 0]        # parked by LayerNorm backwards / absorbed by dgrad epilogues (since import)


class _Linear(Function):
    @staticmethod
    def forward(ctx, x, w, b, act, trans_w, drop, wgrad, bgrad, w16, tok_out=None, tok_in=None):
        _need_gpu(x)
        x_lo = lo_off(x)
        x = _rows2d(x)
        w_lo = lo_off(w16) if w16 is not None else None
        w = _c(w if w16 is None else w16)      # bf16 shadow: both GEMM operands stream straight into LDS
        M, K = x.shape
        N = w.shape[1] if trans_w else w.shape[0]
        p, site, seed = _drop_args(drop)
        if x_lo is not None:
            # bf16x3 stream: split activations × split weight shadow → split output (gemm_p8x3.hip); the pre-activation copy z is a
            # plain bf16 matrix (all the bf16 backward needs, for ReLU too: z > 0 ⇔ y > 0)
            if w_lo is None or trans_w or p > 0.0:
                raise _lib.SvpcKernelError("linear: a split activation needs a split weight shadow, an (out, in) weight and no dropout")
            y = new_split(M, N, x.device)
            z = torch.empty(M, N, dtype=torch.bfloat16, device=x.device) if act != ACT_NONE else None
            # (bench.py's roofline bracket: dtype code 2 = split operands; work = the product's 2·M·N·K, the kernel issues 3× that)
            ev = GEMM_TIMER.bracket(2.0 * M * N * K, (M, N, K, 1, 1, 2, 2, 2)) if GEMM_TIMER is not None else None
            if ev:
                ev[0].record()
            # 256×256 tiles when they fill the chip, else 128×128 (the decoder's 4,224 / 576 rows)
            kern = "gemm_p8x3" if (-(-M // 256)) * (-(-N // 256)) >= X3_BIG_TILES else "gemm_s4x3"
            _lib.call(kern, _p(x), x.stride(0), x_lo, _p(w), w.stride(0), w_lo, _p(y), y.stride(0), y._svpc_lo, _p(z), N, M, N, K,
                      _p(b), act, _stream())
            if ev:
                ev[1].record()
            ctx.save_for_backward(x, w, z)
            ctx.cfg = (act, trans_w, p, site, seed, b is not None)
            ctx.direct = (wgrad, bgrad)
            ctx.tok_out, ctx.tok_in = tok_out, tok_in
            if tok_out is not None:
                tok_out["aux"], tok_out["act"] = z, act
            return y
        y = torch.empty(M, N, dtype=x.dtype, device=x.device)
        z = torch.empty_like(y) if act == ACT_GELU else None
        _gemm(x, x.stride(0), 1, w, w.stride(0), 0 if trans_w else 1, y, M, N, K, Z=z, bias=b, act=act, p=p, site=site, seed=seed,
              x3=is_x3())
        ctx.save_for_backward(x, w, z if act == ACT_GELU else (y if act != ACT_NONE else None))
        ctx.cfg = (act, trans_w, p, site, seed, b is not None)
        ctx.direct = (wgrad, bgrad)
        # activation backward folded into the NEXT projection's dgrad (see linear(): fuse_act_bwd): this node publishes what its
        # activation's backward needs; the consumer's backward reports the gradient it has already multiplied
        ctx.tok_out, ctx.tok_in = tok_out, tok_in
        if tok_out is not None:
            tok_out["aux"], tok_out["act"] = (z if act == ACT_GELU else y), act
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, aux = ctx.saved_tensors
        act, trans_w, p, site, seed, has_b = ctx.cfg
        M, K = x.shape
        N = w.shape[1] if trans_w else w.shape[0]
        dy = _c(dy)
        tok = ctx.tok_out
        premul = tok is not None and tok.get("done") is not None
        if premul:
            if tok["done"] != (dy.data_ptr(), tuple(dy.shape)):
                raise _lib.SvpcKernelError("fused activation backward: the activated tensor has a second consumer (its gradient is not "
                                           "the one the following projection wrote)")
            tok["done"] = None
        if premul:
            dz = dy                  # the following projection's dgrad has applied act'(.) already
        elif act != ACT_NONE or p > 0.0:
            dz = torch.empty_like(dy)
            _lib.call("act_bwd_t", _p(dy), _p(aux if aux is not None else dy), _p(dz), _dt(dy), dy.numel(), act, p, site, _p(seed),
                      _stream())
        else:
            dz = dy
        dx = dw = db = None
        wgrad, bgrad = ctx.direct
        if isinstance(bgrad, tuple):
            # the bias is the sum of several parameters (the LSTM's b_ih + b_hh, model.py:1022): each of them receives Σ_rows dz in place —
            # the first the usual way below, the others through one more entry of the grouped column sum
            for e in bgrad[1:]:
                bias_grad(dz, e)
            bgrad = bgrad[0]
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, K, dtype=x.dtype, device=dy.device)
            parked = _RES_SINK.pop(x.data_ptr(), None) if _RES_SINK else None
            if parked is not None:
                SINK_STATS[1] += 1
            if parked is not None and (parked.shape != dx.shape or parked.dtype != dx.dtype):
                raise _lib.SvpcKernelError("residual-gradient hand-over: parked gradient does not match the projection's input")
            tin = ctx.tok_in
            G = (tin["aux"], tin["act"]) if (tin is not None and tin.get("aux") is not None and parked is None) else None
            if _gemm(dz, N, 1, w, w.stride(0), 1 if trans_w else 0, dx, M, K, N, R=parked, G=G):
                tin["done"] = (dx.data_ptr(), tuple(dx.shape))
        w_done = False
        if wgrad is not None and not trans_w and (not has_b or bgrad is not None):
            if dz.dtype == torch.bfloat16:
                # bf16 stream: grouped wgrad; the bias gradient rides along (taken from the dz tiles the launch stages) when it is a
                # plain fp32 arena vector, else it goes its usual way below
                ride = (P8W_BIAS and USE_P8W and has_b and bgrad is not None and bgrad.dtype == torch.float32 and bgrad.is_contiguous()
                        and bgrad.numel() == N and min(N, K) >= 256)
                if defer_wgrad(dz, x, wgrad, bgrad if ride else None):
                    w_done = True
                    if ride:
                        return dx, None, None, None, None, None, None, None, None, None, None
            elif defer_wgrad(dz, x, wgrad, bgrad if has_b else None):
                return dx, None, None, None, None, None, None, None, None, None, None
        if not w_done and (wgrad is not None or ctx.needs_input_grad[1]):
            acc = 1 if wgrad is not None else 0
            dw = wgrad if wgrad is not None else torch.empty_like(w)
            if trans_w:   # w (K, N): dw = xᵀ dz
                _gemm(x, x.stride(0), 0, dz, N, 0, dw, K, N, M, accumulate=acc)
            else:         # w (N, K): dw = dzᵀ x
                _gemm(dz, N, 0, x, x.stride(0), 0, dw, N, K, M, accumulate=acc)
            if wgrad is not None:
                _ready(wgrad, "w")
                dw = None
        if has_b and (bgrad is not None or ctx.needs_input_grad[2]):
            if bgrad is not None:
                bias_grad(dz, bgrad)
            else:
                db = _colsum(dz).view(-1)
        return dx, dw, db, None, None, None, None, None, None, None, None


# ---- bf16x3 ablation experiments (tools/x3_ablation.py; None in the product): which contractions need their lo planes?  One family of
# projections at a time is degraded — its activation operand's lo plane dropped ("a"), its weight operand's ("b"), its output's ("o": the
# stored value becomes plain bf16) — by handing the UNCHANGED three-term kernels operands whose lo plane is zero (fp32-storage families:
# operands rounded to bf16 first), forward only, under no_grad.  ABLATE = {"match": f(param_name) -> str of "abo" flags or "", "names":
# {data_ptr: parameter name}}.
ABLATE = None


def _ablate_flags(w):
    if ABLATE is None:
        return ""
    name = ABLATE["names"].get(w.data_ptr())
    return ABLATE["match"](name) if name is not None else ""


def _zero_lo_copy(t):
    lo = lo_off(t)
    if lo is None:
        return t.to(torch.bfloat16).float() if t.dtype == torch.float32 else t
    c = new_split(t.shape[0], t.shape[1], t.device)
    c.copy_(t.detach())
    _lo_view(c).zero_()
    return c


def linear(x, w, b=None, act=ACT_NONE, trans_w=False, drop=None, wgrad=None, bgrad=None, w16=None, fuse_act_bwd=False):
    """fuse_act_bwd=True (with an activation, no dropout): the caller promises that the returned tensor is consumed by exactly ONE
    ops.linear; on a bf16 stream that projection's dgrad then writes the gradient of this projection's pre-activation directly
    (C = dz·W ⊙ act'(z), svpc_gemm_glds_rg) and the separate activation-backward pass over the stream is skipped.  A second consumer
    is detected in backward and fails loudly."""
    tok_in = getattr(x, "_svpc_act_tok", None)
    require_split_tag(x, "linear")
    abl = _ablate_flags(w) if ABLATE is not None else ""
    if abl:
        assert not torch.is_grad_enabled(), "ablation experiments are forward-only"
        if "a" in abl:
            x = _zero_lo_copy(x)
        if "b" in abl:
            if w16 is None:
                w16 = _shadow(w)
            if w16 is not None and lo_off(w16) is not None:          # (a weight shadow keeps its lo plane numel-strided, like _transient_split)
                buf = torch.zeros(2, *w16.shape, dtype=torch.bfloat16, device=w16.device)
                buf[0].copy_(w16)
                w16 = buf[0]
                w16._svpc_lo = w16.numel()
            w = w.detach().to(torch.bfloat16).float()
    split = lo_off(x) is not None
    if x.dtype == torch.bfloat16:
        n_out = w.shape[1] if trans_w else w.shape[0]
        ok = bf16_stream_ok(x.shape[0], x.shape[1], n_out) and not trans_w and drop is None
        if ok and split:
            ok = act != ACT_SIGMOID and _lib.load().svpc_gemm_p8x3_supported(x.stride(0), x._svpc_lo, x.shape[1], 2 * n_out, n_out, n_out,
                                                                             x.shape[0], n_out, x.shape[1]) == 1
        if not ok:
            x = to_f32(x)          # shapes outside the bf16-stream GEMM variants fall back to fp32 storage
            split = False
    if wgrad is None:
        wgrad = _direct(w)
    if bgrad is None and b is not None:
        bgrad = _direct(b)
    if x.dtype == torch.bfloat16 and USE_GLDS:
        if w16 is None:
            w16 = _shadow(w)
        if split and (w16 is None or lo_off(w16) is None):
            w16 = _transient_split(w)          # no store with a lo plane (first step, a store built in another mode): split on the fly
        if w16 is None:            # no weight store yet (first step, inference without one): a transient bf16 copy
            w16 = w.detach().to(torch.bfloat16)
    else:
        w16 = None
    # (bf16 streams: the direct-to-LDS dgrads; fp32 storage in the fast modes: svpc_gemm_l32_rg)
    can_g = (x.dtype == torch.bfloat16 and USE_GLDS) or (x.dtype == torch.float32 and USE_L32 and FUSE_ACT_BWD_F32 and _fast())
    fuse = fuse_act_bwd and FUSE_ACT_BWD and act != ACT_NONE and drop is None and can_g and torch.is_grad_enabled()
    tok_out = {} if fuse else None
    if tok_in is not None and (trans_w or not can_g):
        tok_in = None
    y = _Linear.apply(x, w, b, act, trans_w, drop, wgrad, bgrad, w16, tok_out, tok_in)
    if split:
        y._svpc_lo = y.shape[1]        # (a split activation yields a split output: see _Linear.forward)
    if abl and "o" in abl:
        if split:
            _lo_view(y).zero_()
        else:
            y = y.to(torch.bfloat16).float()
    if tok_out is not None:
        y._svpc_act_tok = tok_out
    return y


# ------------------------------------------------------------------------------------------------ LayerNorm family
class _LayerNorm(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, add2, eps, src_rows, pad_row, pre_drop, post_drop, add1, add1_mod, add2_idx,
                out_bf16=False, sink=False, out_split=False):
        _need_gpu(x)
        ctx.sink = bool(sink)
        ctx.direct = (_direct(gamma), _direct(beta), _direct(x) if src_rows is not None else None,
                      _direct(add2) if add2 is not None else None)
        x_lo = lo_off(x)
        r_lo = lo_off(residual) if residual is not None else None
        split = out_split or x_lo is not None or r_lo is not None
        if x_lo is None:
            x = _c(x)
        D = x.shape[1]
        R = src_rows.numel() if src_rows is not None else x.shape[0]
        p_pre, s_pre, seed1 = _drop_args(pre_drop)
        p_post, s_post, seed2 = _drop_args(post_drop)
        seed = seed1 if seed1 is not None else seed2
        mean = torch.empty(R, dtype=torch.float32, device=x.device)
        rstd = torch.empty(R, dtype=torch.float32, device=x.device)
        add1 = _c(add1) if add1 is not None else None
        if split:
            # bf16x3 stream: x is fp32 (the gathered feature / embedding rows) or split, the residual is split, y is split
            if (x_lo is None and x.dtype != torch.float32) or (residual is not None and r_lo is None):
                raise _lib.SvpcKernelError("layernorm: a split output needs fp32 or split inputs and a split residual")
            y = new_split(R, D, x.device)
            _lib.call("ln_fwd_s", _p(x), 2 if x_lo is not None else 0, x.stride(0), x_lo or 0, _p(src_rows), _p(residual),
                      residual.stride(0) if residual is not None else 0, r_lo or 0, _p(gamma), _p(beta), _p(y), 2, y.stride(0), y._svpc_lo,
                      _p(mean), _p(rstd), R, D, float(eps), p_pre, s_pre, p_post, s_post, _p(seed), _p(add1), int(add1_mod), _p(add2),
                      _p(add2_idx), _stream())
            ctx.save_for_backward(x, gamma, residual, mean, rstd, src_rows, add2_idx, seed)      # (the hi planes: bf16 views)
            ctx.cfg = (R, D, p_pre, s_pre, p_post, s_post, pad_row, add2.shape[0] if add2 is not None else 0)
            return y
        residual = _c(residual) if residual is not None else None
        y_dtype = torch.bfloat16 if (out_bf16 or x.dtype == torch.bfloat16) else torch.float32
        if residual is not None and residual.dtype != y_dtype:
            residual = residual.to(y_dtype)
        y = torch.empty(R, D, dtype=y_dtype, device=x.device)
        _lib.call("ln_fwd_t", _p(x), _dt(x), _p(src_rows), _p(residual), _p(gamma), _p(beta), _p(y), _dt(y), _p(mean), _p(rstd), R, D,
                  float(eps), p_pre, s_pre, p_post, s_post, _p(seed), _p(add1), int(add1_mod), _p(add2), _p(add2_idx), _stream())
        ctx.save_for_backward(x, gamma, residual, mean, rstd, src_rows, add2_idx, seed)
        ctx.cfg = (R, D, p_pre, s_pre, p_post, s_post, pad_row, add2.shape[0] if add2 is not None else 0)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, residual, mean, rstd, src_rows, add2_idx, seed = ctx.saved_tensors
        R, D, p_pre, s_pre, p_post, s_post, pad_row, k_add2 = ctx.cfg
        dy = _c(dy)
        dev = dy.device
        need_x, need_res = ctx.needs_input_grad[0], (residual is not None and ctx.needs_input_grad[3])
        dh = dx_rows = None
        same_t = x.dtype == dy.dtype
        if need_res or (need_x and p_pre <= 0.0 and same_t):
            dh = torch.empty(R, D, dtype=dy.dtype, device=dev)
        if need_x:
            dx_rows = dh if (p_pre <= 0.0 and same_t) else torch.empty(R, D, dtype=x.dtype, device=dev)
        g_dir, b_dir, x_dir, a2_dir = ctx.direct
        # the dgamma/dbeta tail only feeds the optimizer: per-group partials now, their column sums with every other pending tail
        groups = (_lib.load().svpc_ln_param_only_groups(R) if dh is None and dx_rows is None else _lib.load().svpc_ln_bwd_groups(R))
        partial = torch.empty(groups * 2 * D, dtype=torch.float32, device=dev)
        # (strided form: in bf16x3 mode the saved x / residual are the hi planes of split rows, read in place)
        _lib.call("ln_bwd_rows_s", _p(dy), _p(x), _dt(x), x.stride(0), _dt(dy), _p(src_rows), _p(residual),
                  residual.stride(0) if residual is not None else 0, _p(gamma), _p(mean), _p(rstd), _p(dh), _p(dx_rows), _p(partial), R, D,
                  p_pre, s_pre, p_post, s_post, _p(seed), _stream())
        dgamma = dbeta = None
        if not defer_partials(partial, groups, 2 * D, g_dir, b_dir, D):
            dgamma, dbeta = torch.empty(D, dtype=torch.float32, device=dev), torch.empty(D, dtype=torch.float32, device=dev)
            _lib.call("ln_param_grads_g", _p(partial), groups, D, _p(dgamma), _p(dbeta), 0, _stream())
        dx = None
        if need_x:
            if src_rows is not None:
                dx = x_dir if x_dir is not None else torch.zeros_like(x)
                _lib.call("scatter_add_rows", _p(dx_rows), _p(src_rows), _p(dx), R, D, int(pad_row), _stream())
                if x_dir is not None:
                    _ready(dx)
                    dx = None
            else:
                dx = dx_rows
        dadd2 = None
        if k_add2 and ctx.needs_input_grad[4]:
            if a2_dir is not None:
                _colsum(dy, add2_idx, k_add2, out=a2_dir, accumulate=1)
                _ready(a2_dir)
            else:
                dadd2 = _colsum(dy, add2_idx, k_add2)
        dres = dh if need_res else None
        if need_res and ctx.sink and USE_RES_SINK and (dh.dtype == torch.bfloat16 or (_fast() and USE_L32)):
            _RES_SINK[residual.data_ptr()] = dh       # joins the dgrad of the projection that consumes the residual tensor
            SINK_STATS[0] += 1
            _queue_end_of_backward_join()
            dres = None
        return dx, dgamma, dbeta, dres, dadd2, None, None, None, None, None, None, None, None, None, None, None


def layernorm(x, gamma, beta, eps, residual=None, src_rows=None, pad_row=-1, pre_drop=None, post_drop=None,
              add1=None, add1_mod=0, add2=None, add2_idx=None, out_bf16=False, sink=False):
    """sink=True: the residual tensor's only other consumer is an ops.linear whose backward will absorb this LayerNorm's
    residual-path gradient in its dgrad epilogue (see _RES_SINK).  out_bf16: the output joins an activation stream — bf16 in the
    bf16 mode, split (two bf16 planes) in the bf16x3 mode; split inputs always give a split output."""
    require_split_tag(x, "layernorm")
    require_split_tag(residual, "layernorm (residual)")
    out_split = bool(out_bf16) and is_x3()
    split = out_split or lo_off(x) is not None or (residual is not None and lo_off(residual) is not None)
    y = _LayerNorm.apply(x, gamma, beta, residual, add2, eps, src_rows, pad_row, pre_drop, post_drop, add1, add1_mod,
                         add2_idx, out_bf16, sink, out_split)
    if split:
        y._svpc_lo = y.shape[1]
    if ABLATE is not None and "o" in _ablate_flags(gamma):          # (experiments: the normalised rows stored as plain bf16)
        if split:
            _lo_view(y).zero_()
        else:
            y = y.to(torch.bfloat16).float()
    return y


# ------------------------------------------------------------------------------------------------ attention
class _Attention(Function):
    @staticmethod
    def forward(ctx, qt, kvt, cols, D, H, seq, key_mask, causal, drop):
        _need_gpu(qt)
        q_lo, kv_lo = lo_off(qt), lo_off(kvt)
        qt, kvt_c = _rows2d(qt), None
        same = kvt is qt or (kvt.data_ptr() == qt.data_ptr() and kvt.shape == qt.shape)
        kvt_c = qt if same else _rows2d(kvt)
        dh = D // H
        p, site, seed = _drop_args(drop)
        if qt.dtype == torch.float32 and kvt_c.dtype == torch.bfloat16:
            # ONE fp32 query per sequence against bf16 / split keys and values (the [CLS]-only clip-encoder layer): attention_q1s.hip
            # (the wrapper has checked the shape)
            es = 2
            out = torch.empty(seq.n_q_rows, D, dtype=torch.float32, device=qt.device)
            lse = torch.empty(seq.n, H, 1, dtype=torch.float32, device=qt.device)
            tbl = seq.table if seq.table.device == qt.device else seq.table.to(qt.device)
            ev1 = _attn_bracket("fwd", seq.n * H, seq.max_q, seq.max_k, 2 * seq.n_k_rows * D * (4 if kv_lo else 2)) if ATTN_TIMER is not None else None
            _lib.call("attn_q1s_fwd", qt.data_ptr() + cols[0] * 4, qt.stride(0), kvt_c.data_ptr() + cols[1] * es, kvt_c.stride(0), kv_lo or 0,
                      kvt_c.data_ptr() + cols[2] * es, kvt_c.stride(0), kv_lo or 0, _p(out), D, _p(lse), _p(tbl), seq.n, H, dh, seq.max_k,
                      _p(key_mask), 1.0 / math.sqrt(dh), p, site, _p(seed), _stream())
            if ev1 is not None:
                ev1.record()
            ctx.save_for_backward(qt, kvt_c, out, lse, key_mask, seed, tbl)
            ctx.cfg = (cols, D, H, seq.n, seq.max_q, seq.max_k, causal, p, site, False)
            ctx.kv_into = getattr(kvt, "_svpc_grad_into", None)
            ctx.mfma, ctx.q1s = False, (kv_lo or 0, True)
            ctx.n_k_rows = seq.n_k_rows
            return out
        ctx.q1s = None
        if kvt_c.dtype != qt.dtype:
            raise _lib.SvpcKernelError("attention: query and key/value tensors must have the same dtype")
        split = q_lo is not None
        if split != (kv_lo is not None):
            raise _lib.SvpcKernelError("attention: query and key/value tensors must both be split or both be plain")
        out = new_split(seq.n_q_rows, D, qt.device) if split else torch.empty(seq.n_q_rows, D, dtype=qt.dtype, device=qt.device)
        lse = torch.empty(seq.n, H, seq.max_q, dtype=torch.float32, device=qt.device)
        tbl = seq.table if seq.table.device == qt.device else seq.table.to(qt.device)
        es = qt.element_size()
        qp, kp, vp = qt.data_ptr() + cols[0] * es, kvt_c.data_ptr() + cols[1] * es, kvt_c.data_ptr() + cols[2] * es
        mfma = (_fast() and ((qp | kp | vp) & 15) == 0 and
                _lib.load().svpc_attn_mfma_supported(dh, seq.max_q, seq.max_k, qt.stride(0), kvt_c.stride(0), kvt_c.stride(0), _dt(qt)) == 1)
        fwd_done = False
        # incremental decoding (one query per sequence, nothing differentiates through it): a wave per (sequence, head), exact fp32.
        # (grad mode is always off INSIDE a Function.forward: what tells inference from training here is requires_grad of the inputs)
        use_q1 = (seq.max_q == 1 and p <= 0.0 and not causal and qt.dtype == torch.float32 and dh <= 64
                  and not (qt.requires_grad or kvt_c.requires_grad))
        # algorithmic bytes of this launch: Q, O rows and K, V rows of every (sequence, head), in their storage types
        ev1 = _attn_bracket("fwd", seq.n * H, seq.max_q, seq.max_k,
                            (2 * seq.n_q_rows + 2 * seq.n_k_rows) * D * (4 if split else es)) if ATTN_TIMER is not None else None
        if split:
            # bf16x3 stream (the wrapper has checked the shape): three-term products over the hi / lo planes; the backward is the
            # bf16 kernel on the hi planes
            if not mfma or (causal and (seq.max_q > 32 or seq.max_k > 32)):
                raise _lib.SvpcKernelError("attention: split tensors need the MFMA shape (head dim 32/64, ≤128 rows; causal: ≤32 rows)")
            _lib.call("attn_x3_fwd", qp, qt.stride(0), q_lo, kp, kvt_c.stride(0), kv_lo, vp, kvt_c.stride(0), kv_lo, _p(out),
                      out.stride(0), out._svpc_lo, _p(lse), _p(tbl), seq.n, H, dh, seq.max_q, seq.max_k, _p(key_mask), 1 if causal else 0,
                      1.0 / math.sqrt(dh), p, site, _p(seed), _stream())
            fwd_done = True
        elif is_x3() and qt.dtype == torch.float32 and not use_q1:
            # bf16x3 mode, fp32 storage (step encoder, decoder, the [CLS]-only layer): exact fp32 forward; the backward still runs
            # on the matrix cores when the shape allows (same LSE definition in both kernel families)
            _lib.call("attn_fwd", qp, qt.stride(0), kp, kvt_c.stride(0), vp, kvt_c.stride(0), _p(out), D, _p(lse), _p(tbl), seq.n, H,
                      dh, seq.max_q, seq.max_k, _p(key_mask), 1 if causal else 0, 1.0 / math.sqrt(dh), p, site, _p(seed), _stream())
            fwd_done = True
        if fwd_done:
            pass
        elif use_q1:
            # incremental decoding: one query per sequence — a wave per (sequence, head), no tiles, no LDS
            _lib.call("attn_q1_fwd", qp, qt.stride(0), kp, kvt_c.stride(0), vp, kvt_c.stride(0), _p(out), D, _p(lse), _p(tbl), seq.n, H,
                      dh, seq.max_k, _p(key_mask), 1.0 / math.sqrt(dh), _stream())
            mfma = False
        elif mfma:
            _lib.call("attn_mfma_fwd_t", qp, qt.stride(0), kp, kvt_c.stride(0), vp, kvt_c.stride(0), _p(out), D, _dt(qt), _p(lse),
                      _p(tbl), seq.n, H, dh, seq.max_q, seq.max_k, _p(key_mask), 1 if causal else 0, 1.0 / math.sqrt(dh), p, site,
                      _p(seed), _stream())
        else:
            if qt.dtype != torch.float32:
                raise _lib.SvpcKernelError("attention: the bf16 stream needs the MFMA kernel (head dim 32/64, ≤128 rows)")
            _lib.call("attn_fwd", qp, qt.stride(0), kp, kvt_c.stride(0), vp, kvt_c.stride(0), _p(out), D, _p(lse), _p(tbl), seq.n, H,
                      dh, seq.max_q, seq.max_k, _p(key_mask), 1 if causal else 0, 1.0 / math.sqrt(dh), p, site, _p(seed), _stream())
        if ev1 is not None:
            ev1.record()
        ctx.save_for_backward(qt, kvt_c, out, lse, key_mask, seed, tbl)
        ctx.cfg = (cols, D, H, seq.n, seq.max_q, seq.max_k, causal, p, site, same)
        ctx.kv_into = None if same else getattr(kvt, "_svpc_grad_into", None)     # a column block of a shared gradient buffer
        ctx.mfma = mfma and not (ATTN_BWD_EXACT and qt.dtype == torch.float32)
        ctx.n_k_rows = seq.n_k_rows
        return out

    @staticmethod
    def backward(ctx, dO):
        qt, kvt, out, lse, key_mask, seed, tbl = ctx.saved_tensors
        cols, D, H, n, max_q, max_k, causal, p, site, same = ctx.cfg
        dh = D // H
        dO = _c(dO)
        dev = dO.device
        def covered(t, used_cols, used_rows):
            full = t.shape[1] == used_cols and t.shape[0] == used_rows
            mk = torch.empty_like if full else torch.zeros_like
            return mk(t, memory_format=torch.contiguous_format)
        n_q_rows, n_k_rows = out.shape[0], ctx.n_k_rows
        if ctx.q1s is not None:
            kv_lo = ctx.q1s[0]
            dq_t = covered(qt, D, n_q_rows)
            into = ctx.kv_into
            if into is not None and into.shape == kvt.shape and into.dtype == kvt.dtype and kvt.shape == (n_k_rows, 2 * D):
                dkv_t = into
            else:
                dkv_t = covered(kvt, 2 * D, n_k_rows)
            _lib.call("attn_q1s_bwd", qt.data_ptr() + cols[0] * 4, qt.stride(0), kvt.data_ptr() + cols[1] * 2, kvt.stride(0), kv_lo,
                      kvt.data_ptr() + cols[2] * 2, kvt.stride(0), kv_lo, _p(dO), D, dq_t.data_ptr() + cols[0] * 4, dq_t.stride(0),
                      dkv_t.data_ptr() + cols[1] * 2, dkv_t.stride(0), dkv_t.data_ptr() + cols[2] * 2, dkv_t.stride(0), _p(tbl), n, H, dh,
                      max_k, _p(key_mask), 1.0 / math.sqrt(dh), p, site, _p(seed), _stream())
            return dq_t, dkv_t, None, None, None, None, None, None, None
        if same:
            dq_t = covered(qt, 3 * D, n_q_rows)
            dkv_t = dq_t
        else:
            dq_t = covered(qt, D, n_q_rows)
            into = ctx.kv_into
            if into is not None and into.shape == kvt.shape and into.dtype == kvt.dtype and kvt.shape == (n_k_rows, 2 * D):
                dkv_t = into                 # every element is written by the kernel below
            else:
                dkv_t = covered(kvt, 2 * D, n_k_rows)
        es = qt.element_size()
        # backward: Q, K, V, O, dO read, dQ, dK, dV written (their storage types: the hi planes in bf16x3 mode)
        ev1 = _attn_bracket("bwd", n * H, max_q, max_k, (3 * n_q_rows + 2 * n_k_rows + n_q_rows + 2 * n_k_rows) * D * es) \
            if ATTN_TIMER is not None else None
        if ctx.mfma:
            _lib.call("attn_mfma_bwd_t", qt.data_ptr() + cols[0] * es, qt.stride(0), kvt.data_ptr() + cols[1] * es, kvt.stride(0),
                      kvt.data_ptr() + cols[2] * es, kvt.stride(0), _p(out), out.stride(0), _dt(qt), _p(lse), _p(dO), D,
                      dq_t.data_ptr() + cols[0] * es, dq_t.stride(0), dkv_t.data_ptr() + cols[1] * es, dkv_t.stride(0),
                      dkv_t.data_ptr() + cols[2] * es, dkv_t.stride(0), _p(tbl), n, H, dh, max_q, max_k, _p(key_mask),
                      1 if causal else 0, 1.0 / math.sqrt(dh), p, site, _p(seed), _stream())
            if ev1 is not None:
                ev1.record()
            return dq_t, (None if same else dkv_t), None, None, None, None, None, None, None
        delta = torch.empty(n, H, max_q, dtype=torch.float32, device=dev)
        _lib.call("attn_bwd", qt.data_ptr() + cols[0] * es, qt.stride(0), kvt.data_ptr() + cols[1] * es, kvt.stride(0),
                  kvt.data_ptr() + cols[2] * es, kvt.stride(0), _p(out), D, _p(lse), _p(dO), D,
                  dq_t.data_ptr() + cols[0] * es, dq_t.stride(0), dkv_t.data_ptr() + cols[1] * es, dkv_t.stride(0),
                  dkv_t.data_ptr() + cols[2] * es, dkv_t.stride(0), _p(delta), _p(tbl), n, H, dh, max_q, max_k, _p(key_mask),
                  1 if causal else 0, 1.0 / math.sqrt(dh), p, site, _p(seed), _stream())
        return dq_t, (None if same else dkv_t), None, None, None, None, None, None, None


USE_Q1S = os.environ.get("SVPC_NO_Q1S", "") == ""
USE_P8W = os.environ.get("SVPC_NO_P8W", "") == ""                 # grouped stream wgrads on gemm_p8w.hip (else the round-1 ping-pong kernel)
USE_P8T = os.environ.get("SVPC_NO_P8T", "") == ""                 # stream dgrads on gemm_p8t.hip (else the round-1 ping-pong kernel)
P8T_MIN_TILES = int(os.environ.get("SVPC_P8T_MIN_TILES", "150"))   # 256² tiles needed to fill the chip
USE_S4T = os.environ.get("SVPC_NO_S4T", "") == ""                 # small-M stream dgrads (the decoder) on gemm_s4t.hip (128² tiles)
S4T_MIN_TILES = int(os.environ.get("SVPC_S4T_MIN_TILES", "64"))    # fewer 128² tiles: a long k-loop on a few CUs wants split-K (gemm_glds)
S4T_MAX_TILES = int(os.environ.get("SVPC_S4T_MAX_TILES", "640"))
X3_BIG_TILES = int(os.environ.get("SVPC_X3_BIG_TILES", "128"))      # fewer 256² tiles than this → the 128² split GEMM (gemm_s4x3.hip)


def attention(qt, kvt, cols, D, n_heads, seq, key_mask=None, causal=False, drop=None):
    require_split_tag(qt, "attention (queries)")
    require_split_tag(kvt, "attention (keys / values)")
    if qt.dtype == torch.float32 and kvt.dtype == torch.bfloat16 and kvt is not qt:
        # fp32 queries against bf16 / split keys and values: one query per sequence (the [CLS]-only layer) has its own exact kernels;
        # anything else joins one domain first
        dh = D // n_heads
        lo = lo_off(kvt) or 0
        if (USE_Q1S and _fast() and seq.max_q == 1 and not causal and qt.is_cuda and qt.stride(1) == 1 and kvt.stride(1) == 1 and
                (qt.data_ptr() | kvt.data_ptr()) % 16 == 0 and
                _lib.load().svpc_attn_q1s_supported(dh, seq.max_k, qt.stride(0), kvt.stride(0), kvt.stride(0), lo, lo) == 1):
            return _Attention.apply(qt, kvt, cols, D, n_heads, seq, key_mask, causal, drop)
        if lo_off(kvt) is not None:
            kvt = to_f32(kvt)
        else:
            qt = qt.to(torch.bfloat16)
    split = lo_off(qt) is not None or lo_off(kvt) is not None
    if ABLATE is not None and split and kvt is qt and ABLATE.get("attn"):      # (experiments: Q / K or V operands of the clip encoder's core
        flags = ABLATE["attn"] if seq.max_q > 32 else ""                      # without their lo planes)
        if flags:
            assert not torch.is_grad_enabled()
            c = new_split(qt.shape[0], qt.shape[1], qt.device)
            c.copy_(qt.detach()); _lo_view(c).copy_(_lo_view(qt))
            lo = _lo_view(c)
            if "q" in flags:
                lo[:, cols[0]:cols[0] + D].zero_()
            if "k" in flags:
                lo[:, cols[1]:cols[1] + D].zero_()
            if "v" in flags:
                lo[:, cols[2]:cols[2] + D].zero_()
            qt = kvt = c
    if split:
        dh = D // n_heads
        # (the same conditions _Attention.forward demands of a split stream, 16-byte aligned column blocks included: what fails them
        # leaves the split domain here instead of raising there)
        ok = ((not causal or (seq.max_q <= 32 and seq.max_k <= 32)) and lo_off(qt) is not None and lo_off(kvt) is not None and
              _lib.load().svpc_attn_mfma_supported(dh, seq.max_q, seq.max_k, 8, 8, 8, 1) == 1 and qt.stride(0) % 8 == 0 and kvt.stride(0) % 8 == 0 and
              ((qt.data_ptr() + cols[0] * 2) | (kvt.data_ptr() + cols[1] * 2) | (kvt.data_ptr() + cols[2] * 2)) % 16 == 0)
        if not ok:          # leave the split domain: exact fp32 attention on fp32 copies
            same = kvt is qt
            qt = to_f32(qt)
            kvt = qt if same else to_f32(kvt)
            split = False
    if kvt.requires_grad and torch.is_grad_enabled() and seq.shares_keys:
        raise _lib.SvpcKernelError("attention: sequences that share key / value rows have no backward (every sequence writes its own dK / dV "
                                   "rows: they would be overwritten, not summed) — replicate the rows through a differentiable gather")
    out = _Attention.apply(qt, kvt, cols, D, n_heads, seq, key_mask, causal, drop)
    if split:
        out._svpc_lo = out.shape[1]
    return out


class _SplitCols(Function):
    """One wide projection output (R, n·w) handed out as n column blocks (views, row stride n·w).  The gradient of the wide
    tensor is ONE buffer allocated up front: a consumer that finds ``_svpc_grad_into`` on its block (ops.attention does) writes
    its gradient straight into that block's columns and returns the view, so backward neither concatenates nor adds."""

    @staticmethod
    def forward(ctx, wide, n, gbuf):
        w = wide.shape[1] // n
        ctx.gbuf, ctx.n, ctx.w = gbuf, n, w
        return tuple(wide[:, i * w:(i + 1) * w] for i in range(n))

    @staticmethod
    def backward(ctx, *grads):
        g, w = ctx.gbuf, ctx.w
        for i, gi in enumerate(grads):
            blk = g[:, i * w:(i + 1) * w]
            if gi is None:
                blk.zero_()
            elif gi.data_ptr() != blk.data_ptr() or gi.stride() != blk.stride():
                blk.copy_(gi)
        ctx.gbuf = None
        return g, None, None


def attn_q1_ln(q, kv, k_stride, n_keys, residual, gamma, beta, eps, n_heads, new_kv=None, key_rows=None, q_group=1):
    """One decoding step of an attention block (reference decoder layer model.py:620-663 for one new position per sentence,
    translator.py:88-112): LayerNorm(residual + Attention(q; the sentence's key / value rows)), one launch.  ``q``: (T, ≥D) fp32, the
    query in its first D columns; ``kv``: (rows, 2D) fp32, K | V, sentence t owning rows t·k_stride … t·k_stride + n_keys − 1;
    ``new_kv`` (T, 2D view): the token's own K | V, stored as the sentence's row n_keys − 1 first (the cache append).  Forward only.
    Beam search (svpc_attn_q1_ln_idx_fwd): ``key_rows`` ((T, ≥ n_keys) int32, the ancestry table of ``beam_step``) names the kv rows of
    query t — the new row goes to key_rows[t, n_keys − 1]; without a table, ``q_group`` > 1 lets queries t read the rows of t // q_group.
    Returns None when the shape is not taken (the caller then runs copy / attention / layernorm separately)."""
    T, D = residual.shape
    indexed = key_rows is not None or q_group != 1
    if key_rows is not None:
        if not (key_rows.dtype == torch.int32 and key_rows.is_contiguous() and key_rows.dim() == 2 and key_rows.shape[0] == T
                and key_rows.shape[1] >= n_keys and key_rows.device == residual.device):
            raise ValueError("attn_q1_ln: key_rows must be a contiguous int32 (T, >= n_keys) table on the rows' device")
    elif q_group != 1 and (q_group < 1 or T % q_group or kv.shape[0] < (T // q_group) * k_stride):
        raise ValueError("attn_q1_ln: q_group must divide T and the kv rows must cover T / q_group sentences")
    if torch.is_grad_enabled() and (q.requires_grad or residual.requires_grad):
        return None
    ts = (q, kv, residual) + ((new_kv,) if new_kv is not None else ())
    if not all(t.is_cuda and t.dtype == torch.float32 and lo_off(t) is None and t.stride(1) == 1 for t in ts) or D % n_heads:
        return None
    lib = _lib.load()
    ldn = new_kv.stride(0) if new_kv is not None else 0
    if lib.svpc_attn_q1_ln_supported(D, D // n_heads, n_keys, q.stride(0), kv.stride(0), ldn, residual.stride(0), D) != 1:
        return None
    if any(t.data_ptr() % 16 for t in ts) or kv.shape[1] != 2 * D or k_stride < n_keys:
        return None
    out = torch.empty(T, D, dtype=torch.float32, device=q.device)
    nk = new_kv.data_ptr() if new_kv is not None else None
    if indexed:
        _lib.call("attn_q1_ln_idx_fwd", _p(q), q.stride(0), kv.data_ptr(), kv.data_ptr() + 4 * D, kv.stride(0), k_stride, n_keys, _p(key_rows),
                  key_rows.shape[1] if key_rows is not None else 0, int(q_group), nk, (nk + 4 * D) if nk is not None else None, ldn,
                  _p(residual), residual.stride(0), _p(gamma), _p(beta), float(eps), _p(out), D, T, D, D // n_heads, 1.0 / math.sqrt(D // n_heads),
                  _stream())
        return out
    _lib.call("attn_q1_ln_fwd", _p(q), q.stride(0), kv.data_ptr(), kv.data_ptr() + 4 * D, kv.stride(0), k_stride, n_keys, nk,
              (nk + 4 * D) if nk is not None else None, ldn, _p(residual), residual.stride(0), _p(gamma), _p(beta), float(eps), _p(out), D, T, D,
              D // n_heads, 1.0 / math.sqrt(D // n_heads), _stream())
    return out


def split_cols(wide, n):
    """→ n column blocks of ``wide`` (R, n·w) whose gradients are gathered in place (see _SplitCols).  A split ``wide`` gives split
    blocks: the lo plane of a block lies the same number of columns behind it as the lo plane of the whole row."""
    lo = lo_off(wide)
    w = wide.shape[1] // n
    if not (torch.is_grad_enabled() and wide.requires_grad):
        outs = tuple(wide[:, i * w:(i + 1) * w] for i in range(n))
    else:
        gbuf = torch.empty(wide.shape, dtype=wide.dtype, device=wide.device)
        outs = _SplitCols.apply(wide, n, gbuf)
        for i, o in enumerate(outs):
            o._svpc_grad_into = gbuf[:, i * w:(i + 1) * w]
    if lo is not None:
        for o in outs:
            o._svpc_lo = lo
    return outs


def to_split(t):
    """split copy (two bf16 planes) of an fp32 2-D tensor joining a bf16x3 stream (a handful of rows: the decoder's memory slots);
    the gradient comes back as the dense bf16 tensor every split tensor has"""
    y = _ToSplit.apply(t)
    y._svpc_lo = t.shape[1]
    return y


class _ToSplit(Function):
    @staticmethod
    def forward(ctx, t):
        out = new_split(t.shape[0], t.shape[1], t.device)
        if t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.dtype == torch.float32:
            _rows_move(t, None, None, out, out._svpc_lo, t.shape[0], t.shape[1])
            return out
        out.copy_(t)
        torch.as_strided(out, out.shape, out.stride(), out.storage_offset() + out._svpc_lo).copy_(t - out.float())
        return out

    @staticmethod
    def backward(ctx, g):
        return g.float()


# ------------------------------------------------------------------------------------------------ decoder cross-attention, fused
# Cross-attention of every sentence row to the ≤ 3 memory rows of its sentence + residual + LayerNorm in ONE launch, forward and backward
# (svpc_amd/csrc/cross_attn.hip; reference model.py:657-658 in :630-663; SURVEY §2.3 K6 "trivial; fuse").
USE_XATTN = os.environ.get("SVPC_NO_XATTN", "") == ""


def cross_attn_ln_usable(D, H, lt, nm, mem_mask=None):
    return (USE_XATTN and mem_mask is None and H > 0 and D % H == 0
            and _lib.load().svpc_cross_attn_ln_supported(int(D), int(H), int(lt), int(nm)) == 1)


def _kind(t):
    """storage code of the C-ABI: 0 fp32, 1 bf16, 2 split"""
    return 2 if lo_off(t) is not None else _dt(t)


class _CrossAttnLn(Function):
    @staticmethod
    def forward(ctx, q, x1, kv, gamma, beta, eps, H, lt, nm, drop, sink, rows=None):
        _need_gpu(q)
        D = gamma.shape[0]
        R = q.shape[0]
        T = R // lt if rows is None else rows[0].numel()       # rows = (row_off, row_len) int32 device tensors: ragged sentences
        ro, rl = rows if rows is not None else (None, None)
        dev = q.device
        out_kind = _kind(x1)
        if out_kind == 2:
            y = new_split(R, D, dev)
            loy = y._svpc_lo
        else:
            y = torch.empty(R, D, dtype=x1.dtype, device=dev)
            loy = 0
        probs = torch.empty(R, H, 4, dtype=torch.float32, device=dev)
        mean = torch.empty(R, dtype=torch.float32, device=dev)
        rstd = torch.empty(R, dtype=torch.float32, device=dev)
        p, site, seed = _drop_args(drop)
        scale = 1.0 / math.sqrt(D // H)
        es = kv.element_size()
        _lib.call("cross_attn_ln_fwd_r", _p(q), _kind(q), q.stride(0), lo_off(q) or 0, _p(x1), out_kind, x1.stride(0), lo_off(x1) or 0,
                  kv.data_ptr(), kv.data_ptr() + D * es, _kind(kv), kv.stride(0), lo_off(kv) or 0, _p(gamma), _p(beta), float(eps),
                  _p(y), out_kind, y.stride(0), loy, _p(probs), _p(mean), _p(rstd), T, lt, nm, D, H, scale, p, site, _p(seed), _p(ro), _p(rl),
                  _stream())
        ctx.save_for_backward(q, x1, kv, gamma, probs, mean, rstd, seed, ro, rl)
        ctx.cfg = (T, lt, nm, D, H, scale, p, site, _kind(q), lo_off(q) or 0, out_kind, lo_off(x1) or 0, _kind(kv), lo_off(kv) or 0)
        ctx.kv_into = getattr(kv, "_svpc_grad_into", None)
        ctx.direct = (_direct(gamma), _direct(beta))
        ctx.sink = bool(sink)
        return y

    @staticmethod
    def backward(ctx, dy):
        q, x1, kv, gamma, probs, mean, rstd, seed, ro, rl = ctx.saved_tensors
        T, lt, nm, D, H, scale, p, site, q_dt, q_lo, x_dt, x_lo, kv_dt, kv_lo = ctx.cfg
        dev = dy.device
        dy = _c(dy)
        R = q.shape[0]
        dq = torch.empty(R, D, dtype=dy.dtype, device=dev)
        dres = torch.empty(R, D, dtype=dy.dtype, device=dev)
        into = ctx.kv_into
        if into is not None and into.shape == kv.shape and into.dtype == kv.dtype:
            dkv = into                                 # the layer's block of the stacked projection's gradient buffer: written in place
        else:
            dkv = torch.empty(kv.shape, dtype=kv.dtype, device=dev)
        part_ln = torch.empty(T, 2 * D, dtype=torch.float32, device=dev)
        es = dkv.element_size()
        _lib.call("cross_attn_ln_bwd_r", _p(q), q_dt, q.stride(0), q_lo, _p(x1), x_dt, x1.stride(0), x_lo, kv.data_ptr(),
                  kv.data_ptr() + D * kv.element_size(), kv_dt, kv.stride(0), kv_lo, _p(gamma), _p(probs), _p(mean), _p(rstd), _p(dy), _dt(dy),
                  dy.stride(0), _p(dq), _p(dres), _dt(dq), dq.stride(0), dkv.data_ptr(), dkv.data_ptr() + D * es, _dt(dkv), dkv.stride(0),
                  _p(part_ln), T, lt, nm, D, H, scale, p, site, _p(seed), _p(ro), _p(rl), _stream())
        g_d, b_d = ctx.direct
        dgamma = dbeta = None
        if not defer_partials(part_ln, T, 2 * D, g_d, b_d, D):
            sl = _colsum(part_ln).view(-1)
            dgamma, dbeta = sl[:D].clone(), sl[D:].clone()
            if g_d is not None:
                g_d.add_(dgamma); dgamma = None
            if b_d is not None:
                b_d.add_(dbeta); dbeta = None
        if ctx.sink and USE_RES_SINK and (dres.dtype == torch.bfloat16 or (_fast() and USE_L32)):
            _RES_SINK[x1.data_ptr()] = dres            # joins the dgrad of the query projection, the other consumer of x1 (see _RES_SINK)
            SINK_STATS[0] += 1
            _queue_end_of_backward_join()
            dres = None
        return dq, dres, dkv, dgamma, dbeta, None, None, None, None, None, None, None


def cross_attn_ln(q, x1, kv, gamma, beta, eps, n_heads, lt, nm, drop=None, sink=False, rows=None):
    """LayerNorm(x1 + CrossAttention(q; the sentence's nm memory rows)) in one launch — q, x1 (T·lt, D) fp32 / bf16 / split; kv (T·nm, 2D)
    [K | V] rows of the same storage family (may be a column block of the stacked memory projection).  Output in x1's storage kind.
    rows = (row_off, row_len): ragged sentences (valid tokens only) — sentence s owns rows [row_off[s], row_off[s] + row_len[s]), ≤ lt each.
    sink=True: x1's only other consumer is the ops.linear that produced q — its dgrad absorbs the residual-path gradient (_RES_SINK)."""
    require_split_tag(q, "cross_attn_ln (queries)")
    require_split_tag(x1, "cross_attn_ln (residual)")
    require_split_tag(kv, "cross_attn_ln (memory rows)")
    y = _CrossAttnLn.apply(q, x1, kv, gamma, beta, float(eps), int(n_heads), int(lt), int(nm), drop, sink, rows)
    if lo_off(x1) is not None:
        y._svpc_lo = y.shape[1]
    return y


# ------------------------------------------------------------------------------------------------ spans / rows
class _SpanMean(Function):
    @staticmethod
    def forward(ctx, x, starts, lens, weights, add, add_idx):
        _need_gpu(x)
        x = _c(x)
        G, D = len(starts), x.shape[1]
        dev = x.device
        out = torch.empty(G, D, dtype=torch.float32, device=dev)
        st, ln = starts.dev(dev), lens.dev(dev)
        ai = add_idx.dev(dev) if add is not None else None
        _lib.call("span_mean_fwd", _p(x), _p(st), _p(ln), _p(weights), _p(add), _p(ai), _p(out), G, D, _stream())
        ctx.save_for_backward(st, ln, weights)
        ctx.cfg = (tuple(x.shape), G, D)
        ctx.tiles = _spans_tile(starts, lens, x.shape[0])       # the spans cover every row exactly once: the backward writes all of dx
        return out

    @staticmethod
    def backward(ctx, dout):
        st, ln, weights = ctx.saved_tensors
        shape, G, D = ctx.cfg
        dout = _c(dout)
        dx = (torch.empty if ctx.tiles else torch.zeros)(shape, dtype=torch.float32, device=dout.device)
        _lib.call("span_mean_bwd", _p(dout), _p(st), _p(ln), _p(weights), _p(dx), G, D, _stream())
        return dx, None, None, None, None, None


_TILES = {}


def _spans_tile(starts, lens, n_rows):
    """whether the spans (host lists of two ``Idx``) are consecutive and cover rows 0..n_rows-1 exactly; cached per Idx pair"""
    key = (id(starts), id(lens), n_rows)
    hit = _TILES.get(key)
    if hit is not None and hit[0] is starts and hit[1] is lens:
        return hit[2]
    pos, ok = 0, True
    for s_, l_ in zip(starts.host, lens.host):
        if s_ != pos or l_ < 1:
            ok = False
            break
        pos += l_
    ok = ok and pos == n_rows
    if len(_TILES) > 256:
        _TILES.clear()
    _TILES[key] = (starts, lens, ok)
    return ok


def span_mean(x, starts, lens, weights=None, add=None, add_idx=None):
    return _SpanMean.apply(x, as_idx(starts), as_idx(lens), weights, add, as_idx(add_idx) if add_idx is not None else None)


class _RowNorm(Function):
    @staticmethod
    def forward(ctx, a, mode):
        _need_gpu(a)
        a = _c(a)
        y = torch.empty_like(a)
        _lib.call("rownorm_fwd", _p(a), _p(y), a.shape[0], a.shape[1], mode, _stream())
        ctx.save_for_backward(a, y)
        ctx.mode = mode
        return y

    @staticmethod
    def backward(ctx, dy):
        a, y = ctx.saved_tensors
        dy = _c(dy)
        da = torch.empty_like(a)
        _lib.call("rownorm_bwd", _p(dy), _p(y), _p(a), _p(da), a.shape[0], a.shape[1], ctx.mode, _stream())
        return da, None


def row_normalize(a):
    return _RowNorm.apply(a, 0)


def softmax_rows(x):
    return _RowNorm.apply(x, 1)


class _SumAll(Function):
    @staticmethod
    def forward(ctx, x):
        _need_gpu(x)
        x = _c(x)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        _lib.call("sum_all", _p(x), x.numel(), _p(out), 1.0, _stream())
        ctx.shape = tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=dout.device)
        _lib.call("fill_from", _p(dx), dx.numel(), _p(_c(dout)), _stream())
        return dx


def sum_all(x):
    return _SumAll.apply(x)


class _Add(Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _c(a), _c(b)
        c = torch.empty_like(a)
        _lib.call("add", _p(a), _p(b), _p(c), a.numel(), _stream())
        return c

    @staticmethod
    def backward(ctx, d):
        return d, d


def add(a, b):
    return _Add.apply(a, b)


def take_rows(x, idx):
    """Row gather (data movement only)."""
    return torch.index_select(x, 0, idx)


class _GcSeg(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("idx", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("src_dt", ctypes.c_int),
                ("dst_dt", ctypes.c_int), ("n", ctypes.c_int)]


_GC_CODE = {torch.float32: 0, torch.int64: 1, torch.int32: 2}


def gather_cast_multi(items, rng=None):
    """items: [(src 1-D tensor, int32 row index or None, torch.float32 | torch.int32)] → [dst]; dst[i] = cast(src[idx[i]]) for all
    items in ONE launch (data movement only, no gradient) — the token staging of the batched forward.  rng: advance its seed in the
    same launch (``rng.begin_step(defer=True)`` was called)."""
    outs, segs = [], []
    for src, idx, dt in items:
        src = _c(src.reshape(-1))
        if src.dtype not in _GC_CODE:
            src = src.to(torch.float32 if src.dtype.is_floating_point else torch.int64)
        n = idx.numel() if idx is not None else src.numel()
        dst = torch.empty(n, dtype=dt, device=src.device)
        outs.append(dst)
        segs.append((src, idx, dst))
    for k in range(0, len(segs), 8):
        part = segs[k:k + 8]
        arr = (_GcSeg * len(part))()
        for i, (src, idx, dst) in enumerate(part):
            arr[i] = _GcSeg(src.data_ptr(), idx.data_ptr() if idx is not None else None, dst.data_ptr(), _GC_CODE[src.dtype],
                            _GC_CODE[dst.dtype], dst.numel())
        _lib.call("gather_cast_multi_seed", ctypes.addressof(arr), len(part), _p(rng.seed) if (rng is not None and k == 0) else None, _stream())
    if rng is not None and not segs:
        _lib.call("bump_seed", _p(rng.seed), _stream())
    return outs


def clamp_labels(labels, vocab, unk):
    out = torch.empty_like(labels)
    _lib.call("clamp_labels", _p(labels), _p(out), labels.numel(), int(vocab), int(unk), _stream())
    return out


def row_any_eq1(x):
    x = _c(x)
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    _lib.call("row_any_eq1", _p(x), _p(out), x.shape[0], x.shape[1], _stream())
    return out


# ------------------------------------------------------------------------------------------------ simulator recurrence
class _SimRecur(Function):
    @staticmethod
    def forward(ctx, q, c, w4f, E0, step_off, step_len, ent_off, ent_len, e_max):
        _need_gpu(q)
        q, c, w4f, E0 = _c(q), _c(c), _c(w4f), _c(E0)
        T, D = q.shape
        dev = q.device
        idx = [v.dev(dev) for v in (step_off, step_len, ent_off, ent_len)]
        e = torch.empty(T, e_max, dtype=torch.float32, device=dev)
        ebar = torch.empty(T, D, dtype=torch.float32, device=dev)
        eall = torch.empty(T, e_max, D, dtype=torch.float32, device=dev)
        _lib.call("sim_recur_fwd", _p(q), _p(c), _p(w4f), _p(E0), _p(idx[0]), _p(idx[1]), _p(idx[2]), _p(idx[3]), len(step_off), e_max,
                  D, _p(e), _p(ebar), _p(eall), _stream())
        ctx.save_for_backward(q, c, w4f, E0, e, ebar, eall, *idx)
        ctx.cfg = (len(step_off), e_max, D)
        ctx.set_materialize_grads(False)
        return e, ebar, eall

    @staticmethod
    def backward(ctx, de, debar, deall):
        q, c, w4f, E0, e, ebar, eall, so, sl, eo, el = ctx.saved_tensors
        n, e_max, D = ctx.cfg
        dev = q.device
        de = _c(de) if de is not None else None
        debar = _c(debar) if debar is not None else None
        deall = _c(deall) if deall is not None else None
        dq = torch.empty_like(q)
        dc = torch.empty_like(c)
        dw = torch.empty_like(w4f)
        dE0 = torch.empty_like(E0)
        _lib.call("sim_recur_bwd", _p(q), _p(c), _p(w4f), _p(E0), _p(so), _p(sl), _p(eo), _p(el), n, e_max, D, _p(e), _p(ebar),
                  _p(eall), _p(de), _p(debar), _p(deall), _p(dq), _p(dc), _p(dw), _p(dE0), _stream())
        return dq, dc, dw, dE0, None, None, None, None, None


def sim_recur(q, c, w4f, E0, step_off, step_len, ent_off, ent_len, e_max):
    return _SimRecur.apply(q, c, w4f, E0, as_idx(step_off), as_idx(step_len), as_idx(ent_off), as_idx(ent_len), int(e_max))


class _SimHeads(Function):
    """c = softmax(ĥ·W3ᵀ + b3), w = f̄·W4ᵀ + b4 (reference model.py:801, :804-805) in one launch; backward in one launch (svpc_sim_heads_*)."""

    @staticmethod
    def forward(ctx, hh, fb, W3, b3, W4, b4):
        _need_gpu(hh)
        hh, fb, W3, W4 = _c(hh), _c(fb), _c(W3), _c(W4)
        T, D = hh.shape
        Wd = fb.shape[1]
        c = torch.empty(T, 3, dtype=torch.float32, device=hh.device)
        w = torch.empty(T, dtype=torch.float32, device=hh.device)
        _lib.call("sim_heads_fwd", _p(hh), _p(fb), _p(W3), _p(b3), _p(W4), _p(b4), _p(c), _p(w), T, D, Wd, _stream())
        ctx.save_for_backward(hh, fb, W3, W4, c)
        ctx.direct = (_direct(W3), _direct(b3), _direct(W4), _direct(b4))
        ctx.set_materialize_grads(False)
        return c, w

    @staticmethod
    def backward(ctx, dc, dw):
        hh, fb, W3, W4, c = ctx.saved_tensors
        T, D = hh.shape
        Wd = fb.shape[1]
        dev = hh.device
        dc = _c(dc) if dc is not None else None
        dw = _c(dw) if dw is not None else None
        G = _lib.load().svpc_sim_heads_groups(T)
        dhh, dfb = torch.empty_like(hh), torch.empty_like(fb)
        p3 = torch.empty(G, 3 * D + 3, dtype=torch.float32, device=dev)
        p4 = torch.empty(G, Wd + 1, dtype=torch.float32, device=dev)
        _lib.call("sim_heads_bwd", _p(hh), _p(fb), _p(W3), _p(W4), _p(c), _p(dc), _p(dw), _p(dhh), _p(dfb), _p(p3), _p(p4), T, D, Wd, _stream())
        w3d, b3d, w4d, b4d = ctx.direct
        if all(t is not None for t in ctx.direct):
            defer_partials(p3, G, 3 * D + 3, w3d, b3d, 3 * D)
            defer_partials(p4, G, Wd + 1, w4d, b4d, Wd)
            return dhh, dfb, None, None, None, None
        s3, s4 = _colsum(p3).view(-1), _colsum(p4).view(-1)
        outs = [s3[:3 * D].reshape(3, D), s3[3 * D:].clone(), s4[:Wd].reshape(1, Wd), s4[Wd:].clone()]
        res = []
        for tgt, val in zip(ctx.direct, outs):
            if tgt is not None:
                tgt.add_(val.view_as(tgt)); res.append(None)
            else:
                res.append(val)
        return (dhh, dfb) + tuple(res)


def sim_heads(hh, fb, W3, b3, W4, b4):
    """(c (T, 3), w (T,)) — the simulator's choice softmax and verb scalar; None when the shape is not taken"""
    if (not hh.is_cuda or hh.dtype != torch.float32 or fb.dtype != torch.float32 or tuple(W3.shape) != (3, hh.shape[1]) or
            tuple(W4.shape) != (1, fb.shape[1]) or hh.shape[1] > 1024 or fb.shape[1] > 512 or b3 is None or b4 is None):
        return None
    return _SimHeads.apply(hh, fb, W3, b3, W4, b4)


# ------------------------------------------------------------------------------------------------ pointer-generator
class _PtrAttn(Function):
    @staticmethod
    def forward(ctx, dec, proj, bank, step_ne, lt):
        _need_gpu(dec)
        dec, proj, bank = _c(dec), _c(proj), _c(bank)
        T, e_max, D = bank.shape
        dev = dec.device
        ne = step_ne.dev(dev)
        pi = torch.empty(T * lt, e_max, dtype=torch.float32, device=dev)
        att = torch.empty(T * lt, D, dtype=torch.float32, device=dev)
        _lib.call("ptr_attn_fwd", _p(dec), _p(proj), _p(bank), _p(ne), _p(pi), _p(att), T, lt, e_max, D, _stream())
        ctx.save_for_backward(dec, proj, bank, ne, pi)
        ctx.cfg = (T, lt, e_max, D)
        ctx.set_materialize_grads(False)
        return pi, att

    @staticmethod
    def backward(ctx, dpi, datt):
        dec, proj, bank, ne, pi = ctx.saved_tensors
        T, lt, e_max, D = ctx.cfg
        if datt is None:
            datt = torch.zeros(T * lt, D, dtype=torch.float32, device=dec.device)
        datt = _c(datt)
        dpi = _c(dpi) if dpi is not None else None
        ddec = torch.empty_like(dec)
        dproj = torch.empty_like(proj)
        dbank = torch.empty_like(bank)
        _lib.call("ptr_attn_bwd", _p(dec), _p(proj), _p(bank), _p(ne), _p(pi), _p(dpi), _p(datt), _p(ddec), _p(dproj), _p(dbank), T, lt,
                  e_max, D, _stream())
        return ddec, dproj, dbank, None, None


def ptr_attn(dec, proj, bank, step_ne, lt):
    return _PtrAttn.apply(dec, proj, bank, as_idx(step_ne), int(lt))


class _PtrAttnGate(Function):
    """Pointer attention + generation gate of every row in one launch, forward and backward (svpc_ptr_attn_gate_fwd/bwd): the attended
    vector feeds only the gate (model.py:903-908), so neither it nor the [dec ; att] concatenation nor the gate's 1,536-deep one-column
    projection (with its dgrad / wgrad / bias-sum launches) exist."""

    @staticmethod
    def forward(ctx, dec, proj, bank, w, b, step_ne, lt, rows=None):
        _need_gpu(dec)
        dec, proj, bank, w = _c(dec), _c(proj), _c(bank), _c(w)
        T, e_max, D = bank.shape
        dev = dec.device
        ne = step_ne.dev(dev)
        ro, rl = rows if rows is not None else (None, None)      # ragged sentences: (row_off, row_len) int32 device tensors
        R = dec.shape[0]
        pi = torch.empty(R, e_max, dtype=torch.float32, device=dev)
        g = torch.empty(R, 1, dtype=torch.float32, device=dev)
        _lib.call("ptr_attn_gate_fwd_r", _p(dec), _p(proj), _p(bank), _p(ne), _p(pi), _p(w), _p(b), _p(g), T, lt, e_max, D, _p(ro), _p(rl),
                  _stream())
        ctx.save_for_backward(dec, proj, bank, w, ne, pi, g, ro, rl)
        ctx.cfg = (T, lt, e_max, D)
        ctx.direct = (_direct(w), _direct(b))
        ctx.set_materialize_grads(False)
        return pi, g

    @staticmethod
    def backward(ctx, dpi, dg):
        dec, proj, bank, w, ne, pi, g, ro, rl = ctx.saved_tensors
        T, lt, e_max, D = ctx.cfg
        dev = dec.device
        dpi = _c(dpi) if dpi is not None else None
        dg = _c(dg) if dg is not None else None
        ddec, dproj, dbank = torch.empty_like(dec), torch.empty_like(proj), torch.empty_like(bank)
        wpart = torch.empty(T, 2 * D + 1, dtype=torch.float32, device=dev)
        _lib.call("ptr_attn_gate_bwd_r", _p(dec), _p(proj), _p(bank), _p(ne), _p(pi), _p(dpi), _p(g), _p(dg), _p(w), _p(ddec), _p(dproj),
                  _p(dbank), _p(wpart), T, lt, e_max, D, _p(ro), _p(rl), _stream())
        wg, bg = ctx.direct
        dw = db = None
        if not defer_partials(wpart, T, 2 * D + 1, wg, bg, 2 * D):      # (else: with every other pending tail)
            sums = _colsum(wpart).view(-1)
            dw, db = sums[:2 * D].reshape(1, 2 * D), sums[2 * D:]
            if wg is not None:
                wg.add_(dw); dw = None
            if bg is not None:
                bg.add_(db); db = None
        return ddec, dproj, dbank, dw, db, None, None, None


def ptr_attn_gate(dec, proj, bank, step_ne, lt, w, b, rows=None):
    """(pi (T·lt, e_max), p_gen (T·lt, 1)) with p_gen = sigmoid([dec ; att]·wᵀ + b), att = Σ_e pi·bank — training form (differentiable
    in dec, proj, bank, w, b); None when the shape is not taken (the caller then uses ptr_attn + linear).  rows = (row_off, row_len): ragged
    sentences (valid tokens only) — sentence j owns the dec rows [row_off[j], row_off[j] + row_len[j]), ≤ lt each."""
    T, e_max, D = bank.shape
    if (not dec.is_cuda or dec.dtype != torch.float32 or D % 4 or tuple(w.shape) != (1, 2 * D) or b is None or b.numel() != 1
            or lt > 32 or e_max > 32 or (rows is None and dec.shape != (T * lt, D)) or dec.shape[1] != D or w.dtype != torch.float32
            or (w.data_ptr() % 16) or lo_off(dec) is not None):
        return None
    return _PtrAttnGate.apply(dec, proj, bank, w, b, as_idx(step_ne), int(lt), rows)


def ptr_attn_pgen(dec, proj, bank, step_ne, w, b):
    """Decoding iteration (one position per step row, no gradients): (pi, p_gen) with p_gen = sigmoid([dec ; att]·w + b) computed inside
    the pointer-attention launch — replaces ptr_attn + concatenation + the 1,536-deep one-column projection.  None if not applicable."""
    T, e_max, D = bank.shape
    if (torch.is_grad_enabled() or not dec.is_cuda or dec.dtype != torch.float32 or D > 768 or D % 4 or w.shape != (1, 2 * D)
            or dec.shape != (T, D) or not (dec.is_contiguous() and proj.is_contiguous() and bank.is_contiguous() and w.is_contiguous())):
        return None
    dev = dec.device
    pi = torch.empty(T, e_max, dtype=torch.float32, device=dev)
    g = torch.empty(T, 1, dtype=torch.float32, device=dev)
    _lib.call("ptr_attn_pgen_fwd", _p(dec), _p(proj), _p(bank), _p(as_idx(step_ne).dev(dev)), _p(pi), None, _p(w), _p(b), _p(g), T, 1, e_max, D,
              _stream())
    return pi, g


class _PtrMixLoss(Function):
    @staticmethod
    def forward(ctx, logits, g, pi, labels, row_c, row_vid, csr_off, csr_ent, csr_id, csr_w, c_max, smoothing):
        _need_gpu(logits)
        logits = _c(logits)
        R, V = logits.shape
        dev = logits.device
        g = _c(g) if g is not None else None
        pi = _c(pi) if pi is not None else None
        e_max = pi.shape[1] if pi is not None else 0
        rc, rv = row_c.dev(dev), row_vid.dev(dev)
        co, ce, ci, cw = csr_off.dev(dev), csr_ent.dev(dev), csr_id.dev(dev), csr_w.dev(dev)
        P = torch.empty(R, c_max, dtype=torch.float32, device=dev)
        loss_rows = torch.empty(R, dtype=torch.float32, device=dev)
        row_w = None
        if not smoothing > 0:
            # label_smoothing == 0 (reference model.py:869-870): cross-entropy of the probabilities, a mean per video → per-row weights
            row_w = torch.empty(R, dtype=torch.float32, device=dev)
            _lib.call("ce_row_weights", _p(labels), _p(rv), R, len(csr_off) - 1, _p(row_w), _stream())
        _lib.call("ptr_mix_ce_fwd", _p(logits), _p(g), _p(pi), _p(labels), _p(rc), _p(rv), _p(co), _p(ce), _p(ci), _p(cw), _p(P),
                  _p(loss_rows), R, V, c_max, e_max, float(smoothing), _p(row_w), _stream())
        ctx.save_for_backward(logits, g, pi, labels, rc, rv, co, ce, ci, cw, P, row_w)
        ctx.cfg = (R, V, c_max, e_max, float(smoothing))
        ctx.set_materialize_grads(False)
        return P, loss_rows

    @staticmethod
    def backward(ctx, dP, dloss):
        logits, g, pi, labels, rc, rv, co, ce, ci, cw, P, row_w = ctx.saved_tensors
        R, V, c_max, e_max, smoothing = ctx.cfg
        dev = logits.device
        dP = _c(dP) if dP is not None else None
        if dloss is None:
            dloss = torch.zeros(R, dtype=torch.float32, device=dev)
        dloss = _c(dloss)
        dlogits = torch.empty_like(logits)
        dg = torch.empty_like(g) if g is not None else None
        dpi = torch.empty_like(pi) if pi is not None else None
        _lib.call("ptr_mix_ce_bwd", _p(logits), _p(g), _p(pi), _p(labels), _p(rc), _p(rv), _p(co), _p(ce), _p(ci), _p(cw), _p(P),
                  _p(dP), _p(dloss), _p(dlogits), _p(dg), _p(dpi), R, V, c_max, e_max, smoothing, _p(row_w), _stream())
        return dlogits, dg, dpi, None, None, None, None, None, None, None, None, None


def ptr_mix_loss(logits, g, pi, labels, row_c, row_vid, csr_off, csr_ent, csr_id, csr_w, c_max, smoothing):
    return _PtrMixLoss.apply(logits, g, pi, labels, as_idx(row_c), as_idx(row_vid), as_idx(csr_off), as_idx(csr_ent),
                             as_idx(csr_id), csr_w if isinstance(csr_w, FIdx) else FIdx(csr_w), int(c_max), float(smoothing))


# ------------------------------------------------------------------------------------------------ Gumbel bag of words
class _GumbelBow(Function):
    @staticmethod
    def forward(ctx, P, emb, row_c, tau, noise):
        _need_gpu(P)
        ctx.emb_direct = _direct(emb)
        P, emb, noise = _c(P), _c(emb), _c(noise)
        R, c_max = P.shape
        V, W = emb.shape
        dev = P.device
        rc = row_c.dev(dev)
        bow = torch.empty(R, W, dtype=torch.float32, device=dev)
        idx = torch.empty(R, dtype=torch.int32, device=dev)
        stats = torch.empty(R, 2, dtype=torch.float32, device=dev)
        _lib.call("gumbel_fwd", _p(P), _p(noise), _p(rc), _p(emb), _p(bow), _p(idx), _p(stats), R, c_max, V, W, float(tau), _stream())
        ctx.save_for_backward(P, emb, noise, rc, idx, stats)
        ctx.cfg = (R, c_max, V, W, float(tau))
        return bow

    @staticmethod
    def backward(ctx, dbow):
        P, emb, noise, rc, idx, stats = ctx.saved_tensors
        R, c_max, V, W, tau = ctx.cfg
        dev = P.device
        dbow = _c(dbow)
        dP = demb = None
        if ctx.needs_input_grad[0]:
            dy = torch.empty(R, V, dtype=torch.float32, device=dev)
            _gemm(dbow, W, 1, emb, W, 1, dy, R, V, W)                      # dy = dbow @ embᵀ
            dP = torch.empty_like(P)
            _lib.call("gumbel_bwd", _p(P), _p(noise), _p(rc), _p(stats), _p(dy), _p(dP), R, c_max, V, tau, _stream())
        if ctx.needs_input_grad[1]:
            demb = ctx.emb_direct if ctx.emb_direct is not None else torch.zeros_like(emb)
            _lib.call("gumbel_emb_grad", _p(dbow), _p(idx), _p(stats), _p(demb), R, V, W, _stream())
            if ctx.emb_direct is not None:
                _ready(demb)
                demb = None
        return dP, demb, None, None, None


def gumbel_bow(P, row_c, emb, tau, noise=None, rng=None, site=0):
    if noise is None:
        noise = torch.empty_like(P)
        _lib.call("gumbel_noise", _p(noise), noise.numel(), int(site), _p(rng.seed), _stream())
    return _GumbelBow.apply(P, emb, as_idx(row_c), float(tau), noise)


# ------------------------------------------------------------------------------------------------ LSTM cell / losses
class _LstmCell(Function):
    @staticmethod
    def forward(ctx, gx, gh, c_prev, h_prev, active):
        _need_gpu(gx)
        gx, gh, c_prev, h_prev = _c(gx), _c(gh), _c(c_prev), _c(h_prev)
        N, D = c_prev.shape
        h = torch.empty_like(c_prev)
        c = torch.empty_like(c_prev)
        gates = torch.empty_like(gx)
        _lib.call("lstm_cell_fwd", _p(gx), _p(gh), _p(c_prev), _p(h_prev), _p(active), _p(h), _p(c), _p(gates), N, D, _stream())
        ctx.save_for_backward(gates, c_prev, active)
        ctx.cfg = (N, D)
        ctx.set_materialize_grads(False)
        return h, c

    @staticmethod
    def backward(ctx, dh, dc):
        gates, c_prev, active = ctx.saved_tensors
        N, D = ctx.cfg
        dev = gates.device
        dh = _c(dh) if dh is not None else torch.zeros(N, D, dtype=torch.float32, device=dev)
        dc = _c(dc) if dc is not None else torch.zeros(N, D, dtype=torch.float32, device=dev)
        dg = torch.empty_like(gates)
        dcp = torch.empty_like(c_prev)
        dhp = torch.empty_like(c_prev)
        _lib.call("lstm_cell_bwd", _p(dh), _p(dc), _p(gates), _p(c_prev), _p(active), _p(dg), _p(dcp), _p(dhp), N, D, _stream())
        return dg, dg, dcp, dhp, None


def lstm_cell(gx, gh, c_prev, h_prev, active):
    return _LstmCell.apply(gx, gh, c_prev, h_prev, active)


class _LstmSeq(Function):
    """One direction of the LSTM recurrence over every video's step sequence as a single autograd node.

    Per time step: one (N, D)×(D, 4D) GEMM + one fused cell kernel forward; one cell kernel + one dgrad GEMM (accumulating onto
    the pass-through gradient) backward.  The recurrent weight gradient is ONE GEMM over all time steps (K = S·N rows) on a side
    stream, the input-projection gradient one row gather.  No per-step gathers, adds or fills (reference: nn.LSTM model.py:859-860
    as used at :1022-1024; time-major state, inactive (padded) steps pass (h, c) through)."""

    @staticmethod
    def forward(ctx, gx_all, w_hh, rows_t, active_t, pick, wgrad):
        _need_gpu(gx_all)
        gx_all, w = _c(gx_all), _c(w_hh)
        S, N = len(rows_t), rows_t[0].numel()
        D = w.shape[1]
        dev = gx_all.device
        h_all = torch.empty(S + 1, N, D, dtype=torch.float32, device=dev)
        c_all = torch.empty(S + 1, N, D, dtype=torch.float32, device=dev)
        h_all[0].zero_(); c_all[0].zero_()
        gates = torch.empty(S, N, 4 * D, dtype=torch.float32, device=dev)
        gh = torch.empty(N, 4 * D, dtype=torch.float32, device=dev)
        for t in range(S):
            _gemm(h_all[t], D, 1, w, D, 1, gh, N, 4 * D, D)
            _lib.call("lstm_cell_fwd_idx", _p(gx_all), _p(rows_t[t]), _p(gh), _p(c_all[t]), _p(h_all[t]), _p(active_t[t]),
                      _p(h_all[t + 1]), _p(c_all[t + 1]), _p(gates[t]), N, D, _stream())
        out = torch.index_select(h_all[1:].reshape(S * N, D), 0, pick)
        ctx.save_for_backward(gates, c_all, h_all, w, pick)
        ctx.lists = (rows_t, active_t)
        ctx.direct = wgrad
        ctx.cfg = (S, N, D, gx_all.shape[0])
        return out

    @staticmethod
    def backward(ctx, dout):
        gates, c_all, h_all, w, pick = ctx.saved_tensors
        rows_t, active_t = ctx.lists
        S, N, D, T = ctx.cfg
        dev = dout.device
        dhs = torch.zeros(S * N, D, dtype=torch.float32, device=dev)
        dhs.index_copy_(0, pick.long() if pick.dtype != torch.int64 else pick, _c(dout))
        dhs = dhs.view(S, N, D)
        dG = torch.empty(S, N, 4 * D, dtype=torch.float32, device=dev)
        dh = torch.zeros(N, D, dtype=torch.float32, device=dev)
        dc = torch.zeros(N, D, dtype=torch.float32, device=dev)
        dh2, dc2 = torch.empty_like(dh), torch.empty_like(dc)
        wt = w.t().contiguous()         # (D, 4D): the S dgrad GEMMs then read both operands k-contiguously (12 tiles × K = 4D)
        for t in range(S - 1, -1, -1):
            _lib.call("lstm_cell_bwd_seq", _p(dhs[t]), _p(dh), _p(dc), _p(gates[t]), _p(c_all[t]), _p(active_t[t]), _p(dG[t]), _p(dc2),
                      _p(dh2), N, D, _stream())
            _gemm(dG[t], 4 * D, 1, wt, 4 * D, 1, dh2, N, D, 4 * D, accumulate=1)      # dh_{t-1} = pass-through + dgates · W_hh
            dh, dh2 = dh2, dh
            dc, dc2 = dc2, dc
        dG2, hp = dG.view(S * N, 4 * D), h_all[:S].reshape(S * N, D)
        wgrad = ctx.direct
        dw = None
        if wgrad is not None or ctx.needs_input_grad[1]:
            acc = 1 if wgrad is not None else 0
            dw = wgrad if wgrad is not None else torch.empty_like(w)
            _gemm(dG2, 4 * D, 0, hp, D, 0, dw, 4 * D, D, S * N, accumulate=acc)
            if wgrad is not None:
                _ready(wgrad, "w")
                dw = None
        dgx = torch.index_select(dG2, 0, pick) if ctx.needs_input_grad[0] else None
        return dgx, dw, None, None, None, None


class _GemmProblem(ctypes.Structure):
    _fields_ = [("A", ctypes.c_void_p), ("B", ctypes.c_void_p), ("C", ctypes.c_void_p), ("M", ctypes.c_int), ("N", ctypes.c_int),
                ("K", ctypes.c_int), ("lda", ctypes.c_int), ("ldb", ctypes.c_int), ("ldc", ctypes.c_int)]


def _gemm_pair(As, Bs, Cs, M, N, K, accumulate=0, x3=False):
    """C_z (+)= A_z · B_zᵀ for z = 0, 1 (all k-contiguous fp32) in one grouped launch"""
    probs = (_GemmProblem * 2)()
    for z in range(2):
        probs[z] = _GemmProblem(As[z].data_ptr(), Bs[z].data_ptr(), Cs[z].data_ptr(), M, N, K, As[z].stride(0), Bs[z].stride(0),
                                Cs[z].stride(0))
    _lib.call("gemm_group_x3" if x3 else "gemm_group", ctypes.addressof(probs), 2, 1, 1, accumulate, _stream())


def _ptr2(a, b):
    arr = (ctypes.c_void_p * 2)(a.data_ptr(), b.data_ptr())
    return ctypes.addressof(arr), arr          # keep `arr` alive until the call returns


LSTM_DGRAD_PARTS = int(os.environ.get("SVPC_LSTM_DGRAD_PARTS", "4"))
LSTM_FUSED_STEP = os.environ.get("SVPC_LSTM_FUSED_STEP", "1") != "0"      # recurrent projection and cell of a time step in one launch


class _BiLstmSeq(Function):
    """Both directions of the BiLSTM recurrence as ONE autograd node advancing in lockstep: per time step one grouped GEMM (the two
    recurrent projections) and one cell launch (both directions) forward, one cell launch and one grouped dgrad GEMM backward —
    half the launches of two independent direction nodes (see _LstmSeq for the per-direction scheme).  bf16-MFMA precision only."""

    @staticmethod
    def forward(ctx, gx_f, gx_b, w_f, w_b, rows_f, rows_b, active_t, pick_f, pick_b, wgrad_f, wgrad_b, summed=False):
        _need_gpu(gx_f)
        ctx.summed = bool(summed)
        gx = [_c(gx_f), _c(gx_b)]
        w = [_c(w_f), _c(w_b)]
        rows = [rows_f, rows_b]
        S, N = len(rows_f), rows_f[0].numel()
        D = w[0].shape[1]
        dev = gx_f.device
        mk = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
        # states of both directions in ONE buffer (direction, h|c, time, N, D) with the four initial states adjacent: one fill
        state = mk(2, 2, S + 1, N, D)
        state[:, :, 0].zero_()
        h_all, c_all = [state[0, 0], state[1, 0]], [state[0, 1], state[1, 1]]
        gates = [mk(S, N, 4 * D) for _ in range(2)]
        gh = [mk(N, 4 * D) for _ in range(2)]
        st = _stream()
        fused = LSTM_FUSED_STEP and D % 16 == 0 and (w[0].data_ptr() | w[1].data_ptr()) % 16 == 0
        pw = _ptr2(w[0], w[1])
        pgx = _ptr2(gx[0], gx[1])
        for t in range(S):
            args = [pgx, _ptr2(rows[0][t], rows[1][t]), _ptr2(gh[0], gh[1]), _ptr2(c_all[0][t], c_all[1][t]),
                    _ptr2(h_all[0][t], h_all[1][t]), None, _ptr2(h_all[0][t + 1], h_all[1][t + 1]),
                    _ptr2(c_all[0][t + 1], c_all[1][t + 1]), _ptr2(gates[0][t], gates[1][t])]
            if fused:       # recurrent projection + cell in one launch per time step
                _lib.call("lstm_pair_step_fwd_x3" if is_x3() else "lstm_pair_step_fwd", args[4][0], args[3][0], pw[0], args[0][0],
                          args[1][0], _p(active_t[t]), args[6][0], args[7][0], args[8][0], N, D, st)
                continue
            _gemm_pair([h_all[0][t], h_all[1][t]], w, gh, N, 4 * D, D, x3=is_x3())
            _lib.call("lstm_pair_fwd", args[0][0], args[1][0], args[2][0], args[3][0], args[4][0], _p(active_t[t]), args[6][0],
                      args[7][0], args[8][0], N, D, st)
        ctx.save_for_backward(gates[0], gates[1], c_all[0], c_all[1], h_all[0], h_all[1], w[0], w[1], pick_f, pick_b)
        ctx.lists = active_t
        ctx.direct = (wgrad_f, wgrad_b)
        ctx.cfg = (S, N, D)
        pair_ok = (D % 4 == 0 and pick_f.dtype == torch.int32 and pick_b.dtype == torch.int32 and pick_f.numel() == pick_b.numel())
        ctx.pair_ok = pair_ok
        if summed and pair_ok:      # the two directions' outputs picked from the time-major states and summed in one launch
            out = mk(pick_f.numel(), D)
            _lib.call("pair_rows", _p(h_all[0][1:]), _p(pick_f), _p(h_all[1][1:]), _p(pick_b), _p(out), None, pick_f.numel(), D, 0, st)
            return out
        outs = [torch.index_select(h_all[z][1:].reshape(S * N, D), 0, pk) for z, pk in enumerate((pick_f, pick_b))]
        if summed:
            return outs[0] + outs[1]
        return outs[0], outs[1]

    @staticmethod
    def backward(ctx, dout_f, dout_b=None):
        if ctx.summed:
            dout_b = dout_f
        g0, g1, c0, c1, h0, h1, w0, w1, pick_f, pick_b = ctx.saved_tensors
        gates, c_all, h_all, w, picks = [g0, g1], [c0, c1], [h0, h1], [w0, w1], [pick_f, pick_b]
        active_t = ctx.lists
        S, N, D = ctx.cfg
        dev = g0.device
        mk = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
        # every zero-initialised buffer of the backward in ONE allocation (one fill): the scattered output gradients of both
        # directions (2·S·N rows) and the four running state gradients (4·N rows)
        zeros = torch.zeros(2 * S * N + 4 * N, D, dtype=torch.float32, device=dev)
        dhs = []
        if ctx.summed and ctx.pair_ok and dout_f is not None:      # the one output gradient into both directions' time-major rows: one launch
            _lib.call("pair_rows", _p(zeros), _p(picks[0]), _p(zeros[S * N:]), _p(picks[1]), _p(_c(dout_f)), None, picks[0].numel(), D, 1,
                      _stream())
            dhs = [zeros[:S * N].view(S, N, D), zeros[S * N:2 * S * N].view(S, N, D)]
        else:
            for z, d in enumerate((dout_f, dout_b)):
                t_ = zeros[z * S * N:(z + 1) * S * N]
                if d is not None:
                    t_.index_copy_(0, picks[z].long(), _c(d))
                dhs.append(t_.view(S, N, D))
        dG = [mk(S, N, 4 * D) for _ in range(2)]
        tail = zeros[2 * S * N:].view(4, N, D)
        dh = [tail[0], tail[1]]
        dc = [tail[2], tail[3]]
        dh2, dc2 = [mk(N, D) for _ in range(2)], [mk(N, D) for _ in range(2)]
        st = _stream()
        # (the per-step dgrad dh = dG·W_hh reads W_hh (4D, D) k-strided IN PLACE — svpc_gemm_group with b_kc = 0 — instead of a transposed
        # copy of both directions' weights made every step: 2 × 14 µs of ATen copies at D = 768)
        # the per-step dgrad (N × D over K = 4D) is bound by how fast ONE workgroup can pull its weight columns: cut K into
        # LSTM_DGRAD_PARTS k-parts (separate problems of the grouped launch, each writing a slab) that the next cell launch adds
        P = LSTM_DGRAD_PARTS if (4 * D) % (32 * LSTM_DGRAD_PARTS) == 0 else 1
        Kp = 4 * D // P
        slabs = [mk(P, N, D) for _ in range(2)] if P > 1 else None
        have_parts = False
        for t in range(S - 1, -1, -1):
            a = [_ptr2(dhs[0][t], dhs[1][t]), _ptr2(dh[0], dh[1]), _ptr2(dc[0], dc[1]), _ptr2(gates[0][t], gates[1][t]),
                 _ptr2(c_all[0][t], c_all[1][t]), None, _ptr2(dG[0][t], dG[1][t]), _ptr2(dc2[0], dc2[1]), _ptr2(dh2[0], dh2[1])]
            if P > 1:
                sp = _ptr2(slabs[0], slabs[1])
                _lib.call("lstm_pair_bwd_parts", a[0][0], a[1][0], sp[0] if have_parts else None, P if have_parts else 0, a[2][0], a[3][0],
                          a[4][0], _p(active_t[t]), a[6][0], a[7][0], a[8][0], N, D, st)
                if t > 0:
                    probs = (_GemmProblem * (2 * P))()
                    for z in range(2):
                        for k in range(P):
                            probs[z * P + k] = _GemmProblem(dG[z][t].data_ptr() + 4 * k * Kp, w[z].data_ptr() + 4 * k * Kp * D,
                                                            slabs[z][k].data_ptr(), N, D, Kp, 4 * D, D, D)
                    _lib.call("gemm_group", ctypes.addressof(probs), 2 * P, 1, 0, 0, st)
                    have_parts = True
            else:
                _lib.call("lstm_pair_bwd", a[0][0], a[1][0], a[2][0], a[3][0], a[4][0], _p(active_t[t]), a[6][0], a[7][0], a[8][0], N, D, st)
                wt = [w[z].t().contiguous() for z in range(2)] if t == S - 1 else wt      # (unsplit fallback: a transposed copy, once)
                _gemm_pair([dG[0][t], dG[1][t]], wt, dh2, N, D, 4 * D, accumulate=1)      # dh_{t-1} = pass-through + dgates · W_hh
            dh, dh2 = dh2, dh
            dc, dc2 = dc2, dc
        dws, dgx = [None, None], [None, None]
        for z in range(2):
            dG2, hp = dG[z].view(S * N, 4 * D), h_all[z][:S].reshape(S * N, D)
            wgrad = ctx.direct[z]
            if wgrad is not None or ctx.needs_input_grad[2 + z]:
                if not (wgrad is not None and defer_wgrad(dG2, hp, wgrad, None)):
                    acc = 1 if wgrad is not None else 0
                    dw = wgrad if wgrad is not None else torch.empty_like(w[z])
                    _gemm(dG2, 4 * D, 0, hp, D, 0, dw, 4 * D, D, S * N, accumulate=acc)
                    if wgrad is not None:
                        _ready(wgrad, "w")
                    else:
                        dws[z] = dw
            if ctx.needs_input_grad[z] and not (ctx.pair_ok and ctx.needs_input_grad[0] and ctx.needs_input_grad[1]):
                dgx[z] = torch.index_select(dG2, 0, picks[z])
        if ctx.pair_ok and ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:       # both gate gradients gathered in one launch
            R_ = picks[0].numel()
            dgx = [mk(R_, 4 * D), mk(R_, 4 * D)]
            _lib.call("pair_rows", _p(dG[0]), _p(picks[0]), _p(dG[1]), _p(picks[1]), _p(dgx[0]), _p(dgx[1]), R_, 4 * D, 2, _stream())
        return dgx[0], dgx[1], dws[0], dws[1], None, None, None, None, None, None, None, None


def bilstm_sequences(gx_f, gx_b, w_f, w_b, rows_f, rows_b, active_t, pick_f, pick_b, summed=False):
    """Both LSTM directions (see lstm_sequence for the arguments) → (out_f, out_b), each (T, D); summed=True: their sum (what the model
    uses, model.py:1024) — picked and added in one launch, the backward scatters / gathers both directions in one launch each."""
    if _fast() and gx_f.is_cuda and not BWD_EXACT:
        return _BiLstmSeq.apply(gx_f, gx_b, w_f, w_b, rows_f, rows_b, active_t, pick_f, pick_b, _direct(w_f), _direct(w_b), summed)
    of, ob = lstm_sequence(gx_f, w_f, rows_f, active_t, pick_f), lstm_sequence(gx_b, w_b, rows_b, active_t, pick_b)
    return add(of, ob) if summed else (of, ob)


def lstm_sequence(gx_all, w_hh, rows_t, active_t, pick):
    """gx_all (T, 4D): input projections of every step row; rows_t[t] (N,) the step row each video consumes at time t;
    active_t[t] (N,) 1/0; pick (T,) position of every step row's output in the time-major (S·N) state → (T, D)."""
    return _LstmSeq.apply(gx_all, w_hh, rows_t, active_t, pick, _direct(w_hh))


class _BceRows(Function):
    @staticmethod
    def forward(ctx, p, y, widths):
        _need_gpu(p)
        p, y = _c(p), _c(y)
        R, C = p.shape
        w = widths.dev(p.device)
        out = torch.empty(R, dtype=torch.float32, device=p.device)
        _lib.call("bce_rows_fwd", _p(p), _p(y), _p(w), _p(out), R, C, _stream())
        ctx.save_for_backward(p, y, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        p, y, w = ctx.saved_tensors
        dp = torch.empty_like(p)
        _lib.call("bce_rows_bwd", _p(_c(dout)), _p(p), _p(y), _p(w), _p(dp), p.shape[0], p.shape[1], _stream())
        return dp, None, None


def bce_rows(p, y, widths):
    return _BceRows.apply(p, y, as_idx(widths))


class _AslRows(Function):
    @staticmethod
    def forward(ctx, p, y, active, gneg, gpos, clip, eps):
        _need_gpu(p)
        p, y = _c(p), _c(y)
        R, C = p.shape
        out = torch.empty(R, dtype=torch.float32, device=p.device)
        _lib.call("asl_rows_fwd", _p(p), _p(y), _p(active), _p(out), R, C, gneg, gpos, clip, eps, _stream())
        ctx.save_for_backward(p, y, active)
        ctx.cfg = (gneg, gpos, clip, eps)
        return out

    @staticmethod
    def backward(ctx, dout):
        p, y, active = ctx.saved_tensors
        dp = torch.empty_like(p)
        _lib.call("asl_rows_bwd", _p(_c(dout)), _p(p), _p(y), _p(active), _p(dp), p.shape[0], p.shape[1], *ctx.cfg, _stream())
        return dp, None, None, None, None, None, None


def asl_rows(p, y, row_active, gamma_neg=4.0, gamma_pos=1.0, clip=0.05, eps=1e-8):
    return _AslRows.apply(p, y, row_active, float(gamma_neg), float(gamma_pos), float(clip), float(eps))


_TICKETS = {}


class _LossTail(Function):
    """total = Σ cap_rows + Σ BCE(e_p) + Σ ASL(a_p) + λ·(Σ BCE(r_e) + Σ ASL(r_a)) in one launch; backward in one launch."""

    @staticmethod
    def forward(ctx, cap_rows, e_p, a_p, r_e, r_a, align, act, widths, lam, gneg, gpos, clip, eps):
        _need_gpu(cap_rows)
        cap_rows = _c(cap_rows)
        e_p, a_p, r_e, r_a = [(_c(t) if t is not None else None) for t in (e_p, a_p, r_e, r_a)]
        align, act = _c(align), _c(act)
        dev = cap_rows.device
        R, Ce = align.shape
        Ca = act.shape[1]
        w = widths.dev(dev)
        out = torch.empty(5, dtype=torch.float32, device=dev)
        scratch = torch.empty(_lib.load().svpc_loss_tail_ws_floats(cap_rows.numel(), R), dtype=torch.float32, device=dev)
        tkey = (dev, _stream())   # one counter per (device, stream): launches on one stream are ordered, two streams (or two models on
        counter = _TICKETS.get(tkey)    # their own streams) must not share the ticket word of a launch in flight
        if counter is None:       # zeroed once; every launch leaves it at zero
            counter = _TICKETS[tkey] = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.call("loss_tail_fwd", _p(cap_rows), cap_rows.numel(), _p(e_p), _p(align), _p(w), R, Ce, _p(a_p), _p(act), Ca, _p(r_e), _p(r_a),
                  float(lam), gneg, gpos, clip, eps, _p(out), _p(scratch), _p(counter), _stream())
        ctx.save_for_backward(e_p, a_p, r_e, r_a, align, act, w)
        ctx.cfg = (cap_rows.numel(), R, Ce, Ca, float(lam), gneg, gpos, clip, eps)
        ctx.parts = out
        return out[0]

    @staticmethod
    def backward(ctx, dout):
        e_p, a_p, r_e, r_a, align, act, w = ctx.saved_tensors
        n_cap, R, Ce, Ca, lam, gneg, gpos, clip, eps = ctx.cfg
        dev = align.device
        need = ctx.needs_input_grad
        mk = lambda t, on: torch.empty_like(t) if (t is not None and on) else None
        d_cap = torch.empty(n_cap, dtype=torch.float32, device=dev) if need[0] else None
        de, da, dre, dra = mk(e_p, need[1]), mk(a_p, need[2]), mk(r_e, need[3]), mk(r_a, need[4])
        _lib.call("loss_tail_bwd", _p(_c(dout)), n_cap, _p(e_p), _p(align), _p(w), R, Ce, _p(a_p), _p(act), Ca, _p(r_e), _p(r_a), lam, gneg,
                  gpos, clip, eps, _p(d_cap), _p(de), _p(da), _p(dre), _p(dra), _stream())
        return d_cap, de, da, dre, dra, None, None, None, None, None, None, None, None


def loss_tail(cap_rows, e_p, a_p, r_e, r_a, align, act, widths, lam, gamma_neg=4.0, gamma_pos=1.0, clip=0.05, eps=1e-8):
    """Scalar training loss from the caption-loss rows and the (re-)simulator probabilities; e_p / a_p / r_e / r_a may be None."""
    return _LossTail.apply(cap_rows, e_p, a_p, r_e, r_a, align, act, as_idx(widths), float(lam), float(gamma_neg), float(gamma_pos),
                           float(clip), float(eps))


def greedy_pick(scores, row_c, row_x, lt, pos, unk, append=None):
    """scores (T*lt, ≥C): → (next_ext, next_model) int32 (T,), see svpc_greedy_pick.  ``append`` = (text, ext, col): the picked ids are
    also stored as column ``col`` of the two (T, Lt) int32 id matrices of the decoding loop (one launch instead of three)."""
    scores = _c(scores)
    dev = scores.device
    n = scores.shape[0] // lt
    ext = torch.empty(n, dtype=torch.int32, device=dev)
    mod = torch.empty(n, dtype=torch.int32, device=dev)
    if append is not None:
        tm, em, col = append
        assert tm.dtype == em.dtype == torch.int32 and tm.is_contiguous() and em.is_contiguous() and tm.shape == em.shape and tm.shape[0] == n
        _lib.call("greedy_pick_append", _p(scores), scores.stride(0), _p(as_idx(row_c).dev(dev)), _p(as_idx(row_x).dev(dev)), n, lt, int(pos),
                  int(unk), _p(ext), _p(mod), _p(tm), _p(em), tm.shape[1], int(col), _stream())
        return ext, mod
    _lib.call("greedy_pick", _p(scores), scores.stride(0), _p(as_idx(row_c).dev(dev)), _p(as_idx(row_x).dev(dev)), n, lt, int(pos),
              int(unk), _p(ext), _p(mod), _stream())
    return ext, mod


BEAM_MAX = 8


LENGTH_PENALTIES = ("none", "avg", "wu")


BLOCK_SCOPES = ("sentence", "paragraph")


def _as_int(name, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
        raise ValueError("%s must be an integer, got %r" % (name, v))
    return int(v)


def _lp_table(lp, lt, device=None):
    """``lp`` is a contiguous float64 table of at least ``lt`` entries (on ``device``, when given)"""
    return lp.dtype == torch.float64 and lp.dim() == 1 and lp.shape[0] >= lt and lp.is_contiguous() and (device is None or lp.device == device)


def check_beam_controls(lt, vocab, beam=None, block_ngram_repeat=0, exclusion_tokens=(), min_length=0, length_penalty_name="none",
                        length_penalty_alpha=0.0, n_best=None, block_ngram_scope="sentence", max_cols=None):
    """The decoding controls of a beam decode over Lt = ``lt`` positions and ``vocab`` text ids, checked on the host (ValueError) and
    normalised → dict(block_ngram_repeat, exclusion_tokens (sorted tuple), min_length, length_penalty_name, length_penalty_alpha,
    block_ngram_scope [, n_best]).  n: 0 … Lt − 1 (and Lt ≤ 64 when n > 0); m: 0 … Lt − 1; exclusion ids in [0, vocab); alpha finite ≥ 0;
    n_best 1 … beam; scope ``sentence`` or ``paragraph`` (needs n > 0 and score rows of at most SAMPLE_COLS_MAX columns: ``max_cols``, the
    widest row V + X, default ``vocab``)."""
    n = _as_int("block_ngram_repeat", block_ngram_repeat)
    m = _as_int("min_length", min_length)
    if not 0 <= n <= lt - 1:
        raise ValueError("block_ngram_repeat must be 0..%d (Lt - 1), got %d" % (lt - 1, n))
    if n > 0 and lt > 64:
        raise ValueError("block_ngram_repeat needs Lt <= 64 (one wave holds a hypothesis's ids), Lt = %d" % lt)
    if not 0 <= m <= lt - 1:
        raise ValueError("min_length must be 0..%d (Lt - 1), got %d" % (lt - 1, m))
    excl = tuple(sorted({_as_int("exclusion_tokens", e) for e in (exclusion_tokens or ())}))
    for e in excl:
        if not 0 <= e < vocab:
            raise ValueError("exclusion_tokens must be text ids in [0, %d), got %d" % (vocab, e))
    name = length_penalty_name if length_penalty_name is not None else "none"
    if name not in LENGTH_PENALTIES:
        raise ValueError("length_penalty_name must be one of %s, got %r" % (", ".join(LENGTH_PENALTIES), name))
    try:
        alpha = float(length_penalty_alpha)
    except (TypeError, ValueError):
        raise ValueError("length_penalty_alpha must be a number, got %r" % (length_penalty_alpha,))
    if not math.isfinite(alpha) or alpha < 0:
        raise ValueError("length_penalty_alpha must be finite and >= 0, got %r" % (length_penalty_alpha,))
    scope = block_ngram_scope if block_ngram_scope is not None else "sentence"
    if scope not in BLOCK_SCOPES:
        raise ValueError("block_ngram_scope must be one of %s, got %r" % (", ".join(BLOCK_SCOPES), block_ngram_scope))
    if scope == "paragraph":
        if n == 0:
            raise ValueError("block_ngram_scope='paragraph' needs block_ngram_repeat > 0 (there is nothing to block)")
        check_paragraph_cols(vocab if max_cols is None else max_cols)
    out = dict(block_ngram_repeat=n, exclusion_tokens=excl, min_length=m, length_penalty_name=name, length_penalty_alpha=alpha,
               block_ngram_scope=scope)
    if n_best is not None:
        k = _as_int("n_best", n_best)
        if beam is None or not 1 <= k <= beam:
            raise ValueError("n_best must be 1..%s (the beam width), got %d" % (beam, k))
        out["n_best"] = k
    return out


def check_paragraph_cols(max_cols):
    """paragraph-scope blocking keeps a row's bans as a bitmap of SAMPLE_COLS_MAX columns: wider score rows (V + X) are refused"""
    if int(max_cols) > SAMPLE_COLS_MAX:
        raise ValueError("block_ngram_scope='paragraph' reads score rows of at most %d columns (vocabulary + copied words), got %d"
                         % (SAMPLE_COLS_MAX, max_cols))


def length_penalty_table(name, alpha, lt):
    """lp[len] for len = 0 … lt − 1 as float64 (Python floats): ``none`` 1, ``avg`` len, ``wu`` ((5 + len) / 6) ** alpha.  Computed once on
    the host; the kernels and the CPU reference divide by the same numbers.  (len 0 never ranks: ``avg`` stores 1 there.)"""
    if name == "none":
        return [1.0] * lt
    if name == "avg":
        return [1.0] + [float(n) for n in range(1, lt)]
    if name == "wu":
        return [((5.0 + n) / 6.0) ** float(alpha) for n in range(lt)]
    raise ValueError("length_penalty_name must be one of %s, got %r" % (", ".join(LENGTH_PENALTIES), name))


def exclusion_bitmap(tokens, vocab, device):
    """(ceil(vocab / 32),) int32: bit t of word t // 32 set for every id t of ``tokens`` (the exclusion set of n-gram blocking)."""
    words = [0] * ((vocab + 31) // 32)
    for t in tokens:
        words[t >> 5] |= 1 << (t & 31)
    return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32, device=device)


def _beam_step_shared(fn, scores, row_c, row_x, beam, pos, logits, unk, eos, pad, cum, finished, toks_in, toks_out, slot_rows):
    """What the four selection steps check and build alike (``fn``: the caller's name, for the error texts) → ((R, Lt, device), the
    (parent, next_ext, next_model) outputs, the 24 leading arguments of the library call)."""
    if not 1 <= beam <= BEAM_MAX:
        raise ValueError("%s: beam width must be 1..%d" % (fn, BEAM_MAX))
    R, dev = cum.shape[0], scores.device
    if scores.dim() != 2 or scores.shape[0] != R or R % beam or scores.stride(1) != 1 or scores.dtype != torch.float32:
        raise ValueError("%s: scores must be fp32 (T·beam, C) rows with unit column stride" % fn)
    if not (_row_vec(cum, R, torch.float32) and _row_vec(finished, R, torch.int32)):
        raise ValueError("%s: cum fp32 and finished int32, both contiguous (T·beam,)" % fn)
    lt = toks_in[0].shape[1]
    for m in tuple(toks_in) + tuple(toks_out):
        if not _id_rows(m, R, lt, dev):
            raise ValueError("%s: token / ancestry tables must be contiguous int32 (T·beam, Lt) on the scores' device" % fn)
    if any(i.data_ptr() == o.data_ptr() for i, o in zip(toks_in, toks_out)):
        raise ValueError("%s: the token and ancestry tables are ping-pong pairs" % fn)
    if not 0 <= pos < lt - 1 or slot_rows < lt:
        raise ValueError("%s: position %d outside the %d-column tables" % (fn, pos, lt))
    outs = tuple(torch.empty(R, dtype=torch.int32, device=dev) for _ in range(3))
    args = [_p(scores), scores.stride(0), _p(as_idx(row_c).dev(dev)), _p(as_idx(row_x).dev(dev)), R // beam, int(beam), int(pos),
            1 if logits else 0, int(unk), int(eos), int(pad), int(slot_rows), _p(cum), _p(finished), _p(toks_in[0]), _p(toks_in[1]),
            _p(toks_in[2]), _p(toks_out[0]), _p(toks_out[1]), _p(toks_out[2]), lt, _p(outs[0]), _p(outs[1]), _p(outs[2])]
    return (R, lt, dev), outs, args


def _beam_step_controls(fn, R, lt, dev, length, min_length, block_ngram_repeat, lp, exclusion, need_length=True):
    """The decoding controls of a selection step, checked → their six arguments of the library call."""
    if not (0 <= int(min_length) < lt and 0 <= int(block_ngram_repeat) < lt):
        raise ValueError("%s: min_length and block_ngram_repeat must be 0..%d" % (fn, lt - 1))
    if block_ngram_repeat and lt > 64:
        raise ValueError("%s: block_ngram_repeat needs Lt <= 64" % fn)
    if (length is None and need_length) or (length is not None and not _row_vec(length, R, torch.int32, dev)):
        raise ValueError("%s: length must be contiguous int32 (T·beam,) on the scores' device" % fn)
    if lp is not None and (length is None or not _lp_table(lp, lt, dev)):
        raise ValueError("%s: lp must be a contiguous float64 table of >= Lt entries on the scores' device, with length" % fn)
    bits, vocab = exclusion if exclusion is not None else (None, 0)
    if exclusion is not None and (bits.dtype != torch.int32 or bits.dim() != 1 or bits.shape[0] * 32 < vocab or vocab < 1
                                  or not bits.is_contiguous() or bits.device != dev):
        raise ValueError("%s: exclusion must be (int32 bitmap of >= vocab bits, vocab) on the scores' device" % fn)
    return [int(min_length), int(block_ngram_repeat), _p(bits), int(vocab), _p(lp), _p(length)]


def beam_step(scores, row_c, row_x, beam, pos, logits, unk, eos, pad, cum, finished, toks_in, toks_out, slot_rows, *, length=None,
              min_length=0, block_ngram_repeat=0, exclusion=None, lp=None, history=None):
    """One beam-search selection step (svpc_beam_step) over ``scores`` (T·beam, ≥ C) — probabilities, or logits when ``logits``.
    ``cum`` (T·beam,) fp32 and ``finished`` (T·beam,) int32 are updated in place; ``toks_in`` / ``toks_out`` = (text, ext, key_rows): the
    ping-pong (T·beam, Lt) int32 id matrices and KV-cache ancestry tables, the children's written for positions ≤ pos + 1.
    Decoding controls (keyword-only; any given → svpc_beam_step_ctl): ``length`` (T·beam,) int32 hypothesis lengths, updated in place;
    ``min_length`` m; ``block_ngram_repeat`` n; ``exclusion`` = (bitmap of ``exclusion_bitmap``, vocab); ``lp`` float64 (Lt,) table of
    ``length_penalty_table`` (needs ``length``).
    Paragraph scope (``history`` given → svpc_beam_step_para; needs n ≥ 1 and rows of at most SAMPLE_COLS_MAX columns): ``history`` =
    (table, desc, bos): ``table`` a contiguous int32 (rows, Lt) matrix of earlier sentences' chosen extended ids on the scores' device,
    ``desc`` 2·T host ints (an Idx or a list) — sentence t's history is rows desc[2t] … desc[2t] + desc[2t + 1] − 1 — and the BOS id.
    → (parent, next_ext, next_model) int32 (T·beam,)."""
    (R, lt, dev), outs, args = _beam_step_shared("beam_step", scores, row_c, row_x, beam, pos, logits, unk, eos, pad, cum, finished, toks_in,
                                                 toks_out, slot_rows)
    ctl = _beam_step_controls("beam_step", R, lt, dev, length, min_length, block_ngram_repeat, lp, exclusion, need_length=False)
    name = "beam_step"
    if length is not None or min_length or block_ngram_repeat or exclusion is not None or lp is not None or history is not None:
        name, args = "beam_step_ctl", args + ctl
    if history is not None:
        table, desc, bos = history
        desc = as_idx(desc)
        if int(block_ngram_repeat) < 1 or lt > 64:
            raise ValueError("beam_step: paragraph scope needs block_ngram_repeat >= 1 and Lt <= 64")
        if table.dim() != 2 or not _id_rows(table, table.shape[0], lt, dev):
            raise ValueError("beam_step: the history must be a contiguous int32 (rows, Lt) matrix on the scores' device")
        d = desc.host
        if len(d) != 2 * (R // beam) or any(c < 0 or f < 0 or f + c > table.shape[0] for f, c in zip(d[0::2], d[1::2])):
            raise ValueError("beam_step: the history descriptors must be (first row, count) pairs inside the history, one per sentence")
        rc = as_idx(row_c).host
        if rc and max(rc) > SAMPLE_COLS_MAX:
            raise ValueError("beam_step: paragraph scope reads rows of at most %d columns" % SAMPLE_COLS_MAX)
        name, args = "beam_step_para", args + [_p(table), _p(desc.dev(dev)), int(bos)]
    _need_gpu(scores)
    _lib.call(name, *args, _stream())
    return outs


def check_diverse(beam, num_groups, diversity_strength, n_best=None):
    """The arguments of diverse (group) beam search, checked on the host (ValueError) → (W, G, λ as the fp32 value the table is built
    from, n_best): W = ``beam`` 1 … BEAM_MAX, G = ``num_groups`` an integer ≥ 1 that divides W, λ = ``diversity_strength`` a finite number
    ≥ 0, ``n_best`` 1 … W / G rows per group (None: all W / G)."""
    W = _as_int("beam_size", beam)
    if not 1 <= W <= BEAM_MAX:
        raise ValueError("beam_size must be 1..%d, got %r" % (BEAM_MAX, beam))
    G = _as_int("num_groups", num_groups)
    if G < 1 or W % G:
        raise ValueError("num_groups must be >= 1 and divide the beam width %d, got %d" % (W, G))
    if isinstance(diversity_strength, bool) or not isinstance(diversity_strength, numbers.Real):
        raise ValueError("diversity_strength must be a number, got %r" % (diversity_strength,))
    lam = float(diversity_strength)
    if not math.isfinite(lam) or lam < 0:
        raise ValueError("diversity_strength must be finite and >= 0, got %r" % (diversity_strength,))
    try:
        lam = struct.unpack("f", struct.pack("f", lam))[0]
    except OverflowError:
        lam = float("inf")
    if not math.isfinite(lam):
        raise ValueError("diversity_strength must be finite in fp32, got %r" % (diversity_strength,))
    k = W // G if n_best is None else _as_int("n_best", n_best)
    if not 1 <= k <= W // G:
        raise ValueError("n_best must be 1..%d (the rows of a group), got %d" % (W // G, k))
    return W, G, lam, k


def diversity_table(strength, beam):
    """pen[n] = fp32(fp32(λ) · n) for n = 0 … ``beam`` − 1, as Python floats: what a candidate pays when n rows of earlier groups picked
    its word at this step.  Computed once on the host; the kernel and the CPU restatement subtract the same numbers."""
    lam = struct.unpack("f", struct.pack("f", float(strength)))[0]
    return [struct.unpack("f", struct.pack("f", min(lam * n, 3.4028234663852886e38)))[0] for n in range(int(beam))]


def beam_step_groups(scores, row_c, row_x, beam, groups, pos, logits, unk, eos, pad, cum, aug, finished, length, toks_in, toks_out, slot_rows,
                     pen, *, min_length=0, block_ngram_repeat=0, exclusion=None, lp=None):
    """One selection step of diverse (group) beam search (svpc_beam_step_groups): ``beam_step`` with controls over ``beam`` rows per
    sentence in ``groups`` groups (row g·Bg + j: hypothesis j of group g), the groups picking in order under the Hamming penalty table
    ``pen`` (fp32 (≥ beam,), ``diversity_table``).  In place: ``cum`` (the model's score), ``aug`` (the selection score, fp32
    (T·beam,)), ``finished``, ``length`` (required).  → (parent, next_ext, next_model) int32 (T·beam,)."""
    (R, lt, dev), outs, args = _beam_step_shared("beam_step_groups", scores, row_c, row_x, beam, pos, logits, unk, eos, pad, cum, finished,
                                                 toks_in, toks_out, slot_rows)
    ctl = _beam_step_controls("beam_step_groups", R, lt, dev, length, min_length, block_ngram_repeat, lp, exclusion)
    if isinstance(groups, bool) or not isinstance(groups, numbers.Integral) or groups < 1 or beam % groups:
        raise ValueError("beam_step_groups: the number of groups must divide the beam width")
    if not _row_vec(aug, R, torch.float32, dev) or aug.data_ptr() == cum.data_ptr():
        raise ValueError("beam_step_groups: aug must be contiguous fp32 (T·beam,) on the scores' device, and not cum itself")
    if pen.dtype != torch.float32 or pen.dim() != 1 or pen.shape[0] < beam or not pen.is_contiguous() or pen.device != dev:
        raise ValueError("beam_step_groups: pen must be a contiguous fp32 table of >= beam entries on the scores' device")
    _need_gpu(scores)
    _lib.call("beam_step_groups", *args, *ctl, int(groups), _p(pen), _p(aug), _stream())
    return outs


def check_stochastic_beam(max_t_len, beam_size, seed=None, max_cols=None, random_sampling_temp=1.0, min_length=0):
    """The settings of a stochastic beam search (Kool et al. 2019) over Lt = ``max_t_len`` positions, checked on the host (ValueError)
    and normalised → dict(beam_size W (1 … BEAM_MAX), random_sampling_temp τ (finite > 0), min_length m (0 … Lt − 1), seed (None or an
    int in [0, 2⁶³))).  ``max_cols``: the widest score row C_r = V + X of the batch (≤ SAMPLE_COLS_MAX: the draw index is r·4096 + c)."""
    W = _as_int("beam_size", beam_size)
    if not 1 <= W <= BEAM_MAX:
        raise ValueError("beam_size must be 1..%d, got %d" % (BEAM_MAX, W))
    if isinstance(random_sampling_temp, bool) or not isinstance(random_sampling_temp, numbers.Real):
        raise ValueError("random_sampling_temp must be a number, got %r" % (random_sampling_temp,))
    temp = float(random_sampling_temp)
    if not math.isfinite(temp) or temp <= 0:
        raise ValueError("random_sampling_temp must be finite and > 0, got %r" % (random_sampling_temp,))
    m = _as_int("min_length", min_length)
    if not 0 <= m <= max_t_len - 1:
        raise ValueError("min_length must be 0..%d (Lt - 1), got %d" % (max_t_len - 1, m))
    if seed is not None:
        seed = _as_int("seed", seed)
        if not 0 <= seed < 1 << 63:
            raise ValueError("seed must be None or an integer in [0, 2**63), got %d" % seed)
    if max_cols is not None and int(max_cols) > SAMPLE_COLS_MAX:
        raise ValueError("stochastic beam search reads score rows of at most %d columns (vocabulary + copied words), got %d"
                         % (SAMPLE_COLS_MAX, max_cols))
    return dict(beam_size=W, random_sampling_temp=temp, min_length=m, seed=seed)


def stochastic_beam_step(scores, row_c, row_x, beam, pos, logits, unk, eos, pad, cum, phi, gkey, finished, length, toks_in, toks_out,
                         slot_rows, seed, *, temp=1.0, min_length=0, max_cols=None):
    """One selection step of stochastic beam search (svpc_beam_step_gumbel): ``beam_step``'s tables over ``beam`` rows per sentence,
    selected by Gumbel-perturbed log-probabilities — the sentence's rows are a sample without replacement, in the order drawn.  In place,
    all contiguous (T·beam,) on the scores' device: ``cum`` fp32 (the model's score), ``phi`` / ``gkey`` float64 (the tempered
    log-probability and the perturbed log-probability G of a row; a dead row holds −inf and is finished), ``finished`` / ``length`` int32.
    ``seed`` is a device int64 (1,) tensor (read by the kernel: a captured graph replays with whatever it holds); ``temp`` τ divides the
    step scores, EOS is barred while pos + 1 ≤ ``min_length``; ``max_cols``: max(row_c) when the caller knows it (else taken from the
    host copy).  → (parent, next_ext, next_model) int32 (T·beam,)."""
    if isinstance(beam, bool) or not isinstance(beam, numbers.Integral) or not 1 <= beam <= BEAM_MAX:
        raise ValueError("stochastic_beam_step: beam width must be 1..%d" % BEAM_MAX)
    (R, lt, dev), outs, args = _beam_step_shared("stochastic_beam_step", scores, row_c, row_x, beam, pos, logits, unk, eos, pad, cum, finished,
                                                 toks_in, toks_out, slot_rows)
    for t, dt in ((cum, torch.float32), (phi, torch.float64), (gkey, torch.float64), (finished, torch.int32), (length, torch.int32)):
        if not _row_vec(t, R, dt, dev):
            raise ValueError("stochastic_beam_step: cum fp32, phi and gkey float64, finished and length int32, all contiguous (T·beam,) "
                             "on the scores' device")
    if seed.dtype != torch.int64 or seed.numel() < 1 or seed.device != dev:
        raise ValueError("stochastic_beam_step: seed must be a device int64 tensor")
    if not (math.isfinite(temp) and temp > 0 and 0 <= int(min_length) < lt):
        raise ValueError("stochastic_beam_step: temp finite > 0, min_length 0..Lt-1")
    max_c = int(max_cols) if max_cols is not None else (max(as_idx(row_c).host) if R else 1)
    if max_c > SAMPLE_COLS_MAX or max_c > scores.shape[1] or max_c < 1:
        raise ValueError("stochastic_beam_step: rows of 1..%d columns, inside the score matrix" % SAMPLE_COLS_MAX)
    _need_gpu(scores)
    _lib.call("beam_step_gumbel", *args, float(temp), int(min_length), _p(seed), _p(phi), _p(gkey), _p(length), int(max_c), _stream())
    return outs


def check_contrastive(lt, top_k, penalty_alpha, min_length=0, max_cols=None):
    """The settings of a contrastive search (Su et al. 2022) over Lt = ``lt`` positions, checked on the host (ValueError) and normalised →
    dict(top_k k (an integer 1 … BEAM_MAX), penalty_alpha α (a finite number in [0, 1], rounded to fp32: the value the kernel and a
    captured graph hold), min_length m (0 … Lt − 1)).  ``max_cols``: the widest score row C_r = V + X of the batch (≤ SAMPLE_COLS_MAX)."""
    k = _as_int("top_k", top_k)
    if not 1 <= k <= BEAM_MAX:
        raise ValueError("top_k must be 1..%d, got %d" % (BEAM_MAX, k))
    if isinstance(penalty_alpha, bool) or not isinstance(penalty_alpha, numbers.Real):
        raise ValueError("penalty_alpha must be a number, got %r" % (penalty_alpha,))
    alpha = float(penalty_alpha)
    if not math.isfinite(alpha) or not 0.0 <= alpha <= 1.0:
        raise ValueError("penalty_alpha must be a finite number in [0, 1], got %r" % (penalty_alpha,))
    m = _as_int("min_length", min_length)
    if not 0 <= m <= lt - 1:
        raise ValueError("min_length must be 0..%d (Lt - 1), got %d" % (lt - 1, m))
    if max_cols is not None and int(max_cols) > SAMPLE_COLS_MAX:
        raise ValueError("contrastive search reads score rows of at most %d columns (vocabulary + copied words), got %d"
                         % (SAMPLE_COLS_MAX, max_cols))
    return dict(top_k=k, penalty_alpha=struct.unpack("f", struct.pack("f", alpha))[0], min_length=m)


def contrastive_step(scores, row_c, row_x, top_k, pos, logits, unk, eos, pad, hidden, cand_p, cand_score, ids, cum, length, pen, finished,
                     hist, hist_n2, toks_in, toks_out, slot_rows, *, alpha, min_length=0, max_cols=None):
    """One selection step of contrastive search (svpc_contrastive_step) after the decoder pass at position ``pos`` over ``top_k`` candidate
    rows per sentence: ``hidden`` (T·k, D) fp32 is the pass's last-layer output, ``scores`` (T·k, ≥ C) its score rows (``beam_step``'s; None
    at the last position pos = Lt − 1, which has no expansion).  In place, all contiguous on the hidden rows' device — per row (T·k,):
    ``cand_p`` / ``cand_score`` fp32, the probability (0: a dead candidate) and the step score of the word the row carries, replaced by
    the children's; per sentence: ``ids`` (T, Lt) int32 committed extended ids, ``cum`` (T,) fp32, ``length`` (T,) int32, ``pen`` (T, Lt)
    fp32 the winners' penalties, ``finished`` (T,) int32, ``hist`` (T, Lt, D) fp32 the committed positions' hidden states and ``hist_n2``
    (T, Lt) float64 their squared norms.  ``toks_in`` / ``toks_out`` as ``beam_step``'s (the k children descend from the winner).
    ``alpha`` the degeneration penalty's weight in [0, 1]; EOS is barred while pos + 1 ≤ ``min_length``; ``max_cols``: max(row_c) when the
    caller knows it.  → (winner (T,) int32: the winning row of each sentence, −1 for none; parent, next_ext, next_model (T·k,) int32)."""
    k = top_k
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= k <= BEAM_MAX:
        raise ValueError("contrastive_step: top_k must be 1..%d" % BEAM_MAX)
    dev = hidden.device
    if hidden.dim() != 2 or hidden.dtype != torch.float32 or hidden.stride(1) != 1 or hidden.shape[0] % k or hidden.shape[1] < 1:
        raise ValueError("contrastive_step: hidden must be fp32 (T·k, D) rows with unit column stride")
    R, D = hidden.shape
    T = R // k
    lt = toks_in[0].shape[1]
    if not 0 <= pos < lt or slot_rows < lt:
        raise ValueError("contrastive_step: position %d outside the %d-column tables" % (pos, lt))
    if scores is None:
        if pos != lt - 1:
            raise ValueError("contrastive_step: only the last position runs without score rows")
    elif scores.dim() != 2 or scores.shape[0] != R or scores.stride(1) != 1 or scores.dtype != torch.float32 or scores.device != dev:
        raise ValueError("contrastive_step: scores must be fp32 (T·k, C) rows with unit column stride on the hidden rows' device")
    if not (_row_vec(cand_p, R, torch.float32, dev) and _row_vec(cand_score, R, torch.float32, dev)):
        raise ValueError("contrastive_step: cand_p and cand_score fp32, contiguous (T·k,) on the hidden rows' device")
    if not (_row_vec(cum, T, torch.float32, dev) and _row_vec(length, T, torch.int32, dev) and _row_vec(finished, T, torch.int32, dev)
            and _id_rows(ids, T, lt, dev) and pen.dtype == torch.float32 and tuple(pen.shape) == (T, lt) and pen.is_contiguous()
            and pen.device == dev):
        raise ValueError("contrastive_step: cum fp32, length and finished int32 (T,), ids int32 and pen fp32 (T, Lt), all contiguous on "
                         "the hidden rows' device")
    if not (hist.dtype == torch.float32 and tuple(hist.shape) == (T, lt, D) and hist.is_contiguous() and hist.device == dev
            and hist_n2.dtype == torch.float64 and tuple(hist_n2.shape) == (T, lt) and hist_n2.is_contiguous() and hist_n2.device == dev):
        raise ValueError("contrastive_step: hist fp32 (T, Lt, D) and hist_n2 float64 (T, Lt), contiguous on the hidden rows' device")
    for m in tuple(toks_in) + tuple(toks_out):
        if not _id_rows(m, R, lt, dev):
            raise ValueError("contrastive_step: token / ancestry tables must be contiguous int32 (T·k, Lt) on the hidden rows' device")
    if any(i.data_ptr() == o.data_ptr() for i, o in zip(toks_in, toks_out)):
        raise ValueError("contrastive_step: the token and ancestry tables are ping-pong pairs")
    a = float(alpha)
    if not (math.isfinite(a) and 0.0 <= a <= 1.0 and 0 <= int(min_length) < lt):
        raise ValueError("contrastive_step: alpha a finite number in [0, 1], min_length 0..Lt-1")
    max_c = int(max_cols) if max_cols is not None else (max(as_idx(row_c).host) if R else 1)
    if max_c > SAMPLE_COLS_MAX or max_c < 1 or (scores is not None and max_c > scores.shape[1]):
        raise ValueError("contrastive_step: rows of 1..%d columns, inside the score matrix" % SAMPLE_COLS_MAX)
    _need_gpu(hidden)
    winner = torch.empty(T, dtype=torch.int32, device=dev)
    outs = tuple(torch.empty(R, dtype=torch.int32, device=dev) for _ in range(3))
    _lib.call("contrastive_step", _p(scores), scores.stride(0) if scores is not None else max_c, _p(as_idx(row_c).dev(dev)),
              _p(as_idx(row_x).dev(dev)), T, int(k), int(pos), 1 if logits else 0, int(unk), int(eos), int(pad), int(slot_rows), _p(hidden),
              hidden.stride(0), D, a, int(min_length), max_c, _p(cand_p), _p(cand_score), _p(toks_in[0]), _p(toks_in[1]), _p(toks_in[2]),
              _p(toks_out[0]), _p(toks_out[1]), _p(toks_out[2]), lt, _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(ids), _p(cum), _p(length),
              _p(pen), _p(finished), _p(hist), _p(hist_n2), _p(winner), _stream())
    return (winner,) + outs


CONS_MAX = 4                    # constraints (phrases) of a sentence
CONS_LEN = 4                    # extended ids of a phrase


def check_constraints(constraints, batch_step_num, c_list, lt):
    """The lexical constraints of a constrained beam decode, checked on the host (ValueError) → the (T, CONS_MAX, CONS_LEN) int32 host
    table ``beam_step_cons`` reads (a phrase: the leading ids of its row, the rest −1; a sentence's phrases: its leading rows).
    ``constraints``: per video a list of S_b (``batch_step_num``) entries, each None / empty (no constraint) or a list of at most CONS_MAX
    phrases of 1 … CONS_LEN extended ids; an id is a word of the video's C_b = ``c_list[b]`` columns other than PAD, BOS, EOS and UNK;
    the ids of a sentence's phrases together must leave room for BOS and EOS: Σ len ≤ ``lt`` − 2."""
    from .synthetic import BOS, EOS, PAD, UNK
    steps = [int(s) for s in batch_step_num]
    if isinstance(constraints, (str, bytes)) or not hasattr(constraints, "__len__") or len(constraints) != len(steps) or len(c_list) != len(steps):
        raise ValueError("constraints must hold one list per video (%d videos)" % len(steps))
    rows = [-1] * (sum(steps) * CONS_MAX * CONS_LEN)           # (filled as a flat Python list: one tensor construction per call)
    t = 0
    for b, (per_video, S_b) in enumerate(zip(constraints, steps)):
        if isinstance(per_video, (str, bytes)) or not hasattr(per_video, "__len__") or len(per_video) != S_b:
            raise ValueError("constraints of video %d must hold one entry per sentence (%d sentences)" % (b, S_b))
        for s, phrases in enumerate(per_video):
            phrases = [] if phrases is None else phrases
            if isinstance(phrases, (str, bytes)) or not hasattr(phrases, "__len__"):
                raise ValueError("constraints of video %d sentence %d must be a list of phrases, got %r" % (b, s, phrases))
            if len(phrases) > CONS_MAX:
                raise ValueError("video %d sentence %d has %d phrases, at most %d are supported" % (b, s, len(phrases), CONS_MAX))
            total = 0
            for j, phrase in enumerate(phrases):
                if isinstance(phrase, (str, bytes)) or not hasattr(phrase, "__len__"):
                    raise ValueError("a phrase must be a list of ids, got %r (video %d sentence %d)" % (phrase, b, s))
                if not 1 <= len(phrase) <= CONS_LEN:
                    raise ValueError("a phrase holds 1..%d ids, got %d (video %d sentence %d)" % (CONS_LEN, len(phrase), b, s))
                for q, w in enumerate(phrase):
                    w = _as_int("a constraint id", w.item() if isinstance(w, torch.Tensor) and w.dim() == 0 else w)
                    if w in (PAD, BOS, EOS, UNK):
                        raise ValueError("a constraint id may not be PAD, BOS, EOS or UNK, got %d (video %d sentence %d)" % (w, b, s))
                    if not 0 <= w < int(c_list[b]):
                        raise ValueError("constraint id %d is outside the %d columns of video %d" % (w, int(c_list[b]), b))
                    rows[(t * CONS_MAX + j) * CONS_LEN + q] = w
                total += len(phrase)
            if total > lt - 2:
                raise ValueError("the phrases of video %d sentence %d hold %d ids, a caption has room for %d (Lt - 2)" % (b, s, total, lt - 2))
            t += 1
    return torch.tensor(rows, dtype=torch.int32).view(sum(steps), CONS_MAX, CONS_LEN)


def _check_cons(fn, cons, cstate, T, R, device):
    if cons.dtype != torch.int32 or tuple(cons.shape) != (T, CONS_MAX, CONS_LEN) or not cons.is_contiguous() or cons.device != device:
        raise ValueError("%s: cons must be a contiguous int32 (T, %d, %d) table on the scores' device" % (fn, CONS_MAX, CONS_LEN))
    if not _row_vec(cstate, R, torch.int32, device):
        raise ValueError("%s: cstate must be contiguous int32 (T·beam,) on the scores' device" % fn)


def beam_step_cons(scores, row_c, row_x, beam, pos, logits, unk, eos, pad, cum, cstate, finished, length, toks_in, toks_out, slot_rows, cons,
                   *, min_length=0, block_ngram_repeat=0, exclusion=None, lp=None):
    """One selection step of lexically constrained beam search (svpc_beam_step_cons): ``beam_step`` with controls whose sentences have up
    to CONS_MAX phrases that a caption must contain — ``cons`` the (T, CONS_MAX, CONS_LEN) int32 device table of ``check_constraints``,
    ``cstate`` (T·beam,) int32 the rows' tracker states (start 0).  In place: ``cum``, ``cstate``, ``finished``, ``length`` (required).
    → (parent, next_ext, next_model) int32 (T·beam,)."""
    (R, lt, dev), outs, args = _beam_step_shared("beam_step_cons", scores, row_c, row_x, beam, pos, logits, unk, eos, pad, cum, finished,
                                                 toks_in, toks_out, slot_rows)
    ctl = _beam_step_controls("beam_step_cons", R, lt, dev, length, min_length, block_ngram_repeat, lp, exclusion)
    _check_cons("beam_step_cons", cons, cstate, R // beam, R, dev)
    _need_gpu(scores)
    _lib.call("beam_step_cons", *args, *ctl, _p(cons), _p(cstate), _stream())
    return outs


def beam_finalize_cons(cum, ext, beam, n_best, cstate, length=None, lp=None):
    """→ (ids (T, n_best, Lt) int32, score (T, n_best) fp32, len (T, n_best) int32, met (T, n_best) int32): ``beam_finalize_nbest`` in the
    order of constrained beam search — rows with cum = −inf last; above them more constraints met (bits 0–3 of ``cstate``) first, then the
    higher (double)cum / lp[len], then the lower beam index — svpc_beam_finalize_cons."""
    return _beam_finalize_nbest("beam_finalize_cons", cum, ext, beam, n_best, length, lp, cstate)


def _check_finalize(cum, ext, beam, n_best=1):
    """the arguments the two final picks share → (T, Lt)"""
    if not 1 <= beam <= BEAM_MAX:
        raise ValueError("beam_finalize: beam width must be 1..%d" % BEAM_MAX)
    if not 1 <= n_best <= beam:
        raise ValueError("beam_finalize: n_best must be 1..%d, got %r" % (beam, n_best))
    R, lt = ext.shape
    if R % beam or not _row_vec(cum, R, torch.float32) or not _id_rows(ext, R, lt):
        raise ValueError("beam_finalize: cum fp32 (T·beam,) and ext int32 (T·beam, Lt), contiguous")
    return R // beam, lt


def beam_finalize(cum, ext, beam):
    """→ (ids (T, Lt) int32, score (T,) fp32): per sentence the hypothesis of highest ``cum`` (ties: lowest index) — svpc_beam_finalize."""
    T, lt = _check_finalize(cum, ext, beam)
    _need_gpu(ext)
    ids = torch.empty(T, lt, dtype=torch.int32, device=ext.device)
    score = torch.empty(T, dtype=torch.float32, device=ext.device)
    _lib.call("beam_finalize", _p(cum), _p(ext), lt, T, int(beam), lt, _p(ids), _p(score), _stream())
    return ids, score


def beam_finalize_nbest(cum, ext, beam, n_best, length=None, lp=None):
    """→ (ids (T, n_best, Lt) int32, score (T, n_best) fp32, len (T, n_best) int32): per sentence its ``n_best`` hypotheses in order of
    (double)cum / lp[len] (``lp`` None: cum), ties to the lower beam index — svpc_beam_finalize_nbest.  ``length`` (T·beam,) int32 (needed
    with ``lp``; None: len 0)."""
    return _beam_finalize_nbest("beam_finalize", cum, ext, beam, n_best, length, lp)


def _beam_finalize_nbest(fn, cum, ext, beam, n_best, length, lp, *cstate):
    """the body of the two n-best picks: ``cstate`` given → svpc_beam_finalize_cons and a fourth output, the constraints met"""
    T, lt = _check_finalize(cum, ext, beam, n_best)
    if length is not None and not _row_vec(length, T * beam, torch.int32):
        raise ValueError("%s: length must be contiguous int32 (T·beam,)" % fn)
    if lp is not None and (length is None or not _lp_table(lp, lt)):
        raise ValueError("%s: lp must be a contiguous float64 table of >= Lt entries, with length" % fn)
    if cstate and not _row_vec(cstate[0], T * beam, torch.int32, ext.device):
        raise ValueError("%s: cstate must be contiguous int32 (T·beam,) on the ids' device" % fn)
    _need_gpu(ext)
    outs = [torch.empty(T, n_best, lt, dtype=torch.int32, device=ext.device), torch.empty(T, n_best, dtype=torch.float32, device=ext.device)]
    outs += [torch.empty(T, n_best, dtype=torch.int32, device=ext.device) for _ in range(1 + len(cstate))]      # len [, met]
    _lib.call("beam_finalize_cons" if cstate else "beam_finalize_nbest", _p(cum), _p(length), _p(lp), _p(ext), *map(_p, cstate), lt, T,
              int(beam), lt, int(n_best), *map(_p, outs), _stream())
    return tuple(outs)


SAMPLE_COLS_MAX = 4096          # columns of a sample row (the draw index is r·4096 + c)


def check_sampling(lt, num_samples=1, random_sampling_temp=1.0, random_sampling_topk=0, random_sampling_topp=0.0, min_length=0,
                   seed=None, max_cols=None):
    """The settings of a random-sampling decode over Lt = ``lt`` positions, checked on the host (ValueError) and normalised → dict(
    num_samples R (1 … BEAM_MAX), random_sampling_temp τ (finite > 0), random_sampling_topk k (0: off; OpenNMT's −1 is taken as 0),
    random_sampling_topp q (in [0, 1]; 0 and 1: off), min_length m (0 … Lt − 1), seed (None or an int in [0, 2⁶³))).  ``max_cols``: the
    widest score row C_r = V + X of the batch (≤ SAMPLE_COLS_MAX)."""
    R = _as_int("num_samples", num_samples)
    if not 1 <= R <= BEAM_MAX:
        raise ValueError("num_samples must be 1..%d, got %d" % (BEAM_MAX, R))
    try:
        temp = float(random_sampling_temp)
    except (TypeError, ValueError):
        raise ValueError("random_sampling_temp must be a number, got %r" % (random_sampling_temp,))
    if not math.isfinite(temp) or temp <= 0:
        raise ValueError("random_sampling_temp must be finite and > 0, got %r" % (random_sampling_temp,))
    k = _as_int("random_sampling_topk", random_sampling_topk)
    if k < -1:
        raise ValueError("random_sampling_topk must be >= -1 (0 or -1: the full distribution), got %d" % k)
    try:
        q = float(random_sampling_topp)
    except (TypeError, ValueError):
        raise ValueError("random_sampling_topp must be a number, got %r" % (random_sampling_topp,))
    if not 0.0 <= q <= 1.0:                       # (NaN fails too)
        raise ValueError("random_sampling_topp must be in [0, 1], got %r" % (random_sampling_topp,))
    m = _as_int("min_length", min_length)
    if not 0 <= m <= lt - 1:
        raise ValueError("min_length must be 0..%d (Lt - 1), got %d" % (lt - 1, m))
    if seed is not None:
        seed = _as_int("seed", seed)
        if not 0 <= seed < 1 << 63:
            raise ValueError("seed must be None or an integer in [0, 2**63), got %d" % seed)
    if max_cols is not None and int(max_cols) > SAMPLE_COLS_MAX:
        raise ValueError("sampling reads score rows of at most %d columns (vocabulary + copied words), got %d" % (SAMPLE_COLS_MAX, max_cols))
    return dict(num_samples=R, random_sampling_temp=temp, random_sampling_topk=max(k, 0), random_sampling_topp=q, min_length=m, seed=seed)


def check_truncation(min_p=0.0, typical_p=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """The truncation settings of a sampling decode, checked on the host (ValueError for a non-number, a bool, NaN or a value out of
    range) and normalised → dict(min_p a (in [0, 1); 0: off), typical_p m (in [0, 1]; 0 and 1: off, 1 is returned as 0), epsilon_cutoff ε
    and eta_cutoff η (in [0, 1); 0: off)), all floats."""
    out = {}
    for name, v, closed in (("min_p", min_p, False), ("typical_p", typical_p, True), ("epsilon_cutoff", epsilon_cutoff, False),
                            ("eta_cutoff", eta_cutoff, False)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            raise ValueError("%s must be a number, got %r" % (name, v))
        f = float(v)
        if not (0.0 <= f <= 1.0 if closed else 0.0 <= f < 1.0):          # (NaN fails too)
            raise ValueError("%s must be in [0, 1%s, got %r" % (name, "]" if closed else ")", v))
        out[name] = f + 0.0                                               # (−0.0 → 0.0)
    if out["typical_p"] == 1.0:
        out["typical_p"] = 0.0
    return out


def _sample_step_checks(name, scores, row_c, cum, finished, length, text, ext, seed, pos, temp, topk, topp, min_length, max_cols):
    """the checks ``sample_step`` and ``sample_step_trunc`` share → (rows, Lt, the row_c index, max(row_c))"""
    R = cum.shape[0]
    if scores.dim() != 2 or scores.shape[0] != R or scores.stride(1) != 1 or scores.dtype != torch.float32:
        raise ValueError("%s: scores must be fp32 (T·R, C) rows with unit column stride" % name)
    for t, dt in ((cum, torch.float32), (finished, torch.int32), (length, torch.int32)):
        if not _row_vec(t, R, dt, scores.device):
            raise ValueError("%s: cum fp32, finished and length int32, all contiguous (T·R,) on the scores' device" % name)
    lt = text.shape[1]
    for m in (text, ext):
        if not _id_rows(m, R, lt, scores.device):
            raise ValueError("%s: id matrices must be contiguous int32 (T·R, Lt) on the scores' device" % name)
    if seed.dtype != torch.int64 or seed.numel() < 1 or seed.device != scores.device:
        raise ValueError("%s: seed must be a device int64 tensor" % name)
    if not 0 <= pos < lt - 1:
        raise ValueError("%s: position %d outside the %d-column matrices" % (name, pos, lt))
    if not (math.isfinite(temp) and temp > 0 and topk >= 0 and 0.0 <= topp <= 1.0 and 0 <= min_length < lt):
        raise ValueError("%s: temp finite > 0, topk >= 0, topp in [0, 1], min_length 0..Lt-1" % name)
    rc = as_idx(row_c)
    max_c = int(max_cols) if max_cols is not None else (max(rc.host) if R else 1)
    if max_c > SAMPLE_COLS_MAX or max_c > scores.shape[1]:
        raise ValueError("%s: rows of at most %d columns, inside the score matrix" % (name, SAMPLE_COLS_MAX))
    _need_gpu(scores)
    return R, lt, rc, max_c


def sample_step(scores, row_c, row_x, pos, logits, unk, eos, pad, cum, finished, length, text, ext, seed, *, temp=1.0, topk=0, topp=0.0,
                min_length=0, max_cols=None):
    """One random-sampling step (svpc_sample_step) over ``scores`` (T·R, ≥ C) — probabilities, or logits when ``logits``: every row draws
    its pick at position pos + 1 from its step scores / ``temp`` restricted to the top-``topk`` columns and the top-``topp`` mass (0: off),
    EOS barred while pos + 1 ≤ ``min_length``.  ``seed`` is a device int64 (1,) tensor (read by the kernel: a captured graph replays with
    whatever it holds).  ``cum`` fp32, ``finished`` / ``length`` int32 (T·R,) are updated in place, and column pos + 1 of the (T·R, Lt)
    int32 id matrices ``text`` / ``ext``.  ``max_cols``: max(row_c) when the caller knows it (else taken from the host copy).
    → (next_ext, next_model) int32 (T·R,)."""
    R, lt, rc, max_c = _sample_step_checks("sample_step", scores, row_c, cum, finished, length, text, ext, seed, pos, temp, topk, topp,
                                           min_length, max_cols)
    dev = scores.device
    nxt_ext = torch.empty(R, dtype=torch.int32, device=dev)
    nxt = torch.empty(R, dtype=torch.int32, device=dev)
    _lib.call("sample_step", _p(scores), scores.stride(0), _p(rc.dev(dev)), _p(as_idx(row_x).dev(dev)), R, int(max_c), int(pos),
              1 if logits else 0, int(unk), int(eos), int(pad), float(temp), int(topk), float(topp), int(min_length), _p(seed), _p(cum),
              _p(finished), _p(length), _p(text), _p(ext), lt, _p(nxt_ext), _p(nxt), _stream())
    return nxt_ext, nxt


def sample_step_trunc(scores, row_c, row_x, pos, logits, unk, eos, pad, cum, finished, length, text, ext, seed, *, temp=1.0, topk=0,
                      topp=0.0, min_length=0, max_cols=None, min_p=0.0, typical_p=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0, kept=None):
    """``sample_step`` with the four truncation stages of ``check_truncation`` between top-p and the draw (svpc_sample_step_trunc; min-p,
    locally typical, epsilon and eta, in this order, each off at 0, each over the distribution renormalised over what the stage before
    left).  Everything else — arguments, checks, what is updated in place — is ``sample_step``'s; with all four off so are the results,
    bit for bit.  → (next_ext, next_model, kept) int32 (T·R,): ``kept`` is the size of the set each live row drew from (0 for a
    finished row or one without candidates), written into ``kept`` when the caller brings one."""
    R, lt, rc, max_c = _sample_step_checks("sample_step_trunc", scores, row_c, cum, finished, length, text, ext, seed, pos, temp, topk,
                                           topp, min_length, max_cols)
    tr = check_truncation(min_p, typical_p, epsilon_cutoff, eta_cutoff)
    dev = scores.device
    nxt_ext = torch.empty(R, dtype=torch.int32, device=dev)
    nxt = torch.empty(R, dtype=torch.int32, device=dev)
    if kept is None:
        kept = torch.empty(R, dtype=torch.int32, device=dev)
    elif not _row_vec(kept, R, torch.int32, dev):
        raise ValueError("sample_step_trunc: kept must be a contiguous int32 (T·R,) tensor on the scores' device")
    _lib.call("sample_step_trunc", _p(scores), scores.stride(0), _p(rc.dev(dev)), _p(as_idx(row_x).dev(dev)), R, int(max_c), int(pos),
              1 if logits else 0, int(unk), int(eos), int(pad), float(temp), int(topk), float(topp), int(min_length), _p(seed), _p(cum),
              _p(finished), _p(length), _p(text), _p(ext), lt, _p(nxt_ext), _p(nxt), tr["min_p"], tr["typical_p"], tr["epsilon_cutoff"],
              tr["eta_cutoff"], _p(kept), _stream())
    return nxt_ext, nxt, kept


def sample_seed(src, word, used):
    """The seed of one sampling decode, on the device (svpc_sample_seed): ``src`` int64 (2,) = (fixed, value); fixed: ``used`` = value,
    otherwise ``used`` is drawn from the seed word ``word`` (int64 (1,)), which advances.  All three device tensors."""
    for t, n in ((src, 2), (word, 1), (used, 1)):
        if t.dtype != torch.int64 or t.numel() != n or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("sample_seed: src int64 (2,), word and used int64 (1,), contiguous device tensors")
    _need_gpu(src)
    _lib.call("sample_seed", _p(src), _p(word), _p(used), _stream())
    return used


ENSEMBLE_MAX = 8                # members of one ensemble: the kernel's argument struct holds their pointers by value
ENSEMBLE_RULES = {"prob": 0, "logprob": 1}


def ensemble_weights(weights, n):
    """The fp64 weights of an ``n``-member ensemble, normalised to sum 1 (None: uniform; the sum is taken in member order and every
    weight divided by it) → a list of floats.  ValueError for a wrong count, ``n`` outside 1..8, a negative or non-finite weight, and
    weights that are all zero."""
    if not 1 <= n <= ENSEMBLE_MAX:
        raise ValueError("an ensemble has 1..%d members, got %d" % (ENSEMBLE_MAX, n))
    w = [1.0] * n if weights is None else [float(v) for v in weights]
    if len(w) != n:
        raise ValueError("ensemble: %d weights for %d members" % (len(w), n))
    total = 0.0
    for v in w:
        total += v
    if not all(math.isfinite(v) and v >= 0 for v in w) or not (total > 0 and math.isfinite(total)):
        raise ValueError("ensemble: weights must be finite, >= 0 and not all zero, got %r" % (w,))
    return [v / total for v in w]


def ensemble_combine(scores_list, row_c, *, weights, rule, logits, unk, rows_per=1, max_cols=None):
    """The members' score matrices of one decoding step combined into ONE probability matrix (svpc_ensemble_combine):
    ``scores_list`` M fp32 (n_rows, ≥ C) matrices with unit column stride (each its own row stride) — probabilities, or logits when
    ``logits`` —, ``row_c`` the column counts (row r has C = row_c[r // rows_per] columns), ``weights`` M non-negative numbers (normalised
    here; None: uniform; a zero-weight member is never read), ``rule`` "prob" (the weighted mean of the members' probabilities) or
    "logprob" (exp of the weighted mean of their log-probabilities, not renormalised).  → out (n_rows, max_c) fp32 probabilities (0 in
    the UNK column in logits mode and past a row's C): what the step kernels take with ``logits=False``.  The member pointers travel as
    kernel arguments: nothing is uploaded."""
    if rule not in ENSEMBLE_RULES:
        raise ValueError("ensemble_combine: rule must be one of %s, got %r" % (", ".join(ENSEMBLE_RULES), rule))
    ms = list(scores_list)
    w = ensemble_weights(weights, len(ms))
    for s in ms:
        if s.dim() != 2 or s.dtype != torch.float32 or (s.stride(1) != 1 and s.shape[1] != 1):
            raise ValueError("ensemble_combine: every member's scores must be an fp32 (rows, C) matrix with unit column stride")
    n_rows, dev = ms[0].shape[0], ms[0].device
    if any(s.shape[0] != n_rows or s.device != dev for s in ms):
        raise ValueError("ensemble_combine: the members' score matrices must have the same rows on the same device")
    if int(rows_per) < 1:
        raise ValueError("ensemble_combine: rows_per must be >= 1")
    rc = as_idx(row_c)
    if len(rc) * int(rows_per) < n_rows:
        raise ValueError("ensemble_combine: %d column counts for %d rows (%d rows each)" % (len(rc), n_rows, rows_per))
    max_c = int(max_cols) if max_cols is not None else (max(rc.host) if n_rows else 1)
    if not 1 <= max_c <= SAMPLE_COLS_MAX or any(max_c > s.shape[1] for s in ms):
        raise ValueError("ensemble_combine: rows of 1..%d columns, inside every score matrix" % SAMPLE_COLS_MAX)
    _need_gpu(ms[0])
    out = torch.empty(n_rows, max_c, dtype=torch.float32, device=dev)
    if n_rows == 0:
        return out
    M = len(ms)
    _lib.call("ensemble_combine", (ctypes.c_void_p * M)(*[s.data_ptr() for s in ms]), (ctypes.c_int * M)(*[s.stride(0) for s in ms]),
              (ctypes.c_double * M)(*w), M, _p(rc.dev(dev)), int(rows_per), n_rows, max_c, 1 if logits else 0, int(unk),
              ENSEMBLE_RULES[rule], _p(out), out.stride(0), _stream())
    return out


def contrast_coefficients(expert_weight, amateur_weight, alpha, who="contrast_combine"):
    """(we, wa, α, log α) as the kernel takes them: fp64, ``log α`` from ``math.log`` (−inf for α = 0).  ValueError for an expert weight
    that is not finite or ≤ 0, an amateur weight that is not finite or < 0, and an α outside [0, 1] or NaN."""
    try:
        we, wa, al = float(expert_weight), float(amateur_weight), float(alpha)
    except (TypeError, ValueError):
        raise ValueError("%s: expert_weight, amateur_weight and alpha must be numbers, got %r, %r, %r"
                         % (who, expert_weight, amateur_weight, alpha))
    if not (math.isfinite(we) and we > 0):
        raise ValueError("%s: expert_weight must be finite and > 0, got %r" % (who, expert_weight))
    if not (math.isfinite(wa) and wa >= 0):
        raise ValueError("%s: amateur_weight must be finite and >= 0, got %r" % (who, amateur_weight))
    if not 0.0 <= al <= 1.0:
        raise ValueError("%s: alpha must lie in [0, 1], got %r" % (who, alpha))
    return we, wa, al, (math.log(al) if al > 0 else -math.inf)


def contrast_combine(expert, amateur, row_c, *, expert_weight, amateur_weight, alpha, logits, unk, rows_per=1, max_cols=None):
    """Contrastive decoding's step rule (svpc_contrast_combine): an expert's score matrix held against an amateur's.
    ``expert`` / ``amateur`` fp32 (n_rows, ≥ C) matrices with unit column stride (each its own row stride) — probabilities, or logits
    when ``logits`` —, ``row_c`` the column counts (row r has C = row_c[r // rows_per] columns).  Over the head — the columns whose
    expert probability is at least ``alpha`` times the row's highest, UNK never among them — out is the softmax of
    ``expert_weight``·log p_expert − ``amateur_weight``·max(log p_amateur, log 1e-30); everything else is 0.  With
    ``amateur_weight == 0`` the amateur's matrix is checked but never read.  → out (n_rows, max_c) fp32: a distribution over the head,
    what the step kernels take with ``logits=False``.  The coefficients travel as kernel arguments: nothing is uploaded."""
    we, wa, al, log_al = contrast_coefficients(expert_weight, amateur_weight, alpha)
    ms = [expert, amateur]
    for s in ms:
        if not isinstance(s, torch.Tensor) or s.dim() != 2 or s.dtype != torch.float32 or (s.stride(1) != 1 and s.shape[1] != 1):
            raise ValueError("contrast_combine: the expert's and the amateur's scores must be fp32 (rows, C) matrices with unit column stride")
    n_rows, dev = expert.shape[0], expert.device
    if amateur.shape[0] != n_rows or amateur.device != dev:
        raise ValueError("contrast_combine: the two score matrices must have the same rows on the same device")
    if int(rows_per) < 1:
        raise ValueError("contrast_combine: rows_per must be >= 1")
    rc = as_idx(row_c)
    if len(rc) * int(rows_per) < n_rows:
        raise ValueError("contrast_combine: %d column counts for %d rows (%d rows each)" % (len(rc), n_rows, rows_per))
    max_c = int(max_cols) if max_cols is not None else (max(rc.host) if n_rows else 1)
    if not 1 <= max_c <= SAMPLE_COLS_MAX or any(max_c > s.shape[1] for s in ms):
        raise ValueError("contrast_combine: rows of 1..%d columns, inside both score matrices" % SAMPLE_COLS_MAX)
    _need_gpu(expert)
    out = torch.empty(n_rows, max_c, dtype=torch.float32, device=dev)
    if n_rows == 0:
        return out
    _lib.call("contrast_combine", _p(expert), expert.stride(0), _p(amateur), amateur.stride(0), ctypes.c_double(we), ctypes.c_double(wa),
              ctypes.c_double(al), ctypes.c_double(log_al), _p(rc.dev(dev)), int(rows_per), n_rows, max_c, 1 if logits else 0, int(unk),
              _p(out), out.stride(0), _stream())
    return out


CAPTION_LT_MAX = 64             # a caption row: one lane per position
CAPTION_VIDEO_WORDS = 4096      # positions (S_b · Lt) of one video's captions: the words live in the workgroup's LDS
CAPTION_COUNT_COLS = 12         # total_1..4, distinct_1..4, n_sen, n_words, n_empty, n_copied
_NO_ID = -(1 << 31)             # "no such id" for the punctuation rule


def check_caption_metrics(lt, ids_dtype=None, steps=None, k=None, row=None, period_id=None, comma_id=None):
    """Host checks of the caption clean-up / counters (ValueError): ``lt`` ≤ 64 positions per row; ids int32 or int64; every video's
    ``steps[b]`` · lt ≤ 4096 positions; ``row`` inside the ``k`` rows per sentence of a 3-D result (None or 0 for a 2-D one); the two
    punctuation ids different.  → (row index, period, comma) as the kernels take them."""
    if not 1 <= int(lt) <= CAPTION_LT_MAX:
        raise ValueError("caption rows hold 1..%d positions, got Lt = %d" % (CAPTION_LT_MAX, lt))
    if ids_dtype is not None and ids_dtype not in (torch.int32, torch.int64):
        raise ValueError("caption ids must be int32 or int64, got %s" % (ids_dtype,))
    for s in steps or ():
        if int(s) < 0 or int(s) * int(lt) > CAPTION_VIDEO_WORDS:
            raise ValueError("a video's captions hold at most %d positions (S_b · Lt), got %d · %d" % (CAPTION_VIDEO_WORDS, s, lt))
    if isinstance(row, bool) or (row is not None and not isinstance(row, numbers.Integral)):
        raise ValueError("row must be an integer, got %r" % (row,))
    r = 0 if row is None else int(row)
    if not 0 <= r < (1 if k is None else int(k)):
        raise ValueError("row %d outside the %d row(s) per sentence" % (r, 1 if k is None else int(k)))
    for name, v in (("period_id", period_id), ("comma_id", comma_id)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= int(v) < (1 << 31)):
            raise ValueError("%s must be None or a token id, got %r" % (name, v))
    if period_id is not None and period_id == comma_id:
        raise ValueError("period_id and comma_id must differ, both are %d" % period_id)
    return r, (_NO_ID if period_id is None else int(period_id)), (_NO_ID if comma_id is None else int(comma_id))


def _clean_pair(fn, words, length):
    """``words`` (T, Lt) / ``length`` (T,) are contiguous int32 as ``clean_captions`` returns them → (T, Lt)"""
    if words.dim() != 2 or words.dtype != torch.int32 or not words.is_contiguous():
        raise ValueError("%s: words must be contiguous int32 (T, Lt)" % fn)
    T, lt = words.shape
    if not _row_vec(length, T, torch.int32):
        raise ValueError("%s: len must be contiguous int32 (T,)" % fn)
    return T, lt


def _plan_rows(fn, plan, steps, T, signed=False):
    """``steps`` gives the plan's videos' row counts and they add up to T (``signed``: a negative count passes here)"""
    if len(steps) != plan.n_vid or sum(steps) != T or (not signed and any(s < 0 for s in steps)):
        raise ValueError("%s: the plan's %d video(s) with rows %r do not add up to T = %d" % (fn, plan.n_vid, steps, T))


def _plan_device(fn, plan, t, what):
    if plan.buf.device != t.device:
        raise ValueError("%s: the plan lives on %s, the %s on %s" % (fn, plan.buf.device, what, t.device))


def _accumulator(fn, name, acc, dtype, n, like, what):
    """``acc`` is a contiguous tensor of ``n`` elements of ``dtype`` on the device of ``like`` (the caller's ``what``)"""
    if acc.dtype != dtype or acc.numel() != n or not acc.is_contiguous() or acc.device != like.device:
        raise ValueError("%s: %s must be a contiguous %s (%d,) tensor on the %s' device" % (fn, name, str(dtype)[6:], n, what))


def clean_captions(ids, pad, eos, ignore=-1, remove_dup=True, row=None):
    """The captions the reference submits, from decoded ids (svpc_caption_clean): ``ids`` (T, Lt) or (T, K, Lt) int64 / int32 (``row``
    picks one of the K rows per sentence, default 0) → (words (T, Lt) int32: the ids without ``pad`` / ``ignore``, without the first of
    those, up to the first ``eos``, runs collapsed when ``remove_dup`` — left-aligned, ``pad``-filled; len (T,) int32)."""
    if ids.dim() not in (2, 3):
        raise ValueError("clean_captions: ids must be (T, Lt) or (T, K, Lt), got %s" % (tuple(ids.shape),))
    lt = ids.shape[-1]
    k = ids.shape[1] if ids.dim() == 3 else None
    r, _, _ = check_caption_metrics(lt, ids.dtype, k=k, row=row)
    _need_gpu(ids)
    ids = _c(ids)
    T = ids.shape[0]
    words = torch.empty(T, lt, dtype=torch.int32, device=ids.device)
    ln = torch.empty(T, dtype=torch.int32, device=ids.device)
    _lib.call("caption_clean", _p(ids), 1 if ids.dtype == torch.int64 else 0, lt, 1 if k is None else int(k), r, T, lt, int(pad), int(eos),
              int(ignore), 1 if remove_dup else 0, _p(words), _p(ln), _stream())
    return words, ln


def caption_ngram_counts(words, length, vid_off, V, period_id=None, comma_id=None, vocab_bits=None, steps=None):
    """Per-video n-gram counts of clean captions (svpc_caption_ngram_counts): ``words`` (T, Lt) / ``length`` (T,) int32 as
    ``clean_captions`` returns them, ``vid_off`` (N + 1,) int32 device tensor (or a host list, uploaded) of the videos' first rows →
    counts (N, 12) int32: total_1..4, distinct_1..4, n_sen, n_words, n_empty, n_copied.  ``vocab_bits``: an int32 device bitmap of
    ≥ ⌈V / 32⌉ words that collects the ids < V seen.  ``steps``: the videos' row counts when the caller knows them (a device ``vid_off``
    is not read back to check the 4096-position cap)."""
    T, lt = _clean_pair("caption_ngram_counts", words, length)
    if not torch.is_tensor(vid_off):
        off = [int(v) for v in vid_off]
        if steps is None:
            steps = [b - a for a, b in zip(off[:-1], off[1:])]
        if not off or off[0] != 0 or off[-1] != T:
            raise ValueError("caption_ngram_counts: vid_off must run from 0 to T = %d" % T)
    elif vid_off.dtype != torch.int32 or vid_off.dim() != 1 or vid_off.shape[0] < 1 or not vid_off.is_contiguous():
        raise ValueError("caption_ngram_counts: vid_off must be a contiguous int32 (N + 1,) tensor")
    _, period, comma = check_caption_metrics(lt, steps=steps, period_id=period_id, comma_id=comma_id)
    if steps is not None and sum(int(s) for s in steps) != T:
        raise ValueError("caption_ngram_counts: the videos' rows must add up to T = %d" % T)
    if not 0 <= int(V) < (1 << 31):
        raise ValueError("caption_ngram_counts: vocabulary size must be >= 0, got %r" % (V,))
    if vocab_bits is not None and (vocab_bits.dtype != torch.int32 or not vocab_bits.is_contiguous() or vocab_bits.numel() * 32 < V
                                   or vocab_bits.device != words.device):
        raise ValueError("caption_ngram_counts: vocab_bits must be a contiguous int32 bitmap of >= V bits on the words' device")
    _need_gpu(words)
    if not torch.is_tensor(vid_off):
        vid_off = torch.tensor(off, dtype=torch.int32, device=words.device)
    N = vid_off.shape[0] - 1
    counts = torch.empty(N, CAPTION_COUNT_COLS, dtype=torch.int32, device=words.device)
    _lib.call("caption_ngram_counts", _p(words), _p(length), _p(vid_off), N, lt, period, comma, int(V), _p(counts), _p(vocab_bits), _stream())
    return counts


def decode_metric_accum(counts, acc):
    """acc (13,) float64 += Σ over the rows of ``counts`` of (re_1..4, div_1..4, 1, n_sen, n_words, n_empty, n_copied) —
    svpc_decode_metric_accum (fixed summation order)."""
    if counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[1] != CAPTION_COUNT_COLS or not counts.is_contiguous():
        raise ValueError("decode_metric_accum: counts must be contiguous int32 (N, %d)" % CAPTION_COUNT_COLS)
    _accumulator("decode_metric_accum", "acc", acc, torch.float64, 13, counts, "counts")
    _need_gpu(counts)
    _lib.call("decode_metric_accum", _p(counts), counts.shape[0], _p(acc), _stream())
    return acc


def stack_captions(dec_seq_list):
    """A decode's per-video id tensors ((S_b, Lt) or (S_b, K, Lt)) as one (T, …) tensor and the S_b: zero-copy when they are consecutive
    views of one buffer (what the translator returns; ``model._stacked``'s test), else one ``torch.cat``."""
    if not len(dec_seq_list):
        raise ValueError("no captions: an empty list of videos")
    t0 = dec_seq_list[0]
    steps = [int(t.shape[0]) for t in dec_seq_list]
    if any(t.dim() != t0.dim() or t.shape[1:] != t0.shape[1:] or t.dtype != t0.dtype or t.device != t0.device for t in dec_seq_list):
        raise ValueError("the videos' id tensors must agree in dtype, device and all dimensions but the first")
    if t0.dim() not in (2, 3):
        raise ValueError("per-video ids must be (S_b, Lt) or (S_b, K, Lt), got %s" % (tuple(t0.shape),))
    if len(dec_seq_list) == 1:
        return _c(t0), steps
    per = t0[0].numel() * t0.element_size() if steps[0] else 0
    ptr, ok = t0.data_ptr(), per > 0
    for t, s in zip(dec_seq_list, steps):
        ok = ok and t.is_contiguous() and t.data_ptr() == ptr
        ptr += s * per
    root = t0._base
    if ok and root is not None and root.is_contiguous() and root.dtype == t0.dtype:
        start = (t0.data_ptr() - root.data_ptr()) // t0.element_size()
        n = sum(steps) * t0[0].numel()
        flat = root.reshape(-1)
        if 0 <= start and start + n <= flat.numel():
            return flat[start:start + n].view(sum(steps), *t0.shape[1:]), steps
    return torch.cat(list(dec_seq_list)), steps


def caption_ingredients(words, length, plan, acc=None, steps=None):
    """Which ingredients clean captions mention, and the ingredient-F1 counts against the plan's ground truth (svpc_caption_ingredients;
    DESIGN §11.5): ``words`` (T, Lt) / ``length`` (T,) int32 as ``clean_captions`` returns them (run collapse on), ``plan`` an
    ``ingredients.IngredientPlan``, ``steps`` the videos' row counts (default: their ground-truth step counts), ``acc`` a contiguous int64
    (3,) device tensor (correct, precision total = Σ len(generated list), recall total = Σ len(ground-truth list); None: nothing
    accumulated) →
    (masks (T,) int64: bit e = listed ingredient e of the row's video is mentioned; extra (T,) int32 extra words;
    row_counts (T, 3) int32 = correct, len(generated list), len(ground-truth list), zeros for a row without a ground-truth step;
    vid_counts (N, 3) int32 their sums per video).  Two launches, nothing uploaded for a recurring (S_b) structure."""
    T, lt = _clean_pair("caption_ingredients", words, length)
    check_caption_metrics(lt)
    steps = plan.default_steps() if steps is None else [int(s) for s in steps]
    _plan_rows("caption_ingredients", plan, steps, T, signed=True)          # (a negative count is plan.rows' error, below)
    _plan_device("caption_ingredients", plan, words, "captions")
    if acc is not None:
        _accumulator("caption_ingredients", "acc", acc, torch.int64, 3, words, "captions")
    _need_gpu(words)
    rows = plan.rows(steps)
    lex, N = plan.lexicon, plan.n_vid
    dev = words.device
    masks = torch.empty(T, dtype=torch.int64, device=dev)
    extra = torch.empty(T, dtype=torch.int32, device=dev)
    row_counts = torch.empty(T, 3, dtype=torch.int32, device=dev)
    vid_counts = torch.empty(N, 3, dtype=torch.int32, device=dev)
    _lib.call("caption_ingredients", _p(words), _p(length), T, lt, rows.data_ptr(), rows.data_ptr() + 4 * (N + 1), N,
              _p(lex.table), lex.W, lex.n_rows, _p(lex.a_bits), lex.V, plan.ptr("vid"), plan.ptr("ing_tok"), plan.ptr("tok_row"),
              plan.ptr("tok_oov"), plan.ptr("eq_ids"), plan.ptr("oov_a"), plan.ptr("gt_mask"), plan.ptr("gt_len"), plan.ptr("gx_off"),
              plan.ptr("gx_ids"), _p(masks), _p(extra), _p(row_counts), _p(vid_counts), _p(acc), _stream())
    return masks, extra, row_counts, vid_counts


CAPTION_TOKENS = 1024           # tokens of one video's hypothesis paragraph (and of a reference): they live in the workgroup's LDS
CAPTION_SCORE_COUNT_COLS = 11   # correct_1..4, guess_1..4, testlen, reflen, lcs
CAPTION_SCORE_COLS = 6          # Bleu_1..4, ROUGE_L, CIDEr


def caption_tokens(words, length, plan, steps):
    """The token stream of every video's clean captions (svpc_caption_tokens): ``words`` (T, Lt) / ``length`` (T,) int32 as
    ``clean_captions`` returns them (run collapse on), ``plan`` a ``caption_scores.ScorePlan``, ``steps`` the videos' row counts →
    (tokens (N, 1024) int32 lexicon ids, zero past the end; tok_len (N,) int32).  ValueError when a video's hypothesis could exceed 1,024
    tokens (S_b · (Lt − 1) · the longest expansion of a word)."""
    T, lt = _clean_pair("caption_tokens", words, length)
    steps = [int(s) for s in steps]
    check_caption_metrics(lt)
    _plan_rows("caption_tokens", plan, steps, T)
    plan.check_cap(steps, lt)
    _plan_device("caption_tokens", plan, words, "captions")
    _need_gpu(words)
    cp, N = plan.corpus, plan.n_vid
    vid_off = plan.vid_off(steps)
    tokens = torch.empty(N, CAPTION_TOKENS, dtype=torch.int32, device=words.device)
    tok_len = torch.empty(N, dtype=torch.int32, device=words.device)
    _lib.call("caption_tokens", _p(words), _p(length), _p(vid_off), N, lt, cp.V, _p(cp.voc_off), _p(cp.voc_tok), cp.voc_tok.numel(),
              plan.ptr("vid"), plan.ptr("oov_off"), plan.size("oov_off"), plan.ptr("oov_tok"), plan.size("oov_tok"), _p(tokens), _p(tok_len),
              _stream())
    return tokens, tok_len


def caption_score_counts(tokens, tok_len, plan, seen=None):
    """Per-video Bleu / ROUGE_L / CIDEr counts and scores (svpc_caption_score_counts): ``tokens`` (N, 1024) / ``tok_len``
    (N,) int32 as ``caption_tokens`` returns them, ``plan`` the same ``ScorePlan``; ``seen``: a contiguous int64 device tensor with one
    entry per video of the reference set (the entries of this batch's videos are set to 1) →
    (counts (N, 11) int32: correct_1..4, guess_1..4, testlen, reflen, the largest LCS; scores (N, 6) float64: the video's own Bleu_1..4,
    ROUGE_L, CIDEr)."""
    N = plan.n_vid
    if tokens.dtype != torch.int32 or tuple(tokens.shape) != (N, CAPTION_TOKENS) or not tokens.is_contiguous():
        raise ValueError("caption_score_counts: tokens must be contiguous int32 (%d, %d)" % (N, CAPTION_TOKENS))
    if tok_len.dtype != torch.int32 or tuple(tok_len.shape) != (N,) or not tok_len.is_contiguous():
        raise ValueError("caption_score_counts: tok_len must be contiguous int32 (%d,)" % N)
    _plan_device("caption_score_counts", plan, tokens, "tokens")
    cp = plan.corpus
    if seen is not None:
        _accumulator("caption_score_counts", "seen", seen, torch.int64, cp.n_docs, tokens, "tokens")
    _need_gpu(tokens)
    counts = torch.empty(N, CAPTION_SCORE_COUNT_COLS, dtype=torch.int32, device=tokens.device)
    scores = torch.empty(N, CAPTION_SCORE_COLS, dtype=torch.float64, device=tokens.device)
    _lib.call("caption_score_counts", _p(tokens), _p(tok_len), N, plan.ptr("vid"), plan.ptr("ref_norm"), _p(cp.ref_tok), cp.n_ref_tok,
              _p(cp.tab_key), _p(cp.tab_idf), cp.table_capacity, cp.log_docs, _p(cp.gauss), _p(counts), _p(scores), _p(seen),
              0 if seen is None else cp.n_docs, _stream())
    return counts, scores


def caption_score_accum(counts, scores, acc_i, acc_f):
    """acc_i (11,) int64 += Σ (correct_1..4, guess_1..4, testlen, reflen, 1), acc_f (2,) float64 += Σ (ROUGE_L, CIDEr) over the rows —
    svpc_caption_score_accum (integer adds; the fp64 sums in a fixed order)."""
    if counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[1] != CAPTION_SCORE_COUNT_COLS or not counts.is_contiguous():
        raise ValueError("caption_score_accum: counts must be contiguous int32 (N, %d)" % CAPTION_SCORE_COUNT_COLS)
    if scores.dtype != torch.float64 or tuple(scores.shape) != (counts.shape[0], CAPTION_SCORE_COLS) or not scores.is_contiguous():
        raise ValueError("caption_score_accum: scores must be contiguous float64 (N, %d)" % CAPTION_SCORE_COLS)
    _accumulator("caption_score_accum", "acc_i", acc_i, torch.int64, 11, counts, "counts")
    _accumulator("caption_score_accum", "acc_f", acc_f, torch.float64, 2, counts, "counts")
    _need_gpu(counts)
    _lib.call("caption_score_accum", _p(counts), _p(scores), counts.shape[0], _p(acc_i), _p(acc_f), _stream())
    return acc_i, acc_f


CONSENSUS_MAX = 16              # candidates of one group: their token streams (≤ 16 · 1,028 16-bit tokens) sit in the workgroup's LDS
CONSENSUS_UTILITIES = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")
CONSENSUS_SCOPES = ("paragraph", "sentence")
CONSENSUS_WEIGHTS = ("uniform", "posterior")


def check_consensus(k=None, utility="CIDEr", scope="paragraph", weights="uniform", scores=True):
    """Host checks of consensus selection (ValueError): 1 ≤ ``k`` ≤ 16 candidates, ``utility`` one of the six score
    columns, ``scope`` "paragraph" or "sentence", ``weights`` "uniform" or "posterior" (which needs the candidates' ``scores``) →
    the utility's column."""
    if k is not None and (isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= int(k) <= CONSENSUS_MAX):
        raise ValueError("consensus selection takes 1..%d candidates, got K = %r" % (CONSENSUS_MAX, k))
    if utility not in CONSENSUS_UTILITIES:
        raise ValueError("utility must be one of %s, got %r" % (", ".join(CONSENSUS_UTILITIES), utility))
    if scope not in CONSENSUS_SCOPES:
        raise ValueError("scope must be one of %s, got %r" % (", ".join(CONSENSUS_SCOPES), scope))
    if weights not in CONSENSUS_WEIGHTS:
        raise ValueError("weights must be one of %s, got %r" % (", ".join(CONSENSUS_WEIGHTS), weights))
    if weights == "posterior" and scores is None:
        raise ValueError("weights=\"posterior\" needs the candidates' scores")
    return CONSENSUS_UTILITIES.index(utility)


def _candidates(fn, ids, plan, steps):
    """``ids`` is a decode's stacked (T, K, Lt) result of the plan's videos → (T, K, Lt, steps)"""
    if ids.dim() != 3:
        raise ValueError("%s: ids must be (T, K, Lt), got %s" % (fn, tuple(ids.shape)))
    T, K, lt = ids.shape
    check_consensus(K)
    check_caption_metrics(lt, ids.dtype)
    steps = [int(s) for s in steps]
    _plan_rows(fn, plan, steps, T)
    _plan_device(fn, plan, ids, "ids")
    return T, K, lt, steps


def consensus_pair_scores(ids, plan, steps, pad, eos, ignore=-1, scope="paragraph"):
    """Every candidate of a group scored against every other (svpc_caption_clean over the T · K rows, svpc_consensus_tokens,
    svpc_consensus_pair_scores: four launches whatever N and K): ``ids`` (T, K, Lt) int64 / int32 as
    ``translate_batch_sample`` / ``translate_batch_nbest`` return them (stacked; cleaned as ``clean_captions`` does with ``pad`` /
    ``eos`` / ``ignore``, run collapse on), ``plan`` a ``ScorePlan`` of the same videos (with or without references: only its copied
    words and its corpus's idf are used), ``steps`` the videos' row counts.  ``scope``:
    "paragraph" — one group per video, candidate k is row k of all its sentences; "sentence" — one group per sentence →
    (pair (G, K, K, 6) float64: pair[g, i, j] = Bleu_1..4, ROUGE_L, CIDEr of candidate i against the single reference j;
    tok_len (G, K) int32).  ValueError when a candidate's stream could exceed 1,024 tokens."""
    T, K, lt, steps = _candidates("consensus_pair_scores", ids, plan, steps)
    check_consensus(K, scope=scope)
    plan.check_cap(steps if scope == "paragraph" else [min(s, 1) for s in steps], lt)
    _need_gpu(ids)
    ids = _c(ids)
    dev = ids.device
    table, G = plan.groups(steps, K, scope)
    cp = plan.corpus
    words = torch.empty(T * K, lt, dtype=torch.int32, device=dev)
    ln = torch.empty(T * K, dtype=torch.int32, device=dev)
    tokens = torch.empty(G * K, CAPTION_TOKENS, dtype=torch.int16, device=dev)
    tok_len = torch.empty(G, K, dtype=torch.int32, device=dev)
    pair = torch.empty(G, K, K, CAPTION_SCORE_COLS, dtype=torch.float64, device=dev)
    work = torch.empty(G, K, 4, dtype=torch.float64, device=dev)                   # the candidates' squared CIDEr norms
    if T:
        _lib.call("caption_clean", _p(ids), 1 if ids.dtype == torch.int64 else 0, lt, 1, 0, T * K, lt, int(pad), int(eos), int(ignore), 1,
                  _p(words), _p(ln), _stream())             # the (T, K, Lt) ids as T · K rows
    _lib.call("consensus_tokens", _p(words), _p(ln), T * K, _p(table), G * K, lt, cp.V, _p(cp.voc_off), _p(cp.voc_tok), cp.voc_tok.numel(),
              plan.ptr("vid"), plan.n_vid, plan.ptr("oov_off"), plan.size("oov_off"), plan.ptr("oov_tok"), plan.size("oov_tok"), _p(tokens),
              _p(tok_len), _stream())
    _lib.call("consensus_pair_scores", _p(tokens), _p(tok_len), G, K, _p(cp.tab_key), _p(cp.tab_idf), cp.table_capacity, cp.log_docs,
              _p(cp.gauss), _p(pair), _p(work), _stream())
    return pair, tok_len


def consensus_pick(pair, ids, plan, steps, utility="CIDEr", scope="paragraph", weights="uniform", scores=None, lengths=None):
    """The expected utility of every candidate, the pick of every group and the chosen rows, in one launch (svpc_consensus_pick; DESIGN
    §11.7): ``pair`` (G, K, K, 6) float64 as ``consensus_pair_scores`` returns it for the same ``ids`` / ``plan`` / ``steps`` /
    ``scope``; ``scores`` (T, K) float32 cumulative scores and ``lengths`` (T, K) int64 as the decode returns them (optional;
    ``weights="posterior"`` needs ``scores``) → a dict: ``pick`` (G,) int32, ``expected`` (G, K) float64, ``ids`` (T, Lt) int64 the
    chosen row of every sentence, ``row_pick`` (T,) int64 its index, ``scores`` (T,) float32 / ``lengths`` (T,) int64 or None."""
    col = check_consensus(None, utility, scope, weights, scores)
    T, K, lt, steps = _candidates("consensus_pick", ids, plan, steps)
    table, G = plan.groups(steps, K, scope)
    if pair.dtype != torch.float64 or tuple(pair.shape) != (G, K, K, CAPTION_SCORE_COLS) or not pair.is_contiguous() or pair.device != ids.device:
        raise ValueError("consensus_pick: pair must be contiguous float64 (%d, %d, %d, %d) on the ids' device" % (G, K, K, CAPTION_SCORE_COLS))
    for name, t, dt in (("scores", scores, torch.float32), ("lengths", lengths, torch.int64)):
        if t is not None and (t.dtype != dt or tuple(t.shape) != (T, K) or t.device != ids.device):
            raise ValueError("consensus_pick: %s must be %s (%d, %d) on the ids' device" % (name, str(dt)[6:], T, K))
    _need_gpu(ids)
    ids = _c(ids)
    scores = None if scores is None else _c(scores)
    lengths = None if lengths is None else _c(lengths)
    dev = ids.device
    pick = torch.empty(G, dtype=torch.int32, device=dev)
    expected = torch.empty(G, K, dtype=torch.float64, device=dev)
    out_ids = torch.empty(T, lt, dtype=torch.int64, device=dev)
    row_pick = torch.empty(T, dtype=torch.int64, device=dev)
    out_scores = None if scores is None else torch.empty(T, dtype=torch.float32, device=dev)
    out_len = None if lengths is None else torch.empty(T, dtype=torch.int64, device=dev)
    _lib.call("consensus_pick", _p(pair), G, K, col, 1 if weights == "posterior" else 0, _p(scores), table.data_ptr() + 16 * G * K, T,
              _p(ids), 1 if ids.dtype == torch.int64 else 0, lt, _p(lengths), _p(pick), _p(expected), _p(out_ids), _p(row_pick),
              _p(out_scores), _p(out_len), _stream())
    return dict(pick=pick, expected=expected, ids=out_ids, row_pick=row_pick, scores=out_scores, lengths=out_len)


FORCE_MAX = 16                  # given captions per sentence (what ``consensus`` takes)
FORCE_UNK = ("bar", "skip")


def check_force(ids, lt=None, steps=None, unk="bar"):
    """Host checks of forced scoring: ``ids`` the stacked given captions, (T, K, Lt) or (T, Lt) int32 / int64 extended ids
    with 1 ≤ K ≤ 16; ``lt`` the model's Lt when the caller has one; ``steps`` the videos' sentence counts, which must add up to T;
    ``unk`` "bar" or "skip".  ValueError for each; ``SvpcKernelError`` for ids that are not on the GPU (no CPU fallback exists).
    → (T, K, Lt, skip flag)."""
    if unk not in FORCE_UNK:
        raise ValueError("unk must be one of %s, got %r" % (", ".join(FORCE_UNK), unk))
    if not torch.is_tensor(ids) or ids.dim() not in (2, 3) or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError("forced scoring takes int32 / int64 ids of shape (T, K, Lt) or (T, Lt), got %s"
                         % ((tuple(ids.shape), ids.dtype) if torch.is_tensor(ids) else type(ids).__name__,))
    T, K, n = (ids.shape[0], 1, ids.shape[1]) if ids.dim() == 2 else tuple(ids.shape)
    if not 1 <= K <= FORCE_MAX:
        raise ValueError("forced scoring takes 1..%d captions per sentence, got K = %d" % (FORCE_MAX, K))
    if n < 2:
        raise ValueError("captions need at least two positions (BOS and one word), got Lt = %d" % n)
    if lt is not None and n != int(lt):
        raise ValueError("captions of %d positions, the model's Lt is %d" % (n, lt))
    if steps is not None and (any(int(s) < 0 for s in steps) or sum(int(s) for s in steps) != T):
        raise ValueError("the videos' sentence counts %r do not add up to the %d caption rows given" % (list(steps), T))
    if not ids.is_cuda:
        raise _lib.SvpcKernelError("svpc_amd.ops: forced scoring runs on the GPU only (no CPU fallback exists)")
    return T, K, n, 1 if unk == "skip" else 0


def force_inputs(ids, vocab, unk_id, eos, pad, ignore=-1):
    """What the decoder and ``force_score`` need of given captions (svpc_force_inputs): ``ids`` (T, K, Lt) or (T, Lt) int32 / int64
    extended ids → (model_ids (R, Lt) int32 — an id outside the text vocabulary is ``unk_id``, ``pad`` after the caption's end —,
    mask (R, Lt) fp32 — 1 on positions 0 … len —, tgt (R, Lt) int32 target columns, len (R,) int32, finished (R,) int32), R = T·K."""
    if not 0 <= int(unk_id) < int(vocab):
        raise ValueError("force_inputs: the UNK id must lie inside the text vocabulary")
    T, K, lt, _ = check_force(ids)
    _need_gpu(ids)
    ids = _c(ids)
    R, dev = T * K, ids.device
    model_ids = torch.empty(R, lt, dtype=torch.int32, device=dev)
    mask = torch.empty(R, lt, dtype=torch.float32, device=dev)
    tgt = torch.empty(R, lt, dtype=torch.int32, device=dev)
    ln = torch.empty(R, dtype=torch.int32, device=dev)
    fin = torch.empty(R, dtype=torch.int32, device=dev)
    _lib.call("force_inputs", _p(ids), 1 if ids.dtype == torch.int64 else 0, R, lt, int(vocab), int(unk_id), int(eos), int(pad), int(ignore),
              _p(model_ids), _p(mask), _p(tgt), _p(ln), _p(fin), _stream())
    return model_ids, mask, tgt, ln, fin


def force_score(scores, row_c, tgt, length, logits, unk_id, unk="bar", max_cols=None):
    """The scores of given captions from the decoder's score matrix (svpc_force_score, svpc_force_finish: two launches):
    ``scores`` (≥ R·Lt, ≥ C) fp32 — row r·Lt + i is step i of caption row r; probabilities, or logits when ``logits`` —, ``row_c`` the R
    rows' column counts C_r (an Idx or host ints), ``tgt`` (R, Lt) / ``length`` (R,) int32 as ``force_inputs`` returns them,
    ``max_cols`` max(row_c) when the caller knows it → a dict: ``cum`` (R,) fp32, ``n_scored`` (R,) int32, and (R, Lt − 1) ``step`` fp32,
    ``rank`` int32, ``top`` int32, ``top_step`` fp32.  Reads the score matrix once (twice in logits mode); allocates the six results."""
    if unk not in FORCE_UNK:
        raise ValueError("unk must be one of %s, got %r" % (", ".join(FORCE_UNK), unk))
    if tgt.dim() != 2 or tgt.shape[1] < 2 or not _id_rows(tgt, tgt.shape[0], tgt.shape[1], scores.device):
        raise ValueError("force_score: tgt must be a contiguous int32 (R, Lt >= 2) matrix on the scores' device")
    R, lt = tgt.shape
    if scores.dim() != 2 or scores.shape[0] < R * lt or scores.stride(1) != 1 or scores.dtype != torch.float32:
        raise ValueError("force_score: scores must be fp32 (>= R·Lt, C) rows with unit column stride")
    if not _row_vec(length, R, torch.int32, scores.device):
        raise ValueError("force_score: length must be contiguous int32 (R,) on the scores' device")
    rc = as_idx(row_c)
    if len(rc.host) != R:
        raise ValueError("force_score: one column count per caption row (%d), got %d" % (R, len(rc.host)))
    max_c = int(max_cols) if max_cols is not None else (max(rc.host) if R else 1)
    if max_c > scores.shape[1] or (R and min(rc.host) < 1):
        raise ValueError("force_score: rows of 1..%d columns, inside the score matrix" % scores.shape[1])
    _need_gpu(scores)
    dev = scores.device
    skip = 1 if unk == "skip" else 0
    step = torch.empty(R, lt - 1, dtype=torch.float32, device=dev)
    top_step = torch.empty(R, lt - 1, dtype=torch.float32, device=dev)
    rank = torch.empty(R, lt - 1, dtype=torch.int32, device=dev)
    top = torch.empty(R, lt - 1, dtype=torch.int32, device=dev)
    cum = torch.empty(R, dtype=torch.float32, device=dev)
    n_scored = torch.empty(R, dtype=torch.int32, device=dev)
    rcd = rc.dev(dev)
    _lib.call("force_score", _p(scores), scores.stride(0), _p(rcd), max_c, _p(tgt), _p(length), R, lt, 1 if logits else 0, int(unk_id), skip,
              _p(step), _p(rank), _p(top), _p(top_step), _stream())
    _lib.call("force_finish", _p(tgt), _p(length), _p(rcd), R, lt, int(unk_id), skip, _p(step), _p(rank), _p(top), _p(top_step), _p(cum),
              _p(n_scored), _stream())
    return dict(cum=cum, n_scored=n_scored, step=step, rank=rank, top=top, top_step=top_step)


def ptr_attn_gate_groups(dec, proj, bank, step_ne, lt, group_rows, w, b):
    """Pointer attention and generation gate (``ptr_attn_gate``, inference) for ``len(group_rows)`` sentences' worth of rows per step row
    of the bank: ``dec`` (T·G·lt, D) holds G groups of ``lt`` rows per sentence, ``group_rows[g]`` = (row_off, row_len) int32 device
    tables naming group g's rows of every sentence.  One launch per group into shared results, so the bank and its projection are not
    replicated → (pi (T·G·lt, e_max), p_gen (T·G·lt, 1)).  ``SvpcKernelError`` for a shape the kernel does not take."""
    T, e_max, D = bank.shape
    G = len(group_rows)
    if (not dec.is_cuda or dec.dtype != torch.float32 or D % 4 or tuple(w.shape) != (1, 2 * D) or b is None or b.numel() != 1 or lt > 32
            or e_max > 32 or tuple(dec.shape) != (T * G * lt, D) or w.dtype != torch.float32 or (w.data_ptr() % 16) or lo_off(dec) is not None):
        raise _lib.SvpcKernelError("ptr_attn_gate_groups: fp32 rows of D %% 4 == 0 columns, at most 32 positions and 32 entities per sentence")
    _need_gpu(dec)
    dec, proj, bank, w = _c(dec), _c(proj), _c(bank), _c(w)
    dev = dec.device
    ne = as_idx(step_ne).dev(dev)
    pi = torch.empty(dec.shape[0], e_max, dtype=torch.float32, device=dev)
    g = torch.empty(dec.shape[0], 1, dtype=torch.float32, device=dev)
    for ro, rl in group_rows:
        _lib.call("ptr_attn_gate_fwd_r", _p(dec), _p(proj), _p(bank), _p(ne), _p(pi), _p(w), _p(b), _p(g), T, lt, e_max, D, _p(ro), _p(rl),
                  _stream())
    return pi, g


FORCE_ACC_COLS = 9              # captions, positions, Σ cum / Σ n_scored (finite captions), −inf captions, rank-0, Σ rank, ranked, finished


def force_accum(cum, n_scored, finished, length, rank, acc):
    """acc (9,) float64 += the sums ``metrics.ForcedScores`` keeps (svpc_force_accum, fixed order): ``cum`` fp32, ``n_scored`` /
    ``finished`` / ``length`` int32 of R caption rows (any shape of R elements) and ``rank`` (R, Lt − 1) int32, as ``force_score`` /
    ``Translator.score_captions`` return them."""
    R = cum.numel()
    if cum.dtype != torch.float32 or rank.dtype != torch.int32 or rank.dim() < 2 or rank.numel() != R * rank.shape[-1] or any(
            t.dtype != torch.int32 or t.numel() != R or t.device != cum.device for t in (n_scored, finished, length)) or rank.device != cum.device:
        raise ValueError("force_accum: cum fp32, n_scored / finished / length int32 of R rows and rank int32 (R, Lt - 1), on one device")
    _accumulator("force_accum", "acc", acc, torch.float64, FORCE_ACC_COLS, cum, "scores")
    _need_gpu(cum)
    cum, n_scored, finished, length, rank = (_c(t) for t in (cum, n_scored, finished, length, rank))
    _lib.call("force_accum", _p(cum), _p(n_scored), _p(finished), _p(length), _p(rank), R, rank.shape[-1] + 1, _p(acc), _stream())
    return acc
