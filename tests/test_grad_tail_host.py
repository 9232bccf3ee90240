"""The queue logic of the gradient tail (svpc_amd/grad_tail.py) without a GPU: the kernel library is replaced by a recorder that decodes
the ctypes tables a launch points to at the moment of the call, its limit getters by small fixed numbers, the stream getter by 0.  CPU
tensors stand in for device tensors — only their address, shape and stride are read.  The expected sequences are those of the code as it
stood in ops.py before the tail got a module of its own."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from svpc_amd import _lib, grad_tail as gt, ops

WGRAD_MAX, FINALIZE_MAX = 4, 6
TABLES = {"gemm_group_wgrad": gt._WgradProblem, "gemm_group_wgrad_bf16_p8": gt._WgradProblem, "gemm_group_wgrad_bf16_ws": gt._WgradProblem,
          "multi_colsum": gt._ColsumEntry, "multi_finalize": gt._FinalizeEntry}


class StubLib:
    def __init__(self):
        self.p8_ok, self.finalize_max = 1, FINALIZE_MAX

    def svpc_gemm_group_wgrad_max(self):
        return WGRAD_MAX

    def svpc_multi_finalize_max(self):
        return self.finalize_max

    def svpc_colsum_chunks(self, rows):
        return -(-rows // 8)

    def svpc_gemm_group_wgrad_bf16_p8_ok(self, table, n):
        return self.p8_ok


class Tail:
    """what a test sees: ``calls`` (name, decoded table rows or raw arguments, trailing arguments), ``ready`` (hook reports), ``lib``"""

    def __init__(self):
        self.calls, self.ready, self.lib = [], [], StubLib()

    def call(self, name, *args):
        if name in TABLES:
            rows = (TABLES[name] * args[1]).from_address(args[0])
            self.calls.append((name, [tuple(getattr(r, f) for f, _ in r._fields_) for r in rows], args[2:]))
        else:
            self.calls.append((name, None, args))
        return 0

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture
def tail(monkeypatch):
    t = Tail()
    monkeypatch.setattr(_lib, "call", t.call)
    monkeypatch.setattr(_lib, "load", lambda: t.lib)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_WS_BYTES", 4096)
    monkeypatch.setattr(ops, "_WS", {})
    monkeypatch.setattr(gt, "GRAD_READY_HOOK", lambda ptr, numel, kind: t.ready.append((ptr, numel, kind)))
    queues = (gt._WQ16, gt._WQ, gt._CQ, gt._FQ)
    assert not any(queues) and not ops._RES_SINK
    ops.set_precision("bf16")
    try:
        yield t
    finally:
        ops.set_precision("fp32")
        for q in queues:
            del q[:]
        ops._RES_SINK.clear()
        gt._JOIN_QUEUED[0] = False


def f32(*shape):
    return torch.zeros(*shape, dtype=torch.float32)


def b16(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16)


def problem(mk, rows=8, n_out=16, n_in=24, bias=True):
    return mk(rows, n_out), mk(rows, n_in), f32(n_out, n_in), (f32(n_out) if bias else None)


def row(dz, x, wg, bg, null_bias=False):
    """the _WgradProblem a queued problem becomes"""
    return (dz.data_ptr(), x.data_ptr(), wg.data_ptr(), None if (bg is None or null_bias) else bg.data_ptr(), dz.shape[1], x.shape[1],
            dz.shape[0], dz.stride(0), x.stride(0), wg.stride(0))


def reports(probs, bias=True):
    out = []
    for _, _, wg, bg in probs:
        out.append((wg.data_ptr(), wg.numel(), "w"))
        if bg is not None and bias:
            out.append((bg.data_ptr(), bg.numel(), "b"))
    return out


# ------------------------------------------------------------------------------------------------ fp32 wgrad queue
def test_fp32_wgrads_flush_at_capacity_in_queue_order(tail):
    assert min(gt.GROUP_FLUSH_AT, WGRAD_MAX) == WGRAD_MAX
    probs = [problem(f32, rows=3 + i, bias=i % 2 == 0) for i in range(WGRAD_MAX + 1)]
    for p in probs[:WGRAD_MAX - 1]:
        assert gt.defer_wgrad(*p) is True
    assert tail.calls == [] and tail.ready == []
    assert gt.defer_wgrad(*probs[WGRAD_MAX - 1]) is True
    assert tail.calls == [("gemm_group_wgrad", [row(*p) for p in probs[:WGRAD_MAX]], (0,))]
    assert tail.ready == reports(probs[:WGRAD_MAX])
    assert gt.defer_wgrad(*probs[WGRAD_MAX]) is True
    assert len(tail.calls) == 1 and len(gt._WQ) == 1


def test_fp32_wgrad_for_a_pending_target_flushes_first(tail):
    dz0, x0, wg, bg = problem(f32)
    dz1, x1, _, _ = problem(f32, rows=5)
    assert gt.defer_wgrad(dz0, x0, wg, bg) and gt.defer_wgrad(dz1, x1, wg, None)
    assert tail.calls == [("gemm_group_wgrad", [row(dz0, x0, wg, bg)], (0,))]
    gt.flush_pending()
    assert tail.calls[1:] == [("gemm_group_wgrad", [row(dz1, x1, wg, None)], (0,))]
    assert tail.ready == reports([(dz0, x0, wg, bg), (dz1, x1, wg, None)])


def test_fp32_wgrad_that_fails_the_layout_or_tile_test_is_refused(tail, monkeypatch):
    dz, x, wg, bg = problem(f32)
    assert gt.defer_wgrad(*problem(f32, n_out=6)) is False              # n_out % 4
    assert gt.defer_wgrad(*problem(f32, n_in=10)) is False              # n_in % 4
    assert gt.defer_wgrad(dz[:0], x[:0], wg, bg) is False               # no rows
    assert gt.defer_wgrad(dz.view(-1)[1:1 + 7 * 16].view(7, 16), x[:7], wg, bg) is False      # dz not 16-byte aligned
    assert gt.defer_wgrad(dz, x, f32(24, 16).t(), bg) is False          # gradient not contiguous
    assert gt.defer_wgrad(dz, x, None, bg) is False
    monkeypatch.setattr(gt, "GROUP_MAX_TILES", 1)
    assert gt.defer_wgrad(*problem(f32, n_out=128, n_in=64)) is False   # 2 tiles of 64² > GROUP_MAX_TILES
    assert gt.defer_wgrad(*problem(f32, n_out=64, n_in=64)) is True
    del gt._WQ[:]
    monkeypatch.setattr(ops, "BWD_EXACT", True)                         # the ablation switch, read at call time
    assert gt.defer_wgrad(dz, x, wg, bg) is False
    monkeypatch.setattr(ops, "BWD_EXACT", False)
    ops.set_precision("fp32")
    assert gt.defer_wgrad(dz, x, wg, bg) is False
    gt.flush_pending()
    assert tail.calls == [] and tail.ready == [] and not gt._WQ and not gt._WQ16


# ------------------------------------------------------------------------------------------------ bf16 wgrad queue
def test_bf16_wgrads_flush_when_full_and_carry_their_biases_on_the_p8_kernel(tail):
    probs = [problem(b16, rows=8 * (i + 1), bias=i != 1) for i in range(WGRAD_MAX + 1)]
    for p in probs[:WGRAD_MAX]:
        assert gt.defer_wgrad(*p) is True
    assert tail.calls == []                                             # full, but only the next arrival flushes
    assert gt.defer_wgrad(*probs[WGRAD_MAX]) is True
    ws = ops._ws(torch.device("cpu"))
    assert tail.calls == [("gemm_group_wgrad_bf16_p8", [row(*p) for p in probs[:WGRAD_MAX]], (ws.data_ptr(), ws.numel() * 4, 0))]
    assert tail.ready == reports(probs[:WGRAD_MAX])
    assert len(gt._WQ16) == 1 and not gt._CQ and not gt._FQ


def test_bf16_wgrads_without_the_p8_kernel_send_their_biases_to_the_column_sums(tail):
    tail.lib.p8_ok = 0
    probs = [problem(b16), problem(b16, rows=16, bias=False), problem(b16, rows=24)]
    for p in probs:
        assert gt.defer_wgrad(*p) is True
    gt.flush_wgrads()
    ws = ops._ws(torch.device("cpu"))
    assert tail.calls == [("gemm_group_wgrad_bf16_ws", [row(*p, null_bias=True) for p in probs], (ws.data_ptr(), ws.numel() * 4, 0))]
    assert tail.ready == reports(probs, bias=False)
    assert [(x.data_ptr(), o.data_ptr()) for (x, _), (_, o, _, _, _, _) in zip(gt._CQ, gt._FQ)] == \
        [(p[0].data_ptr(), p[3].data_ptr()) for p in probs if p[3] is not None]
    gt.flush_pending()
    assert tail.names() == ["gemm_group_wgrad_bf16_ws", "multi_colsum", "multi_finalize"]
    assert tail.ready[len(probs):] == [(p[3].data_ptr(), p[3].numel(), "b") for p in probs if p[3] is not None]


@pytest.mark.parametrize("same", ["wgrad", "bgrad"])
def test_bf16_wgrad_for_a_pending_target_flushes_first(tail, same):
    a, b = problem(b16), problem(b16, rows=16)
    b = (b[0], b[1], a[2], b[3]) if same == "wgrad" else (b[0], b[1], b[2], a[3])
    assert gt.defer_wgrad(*a) and gt.defer_wgrad(*b)
    assert [(n, t) for n, t, _ in tail.calls] == [("gemm_group_wgrad_bf16_p8", [row(*a)])]
    gt.flush_pending()
    assert [(n, t) for n, t, _ in tail.calls[1:]] == [("gemm_group_wgrad_bf16_p8", [row(*b)])]
    assert tail.ready == reports([a, b])


def test_bf16_wgrad_that_fails_the_layout_test_is_refused(tail):
    dz, x, wg, bg = problem(b16)
    assert gt.defer_wgrad(*problem(b16, n_out=12)) is False             # n_out % 8
    assert gt.defer_wgrad(dz[:0], x[:0], wg, bg) is False
    assert gt.defer_wgrad(dz, x, f32(24, 16).t(), bg) is False
    assert tail.calls == [] and not gt._WQ16


# ------------------------------------------------------------------------------------------------ column sums and finalizers
def test_defer_colsum_queues_both_stages_and_flushes_at_48_pending(tail):
    tail.lib.finalize_max = 1000
    xs = [b16(20, 8) if i % 2 else f32(20, 8) for i in range(49)]
    outs = [f32(8) for _ in xs]
    gt.defer_colsum(xs[0], outs[0])
    (x, partial), = gt._CQ
    assert x is xs[0] and partial.numel() == 3 * 8 and partial.dtype == torch.float32          # chunks(20) = 3 in the stub
    assert [(q[0] is partial, q[1] is outs[0], q[2]) + q[3:] for q in gt._FQ] == [(True, True, None, 3, 8, 8)]
    for x, o in zip(xs[1:48], outs[1:48]):
        gt.defer_colsum(x, o)
    assert tail.calls == [] and len(gt._CQ) == 48
    partials = [p.data_ptr() for _, p in gt._CQ]
    gt.defer_colsum(xs[48], outs[48])
    assert tail.names() == ["multi_colsum", "multi_finalize"]
    assert tail.calls[0][1] == [(x.data_ptr(), p, 1 if x.dtype == torch.bfloat16 else 0, 8, 20, 8) for x, p in zip(xs[:48], partials)]
    assert tail.calls[1][1] == [(p, o.data_ptr(), o.data_ptr(), 3, 8, 8) for p, o in zip(partials, outs[:48])]
    assert tail.calls[0][2] == tail.calls[1][2] == (0,)
    assert tail.ready == [(o.data_ptr(), 8, "b") for o in outs[:48]]
    assert len(gt._CQ) == len(gt._FQ) == 1


def test_finalizers_flush_at_capacity_for_a_pending_target_and_pass_one_target_twice(tail):
    parts = [f32(4, 10) for _ in range(FINALIZE_MAX + 2)]
    g, b, v = f32(6), f32(4), f32(10)
    gt.defer_finalize(parts[0], 4, 10, g, b, 6)
    gt.defer_finalize(parts[1], 4, 10, v)                               # out1=None: out0 twice, split = ncols
    assert tail.calls == []
    gt.defer_finalize(parts[2], 4, 10, f32(6), b, 6)                    # b is pending: flush first
    assert tail.calls == [("multi_finalize", [(parts[0].data_ptr(), g.data_ptr(), b.data_ptr(), 4, 10, 6),
                                              (parts[1].data_ptr(), v.data_ptr(), v.data_ptr(), 4, 10, 10)], (0,))]
    assert tail.ready == [(g.data_ptr(), 6, None), (b.data_ptr(), 4, None), (v.data_ptr(), 10, "b")]
    for p in parts[3:3 + FINALIZE_MAX - 2]:
        gt.defer_finalize(p, 4, 10, f32(10))
    assert len(tail.calls) == 1 and len(gt._FQ) == FINALIZE_MAX - 1
    gt.defer_finalize(parts[-1], 4, 10, f32(10))
    assert tail.names() == ["multi_finalize", "multi_finalize"] and len(tail.calls[1][1]) == FINALIZE_MAX and not gt._FQ


def test_flush_pending_order_and_idempotence(tail):
    w16, w32 = problem(b16, bias=False), problem(f32, bias=False)
    gt.defer_finalize(f32(2, 10), 2, 10, f32(6), f32(4), 6)
    gt.defer_colsum(f32(9, 8), f32(8))
    assert gt.defer_wgrad(*w32) and gt.defer_wgrad(*w16)
    assert tail.calls == []
    gt.flush_pending()
    assert tail.names() == ["gemm_group_wgrad_bf16_p8", "gemm_group_wgrad", "multi_colsum", "multi_finalize"]
    assert [len(c[1]) for c in tail.calls] == [1, 1, 1, 2]
    gt.flush_pending()
    assert len(tail.calls) == 4


# ------------------------------------------------------------------------------------------------ routing helpers
def test_bias_grad_defers_an_aligned_row_and_launches_any_other_now(tail):
    ok, tgt = f32(5, 8), f32(8)
    gt.bias_grad(ok, tgt)
    assert tail.calls == [] and tail.ready == [] and len(gt._CQ) == 1
    del gt._CQ[:], gt._FQ[:]
    odd, tgt6 = f32(5, 6), f32(6)                                       # N % 4: the accumulating column sum, now
    gt.bias_grad(odd, tgt6)
    ws = ops._ws(torch.device("cpu"))
    assert tail.calls == [("bucket_colsum_t", None, (odd.data_ptr(), 0, 6, None, 5, 6, 1, tgt6.data_ptr(), 1, ws.data_ptr(), 0))]
    assert tail.ready == [(tgt6.data_ptr(), 6, "b")]
    for dz in (b16(5, 12), f32(5, 10)[:, :8], f32(6, 8).view(-1)[1:41].view(5, 8)):      # N % 8 in bf16, row stride, address
        gt.bias_grad(dz, tgt)
    assert tail.names() == ["bucket_colsum_t"] * 4 and not gt._CQ
    gt.bias_grad(f32(0, 8), tgt)                                        # no rows: nothing to add, still reported
    assert len(tail.calls) == 4 and tail.ready[-1] == (tgt.data_ptr(), 8, "b") and not gt._CQ


def test_defer_partials_needs_both_arena_targets(tail):
    part, g, b = f32(3, 12), f32(6), f32(6)
    assert gt.defer_partials(part, 3, 12, g, None, 6) is False and gt.defer_partials(part, 3, 12, None, b, 6) is False
    assert not gt._FQ
    assert gt.defer_partials(part, 3, 12, g, b, 6) is True
    assert [(q[0] is part, q[1] is g, q[2] is b) + q[3:] for q in gt._FQ] == [(True, True, True, 3, 12, 6)]


# ------------------------------------------------------------------------------------------------ notifications, join, retired names
def test_no_report_while_hooks_are_paused(tail):
    assert ops.hooks_paused is gt.hooks_paused and ops.HOOKS_PAUSED is gt.HOOKS_PAUSED
    with ops.hooks_paused():
        assert gt.defer_wgrad(*problem(f32)) and gt.defer_wgrad(*problem(b16))
        gt.defer_colsum(f32(9, 8), f32(8))
        gt.flush_pending()
    assert len(tail.calls) == 4 and tail.ready == [] and gt.HOOKS_PAUSED[0] == 0


def test_join_side_flushes_clears_the_flag_and_fails_on_a_parked_gradient(tail):
    assert ops.join_side is gt.join_side and ops.flush_pending is gt.flush_pending
    assert gt.defer_wgrad(*problem(f32))
    assert gt._JOIN_QUEUED[0] is False                                  # (not inside a backward pass: nothing to hang the callback on)
    gt._JOIN_QUEUED[0] = True
    ops.join_side()
    assert tail.names() == ["gemm_group_wgrad"] and gt._JOIN_QUEUED[0] is False
    ops._RES_SINK[1234] = f32(2, 2)
    ops._RES_SINK[5678] = f32(2, 2)
    gt._JOIN_QUEUED[0] = True
    with pytest.raises(_lib.SvpcKernelError, match="2 parked gradient"):
        ops.join_side()
    assert not ops._RES_SINK and gt._JOIN_QUEUED[0] is False
    ops.join_side()


def test_the_stream_experiments_are_gone():
    retired = ("SIDE_WGRAD", "branch_stream", "BRANCH_STREAMS", "_side_of", "_SIDE", "_N_SIDE", "_SIDE_DIRTY", "_BRANCH",
               "USE_MULTI_FINALIZE", "GROUP_COLSUM")
    assert not [n for n in retired if hasattr(ops, n) or hasattr(gt, n)]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SVPC_SIDE="1", SVPC_N_SIDE="3", SVPC_BRANCH="1", SVPC_NO_MULTI_FINALIZE="1", SVPC_NO_GROUP_COLSUM="1")
    out = subprocess.run([sys.executable, "-c", "import json, svpc_amd.ops as o, svpc_amd.grad_tail as g; "
                          "print(json.dumps([sorted(dir(o)), sorted(dir(g))]))"], cwd=root, env=env, capture_output=True, text=True, check=True)
    there_ops, there_tail = json.loads(out.stdout.strip().splitlines()[-1])
    assert not [n for n in retired if n in there_ops or n in there_tail]
    assert there_ops == sorted(dir(ops)) and there_tail == sorted(dir(gt))
