"""The short-loop corners of the four kernels that share the 256×256 8-phase main loop (gemm_common.h: p8_main_loop) — what one loop can
get wrong for one policy and not for another: one, two and three k-tiles (prologue only; either LDS buffer ends the loop), the fewest
staged buffers the split kernel accepts, zero-sourced k-rows and every bias-gradient mask of the grouped wgrad.  C-ABI calls only, each
against fp64 of the same bf16 operands with the tolerance of the kernel's own test (tests/test_p8t_gpu.py, tests/test_x3_gpu.py);
outputs are pre-filled with 7.0 and carry guard rows.  gemm_p8's corners are in tests/test_ops_gpu.py::test_gemm_p8_forward_form."""
import ctypes
import math

import pytest
import torch

from svpc_amd import _lib
from svpc_amd.grad_tail import _WgradProblem
from svpc_amd.ops_common import ACT_GELU, ACT_NONE, ACT_RELU

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed * 1000 + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _gelu(z):
    return z * 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))


# ------------------------------------------------------------------------------------------------ p8t: C = (A·B) ⊙ act'(G) + R
def _p8t_case(M, N, K, gact):
    A = _rand(M, K, seed=1).to(BF)
    W = _rand(K, N, seed=2, scale=1.0 / math.sqrt(K)).to(BF)
    G = _rand(M, N, seed=3).to(BF) if gact != ACT_NONE else None
    R = _rand(M, N, seed=4).to(BF) if gact != ACT_NONE else None
    ref = A.double() @ W.double()
    if gact == ACT_GELU:
        ref = ref * _gelu_grad(G.double())
    elif gact == ACT_RELU:
        ref = ref * (G.double() > 0).double()
    if R is not None:
        ref = ref + R.double()
    return A, W, G, R, ref


def _p8t_check(C, ref, M):
    err = float((C[:M].double() - ref).abs().max())
    assert err <= 6e-3 * float(ref.abs().max()), (err, float(ref.abs().max()))
    assert bool((C[M:] == 7.0).all())


@pytest.mark.parametrize("M,N,K,gact", [(300, 264, 128, ACT_GELU), (260, 520, 192, ACT_RELU), (130, 264, 64, ACT_NONE)])
def test_p8t_one_to_three_k_tiles(M, N, K, gact):
    """2, 3 and 1 k-tiles; a second column tile with 8 valid columns, a ragged row tile; GELU' + R, ReLU' + R, neither"""
    A, W, G, R, ref = _p8t_case(M, N, K, gact)
    C = torch.full((M + 3, N), 7.0, dtype=BF, device=DEV)
    _lib.call("gemm_p8t", A.data_ptr(), K, W.data_ptr(), N, C.data_ptr(), N, G.data_ptr() if G is not None else None, gact,
              R.data_ptr() if R is not None else None, M, N, K, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _p8t_check(C, ref, M)


# ------------------------------------------------------------------------------------------------ p8x3 / s4x3: split in, split out
def _split_rows(t):
    """fp32 (R, W) → bf16 (R, 2W): hi plane at columns [0, W), lo plane at [W, 2W); and the value the pair represents"""
    hi = t.to(BF)
    lo = (t - hi.float()).to(BF)
    return torch.cat([hi, lo], dim=1).contiguous(), hi.float() + lo.float()


def _x3_case(M, N, K, act):
    x, xv = _split_rows(_rand(M, K, seed=30))
    w = _rand(N, K, seed=31, scale=1.0 / math.sqrt(K))
    w_hi = w.to(BF)
    w_lo = (w - w_hi.float()).to(BF)
    w2 = torch.stack([w_hi, w_lo]).contiguous()           # two planes of identical layout N·K elements apart
    b = _rand(N, seed=32, scale=0.1)
    z64 = xv.double() @ (w_hi.double() + w_lo.double()).t() + b.double()
    ref = _gelu(z64) if act == ACT_GELU else z64
    return x, w2, b, z64, ref


def _x3_check(buf, zbuf, z64, ref, M, N):
    got = buf[:M, :N].double() + buf[:M, N + 8:2 * N + 8].double()
    err = float((got - ref).abs().max())
    assert err <= 3e-5 * float(ref.abs().max()), (err, float(ref.abs().max()))
    assert bool((buf[M:] == 7.0).all()) and bool((buf[:M, N:N + 8] == 7.0).all()) and bool((buf[:M, 2 * N + 8:] == 7.0).all())
    if zbuf is not None:
        errz = float((zbuf[:M, :N].double() - z64).abs().max())
        assert errz <= 6e-3 * float(z64.abs().max()), (errz, float(z64.abs().max()))
        assert bool((zbuf[M:] == 7.0).all()) and bool((zbuf[:M, N:] == 7.0).all())


@pytest.mark.parametrize("kernel", ["gemm_p8x3", "gemm_s4x3"])
@pytest.mark.parametrize("K,act", [(64, ACT_NONE), (96, ACT_GELU), (160, ACT_GELU)])
def test_split_gemm_two_three_five_buffers(kernel, K, act):
    """2 (the least the kernels accept: the prologue stages buffer 1 unasked), 3 and 5 staged 32-deep buffers; GELU with the plain-bf16
    pre-activation copy, or no activation; rows and columns past the edges are not written"""
    M, N = 300, 264
    x, w2, b, z64, ref = _x3_case(M, N, K, act)
    buf = torch.full((M + 3, 2 * N + 16), 7.0, dtype=BF, device=DEV)      # guard rows / columns around the output
    zbuf = torch.full((M + 3, N + 8), 7.0, dtype=BF, device=DEV) if act != ACT_NONE else None
    _lib.call(kernel, x.data_ptr(), x.stride(0), K, w2.data_ptr(), K, N * K, buf.data_ptr(), buf.stride(0), N + 8,
              zbuf.data_ptr() if zbuf is not None else None, zbuf.stride(0) if zbuf is not None else 0, M, N, K, b.data_ptr(), act,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _x3_check(buf, zbuf, z64, ref, M, N)


# ------------------------------------------------------------------------------------------------ p8w: dW += dzᵀ·x, db += Σ_rows dz
P8W_TABLE = [(40, 264, 256), (64, 256, 520), (100, 264, 264), (192, 520, 256)]      # (rows, n_out, n_in)


def _p8w_case(i, rows, n_out, n_in):
    dz = _rand(rows, n_out, seed=20 + i).to(BF)
    x = _rand(rows, n_in, seed=40 + i).to(BF)
    dw = torch.full((n_out + 2, n_in), 7.0, dtype=torch.float32, device=DEV)      # two guard rows
    dw[:n_out] += _rand(n_out, n_in, seed=60 + i, scale=0.5)
    db = torch.full((n_out + 2,), 7.0, dtype=torch.float32, device=DEV)
    db[:n_out] += _rand(n_out, seed=80 + i, scale=2.0)
    ref_w = dw[:n_out].double() + dz.double().t() @ x.double()
    ref_b = db[:n_out].double() + dz.double().sum(0)
    return dz, x, dw, db, ref_w, ref_b


def _p8w_check(i, rows, n_out, dw, db, ref_w, ref_b):
    grow = math.sqrt(rows / 1000.0)
    err = float((dw[:n_out].double() - ref_w).abs().max())
    assert err <= 2e-5 * float(ref_w.abs().max()) * grow + 1e-4, ("dw", i, err)
    errb = float((db[:n_out].double() - ref_b).abs().max())
    assert errb <= 2e-5 * float(ref_b.abs().max()) * grow + 1e-4, ("db", i, errb)
    assert bool((dw[n_out:] == 7.0).all()) and bool((db[n_out:] == 7.0).all())


def test_grouped_wgrad_p8_short_reductions():
    """one table, no workspace (every tile runs whole): a single k-tile with zero-sourced k-rows, an exact k-tile, a ragged second
    k-tile, three k-tiles; bias masks 3 (one tile column), 1 / 2 and 0 (a third tile column); accumulation into non-zero dW and db"""
    cases = [_p8w_case(i, *spec) for i, spec in enumerate(P8W_TABLE)]
    probs = (_WgradProblem * len(cases))()
    for i, ((rows, n_out, n_in), (dz, x, dw, db, _, _)) in enumerate(zip(P8W_TABLE, cases)):
        probs[i] = _WgradProblem(dz.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr(), n_out, n_in, rows, dz.stride(0), x.stride(0),
                                 dw.stride(0))
    assert _lib.load().svpc_gemm_group_wgrad_bf16_p8_ok(ctypes.addressof(probs), len(cases)) == 1
    _lib.call("gemm_group_wgrad_bf16_p8", ctypes.addressof(probs), len(cases), None, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for i, ((rows, n_out, _), (_, _, dw, db, ref_w, ref_b)) in enumerate(zip(P8W_TABLE, cases)):
        _p8w_check(i, rows, n_out, dw, db, ref_w, ref_b)
