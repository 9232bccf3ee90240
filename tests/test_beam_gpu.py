"""Beam-search decoding on the MI355X: the selection kernel (svpc_beam_step) against tests/beam_reference.py::select, the indexed
decoding-step attention (svpc_attn_q1_ln_idx_fwd) against gather-then-torch, and Translator.translate_batch(use_beam=True) against greedy
(B = 1) and the CPU beam reference (B = 2, 4), eager and replayed, up to config 5 at its headline size."""
import copy
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import beam_reference as br  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import ops, synthetic as syn  # noqa: E402
from svpc_amd.ops_common import Idx  # noqa: E402
from svpc_amd.synthetic import EOS, PAD, UNK  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [("tiny", "v"), ("tiny", "vi"), ("tiny", "viv"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")]
O = type("O", (), {"cuda": True})


# ------------------------------------------------------------------------------------------------ 1. the selection kernel
def _tables(rng, T, B, logits, adversarial):
    """scores / row_c / row_x / cum / finished for T sentences × B hypotheses: ragged C per sentence, OOV columns, finished
    hypotheses, and (adversarial) exact ties everywhere: few distinct values, equal cums, zero probabilities, a dead beam."""
    Cs = rng.integers(16, 700, size=T)
    Xs = np.array([rng.integers(0, min(4, c - UNK - 1)) for c in Cs])
    cmax = int(Cs.max())
    R = T * B
    if adversarial:
        vals = np.array([0.0, 0.125, 0.25, 0.5] if not logits else [-3.0, -1.0, 0.0, 2.0], np.float32)
        s = vals[rng.integers(0, len(vals), size=(R, cmax))]
        cum = np.array([-1.0, -0.5, -np.inf, 0.0], np.float32)[rng.integers(0, 4, size=R)]
        cum[::B] = -0.5
    else:
        s = (rng.random((R, cmax)) ** 4).astype(np.float32) if not logits else rng.standard_normal((R, cmax)).astype(np.float32) * 3
        cum = (-rng.random(R) * 5).astype(np.float32)
    s[:, UNK] = 1.0 if not logits else 50.0            # UNK would win every comparison were it a candidate
    fin = (rng.random(R) < 0.3).astype(np.int32)
    row_c = np.repeat(Cs, B)
    row_x = np.repeat(Xs, B)
    return s, row_c, row_x, cum, fin


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("B", [1, 2, 3, 4, 8])
def test_beam_step_kernel_equals_select(B, logits):
    rng = np.random.default_rng(10 * B + logits)
    for adversarial in (False, True):
        T, Lt, pos = 37, 9, 5
        s, row_c, row_x, cum, fin = _tables(rng, T, B, logits, adversarial)
        R = T * B
        sd = torch.from_numpy(s).to(DEV)
        cum_d = torch.from_numpy(cum).to(DEV)
        fin_d = torch.from_numpy(fin).to(DEV)
        t_in = [torch.from_numpy(rng.integers(0, 1000, size=(R, Lt)).astype(np.int32)).to(DEV) for _ in range(3)]
        t_out = [torch.full((R, Lt), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
        par, nx_ext, nx_mod = ops.beam_step(sd, Idx(row_c.tolist()), Idx(row_x.tolist()), B, pos, logits, UNK, EOS, PAD, cum_d, fin_d,
                                            t_in, t_out, Lt)
        torch.cuda.synchronize()
        r_par, r_ext, r_mod, r_cum, r_fin = br.select(s, row_c, row_x, B, logits, cum, fin.astype(bool))
        np.testing.assert_array_equal(par.cpu().numpy(), r_par)
        np.testing.assert_array_equal(nx_ext.cpu().numpy(), r_ext)
        np.testing.assert_array_equal(nx_mod.cpu().numpy(), r_mod)
        np.testing.assert_array_equal(cum_d.cpu().numpy().view(np.int32), r_cum.view(np.int32))      # bit for bit (−inf included)
        np.testing.assert_array_equal(fin_d.cpu().numpy().astype(bool), r_fin)
        tin = [t.cpu().numpy() for t in t_in]
        tout = [t.cpu().numpy() for t in t_out]
        for k in range(3):
            np.testing.assert_array_equal(tout[k][:, :pos + 1], tin[k][r_par, :pos + 1])
            assert np.all(tout[k][:, pos + 2:] == -7)            # nothing past the child's new position is touched
        np.testing.assert_array_equal(tout[0][:, pos + 1], r_mod)
        np.testing.assert_array_equal(tout[1][:, pos + 1], r_ext)
        np.testing.assert_array_equal(tout[2][:, pos + 1], np.arange(R) * Lt + pos + 1)


def test_beam_finalize_picks_the_best_hypothesis():
    T, B, Lt = 50, 4, 7
    cum = torch.randn(T * B, device=DEV)
    cum[4:8] = 0.5                                   # a tie: the lowest beam index
    ext = torch.randint(0, 100, (T * B, Lt), dtype=torch.int32, device=DEV)
    ids, score = ops.beam_finalize(cum, ext, B)
    c = cum.view(T, B).cpu()
    best = torch.tensor([int(np.argmax(c[t].numpy())) for t in range(T)])
    assert int(best[1]) == 0
    assert torch.equal(ids.cpu(), ext.cpu().view(T, B, Lt)[torch.arange(T), best])
    assert torch.equal(score.cpu(), c[torch.arange(T), best])


# ------------------------------------------------------------------------------------------------ 2. the indexed attention step
def _ln_ref(q, K, V, x, g, b, eps, H):
    T, D = q.shape
    dh = D // H
    qh = q.double().view(T, H, 1, dh)
    Kh = K.double().view(T, -1, H, dh).transpose(1, 2)
    Vh = V.double().view(T, -1, H, dh).transpose(1, 2)
    p = torch.softmax(qh @ Kh.transpose(-1, -2) / math.sqrt(dh), -1)
    y = (p @ Vh).reshape(T, D) + x.double()
    u = y.mean(-1, keepdim=True)
    s = ((y - u) ** 2).mean(-1, keepdim=True)
    return (y - u) / torch.sqrt(s + eps) * g.double() + b.double()


@pytest.mark.parametrize("n_keys", list(range(1, 23)))
def test_indexed_self_attention_step(n_keys):
    """query t (T = 13 sentences × 4 hypotheses) attends to the cache rows its ancestry table names, its own row appended to its slot"""
    torch.manual_seed(n_keys)
    D, H, B, Lt, Ts = 768, 12, 4, 22, 13
    T = Ts * B
    pos = n_keys - 1
    g = torch.Generator().manual_seed(n_keys)
    cache = torch.randn(T * Lt, 2 * D, device=DEV)
    qkv = torch.randn(T, 3 * D, device=DEV)
    x = torch.randn(T, D, device=DEV)
    gam, bet = torch.rand(D, device=DEV) + 0.5, torch.randn(D, device=DEV)
    # ancestry: position j of hypothesis t lives in the slot of some hypothesis of the same sentence, row j; own slot at pos
    anc = torch.empty(T, Lt, dtype=torch.int32)
    for t in range(T):
        s = t // B
        for j in range(pos):
            anc[t, j] = (s * B + int(torch.randint(0, B, (1,), generator=g))) * Lt + j
        anc[t, pos] = t * Lt + pos
    anc = anc.to(DEV)
    before = cache.clone()
    out = ops.attn_q1_ln(qkv, cache, Lt, n_keys, x, gam, bet, 1e-12, H, new_kv=qkv[:, D:], key_rows=anc)
    assert out is not None
    torch.cuda.synchronize()
    own = (torch.arange(T, device=DEV) * Lt + pos).long()
    expect = before.clone()
    expect[own] = qkv[:, D:]
    assert torch.equal(cache, expect)                            # exactly the own rows are written
    kv = expect[anc[:, :n_keys].long().reshape(-1)].view(T, n_keys, 2 * D)
    ref = _ln_ref(qkv[:, :D], kv[:, :, :D], kv[:, :, D:], x, gam, bet, 1e-12, H)
    torch.testing.assert_close(out.double(), ref, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("n_mem", [1, 2, 3])
def test_indexed_cross_attention_step(n_mem):
    """queries t read the memory rows of sentence t // B (q_group = B)"""
    torch.manual_seed(n_mem)
    D, H, B, Ts = 768, 12, 3, 17
    T = Ts * B
    mem = torch.randn(Ts * n_mem, 2 * D, device=DEV)
    q = torch.randn(T, D, device=DEV)
    x = torch.randn(T, D, device=DEV)
    gam, bet = torch.rand(D, device=DEV) + 0.5, torch.randn(D, device=DEV)
    out = ops.attn_q1_ln(q, mem, n_mem, n_mem, x, gam, bet, 1e-12, H, q_group=B)
    assert out is not None
    kv = mem.view(Ts, n_mem, 2 * D).repeat_interleave(B, 0)
    ref = _ln_ref(q, kv[:, :, :D], kv[:, :, D:], x, gam, bet, 1e-12, H)
    torch.testing.assert_close(out.double(), ref, rtol=2e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------------ 3-5. the translator
def _ref_beam(cfg, model, batch, B):
    P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    cpu = {k: ([t.cpu() for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor) else
               (v.cpu() if isinstance(v, torch.Tensor) else v)) for k, v in batch.items()}
    return br.beam_decode(P, cfg, cpu["input_ids_list"], cpu["video_features_list"], cpu["input_masks_list"], cpu["ingr_input_ids"],
                          cpu["ingr_sep_masks"], cpu["batch_step_num"], cpu["ingr_id_dict"], cpu["oov_word_dict"], beam=B)


def _compare(dec, scores, ref, tie=1e-4):
    """ids exactly and scores within 1e-4 relative — except for sentences where the reference itself shows a near-tie (the margin
    between its last kept and first dropped candidate ≤ ``tie`` at some step), which are counted and returned."""
    r_ids, r_sc, r_mg = ref
    near = 0
    for d, s, ri, rs, rm in zip(dec, scores, r_ids, r_sc, r_mg):
        d, s = d.cpu(), s.cpu().numpy()
        for j in range(ri.shape[0]):
            if torch.equal(d[j], ri[j]):
                np.testing.assert_allclose(s[j], rs[j], rtol=1e-4, atol=1e-6)
                continue
            assert rm[j].size and float(rm[j].min()) <= tie, ("ids differ without a near-tie", d[j].tolist(), ri[j].tolist(),
                                                              float(rm[j].min()) if rm[j].size else None)
            near += 1
    return near


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("case,mt", CASES)
def test_width_one_is_greedy(golden_dir, case, mt, graph):
    from svpc_amd.translator import Translator
    z, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    opt = O()
    opt.beam_size = 1
    tr = Translator(opt, {"model_cfg": cfg, "model": model.state_dict()}, model=model, graph=graph)
    for _ in range(2 if graph else 1):                 # (graph: the second call replays)
        dec, _ = tr.translate_batch(syn.translate_inputs(batch), use_beam=True)
        for b, d in enumerate(dec):
            assert d.dtype == torch.int64
            np.testing.assert_array_equal(d.cpu().numpy(), br.greedy_equivalent(torch.from_numpy(z["decode/%d" % b])).numpy())
    greedy, _ = tr.translate_batch(syn.translate_inputs(batch))       # use_beam=False is the greedy path, unchanged
    for b, d in enumerate(greedy):
        np.testing.assert_array_equal(d.cpu().numpy(), z["decode/%d" % b])


@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("case,mt", CASES)
def test_beams_against_the_cpu_reference(golden_dir, case, mt, B):
    from svpc_amd.translator import Translator
    z, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    tr = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model)
    dec, _, scores = tr.translate_batch_beam(syn.translate_inputs(batch), B)
    assert _compare(dec, scores, _ref_beam(cfg, model, batch, B)) == 0


def test_beams_with_copied_oov_words(golden_dir):
    """a synthetic batch with out-of-vocabulary words in the copy distribution (extended columns ≥ V in the score rows)"""
    from svpc_amd.translator import Translator
    _, cfg, _, model = build_model("tiny", "vivt", golden_dir, DEV)
    batch = syn.make_batch(cfg, n_videos=3, max_steps=3, n_ingr=[3, 2, 3], n_oov=[2, 0, 3], seed=77, device=DEV)
    for B in (2, 4):
        tr = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model)
        dec, _, scores = tr.translate_batch_beam(syn.translate_inputs(batch), B)
        assert _compare(dec, scores, _ref_beam(cfg, model, batch, B)) == 0


@pytest.mark.parametrize("case,mt", [("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")])
def test_graph_replay_equals_eager(golden_dir, case, mt):
    from svpc_amd.translator import Translator
    z, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    eager = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model)
    graphed = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, graph=True)
    d0, _, s0 = eager.translate_batch_beam(syn.translate_inputs(batch), 4)
    for _ in range(2):                                  # capture, then replay
        d1, _, s1 = graphed.translate_batch_beam(syn.translate_inputs(batch), 4)
        for a, b, sa, sb in zip(d0, d1, s0, s1):
            assert torch.equal(a, b) and torch.equal(sa, sb)
    assert len(graphed._preps) == 1 and next(iter(graphed._preps.values())).graphs


# ------------------------------------------------------------------------------------------------ 6. config 5 at its headline size
# the parity record is written here (profiles/beam_parity.json is the committed copy); SVPC_REPORT_DIR overrides the directory
REPORT_DIR = os.environ.get("SVPC_REPORT_DIR") or os.path.join(ROOT, "reports")
FLOOR_X3 = 0.9        # bf16x3: fraction of the 8 × 12 × 22 ids identical to the fp32 CPU beam reference


@pytest.mark.timeout(2400)
def test_config5_beam_at_headline_size():
    import bench
    from svpc_amd.optim import WeightStore
    from svpc_amd.translator import Translator
    args = bench.parse_args([])
    cfg, model_cpu = bench.build(args, "cpu", model_type="vivt")
    drawn = syn.draw_parameters(list(model_cpu.named_parameters()), seed=7)
    with torch.no_grad():
        for n, p in model_cpu.named_parameters():
            p.copy_(drawn[n])
    model_cpu.eval()
    batch = syn.make_batch(cfg, n_videos=8, max_steps=12, n_ingr=10, n_oov=0, seed=2021, full_clips=True)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ref = _ref_beam(cfg, model_cpu, batch, 4)
    report = {}
    for precision in ("fp32", "bf16x3"):
        ops.set_precision(precision)
        try:
            model = copy.deepcopy(model_cpu).to(DEV)
            model.eval()
            WeightStore.for_model(model)
            tr = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, graph=True)
            b = {k: ([t.to(DEV) for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor) else
                     (v.to(DEV) if isinstance(v, torch.Tensor) else v)) for k, v in batch.items()}
            dec, _, scores = tr.translate_batch_beam(syn.translate_inputs(b), 4)
            torch.cuda.synchronize()
        finally:
            ops.set_precision("fp32")
        same = total = sent_same = 0
        for d, r in zip(dec, ref[0]):
            d = d.cpu()
            same += int((d == r).sum()); total += r.numel(); sent_same += int((d == r).all(1).sum())
        report[precision] = dict(token_agreement=same / total, identical_sentences=sent_same, sentences=sum(r.shape[0] for r in ref[0]),
                                 tokens=total)
        if precision == "fp32":
            report[precision]["near_tie_sentences"] = _compare(dec, scores, ref)
        os.makedirs(REPORT_DIR, exist_ok=True)
        with open(os.path.join(REPORT_DIR, "beam_parity.json"), "w") as f:
            json.dump(dict(beam=4, videos=8, clips=12, **report), f, indent=1)
        print("config 5, B = 4, %s: %d / %d ids identical to the CPU beam reference" % (precision, same, total))
    assert report["bf16x3"]["token_agreement"] >= FLOOR_X3, report
