"""Beam-search decoding controls on the MI355X: the selection kernel (svpc_beam_step_ctl) against tests/beam_controls_reference.py::
select_ctl bit for bit, the n-best finalize, and Translator.translate_batch_beam / translate_batch_nbest with controls against the CPU
reference (fp32 goldens), replayed against eager, greedy-with-controls against the width-1 beam, and config 5 at 64 videos in bf16x3."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import beam_controls_reference as bcr  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import ops, synthetic as syn  # noqa: E402
from svpc_amd.ops_common import Idx  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, PAD, UNK  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = type("O", (), {"cuda": True})
HOT = [8, 9, 10, 11, 12, EOS]                    # the few words the histories are drawn from; the scores favour them


# ------------------------------------------------------------------------------------------------ (a), (b) the selection kernel
def _tables(rng, T, B, Lt, pos, logits, adversarial):
    """scores / row_c / row_x / cum / finished / length / extended-id history for T sentences × B hypotheses: ragged C, OOV columns,
    finished rows, histories over a handful of words (so bans bite) that the scores rank first; adversarial: ties everywhere, −inf cums,
    a row of equal logits or zero probabilities."""
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
    hist = np.full((R, Lt), PAD, np.int64)
    hist[:, 0] = BOS
    hist[:, 1:pos + 1] = rng.choice(HOT[:-1], size=(R, pos), p=[0.3, 0.3, 0.3, 0.05, 0.05])
    for r in range(R):                            # a copied OOV word in some histories (its column is favoured too)
        C, X = int(Cs[r // B]), int(Xs[r // B])
        if X and rng.random() < 0.5:
            hist[r, rng.integers(1, pos + 1)] = C - 1
            s[r, C - 1] = s[r].max() if adversarial else (1.0 if not logits else 9.0)
    # every row ranks the HOT words first, in a random order (adversarial: tied at the two largest values)
    if adversarial:
        s[:, HOT] = vals[-2:][rng.integers(0, 2, size=(R, len(HOT)))]
    else:
        s[:, HOT] = rng.uniform(0.3, 0.6, size=(R, len(HOT))) if not logits else rng.uniform(4.0, 7.0, size=(R, len(HOT)))
    # half the rows repeat their first three words (positions 4 … 6 = 1 … 3) and rank the word that followed them first: every n ≤ 3
    # bans it unless an exclusion saves the gram
    top = (1.0 if not logits else 20.0) if not adversarial else (0.75 if not logits else 3.0)
    for r in np.nonzero(rng.random(R) < 0.5)[0]:
        hist[r, 4:7] = hist[r, 1:4]
        s[r, hist[r, 4]] = top
    if adversarial:
        s[R // 2] = 0.0                          # (zero probabilities: −inf step scores; equal logits: ties at every column)
    s[:, UNK] = 1.0 if not logits else 50.0
    fin = (rng.random(R) < 0.3).astype(np.int32)
    length = np.where(fin, rng.integers(1, pos + 1, size=R), rng.integers(0, Lt, size=R)).astype(np.int32)
    return s, np.repeat(Cs, B), np.repeat(Xs, B), cum, fin, length, hist


SETTINGS = {
    "off": dict(),
    "unigram": dict(block_ngram_repeat=1),
    "bigram": dict(block_ngram_repeat=2),
    "trigram_excl": dict(block_ngram_repeat=3, exclusion_tokens=(12,)),
    "unigram_excl": dict(block_ngram_repeat=1, exclusion_tokens=(8, EOS)),
    "min_length": dict(min_length=7),
    "min_length_edge": dict(min_length=6),
    "avg": dict(length_penalty_name="avg"),
    "wu": dict(length_penalty_name="wu", length_penalty_alpha=0.7),
    "all": dict(block_ngram_repeat=2, exclusion_tokens=(10,), min_length=7, length_penalty_name="wu", length_penalty_alpha=1.3),
}


def _kernel_args(c, Lt, V, dev):
    excl = (ops.exclusion_bitmap(c["exclusion_tokens"], V, dev), V) if c.get("exclusion_tokens") else None
    name = c.get("length_penalty_name", "none")
    lp_host = None if name == "none" else ops.length_penalty_table(name, c.get("length_penalty_alpha", 0.0), Lt)
    lp = torch.tensor(lp_host, dtype=torch.float64, device=dev) if lp_host is not None else None
    return dict(min_length=c.get("min_length", 0), block_ngram_repeat=c.get("block_ngram_repeat", 0), exclusion=excl, lp=lp), lp_host


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("B", [1, 2, 3, 4, 8])
def test_beam_step_ctl_equals_select_ctl(B, logits, setting):
    c = SETTINGS[setting]
    rng = np.random.default_rng(100 * B + 10 * logits + list(SETTINGS).index(setting))
    V = 700
    bans = 0
    for adversarial in (False, True):
        T, Lt, pos = 48, 12, 6
        s, row_c, row_x, cum, fin, length, hist = _tables(rng, T, B, Lt, pos, logits, adversarial)
        R = T * B
        kw, lp_host = _kernel_args(c, Lt, V, DEV)
        sd = torch.from_numpy(s).to(DEV)
        cum_d, fin_d, len_d = (torch.from_numpy(x).to(DEV) for x in (cum, fin, length))
        t_in = [torch.from_numpy(rng.integers(0, 1000, size=(R, Lt)).astype(np.int32)).to(DEV), torch.from_numpy(hist.astype(np.int32)).to(DEV),
                torch.from_numpy(rng.integers(0, 1000, size=(R, Lt)).astype(np.int32)).to(DEV)]
        t_out = [torch.full((R, Lt), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
        par, nx_ext, nx_mod = ops.beam_step(sd, Idx(row_c.tolist()), Idx(row_x.tolist()), B, pos, logits, UNK, EOS, PAD, cum_d, fin_d,
                                            t_in, t_out, Lt, length=len_d, **kw)
        torch.cuda.synchronize()
        ref = bcr.select_ctl(s, row_c, row_x, B, logits, cum, fin.astype(bool), length, hist, pos, min_length=c.get("min_length", 0),
                             block_ngram_repeat=c.get("block_ngram_repeat", 0), exclusion_tokens=c.get("exclusion_tokens", ()),
                             lp=lp_host)
        r_par, r_ext, r_mod, r_cum, r_fin, r_len = ref
        np.testing.assert_array_equal(par.cpu().numpy(), r_par)
        np.testing.assert_array_equal(nx_ext.cpu().numpy(), r_ext)
        np.testing.assert_array_equal(nx_mod.cpu().numpy(), r_mod)
        np.testing.assert_array_equal(cum_d.cpu().numpy().view(np.int32), r_cum.view(np.int32))
        np.testing.assert_array_equal(fin_d.cpu().numpy().astype(bool), r_fin)
        np.testing.assert_array_equal(len_d.cpu().numpy(), r_len)
        tin = [t.cpu().numpy() for t in t_in]
        tout = [t.cpu().numpy() for t in t_out]
        for k in range(3):
            np.testing.assert_array_equal(tout[k][:, :pos + 1], tin[k][r_par, :pos + 1])
            assert np.all(tout[k][:, pos + 2:] == -7)
        np.testing.assert_array_equal(tout[0][:, pos + 1], r_mod)
        np.testing.assert_array_equal(tout[1][:, pos + 1], r_ext)
        np.testing.assert_array_equal(tout[2][:, pos + 1], np.arange(R) * Lt + pos + 1)
        off = bcr.select_ctl(s, row_c, row_x, B, logits, cum, fin.astype(bool), length, hist, pos)
        bans += int(np.sum(off[1] != r_ext))
    if setting not in ("off", "min_length_edge") and not (B == 1 and setting in ("avg", "wu")):   # (B = 1: one row, one key order)
        assert bans > 0, "the control never changed a pick: the tables do not exercise it"


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("B", [1, 2, 3, 4, 8])
def test_beam_step_ctl_all_off_equals_beam_step(B, logits):
    """the new entry point with every control off (and a length array) = svpc_beam_step bit for bit"""
    rng = np.random.default_rng(7 * B + logits)
    for adversarial in (False, True):
        T, Lt, pos = 31, 10, 4
        s, row_c, row_x, cum, fin, length, hist = _tables(rng, T, B, Lt, pos, logits, adversarial)
        R = T * B
        outs = []
        for ctl in (False, True):
            sd = torch.from_numpy(s).to(DEV)
            cum_d, fin_d, len_d = (torch.from_numpy(x.copy()).to(DEV) for x in (cum, fin, length))
            t_in = [torch.from_numpy(hist.astype(np.int32)).to(DEV) for _ in range(3)]
            t_out = [torch.full((R, Lt), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
            kw = dict(length=len_d) if ctl else {}
            r = ops.beam_step(sd, Idx(row_c.tolist()), Idx(row_x.tolist()), B, pos, logits, UNK, EOS, PAD, cum_d, fin_d, t_in, t_out, Lt, **kw)
            outs.append([x.cpu() for x in r] + [cum_d.cpu(), fin_d.cpu()] + [t.cpu() for t in t_out])
        for a, b in zip(*outs):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("name,alpha", [("none", 0.0), ("avg", 0.0), ("wu", 0.9)])
@pytest.mark.parametrize("B", [1, 3, 4, 8])
def test_finalize_nbest(B, name, alpha):
    T, Lt = 70, 9
    g = torch.Generator().manual_seed(B)
    cum = torch.randn(T * B, generator=g)
    cum[B:2 * B] = -1.0                              # ties: the lower beam index first
    cum[2 * B] = float("-inf")
    length = torch.randint(1, Lt, (T * B,), generator=g, dtype=torch.int32)
    length[B:2 * B] = 3
    ext = torch.randint(0, 100, (T * B, Lt), dtype=torch.int32, generator=g)
    lp_host = None if name == "none" else ops.length_penalty_table(name, alpha, Lt)
    lp = torch.tensor(lp_host, dtype=torch.float64, device=DEV) if lp_host is not None else None
    for n_best in sorted({1, (B + 1) // 2, B}):
        ids, score, ln = ops.beam_finalize_nbest(cum.to(DEV), ext.to(DEV), B, n_best, length.to(DEV), lp)
        ids, score, ln = ids.cpu(), score.cpu(), ln.cpu()
        for t in range(T):
            order, _ = bcr.final_order(cum[t * B:(t + 1) * B].numpy(), length[t * B:(t + 1) * B].numpy(), lp_host)
            rows = [t * B + h for h in order[:n_best]]
            assert torch.equal(ids[t], ext[rows]) and torch.equal(score[t], cum[rows]) and torch.equal(ln[t], length[rows])
        if name == "none" and n_best == 1:           # = svpc_beam_finalize
            i1, s1 = ops.beam_finalize(cum.to(DEV), ext.to(DEV), B)
            assert torch.equal(i1.cpu(), ids[:, 0]) and torch.equal(s1.cpu(), score[:, 0])


# ------------------------------------------------------------------------------------------------ (c)-(e) the translator
CTL = dict(block_ngram_repeat=1, min_length=3, length_penalty_name="avg")


def _ref(cfg, model, batch, B, **ctl):
    P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    cpu = {k: ([t.cpu() for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor) else
               (v.cpu() if isinstance(v, torch.Tensor) else v)) for k, v in batch.items()}
    return bcr.beam_decode_ctl(P, cfg, cpu["input_ids_list"], cpu["video_features_list"], cpu["input_masks_list"], cpu["ingr_input_ids"],
                               cpu["ingr_sep_masks"], cpu["batch_step_num"], cpu["ingr_id_dict"], cpu["oov_word_dict"], beam=B, **ctl)


def _compare(dec, scores, lens, ref, n_best, tie=1e-4):
    """ids exactly, scores within 1e-4 relative (test_beam_gpu._compare's rule), lengths exactly — except for sentences where the reference
    itself shows a near-tie (a selection margin or a gap between final keys ≤ ``tie``), which are counted and returned"""
    r_ids, r_cum, r_len, r_mg = ref
    near = 0
    for v, (d, s) in enumerate(zip(dec, scores)):
        d, s = d.cpu(), s.cpu().numpy()
        if d.dim() == 2:
            d, s = d.unsqueeze(1), s[:, None]
        for j in range(d.shape[0]):
            ri = r_ids[v][j, :n_best]
            if torch.equal(d[j], ri):
                np.testing.assert_allclose(s[j], r_cum[v][j, :n_best], rtol=1e-4, atol=1e-6)
                if lens is not None:
                    np.testing.assert_array_equal(lens[v][j].cpu().numpy(), r_len[v][j, :n_best])
                continue
            assert float(np.nanmin(r_mg[v][j])) <= tie, ("ids differ without a near-tie", d[j].tolist(), ri.tolist())
            near += 1
    return near


@pytest.mark.parametrize("case,mt", [("tiny", "v"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")])
def test_controls_against_the_cpu_reference(golden_dir, case, mt):
    from svpc_amd.translator import Translator
    _, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    B = 3
    tr = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model)
    ref = _ref(cfg, model, batch, B, **CTL)
    dec, _, scores = tr.translate_batch_beam(syn.translate_inputs(batch), B, **CTL)
    assert _compare(dec, scores, None, ref, 1) == 0
    nd, _, ns, nl = tr.translate_batch_nbest(syn.translate_inputs(batch), B, B, **CTL)
    assert _compare(nd, ns, nl, ref, B) == 0
    for a, b, sa, sb in zip(dec, nd, scores, ns):
        assert a.dtype == b.dtype == torch.int64 and b.shape[1] == B
        assert torch.equal(a, b[:, 0]) and torch.equal(sa, sb[:, 0])
    plain, _, _ = tr.translate_batch_beam(syn.translate_inputs(batch), B)
    assert any(not torch.equal(a, b) for a, b in zip(plain, dec)), "the controls changed no caption: the test would pass vacuously"


def test_controls_with_copied_oov_words(golden_dir):
    from svpc_amd.translator import Translator
    _, cfg, _, model = build_model("tiny", "vivt", golden_dir, DEV)
    batch = syn.make_batch(cfg, n_videos=3, max_steps=3, n_ingr=[3, 2, 3], n_oov=[2, 0, 3], seed=77, device=DEV)
    ctl = dict(block_ngram_repeat=1, length_penalty_name="wu", length_penalty_alpha=0.8)
    tr = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model)
    nd, _, ns, nl = tr.translate_batch_nbest(syn.translate_inputs(batch), 4, 2, **ctl)
    assert _compare(nd, ns, nl, _ref(cfg, model, batch, 4, **ctl), 2) == 0


@pytest.mark.parametrize("case,mt", [("tiny", "vivt"), ("c1", "vivt")])
def test_graph_replay_equals_eager_with_controls(golden_dir, case, mt):
    from svpc_amd.translator import Translator
    _, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    ctl = dict(block_ngram_repeat=2, exclusion_tokens=(7,), min_length=2, length_penalty_name="wu", length_penalty_alpha=1.0)
    eager = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model)
    graphed = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, graph=True)
    e = eager.translate_batch_nbest(syn.translate_inputs(batch), 4, 3, **ctl)
    for _ in range(2):                                  # capture, then replay
        g = graphed.translate_batch_nbest(syn.translate_inputs(batch), 4, 3, **ctl)
        for k in (0, 2, 3):
            for a, b in zip(e[k], g[k]):
                assert torch.equal(a, b)
    graphed.translate_batch_beam(syn.translate_inputs(batch), 4)          # another setting: its own prep and graph
    assert len(graphed._preps) == 2 and all(p.graphs for p in graphed._preps.values())


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("case,mt", [("tiny", "v"), ("tiny", "vivt"), ("c1", "vivt")])
def test_greedy_with_controls_is_the_width_one_beam(golden_dir, case, mt, graph):
    from svpc_amd.translator import Translator
    z, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    opt = O()
    opt.block_ngram_repeat = 1
    opt.min_length = 2
    tr = Translator(opt, {"model_cfg": cfg, "model": model.state_dict()}, model=model, graph=graph)
    g, _ = tr.translate_batch(syn.translate_inputs(batch))
    b1, _, _ = tr.translate_batch_beam(syn.translate_inputs(batch), 1)
    for a, b in zip(g, b1):
        assert torch.equal(a, b)
    plain, _ = tr.translate_batch(syn.translate_inputs(batch), block_ngram_repeat=0, min_length=0)  # keywords override opt: greedy
    for v, a in enumerate(plain):
        np.testing.assert_array_equal(a.cpu().numpy(), z["decode/%d" % v])


# ------------------------------------------------------------------------------------------------ (f) config 5, 64 videos, bf16x3
@pytest.mark.timeout(1200)
def test_config5_controls_at_64_videos():
    import bench
    from svpc_amd.optim import WeightStore
    from svpc_amd.translator import Translator
    n, m, B = 3, 3, 4
    excl = (PAD, 7)
    args = bench.parse_args([])
    ops.set_precision("bf16x3")
    try:
        cfg, model = bench.build(args, DEV, model_type="vivt")
        model.eval()
        WeightStore.for_model(model)
        b = syn.make_batch(cfg, n_videos=64, max_steps=12, n_ingr=10, n_oov=0, seed=2019, full_clips=True, device=DEV)
        tr = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, graph=True)
        ctl = dict(block_ngram_repeat=n, exclusion_tokens=excl, min_length=m, length_penalty_name="avg")
        dec, _, cums, lens = tr.translate_batch_nbest(syn.translate_inputs(b), B, B, **ctl)
        best, _, best_s = tr.translate_batch_beam(syn.translate_inputs(b), B, **ctl)
        torch.cuda.synchronize()
    finally:
        ops.set_precision("fp32")
    lp = ops.length_penalty_table("avg", 0.0, cfg.max_t_len)
    n_sent = 0
    for d, c, ln, bd, bs in zip(dec, cums, lens, best, best_s):
        d, c, ln = d.cpu(), c.cpu().numpy(), ln.cpu().numpy()
        assert torch.equal(d[:, 0], bd.cpu()) and np.array_equal(c[:, 0], bs.cpu().numpy())
        for s in range(d.shape[0]):
            n_sent += 1
            keys = [float(np.float64(c[s, k]) / lp[ln[s, k]]) for k in range(B)]
            assert all(keys[k] >= keys[k + 1] for k in range(B - 1)), keys
            for k in range(B):
                y = d[s, k].tolist()
                L = int(ln[s, k])
                assert np.isfinite(c[s, k]) and 1 <= L <= cfg.max_t_len - 1
                assert EOS not in y[1:m + 1], y
                assert (L == cfg.max_t_len - 1 or y[L] == EOS) and EOS not in y[1:L] and all(v == PAD for v in y[L + 1:]), (y, L)
                grams = [tuple(y[j:j + n]) for j in range(1, L - n + 2) if not set(y[j:j + n]) & set(excl)]
                assert len(grams) == len(set(grams)), y
    assert n_sent == 64 * 12
