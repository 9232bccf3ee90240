"""Paragraph-scope n-gram blocking on the MI355X: the selection kernel (svpc_beam_step_para) against tests/paragraph_block_reference.py::
select_para bit for bit, the entry point with empty histories against svpc_beam_step_ctl, and Translator with block_ngram_scope="paragraph"
against the CPU reference (fp32 goldens, each sentence under the GPU's own earlier captions), sentence scope unchanged, greedy and n-best,
replay against eager, and config 5 at 64 ragged videos in bf16x3."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import beam_controls_reference as bcr  # noqa: E402
import paragraph_block_reference as pbr  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import ops, synthetic as syn  # noqa: E402
from svpc_amd.ops_common import Idx  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, PAD, UNK  # noqa: E402
from test_beam_controls_gpu import HOT, _compare, _kernel_args, _tables  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = type("O", (), {"cuda": True})


# ------------------------------------------------------------------------------------------------ the selection kernel
def _history(rng, T, Lt, row_c, row_x, B, kind):
    """a top-1 matrix of earlier captions and one (first row, count) pair per sentence.  kind: "empty" (no history), "short" (0 … 3
    captions), "long" (20 … 24 captions), "mixed"; captions are drawn from the HOT words (so they ban what the scores favour), with early
    EOS, PAD after it, a copied OOV word of the sentence's row and a stray mid-caption BOS now and then"""
    counts = {"empty": lambda: 0, "short": lambda: int(rng.integers(0, 4)), "long": lambda: int(rng.integers(20, 25)),
              "mixed": lambda: int(rng.choice([0, 1, 2, 21]))}[kind]
    rows, desc = [], []
    for t in range(T):
        k = counts()
        desc += [len(rows), k]
        C, X = int(row_c[t * B]), int(row_x[t * B])
        for _ in range(k):
            z = np.full(Lt, PAD, np.int64)
            z[0] = BOS
            L = int(rng.integers(1, Lt))
            z[1:L + 1] = rng.choice(HOT[:-1], size=L)
            if X and rng.random() < 0.4:
                z[rng.integers(1, L + 1)] = C - 1 - int(rng.integers(0, X))
            if rng.random() < 0.15:
                z[rng.integers(1, L + 1)] = BOS
            if L + 1 < Lt and rng.random() < 0.8:
                z[L + 1] = EOS
            elif L + 1 < Lt:
                z[L + 1] = 9                      # (a word after no EOS: PAD ends the caption at L + 2)
            rows.append(z)
    if not rows:
        rows.append(np.full(Lt, PAD, np.int64))
    return np.stack(rows), desc


def _plant(rng, table, desc, s, hist, row_c, B, pos, n):
    """in about half the sentences with a history, the last earlier caption starts with the gram (suffix of hypothesis 0, its best word):
    the history then bans what the scores favour most, unless an exclusion saves it"""
    for t in range(len(desc) // 2):
        if desc[2 * t + 1] == 0 or rng.random() < 0.5:
            continue
        r = t * B
        w = next(int(c) for c in np.argsort(-s[r, :row_c[r]], kind="stable") if c not in (UNK, EOS, PAD, BOS))
        z = table[desc[2 * t] + desc[2 * t + 1] - 1]
        z[1:n] = hist[r, pos - n + 2:pos + 1]
        z[n] = w


def _run_para(s, row_c, row_x, cum, fin, length, hist, table, desc, B, pos, logits, c, Lt, V, rng):
    R = s.shape[0]
    kw, lp_host = _kernel_args(c, Lt, V, DEV)
    sd = torch.from_numpy(s).to(DEV)
    cum_d, fin_d, len_d = (torch.from_numpy(x.copy()).to(DEV) for x in (cum, fin, length))
    t_in = [torch.from_numpy(rng.integers(0, 1000, size=(R, Lt)).astype(np.int32)).to(DEV), torch.from_numpy(hist.astype(np.int32)).to(DEV),
            torch.from_numpy(rng.integers(0, 1000, size=(R, Lt)).astype(np.int32)).to(DEV)]
    t_out = [torch.full((R, Lt), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
    tab_d = torch.from_numpy(table.astype(np.int32)).to(DEV)
    par, nx_ext, nx_mod = ops.beam_step(sd, Idx(row_c.tolist()), Idx(row_x.tolist()), B, pos, logits, UNK, EOS, PAD, cum_d, fin_d, t_in,
                                        t_out, Lt, length=len_d, history=(tab_d, desc, BOS), **kw)
    torch.cuda.synchronize()
    return (par.cpu().numpy(), nx_ext.cpu().numpy(), nx_mod.cpu().numpy(), cum_d.cpu().numpy(), fin_d.cpu().numpy(), len_d.cpu().numpy(),
            [t.cpu().numpy() for t in t_in], [t.cpu().numpy() for t in t_out], lp_host)


SETTINGS = {
    1: dict(block_ngram_repeat=1),
    2: dict(block_ngram_repeat=2, min_length=7, length_penalty_name="avg"),
    3: dict(block_ngram_repeat=3, exclusion_tokens=(12,)),
    4: dict(block_ngram_repeat=4, exclusion_tokens=(8,), length_penalty_name="wu", length_penalty_alpha=0.7),
}


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("B", [1, 2, 3, 4, 8])
def test_beam_step_para_equals_select_para(B, logits, n):
    c = SETTINGS[n]
    rng = np.random.default_rng(1000 + 100 * B + 10 * logits + n)
    V = 700
    para_bans = 0
    for kind, adversarial in (("short", False), ("long", False), ("mixed", True), ("empty", False)):
        T, Lt, pos = 40, 12, 6
        s, row_c, row_x, cum, fin, length, hist = _tables(rng, T, B, Lt, pos, logits, adversarial)
        if kind == "mixed":                       # narrow rows: the ban bitmap's last word, few candidates per sentence
            row_c[:2 * B] = 8
            row_x[:2 * B] = 0
        table, desc = _history(rng, T, Lt, row_c, row_x, B, kind)
        _plant(rng, table, desc, s, hist, row_c, B, pos, n)
        got = _run_para(s, row_c, row_x, cum, fin, length, hist, table, desc, B, pos, logits, c, Lt, V, rng)
        par, nx_ext, nx_mod, cum_g, fin_g, len_g, tin, tout, lp_host = got
        history = [[table[desc[2 * t] + q].tolist() for q in range(desc[2 * t + 1])] for t in range(T)]
        ctl = dict(min_length=c.get("min_length", 0), block_ngram_repeat=n, exclusion_tokens=c.get("exclusion_tokens", ()), lp=lp_host)
        r_par, r_ext, r_mod, r_cum, r_fin, r_len = pbr.select_para(s, row_c, row_x, B, logits, cum, fin.astype(bool), length, hist, pos,
                                                                   history, **ctl)
        np.testing.assert_array_equal(par, r_par)
        np.testing.assert_array_equal(nx_ext, r_ext)
        np.testing.assert_array_equal(nx_mod, r_mod)
        np.testing.assert_array_equal(cum_g.view(np.int32), r_cum.view(np.int32))
        np.testing.assert_array_equal(fin_g.astype(bool), r_fin)
        np.testing.assert_array_equal(len_g, r_len)
        for k in range(3):
            np.testing.assert_array_equal(tout[k][:, :pos + 1], tin[k][r_par, :pos + 1])
            assert np.all(tout[k][:, pos + 2:] == -7)
        np.testing.assert_array_equal(tout[1][:, pos + 1], r_ext)
        np.testing.assert_array_equal(tout[2][:, pos + 1], np.arange(T * B) * Lt + pos + 1)
        own = bcr.select_ctl(s, row_c, row_x, B, logits, cum, fin.astype(bool), length, hist, pos, **ctl)
        para_bans += int(np.sum(own[1] != r_ext))
        if kind == "empty":
            assert np.array_equal(own[1], r_ext)
    assert para_bans > 0, "the history never changed a pick: the tables do not exercise it"


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("B", [1, 2, 4, 8])
def test_empty_history_equals_beam_step_ctl(B, logits):
    """svpc_beam_step_para with every history empty = svpc_beam_step_ctl bit for bit (parents, ids, cum bits, lengths, tables)"""
    rng = np.random.default_rng(77 * B + logits)
    c = dict(block_ngram_repeat=2, exclusion_tokens=(10,), min_length=7, length_penalty_name="wu", length_penalty_alpha=1.3)
    for adversarial in (False, True):
        T, Lt, pos = 31, 10, 4
        s, row_c, row_x, cum, fin, length, hist = _tables(rng, T, B, Lt, pos, logits, adversarial)
        outs = []
        for para in (False, True):
            kw, _ = _kernel_args(c, Lt, 700, DEV)
            sd = torch.from_numpy(s).to(DEV)
            cum_d, fin_d, len_d = (torch.from_numpy(x.copy()).to(DEV) for x in (cum, fin, length))
            t_in = [torch.from_numpy(hist.astype(np.int32)).to(DEV) for _ in range(3)]
            t_out = [torch.full((T * B, Lt), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
            if para:
                kw["history"] = (torch.full((1, Lt), 9, dtype=torch.int32, device=DEV), [0, 0] * T, BOS)
            r = ops.beam_step(sd, Idx(row_c.tolist()), Idx(row_x.tolist()), B, pos, logits, UNK, EOS, PAD, cum_d, fin_d, t_in, t_out, Lt,
                              length=len_d, **kw)
            outs.append([x.cpu() for x in r] + [cum_d.cpu().view(torch.int32), fin_d.cpu(), len_d.cpu()] + [t.cpu() for t in t_out])
        for a, b in zip(*outs):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the translator
PARA = dict(block_ngram_repeat=1, block_ngram_scope="paragraph")


def _cpu(batch):
    return {k: ([t.cpu() for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor) else
                (v.cpu() if isinstance(v, torch.Tensor) else v)) for k, v in batch.items()}


def _ref_para(cfg, model, batch, B, history, **ctl):
    P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    cpu = _cpu(batch)
    ctl = {k: v for k, v in ctl.items() if k != "block_ngram_scope"}
    return pbr.beam_decode_para(P, cfg, cpu["input_ids_list"], cpu["video_features_list"], cpu["input_masks_list"], cpu["ingr_input_ids"],
                                cpu["ingr_sep_masks"], cpu["batch_step_num"], cpu["ingr_id_dict"], cpu["oov_word_dict"], beam=B,
                                history=history, **ctl)


def _assert_no_repeated_gram(dec, n, excl=()):
    """no non-excluded n-gram occurs twice in any video's paragraph (row 0 of each sentence)"""
    for d in dec:
        d = d.cpu()
        caps = [z.tolist() for z in (d[:, 0] if d.dim() == 3 else d)]
        grams = [g for z in caps for g in pbr.caption_grams(z, n) if not set(g) & set(excl)]
        assert len(grams) == len(set(grams)), caps


@pytest.mark.parametrize("case,mt", [("tiny", "v"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")])
def test_paragraph_against_the_cpu_reference(golden_dir, case, mt):
    from svpc_amd.translator import Translator
    _, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    B = 3
    ctl = dict(PARA, min_length=2, length_penalty_name="avg")
    tr = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model)
    nd, _, ns, nl = tr.translate_batch_nbest(syn.translate_inputs(batch), B, B, **ctl)
    hist = [[z.tolist() for z in d[:, 0].cpu()] for d in nd]          # each sentence under the GPU's own earlier captions
    ref = _ref_para(cfg, model, batch, B, hist, **ctl)
    assert _compare(nd, ns, nl, ref, B) == 0
    _assert_no_repeated_gram(nd, 1)
    dec, _, scores = tr.translate_batch_beam(syn.translate_inputs(batch), B, **ctl)
    for a, b, sa, sb in zip(dec, nd, scores, ns):
        assert torch.equal(a, b[:, 0]) and torch.equal(sa, sb[:, 0])
    sent, _, _ = tr.translate_batch_beam(syn.translate_inputs(batch), B, **dict(ctl, block_ngram_scope="sentence"))
    if case == "c1":
        assert any(not torch.equal(a, b) for a, b in zip(sent, dec)), "the scope changed no caption: the test would pass vacuously"


@pytest.mark.parametrize("graph", [False, True])
def test_explicit_sentence_scope_changes_nothing(golden_dir, graph):
    from svpc_amd.translator import Translator
    _, cfg, batch, model = build_model("c1", "vivt", golden_dir, DEV)
    tr = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, graph=graph)
    ctl = dict(block_ngram_repeat=2, min_length=1)
    for call in (lambda **k: tr.translate_batch_nbest(syn.translate_inputs(batch), 4, 2, **k),
                 lambda **k: tr.translate_batch_beam(syn.translate_inputs(batch), 2, **k)):
        for base in ({}, ctl):
            a = call(**base)
            b = call(block_ngram_scope="sentence", **base)
            for k in (0, 2) + ((3,) if len(a) == 4 else ()):
                for x, y in zip(a[k], b[k]):
                    assert torch.equal(x, y)
    g0, _ = tr.translate_batch(syn.translate_inputs(batch))
    g1, _ = tr.translate_batch(syn.translate_inputs(batch), block_ngram_scope="sentence")
    for x, y in zip(g0, g1):
        assert torch.equal(x, y)


@pytest.mark.parametrize("case,mt", [("tiny", "vivt"), ("c1", "v")])
def test_greedy_and_nbest_with_paragraph_scope(golden_dir, case, mt):
    from svpc_amd.translator import Translator
    _, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    opt = O()
    opt.block_ngram_repeat = 2
    opt.block_ngram_scope = "paragraph"
    tr = Translator(opt, {"model_cfg": cfg, "model": model.state_dict()}, model=model)
    g, _ = tr.translate_batch(syn.translate_inputs(batch))
    b1, _, _ = tr.translate_batch_beam(syn.translate_inputs(batch), 1)
    for a, b in zip(g, b1):
        assert torch.equal(a, b)
    nd, _, ns, _ = tr.translate_batch_nbest(syn.translate_inputs(batch), 4, 3)
    bd, _, bs = tr.translate_batch_beam(syn.translate_inputs(batch), 4)
    for a, b, sa, sb in zip(nd, bd, ns, bs):
        assert torch.equal(a[:, 0], b) and torch.equal(sa[:, 0], sb)
    _assert_no_repeated_gram(g, 2)
    _assert_no_repeated_gram(nd, 2)


def test_graph_replay_equals_eager_for_two_batches(golden_dir):
    """two batches of one structure: the second replay reads no history of the first"""
    from svpc_amd.translator import Translator
    _, cfg, _, model = build_model("tiny", "vivt", golden_dir, DEV)
    b0 = syn.make_batch(cfg, n_videos=3, max_steps=3, step_nums=[3, 1, 2], n_ingr=[3, 2, 3], n_oov=[2, 0, 1], seed=5, device=DEV)
    b1 = dict(b0, video_features_list=[f.flip(-1).contiguous() for f in b0["video_features_list"]])    # (same structure, other clips)
    batches = [b0, b1]
    ctl = dict(block_ngram_repeat=1, exclusion_tokens=(7,), min_length=1, length_penalty_name="wu", length_penalty_alpha=1.0,
               block_ngram_scope="paragraph")
    eager = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model)
    graphed = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, graph=True)
    outs = []
    for b in batches + batches:                      # capture on the first, replay the rest
        e = eager.translate_batch_nbest(syn.translate_inputs(b), 4, 2, **ctl)
        g = graphed.translate_batch_nbest(syn.translate_inputs(b), 4, 2, **ctl)
        for k in (0, 2, 3):
            for x, y in zip(e[k], g[k]):
                assert torch.equal(x, y)
        outs.append(g[0])
    assert len(graphed._preps) == 1 and all(p.graphs for p in graphed._preps.values())
    assert any(not torch.equal(x, y) for x, y in zip(outs[0], outs[1]))
    _assert_no_repeated_gram(outs[0], 1, (7,))


# ------------------------------------------------------------------------------------------------ config 5, 64 ragged videos, bf16x3
@pytest.mark.timeout(1200)
def test_config5_paragraph_at_64_videos():
    import bench
    from svpc_amd.optim import WeightStore
    from svpc_amd.translator import Translator
    n, excl = 3, (PAD, 7)
    args = bench.parse_args([])
    rng = np.random.default_rng(64)
    steps = [12] + [int(v) for v in rng.integers(1, 13, size=63)]
    ops.set_precision("bf16x3")
    try:
        cfg, model = bench.build(args, DEV, model_type="vivt")
        model.eval()
        WeightStore.for_model(model)
        b = syn.make_batch(cfg, n_videos=64, max_steps=12, step_nums=steps, n_ingr=10, n_oov=0, seed=2019, full_clips=True, device=DEV)
        tr = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, graph=True)
        res = {}
        for B in (1, 4):
            for scope in ("sentence", "paragraph"):
                ctl = dict(block_ngram_repeat=n, exclusion_tokens=excl, block_ngram_scope=scope)
                for _ in range(2):                   # capture, then replay
                    res[B, scope] = tr.translate_batch_beam(syn.translate_inputs(b), B, **ctl)[0]
        torch.cuda.synchronize()
    finally:
        ops.set_precision("fp32")
    for B in (1, 4):
        dec = res[B, "paragraph"]
        assert [d.shape[0] for d in dec] == steps
        _assert_no_repeated_gram(dec, n, excl)
        assert any(not torch.equal(x, y) for x, y in zip(dec, res[B, "sentence"])), B
