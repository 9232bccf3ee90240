"""Stochastic beam search on the MI355X: the selection kernel (svpc_beam_step_gumbel) against
tests/stochastic_beam_reference.py::stochastic_beam_select on the fixed inputs of tests/stochastic_beam_cases.py — whose margins
tests/test_stochastic_beam_host.py shows to be ≥ 1e-9, so no row is excused —, and Translator.translate_batch_stochastic end to end:
against the CPU restatement (fp32), W = 1 against sampling, distinct rows, forced scoring, seeds eagerly and under graph replay, consensus,
the other decodes left as they were, and bf16x3 at the sampling parity shape against the recorded fp32 CPU decode."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import stochastic_beam_cases as sbc  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import ops, synthetic as syn  # noqa: E402
from svpc_amd.ops_common import Idx  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, IGNORE, PAD, UNK  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = type("O", (), {"cuda": True})
TOL = 1e-9                # phi and G, kernel against reference on the same scores (absolute)


# ------------------------------------------------------------------------------------------------ 1. the selection kernel
def _run_kernel(c):
    W, R = c["W"], c["scores"].shape[0]
    cum, fin, ln = (torch.from_numpy(x.copy()).to(DEV) for x in (c["cum"], c["finished"].astype(np.int32), c["length"].astype(np.int32)))
    phi, G = torch.from_numpy(c["phi"].copy()).to(DEV), torch.from_numpy(c["G"].copy()).to(DEV)
    t_in = [torch.from_numpy(c["toks"][k].copy()).to(DEV) for k in range(3)]
    t_out = [torch.full((R, sbc.LT), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
    seed = torch.tensor([c["seed"]], dtype=torch.int64, device=DEV)
    parent, nx_ext, nx_mod = ops.stochastic_beam_step(torch.from_numpy(c["scores"].copy()).to(DEV), Idx(c["row_c"].tolist()),
                                                      Idx(c["row_x"].tolist()), W, sbc.POS, c["logits"], UNK, EOS, PAD, cum, phi, G, fin, ln,
                                                      t_in, t_out, sbc.LT, seed, temp=c["temp"], min_length=c["min_length"])
    torch.cuda.synchronize()
    return dict(parent=parent, ext=nx_ext, mod=nx_mod, cum=cum, phi=phi, G=G, finished=fin, length=ln), [t.cpu().numpy() for t in t_out]


def _close(got, ref, what):
    """−inf where the reference is −inf, within TOL elsewhere"""
    dead = np.isinf(ref)
    np.testing.assert_array_equal(np.isinf(got), dead, err_msg=what)
    assert np.all(np.abs(got[~dead] - ref[~dead]) <= TOL), (what, float(np.abs(got[~dead] - ref[~dead]).max()))


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("W", sbc.WIDTHS)
def test_kernel_equals_stochastic_beam_select(W, logits):
    keys = [k for k in sbc.case_list() if k[0] == W and k[1] == logits]
    assert [k[2] for k in keys] == list(sbc.COLS)
    for key in keys:
        c, ref = sbc.make_case(*key), sbc.reference(*key)
        assert ref["margin"].min() >= sbc.MARGIN
        out, t_out = _run_kernel(c)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        for k in ("parent", "ext", "mod", "length"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %r" % (k, key))
        np.testing.assert_array_equal(got["finished"].astype(bool), ref["finished"], err_msg="finished %r" % (key,))
        np.testing.assert_array_equal(got["cum"].view(np.int32), ref["cum"].view(np.int32), err_msg="cum bit for bit %r" % (key,))
        _close(got["phi"], ref["phi"], "phi %r" % (key,))
        _close(got["G"], ref["G"], "G %r" % (key,))
        p, R = sbc.POS + 1, len(ref["parent"])
        for k in range(3):                               # a child's tables: its parent's positions 0 … pos, then its own pick
            np.testing.assert_array_equal(t_out[k][:, :p], c["toks"][k][ref["parent"], :p])
            assert np.all(t_out[k][:, p + 1:] == -7)
        np.testing.assert_array_equal(t_out[0][:, p], ref["mod"])
        np.testing.assert_array_equal(t_out[1][:, p], ref["ext"])
        np.testing.assert_array_equal(t_out[2][:, p], np.arange(R) * sbc.LT + p)
        live = np.isfinite(ref["G"])
        assert live.any() and ((~live).any() or (W, key[2]) != (8, 7))       # C = 7 at W = 8: fewer than W candidates, dead rows


def test_kernel_reads_the_seed_on_the_device():
    """the same launch arguments with another seed word draw other rows; with the first seed again, the first rows"""
    key = [k for k in sbc.case_list() if k[0] == 4 and not k[1] and k[2] == 951][0]
    c = dict(sbc.make_case(*key))
    a = _run_kernel(c)[0]
    c["seed"] = c["seed"] ^ 0x5555
    b = _run_kernel(c)[0]
    assert not torch.equal(a["ext"], b["ext"])
    c["seed"] = c["seed"] ^ 0x5555
    a2 = _run_kernel(c)[0]
    assert all(torch.equal(a[k], a2[k]) for k in a)


def test_host_checks_before_any_device_work():
    key = [k for k in sbc.case_list() if k[0] == 2 and not k[1] and k[2] == 64][0]
    c = sbc.make_case(*key)
    R = c["scores"].shape[0]
    s = torch.from_numpy(c["scores"].copy()).to(DEV)
    vec = lambda dt: torch.zeros(R, dtype=dt, device=DEV)                                  # noqa: E731
    tabs = lambda: [torch.zeros(R, sbc.LT, dtype=torch.int32, device=DEV) for _ in range(3)]   # noqa: E731
    seed = torch.zeros(1, dtype=torch.int64, device=DEV)
    good = dict(scores=s, row_c=c["row_c"].tolist(), row_x=c["row_x"].tolist(), beam=2, pos=sbc.POS, logits=False, unk=UNK, eos=EOS, pad=PAD,
                cum=vec(torch.float32), phi=vec(torch.float64), gkey=vec(torch.float64), finished=vec(torch.int32), length=vec(torch.int32),
                toks_in=tabs(), toks_out=tabs(), slot_rows=sbc.LT, seed=seed)
    ops.stochastic_beam_step(**good)
    t = good["toks_in"]
    for bad in (dict(beam=0), dict(beam=9), dict(temp=0.0), dict(temp=float("nan")), dict(min_length=sbc.LT), dict(pos=sbc.LT - 1),
                dict(phi=vec(torch.float32)), dict(gkey=vec(torch.float64)[:-1]), dict(length=vec(torch.int64)), dict(toks_out=t), dict(max_cols=4097),
                dict(seed=torch.zeros(1, dtype=torch.int64))):
        with pytest.raises(ValueError):
            ops.stochastic_beam_step(**dict(good, **bad))


# ------------------------------------------------------------------------------------------------ 2. the translator
def _tr(cfg, model, **kw):
    from svpc_amd.translator import Translator
    return Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, **kw)


def _well_formed(res, batch, W, Lt, m=0):
    dec, _, cums, lens, Gs, phis = res
    assert len(dec) == len(batch["batch_step_num"])
    for d, c, ln, G, ph, S_b in zip(dec, cums, lens, Gs, phis, batch["batch_step_num"]):
        assert d.dtype == torch.int64 and c.dtype == torch.float32 and ln.dtype == torch.int64 and G.dtype == ph.dtype == torch.float64
        assert tuple(d.shape) == (S_b, W, Lt) and all(tuple(x.shape) == (S_b, W) for x in (c, ln, G, ph))
        d, ln, G, ph, c = d.cpu(), ln.cpu(), G.cpu(), ph.cpu(), c.cpu()
        assert torch.all(G[:, 1:] <= G[:, :-1]) and torch.all(torch.isfinite(G[:, 0]))      # the order drawn; row 0 is an ordinary sample
        assert torch.equal(torch.isinf(G), torch.isinf(ph)) and torch.equal(torch.isinf(G), torch.isinf(c))
        for s_ in range(S_b):
            rows = [tuple(d[s_, j].tolist()) for j in range(W) if torch.isfinite(G[s_, j])]
            assert len(set(rows)) == len(rows)                                  # the finite-G rows are pairwise different captions
            for j in range(W):
                y, L = d[s_, j].tolist(), int(ln[s_, j])
                assert y[0] == BOS and 1 <= L <= Lt - 1 and UNK not in y[1:]
                assert EOS not in y[1:L] and EOS not in y[1:m + 1] and all(v == PAD for v in y[L + 1:]), (y, L)
                if torch.isfinite(G[s_, j]):
                    assert float(ph[s_, j]) <= 0.0 and (y[L] == EOS or L == Lt - 1)


@pytest.mark.parametrize("case,mt", sbc.TRANSLATOR_CASES)
def test_decode_against_the_cpu_restatement(golden_dir, case, mt):
    _, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    tr = _tr(cfg, model)
    kw = sbc.TRANSLATOR_KW
    for W in sbc.TRANSLATOR_WIDTHS:
        seed = sbc.translator_seed(case, mt, W)
        ref = sbc.translator_reference(case, mt, W, cfg, model, batch)
        assert min(float(m.min()) for m in ref[5]) >= sbc.DECODE_MARGIN
        res = tr.translate_batch_stochastic(syn.translate_inputs(batch), W, seed=seed, **kw)
        assert int(tr.last_sample_seed) == seed
        _well_formed(res, batch, W, cfg.max_t_len, kw["min_length"])
        for d, c, ln, G, ph, ri, rc, rl, rG, rp in zip(res[0], res[2], res[3], res[4], res[5], *ref[:5]):
            assert torch.equal(d.cpu(), ri), (W, d.cpu().tolist(), ri.tolist())
            np.testing.assert_array_equal(ln.cpu().numpy(), rl)
            np.testing.assert_allclose(c.cpu().numpy(), rc, rtol=1e-4, atol=1e-6)
            np.testing.assert_allclose(G.cpu().numpy(), rG, rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(ph.cpu().numpy(), rp, rtol=1e-4, atol=1e-4)
        if W == 1:        # W = 1 is translate_batch_sample(num_samples=1) with the same τ, m and seed: the same ids, cum bit for bit
            dec, _, cums, lens = tr.translate_batch_sample(syn.translate_inputs(batch), 1, seed=seed, **kw)
            for a, b in zip(res[0] + res[2] + res[3], dec + cums + lens):
                assert torch.equal(a, b)
        # forced scoring reproduces cum: of the finite-G rows, and up to a drawn PAD — PAD is a column like any other to the draw (K0 is
        # sampling's set), while to forced scoring a PAD ends the given caption; the untrained fixtures do draw it now and then
        sc = tr.score_captions(syn.translate_inputs(batch), res[0])
        compared = 0
        for d, ln, c, f, G in zip(res[0], res[3], res[2], sc.score_list, res[4]):
            pos = torch.arange(d.shape[-1], device=d.device)
            drew_pad = ((d == PAD) & (pos >= 1) & (pos <= ln.unsqueeze(-1))).any(-1)
            ok = torch.isfinite(G) & ~drew_pad
            compared += int(ok.sum())
            np.testing.assert_allclose(f[ok].cpu().numpy(), c[ok].cpu().numpy(), rtol=1e-4, atol=1e-6)
        assert compared >= sum(int(torch.isfinite(G).sum()) for G in res[4]) // 2


def test_copied_words_and_dead_rows(golden_dir):
    """a batch with copied OOV words (their extended ids are kept) at the widest beam, against the CPU restatement"""
    _, cfg, _, model = build_model("tiny", "vivt", golden_dir, DEV)
    batch = syn.make_batch(cfg, n_videos=3, max_steps=3, n_ingr=[3, 2, 3], n_oov=[2, 0, 3], seed=77, device=DEV)
    tr = _tr(cfg, model)
    found = None
    for seed in range(5, 25):                      # the first seed whose reference margins clear the fp32 score noise
        sbc.TRANSLATOR_SEEDS[("tiny-oov", "vivt", 8)] = seed
        sbc._DECODES.pop(("tiny-oov", "vivt", 8), None)
        ref = sbc.translator_reference("tiny-oov", "vivt", 8, cfg, model, batch)
        if min(float(m.min()) for m in ref[5]) >= sbc.DECODE_MARGIN:
            found = seed
            break
    assert found is not None
    res = tr.translate_batch_stochastic(syn.translate_inputs(batch), 8, seed=found, **sbc.TRANSLATOR_KW)
    _well_formed(res, batch, 8, cfg.max_t_len, sbc.TRANSLATOR_KW["min_length"])
    for d, ln, ri, rl in zip(res[0], res[3], ref[0], ref[2]):
        assert torch.equal(d.cpu(), ri)
        np.testing.assert_array_equal(ln.cpu().numpy(), rl)
    assert any(int(d.max()) >= cfg.vocab_size for d in res[0]), "no copied word was drawn"


@pytest.mark.parametrize("case,mt", [("tiny", "vivt"), ("c1", "v")])
def test_seeds_eager_and_replayed(golden_dir, case, mt):
    _, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
    kw = dict(random_sampling_temp=1.5)
    eager, graphed = _tr(cfg, model), _tr(cfg, model, graph=True)
    e = eager.translate_batch_stochastic(syn.translate_inputs(batch), 4, seed=99, **kw)
    e2 = eager.translate_batch_stochastic(syn.translate_inputs(batch), 4, seed=100, **kw)
    assert any(not torch.equal(a, b) for a, b in zip(e[0], e2[0])), "another seed drew the same rows"
    for it in range(3):                                 # capture, then replay; a seed=None call in between changes nothing
        g = graphed.translate_batch_stochastic(syn.translate_inputs(batch), 4, seed=99, **kw)
        for k in (0, 2, 3, 4, 5):
            for a, b in zip(e[k], g[k]):
                assert torch.equal(a, b)
        assert int(graphed.last_sample_seed) == 99
        graphed.translate_batch_stochastic(syn.translate_inputs(batch), 4, **kw)
    assert len(graphed._preps) == 1 and next(iter(graphed._preps.values())).graphs
    a = graphed.translate_batch_stochastic(syn.translate_inputs(batch), 4, **kw)
    sa = int(graphed.last_sample_seed)
    b = graphed.translate_batch_stochastic(syn.translate_inputs(batch), 4, **kw)
    sb = int(graphed.last_sample_seed)
    assert sa != sb and sa != 99
    assert any(not torch.equal(x, y) for x, y in zip(a[0], b[0])), "two replays with seed=None drew the same rows"
    r = eager.translate_batch_stochastic(syn.translate_inputs(batch), 4, seed=sb, **kw)      # the seed a replay used reproduces it eagerly
    for x, y in zip(b[0], r[0]):
        assert torch.equal(x, y)
    # another setting is another plan and another graph
    graphed.translate_batch_stochastic(syn.translate_inputs(batch), 4, seed=99, random_sampling_temp=1.5, min_length=2)
    graphed.translate_batch_stochastic(syn.translate_inputs(batch), 3, seed=99, **kw)
    assert len(graphed._preps) == 3


def test_consensus_picks_among_its_own_candidates(golden_dir):
    from svpc_amd.caption_scores import ReferenceCorpus
    _, cfg, batch, model = build_model("tiny", "vivt", golden_dir, DEV)
    Vm, N = cfg.vocab_size, len(batch["batch_step_num"])
    i2w = ["[PAD]", "[CLS]", "[SEP]", "[VID]", "[BOS]", "[EOS]", "[UNK]"] + ["".join(chr(97 + (i // 26 ** k) % 26) for k in range(3))
                                                                             for i in range(7, Vm)]
    refs = {}
    for b in range(N):                                   # the idf corpus: the synthetic labels as "training references"
        inv = {int(v): k for k, v in batch["oov_word_dict"][b].items()}
        sents = [" ".join(i2w[x] if x < Vm else inv[x] for x in batch["input_labels_list"][s][b].cpu().tolist() if x not in (IGNORE, EOS, PAD))
                 for s in range(int(batch["batch_step_num"][b]))]
        refs["vid%d" % b] = [" ".join(sents)]
    plan = ReferenceCorpus(i2w, refs, device=DEV).plan([dict(oov_word_dict=batch["oov_word_dict"][b]) for b in range(N)], references=False)
    tr = _tr(cfg, model)
    K = 3
    dec = tr.translate_batch_stochastic(syn.translate_inputs(batch), K, seed=17, random_sampling_temp=1.2)[0]
    for scope, weights in (("paragraph", "uniform"), ("sentence", "posterior")):
        got, oov, picks = tr.translate_batch_consensus(syn.translate_inputs(batch), plan, source="stochastic", num_candidates=K, seed=17,
                                                       random_sampling_temp=1.2, scope=scope, weights=weights)
        assert len(oov) == N
        for b in range(N):
            S = dec[b].shape[0]
            assert tuple(got[b].shape) == (S, cfg.max_t_len) and got[b].dtype == torch.int64
            assert int(picks[b].min()) >= 0 and int(picks[b].max()) < K
            assert torch.equal(got[b], dec[b][torch.arange(S, device=DEV), picks[b]])
    with pytest.raises(TypeError):
        tr.translate_batch_consensus(syn.translate_inputs(batch), plan, source="stochastic", num_candidates=K, random_sampling_topk=3)


@pytest.mark.parametrize("graph", [False, True])
def test_other_decodes_are_unchanged(golden_dir, graph):
    """greedy, beam, n-best and sampling give the same results before and after stochastic decodes of the same translator"""
    z, cfg, batch, model = build_model("c1", "vivt", golden_dir, DEV)
    tr = _tr(cfg, model, graph=graph)

    def others():
        g = tr.translate_batch(syn.translate_inputs(batch))[0]
        bm = tr.translate_batch_beam(syn.translate_inputs(batch), 3)
        nb = tr.translate_batch_nbest(syn.translate_inputs(batch), 4, 4)
        sm = tr.translate_batch_sample(syn.translate_inputs(batch), 4, seed=11, random_sampling_temp=0.9)
        return [[t.clone() for t in lst] for lst in (g, bm[0], bm[2], nb[0], nb[2], nb[3], sm[0], sm[2], sm[3])]
    before = others()
    for b, d in enumerate(before[0]):
        np.testing.assert_array_equal(d.cpu().numpy(), z["decode/%d" % b])
    tr.translate_batch_stochastic(syn.translate_inputs(batch), 4, seed=11, random_sampling_temp=0.9)
    tr.translate_batch_stochastic(syn.translate_inputs(batch), 3)
    after = others()
    for x, y in zip(before, after):
        for a, b in zip(x, y):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 3. bf16x3 at the sampling parity shape
GOLDEN = os.path.join(ROOT, "tests", "golden", "stochastic_beam_config5.json")
REPORT_DIR = os.environ.get("SVPC_REPORT_DIR") or os.path.join(ROOT, "reports")
MEASURED_X3 = 1.0         # 96 / 96 sentences (fp32: 96 / 96): the share measured on the MI355X, profiles/stochastic_beam_parity.json
REBUILD_ALLOWANCE = 0.05  # a rebuild may move a near-tie


def test_config5_parity_with_the_recorded_cpu_decode():
    """8 videos × 12 clips, W = 4, τ = 0.8, seed 2024: the share of sentences whose W ids equal the fp32 CPU restatement's (recorded by
    tools/make_golden_stochastic_beam.py), fp32 and bf16x3; the run is deterministic, the bf16x3 share is asserted against the measured
    one less the rebuild allowance; written to reports/stochastic_beam_parity.json (profiles/ holds the committed copy)."""
    from tools import make_golden_stochastic_beam as mk
    from svpc_amd.optim import WeightStore
    rec = json.load(open(GOLDEN))
    assert {k: rec[k] for k in mk.SHAPE} == mk.SHAPE
    cfg, model_cpu, batch = mk.model_and_batch()
    assert cfg.max_t_len == rec["max_t_len"] and cfg.vocab_size == rec["vocab_size"]
    W = rec["beam_size"]
    report = {}
    for precision in ("fp32", "bf16x3"):
        ops.set_precision(precision)
        try:
            model = copy.deepcopy(model_cpu).to(DEV)
            model.eval()
            WeightStore.for_model(model)
            tr = _tr(cfg, model, graph=True)
            b = {k: ([t.to(DEV) for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor) else
                     (v.to(DEV) if isinstance(v, torch.Tensor) else v)) for k, v in batch.items()}
            res = tr.translate_batch_stochastic(syn.translate_inputs(b), W, seed=rec["seed"], random_sampling_temp=rec["random_sampling_temp"],
                                                min_length=rec["min_length"])
            torch.cuda.synchronize()
        finally:
            ops.set_precision("fp32")
        _well_formed(res, batch, W, cfg.max_t_len)
        same = rows_same = total = 0
        for d, r in zip(res[0], rec["ids"]):
            eq = (d.cpu() == torch.tensor(r)).all(-1)
            same += int(eq.all(-1).sum()); rows_same += int(eq.sum()); total += eq.shape[0]
        report[precision] = dict(identical_sentences=same, sentences=total, share=same / total, identical_rows=rows_same, rows=total * W)
        print("config 5, W = %d, %s: %d / %d sentences identical to the fp32 CPU restatement (%d / %d rows)"
              % (W, precision, same, total, rows_same, total * W))
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "stochastic_beam_parity.json"), "w") as f:
        json.dump(dict({k: rec[k] for k in mk.SHAPE}, smallest_reference_margin=min(min(v) for v in rec["margin"]), **report), f, indent=1)
    assert MEASURED_X3 is not None, "the bf16x3 share has not been measured yet: %r" % (report,)
    assert report["bf16x3"]["share"] >= MEASURED_X3 - REBUILD_ALLOWANCE, report
