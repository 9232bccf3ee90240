"""Diverse (group) beam search on the MI355X: the selection kernel (svpc_beam_step_groups) against
tests/diverse_beam_reference.py::select_groups bit for bit, against ``ops.beam_step`` where the two must coincide (G = 1; λ = 0 per group),
and ``Translator.translate_batch_diverse`` against the CPU restatement built on the oracle's decoder blocks (fp32 goldens), against
``translate_batch_nbest``, ``score_captions`` and ``consensus``, replayed against eager, and under bf16x3.

Near-ties (the project's rule of §11.7 / §11.8): a sentence whose restatement shows a selection margin in any group, or a gap between
consecutive final keys of a group, ≤ 1e-4 may decode differently; at most 5 % of a fixture's sentences may be such, asserted on the
restatement alone (``test_near_tie_cap_of_the_restatement``).  The batch seeds of the ``c1`` cases and of the OOV batch were chosen on
the CPU, from the restatement alone, so that the cap holds (``C1_SEED``, ``OOV_SEED``)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import diverse_beam_reference as dbr  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import ops, synthetic as syn  # noqa: E402
from svpc_amd.ops_common import Idx  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, PAD, UNK  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = type("O", (), {"cuda": True})
TIE = 1e-4
NEAR_SHARE = 0.05
REPORT_DIR = os.environ.get("SVPC_REPORT_DIR") or os.path.join(ROOT, "reports")
# bf16x3 at the config-1 shape: the worst |cum − fp32 CPU restatement| over the sentences whose ids agree, measured on the MI355X
# (profiles/diverse_beam_parity.json); the assertion is at twice that, the margin §11.8 gives split-product rounding, which varies with
# the caption.
MEASURED_X3 = 0.0004711151123046875         # ("c1", "vivt"); ("c1", "v"): 0.00031; cum there is about −40 … −95
BOUND_X3 = 2.0 * MEASURED_X3

# ------------------------------------------------------------------------------------------------ (a)-(d) the selection kernel
WG = [(1, 1), (2, 2), (3, 1), (3, 3), (4, 2), (6, 2), (6, 3), (8, 1), (8, 4), (8, 8)]
COLS = [7, 64, 65, 951, 4097, "mixed"]             # (C = 7: six candidates per live row, fewer than W = 8)
LAMS = [0.0, 0.5, 1e4]
LT = 12
MID = 6
SETTINGS = [dict(), dict(block_ngram_repeat=1), dict(block_ngram_repeat=2, exclusion_tokens=(2,)), dict(min_length=MID + 1),
            dict(length_penalty_name="wu", length_penalty_alpha=0.7),
            dict(block_ngram_repeat=2, exclusion_tokens=(3,), min_length=MID + 1, length_penalty_name="avg")]


def _tables(rng, T, W, C, pos, logits, adversarial):
    """scores / row_c / row_x / cum / aug / finished / length / extended-id history of T sentences × W rows.  One C per sentence (as the
    decoder has it; "mixed": another C for every sentence of the launch), copied-word columns, histories over a few words that the scores
    rank first (so bans and penalties bite), at a middle position some finished rows, some −inf rows and penalties already paid;
    adversarial: rows of few distinct values (ties), a row of zero probabilities / equal logits."""
    Cs = rng.integers(UNK + 2, 700, size=T) if C == "mixed" else np.full(T, C)
    if C == "mixed":
        Cs[0] = 7
    Xs = np.array([rng.integers(0, min(4, c - UNK - 1)) if c > UNK + 2 else 0 for c in Cs])
    cmax, R = int(Cs.max()), T * W
    if adversarial:
        vals = np.array([0.0, 0.125, 0.25, 0.5] if not logits else [-3.0, -1.0, 0.0, 2.0], np.float32)
        s = vals[rng.integers(0, len(vals), size=(R, cmax))]
    else:
        s = (rng.random((R, cmax)) ** 4).astype(np.float32) if not logits else (rng.standard_normal((R, cmax)) * 3).astype(np.float32)
    hot = [1, 2, 3, EOS]                            # words every C ≥ 7 has
    if not adversarial:                            # every row ranks the hot words first, the rows of a sentence mostly alike
        base = rng.uniform(0.3, 0.6, size=(T, len(hot))) if not logits else rng.uniform(4.0, 7.0, size=(T, len(hot)))
        s[:, hot] = (np.repeat(base, W, 0) + rng.uniform(0, 0.05, size=(R, len(hot)))).astype(np.float32)
    else:
        s[:, hot] = vals[-2:][rng.integers(0, 2, size=(R, len(hot)))]
    hist = np.full((R, LT), PAD, np.int64)
    hist[:, 0] = BOS
    hist[:, 1:pos + 1] = rng.choice(hot[:-1], size=(R, pos))
    for r in range(R):                              # a copied OOV word in some histories, its column favoured too
        c, x = int(Cs[r // W]), int(Xs[r // W])
        if x and pos and rng.random() < 0.5:
            hist[r, rng.integers(1, pos + 1)] = c - 1
            s[r, c - 1] = s[r].max()
    if adversarial:
        s[R // 2] = 0.0
    s[:, UNK] = 1.0 if not logits else 50.0         # UNK would win every comparison were it a candidate
    if pos == 0:                                    # the start: all groups share one parent state
        cum = dbr.start_scores(T, W, W if adversarial and W > 1 else 1)      # (adversarial: every row alive, as with G = W)
        aug, fin, length = cum.copy(), np.zeros(R, np.int32), np.zeros(R, np.int32)
    else:
        cum = (-rng.random(R) * 5).astype(np.float32)
        if adversarial:
            cum = np.array([-1.0, -0.5, 0.0], np.float32)[rng.integers(0, 3, size=R)]
        aug = (cum - np.array([0.0, 0.5, 1.0], np.float32)[rng.integers(0, 3, size=R)]).astype(np.float32)
        dead = rng.random(R) < 0.15
        cum[dead], aug[dead] = -np.inf, -np.inf
        fin = ((rng.random(R) < 0.3) | dead).astype(np.int32) if not adversarial else (rng.random(R) < 0.3).astype(np.int32)
        length = np.where(fin, rng.integers(1, pos + 1, size=R), 0).astype(np.int32)
    return dict(s=s, row_c=np.repeat(Cs, W), row_x=np.repeat(Xs, W), cum=cum, aug=aug, fin=fin, length=length, hist=hist, pos=pos, T=T, W=W,
                logits=logits, tin=[rng.integers(0, 1000, size=(R, LT)).astype(np.int32), hist.astype(np.int32),
                                    rng.integers(0, 1000, size=(R, LT)).astype(np.int32)])


def _kernel_args(c, V):
    excl = (ops.exclusion_bitmap(c["exclusion_tokens"], V, DEV), V) if c.get("exclusion_tokens") else None
    name = c.get("length_penalty_name", "none")
    lp_host = dbr.length_table(name, c.get("length_penalty_alpha", 0.0), LT)
    lp = torch.tensor(lp_host, dtype=torch.float64, device=DEV) if lp_host is not None else None
    return dict(min_length=c.get("min_length", 0), block_ngram_repeat=c.get("block_ngram_repeat", 0), exclusion=excl, lp=lp), lp_host


def _bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _run(tab, rows, W, G, lam, c, plain=False):
    """the kernel on the rows ``rows`` of a table (``plain``: ``ops.beam_step`` with controls instead) → numpy outputs"""
    kw, _ = _kernel_args(c, 700)
    R = len(rows)
    sd = torch.from_numpy(np.ascontiguousarray(tab["s"][rows])).to(DEV)
    cum_d, aug_d, fin_d, len_d = (torch.from_numpy(tab[k][rows].copy()).to(DEV) for k in ("cum", "aug", "fin", "length"))
    t_in = [torch.from_numpy(np.ascontiguousarray(t[rows])).to(DEV) for t in tab["tin"]]
    t_out = [torch.full((R, LT), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
    rc, rx = Idx(tab["row_c"][rows].tolist()), Idx(tab["row_x"][rows].tolist())
    if plain:
        par, ext, mod = ops.beam_step(sd, rc, rx, W, tab["pos"], tab["logits"], UNK, EOS, PAD, cum_d, fin_d, t_in, t_out, LT, length=len_d, **kw)
    else:
        pen = torch.tensor(ops.diversity_table(lam, W), dtype=torch.float32, device=DEV)
        par, ext, mod = ops.beam_step_groups(sd, rc, rx, W, G, tab["pos"], tab["logits"], UNK, EOS, PAD, cum_d, aug_d, fin_d, len_d, t_in,
                                             t_out, LT, pen, **kw)
    torch.cuda.synchronize()
    return dict(par=par.cpu().numpy(), ext=ext.cpu().numpy(), mod=mod.cpu().numpy(), cum=cum_d.cpu().numpy(), aug=aug_d.cpu().numpy(),
                fin=fin_d.cpu().numpy(), len=len_d.cpu().numpy(), tout=[t.cpu().numpy() for t in t_out])


def _cases(W, G, logits):
    """every C at the start and at a middle position; T, λ, the control setting and the kind of rows rotate so that each (W, G, mode)
    meets every C with both positions, and over the 20 (W, G, mode) all combinations come up"""
    off = WG.index((W, G)) * 2 + int(logits)
    for i, (C, pos) in enumerate((C, pos) for C in COLS for pos in (0, MID)):
        T = 1 if (C == 4097 or (i + off) % 4 == 0) and C != "mixed" else 5
        yield C, pos, T, LAMS[(i + i // 6 + off // 6) % 3], SETTINGS[(i + off) % len(SETTINGS)], (i // 2 + off) % 2 == 1


def _restatement(tab, W, G, lam, c):
    _, lp_host = _kernel_args(c, 700)
    return dbr.select_groups(tab["s"], tab["row_c"], tab["row_x"], W, G, tab["logits"], tab["cum"], tab["aug"], tab["fin"].astype(bool),
                             tab["length"], tab["hist"], tab["pos"], dbr.penalty_table(lam, W), min_length=c.get("min_length", 0),
                             block_ngram_repeat=c.get("block_ngram_repeat", 0), exclusion_tokens=c.get("exclusion_tokens", ()), lp=lp_host)


def _against_restatement(tab, W, G, lam, c, what):
    T, pos = tab["T"], tab["pos"]
    R = T * W
    got = _run(tab, np.arange(R), W, G, lam, c)
    ref = _restatement(tab, W, G, lam, c)
    r_par, r_ext, r_mod, r_cum, r_aug, r_fin, r_len = ref
    np.testing.assert_array_equal(got["par"], r_par, err_msg=what)
    np.testing.assert_array_equal(got["ext"], r_ext, err_msg=what)
    np.testing.assert_array_equal(got["mod"], r_mod, err_msg=what)
    np.testing.assert_array_equal(_bits(got["cum"]), _bits(r_cum), err_msg=what)
    np.testing.assert_array_equal(_bits(got["aug"]), _bits(r_aug), err_msg=what)
    np.testing.assert_array_equal(got["fin"].astype(bool), r_fin, err_msg=what)
    np.testing.assert_array_equal(got["len"], r_len, err_msg=what)
    for k in range(3):
        np.testing.assert_array_equal(got["tout"][k][:, :pos + 1], tab["tin"][k][r_par, :pos + 1], err_msg=what)
        assert np.all(got["tout"][k][:, pos + 2:] == -7)
    np.testing.assert_array_equal(got["tout"][0][:, pos + 1], r_mod)
    np.testing.assert_array_equal(got["tout"][1][:, pos + 1], r_ext)
    np.testing.assert_array_equal(got["tout"][2][:, pos + 1], np.arange(R) * LT + pos + 1)
    return got


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("W,G", WG)
def test_kernel_equals_the_restatement(W, G, logits):
    """(a) everything bit for bit; last, fill rows: C = 7 with unigram blocking and a minimum length leaves a row that has used words 0 … 4
    without a candidate, so the groups of a sentence of such rows (all live, finite cum) have fewer than Bg candidates — none at all"""
    rng = np.random.default_rng(1000 * W + 10 * G + logits)
    moved = 0
    for C, pos, T, lam, c, adversarial in _cases(W, G, logits):
        tab = _tables(rng, T, W, C, pos, logits, adversarial)
        got = _against_restatement(tab, W, G, lam, c, "C %s pos %d T %d lam %g %s adversarial %s" % (C, pos, T, lam, c, adversarial))
        if lam > 0 and G > 1:
            moved += int(np.sum(got["ext"] != _restatement(tab, W, G, 0.0, c)[1]))
    assert G == 1 or moved > 0, "the penalty never changed a pick: the tables do not exercise it"
    tab = _tables(rng, 5, W, 7, MID, logits, False)
    starved = np.arange(5 * W) < W + (W + 1) // 2            # sentence 0 and the first rows of sentence 1
    tab["hist"][starved, 1:MID + 1] = [0, 1, 2, 3, 4, 0]
    tab["tin"][1] = tab["hist"].astype(np.int32)
    tab["fin"][starved], tab["length"][starved] = 0, 0
    tab["cum"][starved], tab["aug"][starved] = -1.0, -1.5
    got = _against_restatement(tab, W, G, 0.5, dict(block_ngram_repeat=1, min_length=MID + 1), "fill rows")
    np.testing.assert_array_equal(got["par"][:W], np.arange(W))
    assert np.all(got["ext"][:W] == PAD) and np.all(np.isneginf(got["cum"][:W])) and np.all(np.isneginf(got["aug"][:W]))
    assert np.all(got["fin"][:W] == 1) and np.all(got["len"][:W] == MID + 1)


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("W", [1, 2, 3, 4, 6, 8])
def test_one_group_equals_beam_step(W, logits):
    """(b) G = 1 with aug = cum: ``ops.beam_step`` with controls on the same inputs, bit for bit, whatever λ"""
    rng = np.random.default_rng(77 * W + logits)
    for i, (C, pos) in enumerate((C, pos) for C in (7, 65, "mixed") for pos in (0, MID)):
        tab = _tables(rng, 5, W, C, pos, logits, i % 2 == 1)
        tab["aug"] = tab["cum"].copy()
        c = SETTINGS[(i + W) % len(SETTINGS)]
        rows = np.arange(5 * W)
        a, b = _run(tab, rows, W, 1, LAMS[i % 3], c), _run(tab, rows, W, 1, 0.0, c, plain=True)
        for k in ("par", "ext", "mod", "cum", "fin", "len"):
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)
        np.testing.assert_array_equal(_bits(a["aug"]), _bits(a["cum"]))
        for x, y in zip(a["tout"], b["tout"]):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("W,G", [(2, 2), (4, 2), (6, 2), (6, 3), (8, 4), (8, 8)])
def test_zero_strength_groups_equal_the_narrow_beam_step(W, G, logits):
    """(c) λ = 0: group g's outputs = ``ops.beam_step`` of width Bg on that group's rows, bit for bit"""
    Bg = W // G
    rng = np.random.default_rng(55 * W + 5 * G + logits)
    for i, (C, pos) in enumerate((C, pos) for C in (7, 64, "mixed") for pos in (0, MID)):
        T = 5
        tab = _tables(rng, T, W, C, pos, logits, i % 2 == 1)
        if pos == 0:
            tab["cum"] = dbr.start_scores(T, W, G)
        tab["aug"] = tab["cum"].copy()
        c = SETTINGS[(i + G) % len(SETTINGS)]
        a = _run(tab, np.arange(T * W), W, G, 0.0, c)
        for g in range(G):
            rows = np.array([t * W + g * Bg + j for t in range(T) for j in range(Bg)])
            b = _run(tab, rows, Bg, 1, 0.0, c, plain=True)
            np.testing.assert_array_equal(a["par"][rows], rows[b["par"]])
            for k in ("ext", "mod", "cum", "fin", "len"):
                np.testing.assert_array_equal(_bits(a[k][rows]), _bits(b[k]), err_msg=k)
            np.testing.assert_array_equal(_bits(a["aug"][rows]), _bits(b["cum"]))
            for k in range(2):                      # (the ancestry table's own-slot entry names the row: compared up to pos)
                np.testing.assert_array_equal(a["tout"][k][rows], b["tout"][k])
            np.testing.assert_array_equal(a["tout"][2][rows][:, :pos + 1], b["tout"][2][:, :pos + 1])


@pytest.mark.parametrize("W,G", [(2, 2), (3, 3), (4, 2), (6, 3), (8, 4), (8, 8)])
def test_a_large_penalty_makes_the_rows_pick_distinct_words(W, G):
    """(d) λ = 1e4 at the start, every row with ≥ W columns of positive probability besides UNK: with Bg = 1 the W rows of a sentence
    pick W distinct words; with Bg > 1 the words of different groups never coincide (the rows of one group extend one parent with
    different words anyway)"""
    rng = np.random.default_rng(W * 31 + G)
    T, C = 5, 65
    tab = _tables(rng, T, W, C, 0, False, False)
    tab["s"] = np.maximum(tab["s"], np.float32(1e-6))
    tab["cum"] = dbr.start_scores(T, W, G)
    tab["aug"] = tab["cum"].copy()
    got = _run(tab, np.arange(T * W), W, G, 1e4, dict())
    for t in range(T):
        words = got["ext"][t * W:(t + 1) * W].tolist()
        assert len(set(words)) == W, words


# ------------------------------------------------------------------------------------------------ (e)-(m) the translator
CTL = dict(block_ngram_repeat=1, min_length=3, length_penalty_name="avg")
LAM = 0.5
FIXTURES = [("tiny", "v"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")]
# The c1 configuration and weights (random draws: flat distributions, step margins of 1e-3 are typical) with the fixture's batch
# arguments and a batch seed under which the restatement has no near-tie at λ = 0.5, with and without CTL — with 7 sentences the cap
# allows none.  Searched on the CPU alone (the golden seed 2019 has 5 / 7 near-tie sentences on c1 v with CTL and 2 / 7 on c1 vivt;
# seeds 2019 … 2066 and 3000 … 4400 were tried, about 1 in 50 qualifies; these have the largest smallest margin found: 2.6e-4 and
# 2.0e-4).  The OOV batch: seed 78 (smallest margin 2.0e-3; 77 has one near-tie sentence of 9).
C1_SEED = {"v": 3784, "vivt": 2066}
OOV_SEED = 78
_MODELS, _REFS = {}, {}


def _translator(cfg, model, **kw):
    from svpc_amd.translator import Translator
    return Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, **kw)


def _fixture(golden_dir, case, mt):
    """(cfg, batch, model), built once per module; ``oov``: the tiny vivt weights on a batch with copied OOV words; ``c1``: the
    fixture's configuration, weights and batch arguments with the batch seed ``C1_SEED``"""
    if (case, mt) not in _MODELS:
        if case == "oov":
            _, cfg, _, model = _fixture_raw(golden_dir, "tiny", mt)
            batch = syn.make_batch(cfg, n_videos=3, max_steps=3, n_ingr=[3, 2, 3], n_oov=[2, 0, 3], seed=OOV_SEED, device=DEV)
        else:
            _, cfg, batch, model = _fixture_raw(golden_dir, case, mt)
            if case == "c1":
                from oracle.cases import CASES
                batch = syn.make_batch(cfg, device=DEV, **dict(CASES["c1"][1], seed=C1_SEED[mt]))
        _MODELS[(case, mt)] = (cfg, batch, model)
    return _MODELS[(case, mt)]


def _fixture_raw(golden_dir, case, mt):
    return build_model(case, mt, golden_dir, DEV)


def _ref(golden_dir, case, mt, W, G, lam, ctl=None):
    """the CPU restatement of one setting on one fixture: computed once, shared by the tests, never changed"""
    key = (case, mt, W, G, lam, tuple(sorted((ctl or {}).items())))
    if key not in _REFS:
        cfg, batch, model = _fixture(golden_dir, case, mt)
        P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        cpu = {k: ([t.cpu() for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor) else
                   (v.cpu() if isinstance(v, torch.Tensor) else v)) for k, v in batch.items()}
        _REFS[key] = dbr.diverse_decode(P, cfg, cpu["input_ids_list"], cpu["video_features_list"], cpu["input_masks_list"],
                                        cpu["ingr_input_ids"], cpu["ingr_sep_masks"], cpu["batch_step_num"], cpu["ingr_id_dict"],
                                        cpu["oov_word_dict"], W, G, lam, **(ctl or {}))
    return _REFS[key]


def _near_share(ref):
    """the restatement's own near-ties → (sentences under the margin, sentences)"""
    near = sum(int((np.nanmin(m, 1) <= TIE).sum()) for m in ref[3])
    return near, sum(m.shape[0] for m in ref[3])


def _compare(dec, scores, lens, ref, rows=None, bound=None, tie=TIE):
    """ids exactly, cum within rtol 1e-4 / atol 1e-6 (``test_beam_gpu._compare``'s bound; ``bound``: an absolute one instead), len exactly —
    except for sentences where the restatement itself shows a near-tie, which are counted → (near-ties met, worst |cum − restatement|).
    ``rows``: the columns of the restatement's (S_b, W, …) results the decode returned."""
    r_ids, r_cum, r_len, r_mg = ref
    near, worst = 0, 0.0
    for v, (d, s, ln) in enumerate(zip(dec, scores, lens)):
        d, s, ln = d.cpu(), s.cpu().numpy(), ln.cpu().numpy()
        sel = slice(None) if rows is None else rows
        assert d.dtype == torch.int64 and s.dtype == np.float32 and ln.dtype == np.int64
        for j in range(d.shape[0]):
            ri, rc, rl = r_ids[v][j][sel], r_cum[v][j][sel], r_len[v][j][sel]
            assert d[j].shape == ri.shape
            if torch.equal(d[j], ri):
                if bound is None:
                    np.testing.assert_allclose(s[j], rc, rtol=1e-4, atol=1e-6)
                else:
                    np.testing.assert_array_equal(np.isfinite(s[j]), np.isfinite(rc))
                    ok = np.isfinite(rc)
                    worst = max([worst] + np.abs(s[j][ok].astype(np.float64) - rc[ok]).tolist())
                np.testing.assert_array_equal(ln[j], rl)
                continue
            assert float(np.nanmin(r_mg[v][j])) <= tie, ("ids differ without a near-tie", d[j].tolist(), ri.tolist())
            near += 1
    return near, worst


@pytest.mark.parametrize("ctl", [False, True])
@pytest.mark.parametrize("case,mt", FIXTURES)
def test_translator_against_the_cpu_restatement(golden_dir, case, mt, ctl):
    """(e) W = 4, G = 2, λ = 0.5, with and without controls; also n_best = 1 (row 0 of every group) and the result's layout"""
    cfg, batch, model = _fixture(golden_dir, case, mt)
    c = CTL if ctl else {}
    ref = _ref(golden_dir, case, mt, 4, 2, LAM, c)
    near, _ = _near_share(ref)
    tr = _translator(cfg, model)
    dec, oov, sc, ln = tr.translate_batch_diverse(syn.translate_inputs(batch), 4, 2, LAM, **c)
    assert len(dec) == len(batch["batch_step_num"]) and all(d.shape[1:] == (4, cfg.max_t_len) for d in dec)
    assert _compare(dec, sc, ln, ref)[0] <= near
    d1, _, s1, l1 = tr.translate_batch_diverse(syn.translate_inputs(batch), 4, 2, LAM, 1, **c)
    for a, b, sa, sb, la, lb in zip(dec, d1, sc, s1, ln, l1):
        assert b.shape[1] == 2 and torch.equal(a[:, ::2], b) and torch.equal(sa[:, ::2], sb) and torch.equal(la[:, ::2], lb)


def test_translator_with_copied_oov_words(golden_dir):
    """(e) W = 6, G = 3 on the tiny vivt weights with copied OOV words"""
    cfg, batch, model = _fixture(golden_dir, "oov", "vivt")
    ref = _ref(golden_dir, "oov", "vivt", 6, 3, LAM)
    near, _ = _near_share(ref)
    tr = _translator(cfg, model)
    dec, _, sc, ln = tr.translate_batch_diverse(syn.translate_inputs(batch), 6, 3, LAM)
    assert _compare(dec, sc, ln, ref)[0] <= near
    V = cfg.vocab_size
    assert any(bool((d >= V).any()) for d in dec), "no copied word in any caption: the batch does not exercise the extended ids"


@pytest.mark.parametrize("case,mt,ctl", [(c, m, k) for c, m in FIXTURES for k in (False, True)] + [("oov", "vivt", False)])
def test_near_tie_cap_of_the_restatement(golden_dir, case, mt, ctl):
    """(e) the cap: at most 5 % of a fixture's sentences may be near-ties, asserted on the restatement alone.  Counted on the CPU at
    λ = 0.5 (near-ties / sentences): tiny v 0 / 5 and 0 / 5 with CTL, tiny vivt 0 / 5 and 0 / 5, c1 v (batch seed 3784) 0 / 7 and 0 / 7,
    c1 vivt (batch seed 2066) 0 / 7 and 0 / 7, the OOV batch 0 / 9."""
    W, G = (6, 3) if case == "oov" else (4, 2)
    near, n = _near_share(_ref(golden_dir, case, mt, W, G, LAM, CTL if ctl else {}))
    print("near-ties %s %s ctl %s: %d of %d sentences" % (case, mt, ctl, near, n))
    assert near <= NEAR_SHARE * n, "the restatement has %d near-ties among %d sentences" % (near, n)


@pytest.mark.parametrize("case,mt", FIXTURES)
def test_one_group_is_the_nbest_decode(golden_dir, case, mt):
    """(f) ``translate_batch_diverse(W, num_groups=1)`` = ``translate_batch_nbest(W, W)`` bit for bit, whatever λ; with controls too"""
    cfg, batch, model = _fixture(golden_dir, case, mt)
    tr = _translator(cfg, model)
    for c in ({}, CTL):
        a = tr.translate_batch_diverse(syn.translate_inputs(batch), 4, 1, LAM, **c)
        b = tr.translate_batch_nbest(syn.translate_inputs(batch), 4, 4, **c)
        for k in (0, 2, 3):
            for x, y in zip(a[k], b[k]):
                assert x.dtype == y.dtype and torch.equal(x, y)
    a = tr.translate_batch_diverse(syn.translate_inputs(batch), 4, 1, LAM, 2)
    b = tr.translate_batch_nbest(syn.translate_inputs(batch), 4, 2)
    assert all(torch.equal(x, y) for k in (0, 2, 3) for x, y in zip(a[k], b[k]))


@pytest.mark.parametrize("case,mt", FIXTURES)
def test_zero_strength_groups_are_the_narrow_nbest_decode(golden_dir, case, mt):
    """(g) λ = 0: every group's rows = ``translate_batch_nbest(Bg, Bg)`` under ``_compare``'s rule (decoder GEMMs over T·W rows instead
    of T·Bg may round differently: no bit equality), and the groups are copies of one another"""
    cfg, batch, model = _fixture(golden_dir, case, mt)
    tr = _translator(cfg, model)
    dec, _, sc, ln = tr.translate_batch_diverse(syn.translate_inputs(batch), 4, 2, 0.0)
    nd, _, ns, nl = tr.translate_batch_nbest(syn.translate_inputs(batch), 2, 2)
    ref = None
    for v in range(len(dec)):
        for g in range(2):
            for j in range(dec[v].shape[0]):
                rows = slice(2 * g, 2 * g + 2)
                if torch.equal(dec[v][j, rows], nd[v][j]):
                    np.testing.assert_allclose(sc[v][j, rows].cpu().numpy(), ns[v][j].cpu().numpy(), rtol=1e-4, atol=1e-6)
                    assert torch.equal(ln[v][j, rows], nl[v][j])
                    continue
                ref = ref or _ref(golden_dir, case, mt, 4, 2, 0.0)        # (only when a sentence differs: is it a near-tie?)
                assert float(np.nanmin(ref[3][v][j])) <= TIE, ("group rows differ from the narrow decode without a near-tie", v, j, g)


@pytest.mark.parametrize("case,mt", FIXTURES + [("oov", "vivt")])
def test_the_penalty_changes_captions(golden_dir, case, mt):
    """(h) the guard against a vacuous pass: λ = 0.5 changes at least one caption against λ = 0 on every fixture of (e)"""
    cfg, batch, model = _fixture(golden_dir, case, mt)
    W, G = (6, 3) if case == "oov" else (4, 2)
    tr = _translator(cfg, model)
    for c in ({},) if case == "oov" else ({}, CTL):
        a = tr.translate_batch_diverse(syn.translate_inputs(batch), W, G, LAM, **c)[0]
        b = tr.translate_batch_diverse(syn.translate_inputs(batch), W, G, 0.0, **c)[0]
        assert any(not torch.equal(x, y) for x, y in zip(a, b)), "λ changed no caption: the tests of (e) would pass vacuously"
        Bg = W // G
        assert all(torch.equal(y[:, :Bg], y[:, g * Bg:(g + 1) * Bg]) for y in b for g in range(G))       # λ = 0: identical groups


@pytest.mark.parametrize("case,mt", FIXTURES)
def test_score_captions_reproduces_the_model_score(golden_dir, case, mt):
    """(i) forced scoring of the returned rows gives the returned cum (``test_forced_score_gpu``'s bound: rtol 1e-4 / atol 1e-6) and
    lengths, rows that pick PAD as a word excepted: cum stayed the model's score and did not pick up the penalties"""
    cfg, batch, model = _fixture(golden_dir, case, mt)
    tr = _translator(cfg, model)
    dec, _, sc, ln = tr.translate_batch_diverse(syn.translate_inputs(batch), 4, 2, LAM, **CTL)
    got = tr.score_captions(syn.translate_inputs(batch), dec)
    checked = 0
    for b, (ids, n) in enumerate(zip(dec, ln)):
        pos = torch.arange(ids.shape[-1], device=ids.device)
        ok = ~((ids == PAD) & (pos >= 1) & (pos <= n.unsqueeze(-1))).any(-1) & torch.isfinite(sc[b])
        ok = ok.cpu().numpy()
        np.testing.assert_allclose(got.score_list[b].cpu().numpy()[ok], sc[b].cpu().numpy()[ok], rtol=1e-4, atol=1e-6)
        np.testing.assert_array_equal(got.length_list[b].cpu().numpy()[ok], n.cpu().numpy()[ok])
        checked += int(ok.sum())
    assert checked >= 0.5 * sum(d.shape[0] * d.shape[1] for d in dec)


@pytest.mark.parametrize("case,mt", [("tiny", "vivt"), ("c1", "vivt")])
def test_graph_replay_equals_eager_and_settings_have_their_own_plans(golden_dir, case, mt):
    """(j), (l)"""
    cfg, batch, model = _fixture(golden_dir, case, mt)
    eager, graphed = _translator(cfg, model), _translator(cfg, model, graph=True)
    for W, G, lam in ((4, 2, LAM), (4, 4, 1.0)):
        e = eager.translate_batch_diverse(syn.translate_inputs(batch), W, G, lam, **CTL)
        e2 = eager.translate_batch_diverse(syn.translate_inputs(batch), W, G, lam, **CTL)
        for k in (0, 2, 3):                              # determinism over two calls
            assert all(torch.equal(a, b) for a, b in zip(e[k], e2[k]))
        for _ in range(2):                               # capture, then replay
            g = graphed.translate_batch_diverse(syn.translate_inputs(batch), W, G, lam, **CTL)
            for k in (0, 2, 3):
                assert all(torch.equal(a, b) for a, b in zip(e[k], g[k]))
    graphed.translate_batch_diverse(syn.translate_inputs(batch), 4, 2, 0.25, **CTL)          # another λ: another plan
    graphed.translate_batch_diverse(syn.translate_inputs(batch), 4, 2, LAM, 1, **CTL)        # another n_best: the same plan
    assert len(graphed._preps) == 3 and all(p.graphs for p in graphed._preps.values())
    assert len(eager._preps) == 2


@pytest.mark.parametrize("case", ["tiny", "c1"])
def test_consensus_over_diverse_candidates(golden_dir, case):
    """(k) ``translate_batch_consensus(source="diverse")`` = ``consensus`` applied by hand to ``translate_batch_diverse``'s rows"""
    from test_consensus_gpu import SPECIAL, Case
    from svpc_amd.synthetic import IGNORE
    cfg, batch, model = _fixture(golden_dir, case, "vivt")
    Vm, N = cfg.vocab_size, len(batch["batch_step_num"])
    i2w = SPECIAL + ["".join(chr(97 + (i // 26 ** k) % 26) for k in range(3)) for i in range(7, Vm)]
    refs, videos = {}, []
    for b in range(N):
        inv = {int(v): k for k, v in batch["oov_word_dict"][b].items()}
        sents = []
        for s in range(int(batch["batch_step_num"][b])):
            lab = batch["input_labels_list"][s][b].cpu().tolist()
            sents.append(" ".join(i2w[x] if x < Vm else inv[x] for x in lab if x not in (IGNORE, EOS, PAD)))
        refs["vid%d" % b] = [" ".join(sents)]
        videos.append(dict(oov=batch["oov_word_dict"][b]))
    plan = Case(i2w, refs).plan(videos)
    tr = _translator(cfg, model)
    for scope, weights, K, G, beam in (("paragraph", "uniform", 4, 2, None), ("sentence", "posterior", 3, 3, 6)):
        kw = dict(beam_size=beam) if beam else {}
        W = beam or K
        dec, _, sc, ln = tr.translate_batch_diverse(syn.translate_inputs(batch), W, G, LAM, K // G)
        assert all(d.shape[1] == K for d in dec)
        by_hand = tr.consensus(dec, plan, sc, ln, "CIDEr", scope, weights)
        got, oov, picks = tr.translate_batch_consensus(syn.translate_inputs(batch), plan, source="diverse", num_candidates=K, num_groups=G,
                                                       diversity_strength=LAM, scope=scope, weights=weights, **kw)
        assert len(oov) == N
        for b in range(N):
            assert torch.equal(got[b], by_hand.dec_seq_list[b]) and torch.equal(picks[b], by_hand.pick_list[b])
    with pytest.raises(ValueError):
        tr.translate_batch_consensus(syn.translate_inputs(batch), plan, source="greedy")


def test_bf16x3_deviation_at_config_1(golden_dir):
    """(m) bf16x3 on c1 against the fp32 CPU restatement: the sentences whose ids agree keep |cum − restatement| ≤ BOUND_X3; those whose
    ids disagree fall under the near-tie rule.  The measured worst deviation is written to the report directory
    (profiles/diverse_beam_parity.json is the committed copy)."""
    worst = {}
    for mt in ("v", "vivt"):
        cfg, batch, model = _fixture(golden_dir, "c1", mt)
        ref = _ref(golden_dir, "c1", mt, 4, 2, LAM)
        ops.set_precision("bf16x3")
        try:
            _, _, _, model_x3 = build_model("c1", mt, golden_dir, DEV)          # (the same weights; its weight store gets the mode's lo plane)
            dec, _, sc, ln = _translator(cfg, model_x3).translate_batch_diverse(syn.translate_inputs(batch), 4, 2, LAM)
            torch.cuda.synchronize()
        finally:
            ops.set_precision("fp32")
        worst[mt + "_ids_differ"], worst[mt] = _compare(dec, sc, ln, ref, bound=True)      # (ids may differ only at a near-tie)
        assert worst[mt + "_ids_differ"] <= NEAR_SHARE * _near_share(ref)[1], worst          # … and on at most 5 % of the sentences
    print("bf16x3 c1 diverse: worst |cum - restatement| = %s" % json.dumps(worst))
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "diverse_beam_parity.json"), "w") as f:
        json.dump(dict(case="c1", precision="bf16x3", beam=4, groups=2, strength=LAM, worst_abs_cum_deviation=worst, bound=BOUND_X3), f, indent=1)
    assert max(worst["v"], worst["vivt"]) <= BOUND_X3, worst
