"""Lexically constrained beam search on the MI355X: the selection kernel (svpc_beam_step_cons) and the final pick
(svpc_beam_finalize_cons) against tests/constrained_beam_reference.py bit for bit, against ``ops.beam_step`` / ``ops.beam_finalize_nbest``
where they must coincide (no constraints; equal states), and ``Translator.translate_batch_constrained`` against the CPU restatement built
on the oracle's decoder blocks (fp32 goldens), against ``translate_batch_nbest``, ``score_captions``, replayed against eager, and under
bf16x3.

Every sentence's constraints come from its gold caption: the bigram at caption positions 1–2 and the word at position 4, special ids
(and ids the video cannot generate) dropped.  Near-ties (the project's rule of §11.7 – §11.9): a sentence whose restatement shows a key gap
≤ 1e-4 at a bank's kept / dropped boundary at any step, or between the final keys of consecutive rows of equal popcount, may decode
differently; at most 5 % of a fixture's sentences may be such, asserted on the restatement alone
(``test_near_tie_cap_of_the_restatement``).  The batch seeds of the ``c1`` cases and of the OOV batch were chosen on the CPU, from the
restatement alone, so that the cap holds (``C1_SEED``, ``OOV_SEED``)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import constrained_beam_reference as cbr  # noqa: E402
from diverse_beam_reference import length_table  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import ops, synthetic as syn  # noqa: E402
from svpc_amd.ops_common import Idx  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, IGNORE, PAD, UNK  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = type("O", (), {"cuda": True})
TIE = 1e-4
NEAR_SHARE = 0.05
REPORT_DIR = os.environ.get("SVPC_REPORT_DIR") or os.path.join(ROOT, "reports")
# bf16x3 at the config-1 shape: the worst |cum − fp32 CPU restatement| over the sentences whose ids agree, measured on the MI355X
# (profiles/constrained_beam_parity.json); the assertion is at twice that, as in §11.9 and §11.10.
MEASURED_X3 = 0.0005092620849609375          # ("c1", "vivt"); ("c1", "v"): 0.00037; cum there is about −40 … −95
BOUND_X3 = 2.0 * MEASURED_X3

# ------------------------------------------------------------------------------------------------ (a)-(c) the kernels
WIDTHS = [1, 2, 3, 4, 6, 8]
COLS = [7, 64, 65, 951, 4097, "mixed"]             # (C = 7: three ordinary words per live row, fewer than W = 8)
LT = 12
MID = 6
SETTINGS = [dict(), dict(block_ngram_repeat=1), dict(block_ngram_repeat=2, exclusion_tokens=(2,)), dict(min_length=MID + 1),
            dict(length_penalty_name="wu", length_penalty_alpha=0.7),
            dict(block_ngram_repeat=2, exclusion_tokens=(3,), min_length=MID + 1, length_penalty_name="avg")]
HOT = [1, 2, 3]                                     # words every C ≥ 7 has; the scores rank them (and EOS) first


def _phrases(rng, C, X, M):
    """M phrases of lengths 1 … 4 for a sentence of C columns: hot words (forced columns inside the top-W), other columns (outside it),
    the last copied-word column, now and then an id the rows do not have (≥ C) — and duplicates"""
    out = []
    for j in range(M):
        n = int(rng.integers(1, 5)) if M < 4 else j + 1          # (M = 4: lengths 1, 2, 3, 4)
        pool = list(HOT) + ([int(v) for v in rng.integers(7, C, size=3)] if C > 7 else []) + ([C - 1] if X else [])
        ph = [int(pool[int(rng.integers(0, len(pool)))]) for _ in range(n)]
        if rng.random() < 0.1:
            ph[0] = C + 1
        if out and rng.random() < 0.25:
            ph = list(out[int(rng.integers(0, len(out)))])
        out.append(tuple(ph))
    return out


def _state(rng, phrases, mid):
    """a valid tracker state: at the start 0; at a middle position a random met mask and, sometimes, a phrase in progress"""
    if not mid or not phrases:
        return 0
    met = int(rng.integers(0, 1 << len(phrases)))
    open_ = [j for j, ph in enumerate(phrases) if not (met >> j) & 1 and len(ph) > 1]
    if open_ and rng.random() < 0.5:
        j = open_[int(rng.integers(0, len(open_)))]
        return cbr.pack(met, j, int(rng.integers(1, len(phrases[j]))))
    return cbr.pack(met, -1, 0)


def _tables(rng, T, W, C, pos, logits, adversarial):
    """scores / row_c / row_x / cum / cstate / finished / length / extended-id history of T sentences × W rows, and their constraints:
    M ∈ {0, 1, 2, 4} mixed over the sentences.  One C per sentence ("mixed": another C for every sentence of the launch), copied-word
    columns, histories over the hot words (so bans bite), at a middle position phrases in progress, finished rows and −inf rows;
    adversarial: rows of few distinct values (ties, zero probabilities), a row of zero probabilities / equal logits.  In probabilities
    mode the first ids of some phrases get a very low (1e-30) or zero probability in some rows."""
    Cs = rng.integers(UNK + 2, 700, size=T) if C == "mixed" else np.full(T, C)
    if C == "mixed":
        Cs[0] = 7
    Xs = np.array([rng.integers(0, min(4, c - UNK - 1)) if c > UNK + 2 else 0 for c in Cs])
    cmax, R = int(Cs.max()), T * W
    if adversarial:
        vals = np.array([0.0, 0.125, 0.25, 0.5] if not logits else [-3.0, -1.0, 0.0, 2.0], np.float32)
        s = vals[rng.integers(0, len(vals), size=(R, cmax))]
        s[:, HOT + [EOS]] = vals[-2:][rng.integers(0, 2, size=(R, 4))]
    else:
        s = (rng.random((R, cmax)) ** 4).astype(np.float32) if not logits else (rng.standard_normal((R, cmax)) * 3).astype(np.float32)
        base = rng.uniform(0.3, 0.6, size=(T, 4)) if not logits else rng.uniform(4.0, 7.0, size=(T, 4))
        s[:, HOT + [EOS]] = (np.repeat(base, W, 0) + rng.uniform(0, 0.05, size=(R, 4))).astype(np.float32)
    Ms = [[0, 1, 2, 4][(t + int(rng.integers(0, 4))) % 4] if T > 1 else [1, 2, 4, 0][int(rng.integers(0, 4))] for t in range(T)]
    cons = [_phrases(rng, int(Cs[t]), int(Xs[t]), Ms[t]) for t in range(T)]
    hist = np.full((R, LT), PAD, np.int64)
    hist[:, 0] = BOS
    hist[:, 1:pos + 1] = rng.choice(HOT, size=(R, pos))
    state = np.array([_state(rng, cons[r // W], pos > 0) for r in range(R)], np.int32)
    for r in range(R):
        c = int(Cs[r // W])
        for ph in cons[r // W]:
            u = rng.random()
            if not logits and ph[0] < c and u < 0.3:
                s[r, ph[0]] = 1e-30 if u < 0.15 else 0.0
    if adversarial:
        s[R // 2] = 0.0
    s[:, UNK] = 1.0 if not logits else 50.0         # UNK would win every comparison were it a candidate
    if pos == 0:
        cum = np.zeros((T, W), np.float32)
        if not adversarial:
            cum[:, 1:] = -np.inf                    # the decode's start: beam 0 alone (adversarial: every row alive)
        cum = cum.reshape(-1)
        fin, length = np.zeros(R, np.int32), np.zeros(R, np.int32)
    else:
        cum = (-rng.random(R) * 5).astype(np.float32)
        if adversarial:
            cum = np.array([-1.0, -0.5, 0.0], np.float32)[rng.integers(0, 3, size=R)]
        dead = rng.random(R) < 0.15
        cum[dead] = -np.inf
        fin = ((rng.random(R) < 0.3) | dead).astype(np.int32) if not adversarial else (rng.random(R) < 0.3).astype(np.int32)
        length = np.where(fin, rng.integers(1, pos + 1, size=R), 0).astype(np.int32)
    return dict(s=s, row_c=np.repeat(Cs, W), row_x=np.repeat(Xs, W), cum=cum, state=state, fin=fin, length=length, hist=hist, pos=pos, T=T,
                W=W, logits=logits, cons=cons, tin=[rng.integers(0, 1000, size=(R, LT)).astype(np.int32), hist.astype(np.int32),
                                                    rng.integers(0, 1000, size=(R, LT)).astype(np.int32)])


def _kernel_args(c, V):
    excl = (ops.exclusion_bitmap(c["exclusion_tokens"], V, DEV), V) if c.get("exclusion_tokens") else None
    lp_host = length_table(c.get("length_penalty_name", "none"), c.get("length_penalty_alpha", 0.0), LT)
    lp = torch.tensor(lp_host, dtype=torch.float64, device=DEV) if lp_host is not None else None
    return dict(min_length=c.get("min_length", 0), block_ngram_repeat=c.get("block_ngram_repeat", 0), exclusion=excl, lp=lp), lp_host


def _bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _run(tab, W, c, plain=False):
    """the kernel on a table (``plain``: ``ops.beam_step`` with controls instead) → numpy outputs"""
    kw, _ = _kernel_args(c, 700)
    R = tab["T"] * W
    sd = torch.from_numpy(np.ascontiguousarray(tab["s"])).to(DEV)
    cum_d, st_d, fin_d, len_d = (torch.from_numpy(tab[k].copy()).to(DEV) for k in ("cum", "state", "fin", "length"))
    t_in = [torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in tab["tin"]]
    t_out = [torch.full((R, LT), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
    rc, rx = Idx(tab["row_c"].tolist()), Idx(tab["row_x"].tolist())
    if plain:
        par, ext, mod = ops.beam_step(sd, rc, rx, W, tab["pos"], tab["logits"], UNK, EOS, PAD, cum_d, fin_d, t_in, t_out, LT, length=len_d, **kw)
    else:
        cons_d = torch.from_numpy(cbr.table(tab["cons"])).to(DEV)
        par, ext, mod = ops.beam_step_cons(sd, rc, rx, W, tab["pos"], tab["logits"], UNK, EOS, PAD, cum_d, st_d, fin_d, len_d, t_in, t_out, LT,
                                           cons_d, **kw)
    torch.cuda.synchronize()
    return dict(par=par.cpu().numpy(), ext=ext.cpu().numpy(), mod=mod.cpu().numpy(), cum=cum_d.cpu().numpy(), state=st_d.cpu().numpy(),
                fin=fin_d.cpu().numpy(), len=len_d.cpu().numpy(), tout=[t.cpu().numpy() for t in t_out])


def _restatement(tab, W, c):
    _, lp_host = _kernel_args(c, 700)
    return cbr.select_cons(tab["s"], tab["row_c"], tab["row_x"], W, tab["logits"], tab["cum"], tab["state"], tab["fin"].astype(bool),
                           tab["length"], tab["hist"], tab["pos"], tab["cons"], min_length=c.get("min_length", 0),
                           block_ngram_repeat=c.get("block_ngram_repeat", 0), exclusion_tokens=c.get("exclusion_tokens", ()), lp=lp_host)


def _against_restatement(tab, W, c, what):
    T, pos = tab["T"], tab["pos"]
    R = T * W
    got = _run(tab, W, c)
    r_par, r_ext, r_mod, r_cum, r_st, r_fin, r_len = _restatement(tab, W, c)
    np.testing.assert_array_equal(got["par"], r_par, err_msg=what)
    np.testing.assert_array_equal(got["ext"], r_ext, err_msg=what)
    np.testing.assert_array_equal(got["mod"], r_mod, err_msg=what)
    np.testing.assert_array_equal(_bits(got["cum"]), _bits(r_cum), err_msg=what)
    np.testing.assert_array_equal(got["state"], r_st, err_msg=what)
    np.testing.assert_array_equal(got["fin"].astype(bool), r_fin, err_msg=what)
    np.testing.assert_array_equal(got["len"], r_len, err_msg=what)
    for k in range(3):
        np.testing.assert_array_equal(got["tout"][k][:, :pos + 1], tab["tin"][k][r_par, :pos + 1], err_msg=what)
        assert np.all(got["tout"][k][:, pos + 2:] == -7)
    np.testing.assert_array_equal(got["tout"][0][:, pos + 1], r_mod)
    np.testing.assert_array_equal(got["tout"][1][:, pos + 1], r_ext)
    np.testing.assert_array_equal(got["tout"][2][:, pos + 1], np.arange(R) * LT + pos + 1)
    return got


def _cases(W, logits):
    """every C at the start and at a middle position; T, the control setting and the kind of rows rotate so that each (W, mode) meets
    every C with both positions, and over the 12 (W, mode) all combinations come up"""
    off = WIDTHS.index(W) * 2 + int(logits)
    for i, (C, pos) in enumerate((C, pos) for C in COLS for pos in (0, MID)):
        T = 1 if (C == 4097 or (i + off) % 4 == 0) and C != "mixed" else 5
        yield C, pos, T, SETTINGS[(i + off) % len(SETTINGS)], (i // 2 + off) % 2 == 1


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("W", WIDTHS)
def test_kernel_equals_the_restatement(W, logits):
    """(a) everything bit for bit; last, fill rows: C = 7 with unigram blocking and a minimum length leaves a row that has used words 0 … 4
    without a candidate, so a sentence of such rows (all live, finite cum) has none at all"""
    rng = np.random.default_rng(2000 * W + logits)
    forced, moved = 0, 0
    for C, pos, T, c, adversarial in _cases(W, logits):
        tab = _tables(rng, T, W, C, pos, logits, adversarial)
        got = _against_restatement(tab, W, c, "C %s pos %d T %d %s adversarial %s" % (C, pos, T, c, adversarial))
        forced += int(np.sum((got["state"] != 0) & (got["fin"] == 0)))
        free = dict(tab, cons=[[] for _ in range(T)], state=np.zeros(T * W, np.int32))
        moved += int(np.sum(got["ext"] != _restatement(free, W, c)[1]))
    assert forced > 0 and moved > 0, "the constraints never changed a pick: the tables do not exercise them"
    tab = _tables(rng, 5, W, 7, MID, logits, False)
    starved = np.arange(5 * W) < W + (W + 1) // 2            # sentence 0 and the first rows of sentence 1
    tab["hist"][starved, 1:MID + 1] = [0, 1, 2, 3, 4, 0]
    tab["tin"][1] = tab["hist"].astype(np.int32)
    tab["fin"][starved], tab["length"][starved] = 0, 0
    tab["cum"][starved] = -1.0
    tab["cons"][0] = [(1,), (2, 3)]
    tab["state"][:W] = 0
    got = _against_restatement(tab, W, dict(block_ngram_repeat=1, min_length=MID + 1), "fill rows")
    np.testing.assert_array_equal(got["par"][:W], np.arange(W))
    assert np.all(got["ext"][:W] == PAD) and np.all(np.isneginf(got["cum"][:W])) and np.all(got["state"][:W] == 0)
    assert np.all(got["fin"][:W] == 1) and np.all(got["len"][:W] == MID + 1)


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("W", WIDTHS)
def test_no_constraints_equals_beam_step(W, logits):
    """(b) M = 0 everywhere: ``ops.beam_step`` with controls on the same inputs, bit for bit, and every state stays 0"""
    rng = np.random.default_rng(88 * W + logits)
    for i, (C, pos) in enumerate((C, pos) for C in (7, 65, 951, "mixed") for pos in (0, MID)):
        tab = _tables(rng, 5, W, C, pos, logits, i % 2 == 1)
        tab["cons"], tab["state"] = [[] for _ in range(5)], np.zeros(5 * W, np.int32)
        c = SETTINGS[(i + W) % len(SETTINGS)]
        a, b = _run(tab, W, c), _run(tab, W, c, plain=True)
        for k in ("par", "ext", "mod", "cum", "fin", "len"):
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)
        assert not a["state"].any()
        for x, y in zip(a["tout"], b["tout"]):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("lp_name", ["none", "avg", "wu"])
@pytest.mark.parametrize("W", WIDTHS)
def test_finalize_equals_the_restatement(W, lp_name):
    """(c) the final order: popcount, key, index; −inf rows last; with all states equal it is ``beam_finalize_nbest``"""
    rng = np.random.default_rng(W * 7 + len(lp_name))
    T = 37
    R = T * W
    lp_host = length_table(lp_name, 0.8, LT)
    lp = torch.tensor(lp_host, dtype=torch.float64, device=DEV) if lp_host is not None else None
    cum = np.array([-4.0, -2.0, -1.0, -0.5], np.float32)[rng.integers(0, 4, size=R)]          # few values: ties
    cum[rng.random(R) < 0.2] = -np.inf
    cum[:W] = -np.inf                                                                     # a sentence of −inf rows
    length = rng.integers(1, LT, size=R).astype(np.int32)
    state = np.array([cbr.pack(int(rng.integers(0, 16)), int(rng.integers(-1, 4)), int(rng.integers(0, 4))) for _ in range(R)], np.int32)
    ext = rng.integers(0, 900, size=(R, LT)).astype(np.int32)
    cum_d, len_d, ext_d = (torch.from_numpy(v).to(DEV) for v in (cum, length, ext))
    for st in (state, np.full(R, cbr.pack(0b0101, 1, 1), np.int32)):
        st_d = torch.from_numpy(st).to(DEV)
        for nb in sorted({1, W, (W + 1) // 2}):
            ids, sc, ln, met = (v.cpu().numpy() for v in ops.beam_finalize_cons(cum_d, ext_d, W, nb, st_d, len_d, lp))
            for t in range(T):
                lo = t * W
                order, _ = cbr.final_order_cons(cum[lo:lo + W], length[lo:lo + W], st[lo:lo + W], lp_host)
                rows = [lo + h for h in order[:nb]]
                np.testing.assert_array_equal(ids[t], ext[rows])
                np.testing.assert_array_equal(_bits(sc[t]), _bits(cum[rows]))
                np.testing.assert_array_equal(ln[t], length[rows])
                np.testing.assert_array_equal(met[t], st[rows] & 15)
        i2, s2, l2 = ops.beam_finalize_nbest(cum_d, ext_d, W, W, len_d, lp)
        torch.cuda.synchronize()
        if st is not state:                          # (the last ``st``: all states equal)
            ids, sc, ln, met = ops.beam_finalize_cons(cum_d, ext_d, W, W, st_d, len_d, lp)
            assert torch.equal(ids, i2) and torch.equal(sc.view(torch.int32), s2.view(torch.int32)) and torch.equal(ln, l2)
            assert bool((met == 0b0101).all())


# ------------------------------------------------------------------------------------------------ (d)-(j) the translator
CTL = dict(block_ngram_repeat=1, min_length=3, length_penalty_name="avg")
FIXTURES = [("tiny", "v"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")]
# The c1 configuration and weights with the fixture's batch arguments and a batch seed under which the restatement stays within the cap
# with these constraints, with and without CTL (with 7 sentences the cap allows no near-tie); the OOV batch likewise.  Searched on the
# CPU alone, from the restatement alone (DESIGN §11.11 has the counts).
C1_SEED = {"v": 3311, "vivt": 3061}
OOV_SEED = 78
_MODELS, _REFS = {}, {}
SPECIAL = (PAD, BOS, EOS, UNK, IGNORE)


def _translator(cfg, model, **kw):
    from svpc_amd.translator import Translator
    return Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, **kw)


def _fixture(golden_dir, case, mt):
    """(cfg, batch, model), built once per module; ``oov``: the tiny vivt weights on a batch with copied OOV words; ``c1``: the
    fixture's configuration, weights and batch arguments with the batch seed ``C1_SEED``"""
    if (case, mt) not in _MODELS:
        if case == "oov":
            _, cfg, _, model = build_model("tiny", mt, golden_dir, DEV)
            batch = syn.make_batch(cfg, n_videos=3, max_steps=3, n_ingr=[3, 2, 3], n_oov=[2, 0, 3], seed=OOV_SEED, device=DEV)
        else:
            _, cfg, batch, model = build_model(case, mt, golden_dir, DEV)
            if case == "c1":
                from oracle.cases import CASES
                batch = syn.make_batch(cfg, device=DEV, **dict(CASES["c1"][1], seed=C1_SEED[mt]))
        _MODELS[(case, mt)] = (cfg, batch, model)
    return _MODELS[(case, mt)]


def gold_constraints(cfg, batch, oov=False, other=False):
    """per video, per sentence: the bigram at caption positions 1–2 and the word at position 4 of the gold caption (the label at text
    position j is the word at caption position j + 1), ids that are special or that the video cannot generate (≥ C_b) dropped, empty
    phrases dropped.  ``oov``: videos with copied words take their first copied id (V) as the single word instead.  ``other``: another
    set for the same batch — the word at position 3 and the bigram at positions 5–6."""
    Lv, V = cfg.max_v_len, cfg.vocab_size
    out = []
    for b, S_b in enumerate(batch["batch_step_num"]):
        C_b = V + (len(batch["oov_word_dict"][b]) if cfg.model_mode != "video" else 0)
        per_video = []
        for s in range(S_b):
            lab = batch["input_labels_list"][s][b].cpu().tolist()
            word = lambda p: int(lab[Lv + p - 1])
            groups = [[word(1), word(2)], [word(4)]] if not other else [[word(3)], [word(5), word(6)]]
            if oov and C_b > V:
                groups[1] = [V]
            phrases = [tuple(w for w in g if w not in SPECIAL and 0 <= w < C_b) for g in groups]
            per_video.append([ph for ph in phrases if ph])
        out.append(per_video)
    return out


def _ref(golden_dir, case, mt, W, ctl=None, other=False):
    """the CPU restatement of one setting on one fixture: computed once, shared by the tests, never changed"""
    key = (case, mt, W, tuple(sorted((ctl or {}).items())), other)
    if key not in _REFS:
        cfg, batch, model = _fixture(golden_dir, case, mt)
        P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        cpu = {k: ([t.cpu() for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor) else
                   (v.cpu() if isinstance(v, torch.Tensor) else v)) for k, v in batch.items()}
        _REFS[key] = cbr.constrained_decode(P, cfg, cpu["input_ids_list"], cpu["video_features_list"], cpu["input_masks_list"],
                                            cpu["ingr_input_ids"], cpu["ingr_sep_masks"], cpu["batch_step_num"], cpu["ingr_id_dict"],
                                            cpu["oov_word_dict"], W, gold_constraints(cfg, batch, oov=case == "oov", other=other),
                                            **(ctl or {}))
    return _REFS[key]


def _near_share(ref):
    """the restatement's own near-ties → (sentences under the margin, sentences)"""
    near = sum(int((np.nanmin(m, 1) <= TIE).sum()) for m in ref[4])
    return near, sum(m.shape[0] for m in ref[4])


def _compare(dec, scores, lens, mets, ref, bound=None):
    """ids, len and met exactly, cum within rtol 1e-4 / atol 1e-6 (``bound``: the absolute deviation is measured instead) — except for
    sentences where the restatement itself shows a near-tie, which are counted → (near-ties met, worst |cum − restatement|)"""
    r_ids, r_cum, r_len, r_met, r_mg = ref
    near, worst = 0, 0.0
    for v, (d, s, ln, mt_) in enumerate(zip(dec, scores, lens, mets)):
        d, s, ln, mt_ = d.cpu(), s.cpu().numpy(), ln.cpu().numpy(), mt_.cpu().numpy()
        assert d.dtype == torch.int64 and s.dtype == np.float32 and ln.dtype == np.int64 and mt_.dtype == np.int64
        for j in range(d.shape[0]):
            assert d[j].shape == r_ids[v][j].shape
            if torch.equal(d[j], r_ids[v][j]):
                if bound is None:
                    np.testing.assert_allclose(s[j], r_cum[v][j], rtol=1e-4, atol=1e-6)
                else:
                    np.testing.assert_array_equal(np.isfinite(s[j]), np.isfinite(r_cum[v][j]))
                    ok = np.isfinite(r_cum[v][j])
                    worst = max([worst] + np.abs(s[j][ok].astype(np.float64) - r_cum[v][j][ok]).tolist())
                np.testing.assert_array_equal(ln[j], r_len[v][j])
                np.testing.assert_array_equal(mt_[j], r_met[v][j])
                continue
            assert float(np.nanmin(r_mg[v][j])) <= TIE, ("ids differ without a near-tie", d[j].tolist(), r_ids[v][j].tolist())
            near += 1
    return near, worst


@pytest.mark.parametrize("ctl", [False, True])
@pytest.mark.parametrize("case,mt", FIXTURES)
def test_translator_against_the_cpu_restatement(golden_dir, case, mt, ctl):
    """(d) W = 4, with and without controls; also n_best = 2 (the first two rows) and the result's layout"""
    cfg, batch, model = _fixture(golden_dir, case, mt)
    c = CTL if ctl else {}
    ref = _ref(golden_dir, case, mt, 4, c)
    near, _ = _near_share(ref)
    tr = _translator(cfg, model)
    cons = gold_constraints(cfg, batch)
    dec, oov, sc, ln, met = tr.translate_batch_constrained(syn.translate_inputs(batch), cons, 4, **c)
    assert len(dec) == len(batch["batch_step_num"]) and all(d.shape[1:] == (4, cfg.max_t_len) for d in dec)
    assert _compare(dec, sc, ln, met, ref)[0] <= near
    d2, _, s2, l2, m2 = tr.translate_batch_constrained(syn.translate_inputs(batch), cons, 4, 2, **c)
    for a, b in zip(dec + sc + ln + met, d2 + s2 + l2 + m2):
        assert b.shape[1] == 2 and torch.equal(a[:, :2], b)


def test_translator_with_a_copied_oov_phrase(golden_dir):
    """(d) the tiny vivt weights on a batch with copied OOV words: the videos that have copied words must say their first one"""
    cfg, batch, model = _fixture(golden_dir, "oov", "vivt")
    ref = _ref(golden_dir, "oov", "vivt", 4)
    near, _ = _near_share(ref)
    tr = _translator(cfg, model)
    cons = gold_constraints(cfg, batch, oov=True)
    V = cfg.vocab_size
    assert sum(1 for per_video in cons for phrases in per_video if (V,) in phrases) >= 4
    dec, _, sc, ln, met = tr.translate_batch_constrained(syn.translate_inputs(batch), cons, 4)
    assert _compare(dec, sc, ln, met, ref)[0] <= near
    for d, per_video in zip(dec, cons):
        for j, phrases in enumerate(per_video):
            if (V,) in phrases:
                assert V in d[j, 0].tolist()


@pytest.mark.parametrize("case,mt,ctl", [(c, m, k) for c, m in FIXTURES for k in (False, True)] + [("oov", "vivt", False)])
def test_near_tie_cap_of_the_restatement(golden_dir, case, mt, ctl):
    """(d) the cap: at most 5 % of a fixture's sentences may be near-ties, asserted on the restatement alone (DESIGN §11.11 has the
    counts per fixture)"""
    near, n = _near_share(_ref(golden_dir, case, mt, 4, CTL if ctl else {}))
    print("near-ties %s %s ctl %s: %d of %d sentences" % (case, mt, ctl, near, n))
    assert near <= NEAR_SHARE * n, "the restatement has %d near-ties among %d sentences" % (near, n)


@pytest.mark.parametrize("case,mt", FIXTURES)
def test_no_constraints_is_the_nbest_decode(golden_dir, case, mt):
    """(e) all-empty constraints = ``translate_batch_nbest(W, W)`` bit for bit, with controls too; every mask is 0"""
    cfg, batch, model = _fixture(golden_dir, case, mt)
    tr = _translator(cfg, model)
    none = [[None] * int(s) for s in batch["batch_step_num"]]
    empty = [[[] for _ in range(int(s))] for s in batch["batch_step_num"]]
    for c, cons in (({}, none), (CTL, empty)):
        a = tr.translate_batch_constrained(syn.translate_inputs(batch), cons, 4, **c)
        b = tr.translate_batch_nbest(syn.translate_inputs(batch), 4, 4, **c)
        for k in (0, 2, 3):
            for x, y in zip(a[k], b[k]):
                assert x.dtype == y.dtype and torch.equal(x, y)
        assert all(not bool(m.any()) for m in a[4])


@pytest.mark.parametrize("case,mt", FIXTURES + [("oov", "vivt")])
def test_row_zero_says_every_phrase(golden_dir, case, mt):
    """(f) every sentence's row 0 has the full mask and holds each phrase as a contiguous run (a plain search); the constraints change
    at least one caption against the unconstrained decode"""
    cfg, batch, model = _fixture(golden_dir, case, mt)
    tr = _translator(cfg, model)
    cons = gold_constraints(cfg, batch, oov=case == "oov")
    assert sum(len(p) for per_video in cons for p in per_video) > 0
    for c in ({},) if case == "oov" else ({}, CTL):
        dec, _, sc, ln, met = tr.translate_batch_constrained(syn.translate_inputs(batch), cons, 4, **c)
        free = tr.translate_batch_nbest(syn.translate_inputs(batch), 4, 4, **c)[0]
        for d, m, per_video in zip(dec, met, cons):
            for j, phrases in enumerate(per_video):
                assert int(m[j, 0]) == (1 << len(phrases)) - 1, (case, mt, j, phrases, int(m[j, 0]))
                ids = d[j, 0].tolist()
                for ph in phrases:
                    assert any(ids[i:i + len(ph)] == list(ph) for i in range(len(ids))), (ids, ph)
        assert any(not torch.equal(x[:, 0], y[:, 0]) for x, y in zip(dec, free)), "the constraints changed no caption"


@pytest.mark.parametrize("case,mt", FIXTURES)
def test_score_captions_reproduces_the_model_score(golden_dir, case, mt):
    """(g) forced scoring of the returned rows gives the returned cum (rtol 1e-4 / atol 1e-6) and lengths, rows that pick PAD as a word
    excepted: the allocation reorders candidates, it does not touch their scores"""
    cfg, batch, model = _fixture(golden_dir, case, mt)
    tr = _translator(cfg, model)
    dec, _, sc, ln, _ = tr.translate_batch_constrained(syn.translate_inputs(batch), gold_constraints(cfg, batch), 4, **CTL)
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
def test_graph_replay_equals_eager_and_one_plan_serves_every_constraint_set(golden_dir, case, mt):
    """(h), (i): two constraint sets through one plan and one captured graph each give their own eager result; eager twice is bit-equal"""
    cfg, batch, model = _fixture(golden_dir, case, mt)
    eager, graphed = _translator(cfg, model), _translator(cfg, model, graph=True)
    sets = [gold_constraints(cfg, batch), gold_constraints(cfg, batch, other=True)]
    want = []
    for cons in sets:
        e = eager.translate_batch_constrained(syn.translate_inputs(batch), cons, 4, **CTL)
        e2 = eager.translate_batch_constrained(syn.translate_inputs(batch), cons, 4, **CTL)
        for k in (0, 2, 3, 4):                           # determinism over two calls
            assert all(torch.equal(a, b) for a, b in zip(e[k], e2[k]))
        want.append(e)
    assert any(not torch.equal(a, b) for a, b in zip(want[0][0], want[1][0])), "the two constraint sets decode alike"
    for _ in range(2):                                   # capture with the first set, then replay both
        for cons, e in zip(sets, want):
            g = graphed.translate_batch_constrained(syn.translate_inputs(batch), cons, 4, **CTL)
            for k in (0, 2, 3, 4):
                assert all(torch.equal(a, b) for a, b in zip(e[k], g[k]))
    graphed.translate_batch_constrained(syn.translate_inputs(batch), sets[0], 4, 1, **CTL)      # another n_best: the same plan
    assert len(graphed._preps) == 1 and len(list(graphed._preps.values())[0].graphs) == 1
    assert len(eager._preps) == 1
    graphed.translate_batch_nbest(syn.translate_inputs(batch), 4, 4, **CTL)                     # the unconstrained decode: its own plan
    assert len(graphed._preps) == 2


def test_bf16x3_deviation_at_config_1(golden_dir):
    """(j) bf16x3 on c1 against the fp32 CPU restatement: the sentences whose ids agree keep |cum − restatement| ≤ BOUND_X3; those whose
    ids disagree fall under the near-tie rule.  The measured worst deviation is written to the report directory
    (profiles/constrained_beam_parity.json is the committed copy)."""
    worst = {}
    for mt in ("v", "vivt"):
        cfg, batch, model = _fixture(golden_dir, "c1", mt)
        ref = _ref(golden_dir, "c1", mt, 4)
        ops.set_precision("bf16x3")
        try:
            _, _, _, model_x3 = build_model("c1", mt, golden_dir, DEV)          # (the same weights; its weight store gets the mode's lo plane)
            dec, _, sc, ln, met = _translator(cfg, model_x3).translate_batch_constrained(syn.translate_inputs(batch),
                                                                                         gold_constraints(cfg, batch), 4)
            torch.cuda.synchronize()
        finally:
            ops.set_precision("fp32")
        worst[mt + "_ids_differ"], worst[mt] = _compare(dec, sc, ln, met, ref, bound=True)      # (ids may differ only at a near-tie)
        assert worst[mt + "_ids_differ"] <= NEAR_SHARE * _near_share(ref)[1], worst              # … and on at most 5 % of the sentences
    print("bf16x3 c1 constrained: worst |cum - restatement| = %s" % json.dumps(worst))
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "constrained_beam_parity.json"), "w") as f:
        json.dump(dict(case="c1", precision="bf16x3", beam=4, worst_abs_cum_deviation=worst, bound=BOUND_X3), f, indent=1)
    assert max(worst["v"], worst["vivt"]) <= BOUND_X3, worst
