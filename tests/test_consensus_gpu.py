"""Consensus (minimum Bayes risk) selection among decoded candidates on the MI355X: svpc_consensus_tokens,
svpc_consensus_pair_scores and svpc_consensus_pick against the Python restatement (tests/consensus_reference.py) on the fixture
(tests/golden/caption_scores.json, candidates from the seeded maker) and on hand-built small groups; posterior weights; the gathered
rows; determinism and graph capture; and end to end behind ``Translator.translate_batch_consensus``.

Bounds.  Pair scores and expected utilities: 1e-12 · max(1, |ref|), the project's bound for these fp64 sums (§11.6: every sum has at
most 1,024 non-negative terms, a score composes a handful of them with correctly rounded ÷ and sqrt; an expected utility adds ≤ 15
weighted scores and one division); Bleu values, which get as small as 1e-15 without matches, relatively.  Pick: for every group the
restatement's E at the device's pick is within 1e-9 · max(1, |E_max|) of the restatement's maximum, and where best and second best differ
by more than that margin the pick is the restatement's arg max; the share of groups under the margin is bounded (5 % of paragraph
groups, 15 % of sentence groups — asserted on the restatement alone in tests/test_consensus_host.py, and here on the groups compared)."""
import functools
import json
import math
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import caption_scores_reference as cs  # noqa: E402
import consensus_reference as cr  # noqa: E402
from helpers import build_model  # noqa: E402
from svpc_amd import ops, synthetic as syn  # noqa: E402
from svpc_amd.caption_scores import ReferenceCorpus  # noqa: E402
from svpc_amd.metrics import DecodeMetrics  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, IGNORE, PAD  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = type("O", (), {"cuda": True})
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "caption_scores.json")))
WORDS, V, KEYS, REFS = GOLD["idx2word"], GOLD["V"], GOLD["keys"], GOLD["references"]
VIDEOS = [v for b in GOLD["batches"] for v in b["videos"]]
LT_OF = [b["lt"] for b in GOLD["batches"] for _ in b["videos"]]
SPECIAL = ["[PAD]", "[CLS]", "[SEP]", "[VID]", "[BOS]", "[EOS]", "[UNK]"]
TOL = 1e-12
SHARE = {"paragraph": 0.05, "sentence": 0.15}


def _same_scores(got, ref, what=None):
    assert len(got) == len(ref) == 6
    for k, (g, r) in enumerate(zip(got, ref)):
        bound = TOL * abs(r) if k < 4 else TOL * max(1.0, abs(r))                  # Bleu relatively
        assert abs(g - r) <= bound, (what, k, g, r)


def _translator():
    from svpc_amd.translator import Translator
    return object.__new__(Translator)              # ``consensus`` uses no model


class Case:
    """an idf corpus on the device and the restatement's CIDEr corpus"""

    def __init__(self, idx2word, refs):
        self.idx2word = idx2word
        self.cider = cs.CiderCorpus([[cs.parse_sent(p) for p in refs[k]] for k in refs])
        self.corpus = ReferenceCorpus(idx2word, refs, device=DEV)

    def plan(self, videos):
        return self.corpus.plan([dict(oov_word_dict=v["oov"]) for v in videos], references=False)

    def reference(self, videos, cands, scope, utility="CIDEr", cum=None):
        """→ the groups' (U, E, pick) in group order; ``cum[n][s][k]``"""
        out = []
        for n, v in enumerate(videos):
            out += cr.select(cands[n], self.idx2word, v.get("ref_oov", v["oov"]), self.cider, scope, utility, None if cum is None else cum[n])
        return out

    def run(self, videos, cands, scope, dtype=torch.int64, utility="CIDEr", weights="uniform", cum=None, lengths=None):
        """the two ops on the (T, K, Lt) ids of ``cands[n][k][s]`` → (ids, pair, tok_len, the pick's dict)"""
        plan = self.plan(videos)
        steps = [len(c[0]) for c in cands]
        K = len(cands[0])
        ids = torch.tensor([[cands[n][k][s] for k in range(K)] for n in range(len(videos)) for s in range(steps[n])], dtype=dtype, device=DEV)
        pair, tok_len = ops.consensus_pair_scores(ids, plan, steps, PAD, EOS, IGNORE, scope=scope)
        sc = None if cum is None else torch.tensor([row for c in cum for row in c], dtype=torch.float32, device=DEV)
        ln = None if lengths is None else torch.tensor([row for c in lengths for row in c], dtype=torch.int64, device=DEV)
        return ids, pair, tok_len, ops.consensus_pick(pair, ids, plan, steps, utility, scope, weights, sc, ln)

    def check(self, videos, cands, scope, ref=None, **kw):
        """pair scores, stream lengths, expected utilities, picks and gathered ids of one batch against the restatement →
        a namespace: G, under (groups under the margin), picks, and the device's ids / pair / tok_len / r (the pick's dict)"""
        ids, pair, tok_len, r = self.run(videos, cands, scope, **kw)
        ref = self.reference(videos, cands, scope, kw.get("utility", "CIDEr"), kw.get("cum") if kw.get("weights") == "posterior" else None) \
            if ref is None else ref
        K = len(cands[0])
        G = len(ref)
        assert tuple(pair.shape) == (G, K, K, 6) and pair.dtype == torch.float64 and tuple(tok_len.shape) == (G, K)
        assert tuple(r["expected"].shape) == (G, K) and r["expected"].dtype == torch.float64 and r["pick"].dtype == torch.int32
        pair_h, exp_h, pick_h = pair.cpu().tolist(), r["expected"].cpu().tolist(), r["pick"].cpu().tolist()
        under = 0
        for g, (U, E, _) in enumerate(ref):
            for i in range(K):
                for j in range(K):
                    _same_scores(pair_h[g][i][j], U[i][j], (scope, g, i, j))
                assert abs(exp_h[g][i] - E[i]) <= TOL * max(1.0, abs(E[i])), (scope, g, i, exp_h[g][i], E[i])
            e_max = max(E)
            assert E[pick_h[g]] >= e_max - cr.MARGIN * max(1.0, abs(e_max)), (scope, g, pick_h[g], E)
            if cr.under_margin(E):
                under += 1
            else:
                assert pick_h[g] == cr.pick_of(E), (scope, g, pick_h[g], E)
        # the gathered rows
        steps = [len(c[0]) for c in cands]
        row_pick = r["row_pick"].cpu().tolist()
        want = [pick_h[n] for n, s in enumerate(steps) for _ in range(s)] if scope == "paragraph" else pick_h
        assert row_pick == want and r["ids"].dtype == torch.int64
        t = torch.arange(ids.shape[0], device=DEV)
        assert torch.equal(r["ids"], ids[t, r["row_pick"]].to(torch.int64))
        return SimpleNamespace(G=G, under=under, picks=pick_h, ids=ids, pair=pair, tok_len=tok_len, r=r)


def _rows(sentences, w2i, lt, oov=None):
    look = dict(w2i)
    look.update(oov or {})
    out = []
    for s in sentences:
        ids = [look[w] for w in (s.split(" ") if s else [])]
        assert len(ids) <= lt - 2
        out.append(([BOS] + ids + [EOS] + [PAD] * lt)[:lt])
    return out


@pytest.fixture(scope="module")
def gold():
    return Case(WORDS, REFS)


@functools.lru_cache(maxsize=None)
def _fixture_candidates():
    rng = random.Random(7)
    return [cr.make_candidates(v["ids"], 4, rng, V, BOS, EOS, PAD) for v in VIDEOS]


_FIXTURE_REF = {}


def _fixture_reference(gold, scope):
    """the restatement of all 100 fixture videos at K = 4, once per scope: per video its groups"""
    if scope not in _FIXTURE_REF:
        cands = _fixture_candidates()
        _FIXTURE_REF[scope] = [gold.reference([v], [cands[n]], scope) for n, v in enumerate(VIDEOS)]
    return _FIXTURE_REF[scope]


# ------------------------------------------------------------------------------------------------ 1. the kernels on the fixture
@pytest.mark.parametrize("lt,dtype", [(22, torch.int64), (22, torch.int32), (64, torch.int64), (64, torch.int32)])
@pytest.mark.parametrize("scope", ["paragraph", "sentence"])
def test_kernels_equal_the_restatement_on_the_fixture(gold, scope, lt, dtype):
    """every video of the fixture (96 at Lt = 22, 4 at Lt = 64; 68 with copied words), K = 4"""
    sel = [n for n in range(len(VIDEOS)) if LT_OF[n] == lt]
    assert len(sel) == (96 if lt == 22 else 4) and any(VIDEOS[n]["oov"] for n in sel)
    per_video = _fixture_reference(gold, scope)
    cands = _fixture_candidates()
    c = gold.check([VIDEOS[n] for n in sel], [cands[n] for n in sel], scope, ref=[g for n in sel for g in per_video[n]], dtype=dtype)
    assert c.G == (len(sel) if scope == "paragraph" else sum(len(VIDEOS[n]["ids"]) for n in sel))
    if lt == 22:
        print("%s: %d of %d groups under the margin" % (scope, c.under, c.G))
        assert c.under <= SHARE[scope] * c.G and len(set(c.picks)) == 4              # and the picks are not all one candidate


def test_other_utilities_and_posterior_weights_on_a_fixture_batch(gold):
    vids = GOLD["batches"][1]["videos"]
    cands = _fixture_candidates()[8:16]
    rng = random.Random(11)
    cum = [[[float(np.float32(-rng.random() * 8.0)) for _ in range(4)] for _ in v["ids"]] for v in vids]
    for scope in ("paragraph", "sentence"):
        gold.check(vids, cands, scope, utility="ROUGE_L")
        gold.check(vids, cands, scope, utility="Bleu_4", weights="posterior", cum=cum)
        gold.check(vids, cands, scope, weights="posterior", cum=cum)


# ------------------------------------------------------------------------------------------------ 2. small shapes
EDGE_WORDS = SPECIAL + ["add", "oil", "stir-fry", "1/2", "extra-virgin-olive", "the", "pan", "salt", "to", "and", "mix", "10"]
EDGE_W2I = {w: i for i, w in enumerate(EDGE_WORDS)}
EDGE_REFS = {"one": ["add oil to the pan and mix"], "two": ["add salt and oil to the pan", "mix the salt"], "three": ["stir fry the salt and the oil"],
             "four": ["add extra virgin olive oil and stir fry"], "five": ["mix the oil"]}
EDGE_POOL = ["", "1/2", "oil", "extra-virgin-olive", "add oil", "add oil to the pan", "add salt and oil to the pan", "mix the salt and the oil",
             "stir-fry the salt", "to the pan", "10 1/2", "add the oil to the pan and mix", "salt", "the pan and the salt", "mix", "oil and salt"]


@pytest.fixture(scope="module")
def edge():
    return Case(EDGE_WORDS, EDGE_REFS)


def _edge_groups(K, lt=22):
    """videos of one and of several sentences: streams of 0, 1 and 3 tokens, an all-empty group, a group of identical candidates"""
    n = len(EDGE_WORDS)
    oov = {"mirin": n, "soy-sauce": n + 1}
    pick = lambda i: EDGE_POOL[i % len(EDGE_POOL)]                                 # noqa: E731
    vids = [
        dict(oov={}, sents=[[pick(k) for k in range(K)]]),                                             # S_b = 1: 0, 0, 1, 3 … tokens
        dict(oov={}, sents=[[["", "1/2", "10 1/2"][k % 3] for k in range(K)]]),                        # an all-empty group
        dict(oov={}, sents=[["add oil to the pan"] * K, ["mix the salt"] * K]),                        # identical candidates
        dict(oov=oov, sents=[[(pick(3 * k + s) + (" mirin" if k % 2 else " soy-sauce")).strip() for k in range(K)] for s in range(3)]),
        dict(oov={}, sents=[[pick(5 * k + 2 * s + 1) for k in range(K)] for s in range(2)]),
    ]
    cands = [[_rows([sent[k] for sent in v["sents"]], EDGE_W2I, lt, v["oov"]) for k in range(K)] for v in vids]
    return vids, cands


@pytest.mark.parametrize("K", [1, 2, 3, 16])
def test_small_groups(edge, K):
    vids, cands = _edge_groups(K)
    for scope in ("paragraph", "sentence"):
        for dtype, utility in ((torch.int64, "CIDEr"), (torch.int32, "ROUGE_L")):
            c = edge.check(vids, cands, scope, dtype=dtype, utility=utility)
            G, picks, r, lens = c.G, c.picks, c.r, c.tok_len.cpu().tolist()
            g_empty, g_same = 1, 2                                                   # (in both scopes: the first two videos hold one sentence)
            assert lens[g_empty] == [0] * K and not r["expected"][g_empty].any() and picks[g_empty] == 0          # the all-empty group
            assert len(set(r["expected"][g_same].cpu().tolist())) == 1 and picks[g_same] == 0                        # identical: the lowest
            if K >= 4:
                assert lens[0][:4] == [0, 0, 1, 3]
            if K == 1:
                assert not r["expected"].any() and picks == [0] * G


def test_one_group_and_three_hundred_groups(edge):
    """G = 1; G = 300 one-sentence videos (more groups than a workgroup has threads), K = 3"""
    rng = random.Random(5)
    pool = EDGE_WORDS[7:]
    sent = lambda: " ".join(rng.choice(pool) for _ in range(rng.randrange(0, 9)))      # noqa: E731
    for n_vid in (1, 300):
        vids = [dict(oov={}) for _ in range(n_vid)]
        cands = [[_rows([sent()], EDGE_W2I, 22) for _ in range(3)] for _ in range(n_vid)]
        for scope in ("paragraph", "sentence"):
            assert edge.check(vids, cands, scope).G == n_vid


def test_group_at_the_lds_maximum():
    """K = 16 streams of 992 tokens — within one caption of the 1,024-token cap: the kernel's largest LDS footprint.  A live restatement
    of all 256 pairs would take minutes (the textbook LCS is 10⁶ steps a pair), so the named pairs below are compared, and the
    others by what must hold of them: a candidate against itself scores Bleu 1, ROUGE_L 1, and ROUGE_L is symmetric at equal lengths."""
    names = ["".join(chr(97 + (i // 26 ** k) % 26) for k in range(2)) for i in range(40)]
    words = SPECIAL + names
    rng = np.random.default_rng(8)
    refs = {"r%d" % i: [" ".join(names[int(x)] for x in rng.integers(0, 40, size=30))] for i in range(6)}
    case = Case(words, refs)

    def rows(n_rows, lt):
        out = []
        for _ in range(n_rows):
            ids = []
            while len(ids) < lt - 2:                                              # (no run: the clean-up collapses them)
                x = int(rng.integers(7, 47))
                if not ids or ids[-1] != x:
                    ids.append(x)
            out.append([BOS] + ids + [EOS])
        return out
    K = 16
    cands = [[rows(16, 64) for _ in range(K)]]
    cands[0][5] = [list(r) for r in cands[0][2]]                                   # two identical streams among them
    vids = [dict(oov={})]
    ids, pair, tok_len, r = case.run(vids, cands, "paragraph")
    assert tok_len.cpu().tolist() == [[992] * K]
    streams = cr.group_streams(cands[0], words, {}, "paragraph")[0]
    pair_h = pair.cpu().tolist()[0]
    for i, j in ((0, 1), (15, 0), (7, 7), (2, 5)):
        _same_scores(pair_h[i][j], cr.pair_utility(streams[i], streams[j], case.cider), (i, j))
    for i in range(K):
        assert all(abs(x - 1.0) <= 1e-9 for x in pair_h[i][i][:5])
        for j in range(K):
            assert pair_h[i][j][4] == pair_h[j][i][4] and 0.0 < pair_h[i][j][4] <= 1.0
    assert pair_h[2][5] == pair_h[2][2] and pair_h[5][2] == pair_h[5][5]
    E = r["expected"].cpu().tolist()[0]
    assert abs(E[2] - E[5]) <= TOL * max(E) and int(r["pick"][0]) in (2, 5) and max(E) - E[2] <= TOL * max(E)    # each has a perfect match
    with pytest.raises(ValueError):
        case.run(vids, [[rows(17, 64) for _ in range(2)]], "paragraph")            # 17 · 63 > 1,024: refused on the host
    case.run(vids, [[rows(17, 64) for _ in range(2)]], "sentence")                 # a sentence's stream is one caption


def test_list_that_is_not_one_buffer(gold):
    vids = GOLD["batches"][2]["videos"]
    cands = _fixture_candidates()[16:24]
    tr = _translator()
    plan = gold.plan(vids)
    K = 4
    per = [torch.tensor([[c[k][s] for k in range(K)] for s in range(len(c[0]))], dtype=torch.int64, device=DEV) for c in cands]
    buf = torch.cat(per)
    views, o = [], 0
    for p in per:
        views.append(buf[o:o + p.shape[0]])
        o += p.shape[0]
    assert ops.stack_captions(views)[0].data_ptr() == buf.data_ptr()
    for scope in ("paragraph", "sentence"):
        a, b = tr.consensus(views, plan, scope=scope), tr.consensus(per, plan, scope=scope)
        assert torch.equal(a.pair_scores, b.pair_scores) and torch.equal(a.pick, b.pick)
        for x, y in zip(a.dec_seq_list + a.pick_list + a.expected_list, b.dec_seq_list + b.pick_list + b.expected_list):
            assert torch.equal(x, y)
        # the result's lists: consecutive views of one buffer, (S_b, Lt) / (S_b,) / (S_b, K)
        assert ops.stack_captions(a.dec_seq_list)[0].data_ptr() == a.dec_seq_list[0].data_ptr()
        for n, p in enumerate(per):
            S = p.shape[0]
            assert tuple(a.dec_seq_list[n].shape) == (S, 22) and a.dec_seq_list[n].dtype == torch.int64
            assert tuple(a.pick_list[n].shape) == (S,) and a.pick_list[n].dtype == torch.int64
            assert tuple(a.expected_list[n].shape) == (S, K) and a.expected_list[n].dtype == torch.float64
            assert torch.equal(a.dec_seq_list[n], p[torch.arange(S, device=DEV), a.pick_list[n]])
            if scope == "paragraph":
                assert len(set(a.pick_list[n].cpu().tolist())) == 1
        assert a.score_list is None and a.length_list is None


# ------------------------------------------------------------------------------------------------ 3. posterior weights
def test_anchor_table_on_the_device():
    """corpus references `a b` | `a c`, candidates `a b`, `a b`, `a c` (the issue's table)"""
    words = SPECIAL + ["a", "b", "c"]
    w2i = {w: i for i, w in enumerate(words)}
    case = Case(words, {"x": ["a b"], "y": ["a c"]})
    vids = [dict(oov={})]
    cands = [[_rows([s], w2i, 22) for s in ("a b", "a b", "a c")]]
    ln3, inf = float(np.float32(math.log(3.0))), -math.inf
    for weights, cum, E, pick in (("uniform", None, [2.5, 2.5, 0.0], 0), ("posterior", [0.0, ln3, 0.0], [3.75, 2.5, 0.0], 0),
                                  ("posterior", [ln3, 0.0, 0.0], [2.5, 3.75, 0.0], 1),
                                  ("posterior", [0.0, inf, 0.0], [0.0, 2.5, 0.0], 1),                  # a row of −inf: its weight is 0
                                  ("posterior", [inf, inf, inf], [2.5, 2.5, 0.0], 0)):                 # all −inf: every weight 1
        for scope in ("paragraph", "sentence"):
            ids, pair, _, r = case.run(vids, cands, scope, weights=weights, cum=None if cum is None else [[cum]])
            p = pair.cpu().tolist()[0]
            assert abs(p[0][1][5] - 5.0) <= 1e-12 and p[0][2][5] == 0.0 and p[2][0][5] == 0.0
            got = r["expected"].cpu().tolist()[0]
            assert all(abs(g - e) <= 1e-6 for g, e in zip(got, E)), (weights, cum, got)               # (ln 3 rounded to fp32)
            assert int(r["pick"][0]) == pick
            case.check(vids, cands, scope, weights=weights, cum=None if cum is None else [[cum]])


def test_posterior_weights_sum_over_a_video(edge):
    vids, cands = _edge_groups(3)
    vids, cands = vids[3:], cands[3:]
    flat = [[[-2.5] * 3 for _ in c[0]] for c in cands]
    assert edge.check(vids, cands, "paragraph", weights="posterior", cum=flat).picks == edge.check(vids, cands, "paragraph").picks
    for k in range(3):                                                             # the mass on pseudo-reference k, split over the sentences
        cum = [[[-1.5 if j == k else -3.0 for j in range(3)] for _ in c[0]] for c in cands]
        cum[0][1][(k + 1) % 3] = -math.inf                                         # one sentence at −inf: the video's sum is −inf
        cum[1][0][k] = -0.25
        edge.check(vids, cands, "paragraph", weights="posterior", cum=cum)
        edge.check(vids, cands, "sentence", weights="posterior", cum=cum)


# ------------------------------------------------------------------------------------------------ 4. gathered outputs
def test_gathered_scores_lengths_and_decode_metrics(gold):
    vids = [v for n, v in enumerate(GOLD["batches"][0]["videos"]) if n != 5]       # (video 5 spells no token: every utility is 0)
    K, k_star = 3, 1
    cands = []
    for v in vids:                                                                 # candidate 1 holds both halves of what 0 and 2 hold: by ROUGE_L it wins
        halves = [[], []]
        for row in v["ids"]:
            w = [x for x in row[1:row.index(EOS)]]
            halves[0].append(([BOS] + w[:len(w) // 2] + [EOS] + [PAD] * 22)[:22])
            halves[1].append(([BOS] + w[len(w) // 2:] + [EOS] + [PAD] * 22)[:22])
        cands.append([halves[0], [list(r) for r in v["ids"]], halves[1]])
    rng = random.Random(2)
    cum = [[[float(np.float32(-rng.random() * 5)) for _ in range(K)] for _ in v["ids"]] for v in vids]
    lengths = [[[rng.randrange(1, 22) for _ in range(K)] for _ in v["ids"]] for v in vids]
    assert gold.check(vids, cands, "paragraph", utility="ROUGE_L").picks == [k_star] * len(vids)
    ids, pair, _, r = gold.run(vids, cands, "sentence", cum=cum, lengths=lengths)
    t = torch.arange(ids.shape[0], device=DEV)
    sc = torch.tensor([row for c in cum for row in c], dtype=torch.float32, device=DEV)
    ln = torch.tensor([row for c in lengths for row in c], dtype=torch.int64, device=DEV)
    assert torch.equal(r["ids"], ids[t, r["row_pick"]]) and torch.equal(r["scores"], sc[t, r["row_pick"]]) and torch.equal(r["lengths"], ln[t, r["row_pick"]])
    assert r["scores"].dtype == torch.float32 and r["lengths"].dtype == torch.int64
    # through the translator: the chosen captions flow into DecodeMetrics like any decode result
    tr = _translator()
    steps = [len(v["ids"]) for v in vids]
    dec = list(torch.split(ids, steps))
    res = tr.consensus(dec, gold.plan(vids), scores=list(torch.split(sc, steps)), lengths=list(torch.split(ln, steps)), utility="ROUGE_L")
    assert [int(p[0]) for p in res.pick_list] == [k_star] * len(vids)
    a, b = DecodeMetrics(V, DEV), DecodeMetrics(V, DEV)
    a.update(res.dec_seq_list)
    b.update(dec, row=k_star)
    assert a.result() == b.result()
    for n, (x, y) in enumerate(zip(torch.split(sc, steps), torch.split(ln, steps))):
        assert torch.equal(res.score_list[n], x[:, k_star]) and torch.equal(res.length_list[n], y[:, k_star])


# ------------------------------------------------------------------------------------------------ 5. determinism and capture
def test_determinism_and_capture(gold):
    from svpc_amd.graph import capturing
    vids = GOLD["batches"][3]["videos"]
    K = 4
    steps = [len(v["ids"]) for v in vids]
    plan = gold.plan(vids)
    tr = _translator()
    rng = random.Random(9)
    three = []
    for _ in range(3):
        cands = [cr.make_candidates(v["ids"], K, rng, V, BOS, EOS, PAD) for v in vids]
        ids = torch.tensor([[c[k][s] for k in range(K)] for c in cands for s in range(len(c[0]))], dtype=torch.int64, device=DEV)
        sc = torch.tensor([[-rng.random() * 6 for _ in range(K)] for _ in range(sum(steps))], dtype=torch.float32, device=DEV)
        three.append((ids, sc))
    kw = dict(scope="sentence", weights="posterior", utility="CIDEr")

    def call(ids, sc):
        return tr.consensus(list(torch.split(ids, steps)), plan, scores=list(torch.split(sc, steps)), **kw)

    def bits(r):
        return [x.clone() for x in [r.pair_scores, r.pick] + r.dec_seq_list + r.pick_list + r.expected_list + r.score_list]
    eager = [bits(call(*x)) for x in three]
    again = bits(call(*three[0]))
    assert all(torch.equal(a, b) for a, b in zip(eager[0], again))                 # identical inputs: identical bits
    assert not torch.equal(eager[0][0], eager[1][0])
    s_ids, s_sc = three[0][0].clone(), three[0][1].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        call(s_ids, s_sc)                                                          # eager: caches the group tables of this structure
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capturing(graph, stream=stream):
        res = call(s_ids, s_sc)
    for n in (1, 2):
        s_ids.copy_(three[n][0])
        s_sc.copy_(three[n][1])
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager[n], bits(res))), n


# ------------------------------------------------------------------------------------------------ 6. end to end
@pytest.mark.parametrize("case", ["tiny", "c1"])
def test_translate_batch_consensus_end_to_end(golden_dir, case):
    from svpc_amd.translator import Translator
    z, cfg, batch, model = build_model(case, "vivt", golden_dir, DEV)
    Vm = cfg.vocab_size
    i2w = SPECIAL + ["".join(chr(97 + (i // 26 ** k) % 26) for k in range(3)) for i in range(7, Vm)]
    N = len(batch["batch_step_num"])
    refs, videos = {}, []
    for b in range(N):                                                             # the idf corpus: the synthetic labels as "training references"
        inv = {int(v): k for k, v in batch["oov_word_dict"][b].items()}
        sents = []
        for s in range(int(batch["batch_step_num"][b])):
            lab = batch["input_labels_list"][s][b].cpu().tolist()
            sents.append(" ".join(i2w[x] if x < Vm else inv[x] for x in lab if x not in (IGNORE, EOS, PAD)))
        refs["vid%d" % b] = [" ".join(sents)]
        videos.append(dict(oov=batch["oov_word_dict"][b]))
    c = Case(i2w, refs)
    plan = c.plan(videos)
    tr = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model)
    greedy0 = [d.clone() for d in tr.translate_batch(syn.translate_inputs(batch))[0]]
    dm0 = DecodeMetrics(Vm, DEV)
    dm0.update(greedy0)
    K = 3

    def compare(dec, sc, got, picks, scope, weights):
        rows = [d.cpu().tolist() for d in dec]                                      # [b][s][k]
        cands = [[[rows[b][s][k] for s in range(len(rows[b]))] for k in range(K)] for b in range(N)]
        cum = [x.cpu().tolist() for x in sc] if weights == "posterior" else None
        ref = c.reference(videos, cands, scope, "CIDEr", cum)
        g = 0
        for b in range(N):
            S = len(rows[b])
            assert tuple(got[b].shape) == (S, dec[b].shape[-1]) and got[b].dtype == torch.int64 and picks[b].dtype == torch.int64
            assert torch.equal(got[b], dec[b][torch.arange(S, device=DEV), picks[b]])       # the chosen ids are the decode's rows at pick
            for s in range(S):
                E = ref[g][1]
                e_max = max(E)
                p = int(picks[b][s])
                assert E[p] >= e_max - cr.MARGIN * max(1.0, abs(e_max))
                if not cr.under_margin(E):
                    assert p == cr.pick_of(E)
                g += scope == "sentence"
            g += scope == "paragraph"

    for scope, weights in (("paragraph", "uniform"), ("sentence", "posterior")):
        dec, _, sc, ln = tr.translate_batch_sample(syn.translate_inputs(batch), num_samples=K, seed=17)
        got, oov, picks = tr.translate_batch_consensus(syn.translate_inputs(batch), plan, source="sample", num_candidates=K, seed=17,
                                                       scope=scope, weights=weights)
        assert len(oov) == N
        compare(dec, sc, got, picks, scope, weights)
        dec, _, sc, ln = tr.translate_batch_nbest(syn.translate_inputs(batch), 3, K)
        got, oov, picks = tr.translate_batch_consensus(syn.translate_inputs(batch), plan, source="nbest", num_candidates=K, beam_size=3,
                                                       scope=scope, weights=weights)
        compare(dec, sc, got, picks, scope, weights)
        full = tr.consensus(dec, plan, scores=sc, lengths=ln, scope=scope, weights=weights)
        for b in range(N):
            S = dec[b].shape[0]
            t = torch.arange(S, device=DEV)
            assert torch.equal(full.dec_seq_list[b], got[b]) and torch.equal(full.pick_list[b], picks[b])
            assert torch.equal(full.score_list[b], sc[b][t, picks[b]]) and torch.equal(full.length_list[b], ln[b][t, picks[b]])
        dm = DecodeMetrics(Vm, DEV)
        dm.update(got)                                                             # the result is a decode result like any other
    # greedy and the existing metrics are untouched
    greedy = tr.translate_batch(syn.translate_inputs(batch))[0]
    for a, b in zip(greedy0, greedy):
        assert torch.equal(a, b)
    for b, d in enumerate(greedy):
        np.testing.assert_array_equal(d.cpu().numpy(), z["decode/%d" % b])
    dm1 = DecodeMetrics(Vm, DEV)
    dm1.update(greedy)
    assert dm1.result() == dm0.result()
