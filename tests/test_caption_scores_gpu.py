"""Bleu_1…4 / ROUGE_L / CIDEr of decoded captions on the MI355X: svpc_caption_tokens and svpc_caption_score_counts against the Python
restatement (tests/caption_scores_reference.py) on the fixture (tests/golden/caption_scores.json) and on hand-built edges; CaptionScores
(several updates, ``missing="empty"``, determinism, ``clean=``, N = 1 and N = 300, graph capture); and end to end on the outputs of the
greedy, beam, n-best and sampling decodes.  Integer counts are compared exactly, float scores within 1e-12 · max(1, |ref|) (every sum has
at most 1,024 non-negative terms: ≤ 1.1e-13 relative; a score composes a handful of them with correctly rounded ÷ and sqrt); Bleu values,
which get as small as 1e-15 without matches, relatively."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import caption_scores_reference as cs  # noqa: E402
from helpers import as_views as _views, build_model, host_rows as _host_rows  # noqa: E402
from svpc_amd import ops, synthetic as syn  # noqa: E402
from svpc_amd.caption_scores import ReferenceCorpus  # noqa: E402
from svpc_amd.metrics import CaptionScores, DecodeMetrics  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, IGNORE, PAD  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = type("O", (), {"cuda": True})
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "caption_scores.json")))
WORDS, V, KEYS, REFS = GOLD["idx2word"], GOLD["V"], GOLD["keys"], GOLD["references"]
SPECIAL = ["[PAD]", "[CLS]", "[SEP]", "[VID]", "[BOS]", "[EOS]", "[UNK]"]
TOL = 1e-12


def _same_scores(got, ref, what=None):
    assert len(got) == len(ref) == 6
    for k, (g, r) in enumerate(zip(got, ref)):
        bound = TOL * abs(r) if k < 4 else TOL * max(1.0, abs(r))                  # Bleu relatively
        assert abs(g - r) <= bound, (what, k, g, r)


def _same_result(got, ref):
    for k in ("num_videos", "testlen", "reflen", "correct", "guess"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    _same_scores([got[k] for k in CaptionScores.KEYS], [ref[k] for k in CaptionScores.KEYS])


class Case:
    """a reference set, its corpus on the device and the restatement's expectations"""

    def __init__(self, idx2word, refs, table_capacity=None):
        self.idx2word, self.refs, self.keys = idx2word, refs, list(refs)
        self.index = {k: i for i, k in enumerate(self.keys)}
        self.ref_tokens = [[cs.parse_sent(p) for p in refs[k]] for k in self.keys]
        self.cider = cs.CiderCorpus(self.ref_tokens)
        self.corpus = ReferenceCorpus(idx2word, refs, device=DEV, table_capacity=table_capacity)

    def plan(self, videos):
        return self.corpus.plan([dict(key=v["key"], oov_word_dict=v["oov"]) for v in videos])

    def hyp(self, v, rows=None):
        return cs.hypothesis_tokens(v["ids"] if rows is None else rows, self.idx2word, v.get("ref_oov", v["oov"]))

    def expected(self, v, rows=None):
        return cs.video_scores(self.hyp(v, rows), self.ref_tokens[self.index[v["key"]]], self.cider)

    def check(self, videos, dtype=torch.int64, pick=None):
        """tokens, counts and scores of one batch against the restatement; ``pick``: the ids are row ``pick`` of (T, 3, Lt)"""
        plan = self.plan(videos)
        steps = [len(v["ids"]) for v in videos]
        rows = [r for v in videos for r in v["ids"]]
        ids = torch.tensor(rows, dtype=dtype, device=DEV)
        if pick is not None:
            junk = torch.randint(0, len(self.idx2word), ids.shape, generator=torch.Generator().manual_seed(3)).to(ids)
            ids = torch.stack([ids if k == pick else junk for k in range(3)], dim=1).contiguous()
        words, ln = ops.clean_captions(ids, PAD, EOS, IGNORE, True, row=pick)
        tokens, tok_len = ops.caption_tokens(words, ln, plan, steps)
        assert tokens.dtype == torch.int32 and tuple(tokens.shape) == (len(videos), 1024)
        counts, scores = ops.caption_score_counts(tokens, tok_len, plan)
        strings = self.corpus.token_strings()
        tokens, tok_len, counts, scores = tokens.cpu().tolist(), tok_len.cpu().tolist(), counts.cpu().tolist(), scores.cpu().tolist()
        for n, v in enumerate(videos):
            h = self.hyp(v)
            assert tok_len[n] == len(h) and [strings[t] for t in tokens[n][:len(h)]] == h, v["key"]
            assert not any(tokens[n][len(h):])
            ref_counts, ref_scores = self.expected(v)
            assert counts[n] == ref_counts, (v["key"], counts[n], ref_counts)
            _same_scores(scores[n], ref_scores, v["key"])
        return counts, scores


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


# ------------------------------------------------------------------------------------------------ 1 + 2. the kernels on the fixture
@pytest.mark.parametrize("lt", [22, 64])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_kernels_equal_the_restatement_on_the_fixture(gold, lt, dtype):
    blocks = [b for b in GOLD["batches"] if b["lt"] == lt]
    assert blocks
    seen = 0
    for b in blocks:
        counts, scores = gold.check(b["videos"], dtype)
        for v, c, s in zip(b["videos"], counts, scores):                          # and against the recorded values
            assert c == v["counts"]
            _same_scores(s, v["scores"], v["key"])
            seen += 1
    assert seen == (96 if lt == 22 else 4)                                         # every video of the fixture is compared


def test_kernels_on_row_k_of_3d_ids(gold):
    gold.check(GOLD["batches"][0]["videos"], pick=1)
    gold.check(GOLD["batches"][-1]["videos"], torch.int32, pick=2)


def test_small_capacity_table(gold):
    need = len(gold.corpus.df) + 1
    small = Case(WORDS, REFS, table_capacity=1 << (need - 1).bit_length())
    assert small.corpus.longest_probe > 8
    for b in GOLD["batches"][:2] + GOLD["batches"][-1:]:
        small.check(b["videos"])


# ------------------------------------------------------------------------------------------------ hand-built edges
EDGE_WORDS = SPECIAL + ["add", "oil", "stir-fry", "1/2", "extra-virgin-olive", "the", "pan", "salt", "to", "and", "mix", "10"]
EDGE_W2I = {w: i for i, w in enumerate(EDGE_WORDS)}
EDGE_REFS = {
    "one": ["add oil to the pan and mix"],
    "tie": ["add oil to the pan", "add the oil to the pan and mix"],             # 5 and 8 tokens
    "four": ["add salt", "add salt and oil to the pan", "mix the salt", "stir fry the salt and the oil and the salt"],
    "olive": ["add extra virgin olive oil and stir fry"],
    "copied": ["add mirin and soy sauce to the stir fry"],
    "empty": ["mix the oil"],
}


def _edge_videos(lt=22):
    n = len(EDGE_WORDS)
    oov = {"mirin": n, "soy-sauce": n + 1, "3/4": n + 2, "x": n + 4}                # (id n + 3: a copied id no word spells)
    return [
        dict(key="one", oov={}, ids=_rows(["add oil", "to the pan pan and mix"], EDGE_W2I, lt)),
        dict(key="tie", oov={}, ids=_rows(["add the oil to", "the pan 1/2"], EDGE_W2I, lt)),                  # 6 tokens: |5 − 6| = 1, |8 − 6| = 2
        dict(key="four", oov={}, ids=_rows(["salt salt 10 salt", "the salt and the salt and the salt"], EDGE_W2I, lt)),
        dict(key="olive", oov={}, ids=_rows(["add 1/2 extra-virgin-olive oil", "", "and stir-fry 10"], EDGE_W2I, lt)),
        dict(key="copied", oov=oov, ref_oov=dict(oov, **{"1": n + 3, "2": n + 9, "3": -7}),               # (for the restatement: no token)
             ids=_rows(["add mirin 3/4 and soy-sauce", "to the stir-fry x"], EDGE_W2I, lt, oov)
             + [[BOS, n + 3, n + 9, -7, EDGE_W2I["pan"], EOS] + [PAD] * (lt - 6)]),                           # ids outside the video's universe
        dict(key="empty", oov={}, ids=_rows(["", "1/2 10", ""], EDGE_W2I, lt)),                                # an all-empty video
    ]


@pytest.fixture(scope="module")
def edge():
    return Case(EDGE_WORDS, EDGE_REFS)


@pytest.mark.parametrize("lt,dtype", [(22, torch.int64), (64, torch.int32)])
def test_tokens_and_counts_on_edges(edge, lt, dtype):
    vids = _edge_videos(lt)
    counts, scores = edge.check(vids, dtype)
    by = {v["key"]: c for v, c in zip(vids, counts)}
    assert by["empty"][4:] == [0, 0, 0, 0, 0, 3, 0] and by["olive"][8] == 8 and by["copied"][8] == 11       # words of 0, 1 and 3 tokens
    assert by["tie"][8:10] == [6, 5] and by["four"][9] == 10
    assert edge.hyp(vids[4])[-3:] == ["fry", "x", "pan"]                           # the ids outside the universe spell nothing
    edge.check(vids[::-1], dtype, pick=1)


def test_short_hypotheses_and_the_length_tie(edge):
    """0, 1, 2 and 3 tokens: guess clamps at 0 and `length` is the number of bigrams; two references at the same distance"""
    for sent, n_tok in (("", 0), ("oil", 1), ("add oil", 2), ("add oil to", 3), ("1/2", 0), ("stir-fry", 2)):
        vids = [dict(key=k, oov={}, ids=_rows([sent], EDGE_W2I, 22)) for k in ("one", "four", "tie")]
        counts, _ = edge.check(vids)
        for c in counts:
            assert c[8] == n_tok and c[4:8] == [max(0, n_tok - n) for n in range(4)]
    tie = Case(EDGE_WORDS, {"t": ["add oil to the pan", "add oil to the pan and mix the salt"], "u": ["mix salt"]})    # 5 and 9 tokens
    v = dict(key="t", oov={}, ids=_rows(["add oil to the", "pan and mix"], EDGE_W2I, 22))                           # 7: the tie goes to 5
    counts, _ = tie.check([v, dict(key="u", oov={}, ids=_rows(["salt"], EDGE_W2I, 22))])
    assert counts[0][8:10] == [7, 5]


def test_grams_absent_from_the_table(edge):
    """hypothesis grams no reference holds have idf ln N; a reference the video does not own shares grams with it"""
    vids = [dict(key="empty", oov={}, ids=_rows(["salt salt pan to", "to to salt pan salt"], EDGE_W2I, 22)),
            dict(key="one", oov={"zzz": len(EDGE_WORDS)}, ids=_rows(["zzz add zzz", "zzz add zzz oil"], EDGE_W2I, 22, {"zzz": len(EDGE_WORDS)}))]
    counts, scores = edge.check(vids)
    assert counts[0][0] == 0 and scores[0][5] == 0.0 and counts[1][0] == 2


def _long_case():
    """a 1,024-token reference beside a short one, and hypotheses within one caption of the 1,024-token cap"""
    names = ["".join(chr(97 + (i // 26 ** k) % 26) for k in range(2)) for i in range(40)]
    words = SPECIAL + names
    rng = np.random.default_rng(8)
    para = lambda n: " ".join(names[int(i)] for i in rng.integers(0, 40, size=n))     # noqa: E731
    refs = {"long": [para(1024), para(37)], "two": [para(1000), para(990)], "short": [para(5)]}
    w2i = {w: i for i, w in enumerate(words)}

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
    return words, refs, w2i, rows


def test_long_reference_and_hypothesis_near_the_cap():
    words, refs, w2i, rows = _long_case()
    case = Case(words, refs)
    vids = [dict(key="long", oov={}, ids=rows(16, 64)),                           # 16 · 62 = 992 tokens >= 1024 − 63
            dict(key="two", oov={}, ids=rows(16, 64)),
            dict(key="short", oov={}, ids=rows(3, 64))]
    counts, _ = case.check(vids)
    assert counts[0][8] == 992 and counts[1][8] == 992 and counts[1][9] == 990 and counts[0][10] > 100
    with pytest.raises(ValueError):
        case.check([dict(key="long", oov={}, ids=rows(17, 64))])                  # 17 · 63 > 1024: refused on the host


# ------------------------------------------------------------------------------------------------ 3. CaptionScores
def _update_all(f, case, blocks, dtype=torch.int64, views=True):
    pairs = []
    for b in blocks:
        rows = [v["ids"] for v in b["videos"]]
        lst = _views(rows, b["lt"], dtype) if views else [torch.tensor(r, dtype=dtype, device=DEV) for r in rows]
        f.update(lst, case.plan(b["videos"]))
        pairs += [(case.index[v["key"]], case.hyp(v)) for v in b["videos"]]
    return pairs


def test_caption_scores_against_the_restatement(gold):
    f = CaptionScores(gold.corpus)
    pairs = _update_all(f, gold, GOLD["batches"])
    assert f.last_counts.shape == (4, 11) and f.last_scores.shape == (4, 6) and f.last_scores.dtype == torch.float64
    got = f.result()
    ref, _ = cs.corpus_result(pairs, gold.ref_tokens)
    _same_result(got, ref)
    _same_result(got, GOLD["corpus"])
    assert f.result(missing="empty") == got                                        # every video has been updated
    # the same sequence again: the same bits; int32 ids in separate tensors (one copy): the same result
    f2, f3 = CaptionScores(gold.corpus), CaptionScores(gold.corpus)
    _update_all(f2, gold, GOLD["batches"])
    _update_all(f3, gold, GOLD["batches"], torch.int32, views=False)
    assert torch.equal(f.state, f2.state) and f2.result() == got and torch.equal(f.state, f3.state)
    f.reset()
    assert f.result()["num_videos"] == 0 and f.result()["CIDEr"] == 0.0 and f.last_scores is None and int(f.state.abs().sum()) == 0
    with pytest.raises(ValueError):
        f.result(missing="zero")
    with pytest.raises(ValueError):
        f.update(_views([v["ids"] for v in GOLD["batches"][0]["videos"]], 22), Case(EDGE_WORDS, EDGE_REFS).plan(_edge_videos()[:1]))


def test_missing_empty(gold):
    f = CaptionScores(gold.corpus)
    pairs = _update_all(f, gold, GOLD["batches"][:-1])                             # the four Lt = 64 videos stay without a prediction
    skip, _ = cs.corpus_result(pairs, gold.ref_tokens)
    _same_result(f.result(), skip)
    ref, _ = cs.corpus_result(pairs, gold.ref_tokens, missing="empty")
    got = f.result(missing="empty")
    _same_result(got, ref)
    _same_result(got, GOLD["corpus_missing_empty"])
    assert got["num_videos"] == 100 and got["reflen"] > skip["reflen"] and got["testlen"] == skip["testlen"]


def test_clean_argument_shares_one_clean_up(gold):
    b = GOLD["batches"][2]
    plan = gold.plan(b["videos"])
    views = _views([v["ids"] for v in b["videos"]], 22)
    f, g, h = CaptionScores(gold.corpus), CaptionScores(gold.corpus), CaptionScores(gold.corpus)
    f.update(views, plan)
    ids, _ = ops.stack_captions(views)
    clean = ops.clean_captions(ids, PAD, EOS, IGNORE, True)
    g.update(views, plan, clean=clean)
    dm = DecodeMetrics(V, DEV)
    dm.update(views)
    scores = h.update(views, plan, clean=dm.last_clean)
    assert scores is h.last_scores
    assert torch.equal(f.state, g.state) and torch.equal(f.state, h.state) and torch.equal(f.last_scores, h.last_scores)
    with pytest.raises(ValueError):
        g.update(views, plan, clean=(clean[0][:-1], clean[1][:-1]))


@pytest.mark.parametrize("n", [1, 300])
def test_one_and_three_hundred_one_sentence_videos(n):
    """N = 300: more videos than the accumulation has threads; N = 1: every idf is 0"""
    rng = np.random.default_rng(n)
    pool = EDGE_WORDS[7:]
    sent = lambda k: " ".join(pool[int(i)] for i in rng.integers(0, len(pool), size=k))         # noqa: E731
    refs = {"v%d" % i: [sent(int(rng.integers(3, 12)))] + ([sent(6)] if i % 7 == 0 else []) for i in range(n)}
    case = Case(EDGE_WORDS, refs)
    vids = []
    for i in range(n):
        s = sent(int(rng.integers(0, 12)))                                        # (runs collapse on both sides)
        vids.append(dict(key="v%d" % i, oov={}, ids=_rows([s], EDGE_W2I, 22)))
    f = CaptionScores(case.corpus)
    f.update(_views([v["ids"] for v in vids], 22), case.plan(vids))
    ref, rows = cs.corpus_result([(i, case.hyp(v)) for i, v in enumerate(vids)], case.ref_tokens)
    got = f.result()
    _same_result(got, ref)
    assert got["num_videos"] == n and f.last_counts.cpu().tolist() == [r[0] for r in rows]
    for s, r in zip(f.last_scores.cpu().tolist(), rows):
        _same_scores(s, r[1])
    if n == 1:
        assert got["CIDEr"] == 0.0


def test_update_captured(gold):
    from svpc_amd.graph import capturing
    # three batches of one (S_b) structure and one plan: the same videos, three different decodes
    b = GOLD["batches"][3]
    vids = b["videos"]
    plan = gold.plan(vids)
    steps = [len(v["ids"]) for v in vids]
    base = [r for v in vids for r in v["ids"]]
    rng = np.random.default_rng(6)
    offs = np.cumsum([0] + steps)

    def shuffled():                                                # the captions of every video in another order
        return [base[offs[n] + int(i)] for n, s in enumerate(steps) for i in rng.permutation(s)]
    three = [base, shuffled(), shuffled()]
    eager = CaptionScores(gold.corpus)
    for rows in three:
        buf = torch.tensor(rows, dtype=torch.int64, device=DEV)
        eager.update(list(torch.split(buf, steps)), plan)
    f = CaptionScores(gold.corpus)
    static = torch.tensor(three[0], dtype=torch.int64, device=DEV)
    views, o = [], 0
    for s in steps:
        views.append(static[o:o + s])
        o += s
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        f.update(views, plan)                                       # eager: caches the row table of this structure
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capturing(graph, stream=stream):
        f.update(views, plan)
    for rows in three[1:]:
        static.copy_(torch.tensor(rows, dtype=torch.int64, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        o, got = 0, f.last_counts.cpu().tolist()
        for n, (s, v) in enumerate(zip(steps, vids)):
            assert got[n] == gold.expected(v, rows[o:o + s])[0]
            o += s
    assert torch.equal(f.state, eager.state)
    assert f.result() == eager.result() and f.result()["num_videos"] == 3 * len(vids)


# ------------------------------------------------------------------------------------------------ 4. end to end
@pytest.mark.parametrize("case", ["tiny", "c1"])
def test_caption_scores_end_to_end(golden_dir, case):
    from svpc_amd.translator import Translator
    z, cfg, batch, model = build_model(case, "vivt", golden_dir, DEV)
    Vm = cfg.vocab_size
    i2w = SPECIAL + ["".join(chr(97 + (i // 26 ** k) % 26) for k in range(3)) for i in range(7, Vm)]
    # references from the synthetic labels: a video's paragraph is its steps' target words
    N = len(batch["batch_step_num"])
    refs, videos = {}, []
    for b in range(N):
        inv = {int(v): k for k, v in batch["oov_word_dict"][b].items()}
        sents = []
        for s in range(int(batch["batch_step_num"][b])):
            lab = batch["input_labels_list"][s][b].cpu().tolist()
            sents.append(" ".join(i2w[x] if x < Vm else inv[x] for x in lab if x not in (IGNORE, EOS, PAD)))
        refs["vid%d" % b] = [" ".join(sents)] + ([" ".join(sents[::-1])] if b % 2 else [])
        videos.append(dict(key="vid%d" % b, oov=batch["oov_word_dict"][b]))
    c = Case(i2w, refs)
    plan = c.plan(videos)
    tr = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model)
    dm0 = DecodeMetrics(Vm, DEV)
    before, _ = tr.translate_batch(syn.translate_inputs(batch))
    before = [d.clone() for d in before]
    dm0.update(before)
    f, dm = CaptionScores(c.corpus), DecodeMetrics(Vm, DEV)
    pairs = []

    def seen(dec, row=None):
        rows = _host_rows(dec, row)
        pairs.extend((b, c.hyp(videos[b], rows[b])) for b in range(N))
        return rows

    greedy, _ = tr.translate_batch(syn.translate_inputs(batch))
    dm.update(greedy)
    f.update(greedy, plan, clean=dm.last_clean)
    seen(greedy)
    for a, b in zip(before, greedy):                                # the decode itself is untouched by a live CaptionScores
        assert torch.equal(a, b)
    for b, d in enumerate(greedy):
        np.testing.assert_array_equal(d.cpu().numpy(), z["decode/%d" % b])
    assert dm.result() == dm0.result()                              # and so is DecodeMetrics
    beam, _, _ = tr.translate_batch_beam(syn.translate_inputs(batch), 2)
    f.update(beam, plan)
    seen(beam)
    nbest = tr.translate_batch_nbest(syn.translate_inputs(batch), 2, 2)[0]
    assert nbest[0].dim() == 3
    scores = f.update(nbest, plan, row=1)
    rows = seen(nbest, 1)
    for b in range(N):
        ref_counts, ref_scores = c.expected(videos[b], rows[b])
        assert f.last_counts[b].cpu().tolist() == ref_counts
        _same_scores(scores[b].cpu().tolist(), ref_scores)
    samples = tr.translate_batch_sample(syn.translate_inputs(batch), 2, seed=17)[0]
    f.update(samples, plan, row=1)
    rows = seen(samples, 1)

    ref, _ = cs.corpus_result(pairs, c.ref_tokens)
    got = f.result()
    _same_result(got, ref)
    assert got["num_videos"] == 4 * N and got["testlen"] > 0 and got["reflen"] > 0

    # Translator.caption_scores: the per-video scores on the device
    per = tr.caption_scores(samples, plan, row=1)
    assert per.dtype == torch.float64 and tuple(per.shape) == (N, 6) and per.is_cuda
    for b in range(N):
        _same_scores(per[b].cpu().tolist(), c.expected(videos[b], rows[b])[1])
