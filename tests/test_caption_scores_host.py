"""Bleu_1…4 / ROUGE_L / CIDEr of decoded captions without a GPU: the Python restatement (tests/caption_scores_reference.py) against the
hand-derived anchors and the fixture's recorded values (tests/golden/caption_scores.json, tools/make_golden_caption_scores.py); the
per-word tokenisation; the tables ``svpc_amd.caption_scores`` compiles (lexicon, CSRs, document frequencies, idf, norms, the gram table
probed the way the kernel probes it); every host check; the no-CPU-fallback rule; the C-ABI declarations.

The scores are pinned to the published definitions as the restatement states them, not to outputs of the third-party
scorer, which is not available."""
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

import caption_scores_reference as cs  # noqa: E402
from caption_metrics_reference import clean_caption  # noqa: E402
from svpc_amd import _lib, caption_scores as sc, ops  # noqa: E402
from svpc_amd.caption_scores import ReferenceCorpus  # noqa: E402
from svpc_amd.metrics import CaptionScores  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, PAD  # noqa: E402

GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "caption_scores.json")))
WORDS, V, KEYS, REFS = GOLD["idx2word"], GOLD["V"], GOLD["keys"], GOLD["references"]
REF_TOKENS = [[cs.parse_sent(p) for p in REFS[k]] for k in KEYS]
INDEX = {k: i for i, k in enumerate(KEYS)}
VIDEOS = [(b["lt"], v) for b in GOLD["batches"] for v in b["videos"]]


def _close(got, ref, tol=1e-12):
    return abs(got - ref) <= tol * max(1.0, abs(ref))


def _video(v):
    return dict(key=v["key"], oov_word_dict=v["oov"])


@pytest.fixture(scope="module")
def corpus():
    return ReferenceCorpus(WORDS, REFS, device="cpu")


# ------------------------------------------------------------------------------------------------ 1. the restatement
def test_anchor_clipping():
    h = ["the"] * 7
    refs = ["the cat is on the mat".split(), "there is a cat on the mat".split()]
    correct, guess, testlen, reflen = cs.bleu_counts(h, refs)
    assert correct == [2, 0, 0, 0] and guess == [7, 6, 5, 4] and (testlen, reflen) == (7, 7)


def test_anchor_two_videos_one_reference_each():
    res, rows = cs.corpus_result({0: "a b".split(), 1: "a b".split()}, [["a b".split()], ["a c".split()]])
    assert [r[1][5] for r in rows] == [5.0, 0.0] and res["CIDEr"] == 2.5
    assert res["correct"] == [3, 1, 0, 0] and res["guess"] == [4, 2, 0, 0] and res["testlen"] == res["reflen"] == 4
    assert _close(res["Bleu_1"], 0.7499999996250004, 1e-15) and _close(res["Bleu_2"], 0.6123724353130623, 1e-15)


def test_anchor_two_references():
    refs = [["a b".split(), "a b b c".split()], ["a c".split()]]
    _, rows = cs.corpus_result({0: "a b b".split(), 1: ["c"]}, refs)
    assert _close(rows[0][1][5], 4.599066117289982, 1e-15) and rows[1][1][5] == 0.0


def test_anchor_rouge():
    score, best = cs.rouge_l("a b c d".split(), ["a x c d e".split()])
    assert _close(score, 0.6535714285714286, 1e-15) and best == 3
    assert cs.rouge_l([], ["a b".split()]) == (0.0, 0)


def test_anchor_hypothesis_equal_to_its_reference():
    refs = [[cs.parse_sent(REFS[k][0])] for k in KEYS]
    res, rows = cs.corpus_result({i: r[0] for i, r in enumerate(refs)}, refs)
    assert len(rows) == 100 and _close(res["CIDEr"], 10.0) and _close(res["ROUGE_L"], 1.0)
    assert all(_close(r[1][5], 10.0) and r[1][4] == 1.0 for r in rows)
    assert res["correct"] == res["guess"] and _close(res["Bleu_4"], 1.0, 1e-9)


def test_anchor_one_video_corpus():
    res, _ = cs.corpus_result({0: "a b c".split()}, [["a b c".split()]])
    assert res["CIDEr"] == 0.0 and res["ROUGE_L"] == 1.0                           # every idf is ln 1 − ln 1 = 0


def test_lcs_forms_equal_the_textbook_table():
    """the two wave-friendly forms (row prefix maximum; bit vector) against the dynamic programme"""
    rng = np.random.default_rng(3)
    for _ in range(300):
        a = rng.integers(1, 5, size=int(rng.integers(0, 40))).tolist()
        b = rng.integers(1, 5, size=int(rng.integers(1, 40))).tolist()
        row = [0] * len(b)
        for x in a:
            cand = [max(row[j], (row[j - 1] if j else 0) + (x == b[j])) for j in range(len(b))]
            row = [max(cand[:j + 1]) for j in range(len(b))]
        v = (1 << len(b)) - 1
        for x in a:
            m = sum(1 << j for j, y in enumerate(b) if y == x)
            v = ((v + (v & m)) | (v & ~m)) & ((1 << len(b)) - 1)
        assert cs.lcs(a, b) == (row[-1] if a else 0) == len(b) - bin(v).count("1")


def test_restatement_equals_the_fixture():
    assert len(VIDEOS) == 100 and sorted(INDEX[v["key"]] for _, v in VIDEOS) == list(range(100))       # every video, none twice
    cider = cs.CiderCorpus(REF_TOKENS)
    hyps = {}
    for _, v in VIDEOS:
        h = cs.hypothesis_tokens(v["ids"], WORDS, v["oov"])
        hyps[INDEX[v["key"]]] = h
        counts, scores = cs.video_scores(h, REF_TOKENS[INDEX[v["key"]]], cider)
        assert counts == v["counts"], v["key"]
        assert all(_close(g, r) for g, r in zip(scores, v["scores"])), v["key"]
    res, _ = cs.corpus_result(hyps, REF_TOKENS)
    short = {v["key"] for lt, v in VIDEOS if lt == 64}
    res_e, _ = cs.corpus_result({i: h for i, h in hyps.items() if KEYS[i] not in short}, REF_TOKENS, missing="empty")
    for got, ref in ((res, GOLD["corpus"]), (res_e, GOLD["corpus_missing_empty"])):
        for k, r in ref.items():
            assert got[k] == r if isinstance(r, (int, list)) else _close(got[k], r), k
    assert res_e["num_videos"] == 100 and res_e["reflen"] > res["reflen"] - 400 and res_e["testlen"] < res["testlen"]


def test_fixture_covers_the_definitions():
    assert (GOLD["pad"], GOLD["eos"], GOLD["bos"]) == (PAD, EOS, BOS) and V == 951 == len(WORDS)
    assert {lt for lt, _ in VIDEOS} == {22, 64} and sum(len(v["ids"]) for _, v in VIDEOS) == 798
    assert all(c > 0 for c in GOLD["corpus"]["correct"]) and GOLD["clipped_grams"] >= 50 and GOLD["length_ties"] >= 1
    lens = sorted(v["counts"][8] for _, v in VIDEOS)
    assert lens[0] == 0 and lens[1] == 1
    assert sum(1 for k in KEYS if len(REFS[k]) == 2) == 10
    rows = [r for _, v in VIDEOS for r in v["ids"]]
    with_eos = [r for r in rows if EOS in r]
    assert any(r[-1] == PAD for r in with_eos) and any(EOS in r[r.index(EOS) + 1:] for r in with_eos)        # both fill styles
    n_tok = {len(cs.parse_sent(w)) for _, v in VIDEOS for r in v["ids"] for w in cs.sentence_words(clean_caption(r), WORDS, v["oov"])}
    assert n_tok >= {0, 1, 2}
    assert all(REFS[k][0] == " ".join(GOLD["sentences"][k]) for k in KEYS)


def test_per_word_tokens_equal_the_paragraph_tokens():
    for _, v in VIDEOS:
        assert cs.hypothesis_tokens_per_word(v["ids"], WORDS, v["oov"]) == cs.hypothesis_tokens(v["ids"], WORDS, v["oov"]), v["key"]
    odd = ["[PAD]", "[CLS]", "[SEP]", "[VID]", "[BOS]", "[EOS]", "[UNK]", "stir-fry", "1/2", "Extra-Virgin-Oil", "café", "a.b"]
    rows = [[BOS, 7, 8, 9, EOS] + [PAD] * 5, [BOS, 10, 11, 12, EOS] + [PAD] * 5]
    assert cs.hypothesis_tokens(rows, odd, {"x--y": 12}) == cs.hypothesis_tokens_per_word(rows, odd, {"x--y": 12}) == \
        ["stir", "fry", "extra", "virgin", "oil", "caf", "a", "b", "x", "y"]


# ------------------------------------------------------------------------------------------------ 2. the compiled tables
def _check_tables(corpus):
    strings = corpus.token_strings()
    assert corpus.n_docs == 100 and corpus.log_docs == math.log(100.0) and corpus.n_tokens <= sc.CAP_LEXICON
    cider = cs.CiderCorpus(REF_TOKENS)
    ref_tok = corpus.ref_tok.numpy().view(np.uint16)
    n_grams = 0
    for i, refs in enumerate(REF_TOKENS):
        assert len(corpus.ref_slots[i]) == len(refs) and corpus.min_ref_len[i] == min(len(r) for r in refs)
        for (off, n, norms), r in zip(corpus.ref_slots[i], refs):
            ids = ref_tok[off:off + n].tolist()
            assert n == len(r) and [strings[t] for t in ids] == r
            _, ref_norms, length = cider.vec(r)
            assert all(_close(a, b) for a, b in zip(norms, ref_norms)) and length == max(n - 1, 0)
            for k in range(1, 5):
                for g, c in cs.grams(r, k).items():                               # every reference gram is found by the kernel's probe
                    key = sc.gram_key([corpus._tok[w] for w in g])
                    idf, visited = corpus.probe(key)
                    assert idf is not None and 1 <= visited <= corpus.longest_probe
                    assert corpus.df[key] == cider.df[g] and _close(idf, cider.idf(g))
                    n_grams += 1
    assert len(corpus.df) == len(cider.df) == int((corpus.table_keys != 0).sum())
    # grams absent from the table end at an empty slot
    for key in (sc.gram_key([corpus.n_tokens + 1]), sc.gram_key([1, 1, 1, 1]), sc.gram_key([2, 1])):
        if key not in corpus.df:
            assert corpus.probe(key)[0] is None
    assert [float(x) for x in corpus.gauss_host[:3]] == [1.0, math.exp(-1 / 72), math.exp(-4 / 72)] and len(corpus.gauss_host) == 1024
    return n_grams


def test_reference_corpus_tables(corpus):
    assert _check_tables(corpus) > 20000
    assert corpus.table_capacity >= 2 * len(corpus.df)
    # the vocabulary CSR
    off, tok = corpus.voc_off.numpy(), corpus.voc_tok.numpy()
    strings = corpus.token_strings()
    for i, w in enumerate(WORDS):
        assert [strings[t] for t in tok[off[i]:off[i + 1]]] == cs.parse_sent(cs.ascii_word(w))
    assert corpus.voc_expansion == 1 and sum(1 for i in range(V) if off[i] == off[i + 1]) == 16


def test_small_capacity_table_has_long_probe_chains():
    need = len(ReferenceCorpus(WORDS, REFS, device="cpu").df) + 1
    cap = 1 << (need - 1).bit_length()
    small = ReferenceCorpus(WORDS, REFS, device="cpu", table_capacity=cap)
    assert small.table_capacity == cap < 2 * need
    _check_tables(small)
    assert small.longest_probe > 8
    with pytest.raises(ValueError):
        ReferenceCorpus(WORDS, REFS, device="cpu", table_capacity=cap // 2)        # too small
    with pytest.raises(ValueError):
        ReferenceCorpus(WORDS, REFS, device="cpu", table_capacity=cap + 2)         # no power of two


def test_plan_tables_walked_like_the_kernel(corpus):
    """svpc_caption_tokens' walk over the packed tables, in Python on ids alone, gives the restatement's token lists"""
    for b in GOLD["batches"]:
        plan = corpus.plan([_video(v) for v in b["videos"]])
        assert corpus.plan([_video(v) for v in b["videos"]]) is plan              # cached: a recurring batch uploads nothing
        steps = [len(v["ids"]) for v in b["videos"]]
        assert plan.vid_off(steps) is plan.vid_off(steps) and plan.vid_off(steps).tolist() == np.cumsum([0] + steps).tolist()
        plan.check_cap(steps, b["lt"])
        strings = corpus.token_strings()
        vid, oov_off, oov_tok = (plan.section(k).numpy() for k in ("vid", "oov_off", "oov_tok"))
        norms = plan.section("ref_norm").numpy().view(np.float64).reshape(-1, 4, 4)
        voc_off, voc_tok = corpus.voc_off.numpy(), corpus.voc_tok.numpy()
        for n, v in enumerate(b["videos"]):
            n_ref, idx, X, o0 = (int(x) for x in vid[12 * n:12 * n + 4])
            assert idx == INDEX[v["key"]] and n_ref == len(REFS[v["key"]]) and X == len(v["oov"])
            for r in range(n_ref):
                off, ln, nrm = corpus.ref_slots[idx][r]
                assert (int(vid[12 * n + 4 + r]), int(vid[12 * n + 8 + r])) == (off, ln) and norms[n, r].tolist() == nrm
            toks = []
            for row in v["ids"]:
                for w in clean_caption(row):
                    if 0 <= w < V:
                        toks += voc_tok[voc_off[w]:voc_off[w + 1]].tolist()
                    elif 0 <= w - V < X:
                        toks += oov_tok[oov_off[o0 + w - V]:oov_off[o0 + w - V + 1]].tolist()
            assert [strings[t] for t in toks] == cs.hypothesis_tokens(v["ids"], WORDS, v["oov"]), v["key"]
            assert len(toks) == v["counts"][8]


# ------------------------------------------------------------------------------------------------ 3. host checks
SMALL_WORDS = ["[PAD]", "[CLS]", "[SEP]", "[VID]", "[BOS]", "[EOS]", "[UNK]", "add", "oil", "stir-fry", "1/2", "extra-virgin-olive"]
SMALL_REFS = {"a": ["add oil"], "b": ["stir fry the oil", "add oil and stir"]}


def test_value_errors():
    with pytest.raises(ValueError):
        ReferenceCorpus(SMALL_WORDS, {"a": ["add oil"], "b": ["1/2 ..."]}, device="cpu")                  # an empty reference
    with pytest.raises(ValueError):
        ReferenceCorpus(SMALL_WORDS, {"a": [" ".join(["oil"] * 1025)]}, device="cpu")                     # over 1,024 tokens
    ReferenceCorpus(SMALL_WORDS, {"a": [" ".join(["oil"] * 1024)]}, device="cpu")
    with pytest.raises(ValueError):
        ReferenceCorpus(SMALL_WORDS, {"a": ["add oil"] * 5}, device="cpu")                                # more than 4 references
    with pytest.raises(ValueError):
        ReferenceCorpus(SMALL_WORDS, {"a": []}, device="cpu")
    with pytest.raises(ValueError):
        ReferenceCorpus(SMALL_WORDS, {}, device="cpu")
    with pytest.raises(ValueError):
        ReferenceCorpus([], SMALL_REFS, device="cpu")
    with pytest.raises(ValueError):
        ReferenceCorpus({0: "a", 2: "b"}, SMALL_REFS, device="cpu")

    def name(i):                                                                   # distinct all-letter tokens
        return "".join(chr(97 + (i // 26 ** k) % 26) for k in range(4))
    full = {"v%d" % j: [" ".join(name(1024 * j + i) for i in range(1024))] for j in range(64)}
    with pytest.raises(ValueError):
        ReferenceCorpus(SMALL_WORDS, full, device="cpu")                                                  # an overfull lexicon
    corpus = ReferenceCorpus(SMALL_WORDS, SMALL_REFS, device="cpu")
    n = len(SMALL_WORDS)
    assert corpus.voc_expansion == 3
    with pytest.raises(ValueError):
        corpus.plan([])
    with pytest.raises(ValueError):
        corpus.plan([dict(key="c", oov_word_dict={})])                                                    # not in the reference set
    with pytest.raises(ValueError):
        corpus.plan([dict(key="a", oov_word_dict={"x": n - 1})])                                          # a copied id inside the vocabulary
    with pytest.raises(ValueError):
        corpus.plan([dict(key="a", oov_word_dict={"x": n + 128})])
    with pytest.raises(ValueError):
        corpus.plan([dict(key="a", oov_word_dict={"x": n, "y": n})])
    plan = corpus.plan([dict(key="a", oov_word_dict={"a-b-c-d": n}), dict(key="b", oov_word_dict={})])
    assert plan.max_expansion == [4, 3]
    plan.check_cap([4, 5], 64)                                                     # 4 · 63 · 4 = 1008, 5 · 63 · 3 = 945
    with pytest.raises(ValueError):
        plan.check_cap([5, 5], 64)                                                 # 5 · 63 · 4 = 1260 tokens could be reached
    with pytest.raises(ValueError):
        plan.check_cap([4, 6], 64)
    with pytest.raises(ValueError):
        plan.vid_off([1])
    words, ln = torch.zeros(3, 22, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.caption_tokens(torch.zeros(3, 65, dtype=torch.int32), ln, plan, [1, 2])                       # Lt > 64
    with pytest.raises(ValueError):
        ops.caption_tokens(words.to(torch.int64), ln, plan, [1, 2])
    with pytest.raises(ValueError):
        ops.caption_tokens(words, ln, plan, [2, 2])                                                       # rows do not add up
    with pytest.raises(ValueError):
        ops.caption_tokens(torch.zeros(60, 22, dtype=torch.int32), torch.zeros(60, dtype=torch.int32), plan, [30, 30])     # the cap
    tokens, tok_len = torch.zeros(2, 1024, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.caption_score_counts(tokens[:, :512].contiguous(), tok_len, plan)
    with pytest.raises(ValueError):
        ops.caption_score_counts(tokens, tok_len, plan, seen=torch.zeros(3, dtype=torch.int64))
    counts, scores = torch.zeros(2, 11, dtype=torch.int32), torch.zeros(2, 6, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.caption_score_accum(counts, scores, torch.zeros(11, dtype=torch.float64), torch.zeros(2, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.caption_score_accum(counts, scores[:, :5].contiguous(), torch.zeros(11, dtype=torch.int64), torch.zeros(2, dtype=torch.float64))


def test_no_cpu_fallback():
    corpus = ReferenceCorpus(SMALL_WORDS, SMALL_REFS, device="cpu")
    with pytest.raises(_lib.SvpcKernelError):
        CaptionScores(corpus)
    plan = corpus.plan([dict(key="a", oov_word_dict={})])
    with pytest.raises(_lib.SvpcKernelError):
        ops.caption_tokens(torch.zeros(1, 22, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), plan, [1])
    with pytest.raises(_lib.SvpcKernelError):
        ops.caption_score_counts(torch.zeros(1, 1024, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), plan)
    with pytest.raises(_lib.SvpcKernelError):
        ops.caption_score_accum(torch.zeros(1, 11, dtype=torch.int32), torch.zeros(1, 6, dtype=torch.float64),
                                torch.zeros(11, dtype=torch.int64), torch.zeros(2, dtype=torch.float64))


def test_bleu_from_totals_equals_the_restatement():
    for c, g, t, r in (([3, 1, 0, 0], [4, 2, 0, 0], 4, 4), ([5229, 3669, 2586, 1819], [6262, 6163, 6065, 5967], 6262, 6400),
                       ([0, 0, 0, 0], [0, 0, 0, 0], 0, 7)):
        assert sc.bleu_from_totals(c, g, t, r) == cs.bleu_from_counts(c, g, t, r)


def test_symbols_declared_and_exported():
    decls = _lib.declarations()
    lib = _lib.load()
    for name, n_args in (("svpc_caption_tokens", 17), ("svpc_caption_score_counts", 17), ("svpc_caption_score_accum", 6)):
        assert name in decls and len(decls[name][1]) == n_args and hasattr(lib, name), name
    assert lib.svpc_abi_version() == 2
