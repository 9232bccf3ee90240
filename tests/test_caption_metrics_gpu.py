"""Caption clean-up and repetition / diversity counters on the MI355X: svpc_caption_clean and svpc_caption_ngram_counts against the fixture
recorded from the reference's own functions (tests/golden/caption_metrics.json) and against the Python restatement
(tests/caption_metrics_reference.py) on edge rows and seeded ragged batches; DecodeMetrics (several updates, determinism, lists that are
not one buffer, graph capture); and end to end on the outputs of the greedy, beam, n-best and sampling decodes."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import caption_metrics_reference as cm  # noqa: E402
from helpers import as_views as _as_views, build_model, host_rows as _host_rows  # noqa: E402
from svpc_amd import ops, synthetic as syn  # noqa: E402
from svpc_amd.metrics import DecodeMetrics  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, IGNORE, PAD, UNK  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
O = type("O", (), {"cuda": True})
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "caption_metrics.json")))
V, PERIOD, COMMA = GOLD["V"], GOLD["period_id"], GOLD["comma_id"]
MEANS = ("re1", "re2", "re3", "re4", "div1", "div2", "div3", "div4", "avg_sen_len")
INTS = ("num_videos", "num_sen", "num_words", "num_empty", "num_copied", "vocab_size")


def _same_result(got, ref):
    for k in INTS:
        assert got[k] == ref[k], (k, got, ref)
    for k in MEANS:
        assert abs(got[k] - ref[k]) <= 1e-12, (k, got[k], ref[k])


def _blocks(lt):
    return [b for b in GOLD["batches"] if b["lt"] == lt]


# ------------------------------------------------------------------------------------------------ 1. svpc_caption_clean
@pytest.mark.parametrize("lt", [22, 64])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("remove_dup", [True, False])
def test_clean_equals_the_fixture(lt, dtype, remove_dup):
    rows = [r for b in _blocks(lt) for v in b["videos"] for r in v["ids"]]
    ref, ref_len = cm.clean_rows(rows, lt, remove_dup=remove_dup)
    words, ln = ops.clean_captions(torch.tensor(rows, dtype=dtype, device=DEV), PAD, EOS, IGNORE, remove_dup)
    assert words.dtype == torch.int32 and ln.dtype == torch.int32
    assert words.cpu().tolist() == ref and ln.cpu().tolist() == ref_len
    if remove_dup:                                   # the reference's own strings, from the device's clean ids
        from svpc_amd.translator import ids_to_sentences
        i2w = {i: w for i, w in enumerate(GOLD["idx2word"])}
        o = 0
        for b in _blocks(lt):
            for v in b["videos"]:
                n = len(v["ids"])
                assert ids_to_sentences(words[o:o + n].cpu(), ln[o:o + n].cpu(), i2w, v["oov"]) == v["sentences"]
                o += n


def test_clean_picks_a_row_of_3d_ids():
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 12, size=(37, 3, 22))
    ids[:, :, 0] = BOS
    t = torch.from_numpy(ids).to(DEV)
    for k in range(3):
        words, ln = ops.clean_captions(t, PAD, EOS, row=k)
        ref, ref_len = cm.clean_rows(ids[:, k].tolist(), 22)
        assert words.cpu().tolist() == ref and ln.cpu().tolist() == ref_len
    words, _ = ops.clean_captions(t, PAD, EOS)                      # row=None: row 0
    assert words.cpu().tolist() == cm.clean_rows(ids[:, 0].tolist(), 22)[0]
    with pytest.raises(ValueError):
        ops.clean_captions(t, PAD, EOS, row=3)


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_clean_edge_rows(dtype):
    a, b = 20, 21
    lt = 8
    rows = [[PAD] * lt,                                           # all PAD
            [BOS, a, b, a, b, a, b, a],                           # no EOS
            [BOS, EOS, a, a, EOS, a, PAD, PAD],                   # EOS at position 1
            [BOS, a, PAD, a, EOS, PAD, PAD, PAD],                 # a run across a dropped PAD
            [IGNORE, BOS, a, IGNORE, b, EOS, IGNORE, a],          # IGNORE
            [PAD, a, b, BOS, b, UNK, UNK, EOS],                   # the first remaining token goes whatever it is; BOS / UNK are words
            [IGNORE] * lt,
            [BOS, a, a, a, a, a, a, a],
            [PAD, PAD, PAD, PAD, PAD, PAD, PAD, a],               # one token: it is the dropped first one
            [BOS, V + 2, V + 2, V + 1, EOS, EOS, a, PAD]]         # copied words collapse like any word
    for rd in (True, False):
        words, ln = ops.clean_captions(torch.tensor(rows, dtype=dtype, device=DEV), PAD, EOS, IGNORE, rd)
        ref, ref_len = cm.clean_rows(rows, lt, remove_dup=rd)
        assert words.cpu().tolist() == ref and ln.cpu().tolist() == ref_len, rd
    words, ln = ops.clean_captions(torch.tensor(rows[:5], dtype=dtype, device=DEV), PAD, EOS)
    assert ln.cpu().tolist() == [0, 7, 0, 1, 2] and words[3].cpu().tolist() == [a] + [PAD] * 7
    # Lt = 64: every lane holds a position; alternating ids keep all 63 words, equal ids keep one
    full = [[BOS] + [a, b] * 31 + [a], [BOS] + [a] * 63, [BOS] + [a, a, b] * 21]
    words, ln = ops.clean_captions(torch.tensor(full, dtype=dtype, device=DEV), PAD, EOS)
    ref, ref_len = cm.clean_rows(full, 64)
    assert words.cpu().tolist() == ref and ln.cpu().tolist() == ref_len == [63, 1, 42]


def test_clean_with_other_special_ids():
    """pad / eos / ignore are arguments: nothing is tied to the dataset's values"""
    rng = np.random.default_rng(11)
    ids = rng.integers(-2, 9, size=(50, 17))
    words, ln = ops.clean_captions(torch.from_numpy(ids).to(DEV), 3, 7, -2)
    ref, ref_len = cm.clean_rows(ids.tolist(), 17, pad=3, eos=7, ignore=-2)
    assert words.cpu().tolist() == ref and ln.cpu().tolist() == ref_len


# ------------------------------------------------------------------------------------------------ 2. svpc_caption_ngram_counts
def _counts(videos, lt, period=None, comma=None, vocab=V, bits=False):
    rows = [r for vid in videos for r in vid]
    off = np.cumsum([0] + [len(v) for v in videos]).tolist()
    words, ln = ops.clean_captions(torch.tensor(rows, dtype=torch.int64, device=DEV).view(len(rows), lt), PAD, EOS)
    vb = torch.zeros((vocab + 31) // 32, dtype=torch.int32, device=DEV) if bits else None
    c = ops.caption_ngram_counts(words, ln, off, vocab, period, comma, vocab_bits=vb)
    return c.cpu().tolist(), vb


def _bitmap_ids(vb):
    bits = vb.cpu().numpy().view(np.uint32)
    return {32 * i + j for i, x in enumerate(bits) for j in range(32) if (int(x) >> j) & 1}


@pytest.mark.parametrize("lt", [22, 64])
def test_counts_equal_the_fixture(lt):
    for b in _blocks(lt):
        videos = [v["ids"] for v in b["videos"]]
        got, _ = _counts(videos, lt, PERIOD, COMMA)
        for v, c in zip(b["videos"], got):
            assert c[:4] == v["total"] and c[4:8] == v["distinct"], (c, v["total"], v["distinct"])
        # without the punctuation ids: '.' and ',' are words
        got, _ = _counts(videos, lt)
        _, ref = cm.epoch_result(videos, V)
        assert got == ref


def _random_videos(rng, lt, steps, hi=14, n_oov=3):
    vids = []
    for s in steps:
        vid = []
        for _ in range(s):
            n = int(rng.integers(0, lt))
            body = [int(x) for x in rng.integers(PERIOD, PERIOD + hi, size=n)]
            body = [V + int(rng.integers(0, n_oov)) if rng.random() < 0.1 else x for x in body]
            if rng.random() < 0.15:
                body = []                                         # an empty caption
            row = ([BOS] + body + [EOS] + [PAD] * lt)[:lt]
            vid.append(row)
        vids.append(vid)
    return vids


def test_counts_on_ragged_batches():
    rng = np.random.default_rng(2019)
    empties = copied = 0
    for lt, steps in ((22, [1, 12, 5, 3, 16, 1, 2, 30]), (9, [7, 1, 1, 40]), (64, [3, 20, 1]), (22, [1])):
        vids = _random_videos(rng, lt, steps)
        for period, comma in ((None, None), (PERIOD, COMMA), (PERIOD, None), (None, COMMA)):
            got, vb = _counts(vids, lt, period, comma, bits=True)
            res, ref = cm.epoch_result(vids, V, period, comma)
            assert got == ref, (lt, steps, period, comma)
            seen = _bitmap_ids(vb)
            assert len(seen) == res["vocab_size"]
            assert seen == {x for vid in vids for r in vid for x in cm.clean_caption(r) if 0 <= x < V}
        empties += sum(c[10] for c in ref)
        copied += sum(c[11] for c in ref)
    assert empties > 0 and copied > 0                             # empty captions and copied words occurred


def test_counts_at_the_word_cap():
    """a video of 4096 positions (64 captions of 64 positions, all 63 words kept): the LDS arrays are full to the last caption"""
    rng = np.random.default_rng(5)
    lt = 64
    big = [[BOS] + [int(x) for x in rng.integers(PERIOD + 2, PERIOD + 6, size=63)] for _ in range(64)]
    vids = [_random_videos(rng, lt, [2])[0], big, _random_videos(rng, lt, [1])[0]]
    got, _ = _counts(vids, lt, PERIOD, COMMA)
    _, ref = cm.epoch_result(vids, V, PERIOD, COMMA)
    assert got == ref
    assert ref[1][9] > 2500                                       # (run collapse leaves ≈ 3/4 of 4032 words)
    wide = [[BOS] + [PERIOD + 2 + (i + j) % 5 for j in range(63)] for i in range(64)]          # no runs: all 4032 words in LDS
    got, _ = _counts([wide], lt)
    _, ref = cm.epoch_result([wide], V)
    assert got == ref and ref[0][9] == 64 * 63
    with pytest.raises(ValueError):
        _counts([big + [big[0]]], lt)                             # 65 · 64 positions: refused on the host


# ------------------------------------------------------------------------------------------------ 3. DecodeMetrics
def test_decode_metrics_against_the_restatement():
    rng = np.random.default_rng(8)
    lt = 22
    batches = [_random_videos(rng, lt, s) for s in ([12, 3, 1, 7], [5, 5], [12, 3, 1, 7], [16])]
    dm = DecodeMetrics(V, DEV, period_id=PERIOD, comma_id=COMMA)
    for vids in batches:
        counts = dm.update(_as_views(vids, lt))
        assert counts is dm.last_counts and counts.cpu().tolist() == cm.epoch_result(vids, V, PERIOD, COMMA)[1]
    ref, _ = cm.epoch_result([v for vids in batches for v in vids], V, PERIOD, COMMA)
    got = dm.result()
    _same_result(got, ref)
    assert len(dm._offs) == 3                                      # the recurring structure uploaded nothing
    # a second accumulator fed the same sequence: the same bits
    dm2 = DecodeMetrics(V, DEV, period_id=PERIOD, comma_id=COMMA)
    for vids in batches:
        dm2.update(_as_views(vids, lt))
    assert torch.equal(dm.acc, dm2.acc) and dm2.result() == got
    # lists that are not one buffer (separate tensors; int32 ids): one copy, the same result
    dm3 = DecodeMetrics(V, DEV, period_id=PERIOD, comma_id=COMMA)
    for vids in batches:
        dm3.update([torch.tensor(v, dtype=torch.int32, device=DEV) for v in vids])
    assert torch.equal(dm.acc, dm3.acc) and dm3.result() == got
    dm.reset()
    assert dm.result()["num_videos"] == 0 and dm.result()["vocab_size"] == 0 and dm.result()["re4"] == 0.0
    # remove_dup=False and no punctuation rule
    dm4 = DecodeMetrics(V, DEV, remove_dup=False)
    dm4.update(_as_views(batches[0], lt))
    _same_result(dm4.result(), cm.epoch_result(batches[0], V, remove_dup=False)[0])
    with pytest.raises(ValueError):
        dm4.update(_as_views(batches[0], lt), row=1)


def test_decode_metrics_on_the_fixture_batches():
    for b in GOLD["batches"]:
        dm = DecodeMetrics(V, DEV, period_id=PERIOD, comma_id=COMMA)
        dm.update(_as_views([v["ids"] for v in b["videos"]], b["lt"]))
        res = dm.result()
        for n in range(4):
            assert abs(res["re%d" % (n + 1)] - b["re"][n]) <= 1e-12, (n, res, b["re"])


def test_decode_metrics_update_captured():
    from svpc_amd.graph import capturing
    rng = np.random.default_rng(21)
    lt = 22
    steps = [12, 4, 1, 9]
    three = [_random_videos(rng, lt, steps) for _ in range(3)]
    eager = DecodeMetrics(V, DEV, period_id=PERIOD, comma_id=COMMA)
    for vids in three:
        eager.update(_as_views(vids, lt))
    dm = DecodeMetrics(V, DEV, period_id=PERIOD, comma_id=COMMA)
    static = torch.tensor([r for v in three[0] for r in v], dtype=torch.int64, device=DEV)
    views, o = [], 0
    for s in steps:
        views.append(static[o:o + s])
        o += s
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        dm.update(views)                                           # eager: caches the offsets table of this structure
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capturing(graph, stream=stream):
        dm.update(views)
    for vids in three[1:]:
        static.copy_(torch.tensor([r for v in vids for r in v], dtype=torch.int64, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert dm.last_counts.cpu().tolist() == cm.epoch_result(vids, V, PERIOD, COMMA)[1]
    assert torch.equal(dm.acc, eager.acc)
    assert dm.result() == eager.result()


# ------------------------------------------------------------------------------------------------ 4. end to end
@pytest.mark.parametrize("case", ["tiny", "c1"])
def test_decode_metrics_end_to_end(golden_dir, case):
    from svpc_amd.translator import Translator, ids_to_sentences
    z, cfg, batch, model = build_model(case, "vivt", golden_dir, DEV)
    Vm = cfg.vocab_size
    tr = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model)
    before, _ = tr.translate_batch(syn.translate_inputs(batch))
    before = [d.clone() for d in before]
    period, comma = 9, 10                                          # (any two word ids: the synthetic vocabulary has no punctuation)
    dm = DecodeMetrics(Vm, DEV, period_id=period, comma_id=comma)
    seen = []

    greedy, _ = tr.translate_batch(syn.translate_inputs(batch))
    dm.update(greedy)
    seen += _host_rows(greedy)
    for a, b in zip(before, greedy):                               # the decode itself is untouched by a live DecodeMetrics
        assert torch.equal(a, b)
    for b, d in enumerate(greedy):
        np.testing.assert_array_equal(d.cpu().numpy(), z["decode/%d" % b])

    beam, _, _ = tr.translate_batch_beam(syn.translate_inputs(batch), 2)
    dm.update(beam)
    seen += _host_rows(beam)
    nbest = tr.translate_batch_nbest(syn.translate_inputs(batch), 2, 2)[0]
    assert nbest[0].dim() == 3
    counts = dm.update(nbest, row=1)
    seen += _host_rows(nbest, 1)
    assert counts.cpu().tolist() == cm.epoch_result(_host_rows(nbest, 1), Vm, period, comma)[1]
    samples = tr.translate_batch_sample(syn.translate_inputs(batch), 2, seed=17)[0]
    dm.update(samples, row=1)
    seen += _host_rows(samples, 1)

    ref, _ = cm.epoch_result(seen, Vm, period, comma)
    got = dm.result()
    _same_result(got, ref)
    assert got["num_videos"] == 4 * len(greedy) and got["num_sen"] == 4 * sum(d.shape[0] for d in greedy)

    # Translator.clean_captions: int64 views of one buffer, equal to the restatement; the strings from them
    clean, lens = tr.clean_captions(samples, row=1)
    assert clean[0].dtype == torch.int64 and lens[0].dtype == torch.int64 and clean[0]._base is clean[-1]._base
    i2w = {i: "w%d" % i for i in range(Vm)}
    for d, c, n, oov in zip(samples, clean, lens, batch["oov_word_dict"]):
        ref_c, ref_n = cm.clean_rows(d[:, 1].cpu().tolist(), cfg.max_t_len)
        assert c.cpu().tolist() == ref_c and n.cpu().tolist() == ref_n and tuple(c.shape) == (d.shape[0], cfg.max_t_len)
        words = dict(i2w)
        words.update({int(v): k for k, v in oov.items()})
        assert ids_to_sentences(c, n, i2w, oov) == [" ".join(words[w] for w in r[:k]) for r, k in zip(ref_c, ref_n)]
