"""Caption clean-up and repetition / diversity counters without a GPU: the Python restatement (tests/caption_metrics_reference.py) against
the fixture recorded from the reference's own functions (tests/golden/caption_metrics.json, tools/make_golden_caption_metrics.py), the
host checks of ops.check_caption_metrics, the no-CPU-fallback rule, and the C-ABI declarations."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import caption_metrics_reference as cm  # noqa: E402
from svpc_amd import _lib, ops  # noqa: E402
from svpc_amd.metrics import DecodeMetrics  # noqa: E402
from svpc_amd.synthetic import BOS, EOS, IGNORE, PAD  # noqa: E402
from svpc_amd.translator import ids_to_sentences  # noqa: E402

GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "caption_metrics.json")))
I2W = {i: w for i, w in enumerate(GOLD["idx2word"])}
V, PERIOD, COMMA = GOLD["V"], GOLD["period_id"], GOLD["comma_id"]


def test_fixture_covers_the_definition():
    assert (GOLD["pad"], GOLD["eos"], GOLD["bos"], GOLD["ignore"]) == (PAD, EOS, BOS, IGNORE)
    assert {b["lt"] for b in GOLD["batches"]} == {22, 64}
    rows = [r for b in GOLD["batches"] for v in b["videos"] for r in v["ids"]]
    assert len(rows) >= 500
    with_eos = [r for r in rows if EOS in r]
    assert len(with_eos) < len(rows)                                     # captions that fill the row: no EOS
    assert any(PAD in r[1:r.index(EOS)] for r in with_eos)               # PAD in the middle of a caption
    assert any(r[-1] == PAD for r in with_eos) and any(EOS in r[r.index(EOS) + 1:] for r in with_eos)     # both fill styles
    assert any(x >= V for r in rows for x in r) and any(PERIOD in r for r in rows) and any(COMMA in r for r in rows)
    assert {len(v["ids"]) for b in GOLD["batches"] for v in b["videos"]} >= {1, 16}


def test_strings_equal_the_reference():
    n = 0
    for b in GOLD["batches"]:
        for v in b["videos"]:
            clean, lens = cm.clean_rows(v["ids"], b["lt"])
            assert all(len(r) == b["lt"] for r in clean) and all(0 <= k < b["lt"] for k in lens)
            assert ids_to_sentences(clean, lens, I2W, v["oov"]) == v["sentences"]
            assert ids_to_sentences(torch.tensor(clean), torch.tensor(lens), I2W, v["oov"]) == v["sentences"]
            n += len(lens)
    assert n >= 500


def test_counts_equal_the_reference():
    for b in GOLD["batches"]:
        res, rows = cm.epoch_result([v["ids"] for v in b["videos"]], V, PERIOD, COMMA)
        for v, c in zip(b["videos"], rows):
            assert c[:4] == v["total"] and c[4:8] == v["distinct"], (c, v["total"], v["distinct"])
            re_, div = cm.ratios(c)
            for n in range(4):
                assert abs(re_[n] - v["re"][n]) <= 1e-12
                assert div[n] == (v["distinct"][n] / v["total"][0] if v["total"][0] else 0.0)
            assert c[8] == len(v["ids"]) and c[10] == 0              # (the reference cannot score an empty caption: none recorded)
        for n in range(4):
            assert abs(res["re%d" % (n + 1)] - b["re"][n]) <= 1e-12, (n, res, b["re"])
        assert res["num_videos"] == len(b["videos"])


def test_restatement_edge_rows():
    a, b_ = 20, 21
    assert cm.clean_caption([PAD] * 6) == []
    assert cm.clean_caption([BOS, a, b_, a, b_, a]) == [a, b_, a, b_, a]           # no EOS: everything after the first token
    assert cm.clean_caption([BOS, EOS, a, a, EOS, a]) == []                        # EOS at position 1
    assert cm.clean_caption([BOS, a, PAD, a, EOS, PAD]) == [a]                     # a run across a dropped PAD
    assert cm.clean_caption([BOS, a, PAD, a, EOS, PAD], remove_dup=False) == [a, a]
    assert cm.clean_caption([IGNORE, BOS, a, IGNORE, b_, EOS]) == [a, b_]          # the first REMAINING token is dropped
    assert cm.clean_caption([PAD, a, b_, BOS, b_, EOS]) == [b_, BOS, b_]           # whatever the first token is; BOS later is a word
    assert cm.repetition_words([a, COMMA, b_, PERIOD], PERIOD, COMMA) == [a, b_]
    assert cm.repetition_words([a, PERIOD, PERIOD], PERIOD, COMMA) == [a, PERIOD]  # one period only
    assert cm.repetition_words([PERIOD], PERIOD, COMMA) == []
    assert cm.repetition_words([a, COMMA, b_, PERIOD]) == [a, COMMA, b_, PERIOD]   # no rule by default
    c = cm.video_counts([[a, b_, a, b_], [a, b_], []], V)
    assert c == [6, 4, 2, 1, 2, 2, 2, 1, 3, 6, 1, 0]                               # no gram spans two captions
    assert cm.ratios([0] * 12) == ([0.0] * 4, [0.0] * 4)


def test_check_caption_metrics_errors():
    ops.check_caption_metrics(64, torch.int64, steps=[64, 1, 0], k=3, row=2, period_id=7, comma_id=8)
    assert ops.check_caption_metrics(22) == (0, -(1 << 31), -(1 << 31))
    with pytest.raises(ValueError):
        ops.check_caption_metrics(65)
    with pytest.raises(ValueError):
        ops.check_caption_metrics(0)
    with pytest.raises(ValueError):
        ops.check_caption_metrics(22, steps=[12, 187])               # 187 · 22 > 4096
    with pytest.raises(ValueError):
        ops.check_caption_metrics(22, torch.int16)
    with pytest.raises(ValueError):
        ops.check_caption_metrics(22, torch.float32)
    with pytest.raises(ValueError):
        ops.check_caption_metrics(22, k=3, row=3)
    with pytest.raises(ValueError):
        ops.check_caption_metrics(22, row=1)                          # a 2-D result has one row per sentence
    with pytest.raises(ValueError):
        ops.check_caption_metrics(22, k=3, row=-1)
    with pytest.raises(ValueError):
        ops.check_caption_metrics(22, period_id=7, comma_id=7)
    with pytest.raises(ValueError):
        ops.check_caption_metrics(22, period_id=-3)
    # the same checks through the entry points, before any device work
    with pytest.raises(ValueError):
        ops.clean_captions(torch.zeros(3, 65, dtype=torch.int64), PAD, EOS)
    with pytest.raises(ValueError):
        ops.clean_captions(torch.zeros(3, 22, dtype=torch.int16), PAD, EOS)
    with pytest.raises(ValueError):
        ops.clean_captions(torch.zeros(3, 2, 22, dtype=torch.int64), PAD, EOS, row=2)
    with pytest.raises(ValueError):
        ops.caption_ngram_counts(torch.zeros(400, 22, dtype=torch.int32), torch.zeros(400, dtype=torch.int32), [0, 200, 400], V)
    with pytest.raises(ValueError):
        DecodeMetrics(V, device="cuda", period_id=7, comma_id=7)


def test_no_cpu_fallback():
    with pytest.raises(_lib.SvpcKernelError):
        DecodeMetrics(V, device="cpu")
    with pytest.raises(_lib.SvpcKernelError):
        ops.clean_captions(torch.zeros(3, 22, dtype=torch.int64), PAD, EOS)
    with pytest.raises(_lib.SvpcKernelError):
        ops.caption_ngram_counts(torch.zeros(4, 22, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), [0, 4], V)


def test_stack_captions_views_and_copies():
    buf = torch.arange(7 * 22, dtype=torch.int64).view(7, 22)
    views = [buf[0:3], buf[3:4], buf[4:7]]
    flat, steps = ops.stack_captions(views)
    assert steps == [3, 1, 3] and flat.data_ptr() == buf.data_ptr() and torch.equal(flat, buf)
    flat, steps = ops.stack_captions([buf[0:3], buf[4:7]])               # a gap: one copy
    assert steps == [3, 3] and flat.data_ptr() != buf.data_ptr() and torch.equal(flat, torch.cat([buf[0:3], buf[4:7]]))
    flat, _ = ops.stack_captions([v.clone() for v in views])               # separate tensors: one copy
    assert torch.equal(flat, buf)
    b3 = torch.arange(5 * 2 * 22, dtype=torch.int64).view(5, 2, 22)
    flat, steps = ops.stack_captions([b3[1:3], b3[3:5]])                   # views that start inside the buffer
    assert steps == [2, 2] and flat.data_ptr() == b3[1].data_ptr() and torch.equal(flat, b3[1:])
    with pytest.raises(ValueError):
        ops.stack_captions([buf[0:3], b3[0:1]])
    with pytest.raises(ValueError):
        ops.stack_captions([])


def test_symbols_declared_and_exported():
    decls = _lib.declarations()
    lib = _lib.load()
    for name in ("svpc_caption_clean", "svpc_caption_ngram_counts", "svpc_decode_metric_accum"):
        assert name in decls, name
        assert hasattr(lib, name), name
    assert lib.svpc_abi_version() == 2
