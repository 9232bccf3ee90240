"""``bench.py`` without ``--full`` runs the headline only: set up, warm up, time, dump, print.  Every other leg (roofline steps, ragged
legs, config-5 decode, the other arithmetic modes, the padded layout, ceilings, CPU baseline) runs only with ``--full``.  CPU check of
that dispatch: the legs are replaced by stubs that record how they were called."""
import json
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data", "config"}
FULL_KEYS = {"roofline", "secondary", "fastest_mode", "parity_mode", "padded_text_rows", "ceilings", "cpu_baseline", "ragged"}


def _fake_train_result(full, ragged):
    cfg = types.SimpleNamespace(hidden_size=768, video_feature_size=3072, num_hidden_layers=6, max_v_len=100, max_t_len=22,
                                num_attention_heads=12, vocab_size=100, action_vocab_size=10)
    # a replayed step: the roofline exists only when run_train was asked for its instrumented steps (full)
    gsum = {"work": 1e12, "ms": 10.0, "launches": 10, "bytes": 1e9, "event_overhead_ms": 0.005} if full else None
    rag = {"steps_per_s": 80.0, "clips_per_s": 12000.0, "cold": None} if ragged else None
    return dict(cfg=cfg, model=object(), ms=11.0, elapsed=0.22, final_loss=1.0, host_enqueue_ms=9.0, launch="hipGraph replay",
                text_rows="padded", degraded=None, gsum=gsum, asum=({"frac": 0.5} if full else None), glds=True, bf16_stream=True,
                rows_enc=19200, no_exchange_ms=None, ragged=rag, allreduce_bytes=0, bucket_timeline=None, n_buckets=0)


def _run(monkeypatch, capsys, argv):
    calls = {"train": [], "decode": [], "cpu": 0, "ceilings": 0}

    def run_train(args, precision, device, world, rank, dist, steps, warmup, instrument=True, ragged=0, dump_dir=None, full=False):
        calls["train"].append(dict(precision=precision, steps=steps, warmup=warmup, ragged=ragged, full=full, dump_dir=dump_dir))
        return _fake_train_result(full and instrument, ragged)

    def run_decode(cfg, model, args, device, world, rank, dist, steps, warmup, dump_dir=None, roofline=True):
        calls["decode"].append(dict(roofline=roofline))
        return {k: 1.0 for k in ("metric", "value", "unit", "ms_per_step", "steps", "warmup", "dtype", "mode", "parity", "roofline",
                                 "config")}

    def cpu_baseline(cfg, model, args, threads=None, warmup=None, steps=None):
        calls["cpu"] += 1
        return {"value": 0.1, "cores": 16}

    def measure(device, quick=False):
        calls["ceilings"] += 1
        return {}

    monkeypatch.setattr(bench, "run_train", run_train)
    monkeypatch.setattr(bench, "run_decode", run_decode)
    monkeypatch.setattr(bench, "cpu_baseline", cpu_baseline)
    monkeypatch.setitem(sys.modules, "ceilings", types.SimpleNamespace(measure=measure))
    args = bench.parse_args(argv)
    bench._train_main(args, "cpu", 1, 0, None, 1)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), calls


def test_plain_run_times_the_headline_and_nothing_else(monkeypatch, capsys):
    rec, calls = _run(monkeypatch, capsys, ["--steps", "20", "--warmup", "5", "--dump-outputs", "D"])
    assert calls["train"] == [dict(precision="bf16x3", steps=20, warmup=5, ragged=0, full=False, dump_dir="D")]
    assert calls["decode"] == [] and calls["cpu"] == 0 and calls["ceilings"] == 0
    assert set(rec) == HEADLINE_KEYS
    assert rec["steps"] == 20 and rec["warmup"] == 5 and rec["ms_per_step"] == 11.0 and rec["dtype"] == "bf16x3"
    assert rec["value"] == pytest.approx(20 / 0.22) and rec["higher_is_better"] is True
    assert rec["config"]["final_loss"] == 1.0 and rec["config"]["launch"] == "hipGraph replay"


def test_full_run_adds_every_other_leg(monkeypatch, capsys):
    rec, calls = _run(monkeypatch, capsys, ["--steps", "20", "--warmup", "5", "--full"])
    head = calls["train"][0]
    assert head == dict(precision="bf16x3", steps=20, warmup=5, ragged=20, full=True, dump_dir=None)
    assert [c["precision"] for c in calls["train"][1:]] == ["bf16", "fp32", "bf16x3"]      # fastest_mode, parity_mode, padded rows
    assert calls["decode"] == [dict(roofline=True)] * 2 and calls["cpu"] == 1 and calls["ceilings"] == 1
    assert set(rec) == HEADLINE_KEYS | FULL_KEYS
    assert rec["value"] == pytest.approx(20 / 0.22) and rec["ms_per_step"] == 11.0
    assert {"bound", "achieved", "peak", "frac", "traffic", "attention"} <= set(rec["roofline"])


def test_full_run_is_trimmed_by_its_own_switches(monkeypatch, capsys):
    rec, calls = _run(monkeypatch, capsys, ["--full", "--no-secondary", "--no-cpu-baseline"])
    assert [c["full"] for c in calls["train"]] == [True] and calls["train"][0]["ragged"] == 0
    assert calls["decode"] == [] and calls["cpu"] == 0 and calls["ceilings"] == 0
    assert set(rec) == HEADLINE_KEYS | {"roofline"}
