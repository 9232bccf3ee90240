"""What the evaluation tail of a decode costs at BASELINE config 5 (64 videos × 12 clips, vivt, D = 768, L = 6; bf16x3, hipGraph-replayed
greedy decode).  Three legs on the same batch in one process:

  decode          Translator.translate_batch alone (the path as it was before DecodeMetrics existed);
  decode_update   translate_batch + DecodeMetrics.update on its result (clean → count → accumulate: three launches, no read-back);
  decode_host     translate_batch + the reference-style host tail: one ``.cpu().tolist()`` per sentence (src/translate.py:81-83), then the
                  Python statement of the same clean-up and counts (tests/caption_metrics_reference.py).

``decode`` and ``decode_update`` alternate (A B A B …, ``--rounds`` of ``--steps`` batches each); each leg reports its best and median
round.  ``update_vs_decode`` = captions/s of decode_update / captions/s of decode (the bar: ≥ 0.97); ``update_share_of_batch`` is the part
of a decode_update batch that the update takes.  Prints one JSON line.

    python tools/bench_decode_metrics.py [--steps 10] [--warmup 2] [--rounds 4] [--videos 64] [--precision bf16x3] [--profile]

With --profile only a few replayed decodes + updates run (for rocprofv3 --kernel-trace --stats)."""
import json
import time

from eval_tail_bench import against_decode, alternate, arguments, config5, leg, run


def main(argv=None):
    a = arguments(argv, profile=True)
    import torch
    import caption_metrics_reference as cm
    from svpc_amd.metrics import DecodeMetrics
    with config5(a) as (cfg, dev, b, decode):
        V = cfg.vocab_size
        period, comma = 9, 10                      # (the synthetic vocabulary has no punctuation: any two word ids exercise the rule)
        dm = DecodeMetrics(V, dev, period_id=period, comma_id=comma)
        host = {"videos": []}

        def decode_update():
            dec = decode()
            dm.update(dec)
            return dec

        def decode_host():
            dec = decode()
            vids = [[step.cpu().tolist() for step in video] for video in dec]       # one blocking copy per sentence, as the reference
            host["videos"] += vids
            return dec

        for _ in range(max(1, a.warmup)):              # eager warm-up + capture, then replays; the update's offsets table is cached
            decode_update()
        torch.cuda.synchronize()
        if a.profile:
            run(decode_update, 3)
            print(json.dumps({"profiled": "three replayed decodes, each followed by DecodeMetrics.update", "videos": a.videos}))
            return
        dm.reset()
        times = alternate((("decode", decode), ("decode_update", decode_update)), a.rounds, a.steps)
        res = dm.result()                              # the epoch's single read-back
        t_host = []
        for _ in range(max(1, a.rounds // 2)):
            host["videos"] = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                decode_host()
            cm.epoch_result(host["videos"], V, period, comma)
            t_host.append(time.perf_counter() - t0)
        # one batch through both tails: the same numbers
        dm.reset()
        host["videos"] = []
        decode_update()
        decode_host()
        one, ref = dm.result(), cm.epoch_result(host["videos"], V, period, comma)[0]
        same = all(one[k] == ref[k] for k in ("num_videos", "num_sen", "num_words", "num_empty", "num_copied", "vocab_size")) and all(
            abs(one[k] - ref[k]) <= 1e-12 for k in ("re1", "re2", "re3", "re4", "div1", "div2", "div3", "div4"))
        legs = {"decode": leg(times["decode"], a), "decode_update": leg(times["decode_update"], a), "decode_host_tail": leg(t_host, a)}
        d, u, h = (legs[k] for k in ("decode", "decode_update", "decode_host_tail"))
        print(json.dumps({
            "metric": "greedy decode captions/sec with and without the evaluation tail (config 5)", "videos": a.videos, "clips": a.clips,
            "precision": a.precision, "launch": "hipGraph replay of the decode; DecodeMetrics.update eager (three launches)",
            "steps": a.steps, "order": "decode, decode_update alternating; decode_host_tail afterwards", "legs": legs,
            **against_decode("update", u, d),
            "update_share_of_batch": 1.0 - d["ms_per_batch_median"] / u["ms_per_batch_median"],
            "host_tail_vs_decode_best": h["captions_per_s_best"] / d["captions_per_s_best"],
            "host_tail_ms_per_batch": h["ms_per_batch_median"] - d["ms_per_batch_median"],
            "device_result_equals_host_tail": bool(same),
            "result": {k: res[k] for k in ("re1", "re2", "re3", "re4", "div1", "div2", "num_sen", "avg_sen_len", "vocab_size")}}))


if __name__ == "__main__":
    main()
