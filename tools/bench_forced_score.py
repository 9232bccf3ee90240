"""What forced scoring costs next to decoding at BASELINE config 5 (64 videos × 12 clips, vivt, D = 768, L = 6; bf16x3, hipGraph-replayed;
DESIGN §11.8).  Five legs on the same batch in one process, alternating (``--rounds`` of ``--steps`` batches each):

  sample<K>   Translator.translate_batch_sample(num_samples=K) alone, K = 1 and 4: Lt − 1 dependent iterations over T·K rows;
  score<K>    Translator.score_captions of those K rows alone: one decoder pass over T·K·Lt rows, then svpc_force_score;
  gold        score_captions of the batch's reference captions (Translator.gold_captions, K = 1).

Both kinds of leg share the encoder side.  Each leg reports its best and median round; ``score<K>_vs_sample<K>`` = ms per batch of
score<K> / ms per batch of sample<K> (below 1: scoring K given rows costs less than decoding K rows).  ``ops.force_score`` alone (the
score and finish launches between two device events, full-length captions; at K = 1 the gap between the two launches is most of it — a
``rocprofv3 --kernel-trace --stats`` run of this tool has the kernel by itself) gives the bytes of the (T·K·(Lt − 1), C) score rows it
reads, per second, next to the box's own device-to-device copy rate (tools/ceilings.py); one batch's scores are compared with the
sampling decode's own.  Prints one JSON line.

    python tools/bench_forced_score.py [--steps 10] [--warmup 2] [--rounds 4] [--videos 64] [--precision bf16x3]
"""
import json
import statistics
import sys

from eval_tail_bench import alternate, arguments, config5, leg


def kernel_rate(torch, ops, T, K, Lt, C, dev, iters=20):
    """svpc_force_score + svpc_force_finish alone on (T·K·Lt, C) random probability rows, every caption of full length"""
    from svpc_amd.synthetic import UNK
    R = T * K
    scores = torch.rand(R * Lt, C, device=dev)
    tgt = torch.randint(7, C, (R, Lt), dtype=torch.int32, device=dev)
    length = torch.full((R,), Lt - 1, dtype=torch.int32, device=dev)
    row_c = ops.Idx([C] * R)
    ts = []
    for i in range(iters + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.force_score(scores, row_c, tgt, length, False, UNK, max_cols=C)
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(e0.elapsed_time(e1))
    nbytes = R * (Lt - 1) * C * 4
    ms = statistics.median(ts)
    return {"rows": R * (Lt - 1), "columns": C, "bytes_read": nbytes, "ms_median": ms, "TB_per_s": nbytes / (ms * 1e-3) / 1e12}


def main(argv=None):
    a = arguments(sys.argv[1:] if argv is None else argv)
    import torch
    from svpc_amd import ops, synthetic as syn
    import ceilings
    with config5(a) as (cfg, dev, b, decode):
        tr = decode.translator
        inputs = syn.translate_inputs(b)
        ks = (1, 4)
        rows = {K: tr.translate_batch_sample(inputs, num_samples=K, seed=11) for K in ks}
        gold = tr.gold_captions(b["input_labels_list"], b["batch_step_num"])
        legs_fn = tuple(x for K in ks for x in (("sample%d" % K, lambda K=K: tr.translate_batch_sample(inputs, num_samples=K)),
                                                ("score%d" % K, lambda K=K: tr.score_captions(inputs, rows[K][0]))))
        legs_fn += (("gold", lambda: tr.score_captions(inputs, gold)),)
        for _ in range(max(1, a.warmup)):              # eager warm-up + capture, then replays
            for _, fn in legs_fn:
                fn()
        torch.cuda.synchronize()
        times = alternate(legs_fn, a.rounds, a.steps)
        legs = {k: leg(v, a) for k, v in times.items()}
        out = {"metric": "forced scoring of K given captions per sentence against a sampling decode of K rows (config 5)", "videos": a.videos,
               "clips": a.clips, "precision": a.precision, "launch": "hipGraph replay", "steps": a.steps,
               "order": ", ".join(k for k, _ in legs_fn) + " alternating", "legs": legs}
        for K in ks:
            out["score%d_vs_sample%d_best" % (K, K)] = legs["score%d" % K]["ms_per_batch_best"] / legs["sample%d" % K]["ms_per_batch_best"]
            out["score%d_vs_sample%d_median" % (K, K)] = legs["score%d" % K]["ms_per_batch_median"] / legs["sample%d" % K]["ms_per_batch_median"]
        # the decode's own scores of its rows against forced scoring of them (rows without a PAD picked as a word)
        dec, _, sc, ln = rows[4]
        got = tr.score_captions(inputs, dec)
        ids, n = torch.cat(list(dec)), torch.cat(list(ln))
        pos = torch.arange(ids.shape[-1], device=dev).view(1, 1, -1)
        clean = ~((ids == syn.PAD) & (pos >= 1) & (pos <= n.unsqueeze(-1))).any(-1)
        d = (got.cum - torch.cat(list(sc))).abs()[clean & torch.isfinite(got.cum)]
        out["rows_compared_with_the_decode"] = int(d.numel())
        out["max_abs_cum_difference_to_the_decode"] = float(d.max()) if d.numel() else 0.0
        out["lengths_equal_the_decode"] = bool((got.length.to(torch.int64) == n)[clean].all())
        T, Lt, C = int(sum(b["batch_step_num"])), cfg.max_t_len, cfg.vocab_size
        out["force_score_kernel"] = {"K%d" % K: kernel_rate(torch, ops, T, K, Lt, C, dev) for K in ks}
        out["device_copy_TB_per_s"] = ceilings.measure(dev, True).get("copy_tbps")
        print(json.dumps(out))


if __name__ == "__main__":
    main()
