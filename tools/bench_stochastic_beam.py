"""Stochastic beam search throughput at BASELINE config 5 (64 videos × 12 clips, vivt, D = 768, L = 6; bf16x3 by default, hipGraph
replay): the three ways to get four candidates per sentence — beam n-best (B = 4, n_best = 4), independent samples (R = 4) and stochastic
beam search (W = 4) — on the same batch, alternating in one process, so that box-to-box spread does not enter their ratios.  All three run
the same T·4 decoder rows; a caption is one returned row.  For the sample and stochastic legs it also counts, on the last decode of
every round, the distinct clean captions per sentence (``Translator.clean_captions`` per row: the ids up to the first EOS without PAD —
once as they are, once with runs of one word collapsed, which is how consensus reads them), and asserts that the stochastic leg's uncollapsed
count is exactly its count of finite-G rows.  Prints one JSON line and writes it to --out.

    python tools/bench_stochastic_beam.py [--steps 10] [--warmup 2] [--rounds 3] [--videos 64] [--precision bf16x3] [--width 4]
                                          [--temp 1.0] [--out profiles/stochastic_beam_bench.json] [--profile]

With --profile one replayed decode of every leg runs and nothing is timed (for rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--clips", type=int, default=12)
    ap.add_argument("--precision", default="bf16x3", choices=["bf16", "bf16x3", "fp32"])
    ap.add_argument("--width", type=int, default=4)
    ap.add_argument("--temp", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stochastic_beam_bench.json"))
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args(argv)
    import torch
    import bench
    from svpc_amd import make_batch, ops, synthetic as syn
    from svpc_amd.translator import Translator
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=dev)
    W = a.width
    with torch.cuda.stream(stream):
        ops.set_precision(a.precision)
        args = bench.parse_args([])
        cfg, model = bench.build(args, dev)
        b = make_batch(cfg, n_videos=a.videos, max_steps=a.clips, n_ingr=10, n_oov=0, seed=2019, full_clips=True)
        b["_ingr_host_lists"] = (b["ingr_input_ids"].tolist(), b["ingr_masks"].tolist(), b["ingr_sep_masks"].tolist())
        for k, v in list(b.items()):
            if isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
                b[k] = [t.to(dev) for t in v]
            elif isinstance(v, torch.Tensor):
                b[k] = v.to(dev)
        O = type("O", (), {"cuda": True})
        tr = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, graph=True)

        def call(leg):
            if leg == "beam":
                return tr.translate_batch_nbest(syn.translate_inputs(b), W, W)
            if leg == "sample":
                return tr.translate_batch_sample(syn.translate_inputs(b), W, random_sampling_temp=a.temp)
            return tr.translate_batch_stochastic(syn.translate_inputs(b), W, random_sampling_temp=a.temp)

        def distinct(res, collapse):
            """→ (distinct clean captions among a sentence's live rows, live rows), summed over the batch"""
            clean = [tuple([t.cpu() for t in lst] for lst in tr.clean_captions(res[0], row=j, remove_dup=collapse)) for j in range(W)]
            live = [torch.isfinite(c).cpu() for c in res[2]]
            n_distinct = n_live = 0
            for v in range(len(res[0])):
                rows = [[(tuple(clean[j][0][v][s].tolist()), int(clean[j][1][v][s])) for j in range(W)] for s in range(res[0][v].shape[0])]
                for s, r in enumerate(rows):
                    keep = [x for j, x in enumerate(r) if live[v][s, j]]
                    n_distinct += len(set(keep))
                    n_live += len(keep)
            return n_distinct, n_live

        legs = ("beam", "sample", "stochastic")
        for leg in legs:
            for _ in range(max(1, a.warmup)):          # (the first call of a setting warms up eagerly and captures its graph)
                call(leg)
        torch.cuda.synchronize()
        if a.profile:
            for leg in legs:
                call(leg)
            torch.cuda.synchronize()
            print(json.dumps({"profiled": "one replayed decode of each of beam n-best, sample and stochastic", "width": W, "videos": a.videos}))
            return
        sent = a.videos * a.clips
        el = {leg: 0.0 for leg in legs}
        counts = {leg: [0, 0, 0] for leg in legs[1:]}  # distinct as they are, distinct collapsed, live rows
        for _ in range(a.rounds):
            for leg in legs:
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    res = call(leg)
                torch.cuda.synchronize()
                el[leg] += time.perf_counter() - t0
                if leg != "beam":
                    d0, n = distinct(res, False)
                    d1, _ = distinct(res, True)
                    if leg == "stochastic":
                        finite = sum(int(torch.isfinite(G).sum()) for G in res[4])
                        assert d0 == n == finite, "stochastic beam search returned a repeated caption: %d distinct of %d finite-G rows" % (d0, finite)
                    for i, v in enumerate((d0, d1, n)):
                        counts[leg][i] += v
        n_calls = a.rounds * a.steps
        out_legs = {}
        for leg in legs:
            out_legs[leg] = {"captions_per_s": sent * W * n_calls / el[leg], "sentences_per_s": sent * n_calls / el[leg],
                             "ms_per_batch": 1000.0 * el[leg] / n_calls}
            if leg != "beam":
                d0, d1, n = counts[leg]
                out_legs[leg].update(distinct_captions_per_sentence=d0 / (sent * a.rounds),
                                     distinct_collapsed_captions_per_sentence=d1 / (sent * a.rounds), live_rows_per_sentence=n / (sent * a.rounds))
        ratios = {"stochastic_vs_beam": out_legs["stochastic"]["sentences_per_s"] / out_legs["beam"]["sentences_per_s"],
                  "stochastic_vs_sample": out_legs["stochastic"]["sentences_per_s"] / out_legs["sample"]["sentences_per_s"],
                  "sample_vs_beam": out_legs["sample"]["sentences_per_s"] / out_legs["beam"]["sentences_per_s"]}
        line = json.dumps({"metric": "four candidates per sentence: beam n-best, samples, stochastic beam search (config 5)", "videos": a.videos,
                           "clips": a.clips, "precision": a.precision, "launch": "hipGraph replay per batch structure and setting",
                           "width": W, "temp": a.temp, "steps": a.steps, "rounds": a.rounds, "legs": out_legs, "ratios": ratios})
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
