"""Contrastive-decoding throughput at BASELINE config 5 (64 videos × 12 clips, vivt, D = 768, L = 6; bf16x3 by default, hipGraph replay): ms
per batch and captions/s of greedy (translate_batch) and the width-B beam (translate_batch_beam) under

- ``ContrastTranslator`` with a separate amateur (the benchmark's model against one with parameters drawn from another seed),
- ``ContrastTranslator`` with the expert as its own amateur over zero clip features (``amateur_video="zero"``),
- the yardstick: ``EnsembleTranslator`` of the same two models under ``combine="logprob"`` — two decoder sides per step as well, its
  combine kernel one sweep shorter,

all on the same batch in the same process.  The repetitions are INTERLEAVED (every repetition times every leg once, ``--steps`` batches
each), so a drift of the machine falls on all legs alike: ``ms_per_batch`` is the best repetition, ``ms_spread`` = max − min over the
repetitions, ``ratio_to_ensemble`` = the ensemble's ms over the leg's (captions/s relative to the yardstick; < 1: slower) and
``ratio_spread`` the same ratio's max − min over the repetitions.  The self-amateur runs the encoder side twice over ONE module, as
the separate amateur runs two modules' once each: its extra encoder pass is part of its ms.  Prints one JSON line; ``--out`` also
writes it to a file.

    python tools/bench_contrast_decode.py [--steps 10] [--warmup 2] [--reps 3] [--videos 64] [--precision bf16x3] [--beam 4] [--out F]
                                          [--profile self|separate]

With --profile only one replayed beam decode of that translator runs (for rocprofv3 --kernel-trace --stats)."""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--clips", type=int, default=12)
    ap.add_argument("--precision", default="bf16x3", choices=["bf16", "bf16x3", "fp32"])
    ap.add_argument("--beam", type=int, default=4)
    ap.add_argument("--beta", type=float, default=0.5)
    ap.add_argument("--alpha", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", default=None, choices=["self", "separate"])
    a = ap.parse_args(argv)
    import torch
    import bench
    from svpc_amd import make_batch, ops, synthetic as syn
    from svpc_amd.contrast_decode import ContrastTranslator
    from svpc_amd.ensemble import EnsembleTranslator
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        ops.set_precision(a.precision)
        args = bench.parse_args([])
        cfg, model = bench.build(args, dev)
        other = bench.build(args, dev)[1]              # the separate amateur: the same shapes, parameters from another seed
        drawn = syn.draw_parameters(list(other.named_parameters()), seed=101)
        with torch.no_grad():
            for n, p in other.named_parameters():
                p.copy_(drawn[n].to(dev))
        b = make_batch(cfg, n_videos=a.videos, max_steps=a.clips, n_ingr=10, n_oov=0, seed=2019, full_clips=True)
        b["_ingr_host_lists"] = (b["ingr_input_ids"].tolist(), b["ingr_masks"].tolist(), b["ingr_sep_masks"].tolist())
        for k, v in list(b.items()):
            if isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
                b[k] = [t.to(dev) for t in v]
            elif isinstance(v, torch.Tensor):
                b[k] = v.to(dev)
        O = type("O", (), {"cuda": True})

        def ck(m):
            return {"model_cfg": cfg, "model": m.state_dict()}

        def translator(name):
            if name == "ensemble2_logprob":
                return EnsembleTranslator(O(), [ck(model), ck(other)], [model, other], combine="logprob", graph=True)
            if name == "contrast_separate":
                return ContrastTranslator(O(), ck(model), model, ck(other), other, beta=a.beta, alpha=a.alpha, graph=True)
            return ContrastTranslator(O(), ck(model), model, beta=a.beta, alpha=a.alpha, amateur_video="zero", graph=True)

        def call(tr, kind):
            if kind == "greedy":
                return tr.translate_batch(syn.translate_inputs(b))
            return tr.translate_batch_beam(syn.translate_inputs(b), a.beam)

        if a.profile:
            tr = translator("contrast_" + a.profile)
            call(tr, "beam")                           # eager warm-up twice + capture
            torch.cuda.synchronize()
            call(tr, "beam")                           # the replayed decode
            torch.cuda.synchronize()
            print(json.dumps({"profiled": "one replayed beam decode under ContrastTranslator", "amateur": a.profile, "beam": a.beam,
                              "videos": a.videos}))
            return
        sent = a.videos * a.clips
        names = ["ensemble2_logprob", "contrast_separate", "contrast_self_zero"]
        kinds = ["greedy", "beam"]
        trs = {(n, k): translator(n) for n in names for k in kinds}       # one translator per leg: its graph stays captured
        for key, tr in trs.items():
            for _ in range(max(1, a.warmup)):
                call(tr, key[1])
        torch.cuda.synchronize()
        times = {key: [] for key in trs}
        for _ in range(max(1, a.reps)):                 # interleaved: every repetition times every leg once
            for key, tr in trs.items():
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call(tr, key[1])
                torch.cuda.synchronize()
                times[key].append(1000.0 * (time.perf_counter() - t0) / a.steps)
        legs = {}
        for (n, k), ts in times.items():
            name = "%s%s_%s" % (k, a.beam if k == "beam" else "", n)
            base = times[("ensemble2_logprob", k)]
            ratios = [e / t for e, t in zip(base, ts)]
            legs[name] = {"ms_per_batch": min(ts), "ms_spread": max(ts) - min(ts), "ms_repetitions": ts,
                          "captions_per_s": sent * 1000.0 / min(ts), "ratio_to_ensemble": min(base) / min(ts),
                          "ratio_repetitions": ratios, "ratio_spread": max(ratios) - min(ratios)}
        line = json.dumps({"metric": "contrastive decode ms per batch and captions/sec against the two-member logprob ensemble (config 5)",
                           "videos": a.videos, "clips": a.clips, "precision": a.precision,
                           "launch": "hipGraph replay per batch structure and setting", "steps": a.steps, "reps": a.reps, "beam": a.beam,
                           "beta": a.beta, "alpha": a.alpha, "iterations": cfg.max_t_len, "legs": legs})
        print(line)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
