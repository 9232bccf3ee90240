"""Ensemble decode throughput at BASELINE config 5 (64 videos × 12 clips, vivt, D = 768, L = 6; bf16x3 by default, hipGraph replay): ms per
batch and captions/s of greedy (translate_batch) and the width-B beam (translate_batch_beam) for a single Translator and for an
EnsembleTranslator of M = 2 and M = 4 members under ``combine="prob"``, plus one ``"logprob"`` leg (the largest M, beam), all on the same
batch in the same process.  Members are the benchmark's model and M − 1 more with parameters drawn from other seeds.  Every leg is timed
``--reps`` times (``--steps`` batches each): ``ms_per_batch`` is the best repetition, ``ms_spread`` = max − min over the repetitions.
``yardstick_ms`` of an M-member leg is M × the single-member ms of the same strategy; ``over_yardstick_ms`` what the leg takes beyond it
(DESIGN §11.14 sets it against the combine kernel's launches).  Prints one JSON line.

    python tools/bench_ensemble.py [--steps 10] [--warmup 2] [--reps 3] [--videos 64] [--precision bf16x3] [--members 2,4] [--beam 4]
                                   [--profile-members M]

With --profile-members M only one replayed beam decode of an M-member ensemble runs (for rocprofv3 --kernel-trace --stats)."""
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
    ap.add_argument("--members", default="2,4")
    ap.add_argument("--beam", type=int, default=4)
    ap.add_argument("--profile-members", type=int, default=0)
    a = ap.parse_args(argv)
    import torch
    import bench
    from svpc_amd import make_batch, ops, synthetic as syn
    from svpc_amd.ensemble import EnsembleTranslator
    from svpc_amd.translator import Translator
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        ops.set_precision(a.precision)
        args = bench.parse_args([])
        counts = [int(m) for m in a.members.split(",") if m]
        n_models = max(counts + [a.profile_members, 1])
        cfg, model = bench.build(args, dev)
        models = [model]
        for m in range(1, n_models):                   # further members: the same shapes, parameters from another seed
            other = bench.build(args, dev)[1]
            drawn = syn.draw_parameters(list(other.named_parameters()), seed=100 + m)
            with torch.no_grad():
                for n, p in other.named_parameters():
                    p.copy_(drawn[n].to(dev))
            models.append(other)
        b = make_batch(cfg, n_videos=a.videos, max_steps=a.clips, n_ingr=10, n_oov=0, seed=2019, full_clips=True)
        b["_ingr_host_lists"] = (b["ingr_input_ids"].tolist(), b["ingr_masks"].tolist(), b["ingr_sep_masks"].tolist())
        for k, v in list(b.items()):
            if isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
                b[k] = [t.to(dev) for t in v]
            elif isinstance(v, torch.Tensor):
                b[k] = v.to(dev)
        O = type("O", (), {"cuda": True})

        def translator(M, combine="prob"):
            if M == 1:
                return Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, graph=True)
            return EnsembleTranslator(O(), [{"model_cfg": cfg, "model": m.state_dict()} for m in models[:M]], models[:M], combine=combine,
                                      graph=True)

        def call(tr, kind):
            if kind == "greedy":
                return tr.translate_batch(syn.translate_inputs(b))
            return tr.translate_batch_beam(syn.translate_inputs(b), a.beam)

        if a.profile_members:
            tr = translator(a.profile_members)
            call(tr, "beam")                           # eager warm-up twice + capture
            torch.cuda.synchronize()
            call(tr, "beam")                           # the replayed decode
            torch.cuda.synchronize()
            print(json.dumps({"profiled": "one replayed beam decode of an ensemble", "members": a.profile_members, "beam": a.beam,
                              "videos": a.videos}))
            return
        sent = a.videos * a.clips
        legs = {}
        runs = [(1, "prob", k) for k in ("greedy", "beam")] + [(M, "prob", k) for M in counts for k in ("greedy", "beam")]
        if counts:
            runs.append((max(counts), "logprob", "beam"))
        for M, combine, kind in runs:
            tr = translator(M, combine)
            for _ in range(max(1, a.warmup)):
                call(tr, kind)
            torch.cuda.synchronize()
            times = []
            for _ in range(max(1, a.reps)):
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call(tr, kind)
                torch.cuda.synchronize()
                times.append(1000.0 * (time.perf_counter() - t0) / a.steps)
            name = "%s%s_m%d%s" % (kind, a.beam if kind == "beam" else "", M, "_logprob" if combine == "logprob" else "")
            legs[name] = {"members": M, "combine": combine, "ms_per_batch": min(times), "ms_spread": max(times) - min(times),
                          "ms_repetitions": times, "captions_per_s": sent * 1000.0 / min(times)}
            del tr
        for name, v in legs.items():
            if v["members"] > 1:
                one = legs["%s_m1" % name.split("_m")[0]]
                v["yardstick_ms"] = v["members"] * one["ms_per_batch"]
                v["over_yardstick_ms"] = v["ms_per_batch"] - v["yardstick_ms"]
                v["single_leg_spread_ms"] = one["ms_spread"]
        print(json.dumps({"metric": "ensemble decode ms per batch and captions/sec (config 5)", "videos": a.videos, "clips": a.clips,
                          "precision": a.precision, "launch": "hipGraph replay per batch structure and setting", "steps": a.steps,
                          "reps": a.reps, "beam": a.beam, "iterations": cfg.max_t_len, "legs": legs}))


if __name__ == "__main__":
    main()
