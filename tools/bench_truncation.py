"""Truncated-sampling decode throughput at BASELINE config 5 (64 videos × 12 clips, vivt, D = 768, L = 6; bf16x3 by default, hipGraph
replay): captions/s of Translator.translate_batch_sample with R samples per sentence under top-p alone (the plain path, the launches of
the parent of the truncation stages) and under each truncation rule on top of it (min-p, typical, epsilon, eta, all four), on the same
batch in the same process, with the mean size of the set a live row drew from per step (``last_sample_kept``).  Prints one JSON line.

    python tools/bench_truncation.py [--steps 10] [--warmup 2] [--videos 64] [--precision bf16x3] [--samples 4] [--temp 1.0]
                                     [--topp 0.95] [--seed 2019] [--rules topp,min_p,typical,epsilon,eta,all] [--profile-rule NAME]

--rules picks the legs and their order (a name may repeat: the later legs are reported as NAME#2, …; "topp" must be among them).

With --profile-rule NAME (one of the legs' names) only one replayed decode under that rule runs (for rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RULES = [("topp", {}),
         ("min_p", dict(min_p=0.07)),
         ("typical", dict(typical_p=0.9)),
         ("epsilon", dict(epsilon_cutoff=3e-3)),
         ("eta", dict(eta_cutoff=3e-3)),
         ("all", dict(min_p=0.07, typical_p=0.9, epsilon_cutoff=3e-3, eta_cutoff=3e-3))]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--clips", type=int, default=12)
    ap.add_argument("--precision", default="bf16x3", choices=["bf16", "bf16x3", "fp32"])
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--temp", type=float, default=1.0)
    ap.add_argument("--topp", type=float, default=0.95)
    ap.add_argument("--seed", type=int, default=2019)
    ap.add_argument("--rules", default=",".join(n for n, _ in RULES))
    ap.add_argument("--profile-rule", default="")
    a = ap.parse_args(argv)
    kw = dict(random_sampling_temp=a.temp, random_sampling_topp=a.topp)
    import torch
    import bench
    from svpc_amd import make_batch, ops, synthetic as syn
    from svpc_amd.translator import Translator
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=dev)
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

        def call(rule):
            return tr.translate_batch_sample(syn.translate_inputs(b), a.samples, seed=a.seed, **kw, **rule)

        if a.profile_rule:
            rule = dict(RULES)[a.profile_rule]
            call(rule)                                 # eager warm-up twice + capture
            torch.cuda.synchronize()
            call(rule)                                 # the replayed decode
            torch.cuda.synchronize()
            print(json.dumps({"profiled": "one replayed truncated sampling decode", "rule": a.profile_rule, "samples": a.samples,
                              "videos": a.videos, "settings": dict(kw, **rule)}))
            return
        legs = {}
        caps = a.videos * a.clips * a.samples
        for name in a.rules.split(","):
            rule = dict(RULES)[name]
            while name in legs:                        # a repeated leg: NAME#2, NAME#3, …
                base_name, _, n = name.partition("#")
                name = "%s#%d" % (base_name, int(n or 1) + 1)
            for _ in range(max(1, a.warmup)):
                call(rule)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                out = call(rule)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            leg = {"settings": rule, "captions_per_s": caps * a.steps / el, "ms_per_batch": 1000.0 * el / a.steps,
                   "mean_length": float(torch.cat([x.reshape(-1) for x in out[3]]).double().mean())}
            if tr.last_sample_kept is not None:        # the sets of the live rows (a finished row counts 0 and is left out)
                kept = tr.last_sample_kept
                leg["mean_kept_per_step"] = float(kept[kept > 0].double().mean())
            legs[name] = leg
        base = legs["topp"]["captions_per_s"]
        for v in legs.values():
            v["vs_topp"] = v["captions_per_s"] / base
        print(json.dumps({"metric": "truncated-sampling decode captions/sec (config 5)", "videos": a.videos, "clips": a.clips,
                          "precision": a.precision, "launch": "hipGraph replay per batch structure and setting", "steps": a.steps,
                          "samples": a.samples, "settings": kw, "seed": a.seed, "legs": legs}))


if __name__ == "__main__":
    main()
