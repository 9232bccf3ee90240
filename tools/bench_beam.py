"""Beam-search decode throughput at BASELINE config 5 (64 videos × 12 clips, vivt, D = 768, L = 6; bf16x3 by default, hipGraph replay):
captions/s of Translator.translate_batch for greedy and for beam widths 1, 2, 4 on the same batch, with the encoder-side and per-iteration
milliseconds of one eager call bracketed by HIP events (an upper bound on the replayed phases).  Prints one JSON line.

    python tools/bench_beam.py [--steps 10] [--warmup 2] [--videos 64] [--precision bf16x3] [--widths 1,2,4] [--profile-width 4]

Decoding controls (Translator.translate_batch_beam's keywords): --block-ngram N, --min-length M, --length-penalty {none,avg,wu}, --alpha A.
When any is set, every beam width is timed twice in the same call, without and with them (legs beamB and beamB_ctl, and their ratio).

--block-scope paragraph (needs --block-ngram N > 0): every beam width is timed at both scopes with the same controls in the same call (legs
beamB_ctl and beamB_para, and their ratio), and each leg reports re1 … re4 of its captions: evaluateRepetition.py's per-video repeated
n-gram share (the n-grams of all of a video's chosen captions counted together, none spanning two sentences), averaged over the videos —
an observation of the synthetic random-weight model.  The eager ms per iteration of a paragraph leg is per round-iteration (S_max rounds
of Lt − 1 iterations).

With --profile-width B only one replayed decode of width B runs (for rocprofv3 --kernel-trace --stats), with the controls if given."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def caption_grams(z, n, bos, eos, pad):
    """the n-grams of one id caption: its words are the ids at positions 1 … L (L + 1 its first EOS or PAD), BOS excepted; a gram is n
    consecutive positions that are all words"""
    last = len(z) - 1
    for j in range(1, len(z)):
        if z[j] in (eos, pad):
            last = j - 1
            break
    return [tuple(z[j:j + n]) for j in range(1, last - n + 2) if bos not in z[j:j + n]]


def repetition(dec, bos, eos, pad, n_max=4):
    """re1 … re_{n_max} (evaluateRepetition.py on id captions): per video 1 − distinct / total over the n-grams of all its captions (0
    without n-grams), averaged over the videos"""
    res = {}
    caps = [[z for z in d.tolist()] for d in dec]
    for n in range(1, n_max + 1):
        vals = []
        for video in caps:
            grams = [g for z in video for g in caption_grams(z, n, bos, eos, pad)]
            vals.append(1.0 - len(set(grams)) / len(grams) if grams else 0.0)
        res["re%d" % n] = sum(vals) / len(vals)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--clips", type=int, default=12)
    ap.add_argument("--precision", default="bf16x3", choices=["bf16", "bf16x3", "fp32"])
    ap.add_argument("--widths", default="1,2,4")
    ap.add_argument("--profile-width", type=int, default=0)
    ap.add_argument("--block-ngram", type=int, default=0)
    ap.add_argument("--min-length", type=int, default=0)
    ap.add_argument("--length-penalty", default="none", choices=["none", "avg", "wu"])
    ap.add_argument("--alpha", type=float, default=0.0)
    ap.add_argument("--block-scope", default="sentence", choices=["sentence", "paragraph"])
    a = ap.parse_args(argv)
    ctl = dict(block_ngram_repeat=a.block_ngram, min_length=a.min_length, length_penalty_name=a.length_penalty, length_penalty_alpha=a.alpha)
    ctl_on = a.block_ngram > 0 or a.min_length > 0 or a.length_penalty != "none"
    para = a.block_scope == "paragraph"
    if para and a.block_ngram <= 0:
        ap.error("--block-scope paragraph needs --block-ngram N > 0")
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

        def call(tr_, width, with_ctl=False):
            if width == 0:
                return tr_.translate_batch(syn.translate_inputs(b))
            kw = dict(ctl, block_ngram_scope="paragraph") if with_ctl == "para" else (ctl if with_ctl else {})
            return tr_.translate_batch_beam(syn.translate_inputs(b), width, **kw)

        if a.profile_width:
            mode = "para" if para else ctl_on
            call(tr, a.profile_width, mode)            # eager warm-up twice + capture
            torch.cuda.synchronize()
            call(tr, a.profile_width, mode)            # the replayed decode
            torch.cuda.synchronize()
            print(json.dumps({"profiled": "one replayed beam decode", "beam": a.profile_width, "videos": a.videos,
                              "controls": ctl if ctl_on else None, "block_ngram_scope": a.block_scope}))
            return
        legs = {}
        caps = a.videos * a.clips
        runs = [(0, False)]
        for w in [int(w) for w in a.widths.split(",") if w]:
            runs += [(w, True), (w, "para")] if para else [(w, False)] + ([(w, True)] if ctl_on else [])
        for width, with_ctl in runs:
            for _ in range(max(1, a.warmup)):
                call(tr, width, with_ctl)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                call(tr, width, with_ctl)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            tr_e = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, graph=False)
            call(tr_e, width, with_ctl)
            tr_e.phase_events = []
            call(tr_e, width, with_ctl)
            torch.cuda.synchronize()
            e = tr_e.phase_events
            n_it = (cfg.max_t_len - (1 if width else 0)) * (max(b["batch_step_num"]) if with_ctl == "para" else 1)
            enc_ms, dec_ms = e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])
            name = "greedy" if width == 0 else "beam%d%s" % (width, {"para": "_para", True: "_ctl", False: ""}[with_ctl])
            legs[name] = {
                "captions_per_s": caps * a.steps / el, "ms_per_batch": 1000.0 * el / a.steps,
                "eager_encoder_side_ms": enc_ms, "eager_iterations": n_it, "eager_ms_per_iteration": dec_ms / n_it}
            if para:
                legs[name].update(repetition(call(tr, width, with_ctl)[0], syn.BOS, syn.EOS, syn.PAD))
        g = legs["greedy"]["captions_per_s"]
        for k, v in legs.items():
            v["vs_greedy"] = v["captions_per_s"] / g
            if k.endswith("_ctl") and k[:-len("_ctl")] in legs:
                v["vs_without_controls"] = v["captions_per_s"] / legs[k[:-len("_ctl")]]["captions_per_s"]
            if k.endswith("_para"):
                v["vs_sentence_scope"] = v["captions_per_s"] / legs[k[:-len("_para")] + "_ctl"]["captions_per_s"]
        print(json.dumps({"metric": "beam-search decode captions/sec (config 5)", "videos": a.videos, "clips": a.clips,
                          "precision": a.precision, "launch": "hipGraph replay per batch structure, width and controls", "steps": a.steps,
                          "controls": ctl if ctl_on else None, "block_ngram_scope": a.block_scope, "legs": legs}))


if __name__ == "__main__":
    main()
