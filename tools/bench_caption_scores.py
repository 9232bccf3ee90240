"""What the Bleu / ROUGE_L / CIDEr tail of a decode costs at BASELINE config 5 (64 videos × 12 clips, vivt, D = 768, L = 6; bf16x3,
hipGraph-replayed greedy decode).  Three legs on the same batch in one process, alternating (A B C A B C …, ``--rounds`` of ``--steps``
batches each):

  decode                  Translator.translate_batch alone (the path as it was before CaptionScores existed);
  decode_scores           translate_batch + CaptionScores.update on its result (clean → tokens → counts → accumulate: four launches, no
                          read-back);
  decode_metrics_scores   translate_batch + DecodeMetrics.update + CaptionScores.update(clean=dm.last_clean): both counters on one clean-up.

The references are the synthetic labels of the batch (a video's paragraph is its steps' target words; every second video gets a second
reference); vocabulary word i is an all-letter name.  Each leg reports its best and median round.  ``scores_vs_decode`` = captions/s of
decode_scores / captions/s of decode (the bar: ≥ 0.97).  The device result of one batch is compared with the Python statement
(tests/caption_scores_reference.py).  Prints one JSON line.

    python tools/bench_caption_scores.py [--steps 10] [--warmup 2] [--rounds 4] [--videos 64] [--precision bf16x3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--clips", type=int, default=12)
    ap.add_argument("--precision", default="bf16x3", choices=["bf16", "bf16x3", "fp32"])
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    import bench
    import caption_scores_reference as cs
    from svpc_amd import make_batch, ops, synthetic as syn
    from svpc_amd.caption_scores import ReferenceCorpus
    from svpc_amd.metrics import CaptionScores, DecodeMetrics
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
        V = cfg.vocab_size
        special = ["[PAD]", "[CLS]", "[SEP]", "[VID]", "[BOS]", "[EOS]", "[UNK]"]
        i2w = special + ["".join(chr(97 + (i // 26 ** k) % 26) for k in range(3)) for i in range(len(special), V)]
        refs, videos = {}, []
        for n, (oov, n_steps) in enumerate(zip(b["oov_word_dict"], b["batch_step_num"])):
            inv = {int(v): k for k, v in oov.items()}
            sents = []
            for s in range(int(n_steps)):
                lab = b["input_labels_list"][s][n].cpu().tolist()
                sents.append(" ".join(i2w[x] if x < V else inv[x] for x in lab if x not in (syn.IGNORE, syn.EOS, syn.PAD)))
            refs["vid%d" % n] = [" ".join(sents)] + ([" ".join(sents[::-1])] if n % 2 else [])
            videos.append(dict(key="vid%d" % n, oov_word_dict=oov))
        corpus = ReferenceCorpus(i2w, refs, device=dev)
        plan = corpus.plan(videos)
        scores = CaptionScores(corpus)
        dm = DecodeMetrics(V, dev)

        def decode():
            return tr.translate_batch(syn.translate_inputs(b))[0]

        def decode_scores():
            dec = decode()
            scores.update(dec, plan)
            return dec

        def decode_metrics_scores():
            dec = decode()
            dm.update(dec)
            scores.update(dec, plan, clean=dm.last_clean)
            return dec

        def run(fn, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        for _ in range(max(1, a.warmup)):              # eager warm-up + capture, then replays; the updates' tables are cached
            decode_scores()
            decode_metrics_scores()
        torch.cuda.synchronize()
        sent = a.videos * a.clips
        scores.reset()
        legs_fn = (("decode", decode), ("decode_scores", decode_scores), ("decode_metrics_scores", decode_metrics_scores))
        times = {k: [] for k, _ in legs_fn}
        for _ in range(a.rounds):
            for name, fn in legs_fn:
                times[name].append(run(fn, a.steps))
        res = scores.result()                              # the epoch's single read-back
        # one batch through the device and through the Python statement: the same totals
        scores.reset()
        dec = decode_scores()
        one = scores.result()
        ref_tokens = [[cs.parse_sent(p) for p in refs[k]] for k in corpus.keys]
        ref, _ = cs.corpus_result({n: cs.hypothesis_tokens(d.cpu().tolist(), i2w, v["oov_word_dict"]) for n, (d, v) in
                                   enumerate(zip(dec, videos))}, ref_tokens)
        same = all(one[k] == ref[k] for k in ("num_videos", "testlen", "reflen", "correct", "guess")) and all(
            abs(one[k] - ref[k]) <= 1e-12 * max(1.0, abs(ref[k])) for k in CaptionScores.KEYS)

        def leg(ts):
            return {"captions_per_s_best": sent * a.steps / min(ts), "captions_per_s_median": sent * a.steps / statistics.median(ts),
                    "ms_per_batch_best": 1000.0 * min(ts) / a.steps, "ms_per_batch_median": 1000.0 * statistics.median(ts) / a.steps,
                    "rounds": len(ts)}
        legs = {k: leg(v) for k, v in times.items()}
        d, u, m = (legs[k] for k in ("decode", "decode_scores", "decode_metrics_scores"))
        print(json.dumps({
            "metric": "greedy decode captions/sec with and without the Bleu / ROUGE_L / CIDEr tail (config 5)", "videos": a.videos, "clips": a.clips,
            "precision": a.precision, "launch": "hipGraph replay of the decode; the updates eager", "steps": a.steps,
            "order": "decode, decode_scores, decode_metrics_scores (one shared clean-up) alternating", "legs": legs,
            "scores_vs_decode_best": u["captions_per_s_best"] / d["captions_per_s_best"],
            "scores_vs_decode_median": u["captions_per_s_median"] / d["captions_per_s_median"],
            "scores_ms_per_batch": u["ms_per_batch_median"] - d["ms_per_batch_median"],
            "metrics_scores_vs_decode_best": m["captions_per_s_best"] / d["captions_per_s_best"],
            "metrics_scores_vs_decode_median": m["captions_per_s_median"] / d["captions_per_s_median"],
            "metrics_scores_ms_per_batch": m["ms_per_batch_median"] - d["ms_per_batch_median"],
            "reference_grams": len(corpus.df), "table_capacity": corpus.table_capacity, "lexicon_tokens": corpus.n_tokens,
            "device_result_equals_python_statement": bool(same),
            "result": res}))


if __name__ == "__main__":
    main()
