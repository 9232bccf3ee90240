"""What the ingredient-F1 tail of a decode costs at BASELINE config 5 (64 videos × 12 clips, vivt, D = 768, L = 6; bf16x3, hipGraph-replayed
greedy decode).  Three legs on the same batch in one process, alternating (A B C A B C …, ``--rounds`` of ``--steps`` batches each):

  decode              Translator.translate_batch alone (the path as it was before IngredientF1 existed);
  decode_f1           translate_batch + IngredientF1.update on its result (clean → match: three launches, no read-back);
  decode_metrics_f1   translate_batch + DecodeMetrics.update + IngredientF1.update(clean=dm.last_clean): both counters on one clean-up
                      (five launches).

Ingredient names are synthesised from the batch's ``ingr_id_dict`` (word i is ``w<i>``), ground-truth sentences are seeded draws over the
same words.  Each leg reports its best and median round.  ``f1_vs_decode`` = captions/s of decode_f1 / captions/s of decode (the bar:
≥ 0.97).  The device totals of one batch are compared with the Python statement (tests/ingredient_f1_reference.py).  Prints one JSON line.

    python tools/bench_ingredient_f1.py [--steps 10] [--warmup 2] [--rounds 4] [--videos 64] [--precision bf16x3]
"""
import json

from eval_tail_bench import against_decode, alternate, arguments, config5, leg


def main(argv=None):
    a = arguments(argv)
    import numpy as np
    import torch
    import ingredient_f1_reference as ir
    from svpc_amd.ingredients import IngredientLexicon
    from svpc_amd.metrics import DecodeMetrics, IngredientF1
    with config5(a) as (cfg, dev, b, decode):
        V = cfg.vocab_size
        i2w = ["w%d" % i for i in range(V)]
        rng = np.random.default_rng(2019)
        videos, names_all = [], set()
        for d, oov, n_steps in zip(b["ingr_id_dict"], b["oov_word_dict"], b["batch_step_num"]):
            inv = {int(v): k for k, v in oov.items()}
            names = [" ".join(i2w[i] if i < V else inv[i] for i in d[e]) for e in sorted(d)]
            names_all.update(names)
            pool = [t for n in names for t in n.split(" ")] + [i2w[int(i)] for i in rng.integers(7, V, size=8)]
            gt = [" ".join(pool[int(i)] for i in rng.integers(0, len(pool), size=int(rng.integers(3, 12)))) for _ in range(int(n_steps))]
            videos.append(dict(ingredients=names, oov_word_dict=oov, gt_sentences=gt))
        all_ingredients = names_all | {i2w[int(i)] for i in rng.integers(7, V, size=V // 4)}
        lex = IngredientLexicon(i2w, all_ingredients, device=dev)
        plan = lex.plan(videos)
        f1 = IngredientF1(lex)
        dm = DecodeMetrics(V, dev)

        def decode_f1():
            dec = decode()
            f1.update(dec, plan)
            return dec

        def decode_metrics_f1():
            dec = decode()
            dm.update(dec)
            f1.update(dec, plan, clean=dm.last_clean)
            return dec

        for _ in range(max(1, a.warmup)):              # eager warm-up + capture, then replays; the updates' tables are cached
            decode_f1()
            decode_metrics_f1()
        torch.cuda.synchronize()
        f1.reset()
        legs_fn = (("decode", decode), ("decode_f1", decode_f1), ("decode_metrics_f1", decode_metrics_f1))
        times = alternate(legs_fn, a.rounds, a.steps)
        res = f1.result()                              # the epoch's single read-back
        # one batch through the device and through the Python statement: the same totals
        f1.reset()
        dec = decode_f1()
        one = f1.result()
        ref, _ = ir.epoch_result([[(d.cpu().tolist(), v) for d, v in zip(dec, videos)]], i2w, all_ingredients)
        same = all(one[k] == ref[k] for k in ("n_correct", "n_recall", "n_precision")) and all(
            abs(one[k] - ref[k]) <= 1e-12 for k in ("recall", "precision", "f1"))
        legs = {k: leg(v, a) for k, v in times.items()}
        d, u, m = (legs[k] for k in ("decode", "decode_f1", "decode_metrics_f1"))
        print(json.dumps({
            "metric": "greedy decode captions/sec with and without the ingredient-F1 tail (config 5)", "videos": a.videos, "clips": a.clips,
            "precision": a.precision, "launch": "hipGraph replay of the decode; the updates eager", "steps": a.steps,
            "order": "decode, decode_f1, decode_metrics_f1 (one shared clean-up) alternating", "legs": legs,
            **against_decode("f1", u, d), **against_decode("metrics_f1", m, d),
            "predicate_rows": lex.n_rows, "pattern_tokens_per_video_max": max(sum(len(n.split(" ")) for n in v["ingredients"]) for v in videos),
            "device_result_equals_python_statement": bool(same),
            "result": {k: res[k] for k in ("recall", "precision", "f1", "n_correct", "n_recall", "n_precision")}}))


if __name__ == "__main__":
    main()
