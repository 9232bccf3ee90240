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
import json

from eval_tail_bench import against_decode, alternate, arguments, config5, leg


def main(argv=None):
    a = arguments(argv)
    import torch
    import caption_scores_reference as cs
    from svpc_amd import synthetic as syn
    from svpc_amd.caption_scores import ReferenceCorpus
    from svpc_amd.metrics import CaptionScores, DecodeMetrics
    with config5(a) as (cfg, dev, b, decode):
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

        def decode_scores():
            dec = decode()
            scores.update(dec, plan)
            return dec

        def decode_metrics_scores():
            dec = decode()
            dm.update(dec)
            scores.update(dec, plan, clean=dm.last_clean)
            return dec

        for _ in range(max(1, a.warmup)):              # eager warm-up + capture, then replays; the updates' tables are cached
            decode_scores()
            decode_metrics_scores()
        torch.cuda.synchronize()
        scores.reset()
        legs_fn = (("decode", decode), ("decode_scores", decode_scores), ("decode_metrics_scores", decode_metrics_scores))
        times = alternate(legs_fn, a.rounds, a.steps)
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
        legs = {k: leg(v, a) for k, v in times.items()}
        d, u, m = (legs[k] for k in ("decode", "decode_scores", "decode_metrics_scores"))
        print(json.dumps({
            "metric": "greedy decode captions/sec with and without the Bleu / ROUGE_L / CIDEr tail (config 5)", "videos": a.videos, "clips": a.clips,
            "precision": a.precision, "launch": "hipGraph replay of the decode; the updates eager", "steps": a.steps,
            "order": "decode, decode_scores, decode_metrics_scores (one shared clean-up) alternating", "legs": legs,
            **against_decode("scores", u, d), **against_decode("metrics_scores", m, d),
            "reference_grams": len(corpus.df), "table_capacity": corpus.table_capacity, "lexicon_tokens": corpus.n_tokens,
            "device_result_equals_python_statement": bool(same),
            "result": res}))


if __name__ == "__main__":
    main()
