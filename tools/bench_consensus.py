"""What consensus (minimum Bayes risk) selection costs behind a sampling decode at BASELINE config 5 (64 videos × 12 clips, vivt, D = 768,
L = 6; bf16x3, hipGraph-replayed decode).  For K = 4 and K = 8 samples per sentence, two legs each on the same batch in
one process, alternating (``--rounds`` of ``--steps`` batches each):

  sample<K>             Translator.translate_batch_sample(num_samples=K) alone — the yardstick, unchanged;
  sample<K>_consensus   the same decode + Translator.consensus on its result (clean → tokens → pair sums → pair scores → pick and gather:
                        five launches, no read-back), ``--scope`` paragraph (default) or sentence, utility CIDEr, uniform weights.

The idf corpus is built from the synthetic labels of the batch (a video's paragraph is its steps' target words), the plan is the
reference-free one.  Each leg reports its best and median round; ``consensus<K>_vs_decode`` = captions/s of sample<K>_consensus /
captions/s of sample<K> (the bar: ≥ 0.97).  One batch's device result is compared with the Python statement
(tests/consensus_reference.py) on the first ``--check-videos`` videos.  Prints one JSON line.

    python tools/bench_consensus.py [--steps 10] [--warmup 2] [--rounds 4] [--videos 64] [--precision bf16x3] [--scope paragraph]
"""
import json
import sys

from eval_tail_bench import against_decode, alternate, arguments, config5, leg


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    extra = {"--scope": "paragraph", "--check-videos": "8"}
    for flag in list(extra):
        if flag in argv:
            i = argv.index(flag)
            extra[flag] = argv[i + 1]
            del argv[i:i + 2]
    scope, n_check = extra["--scope"], int(extra["--check-videos"])
    a = arguments(argv)
    import torch
    import caption_scores_reference as cs
    import consensus_reference as cr
    from svpc_amd import synthetic as syn
    from svpc_amd.caption_scores import ReferenceCorpus
    with config5(a) as (cfg, dev, b, decode):
        tr = decode.translator
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
            refs["vid%d" % n] = [" ".join(sents)]
            videos.append(dict(oov_word_dict=oov))
        corpus = ReferenceCorpus(i2w, refs, device=dev)
        plan = corpus.plan(videos, references=False)
        inputs = syn.translate_inputs(b)

        def sample(K):
            return lambda: tr.translate_batch_sample(inputs, num_samples=K)

        def sample_consensus(K):
            def fn():
                dec, _, sc, ln = tr.translate_batch_sample(inputs, num_samples=K)
                return dec, tr.consensus(dec, plan, scores=sc, lengths=ln, scope=scope)
            return fn
        ks = (4, 8)
        legs_fn = tuple(x for K in ks for x in (("sample%d" % K, sample(K)), ("sample%d_consensus" % K, sample_consensus(K))))
        for _ in range(max(1, a.warmup)):              # eager warm-up + capture, then replays; the group tables are cached
            for _, fn in legs_fn:
                fn()
        torch.cuda.synchronize()
        times = alternate(legs_fn, a.rounds, a.steps)
        legs = {k: leg(v, a) for k, v in times.items()}
        # one batch through the device and through the Python statement, on the first videos
        dec, res = sample_consensus(4)()
        torch.cuda.synchronize()
        cider = cs.CiderCorpus([[cs.parse_sent(p) for p in refs[k]] for k in corpus.keys])
        same, under, g = True, 0, 0
        pair, pick = res.pair_scores.cpu().tolist(), res.pick.cpu().tolist()
        for n in range(min(n_check, len(videos))):
            rows = dec[n].cpu().tolist()
            cands = [[rows[s][k] for s in range(len(rows))] for k in range(4)]
            for U, E, _ in cr.select(cands, i2w, videos[n]["oov_word_dict"], cider, scope):
                for i in range(4):
                    for j in range(4):
                        for c in range(6):
                            r = U[i][j][c]
                            same = same and abs(pair[g][i][j][c] - r) <= 1e-12 * (abs(r) if c < 4 else max(1.0, abs(r)))
                if cr.under_margin(E):
                    under += 1
                else:
                    same = same and pick[g] == cr.pick_of(E)
                g += 1
        out = {"metric": "sampling decode captions/sec with and without consensus selection (config 5)", "videos": a.videos, "clips": a.clips,
               "precision": a.precision, "launch": "hipGraph replay of the decode; the selection eager", "steps": a.steps, "scope": scope,
               "utility": "CIDEr", "weights": "uniform", "order": ", ".join(k for k, _ in legs_fn) + " alternating", "legs": legs,
               "reference_grams": len(corpus.df), "groups_compared_with_python_statement": g, "groups_under_the_pick_margin": under,
               "device_result_equals_python_statement": bool(same)}
        for K in ks:
            out.update(against_decode("consensus%d" % K, legs["sample%d_consensus" % K], legs["sample%d" % K]))
        print(json.dumps(out))


if __name__ == "__main__":
    main()
