"""What diverse (group) beam search costs next to the n-best decode of the same width at BASELINE config 5 (64 videos × 12 clips, vivt,
D = 768, L = 6; bf16x3, hipGraph-replayed decode).  Legs on the same batch in one process, alternating (``--rounds`` of
``--steps`` batches each):

  nbest<W>                  Translator.translate_batch_nbest(W, W) — the yardstick, unchanged;
  diverse<W>_<G>            Translator.translate_batch_diverse(W, G, λ) for (W, G) = (4, 2) and (8, 4), λ = ``--strength`` (0.5);
  diverse4_2_consensus      the (4, 2) decode + Translator.consensus on its K = 4 rows (CIDEr, paragraph scope, uniform weights).

Each leg reports its best and median round; ``diverse<W>_vs_nbest`` = captions/s of diverse<W>_<G> / captions/s of nbest<W> (the bar of
§11.4 for additions to a decode: ≥ 0.97).  One batch of every decode is checked on the host: a sentence returns W rows, each group's Bg
rows are pairwise different hypotheses in final-key order (no row drawn twice, none left out).  ``div2``: the distinct bigrams among a
sentence's K candidates over their total (the clean words up to EOS), averaged over the sentences — what the feature is for, n-best
against diverse at the same K; a recorded observation, no bar.  Prints one JSON line.

    python tools/bench_diverse.py [--steps 10] [--warmup 2] [--rounds 4] [--videos 64] [--precision bf16x3] [--strength 0.5]
"""
import json
import sys

from eval_tail_bench import alternate, arguments, config5, leg


def div2(dec, lens):
    """mean over the sentences of |distinct bigrams| / |bigrams| among the sentence's K rows (words: positions 1 … len, EOS and PAD dropped)"""
    from svpc_amd.synthetic import EOS, PAD
    shares = []
    for ids, ln in zip(dec, lens):
        ids, ln = ids.cpu().tolist(), ln.cpu().tolist()
        for rows, ns in zip(ids, ln):
            grams = []
            for y, n in zip(rows, ns):
                w = [v for v in y[1:n + 1] if v not in (EOS, PAD)]
                grams += list(zip(w[:-1], w[1:]))
            if grams:
                shares.append(len(set(grams)) / len(grams))
    return sum(shares) / max(1, len(shares))


def check_rows(dec, scores, lens, W, G):
    """every sentence has W rows; the Bg rows of a group are pairwise different and in final-key order (no length penalty: by cum)"""
    Bg = W // G
    n = 0
    for ids, sc in zip(dec, scores):
        assert ids.shape[1] == W and sc.shape[1] == W, (tuple(ids.shape), W)
        ids, sc = ids.cpu().tolist(), sc.cpu().tolist()
        for rows, cums in zip(ids, sc):
            for g in range(G):
                grp = [tuple(r) for r, c in zip(rows[g * Bg:(g + 1) * Bg], cums[g * Bg:(g + 1) * Bg]) if c != float("-inf")]
                assert len(set(grp)) == len(grp), "a hypothesis was drawn twice"
                c = cums[g * Bg:(g + 1) * Bg]
                assert all(c[k] >= c[k + 1] for k in range(Bg - 1)), c
            n += 1
    return n


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    lam = 0.5
    if "--strength" in argv:
        i = argv.index("--strength")
        lam = float(argv[i + 1])
        del argv[i:i + 2]
    a = arguments(argv)
    import torch
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
        plan = ReferenceCorpus(i2w, refs, device=dev).plan(videos, references=False)
        inputs = syn.translate_inputs(b)
        pairs = ((4, 2), (8, 4))

        def nbest(W):
            return lambda: tr.translate_batch_nbest(inputs, W, W)

        def diverse(W, G):
            return lambda: tr.translate_batch_diverse(inputs, W, G, lam)

        def diverse_consensus():
            dec, _, sc, ln = tr.translate_batch_diverse(inputs, 4, 2, lam)
            return tr.consensus(dec, plan, scores=sc, lengths=ln)
        legs_fn = tuple(x for W, G in pairs for x in (("nbest%d" % W, nbest(W)), ("diverse%d_%d" % (W, G), diverse(W, G))))
        legs_fn += (("diverse4_2_consensus", diverse_consensus),)
        for _ in range(max(1, a.warmup)):              # eager warm-up + capture, then replays
            for _, fn in legs_fn:
                fn()
        torch.cuda.synchronize()
        times = alternate(legs_fn, a.rounds, a.steps)
        legs = {k: leg(v, a) for k, v in times.items()}
        out = {"metric": "n-best and diverse (group) beam decode captions/sec at the same width (config 5)", "videos": a.videos,
               "clips": a.clips, "precision": a.precision, "launch": "hipGraph replay of the decode; the consensus selection eager",
               "steps": a.steps, "diversity_strength": lam, "order": ", ".join(k for k, _ in legs_fn) + " alternating", "legs": legs}
        checked = 0
        for W, G in pairs:
            d, n = legs["diverse%d_%d" % (W, G)], legs["nbest%d" % W]
            out["diverse%d_vs_nbest_best" % W] = d["captions_per_s_best"] / n["captions_per_s_best"]
            out["diverse%d_vs_nbest_median" % W] = d["captions_per_s_median"] / n["captions_per_s_median"]
            nd, _, ns, nl = nbest(W)()
            dd, _, ds, dl = diverse(W, G)()
            torch.cuda.synchronize()
            checked += check_rows(nd, ns, nl, W, 1) + check_rows(dd, ds, dl, W, G)
            out["div2_nbest%d" % W], out["div2_diverse%d_%d" % (W, G)] = div2(nd, nl), div2(dd, dl)
        c, d = legs["diverse4_2_consensus"], legs["diverse4_2"]
        out["consensus_vs_diverse4_median"] = c["captions_per_s_median"] / d["captions_per_s_median"]
        out["consensus_vs_nbest4_median"] = c["captions_per_s_median"] / legs["nbest4"]["captions_per_s_median"]
        out["sentences_checked_for_repeated_or_missing_rows"] = checked
        print(json.dumps(out))


if __name__ == "__main__":
    main()
