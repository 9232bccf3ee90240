"""What lexically constrained beam search costs next to the n-best decode of the same width at BASELINE config 5 (64 videos × 12 clips,
vivt, D = 768, L = 6; bf16x3, hipGraph-replayed decode).  Legs on the same batch in one process, alternating (``--rounds``
of ``--steps`` batches each):

  nbest4            Translator.translate_batch_nbest(4, 4) — the yardstick, unchanged;
  constrained4_0    Translator.translate_batch_constrained(W = 4) with no constraints (the same captions, through the new step);
  constrained4_2    … with two phrases per sentence, one bigram and one single word, taken from a fixed-seed greedy decode of the same
                    batch so that they are generable: the words at positions 1–2 and at position 4 of the greedy caption, ids that cannot
                    be constraints (PAD, BOS, EOS, UNK) dropped.

Each leg reports its best and median round; ``constrained4_<k>_vs_nbest`` = captions/s of the leg / captions/s of nbest4 (the bar of §11.4
for additions to a decode: ≥ 0.97).  One batch is checked on the host: every sentence's row 0 has the full mask and holds each of its
phrases as a contiguous run of ids, and the leg without constraints returns the n-best rows.  Last, untimed, one
``translate_batch_diverse(4, 2, 0.5)`` batch, so that a ``rocprofv3 --kernel-trace --stats`` run of the tool shows the three width-4 step
kernels side by side.  Prints one JSON line.

    python tools/bench_constrained.py [--steps 10] [--warmup 2] [--rounds 4] [--videos 64] [--precision bf16x3]
"""
import json
import sys

from eval_tail_bench import alternate, arguments, config5, leg


def greedy_constraints(greedy, special):
    """per video, per sentence: [(y1, y2), (y4,)] of the greedy caption, ids in ``special`` dropped, empty phrases dropped"""
    out = []
    for ids in greedy:
        per_video = []
        for y in ids.cpu().tolist():
            phrases = [tuple(w for w in g if w not in special) for g in ((y[1], y[2]), (y[4],))]
            per_video.append([ph for ph in phrases if ph])
        out.append(per_video)
    return out


def check_rows(dec, mets, cons):
    """every sentence's row 0: the full mask, and each phrase as a contiguous run of its ids (a plain search) → sentences, phrases"""
    n, n_ph = 0, 0
    for ids, met, per_video in zip(dec, mets, cons):
        ids, met = ids.cpu().tolist(), met.cpu().tolist()
        for rows, m, phrases in zip(ids, met, per_video):
            assert m[0] == (1 << len(phrases)) - 1, ("row 0 misses a constraint", m[0], phrases)
            y = rows[0]
            for ph in phrases:
                assert any(y[i:i + len(ph)] == list(ph) for i in range(len(y))), ("row 0 does not hold the phrase", y, ph)
                n_ph += 1
            n += 1
    return n, n_ph


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    a = arguments(argv)
    import torch
    from svpc_amd import synthetic as syn
    with config5(a) as (cfg, dev, b, decode):
        tr = decode.translator
        inputs = syn.translate_inputs(b)
        torch.manual_seed(2019)
        greedy = tr.translate_batch(inputs)[0]
        cons = greedy_constraints(greedy, (syn.PAD, syn.BOS, syn.EOS, syn.UNK))
        none = [[None] * int(s) for s in b["batch_step_num"]]
        legs_fn = (("nbest4", lambda: tr.translate_batch_nbest(inputs, 4, 4)),
                   ("constrained4_0", lambda: tr.translate_batch_constrained(inputs, none, 4)),
                   ("constrained4_2", lambda: tr.translate_batch_constrained(inputs, cons, 4)))
        for _ in range(max(1, a.warmup)):              # eager warm-up + capture, then replays
            for _, fn in legs_fn:
                fn()
        torch.cuda.synchronize()
        times = alternate(legs_fn, a.rounds, a.steps)
        legs = {k: leg(v, a) for k, v in times.items()}
        out = {"metric": "n-best and lexically constrained beam decode captions/sec at width 4 (config 5)", "videos": a.videos,
               "clips": a.clips, "precision": a.precision, "launch": "hipGraph replay of the decode", "steps": a.steps,
               "order": ", ".join(k for k, _ in legs_fn) + " alternating", "legs": legs}
        for k in ("constrained4_0", "constrained4_2"):
            out[k + "_vs_nbest_best"] = legs[k]["captions_per_s_best"] / legs["nbest4"]["captions_per_s_best"]
            out[k + "_vs_nbest_median"] = legs[k]["captions_per_s_median"] / legs["nbest4"]["captions_per_s_median"]
        nd, _, ns, nl = legs_fn[0][1]()
        zd, _, zs, zl, zm = legs_fn[1][1]()
        cd, _, cs, cl, cm = legs_fn[2][1]()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(nd + ns + nl, zd + zs + zl)), "no constraints: not the n-best rows"
        assert all(not bool(m.any()) for m in zm)
        out["sentences_checked"], out["phrases_checked"] = check_rows(cd, cm, cons)
        out["sentences_changed_by_the_constraints"] = sum(int((x[:, 0] != y[:, 0]).any(-1).sum()) for x, y in zip(cd, nd))
        tr.translate_batch_diverse(inputs, 4, 2, 0.5)      # (untimed: a kernel trace of this run then has beam_step_groups_kernel<4> beside the two others)
        torch.cuda.synchronize()
        print(json.dumps(out))


if __name__ == "__main__":
    main()
