"""Write tests/golden/caption_metrics.json: seeded random id captions and what the REFERENCE's own functions make of them.

    python tools/make_golden_caption_metrics.py --reference <path to the reference checkout> [--out tests/golden/caption_metrics.json]

Only inputs and results are recorded, no reference text:
- ``remove_dup`` (src/translate.py) and ``convert_ids_to_sentence`` (src/rtransformer/recursive_caption_dataset.py) are taken out of
  their files with ``ast`` (the FunctionDef alone is compiled and executed; the latter is called with a stub ``self`` carrying
  ``idx2word``, ``PAD``, ``IGNORE``, ``EOS_TOKEN``) because importing those modules drags in the data loader;
  ``densevid_eval/evaluateRepetition.py`` imports cleanly;
- vocabulary: the special tokens, ``.``, ``,`` and synthetic words ``w<i>``; per video 0 … 3 copied words with ids V, V + 1, …;
- a caption row: BOS, 0 … Lt − 1 tokens from a small per-caption pool (repeats and runs are frequent) that includes PAD, UNK, BOS, ``.``
  and ``,``, then EOS, then PAD fill (beam style) or junk with further EOS (greedy style);
- per video: the id rows, the OOV dictionary, the reference's sentences, and total_n / distinct_n as the reference counted them
  (``evaluate_repetition`` on the one video with the module's ``get_ngrams`` wrapped by a recorder that keeps the four dictionaries it
  returns), and that call's re1 … re4; per batch of videos ``evaluate_repetition``'s re1 … re4 over the batch;
- a caption the reference cannot score (empty, or empty after the period rule) or scores differently from the id-level definition (a
  comma first or last after the period rule: its string split yields an empty "word") is drawn again, so every recorded caption is
  inside the definition.
"""
import argparse
import ast
import contextlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from svpc_amd.synthetic import BOS, EOS, IGNORE, N_SPECIAL, PAD, UNK  # noqa: E402

SPECIAL = ["[PAD]", "[CLS]", "[SEP]", "[VID]", "[BOS]", "[EOS]", "[UNK]"]
PERIOD, COMMA = N_SPECIAL, N_SPECIAL + 1
V = 60


def function_from(path, name, inside_class=None):
    """the function ``name`` of the file at ``path``, compiled on its own"""
    tree = ast.parse(open(path).read())
    body = tree.body
    if inside_class:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == inside_class).body
    fn = next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == name)
    ns = {}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns[name]


def vocabulary():
    words = SPECIAL + [".", ","] + ["w%d" % i for i in range(V - N_SPECIAL - 2)]
    return {i: w for i, w in enumerate(words)}


def draw_row(rng, lt, n_oov, greedy_style):
    n = int(rng.integers(0, lt))                         # 0 … Lt − 1 tokens after BOS
    pool = [int(v) for v in rng.integers(N_SPECIAL + 2, V, size=int(rng.integers(1, 5)))]
    pool += [PERIOD, COMMA, int(rng.choice([PAD, UNK, BOS]))] + ([V + int(rng.integers(0, n_oov))] if n_oov else [])
    body = [pool[int(i)] for i in rng.integers(0, len(pool), size=n)]
    if n and rng.random() < 0.5:
        body[-1] = PERIOD                                # the usual caption ends with a period
    row = [BOS] + body + [EOS]
    while len(row) < lt:
        row.append(int(rng.choice([EOS, UNK, PERIOD, pool[0], PAD])) if greedy_style else PAD)
    return row[:lt]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "caption_metrics.json"))
    ap.add_argument("--seed", type=int, default=2019)
    a = ap.parse_args(argv)
    remove_dup = function_from(os.path.join(a.reference, "src", "translate.py"), "remove_dup")
    to_sentence = function_from(os.path.join(a.reference, "src", "rtransformer", "recursive_caption_dataset.py"),
                                "convert_ids_to_sentence", inside_class="RecursiveCaptionDataset")
    sys.path.insert(0, os.path.join(a.reference, "densevid_eval"))
    import evaluateRepetition as er
    idx2word = vocabulary()
    stub = type("Stub", (), dict(idx2word=idx2word, PAD=PAD, IGNORE=IGNORE, EOS_TOKEN=SPECIAL[EOS]))()
    orig = er.get_ngrams
    kept = []

    def recorder(words_pred, *dicts):
        out = orig(words_pred, *dicts)
        kept[:] = [out]
        return out
    er.get_ngrams = recorder

    def evaluate(data):
        with contextlib.redirect_stdout(io.StringIO()):
            r = er.evaluate_repetition(data, data)
        return [float(r["re%d" % n]) for n in (1, 2, 3, 4)]

    def scorable(sentence):
        """inside the id-level definition: the reference can score it, and no empty-string word appears"""
        try:
            evaluate({"v": [{"sentence": sentence}]})
        except IndexError:
            return False
        return "" not in kept[0][0]

    rng = np.random.default_rng(a.seed)
    redrawn = drawn = 0

    def video(lt, sb):
        nonlocal redrawn, drawn
        n_oov = int(rng.integers(0, 4))
        oov = {"x%d" % i: V + i for i in range(n_oov)}
        rows, sentences = [], []
        greedy_style = bool(rng.integers(0, 2))
        while len(rows) < sb:
            row = draw_row(rng, lt, n_oov, greedy_style)
            s = remove_dup(to_sentence(stub, row, oov))
            drawn += 1
            if not scorable(s):
                redrawn += 1
                continue
            rows.append(row)
            sentences.append(s)
        re_ = evaluate({"v": [{"sentence": s} for s in sentences]})
        d = kept[0]
        return dict(ids=rows, oov=oov, sentences=sentences, total=[int(sum(x.values())) for x in d], distinct=[len(x) for x in d], re=re_)

    blocks = []
    for lt, n_batches, n_vid, sb_hi in ((22, 12, 6, 12), (22, 10, 1, 16), (64, 4, 2, 16)):
        for _ in range(n_batches):
            vids = [video(lt, int(rng.integers(1, sb_hi + 1))) for _ in range(n_vid)]
            re_ = evaluate({"v%d" % i: [{"sentence": s} for s in v["sentences"]] for i, v in enumerate(vids)})
            blocks.append(dict(lt=lt, videos=vids, re=re_))
    out = dict(about="tools/make_golden_caption_metrics.py: seeded id captions and the reference's own results (strings, n-gram counts, re-n)",
               seed=a.seed, V=V, pad=PAD, eos=EOS, bos=BOS, unk=UNK, ignore=IGNORE, period_id=PERIOD, comma_id=COMMA,
               idx2word=[idx2word[i] for i in range(V)], drawn=drawn, redrawn=redrawn, batches=blocks)
    with open(a.out, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("%s: %d batches, %d videos, %d captions drawn, %d drawn again, %d bytes"
          % (a.out, len(blocks), sum(len(b["videos"]) for b in blocks), drawn, redrawn, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
