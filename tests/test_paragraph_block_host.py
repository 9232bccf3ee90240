"""Paragraph-scope n-gram blocking without a GPU: the rule of tests/paragraph_block_reference.py on hand-built rows, the host-side checks of
Translator and ops (ValueError before any device work), the controls key at both scopes, the new kernel entry point, and the reference's
self-consistency on the goldens (S_b = 1 and sentence 0 are the sentence-scope decode; no repeated gram in any paragraph)."""
import types

import numpy as np
import pytest
import torch

import beam_controls_reference as bcr
import paragraph_block_reference as pbr
from svpc_amd import ops, synthetic as syn
from svpc_amd.synthetic import BOS, EOS, PAD, UNK
from test_oracle_golden import load_case

C = 14                                          # columns of the hand-built rows (UNK = 6, EOS = 5)


def _row(best, second, C_=C):
    p = np.full((1, C_), 0.01, np.float32)
    p[0, best] = 0.6
    p[0, second] = 0.3
    return p


def _sel(p, hist, pos, history, C_=C, X=0, **ctl):
    p = np.asarray(p, np.float32)
    R = p.shape[0]
    hist = np.asarray(hist, np.int64).reshape(R, -1)
    return pbr.select_para(p, [C_] * R, [X] * R, 1, False, np.zeros(R, np.float32), np.zeros(R, bool), np.zeros(R, np.int64), hist, pos,
                           [history], **ctl)


def test_trigram_of_an_earlier_sentence_is_banned():
    history = [[BOS, 9, 10, 11, 12, EOS, PAD]]
    hist = [BOS, 8, 9, 10]                           # p = 4: gram (9, 10, w); (9, 10, 11) is a gram of sentence 0
    assert _sel(_row(11, 7), hist, 3, history, block_ngram_repeat=3)[1][0] == 7
    assert _sel(_row(11, 7), hist, 3, [], block_ngram_repeat=3)[1][0] == 11           # (no history: free)
    assert bcr.select_ctl(_row(11, 7), [C], [0], 1, False, [0.0], [False], [0], np.asarray([hist]), 3,
                          block_ngram_repeat=3)[1][0] == 11                            # (sentence scope: free)
    assert pbr.paragraph_banned_words(hist, 3, 3, set(), history) == {11}
    assert pbr.paragraph_banned_words(hist, 3, 2, set(), history) == {11}           # (10, w): (10, 11)
    assert pbr.paragraph_banned_words([BOS, 8, 9, 12], 3, 3, set(), history) == set()


def test_no_gram_spans_two_sentences():
    """the last words of sentence 0 and the first word of sentence 1 form no gram"""
    history = [[BOS, 7, 8, 9, EOS, PAD], [BOS, 10, 11, EOS, PAD, PAD]]
    assert pbr.paragraph_banned_words([BOS, 8, 9], 2, 3, set(), history) == set()  # (8, 9, 10) would span the boundary
    assert pbr.paragraph_banned_words([BOS, 9], 1, 2, set(), history) == set()       # (9, 10) likewise
    assert pbr.paragraph_banned_words([BOS, 7, 8], 2, 3, set(), history) == {9}
    assert pbr.caption_grams(history[0], 3) == [(7, 8, 9)]


def test_eos_and_pad_are_not_words():
    history = [[BOS, 7, 8, EOS, 9, 10, PAD], [BOS, 11, PAD, PAD, 12, 13, PAD]]     # (ids after the first EOS / PAD are no words)
    assert pbr.caption_words(history[0]) == [7, 8] and pbr.caption_words(history[1]) == [11]
    assert pbr.paragraph_banned_words([BOS, 8], 1, 2, set(), history) == set()       # (8, EOS) is no gram
    assert pbr.paragraph_banned_words([BOS, 9], 1, 2, set(), history) == set()       # (9, 10) lies after EOS
    assert pbr.paragraph_banned_words([BOS, 4], 1, 1, set(), history) == {7, 8, 11}  # EOS and PAD are never banned
    assert pbr.caption_words([BOS, 7, BOS, 8, EOS]) == [7, 8]                       # BOS is never a word ...
    assert pbr.caption_grams([BOS, 7, BOS, 8, EOS], 2) == []                        # ... and no gram holds it
    assert pbr.caption_words([BOS, 7, 8, 9]) == [7, 8, 9]                           # no EOS: through Lt − 1


def test_exclusion_token_saves_the_gram():
    history = [[BOS, 9, 10, 11, EOS]]
    hist = [BOS, 9, 10]
    for excl in ((9,), (10,), (11,)):
        assert _sel(_row(11, 7), hist, 2, history, block_ngram_repeat=3, exclusion_tokens=excl)[1][0] == 11, excl
    assert _sel(_row(11, 7), hist, 2, history, block_ngram_repeat=3, exclusion_tokens=(12,))[1][0] == 7
    assert pbr.paragraph_banned_words([BOS, 4], 1, 1, {10}, history) == {9, 11}


def test_copied_oov_word_in_the_history_is_a_word():
    V, X = 12, 2                                     # columns 12, 13 are copied OOV words
    history = [[BOS, 13, 8, EOS]]
    p = _row(13, 7, C_=V + X)
    _, ext, mod, _, _, _ = _sel(p, [BOS, 4], 1, history, C_=V + X, X=X)
    assert ext[0] == 13 and mod[0] == UNK
    assert _sel(p, [BOS, 4], 1, history, C_=V + X, X=X, block_ngram_repeat=1)[1][0] == 7
    assert _sel(_row(12, 7, C_=V + X), [BOS, 4], 1, history, C_=V + X, X=X, block_ngram_repeat=1)[1][0] == 12


def test_unigram_bans_every_earlier_word():
    history = [[BOS, 7, 8, EOS, PAD], [BOS, 9, 12, 10, EOS]]
    assert pbr.paragraph_banned_words([BOS], 0, 1, set(), history) == {7, 8, 9, 10, 12}
    p = np.full((1, C), 0.01, np.float32)
    p[0, [7, 8, 9, 10, 12]] = 0.5
    p[0, 11] = 0.2
    assert _sel(p, [BOS], 0, history, block_ngram_repeat=1)[1][0] == 11


def test_own_repeats_are_still_banned():
    assert _sel(_row(9, 7), [BOS, 9, 4], 2, [[BOS, 11, EOS]], block_ngram_repeat=1)[1][0] == 7


# ------------------------------------------------------------------------------------------------ host-side checks
class _Opt:
    cuda = True


def _translator(V=951, mode="full", **opt):
    from svpc_amd.translator import Translator
    tr = Translator.__new__(Translator)
    tr.incremental = True
    tr.opt = _Opt()
    for k, v in opt.items():
        setattr(tr.opt, k, v)
    tr.model_config = types.SimpleNamespace(max_t_len=22, vocab_size=V, model_mode=mode)
    return tr


BAD = [dict(block_ngram_scope="video"), dict(block_ngram_scope=1), dict(block_ngram_scope="paragraph"),
       dict(block_ngram_scope="paragraph", block_ngram_repeat=0, min_length=2)]


@pytest.mark.parametrize("bad", BAD)
def test_translator_refuses_bad_scope_before_device_work(bad):
    inputs = [None] * 12                              # never unpacked: the checks come first
    tr = _translator()
    with pytest.raises(ValueError):
        tr.translate_batch(inputs, **bad)
    with pytest.raises(ValueError):
        tr.translate_batch(inputs, use_beam=True, **bad)
    with pytest.raises(ValueError):
        tr.translate_batch_beam(inputs, 2, **bad)
    with pytest.raises(ValueError):
        tr.translate_batch_nbest(inputs, 2, 1, **bad)
    with pytest.raises(ValueError):                   # … and the same values read from opt
        _translator(**bad).translate_batch_beam(inputs, 2)


def test_translator_refuses_wide_rows_at_paragraph_scope():
    ctl = dict(block_ngram_repeat=2, block_ngram_scope="paragraph")
    with pytest.raises(ValueError):                   # V alone is too wide
        _translator(V=4097).translate_batch_beam([None] * 12, 2, **ctl)
    _translator(V=4097)._controls(dict(block_ngram_repeat=2))       # (sentence scope takes any width)
    inputs = [None] * 8 + [[{}, {i: 0 for i in range(10)}]] + [None] * 3      # V + X = 4090 + 10 > 4096: the batch's OOV words
    with pytest.raises(ValueError):
        _translator(V=4090).translate_batch_beam(inputs, 2, **ctl)
    with pytest.raises(ValueError):
        _translator(V=4090).translate_batch_nbest(inputs, 2, 1, **ctl)


def test_sampling_does_not_take_the_scope():
    with pytest.raises(TypeError):
        _translator().translate_batch_sample([None] * 12, 1, block_ngram_scope="paragraph")


def test_controls_keys_at_both_scopes():
    tr = _translator(block_ngram_repeat=3, min_length=2, exclusion_tokens=[9, 4, 9])
    c, key = tr._controls({})
    assert c["block_ngram_scope"] == "sentence" and key == (3, (4, 9), 2, "none", 0.0)
    c, key = tr._controls({"block_ngram_scope": "sentence"})
    assert key == (3, (4, 9), 2, "none", 0.0)
    c, key = tr._controls({"block_ngram_scope": "paragraph"})
    assert c["block_ngram_scope"] == "paragraph" and key == (3, (4, 9), 2, "none", 0.0, "paragraph")
    c, key = _translator(block_ngram_repeat=1, block_ngram_scope="paragraph")._controls({})
    assert key == (1, (), 0, "none", 0.0, "paragraph")
    c, key = _translator(block_ngram_scope="paragraph")._controls({"block_ngram_scope": "sentence"})    # keywords override opt
    assert key is None


def _tables_cpu(R=4, lt=8):
    scores = torch.rand(R, 20)
    cum = torch.zeros(R)
    fin = torch.zeros(R, dtype=torch.int32)
    toks = [[torch.zeros(R, lt, dtype=torch.int32) for _ in range(3)] for _ in range(2)]
    return scores, cum, fin, toks


@pytest.mark.parametrize("bad", ["n0", "lt", "dtype", "cols", "desc_len", "desc_range", "desc_neg"])
def test_ops_refuse_bad_history_before_device_work(bad):
    scores, cum, fin, toks = _tables_cpu()
    hist = torch.zeros(3, 8, dtype=torch.int32)
    desc = [0, 1, 1, 2]
    row_c = [20] * 4
    kw = dict(block_ngram_repeat=2)
    if bad == "n0":
        kw = {}
    elif bad == "lt":
        hist = torch.zeros(3, 9, dtype=torch.int32)
    elif bad == "dtype":
        hist = hist.long()
    elif bad == "cols":
        scores = torch.rand(4, 4100)
        row_c = [4097] * 4
    elif bad == "desc_len":
        desc = [0, 1]
    elif bad == "desc_range":
        desc = [0, 1, 2, 2]
    elif bad == "desc_neg":
        desc = [0, -1, 1, 1]
    with pytest.raises(ValueError):
        ops.beam_step(scores, row_c, [0] * 4, 2, 3, False, UNK, EOS, PAD, cum, fin, toks[0], toks[1], 8, history=(hist, desc, BOS), **kw)


def test_ops_check_scope():
    assert ops.check_beam_controls(22, 951, block_ngram_repeat=2, block_ngram_scope="paragraph")["block_ngram_scope"] == "paragraph"
    assert ops.check_beam_controls(22, 951)["block_ngram_scope"] == "sentence"
    for bad in (dict(block_ngram_scope="doc"), dict(block_ngram_scope="paragraph"),
                dict(block_ngram_repeat=2, block_ngram_scope="paragraph", max_cols=4097)):
        with pytest.raises(ValueError):
            ops.check_beam_controls(22, 951, **bad)
    ops.check_beam_controls(22, 951, block_ngram_repeat=2, block_ngram_scope="paragraph", max_cols=4096)


def test_library_exports_the_paragraph_entry_point():
    from svpc_amd import _lib
    decl = _lib.declarations()
    assert "svpc_beam_step_para" in decl
    assert len(decl["svpc_beam_step_para"][1]) == len(decl["svpc_beam_step_ctl"][1]) + 3
    lib = _lib.load()
    assert lib.svpc_abi_version() == 2
    assert hasattr(lib, "svpc_beam_step_para")


# ------------------------------------------------------------------------------------------------ the reference on the goldens
def _args(golden_dir, case, mt):
    z, cfg, batch, P = load_case(golden_dir, case, mt)
    P = {k: v.detach() for k, v in P.items()}
    return cfg, (P, cfg, batch["input_ids_list"], batch["video_features_list"], batch["input_masks_list"], batch["ingr_input_ids"],
                 batch["ingr_sep_masks"], batch["batch_step_num"], batch["ingr_id_dict"], batch["oov_word_dict"]), batch


@pytest.mark.parametrize("mt", ["v", "vivt"])
def test_reference_sentence_zero_and_single_sentence_videos(golden_dir, mt):
    """sentence 0 of every video is the sentence-scope decode; a later sentence decoded under an empty history is too"""
    cfg, args, batch = _args(golden_dir, "tiny", mt)
    ctl = dict(block_ngram_repeat=2, exclusion_tokens=(7,), min_length=1, length_penalty_name="avg")
    c_ids, c_cum, c_len, _ = bcr.beam_decode_ctl(*args, beam=2, **ctl)
    p_ids, p_cum, p_len, _ = pbr.beam_decode_para(*args, beam=2, **ctl)
    steps = batch["batch_step_num"]
    for v in range(len(steps)):
        assert torch.equal(p_ids[v][0], c_ids[v][0])
        np.testing.assert_array_equal(p_cum[v][0], c_cum[v][0])
        np.testing.assert_array_equal(p_len[v][0], c_len[v][0])
    empty = [[[BOS] + [PAD] * (cfg.max_t_len - 1)] * s for s in steps]       # (captions without a word: S_b = 1 for every sentence)
    e_ids, e_cum, e_len, _ = pbr.beam_decode_para(*args, beam=2, history=empty, **ctl)
    for v in range(len(steps)):
        assert torch.equal(e_ids[v], c_ids[v])
        np.testing.assert_array_equal(e_cum[v], c_cum[v])
        np.testing.assert_array_equal(e_len[v], c_len[v])


def _assert_no_repeated_gram(paragraph, n, excl=()):
    grams = [g for z in paragraph for g in pbr.caption_grams(z, n) if not set(g) & set(excl)]
    assert len(grams) == len(set(grams)), paragraph


@pytest.mark.parametrize("n,excl", [(1, ()), (2, (9,))])
def test_reference_paragraphs_repeat_no_gram(golden_dir, n, excl):
    cfg, args, batch = _args(golden_dir, "tiny", "vivt")
    p_ids, _, _, _ = pbr.beam_decode_para(*args, beam=2, block_ngram_repeat=n, exclusion_tokens=excl)
    s_ids, _, _, _ = bcr.beam_decode_ctl(*args, beam=2, block_ngram_repeat=n, exclusion_tokens=excl)
    for ids in p_ids:
        _assert_no_repeated_gram([z.tolist() for z in ids[:, 0]], n, excl)
    assert any(len(ids) > 1 for ids in p_ids)
    if n == 1:               # (the sentence scope repeats words across sentences on these fixtures: the paragraph scope changed something)
        assert any(not torch.equal(a[:, 0], b[:, 0]) for a, b in zip(p_ids, s_ids))


def test_reference_history_override_reproduces_its_own_decode(golden_dir):
    cfg, args, batch = _args(golden_dir, "tiny", "v")
    ctl = dict(block_ngram_repeat=1)
    p_ids, p_cum, _, _ = pbr.beam_decode_para(*args, beam=3, **ctl)
    hist = [[z.tolist() for z in ids[:, 0]] for ids in p_ids]
    o_ids, o_cum, _, _ = pbr.beam_decode_para(*args, beam=3, history=hist, **ctl)
    for a, b, ca, cb in zip(p_ids, o_ids, p_cum, o_cum):
        assert torch.equal(a, b)
        np.testing.assert_array_equal(ca, cb)
