"""Beam search without a GPU: the CPU reference (tests/beam_reference.py) against the oracle's greedy decode at B = 1, its selection
rule on hand-made tables, and the kernel library's new entry points."""
import numpy as np
import pytest
import torch

import beam_reference as br
from oracle import svpc_oracle as orc
from svpc_amd.synthetic import EOS, PAD, UNK
from test_oracle_golden import load_case

NEG = -np.inf


@pytest.mark.parametrize("case,mt", [("tiny", "v"), ("tiny", "vi"), ("tiny", "viv"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")])
def test_reference_at_width_one_is_greedy(golden_dir, case, mt):
    """B = 1 ranks by (cum, raw value, column): log and + are monotone, so it picks greedy's arg-max — up to the first EOS, PAD after."""
    z, cfg, batch, P = load_case(golden_dir, case, mt)
    P = {k: v.detach() for k, v in P.items()}
    args = (P, cfg, batch["input_ids_list"], batch["video_features_list"], batch["input_masks_list"], batch["ingr_input_ids"],
            batch["ingr_sep_masks"], batch["batch_step_num"], batch["ingr_id_dict"], batch["oov_word_dict"])
    greedy = orc.greedy_decode(*args)
    ids, scores, _ = br.beam_decode(*args, beam=1)
    for b, (g, d, s) in enumerate(zip(greedy, ids, scores)):
        np.testing.assert_array_equal(d.numpy(), br.greedy_equivalent(g).numpy())
        np.testing.assert_array_equal(g.numpy(), z["decode/%d" % b])     # (and greedy is the reference's own golden)
        assert np.all(s <= 0) and np.all(np.isfinite(s))


def _sel(scores, beam, logits, cum, fin, C, X=0):
    R = len(cum)
    return br.select(np.asarray(scores, np.float32), [C] * R, [X] * R, beam, logits, np.asarray(cum, np.float32), np.asarray(fin, bool))


def test_select_ties_at_every_level_of_the_order():
    # C = 9 (UNK = 6 excluded).  Level 1, cum: the larger sum wins.
    p = np.full((2, 9), 0.01, np.float32)
    p[0, 3] = 0.5; p[1, 2] = 0.4
    par, ext, mod, cum, fin = _sel(p, 2, False, [0.0, 0.0], [0, 0], 9)
    assert list(ext) == [3, 2] and list(par) == [0, 1]
    # Level 2: equal cum (a dead parent: -inf for every candidate of both) → higher raw value
    p = np.full((2, 9), 0.0, np.float32)
    p[0, 1] = 0.2; p[1, 4] = 0.3
    par, ext, _, cum, _ = _sel(p, 2, False, [NEG, NEG], [0, 0], 9)
    assert list(zip(par, ext)) == [(1, 4), (0, 1)] and np.all(cum == NEG)
    # Level 3: equal cum and raw value → lower flat index h·C + c (beam 0's column 8 before beam 1's column 0)
    p = np.zeros((2, 9), np.float32)
    p[0, 8] = 0.25; p[1, 0] = 0.25
    par, ext, _, _, _ = _sel(p, 2, False, [0.0, 0.0], [0, 0], 9)
    assert list(zip(par, ext)) == [(0, 8), (1, 0)]
    # … and inside one row equal values go to the lower column
    p = np.zeros((1, 9), np.float32); p[0, 5] = p[0, 2] = 0.5
    assert list(_sel(p, 1, False, [0.0], [0], 9)[1]) == [2]


def test_select_first_step_dead_beams_and_log_softmax():
    """initial scores [0, -inf]: every child descends from beam 0 while it has candidates; video mode scores the log_softmax."""
    rng = np.random.default_rng(0)
    lg = rng.standard_normal((2, 12)).astype(np.float32)
    lg[1] = lg[0]
    par, ext, _, cum, _ = _sel(lg, 2, True, [0.0, NEG], [0, 0], 12)
    assert list(par) == [0, 0]
    cols = [c for c in range(12) if c != UNK]
    order = sorted(cols, key=lambda c: (-lg[0, c], c))[:2]
    assert list(ext) == order
    ref = torch.log_softmax(torch.from_numpy(lg[0, cols]).double(), 0).numpy()
    np.testing.assert_allclose(cum, [ref[cols.index(c)] for c in order], rtol=1e-6)


def test_select_unk_is_never_a_candidate_and_oov_maps_to_unk():
    p = np.zeros((1, 10), np.float32)
    p[0, UNK] = 0.9; p[0, 9] = 0.5; p[0, 1] = 0.1            # C = 10 with X = 2 OOV columns (8, 9)
    _, ext, mod, _, _ = _sel(p, 1, False, [0.0], [0], 10, X=2)
    assert ext[0] == 9 and mod[0] == UNK
    p[0, 9] = 0.0
    _, ext, mod, _, _ = _sel(p, 1, False, [0.0], [0], 10, X=2)
    assert ext[0] == 1 and mod[0] == 1


def test_select_finished_beam_carries_itself():
    """a finished hypothesis offers exactly one candidate: itself, PAD, step 0 (raw value +inf); EOS finishes a child."""
    p = np.zeros((2, 9), np.float32)
    p[0, 4] = 0.9                                           # (ignored: hypothesis 0 has finished)
    p[1, EOS] = 0.5; p[1, 3] = 0.4
    par, ext, mod, cum, fin = _sel(p, 2, False, [-1.0, -0.1], [1, 0], 9)
    # candidates: (1, EOS) cum -0.1+log .5 = -0.793, (1, 3) -1.016, (0, PAD) -1.0
    assert list(zip(par, ext)) == [(1, EOS), (0, PAD)]
    assert list(fin) == [True, True] and mod[1] == PAD
    np.testing.assert_allclose(cum, [np.float32(-0.1) + np.float32(np.log(0.5)), -1.0], rtol=1e-6)
    # the finished candidate wins ties on cum (raw +inf)
    p = np.zeros((2, 9), np.float32); p[1, 3] = 1.0
    par, ext, _, cum, _ = _sel(p, 2, False, [-0.5, -0.5], [1, 0], 9)
    assert list(zip(par, ext))[0] == (0, PAD) and list(zip(par, ext))[1] == (1, 3)


def test_select_zero_probability_is_minus_infinity():
    p = np.zeros((1, 9), np.float32)
    p[0, 2] = 1.0
    _, ext, _, cum, _ = _sel(np.vstack([p, p]), 2, False, [0.0, NEG], [0, 0], 9)
    assert ext[0] == 2 and cum[0] == 0.0 and cum[1] == NEG


def test_library_exports_the_beam_entry_points():
    """the header declares them and the built library exports them (no GPU needed to load it)."""
    from svpc_amd import _lib
    decl = _lib.declarations()
    for n in ("svpc_beam_step", "svpc_beam_finalize", "svpc_attn_q1_ln_idx_fwd"):
        assert n in decl, n
    lib = _lib.load()
    assert lib.svpc_abi_version() == 2
    for n in ("svpc_beam_step", "svpc_beam_finalize", "svpc_attn_q1_ln_idx_fwd"):
        assert hasattr(lib, n), n


def test_translator_beam_contract_errors():
    """incremental=False with beams is not implemented; the width is bounded — both refused before any device work."""
    from svpc_amd.translator import Translator
    tr = Translator.__new__(Translator)
    tr.incremental = False
    with pytest.raises(NotImplementedError):
        tr.translate_batch_beam([None] * 12, 2)
    tr.incremental = True
    for bad in (0, 9):
        with pytest.raises(ValueError):
            tr.translate_batch_beam([None] * 12, bad)
