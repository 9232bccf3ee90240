"""Pure-Python restatement of consensus (minimum Bayes risk) selection among decoded candidates (svpc_amd/csrc/consensus.hip, DESIGN
§11.7).  Built on ``caption_scores_reference.video_scores(h, [r], cider)`` — candidate i is the hypothesis, candidate j the single
pseudo-reference — plus the one rule that restatement lacks: ROUGE_L against an empty pseudo-reference is 0 (q = 0).  Shares no code
with the product.

- a group's candidates: ``scope="paragraph"`` — candidate k of a video is row k of every sentence, in sentence order, tokenised as §11.6
  tokenises a hypothesis paragraph; ``scope="sentence"`` — candidate k of sentence s is that one caption;
- ``U[i][j]`` = the six scores (Bleu_1..4, ROUGE_L, CIDEr), for every ordered pair, i = j included;
- ``E[i] = Σ_{j≠i} w_j · U[i][j][u] / Σ_{j≠i} w_j`` (j ascending; 0 when the denominator is 0); w_j = 1, or exp(c_j − max c) with c_j the
  candidate's cumulative score (summed over the video's sentences in paragraph scope; every weight 1 when the maximum is −inf);
- the pick is the arg max of E, ties to the lowest i.
"""
import math
import random

import caption_scores_reference as cs

UTILITIES = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")
MARGIN = 1e-9           # a pick is asserted to be the restatement's arg max where best and second best differ by more than this (relative)


def pair_utility(h, r, cider):
    """the six scores of hypothesis ``h`` against the single pseudo-reference ``r`` (token lists)"""
    if r:
        return cs.video_scores(h, [r], cider)[1]
    correct, guess, testlen, reflen = cs.bleu_counts(h, [r])               # an empty pseudo-reference: ROUGE_L's q = 0
    return cs.bleu_from_counts(correct, guess, testlen, reflen) + [0.0, cider.score(h, [r])]


def pair_scores(streams, cider):
    """→ U[i][j] (six scores) for every ordered pair of the group's token streams"""
    return [[pair_utility(h, r, cider) for r in streams] for h in streams]


def weights_of(cum):
    """posterior weights of the candidates' cumulative scores; every weight 1 when the maximum is −inf"""
    m = max(cum)
    if m == -math.inf:
        return [1.0] * len(cum)
    return [math.exp(c - m) for c in cum]


def expected(U, col, w=None):
    K = len(U)
    w = [1.0] * K if w is None else w
    out = []
    for i in range(K):
        num = den = 0.0
        for j in range(K):
            if j != i:
                num += w[j] * U[i][j][col]
                den += w[j]
        out.append(num / den if den != 0 else 0.0)
    return out


def pick_of(E):
    best = 0
    for i in range(1, len(E)):
        if E[i] > E[best]:
            best = i
    return best


def under_margin(E):
    """best and second best of E closer than the margin: the device's pick may be either"""
    if len(E) < 2:
        return False
    s = sorted(E, reverse=True)
    return s[0] - s[1] <= MARGIN * max(1.0, abs(s[0]))


def group_streams(cands, idx2word, oov, scope):
    """``cands[k]`` = the S_b id rows of candidate k of one video → the video's groups, each a list of K token streams"""
    if scope == "paragraph":
        return [[cs.hypothesis_tokens(rows, idx2word, oov) for rows in cands]]
    return [[cs.hypothesis_tokens([rows[s]], idx2word, oov) for rows in cands] for s in range(len(cands[0]))]


def group_cum(cum, scope):
    """``cum[s][k]`` of one video → per group the K cumulative scores (paragraph: the sum over the sentences, in order)"""
    if scope != "paragraph":
        return [list(row) for row in cum]
    tot = [0.0] * len(cum[0])
    for row in cum:
        for k, c in enumerate(row):
            tot[k] += c
    return [tot]


def select(cands, idx2word, oov, cider, scope, utility="CIDEr", cum=None):
    """one video → per group (U, E, pick)"""
    col = UTILITIES.index(utility)
    cg = group_cum(cum, scope) if cum is not None else None
    out = []
    for g, streams in enumerate(group_streams(cands, idx2word, oov, scope)):
        U = pair_scores(streams, cider)
        E = expected(U, col, weights_of(cg[g]) if cg is not None else None)
        out.append((U, E, pick_of(E)))
    return out


# ---------------------------------------------------------------------------------------------------- the seeded candidate maker
P_DROP, P_REPLACE = 0.15, 0.4


def perturb_row(row, rng, V, bos, eos, pad, first_word=7):
    """a decoded id row with each word dropped with probability 0.15 or replaced by a random vocabulary word with probability 0.4"""
    lt = len(row)
    words = []
    for x in row[1:]:
        if x == eos:
            break
        if x == pad:
            continue
        words.append(x)
    out = []
    for x in words:
        u = rng.random()
        if u < P_DROP:
            continue
        out.append(rng.randrange(first_word, V) if u < P_DROP + P_REPLACE else x)
    return ([bos] + out + [eos] + [pad] * lt)[:lt]


def make_candidates(id_rows, K, rng, V, bos, eos, pad):
    """→ cands[k] (K lists of S_b rows): candidate 0 is ``id_rows``, the others are perturbed copies"""
    if not isinstance(rng, random.Random):
        raise TypeError("the candidate maker takes Python's random.Random")
    return [[list(r) for r in id_rows]] + [[perturb_row(r, rng, V, bos, eos, pad) for r in id_rows] for _ in range(K - 1)]
