"""Greedy and beam-search caption decoding on the MI355X — drop-in for the reference's ``Translator`` (src/translator.py:27-228).

Same constructor and ``translate_batch`` contract (12-element ``model_inputs`` list in, ``(dec_seq_list, oov_word_dict)``
out, one ``(S_b, Lt)`` int64 id matrix per video, extended ids ≥ V kept for copied OOV words).  Restructured for the GPU:
all videos of the batch are decoded together — clip encoder, step-wise encoder and visual simulator run once over every
clip of the batch, then the ``max_t_len`` decoding iterations advance all T = Σ_b S_b sentences at once with arg-max, UNK
suppression and OOV→UNK remapping done by a kernel (no host synchronisation inside the loop).

Decoding is **incremental** by default: iteration i embeds only the token chosen at i-1, appends its self-attention K|V row to a
per-layer cache and attends to the i+1 cached keys; cross-attention K|V of the memory slots and the pointer's bank projection
are computed once.  Under the reference's causal∧pad mask (translator.py:88-100 re-runs all Lt positions every iteration) position
i's output depends on exactly those keys, so the ids are the same — ``incremental=False`` keeps the re-run-everything form, and
the parity tests check both against the reference's ids.

**Beam search** (``translate_batch(model_inputs, use_beam=True)``, width ``B = opt.beam_size`` (default 2, 1 ≤ B ≤ 8), the reference
CLI's ``--use_beam --beam_size``, test.py:207-209 → translate.py:73-74, which the reference's own Translator accepts and ignores).  Returns
what greedy returns; ``translate_batch_beam(model_inputs, beam_size)`` also returns one fp32 score per sentence.  The contract:

- the encoder side runs once per batch; the decoding iterations run over T·B hypothesis rows (hypothesis-major within a sentence);
- step score of a token: pointer modes ``log p`` of the mixed extended-vocabulary probability (p ≤ 0: −inf); ``video`` mode the
  ``log_softmax`` of the logits over the row's columns; the UNK column is never a candidate;
- hypothesis score: the fp32 sum ``cum_child = cum_parent + step``, no length penalty;
- position 0 is BOS; the Lt − 1 picks of positions 1 … Lt − 1 are selected and scored (greedy's last, discarded iteration has no
  counterpart); at the first step only beam 0 is alive (initial scores [0, −inf, …]);
- candidates rank by higher cum, then higher raw value (p, or the logit), then lower flat index parent·C + column — so B = 1 picks what
  greedy picks;
- a hypothesis whose extended id is EOS is finished: from then on its only candidate is itself with token PAD (both id spaces), step
  score 0; rows hold PAD after EOS (the reference's ``convert_ids_to_sentence`` stops at the first EOS and drops PAD);
- copied OOV words keep their extended id ≥ V in the output, the model side sees UNK;
- the result per sentence is the best of the B final hypotheses by cum (ties: the lowest beam index);
- ``incremental=False`` raises NotImplementedError; ``two_streams`` is ignored.

**Decoding controls** (the reference's OpenNMT-derived decoder lineage: ``min_length``, ``block_ngram_repeat``, ``exclusion_tokens``,
``length_penalty``, ``n_best``; src/train.py:548 and src/test.py:209 parse ``--n_best``).  Read from ``opt`` with ``getattr`` defaults,
overridden by keyword arguments of the same names on ``translate_batch``, ``translate_batch_beam`` and ``translate_batch_nbest``; all
default to off, and with every control off nothing changes (same ids, scores, launches and graphs):

- ``block_ngram_repeat`` n (0: off, ≤ Lt − 1; Lt ≤ 64 when on): a hypothesis's words are its extended ids y_1 … y_pos (BOS excluded;
  a copied OOV word is its own word).  Candidate (h, w) at position p = pos + 1 ≥ n is banned when its gram (y_{p−n+1} … y_pos, w)
  equals some earlier (y_j … y_{j+n−1}), j = 1 … p − n, and no token of the gram is in ``exclusion_tokens`` (text ids < V).  The ban is
  per candidate; banned columns are skipped like UNK (but stay in ``video`` mode's log-sum-exp, so a step score is what it was);
- ``min_length`` m (0 … Lt − 1): EOS is not a candidate at positions p ≤ m;
- ``length_penalty_name`` / ``length_penalty_alpha``: candidates rank by key = (double)cum / lp[len], lp = ``none`` 1, ``avg`` len,
  ``wu`` ((5 + len) / 6) ^ alpha (alpha finite ≥ 0), a float64 table computed once on the host (``ops.length_penalty_table``); a live
  parent's child has len = p, a finished hypothesis keeps the len at which it picked EOS, one that never finishes ends at Lt − 1.  Order:
  higher key, then higher raw value, then lower flat index; ``none`` is today's order;
- fewer than B unbanned candidates in a sentence: the leftover slots are PAD, cum −inf, finished, len = p (as before);
- the final pick orders a sentence's hypotheses by the final key (ties: the lower beam index); ``translate_batch_beam``'s score is still
  the fp32 cum; ``translate_batch_nbest(model_inputs, beam_size, n_best)`` (1 ≤ n_best ≤ B, default ``opt.n_best`` = 1) returns
  ``(dec_seq_list, oov_word_dict, score_list, length_list)``: per video ids (S_b, n_best, Lt) int64, cum (S_b, n_best) fp32 and len
  (S_b, n_best) int64 in final-key order, so row 0 is ``translate_batch_beam``'s result;
- greedy (``use_beam=False``) with any control on runs the width-1 beam with those controls; with none, the greedy path is untouched;
- every argument is checked on the host (ValueError) before any device work.  Each setting has its own prepared plan and captured graph.

**Paragraph-scope blocking** (``block_ngram_scope``: ``"sentence"``, the default and the rule above, or ``"paragraph"``; resolved like the
other controls, not taken by ``translate_batch_sample``).  The reference scores a video's captions as one paragraph (its repetition metric
counts the n-grams of all of a video's sentences together, none spanning two sentences), so ``"paragraph"`` also blocks the grams of the
video's earlier captions:

- a video's sentences are taken in index order s = 0 … S_b − 1 (timestamp order); the *words* of a decoded sentence are the extended ids
  of its chosen caption (row 0 in final-key order) at positions 1 … L, L + 1 being its first EOS or PAD (L = Lt − 1 when it has none),
  BOS excepted; a copied OOV word (id ≥ V) is its own word.  A gram is n consecutive positions that are all words, so none spans two
  sentences;
- candidate (h, w) at position p ≥ n of sentence s is also banned when (y_{p−n+1} … y_pos, w) equals a gram of a sentence s′ < s of the
  same video and no token of it is in ``exclusion_tokens``; the within-hypothesis ban applies as well, and everything else (skipped like
  UNK, ``video`` mode's log-sum-exp, ``min_length``, the length penalty, n-best order, fewer than B candidates) is as above;
- so sentence s is decoded after sentences 0 … s − 1 of its video, conditioned on their chosen captions: the decoding iterations run in
  rounds, round s over sentence s of every video with S_b > s.  Sentence 0, and every video with S_b = 1, gets what ``"sentence"`` gives;
  with n-best, later sentences see row 0; greedy with it is the width-1 beam with it;
- ValueError on the host for an unknown scope, ``"paragraph"`` with ``block_ngram_repeat == 0``, and ``"paragraph"`` with score rows wider
  than ``ops.SAMPLE_COLS_MAX`` = 4096 columns (V + X: the kernel keeps a row's bans as a bitmap of that many columns).

The per-layer KV caches hold one slot of Lt rows per hypothesis; a row is written once, into the slot of the hypothesis that computes it,
and ``ops.beam_step`` keeps a per-hypothesis ancestry table of cache rows that the attention reads through (no cache copy per step).

**Random sampling** (the random-sampling half of the reference's OpenNMT decode-strategy lineage, which vendored only the beam half):
``translate_batch_sample(model_inputs, num_samples=1, **kw)`` → ``(dec_seq_list, oov_word_dict, score_list, length_list)``: per video ids
(S_b, R, Lt) int64 (extended ids, BOS at position 0, PAD after EOS), cum (S_b, R) fp32 and len (S_b, R) int64, samples in sample order
(not sorted).  Keywords override ``opt`` attributes of the same name (``getattr`` defaults, as the decoding controls):
``random_sampling_temp`` τ (1.0), ``random_sampling_topk`` k (0: the full distribution; OpenNMT's −1 is taken as 0),
``random_sampling_topp`` q (0.0: off), ``min_length`` m (0); ``seed`` is keyword-only (the reference's ``opt.seed`` is its training seed).

- sample j of sentence t is row r = t·R + j, 1 ≤ R ≤ 8; every sample starts alive at BOS; C_r = V + X columns (X = 0 in ``video``
  mode); step i = 0 … Lt − 2 picks position p = i + 1;
- one step of a live row: raw_c is the mixed probability (pointer modes) or the logit (``video``); the step score s_c is beam's (fp64,
  rounded once: log raw_c, −inf for raw_c ≤ 0; or raw_c − the log-sum-exp of the row without UNK); candidates K0 are the columns c < C_r,
  c ≠ UNK, s_c > −inf, and not EOS while p ≤ m, ordered by higher raw_c then lower c; top-k keeps the first min(k, |K0|) (K1); z_c =
  (double)s_c / τ; top-p (0 < q < 1) keeps the shortest prefix K2 of K1 with Σ w ≥ q·W, w_c = exp(z_c − z_first), W = Σ_K1 w; the pick
  is argmax over K2 of z_c + g_c, g_c = −log(−log u_c), u_c = (svpc_hash32(seed, i, r·4096 + c) + 0.5)·2⁻³² (Gumbel-max: an exact draw
  from softmax(z) over K2), ties to the lower c;
- the pick's extended id is kept, the model side sees UNK for a copied word; cum = fp32(cum + s_pick); len = p; EOS finishes the row; a
  finished row takes PAD (step score 0, len kept); a row with an empty K0 takes PAD, cum −inf, finished, len p;
- so k = 1, m = 0, R = 1 gives greedy's ids up to the first EOS (PAD after it) for any τ, q and seed, and k = 1 makes a sentence's R
  samples identical;
- ``seed=s`` (an int in [0, 2⁶³)) draws from the stream keyed by s alone: the same ids eagerly and replayed, whatever ran before;
  ``seed=None`` draws a fresh stream each call from a device-resident seed word that the decode advances itself (consecutive replays of
  one captured graph differ); ``last_sample_seed`` (a device int64 (1,) tensor) holds the seed the last call used;
- every argument is checked on the host before any device work: ValueError for R, τ (finite > 0), k (≥ −1), q ([0, 1]), m (0 … Lt − 1),
  the seed, and rows wider than 4096 columns; TypeError for an unknown keyword; ``incremental=False`` raises NotImplementedError.
  Each setting (R, τ, k, q, m) has its own prepared plan and captured graph; the seed is a captured input.
- truncation: four further keywords, each off at 0, also read from ``opt`` — ``min_p`` a ∈ [0, 1) (Nguyen et al. 2024),
  ``typical_p`` m ∈ [0, 1] (locally typical sampling, Meister et al. 2022; 1 is off too), ``epsilon_cutoff`` ε and ``eta_cutoff`` η ∈
  [0, 1) (Hewitt et al. 2022).  They run in this order on K2, every stage over the distribution renormalised over the survivors of the
  one before (first = their ≻-first column, w_c = exp(z_c − z_first), W = Σ w, q_c = w_c / W, ln q_c = (z_c − z_first) − ln W, fp64):
  min-p keeps w_c ≥ a; typical keeps d_c = |−ln q_c − H| ≤ d*, H = −Σ q ln q, d* the smallest d whose columns {d_c ≤ d*} hold m of the
  mass (equal d stay or go together; the mode may go; never empty); epsilon keeps q_c ≥ ε; eta keeps q_c ≥ min(η, √η·exp(−H)); min-p,
  epsilon and eta always keep the first column.  The pick is the same Gumbel-max (same z, same hash index, same tie rule) over what is
  left, and cum still adds the model's untruncated step score, so ``score_captions`` reproduces it.  ValueError for a non-number, a
  bool, NaN or a value out of range.  With all four off the decode is the one above — the same plan, the same launches, the same ids
  bit for bit; otherwise the setting joins the plan key, the selection is ``ops.sample_step_trunc``, and ``last_sample_kept`` holds
  the (Lt − 1, T·R) int32 sizes of the sets the rows drew from (0 once finished).  ``translate_batch_stochastic`` rejects the four
  keywords (TypeError): truncation would break its sampling without replacement.

**Captions from ids** (the reference's host tail, src/translate.py:81-83): ``Translator.clean_captions(dec_seq_list, row=0,
remove_dup=True)`` turns any of the results above into the clean captions on the device (the ids without PAD / IGNORE, without the first
of those, up to the first EOS, runs of one word collapsed — ``convert_ids_to_sentence`` then ``remove_dup``), and
``ids_to_sentences(clean, lens, idx2word, oov_word_dict)`` builds the strings on the host.  ``svpc_amd.metrics.DecodeMetrics`` counts
the reference's repetition / diversity numbers from the same ids.  ``Translator.caption_ingredients(dec_seq_list, plan,
row=0)`` tells which of a recipe's ingredients each caption mentions (the rule of src/calculate_ingredient_f1.py, on the device;
``svpc_amd.metrics.IngredientF1`` accumulates its recall / precision / F1 — DESIGN §11.5).  ``Translator.caption_scores(dec_seq_list,
plan, row=0)`` gives every video's Bleu_1…4, ROUGE_L and CIDEr against its reference paragraphs on the device
(``svpc_amd.metrics.CaptionScores`` accumulates the epoch's — DESIGN §11.6).  ``translate_batch*`` themselves do not change.

**Consensus selection** (minimum Bayes risk): ``Translator.consensus(dec_seq_list, plan, …)`` chooses one of the K rows
of an n-best or sampling result without references — every candidate is scored against the others as pseudo-references (one of the six
scores above, CIDEr by default, its idf from the plan's corpus) and the one with the highest expected utility wins, per video
(``scope="paragraph"``: the same row k for all its sentences) or per sentence; ``translate_batch_consensus(model_inputs, plan,
source="sample" | "nbest" | "diverse" | "stochastic", num_candidates=K)`` is the decode followed by it.  On the device, without host synchronisation.

**Diverse (group) beam search** (Vijayakumar et al. 2016, arXiv 1610.02424; fairseq's ``--diverse-beam-groups`` / ``-strength``, HF's
"group beam search"): ``translate_batch_diverse(model_inputs, beam_size, num_groups, diversity_strength, n_best)`` →
``(dec_seq_list, oov_word_dict, score_list, length_list)`` as ``translate_batch_nbest``, with K = G·n_best rows per sentence, group-major.
Restated by tests/diverse_beam_reference.py:

- the W = ``beam_size`` rows of a sentence are G = ``num_groups`` groups of Bg = W / G rows (G divides W); row g·Bg + j is hypothesis j
  of group g; every group starts from BOS on its row 0; hypotheses never cross groups;
- the groups pick in order at every step; a child (h, c) of group g pays pen[n] = fp32(fp32(λ)·n), λ = ``diversity_strength`` (finite,
  ≥ 0), n the rows of groups 0 … g − 1 whose live pick at this step is the word c (Hamming diversity; the PAD of a finished parent and
  fill rows are not counted, EOS is);
- two scores per row: ``cum``, the model's summed step scores — what the call returns and what ``score_captions`` reproduces — and
  ``aug``, cum minus every penalty paid, which ranks the candidates of a group: key (double)aug / lp[len], then the raw value, then the
  flat index; the controls that work are ``min_length``, ``length_penalty_*`` and ``block_ngram_repeat`` / ``exclusion_tokens`` in sentence
  scope (``block_ngram_scope="paragraph"`` with G > 1: ValueError);
- at the end each group's rows are ordered by the final key (double)cum / lp[len] (the penalty steers the search, it does not judge the
  result); the call returns ``n_best`` rows per group (1 … Bg, default Bg);
- G = 1 is ``translate_batch_nbest(W, n_best)`` exactly; λ = 0 makes the G groups identical copies of a width-Bg beam search;
- ``translate_batch_consensus(source="diverse", num_candidates=K, num_groups=G, diversity_strength=λ)`` decodes K / G rows per group
  (``beam_size`` defaults to K) and picks among them.

**Lexically constrained beam search** (Post & Vilar 2018, "dynamic beam allocation", arXiv 1804.06609; fairseq's unordered
``--constraints``): ``translate_batch_constrained(model_inputs, constraints, beam_size, n_best)`` →
``(dec_seq_list, oov_word_dict, score_list, length_list, met_list)``.  Restated by tests/constrained_beam_reference.py:

- a sentence has M ≤ 4 constraints, each a phrase of 1 … 4 extended ids (``constraint_ids`` builds them from words), unordered,
  duplicates met separately; every hypothesis row carries a tracker state — the constraints met, the phrase in progress and the ids of
  it matched so far — whose token count n = Σ len of the met phrases + the progress is the row's bank;
- the tracker: a picked word that continues the phrase in progress advances it (a complete phrase is met); any other word drops the
  progress and starts the lowest unmet phrase that begins with it.  It is not a string matcher: with the phrase ``a a b`` the text
  ``a a a b`` does not complete it;
- candidates of an unfinished row: the allowed columns of the controlled beam step — EOS also barred while a constraint is unmet —, of
  these the row's top-W by (raw, column) and its forced columns (the next id of the phrase in progress, else the first ids of all unmet
  phrases) whose child has a finite score; live candidates rank inside their bank by the beam step's order and the W rows are filled
  best-of-every-bank first, from the highest bank down (fairseq's stride over banks), dead candidates last;
- ``cum`` stays the model's summed step score (``score_captions`` reproduces it); at the end the rows are ordered by more constraints
  met, then the final key (double)cum / lp[len], then the lower index, rows with cum = −inf last; ``met_list`` holds the rows' masks;
- with no constraints it is ``translate_batch_nbest(W, W)`` bit for bit; when Σ len ≤ Lt − 2, no control bans the phrase words and
  their probabilities are positive, row 0 of the sentence holds every phrase, for every W ≥ 1;
- the controls that work: ``min_length``, ``length_penalty_*``, ``block_ngram_repeat`` / ``exclusion_tokens`` in sentence scope
  (``block_ngram_scope="paragraph"``: ValueError); the constraint table is a per-call captured input, so one plan and one graph serve
  every constraint set of a batch structure and setting.

**Stochastic beam search** (Kool, van Hoof and Welling 2019, "Stochastic Beams and Where to Find Them", arXiv 1903.06059):
``translate_batch_stochastic(model_inputs, beam_size, seed=None, random_sampling_temp=1.0, min_length=0)`` → ``(dec_seq_list,
oov_word_dict, score_list, length_list, gumbel_list, logq_list)``: per video ids (S_b, W, Lt) int64, cum (S_b, W) fp32, len (S_b, W)
int64, G (S_b, W) float64 and phi (S_b, W) float64 — W captions per sentence sampled WITHOUT replacement from the model, in the order
drawn.  Restated by tests/stochastic_beam_reference.py:

- a sentence has W = ``beam_size`` rows (1 ≤ W ≤ 8), row r = t·W + h; a row carries ``cum`` (fp32, the model's summed step score, as
  beam's — what ``score_captions`` reproduces), ``phi`` (float64, the log-probability of its sequence under the tempered, renormalised
  model) and ``G`` (float64, the perturbed log-probability); row 0 starts alive at BOS with cum = phi = G = 0, rows 1 … W − 1 *dead*
  (−inf, finished);
- a live row's candidates are sampling's K0 (columns c < C_r, c ≠ UNK, step score s_c > −inf, not EOS while p ≤ ``min_length``); z_c =
  (double)s_c / τ, L their log-sum-exp, φ_c = phi + (z_c − L), g_c = φ_c − log(−log u_c) with sampling's counter-based u_c =
  (svpc_hash32(seed, i, r·4096 + c) + 0.5)·2⁻³²; the row's first W candidates by higher g, then lower c, are short-listed, Z their
  maximum, and each gets G̃_c = G − max(v, 0) − log1p(exp(−|v|)), v = G − g_c + log1p(−exp(g_c − Z)) (the truncated-Gumbel transform:
  the children's perturbed scores conditioned on their maximum being the parent's; the arg max carries G exactly);
- a finished row with finite G offers itself (PAD, step score 0, everything kept); a dead row, and a live row with an empty K0, nothing;
- the sentence's new rows are its first W candidates by higher G̃, then higher g, then lower flat index h·4096 + c: cum = fp32(cum +
  s_c), phi = φ_c, G = G̃_c, len = p, EOS finishes; a copied word keeps its extended id, the model side sees UNK; leftover slots are dead;
- rows stay in selection order — descending G, the order in which the captions were drawn; no final re-ranking, no length penalty, no
  n-gram blocking; the temperature changes what is sampled (phi), not cum;
- so the finite-G rows of a sentence are pairwise different captions, G never increases from parent to child nor from row j to row
  j + 1, and W = 1 is ``translate_batch_sample(num_samples=1)`` with the same τ, m and seed (ids, lengths and cum bit for bit);
- ``seed`` as sampling's (fixed: reproducible eagerly and replayed; None: the device seed word advances; ``last_sample_seed``); ValueError
  on the host for W, τ, m, the seed and rows wider than 4096 columns; TypeError for any other keyword (``random_sampling_topk`` /
  ``random_sampling_topp`` included); ``incremental=False`` raises NotImplementedError.  Each setting (W, τ, m) has its own plan and
  captured graph; ``translate_batch_consensus(source="stochastic", num_candidates=K)`` decodes with W = K.

**Contrastive search** (Su et al. 2022, "A Contrastive Framework for Neural Text Generation"; HuggingFace's ``generate(penalty_alpha,
top_k)``): ``translate_batch_contrastive(model_inputs, top_k=None, penalty_alpha=None, min_length=None)`` →
``(dec_seq_list, oov_word_dict, score_list, length_list, penalty_list)``: per video ids (S_b, Lt) int64, cum (S_b,) fp32, len (S_b,) int64
and pen (S_b, Lt) fp32 — one caption per sentence, deterministic, a soft repetition penalty taken from the model's own representation.
Restated by tests/contrastive_reference.py:

- a sentence has k = ``top_k`` candidate rows (1 ≤ k ≤ 8) and α = ``penalty_alpha`` ∈ [0, 1] (rounded to fp32); the loop runs Lt decoder
  passes, one more than the other loops: a word is chosen by its own hidden state, so the word at position Lt − 1 needs a pass too (that
  pass runs without the head);
- pass 0: every row carries BOS, row 0 alone is live and wins; its last-layer output is history entry 0;
- pass i ≥ 1: row r carries a candidate word for position i with p_r (the model's probability of it given positions 0 … i − 1) and s_r
  (its step score, beam's); h_r is the row's last-layer output (the matrix the head reads, as fp32); penalty_r = max over j < i of
  cos(h_r, H[j]); score_r = (1 − α)·p_r − α·penalty_r; the live row with the highest score wins, ties to the lowest row; its id, fp32(cum +
  s), len = i, its penalty and its hidden state are committed; EOS finishes the sentence;
- expansion (i < Lt − 1, not finished): the top k columns of the winner's score row by higher raw value, then lower column, without UNK,
  without EOS while i + 1 ≤ ``min_length`` (skipped, nothing renormalised) become the k rows' candidates at i + 1; p is the raw value (≤ 0:
  0), in ``video`` mode fp32(exp(raw − lse)); a candidate with p = 0 is dead (PAD, never wins); all k children take the winner's token
  rows and KV ancestry;
- dot products, norms, cosines and scores are fp64 (cos is 0 when a norm is 0); a finished sentence writes PAD; a sentence without a live
  candidate finishes with PAD and cum = −inf;
- the candidate rows are in descending-p order, so α = 0 (any k) and k = 1 (any α) give the width-1 beam's ids and cum; len counts as
  ``translate_batch_nbest``'s; pen is 0 at position 0 and after the end;
- defaults ``opt.top_k`` (4), ``opt.penalty_alpha`` (0.6), ``opt.min_length`` (0); ValueError on the host for k, α, m and rows wider
  than 4096 columns; TypeError for any other keyword; ``incremental=False`` raises NotImplementedError, and so does an
  ``EnsembleTranslator`` (M members have M hidden spaces).  Each setting (k, α, m) has its own plan and captured graph.

**Forced scoring** (the GOLD score / gold perplexity of the reference decoder's OpenNMT lineage):
``Translator.score_captions(model_inputs, dec_seq_list, unk="bar")`` scores GIVEN captions under decoding conditions (text half masked,
``log p`` of the mixed pointer-generator distribution).  The definition, restated by tests/forced_score_reference.py:

- captions come in the shape every ``translate_batch*`` returns: per video (S_b, Lt) or (S_b, K, Lt), int64 or int32 extended ids,
  1 ≤ K ≤ 16, y_0 = BOS; row r = t·K + k has C_r = V + X columns of its video (X = 0 in ``video`` mode);
- step i = 0 … Lt − 2 scores position p = i + 1 with target w = y_p while the row is live: w == EOS: its step score is added, the row is
  finished, len = p; w == PAD or w == IGNORE: the row ends unfinished, len = p − 1, nothing is added and nothing after it is looked at;
  otherwise the step score of column w is added; a row that never ends has len = Lt − 1;
- the step score is exactly the decoder's (fp64, rounded once to fp32: ``log p``, −inf for p ≤ 0; ``video`` mode the logit minus the
  log-sum-exp of the row's columns without UNK); a target that is no candidate of the decoder (w == UNK, w < 0, w ≥ C_r) follows ``unk``:
  ``"bar"`` (default) −inf, ``"skip"`` contributes 0 and is not counted in ``n_scored``;
- cum = fp32(cum + s) in position order, the decoder's own accumulation; the model-side input at position p is w if 0 ≤ w < V, else UNK;
- per row: ``cum`` (T, K) fp32, ``len`` / ``n_scored`` / ``finished`` (T, K) int32; per position (T, K, Lt − 1): ``step`` fp32 (0 past the
  end), ``rank`` int32 — the candidate columns (c < C_r, c ≠ UNK) that precede w in the decoder's order (higher raw value, then lower
  column; 0 is greedy's pick; −1 past the end or for a non-candidate) —, ``top`` int32 the best candidate column and ``top_step`` fp32 its
  step score (−1 and 0 past the end);
- the decoder side runs ONCE over the T·K caption rows of Lt positions (causal ∧ pad mask), not Lt − 1 times; the K captions of a
  sentence share its memory rows and pointer bank; ``incremental`` makes no difference, ``two_streams`` is ignored.

``Translator.gold_captions(input_labels_list, batch_step_num)`` builds the references of a batch as a ``dec_seq_list`` on the device;
``svpc_amd.metrics.ForcedScores`` accumulates gold score, perplexity, top-1 agreement and mean rank.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from .model import BatchPlan, StateAwareRecursiveTransformer, _Ctx
from .ops import check_beam_controls, check_sampling, exclusion_bitmap, length_penalty_table     # (host-side: bound here, not through ``ops``)
from .ops_common import ACT_RELU, BulkUpload, Idx, SeqInfo
from .synthetic import BOS, EOS, IGNORE, PAD, UNK


def ids_to_sentences(clean, lens, idx2word, oov_word_dict):
    """The strings of one video's clean captions (host): ``clean`` (S_b, Lt) ids and ``lens`` (S_b,) as ``Translator.clean_captions``
    returns them (tensors, arrays or lists), ``idx2word`` id → word, ``oov_word_dict`` word → extended id of the video's copied words →
    a list of S_b sentences, words joined by one blank — the reference's ``remove_dup(convert_ids_to_sentence(ids, oov_word_dict))``
    (src/translate.py:82-83) when ``clean`` was made with ``remove_dup=True``."""
    rows = clean.tolist() if hasattr(clean, "tolist") else [list(r) for r in clean]
    ns = lens.tolist() if hasattr(lens, "tolist") else list(lens)
    oov = {int(v): k for k, v in (oov_word_dict or {}).items()}
    return [" ".join(idx2word[w] if w in idx2word else oov[w] for w in row[:int(n)]) for row, n in zip(rows, ns)]


GREEDY, BEAM, SAMPLE, FORCE = "greedy", "beam", "sample", "force"


class Decode(object):
    """What decode a call asks for: built by the public entry points, passed through ``_translate`` to ``_prepare`` and the device part.
    ``kind``: GREEDY, BEAM or SAMPLE; ``width``: the rows per sentence (beam width B, samples R; greedy 1); ``controls`` / ``ctl_key``: the
    checked decoding controls and their key (None: all off); ``sampling``: the checked (τ, k, q, m).  ``key`` is the decode's part of the
    plan cache key.  Outside it: ``n_best`` — the rows per sentence the call returns (0: the chosen caption alone; it only slices the
    result) — and ``seed``, this call's seed (a captured input).  FORCE (``score_captions``): ``width`` is the K given captions per
    sentence, ``sampling`` holds (unk rule, id dtype) — part of the key — and ``given`` this call's (T, K, Lt) ids (a captured input).
    Diverse beam search: BEAM with ``groups`` = (G, fp32 λ) — part of the key; ``n_best`` is then the rows returned per group.
    Constrained beam search: BEAM with ``cons``, this call's (T, CONS_MAX, CONS_LEN) int32 host table of ``ops.check_constraints`` (a
    captured input, like ``given``); only the fact that the decode is constrained is part of the key.
    Stochastic beam search: BEAM with ``stochastic`` = (τ, m) — part of the key — and ``seed`` as sampling's.
    Contrastive search: BEAM with ``contrastive`` = (k, fp32 α, m) — part of the key: α is baked into a captured graph, so two α never
    share one.
    Truncated sampling: SAMPLE with ``truncation`` = (min_p, typical_p, epsilon_cutoff, eta_cutoff), None when all four are off — part
    of the key only then, so a plain sampling decode keeps its key."""
    __slots__ = ("kind", "width", "controls", "ctl_key", "n_best", "sampling", "seed", "given", "groups", "cons", "stochastic", "contrastive",
                 "truncation")

    def __init__(self, kind=GREEDY, width=1, controls=None, ctl_key=None, n_best=0, sampling=None, seed=None, given=None, groups=None,
                 cons=None, stochastic=None, contrastive=None, truncation=None):
        self.kind, self.width, self.controls, self.ctl_key, self.n_best, self.sampling, self.seed, self.given, self.groups, self.cons = (
            kind, width, controls, ctl_key, n_best, sampling, seed, given, groups, cons)
        self.stochastic = stochastic
        self.contrastive = contrastive
        self.truncation = truncation

    @property
    def constrained(self):
        return self.cons is not None

    @property
    def ranked(self):
        """decoding controls and / or n-best: lengths tracked, all B final hypotheses sorted by their key"""
        return self.kind == BEAM and self.stochastic is None and self.contrastive is None and (self.n_best > 0 or self.ctl_key is not None)

    @property
    def key(self):
        return ((self.kind, self.width, self.ctl_key, self.ranked, self.sampling) + ((self.groups,) if self.groups is not None else ())
                + (("constrained",) if self.constrained else ()) + ((("stochastic",) + tuple(self.stochastic),) if self.stochastic is not None else ())
                + ((("contrastive",) + tuple(self.contrastive),) if self.contrastive is not None else ())
                + ((("truncation",) + tuple(self.truncation),) if self.truncation is not None else ()))


class DecodePlan(object):
    """Everything of a decode that depends on the batch STRUCTURE and the ``Decode`` setting only (``Translator._prepare``): cached, and
    the owner of the setting's captured graphs.  A field its mode does not use is None."""
    __slots__ = ("key", "plan", "spans", "c_list", "T",       # the structure: BatchPlan, ingredient spans, columns per video, sentences
                 "kind", "width", "ranked",                     # of the Decode
                 "ptr_all", "x_all",                            # pointer plan and OOV counts, Lt rows per sentence (incremental=False)
                 "ptr_hyp", "x_hyp",                            # the same, ``width`` rows per sentence: row t·width + h (incremental)
                 "controls",                                    # ranked: ops.beam_step's keywords (device tables)
                 "rounds", "rows_max",                          # paragraph scope: the round tables, the largest round's rows
                 "groups", "pen",                               # diverse beam search: G, the device penalty table (ops.diversity_table)
                 "cons",                                        # constrained beam search: the (T, 4, 4) device table, a captured input
                 "sampling", "key_rows", "seed_src", "seed_used",       # sampling: ops.sample_step's keywords, ancestry, seed words
                 "truncation", "kept",                          # truncated sampling: ops.sample_step_trunc's further keywords, kept (Lt − 1, T·R)
                 "stochastic",                                  # stochastic beam search: ops.stochastic_beam_step's keywords (+ the seed words)
                 "contrastive",                                 # contrastive search: ops.contrastive_step's keywords
                 "given", "unk", "ptr_force", "cap_c", "force_self", "force_cross", "group_rows",     # forced scoring (``_force_pass``)
                 "raw",                                         # forced pass stopped at the score matrix (``teacher_scores``)
                 "seq_cross", "seq_self",                       # segmentations, built on first use
                 "graphs")                                      # replay stream → (graph, captured inputs, outputs, signature)

    def __init__(self, **fields):
        for k in self.__slots__:
            setattr(self, k, fields.pop(k, None))
        assert not fields, sorted(fields)
        self.seq_cross, self.graphs = {}, {}


class _DecoderSide(object):
    """The decoder side of one incremental decode, built once after the encoder side: the memory K|V projection (one wide matrix for the
    whole stack, or one per layer), the pointer bank and its projection, the text-embedding table.  The greedy, beam, sampling and
    paragraph loops take their caches and rows from it and run every iteration through ``scores``."""

    def __init__(self, model, cx, mem, bank, tab, T):
        self.model, self.cx, self.bank, self.tab, self.T = model, cx, bank, tab, T
        self.logits = model.config.model_mode == "video"      # what ``scores`` returns: the step kernels' ``logits`` flag
        self.layers = model.decoder.layer
        self.n_mem = mem.shape[0] // T
        st = model.decoder.stacked_memory_kv()
        self.stacked = st is not None          # one projection of the memory rows for the whole stack; each layer reads its columns
        self.wide = [ops.linear(mem, st[0], st[1])] if st is not None else [layer.memory_kv(mem) for layer in self.layers]
        self.proj = model.bank_projection(bank) if bank is not None else None

    def caches(self, n_rows):
        """the per-layer KV caches: one slot of Lt rows per hypothesis row"""
        cfg = self.model.config
        return [torch.zeros(n_rows * cfg.max_t_len, 2 * cfg.hidden_size, dtype=torch.float32, device=self.wide[0].device) for _ in self.layers]

    def seq_cross(self, dp):
        """row r of the T·width hypothesis rows over the memory rows of its sentence r // width"""
        sq = dp.seq_cross.get(self.n_mem)
        if sq is None:
            W, n, R = dp.width, self.n_mem, dp.T * dp.width
            sq = dp.seq_cross[n] = SeqInfo(list(range(R)), [1] * R, [(r // W) * n for r in range(R)], [n] * R, self.wide[0].device)
        return sq

    def rows(self, rd=None):
        """(per-layer memory K|V, bank, bank projection) of the whole batch, or — row gathers — of the sentences of paragraph round ``rd``"""
        wide, bank, proj = self.wide, self.bank, self.proj
        if rd is not None:
            dev = wide[0].device
            mem_rows, sent = rd.mem_rows.dev(dev), rd.sent32.dev(dev)
            wide = [ops.take_rows_f32(w, mem_rows) for w in wide]
            bank = ops.take_rows_f32(bank.reshape(self.T, -1), sent).view(rd.n, *bank.shape[1:]) if bank is not None else None
            proj = ops.take_rows_f32(proj.reshape(self.T, -1), sent).view(rd.n, *proj.shape[1:]) if proj is not None else None
        return ops.split_cols(wide[0], len(self.layers)) if self.stacked else wide, bank, proj

    def scores(self, rows, ptr, nxt, i, caches, seq_self, seq_cross, key_rows=None, group=1, hidden=False, head=True):
        """one decoding iteration over hypothesis rows → their score rows: the text embedding of tokens ``nxt`` at position i (a row of the
        per-checkpoint table: one gather instead of LayerNorm(300) → projection → LayerNorm + position encoding), the layers over each
        row's ancestry ``key_rows`` in the KV caches (``group`` rows per sentence share its memory K|V; greedy: no table, group 1), then
        the head — raw logits in ``video`` mode (the step score is their log_softmax; translator.py:159) — or the pointer-generator's
        probabilities.  ``hidden`` (contrastive search): → (score rows, the last layer's output the head reads); with ``head=False``
        the head is not run and the score rows are None (the last position commits a word and expands nothing)."""
        model, cx = self.model, self.cx
        mem_kv, bank, proj = rows
        x = ops.take_rows(self.tab[i], nxt) if self.tab is not None else model.text_embeddings.run_at(nxt, i, cx)
        for layer, cache, kv in zip(self.layers, caches, mem_kv):
            x = layer.step(x, i, model.config.max_t_len, cache, kv, seq_self, seq_cross, cx, key_rows=key_rows, q_group=group)
        if not head:
            return None, x
        if model.config.model_mode == "video":
            sc = model.decoder_classifier.run(x, cx.eps)
        else:
            sc = model._lm_probs(x, bank, ptr, cx, proj=proj)[0]
        return (sc, x) if hidden else sc


class Translator(object):
    def __init__(self, opt, checkpoint, model=None, incremental=True, graph=False):
        self.opt = opt
        self.incremental = incremental
        self.graph = graph          # replay the decode of a recurring batch structure as one hipGraph (see _decode_graphed)
        # graph mode, ≥ 2·min_half videos: the two halves of the batch as two graphs on two streams.  OFF: measured once on the MI355X
        # (round 5, 64 videos × 12 clips, bf16x3) the two replays did not overlap — 36.3 ms per batch against 27.3 ms for the one graph
        # (encoder side 13.3 ms + 2 × 22 iterations of ≈0.5 ms: every half's iterations cost what the whole batch's cost, and the
        # second half's ran after the first's) — DESIGN §0.  Kept as an option because the ids are identical either way (tested).
        self.two_streams = False
        self.min_half = 8
        self.phase_events = None    # bench.py: a list → _decode_core (eager) appends three HIP events: start, encoder side done, end
        self._preps = {}
        self._ttab = {}             # id(model) → (key, the per-checkpoint text-embedding table): see _text_table
        self._seed_word = None      # sampling with seed=None: the device-resident seed word the decode advances (see translate_batch_sample)
        self.last_sample_seed = None
        self.last_sample_kept = None    # truncated sampling: the last decode's kept-set sizes (Lt − 1, T·R) int32, 0 for finished rows
        self.device = torch.device("cuda" if getattr(opt, "cuda", True) else "cpu")
        self.model_config = checkpoint["model_cfg"]
        self.max_t_len = self.model_config.max_t_len
        self.max_v_len = self.model_config.max_v_len
        self.num_hidden_layers = self.model_config.num_hidden_layers
        model.load_state_dict(checkpoint["model"])
        self.model = model
        self.model.eval()
        if next(model.parameters()).is_cuda:
            # inference without an optimizer: adopt the parameters in a WeightStore, so the packed [Wq Wk Wv] / stacked memory K|V blocks
            # and the bf16 (+ lo plane) weight shadows are resident — without one every packed projection concatenates its weights per call
            from .optim import WeightStore
            WeightStore.for_model(model)

    @classmethod
    def prepare_video_only_inputs(cls, input_ids, input_masks, segment_ids):
        """reference: translator.py:205-228 — overwrites the caller's text half in place, as the reference does."""
        if isinstance(input_ids, list):
            for e1, e2, e3 in zip(input_ids, input_masks, segment_ids):
                text_mask = e3 == 1
                e1[text_mask] = PAD
                e2[text_mask] = 0
            return input_ids, input_masks
        text_mask = segment_ids == 1
        input_ids[text_mask] = PAD
        input_masks[text_mask] = 0
        return input_ids, input_masks

    CONTROLS = dict(block_ngram_repeat=0, exclusion_tokens=(), min_length=0, length_penalty_name="none", length_penalty_alpha=0.0,
                    block_ngram_scope="sentence")

    def _controls(self, kw, beam=None, n_best=None):
        """The decoding controls: ``opt`` attributes overridden by keyword arguments, checked (ValueError) → (normalised dict, key):
        key None when every control is off (the uncontrolled decode); paragraph scope appends ``"paragraph"`` to the key."""
        unknown = set(kw) - set(self.CONTROLS)
        if unknown:
            raise TypeError("unknown decoding control(s): %s" % ", ".join(sorted(unknown)))
        val = {k: kw[k] if k in kw else getattr(self.opt, k, d) for k, d in self.CONTROLS.items()}
        c = check_beam_controls(self.model_config.max_t_len, self.model_config.vocab_size, beam=beam, n_best=n_best, **val)
        on = c["block_ngram_repeat"] > 0 or c["min_length"] > 0 or c["length_penalty_name"] != "none"
        key = (c["block_ngram_repeat"], c["exclusion_tokens"] if c["block_ngram_repeat"] else (), c["min_length"], c["length_penalty_name"],
               c["length_penalty_alpha"] if c["length_penalty_name"] == "wu" else 0.0) if on else None
        if c["block_ngram_scope"] == "paragraph":
            key = key + ("paragraph",)
        return c, key

    def translate_batch(self, model_inputs, use_beam=False, recurrent=True, untied=False, xl=False, mtrans=False, **controls):
        if use_beam:
            dec, oov, _ = self.translate_batch_beam(model_inputs, getattr(self.opt, "beam_size", 2), **controls)
            return dec, oov
        if self._controls(controls)[1] is not None:        # greedy with controls: the width-1 beam (B = 1 picks what greedy picks)
            dec, oov, _ = self.translate_batch_beam(model_inputs, 1, **controls)
            return dec, oov
        return self.translate_batch_greedy(*model_inputs, self.model)

    @torch.no_grad()
    def translate_batch_beam(self, model_inputs, beam_size, **controls):
        """Beam search of width ``beam_size`` (module docstring) → (dec_seq_list, oov_word_dict, score_list): per video an (S_b, Lt)
        int64 id matrix, as greedy, and an (S_b,) fp32 tensor of the chosen hypotheses' summed step scores."""
        B = self._beam_width(beam_size, beam_size)
        ctl, key = self._controls(controls)
        res, oov, scores, _ = self._translate_beam(model_inputs, B, ctl, key, 0)
        return res, oov, scores

    @torch.no_grad()
    def translate_batch_nbest(self, model_inputs, beam_size=None, n_best=None, **controls):
        """The ``n_best`` best hypotheses of a width-``beam_size`` beam search (defaults ``opt.beam_size``, ``opt.n_best``; module
        docstring) → (dec_seq_list, oov_word_dict, score_list, length_list): per video ids (S_b, n_best, Lt) int64, cum (S_b, n_best)
        fp32 and len (S_b, n_best) int64, rows in final-key order."""
        B = self._beam_width(beam_size if beam_size is not None else getattr(self.opt, "beam_size", 2), beam_size)
        ctl, key = self._controls(controls, beam=B, n_best=n_best if n_best is not None else getattr(self.opt, "n_best", 1))
        return self._translate_beam(model_inputs, B, ctl, key, ctl["n_best"])

    def _beam_width(self, beam_size, given):
        B = int(beam_size)
        if not 1 <= B <= ops.BEAM_MAX:
            raise ValueError("beam_size must be 1..%d, got %r" % (ops.BEAM_MAX, given))
        if not self.incremental:
            raise NotImplementedError("beam search decodes incrementally only (Translator(incremental=True))")
        return B

    def _max_cols(self, model_inputs):
        """the widest score row of the batch: V + X columns, X the copied OOV words of a video (``oov_word_dict``, element 8 of the list)"""
        x = [len(d) for d in model_inputs[8]] if self.model_config.model_mode != "video" else []
        return self.model_config.vocab_size + max(x + [0])

    def _translate_beam(self, model_inputs, B, ctl, key, n_best):
        if ctl["block_ngram_scope"] == "paragraph":
            ops.check_paragraph_cols(self._max_cols(model_inputs))
        return self._translate(model_inputs, self.model, decode=Decode(BEAM, B, controls=ctl, ctl_key=key, n_best=n_best))

    @torch.no_grad()
    def translate_batch_diverse(self, model_inputs, beam_size=None, num_groups=None, diversity_strength=None, n_best=None, **controls):
        """Diverse (group) beam search (module docstring): W = ``beam_size`` rows per sentence in G = ``num_groups`` groups
        under the Hamming penalty λ = ``diversity_strength`` (defaults ``opt.beam_size``, ``opt.num_groups`` = 1,
        ``opt.diversity_strength`` = 0.0) → (dec_seq_list, oov_word_dict, score_list, length_list): per video ids (S_b, K, Lt) int64,
        the model score cum (S_b, K) fp32 and len (S_b, K) int64, K = G·``n_best`` rows (``n_best`` 1 … W / G per group, default all),
        group-major, each group's rows in final-key order.  ValueError on the host for the sizes, λ, the controls and
        ``block_ngram_scope="paragraph"`` with G > 1."""
        W, G, lam, nb = ops.check_diverse(beam_size if beam_size is not None else getattr(self.opt, "beam_size", 2),
                                          num_groups if num_groups is not None else getattr(self.opt, "num_groups", 1),
                                          diversity_strength if diversity_strength is not None else getattr(self.opt, "diversity_strength", 0.0),
                                          n_best)
        ctl, key = self._controls(controls)
        if ctl["block_ngram_scope"] == "paragraph":
            if G > 1:
                raise ValueError("block_ngram_scope='paragraph' is not supported with num_groups > 1")
            return self.translate_batch_nbest(model_inputs, W, nb, **controls)     # (G = 1 is the n-best decode by definition)
        self._beam_width(W, beam_size)
        return self._translate(model_inputs, self.model, decode=Decode(BEAM, W, controls=ctl, ctl_key=key, n_best=nb, groups=(G, lam)))

    @torch.no_grad()
    def translate_batch_constrained(self, model_inputs, constraints, beam_size=None, n_best=None, **controls):
        """Lexically constrained beam search (module docstring): a width-``beam_size`` beam search whose captions must
        contain given phrases.  ``constraints``: per video a list of S_b entries, each None / [] (no constraint) or a list of at most
        ``ops.CONS_MAX`` phrases of 1 … ``ops.CONS_LEN`` extended ids (``constraint_ids`` builds them from words) →
        (dec_seq_list, oov_word_dict, score_list, length_list, met_list): per video ids (S_b, K, Lt) int64, cum (S_b, K) fp32, len
        (S_b, K) int64 and met (S_b, K) int64 — bit j set when phrase j is in the row —, K = ``n_best`` (default ``beam_size``, default
        ``opt.beam_size``), rows with more constraints met first, then by the final key.  Controls: ``min_length``,
        ``length_penalty_*`` and ``block_ngram_repeat`` / ``exclusion_tokens`` in sentence scope (``block_ngram_scope="paragraph"``:
        ValueError).  ValueError on the host for the sizes, the controls and the constraints (``ops.check_constraints``)."""
        B = self._beam_width(beam_size if beam_size is not None else getattr(self.opt, "beam_size", 2), beam_size)
        ctl, key = self._controls(controls, beam=B, n_best=n_best if n_best is not None else B)
        if ctl["block_ngram_scope"] == "paragraph":
            raise ValueError("block_ngram_scope='paragraph' is not supported with constraints")
        V = self.model_config.vocab_size
        c_list = [V + (len(d) if self.model_config.model_mode != "video" else 0) for d in model_inputs[8]]
        table = ops.check_constraints(constraints, model_inputs[11], c_list, self.model_config.max_t_len)
        return self._translate(model_inputs, self.model, decode=Decode(BEAM, B, controls=ctl, ctl_key=key, n_best=ctl["n_best"], cons=table))

    @staticmethod
    def constraint_ids(phrases, word2idx, oov_words):
        """The phrases of one sentence as extended ids for ``translate_batch_constrained``: ``phrases`` a list of phrases, each a list
        of words (or one string of blank-separated words); a word of ``oov_words`` — the video's ``oov_word_dict``, word → copied id —
        takes its copied id, otherwise its id in ``word2idx``; a word in neither could never be generated: ValueError."""
        out = []
        for phrase in phrases or []:
            words = phrase.split() if isinstance(phrase, str) else list(phrase)
            ids = []
            for w in words:
                if oov_words and w in oov_words:
                    ids.append(int(oov_words[w]))
                elif w in word2idx:
                    ids.append(int(word2idx[w]))
                else:
                    raise ValueError("the word %r is neither in the vocabulary nor among the video's copied words: it cannot be generated" % (w,))
            out.append(ids)
        return out

    SAMPLING = dict(random_sampling_temp=1.0, random_sampling_topk=0, random_sampling_topp=0.0, min_length=0)
    TRUNCATION = dict(min_p=0.0, typical_p=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0)

    @torch.no_grad()
    def translate_batch_sample(self, model_inputs, num_samples=1, seed=None, **kw):
        """``num_samples`` random samples per sentence (module docstring) → (dec_seq_list, oov_word_dict, score_list, length_list): per
        video ids (S_b, R, Lt) int64, cum (S_b, R) fp32 and len (S_b, R) int64, in sample order."""
        unknown = set(kw) - set(self.SAMPLING) - set(self.TRUNCATION)
        if unknown:
            raise TypeError("unknown sampling keyword(s): %s" % ", ".join(sorted(unknown)))
        val = {k: kw[k] if k in kw else getattr(self.opt, k, d) for k, d in self.SAMPLING.items()}
        s = check_sampling(self.max_t_len, num_samples=num_samples, seed=seed, max_cols=self._max_cols(model_inputs), **val)
        tr = ops.check_truncation(**{k: kw[k] if k in kw else getattr(self.opt, k, d) for k, d in self.TRUNCATION.items()})
        if not self.incremental:
            raise NotImplementedError("sampling decodes incrementally only (Translator(incremental=True))")
        R = s["num_samples"]
        return self._translate(model_inputs, self.model, decode=Decode(
            SAMPLE, R, n_best=R, seed=s["seed"],
            sampling=tuple(s[k] for k in ("random_sampling_temp", "random_sampling_topk", "random_sampling_topp", "min_length")),
            truncation=tuple(tr[k] for k in self.TRUNCATION) if any(tr.values()) else None))

    STOCHASTIC = dict(random_sampling_temp=1.0, min_length=0)

    @torch.no_grad()
    def translate_batch_stochastic(self, model_inputs, beam_size=None, seed=None, **kw):
        """Stochastic beam search of width W = ``beam_size`` (default ``opt.beam_size``; module docstring): W captions
        per sentence sampled WITHOUT replacement from the model, in the order drawn → (dec_seq_list, oov_word_dict, score_list,
        length_list, gumbel_list, logq_list): per video ids (S_b, W, Lt) int64, cum (S_b, W) fp32 (the model's summed step scores, what
        ``score_captions`` reproduces), len (S_b, W) int64, G (S_b, W) float64 (the perturbed log-probabilities, descending) and phi
        (S_b, W) float64 (the log-probability of the row under the tempered, renormalised model); a sentence with fewer than W captions
        of positive probability ends with dead rows (PAD, −inf).  Keywords ``random_sampling_temp`` and ``min_length`` override ``opt``
        attributes of the same name; ``seed`` as ``translate_batch_sample``'s.  ValueError on the host for W, τ, m, the seed and rows wider
        than 4096 columns; TypeError for any other keyword; ``incremental=False`` raises NotImplementedError."""
        unknown = set(kw) - set(self.STOCHASTIC)
        if unknown:
            raise TypeError("unknown stochastic beam search keyword(s): %s" % ", ".join(sorted(unknown)))
        val = {k: kw[k] if k in kw else getattr(self.opt, k, d) for k, d in self.STOCHASTIC.items()}
        s = ops.check_stochastic_beam(self.max_t_len, beam_size if beam_size is not None else getattr(self.opt, "beam_size", 2), seed,
                                      self._max_cols(model_inputs), **val)
        if not self.incremental:
            raise NotImplementedError("stochastic beam search decodes incrementally only (Translator(incremental=True))")
        W = s["beam_size"]
        return self._translate(model_inputs, self.model, decode=Decode(BEAM, W, n_best=W, seed=s["seed"],
                                                                       stochastic=(s["random_sampling_temp"], s["min_length"])))

    @torch.no_grad()
    def translate_batch_contrastive(self, model_inputs, top_k=None, penalty_alpha=None, min_length=None, **unknown):
        """Contrastive search (module docstring): at every position the model's k = ``top_k`` most probable words are run
        through the decoder and the one with the highest (1 − α)·p − α·max cos(its hidden state, the caption's earlier ones) is kept, α =
        ``penalty_alpha`` (defaults ``opt.top_k`` = 4, ``opt.penalty_alpha`` = 0.6, ``opt.min_length`` = 0) → (dec_seq_list,
        oov_word_dict, score_list, length_list, penalty_list): per video ids (S_b, Lt) int64 (BOS first, PAD after EOS), cum (S_b,) fp32
        (the model's summed step scores, what ``score_captions`` reproduces), len (S_b,) int64 and pen (S_b, Lt) fp32, the kept words'
        penalties (0 at position 0 and after the end).  Deterministic; one caption per sentence.  ValueError on the host for k, α,
        ``min_length`` and rows wider than 4096 columns; TypeError for any other keyword; ``incremental=False`` raises
        NotImplementedError."""
        if unknown:
            raise TypeError("unknown contrastive search keyword(s): %s" % ", ".join(sorted(unknown)))
        c = ops.check_contrastive(self.max_t_len, top_k if top_k is not None else getattr(self.opt, "top_k", 4),
                                  penalty_alpha if penalty_alpha is not None else getattr(self.opt, "penalty_alpha", 0.6),
                                  min_length if min_length is not None else getattr(self.opt, "min_length", 0), self._max_cols(model_inputs))
        if not self.incremental:
            raise NotImplementedError("contrastive search decodes incrementally only (Translator(incremental=True))")
        return self._translate(model_inputs, self.model, decode=Decode(BEAM, c["top_k"], contrastive=(
            c["top_k"], c["penalty_alpha"], c["min_length"])))

    @staticmethod
    def _clean(dec_seq_list, row, remove_dup=True):
        """→ (words (T, Lt), len (T,)) int32 of the stacked decode, and the videos' row counts"""
        ids, steps = ops.stack_captions(dec_seq_list)
        return ops.clean_captions(ids, PAD, EOS, IGNORE, remove_dup, row=row) + (steps,)

    @staticmethod
    def _per_video(t, steps):
        """a (T, …) tensor as the videos' consecutive (S_b, …) views"""
        offs = [0]
        for s in steps:
            offs.append(offs[-1] + s)
        return [t[a:b] for a, b in zip(offs[:-1], offs[1:])]

    def clean_captions(self, dec_seq_list, row=0, remove_dup=True):
        """The captions the reference submits, on the device (``ops.clean_captions``): ``dec_seq_list`` as any
        ``translate_batch*`` returns it (per video (S_b, Lt), or (S_b, K, Lt) with ``row`` picking one of the K) →
        (clean_list, len_list): per video (S_b, Lt) int64 clean ids (PAD-filled) and (S_b,) int64 lengths, views of one buffer each.
        One launch for the batch when the list is what the translator returned; no host synchronisation."""
        words, ln, steps = self._clean(dec_seq_list, row, remove_dup)
        return self._per_video(words.to(torch.int64), steps), self._per_video(ln.to(torch.int64), steps)

    def caption_ingredients(self, dec_seq_list, plan, row=0):
        """Which ingredients each decoded caption mentions (``ops.caption_ingredients``): ``dec_seq_list`` as any
        ``translate_batch*`` returns it, ``plan`` = ``IngredientLexicon.plan(videos)`` of the same videos → (mask_list, extra_list): per
        video (S_b,) int64 masks (bit e: listed ingredient e is mentioned; ``ingredients.masks_to_names`` gives the names) and (S_b,)
        int64 counts of the other known ingredient words, views of one buffer each.  No host synchronisation."""
        words, ln, steps = self._clean(dec_seq_list, row)
        masks, extra, _, _ = ops.caption_ingredients(words, ln, plan, None, steps=steps)
        return self._per_video(masks, steps), self._per_video(extra.to(torch.int64), steps)

    def caption_scores(self, dec_seq_list, plan, row=0):
        """Bleu_1…4, ROUGE_L and CIDEr of every video's decoded paragraph against its references (``ops.caption_score_counts``; DESIGN
        §11.6): ``dec_seq_list`` as any ``translate_batch*`` returns it, ``plan`` = ``ReferenceCorpus.plan(videos)`` of the same videos →
        (N, 6) float64 on the device, e.g. to rank n-best rows or samples.  No host synchronisation."""
        words, ln, steps = self._clean(dec_seq_list, row)
        tokens, tok_len = ops.caption_tokens(words, ln, plan, steps)
        return ops.caption_score_counts(tokens, tok_len, plan)[1]

    def consensus(self, dec_seq_list, plan, scores=None, lengths=None, utility="CIDEr", scope="paragraph", weights="uniform"):
        """Consensus (minimum Bayes risk) selection among the K rows of a decode (``ops.consensus_pair_scores``, ``ops.consensus_pick``;
        DESIGN §11.7): ``dec_seq_list`` per video (S_b, K, Lt) as ``translate_batch_sample`` / ``translate_batch_nbest`` return it,
        ``plan`` = ``ReferenceCorpus.plan(videos, references=False)`` (or a plan with references) of the same videos, ``scores`` /
        ``lengths`` the decode's score_list / length_list (optional; ``weights="posterior"`` weighs pseudo-reference j by
        exp(c_j − max c) of its cumulative score and needs ``scores``).  ``scope="paragraph"``: candidate k is row k of all of a
        video's sentences, one pick per video; ``"sentence"``: one pick per sentence.  → a namespace: ``dec_seq_list`` (per video
        (S_b, Lt) int64, consecutive views of one buffer), ``pick_list`` (per video (S_b,) int64), ``expected_list`` (per video
        (S_b, K) float64: the expected utility of the sentence's group), ``score_list`` / ``length_list`` (the chosen entries, or
        None), and the device tensors behind them: ``pair_scores`` (G, K, K, 6) float64, ``pick`` (G,) int32.  Five launches, no host synchronisation, nothing uploaded for a recurring structure."""
        ops.check_consensus(None, utility, scope, weights, scores)
        ids, steps = ops.stack_captions(dec_seq_list)
        if ids.dim() != 3:
            raise ValueError("consensus: per-video ids must be (S_b, K, Lt), got %s" % (tuple(dec_seq_list[0].shape),))
        sc = None if scores is None else ops.stack_captions(scores)[0]
        ln = None if lengths is None else ops.stack_captions(lengths)[0]
        pair, _ = ops.consensus_pair_scores(ids, plan, steps, PAD, EOS, IGNORE, scope=scope)
        r = ops.consensus_pick(pair, ids, plan, steps, utility, scope, weights, sc, ln)
        expected = r["expected"]
        if scope == "paragraph":                 # a video's expected utilities on every one of its rows (a broadcast view: no launch)
            exp_list = [expected[b].unsqueeze(0).expand(s, -1) for b, s in enumerate(steps)]
        else:
            exp_list = self._per_video(expected, steps)
        return SimpleNamespace(dec_seq_list=self._per_video(r["ids"], steps), pick_list=self._per_video(r["row_pick"], steps),
                               expected_list=exp_list, pair_scores=pair, pick=r["pick"],
                               score_list=None if sc is None else self._per_video(r["scores"], steps),
                               length_list=None if ln is None else self._per_video(r["lengths"], steps))

    @torch.no_grad()
    def score_captions(self, model_inputs, dec_seq_list, unk="bar"):
        """Forced decoding: what the model thinks of GIVEN captions (module docstring, **Forced scoring**).
        ``model_inputs`` as ``translate_batch`` takes them (the text half of its ids / masks is blanked in place, as there);
        ``dec_seq_list`` per video (S_b, Lt) or (S_b, K, Lt) int64 / int32 extended ids, 1 ≤ K ≤ 16, position 0 BOS — what any
        ``translate_batch*`` returns, or ``gold_captions``; ``unk`` "bar" or "skip".  → a namespace of per-video lists (consecutive views
        of one buffer each): ``score_list`` (S_b, K) fp32 cum, ``length_list`` / ``finished_list`` / ``n_scored_list`` (S_b, K) int32,
        ``step_list`` / ``top_step_list`` (S_b, K, Lt − 1) fp32, ``rank_list`` / ``top_list`` (S_b, K, Lt − 1) int32 — K = 1 for 2-D
        input — and the flat (T, …) device tensors behind them: ``cum``, ``length``, ``finished``, ``n_scored``, ``step``, ``rank``,
        ``top``, ``top_step``.  One decoder pass over T·K·Lt rows, no host synchronisation; replayed as one graph with ``graph=True``.
        Device memory: the (T·K·Lt, V) logits and, in pointer modes, the (T·K·Lt, V + X) probabilities in fp32 (2 · 257 MB at 64
        videos × 12 clips, K = 4, Lt = 22, V ≈ 950) plus the decoder's activations of T·K·Lt rows; no chunking over sentences.
        ValueError on the host for K, the ids' shape / dtype / Lt, a mismatch with ``batch_step_num`` and an unknown ``unk``;
        ``SvpcKernelError`` for ids or inputs that are not on the GPU; ``two_streams`` is ignored."""
        ids, steps = ops.stack_captions(dec_seq_list)
        if steps != [int(s) for s in model_inputs[11]]:
            raise ValueError("score_captions: the captions' rows per video %r are not the batch's step counts %r" % (steps, list(model_inputs[11])))
        T, K, _, _ = ops.check_force(ids, self.max_t_len, steps, unk)
        r = self._translate(model_inputs, self.model, decode=Decode(FORCE, K, sampling=(unk, ids.dtype), given=ids))
        lists = {name: self._per_video(r[k], steps) for name, k in (
            ("score_list", "cum"), ("length_list", "length"), ("finished_list", "finished"), ("n_scored_list", "n_scored"),
            ("step_list", "step"), ("rank_list", "rank"), ("top_list", "top"), ("top_step_list", "top_step"))}
        return SimpleNamespace(**lists, **r)

    @torch.no_grad()
    def teacher_scores(self, model_inputs, dec_seq_list):
        """The forced pass of ``score_captions`` stopped before ``ops.force_score``: this translator's per-position distribution over GIVEN
        captions, the teacher's side of knowledge distillation (``svpc_amd.distill``).  ``model_inputs`` and
        ``dec_seq_list`` as ``score_captions`` takes them — the same checks, the same in-place blanking of the text half of the ids /
        masks.  → a namespace: ``scores`` (T·K·Lt, ld) fp32 — row (t·K + k)·Lt + i scores position i + 1 of caption k of sentence t; raw
        logits when ``logits`` (a single ``video``-mode model), else probabilities (an ensemble's combined matrix always) —, ``logits``,
        ``cap_c`` the T·K caption rows' column counts (an Idx), ``max_cols``, ``T``, ``K``, ``Lt``.  With ``graph=True`` this pass still
        runs EAGER: the matrix is a fresh tensor the caller owns, never a captured buffer, so it stays valid for as long as it is
        referenced (``score_captions`` keeps its graph).  No host synchronisation."""
        ids, steps = ops.stack_captions(dec_seq_list)
        if steps != [int(s) for s in model_inputs[11]]:
            raise ValueError("teacher_scores: the captions' rows per video %r are not the batch's step counts %r" % (steps, list(model_inputs[11])))
        _, K, _, _ = ops.check_force(ids, self.max_t_len, steps, "bar")
        decode = Decode(FORCE, K, sampling=("bar", ids.dtype, "raw"), given=ids)
        return SimpleNamespace(**self._translate(model_inputs, self.model, decode=decode))

    def gold_captions(self, input_labels_list, batch_step_num):
        """The reference captions of a batch as a ``dec_seq_list`` for ``score_captions``, on the device: ``input_labels_list`` the
        per-step (N, Lv + Lt) label tensors of the training batch (the label at text position j is the word at caption position
        j + 1; IGNORE elsewhere) → per video (S_b, Lt) int64: BOS, then the labels of text positions 0 … Lt − 2 with IGNORE turned into
        PAD — consecutive views of one buffer.  One index upload per call, no read-back."""
        Lv, Lt = self.max_v_len, self.max_t_len
        lab = input_labels_list                                # (S, N, L): the per-step tensors stacked (zero-copy for a stacked loader)
        if isinstance(lab, (list, tuple)):
            lab = StateAwareRecursiveTransformer._stacked(list(lab))
        steps = [int(s) for s in batch_step_num]
        if lab.dim() != 3 or lab.shape[2] < Lv + Lt or len(steps) != lab.shape[1] or any(not 0 <= s <= lab.shape[0] for s in steps):
            raise ValueError("gold_captions: labels must be (S, N, >= Lv + Lt) with one step count <= S per video")
        N = lab.shape[1]
        rows = torch.tensor([s * N + b for b, n in enumerate(steps) for s in range(n)], dtype=torch.int64).to(lab.device)
        text = lab.reshape(-1, lab.shape[2])[:, Lv:Lv + Lt - 1].index_select(0, rows).to(torch.int64)
        out = torch.empty(len(rows), Lt, dtype=torch.int64, device=lab.device)
        out[:, 0] = BOS
        out[:, 1:] = torch.where(text == IGNORE, torch.full_like(text, PAD), text)
        return self._per_video(out, steps)

    @torch.no_grad()
    def translate_batch_consensus(self, model_inputs, plan, source="sample", num_candidates=4, utility="CIDEr", scope="paragraph",
                                  weights="uniform", **decode_kw):
        """``translate_batch_sample(num_samples=num_candidates)`` (``source="sample"``), ``translate_batch_nbest(n_best=
        num_candidates)`` (``"nbest"``; ``beam_size`` defaults to ``num_candidates``) or ``translate_batch_diverse(num_groups=G,
        n_best=num_candidates / G)`` (``"diverse"``; ``beam_size`` defaults to ``num_candidates``) or
        ``translate_batch_stochastic(beam_size=num_candidates)`` (``"stochastic"``) followed by ``consensus`` →
        (dec_seq_list, oov_word_dict, pick_list): one (S_b, Lt) int64 caption matrix per video, as greedy returns."""
        ops.check_consensus(num_candidates, utility, scope, weights)
        if source == "sample":
            dec, oov, sc, ln = self.translate_batch_sample(model_inputs, num_samples=num_candidates, **decode_kw)
        elif source == "nbest":
            beam = decode_kw.pop("beam_size", num_candidates)
            dec, oov, sc, ln = self.translate_batch_nbest(model_inputs, beam, num_candidates, **decode_kw)
        elif source == "diverse":
            beam = decode_kw.pop("beam_size", num_candidates)
            groups = decode_kw.pop("num_groups", getattr(self.opt, "num_groups", 1))
            W, G, _, _ = ops.check_diverse(beam, groups, 0.0)
            if num_candidates % G or not 1 <= num_candidates // G <= W // G:
                raise ValueError("num_candidates must be num_groups times 1..%d rows per group, got %d with %d groups" % (W // G, num_candidates, G))
            dec, oov, sc, ln = self.translate_batch_diverse(model_inputs, W, G, decode_kw.pop("diversity_strength", None), num_candidates // G,
                                                            **decode_kw)
        elif source == "stochastic":
            dec, oov, sc, ln = self.translate_batch_stochastic(model_inputs, num_candidates, **decode_kw)[:4]
        else:
            raise ValueError("source must be \"sample\", \"nbest\", \"diverse\" or \"stochastic\", got %r" % (source,))
        r = self.consensus(dec, plan, sc, ln, utility, scope, weights)
        return r.dec_seq_list, oov, r.pick_list

    # ------------------------------------------------------------------ host part: everything that depends on the batch STRUCTURE only
    def _prepare(self, model, decode, batch_step_num, ingr_sep_masks, ingr_id_dict, oov_word_dict, S_pad, N, L, dev):
        cfg = model.config
        mode = cfg.model_mode
        Lt, V = cfg.max_t_len, cfg.vocab_size
        sep_t = torch.as_tensor(ingr_sep_masks).cpu()
        dicts = ingr_id_dict if mode != "video" else [{}] * N
        n_oov = [len(d) if mode != "video" else 0 for d in oov_word_dict]
        key = (tuple(int(v) for v in batch_step_num), sep_t.numpy().tobytes(), tuple(n_oov), S_pad, N, L, str(dev), self.incremental,
               tuple(tuple((int(e), tuple(int(i) for i in lst)) for e, lst in d.items()) for d in dicts)) + decode.key
        dp = self._preps.get(key)
        if dp is not None:
            return dp
        spans = model.ingredient_embeddings.spans(sep_t)   # one host read per batch structure
        plan = model.plan_for(batch_step_num, spans[3], S_pad, N, L, dev)
        T, W = plan.T, decode.width
        c_list = [V + x_ for x_ in n_oov]
        dp = DecodePlan(key=key, spans=spans, plan=plan, c_list=c_list, T=T, kind=decode.kind, width=W, ranked=decode.ranked)
        if decode.kind == FORCE:
            self._prepare_force(model, dp, decode, dicts, c_list, dev)
        elif not self.incremental:
            dp.ptr_all, dp.x_all = model._ptr_plan(dicts, c_list, Lt, plan.step_ne, plan.row_vid), Idx([n_oov[b] for b in plan.row_vid.host])
        else:
            # hypothesis rows t·W + h: the pointer plan of W rows per sentence (ptr_attn_gate / ptr_mix_loss with lt = W)
            row_vid = plan.step_vid if decode.kind == GREEDY else Idx([b for b in plan.step_vid.host for _ in range(W)])
            dp.ptr_hyp, dp.x_hyp = model._ptr_plan(dicts, c_list, W, plan.step_ne, row_vid), Idx([n_oov[b] for b in row_vid.host])
        if decode.ranked:
            # the controls' device tables live as long as the plan: a replayed graph reads the addresses it captured
            c = decode.controls
            n = c["block_ngram_repeat"]
            dp.controls = dict(
                min_length=c["min_length"], block_ngram_repeat=n,
                exclusion=(exclusion_bitmap(c["exclusion_tokens"], V, dev), V) if n and c["exclusion_tokens"] else None,
                lp=(torch.tensor(length_penalty_table(c["length_penalty_name"], c["length_penalty_alpha"], Lt), dtype=torch.float64,
                                 device=dev) if c["length_penalty_name"] != "none" else None))
            if c["block_ngram_scope"] == "paragraph":
                dp.rounds = self._paragraph_rounds(model, plan, dicts, c_list, n_oov, W, Lt, dev)
                dp.rows_max = max(rd.n for rd in dp.rounds) * W
        if decode.groups is not None:          # (like lp: the table lives as long as the plan and its captured graphs)
            dp.groups = decode.groups[0]
            dp.pen = torch.tensor(ops.diversity_table(decode.groups[1], W), dtype=torch.float32, device=dev)
        if decode.constrained:                 # the call's constraint table is copied into this buffer before the eager run or the replay
            dp.cons = torch.empty(T, ops.CONS_MAX, ops.CONS_LEN, dtype=torch.int32, device=dev)
        if decode.kind == SAMPLE:
            # every sample's ancestry is itself, so the KV-cache rows of row r are r·Lt + j (one static table); the seed source (fixed,
            # value) and the seed the decode used are captured device words
            temp, topk, topp, m = decode.sampling
            dp.sampling = dict(temp=temp, topk=topk, topp=topp, min_length=m, max_cols=dp.ptr_hyp["c_max"])
            dp.key_rows = (torch.arange(T * W, dtype=torch.int32, device=dev).unsqueeze(1) * Lt +
                           torch.arange(Lt, dtype=torch.int32, device=dev)).contiguous()
            dp.seed_src, dp.seed_used = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
            if decode.truncation is not None:      # every step's kept-set sizes: a buffer of the plan, so a replayed graph fills it again
                dp.truncation = dict(zip(self.TRUNCATION, decode.truncation))
                dp.kept = torch.zeros(Lt - 1, T * W, dtype=torch.int32, device=dev)
        if decode.stochastic is not None:      # the seed source and the seed the decode used: captured device words, as sampling's
            temp, m = decode.stochastic
            dp.stochastic = dict(temp=temp, min_length=m, max_cols=dp.ptr_hyp["c_max"])
            dp.seed_src, dp.seed_used = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        if decode.contrastive is not None:     # (k is the plan's width; α and m travel by value into every launch)
            _, alpha, m = decode.contrastive
            dp.contrastive = dict(alpha=alpha, min_length=m, max_cols=dp.ptr_hyp["c_max"])
        if len(self._preps) > 32:
            self._preps.clear()
        self._preps[key] = dp
        return dp

    @staticmethod
    def _prepare_force(model, dp, decode, dicts, c_list, dev):
        """Forced scoring's part of the plan: the T·K caption rows of Lt positions as one decoder pass.  The K captions of a sentence
        share its memory rows through the cross segmentation (row r over the memory rows of sentence r // K) and its pointer bank
        through one (row offset, row count) table per k; the pointer plan has K·Lt rows per sentence; the given ids have a buffer of
        their own, which a captured graph reads."""
        plan, T, K, Lt = dp.plan, dp.T, dp.width, model.config.max_t_len
        n_mem, R = model._n_mem(), dp.T * dp.width
        dp.unk, id_dtype = decode.sampling[:2]
        dp.raw = len(decode.sampling) > 2          # (``teacher_scores``: a third entry of the setting, so a plan of its own)
        dp.given = torch.empty(T, K, Lt, dtype=id_dtype, device=dev)
        dp.cap_c = Idx([c_list[b] for b in plan.step_vid.host for _ in range(K)])
        dp.ptr_force = model._ptr_plan(dicts, c_list, K * Lt, plan.step_ne, Idx([b for b in plan.step_vid.host for _ in range(K * Lt)]))
        if K == 1:
            dp.force_self, dp.force_cross = plan.seq_dec_self, plan.seq_dec_cross
        else:
            dp.force_self = SeqInfo.uniform(R, Lt, Lt, dev)
            dp.force_cross = SeqInfo([r * Lt for r in range(R)], [Lt] * R, [(r // K) * n_mem for r in range(R)], [n_mem] * R, dev)
        lens = torch.full((T,), Lt, dtype=torch.int32, device=dev)
        dp.group_rows = [(torch.tensor([(t * K + k) * Lt for t in range(T)], dtype=torch.int32, device=dev), lens) for k in range(K)]

    @staticmethod
    def _paragraph_rounds(model, plan, dicts, c_list, n_oov, B, Lt, dev):
        """The round tables of a paragraph-scope decode (round s: sentence s of every video with S_b > s, N_s·B hypothesis rows), all
        sent in one copy: per round its sentences' global indices (int64, for the scatters; int32, for the row gathers), the memory rows
        of its sentences, the pointer plan and OOV counts of its rows, the history descriptors (first top-1 row of the video, count s),
        and the attention segmentations."""
        steps, off = plan.h_step_len, plan.h_step_off
        n_mem = model._n_mem()
        ne = plan.step_ne.host
        up = BulkUpload(dev)
        rounds = []
        for s_ in range(max(steps)):
            vids = [b for b in range(plan.N) if steps[b] > s_]
            sent = [off[b] + s_ for b in vids]
            Ns = len(sent)
            TB = Ns * B
            row_vid = Idx([b for b in vids for _ in range(B)])
            rd = SimpleNamespace(n=Ns, step_ne=Idx([ne[t] for t in sent]), row_vid=row_vid, row_xb=Idx([n_oov[b] for b in row_vid.host]),
                                 desc=Idx([v for b in vids for v in (off[b], s_)]), sent32=Idx(sent),
                                 mem_rows=Idx([t * n_mem + j for t in sent for j in range(n_mem)]),
                                 seq_cross=SeqInfo(list(range(TB)), [1] * TB, [(r // B) * n_mem for r in range(TB)], [n_mem] * TB, None),
                                 seq_self=[SeqInfo.uniform(TB, 1, i + 1, None) for i in range(Lt - 1)])
            rd.plb = model._ptr_plan(dicts, c_list, B, rd.step_ne, row_vid)
            up.add(np.asarray(sent, dtype=np.int64).view(np.int32), sink=lambda t, rd=rd: setattr(rd, "sent64", t.view(torch.int64)))
            for v in (rd.step_ne, row_vid, rd.row_xb, rd.desc, rd.sent32, rd.mem_rows) + tuple(
                    rd.plb[k] for k in ("csr_off", "csr_ent", "csr_id", "csr_w", "row_c")):
                up.add_idx(v)
            for sq in [rd.seq_cross] + rd.seq_self:
                up.add_seq(sq)
            rounds.append(rd)
        up.flush()
        return rounds

    def _text_table(self, model, Lt, cx, dev):
        """(Lt, V, D): text_embeddings(token v at position p) for every (p, v) — inference weights are constant, so the embedding stack
        (word vector → LayerNorm → projection → ReLU → LayerNorm, + position encoding; model.py:484-513) is evaluated once per checkpoint
        for the whole vocabulary with the product's own kernels and the decoding iterations gather rows.  None outside eval mode."""
        if model.training or dev.type != "cuda":
            return None
        te = model.text_embeddings
        ps = [te.word_embeddings.weight] + list(te.word_fc.parameters())
        from .optim import WEIGHTS_EPOCH
        key = (tuple((p.data_ptr(), p._version) for p in ps), WEIGHTS_EPOCH[0], ops.get_precision(), Lt)
        tt = self._ttab.get(id(model))
        if tt is None or tt[0] != key:
            V = te.word_embeddings.weight.shape[0]
            ids = torch.arange(V, dtype=torch.int32, device=dev)
            base = te.word_fc.run(te.word_embeddings.weight, cx.eps, src_rows=ids, pad_row=PAD)
            tt = self._ttab[id(model)] = (key, (base.unsqueeze(0) + te.position_embeddings_text.pe[:Lt].unsqueeze(1)).contiguous())
        return tt[1]

    # ------------------------------------------------------------------ device part: encoder side once, then the decoding iterations
    def _decode_core(self, model, dp, feats, ids_all, masks_all, ingr_ids_flat):
        """→ (ids (T, K, Lt) int32, cum (T, K) fp32 or None, len (T, K) int32 or None): K = 1 (greedy, the plain beam: the chosen
        caption), B (ranked: final-key order) or R (samples in sample order)"""
        cx = _Ctx(model.config, False, model.rng(feats.device))
        stamps = self.phase_events if (self.phase_events is not None and not torch.cuda.is_current_stream_capturing()) else None

        def stamp():
            if stamps is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                stamps.append(e)
        stamp()
        enc = self._encode(model, dp, feats, ids_all, masks_all, ingr_ids_flat, cx)
        stamp()          # encoder side (clip encoder, step encoder, simulator, memory) done; the Lt decoding iterations follow
        if dp.kind == FORCE:
            out = self._force(model, dp, enc, cx)
        elif not self.incremental:
            out = self._greedy_rerun(model, dp, enc[0], enc[1], cx)
        else:
            side = self._side(model, dp, enc, cx)
            loop = (self._sample_iterations if dp.kind == SAMPLE else self._paragraph_iterations if dp.rounds is not None else
                    self._contrastive_iterations if dp.contrastive is not None else
                    self._beam_iterations if dp.kind == BEAM else self._greedy_iterations)
            out = loop(dp, side)
        stamp()
        return out

    # the three seams of ``_decode_core`` an ensemble overrides (svpc_amd/ensemble.py): what the encoder side hands on, the decoder side of
    # the incremental loops, and forced scoring
    def _encode(self, model, dp, feats, ids_all, masks_all, ingr_ids_flat, cx):
        return self._encoder_side(model, dp, feats, ids_all, masks_all, ingr_ids_flat, cx)

    def _side(self, model, dp, enc, cx):
        mem, bank = enc
        return _DecoderSide(model, cx, mem, bank, self._text_table(model, model.config.max_t_len, cx, mem.device), dp.T)

    def _force(self, model, dp, enc, cx):
        if dp.raw:                                 # ``teacher_scores``: the forced pass stopped before ``_force_finish``
            text, tmask, _tgt, _len, _fin = self._force_inputs(model, dp)
            scores = self._force_scores(model, dp, enc[0], enc[1], cx, text, tmask)
            return self._force_raw(model, dp, scores, model.config.model_mode == "video")
        return self._force_pass(model, dp, enc[0], enc[1], cx)

    @staticmethod
    def _force_raw(model, dp, scores, logits):
        """what ``teacher_scores`` returns of a (T·K·Lt, C) score matrix (logits when ``logits``)"""
        return dict(scores=scores, logits=bool(logits), cap_c=dp.cap_c, max_cols=max(dp.c_list), T=dp.T, K=dp.width,
                    Lt=model.config.max_t_len)

    def _members(self):
        """the models a decode of this translator reads: a captured graph is valid while all of them stay where they were"""
        return [self.model]

    @staticmethod
    def _encoder_side(model, dp, feats, ids_all, masks_all, ingr_ids_flat, cx):
        """The encoder side of one model over the whole batch → (mem, bank): the memory rows of every sentence (n_mem per sentence) and
        the pointer bank (None in ``video`` mode)"""
        mode = model.config.model_mode
        plan, T, D = dp.plan, dp.T, model.config.hidden_size
        ents = model.ingredient_embeddings.run(ingr_ids_flat, dp.spans, cx)
        cls = model._encode_clips(feats, plan.video_rows, ops.take_rows(ids_all, plan.video_rows),
                                  ops.take_rows(masks_all, plan.video_rows), plan.seq_enc, cx,
                                  cls_only=(plan.cls_rows_dev, plan.seq_enc_cls))
        x = ops.span_mean(cls, plan.arange_T, plan.ones_T, add=model.step_positional_encoding.pe, add_idx=plan.step_idx)
        g = model.step_wise_encoder.run(x, plan.seq_step, None, cx)
        if mode in ("full", "reason_copy"):
            _, _, ebar, eall, fbar = model.reasoner.run(g, ents, plan.sim, cx)
            went = ops.linear(ebar, model.Went[0].weight, model.Went[0].bias, act=ACT_RELU)
            wac = ops.linear(fbar, model.Wac[0].weight, model.Wac[0].bias, act=ACT_RELU)
            return torch.stack([g, went, wac], 1).reshape(T * 3, D), eall
        if mode == "copy":
            mean_ing = ops.span_mean(ents, plan.ent_off, plan.ent_len)
            return torch.stack([g, ops.take_rows(mean_ing, plan.step_vid_dev)], 1).reshape(T * 2, D), model._padded_bank(ents, plan)
        return g, None

    @staticmethod
    def _greedy_iterations(dp, side):
        """greedy, incremental: the Lt iterations over the T sentences, each a row of its own (no ancestry table, group 1)"""
        cfg = side.model.config
        T, Lt, dev = dp.T, cfg.max_t_len, side.wide[0].device
        text = torch.full((T, Lt), PAD, dtype=torch.int32, device=dev)
        ext = torch.full((T, Lt), PAD, dtype=torch.int32, device=dev)
        nxt = torch.full((T,), BOS, dtype=torch.int32, device=dev)
        nxt_ext = nxt.clone()
        caches, rows, seq_cross = side.caches(T), side.rows(), side.seq_cross(dp)
        text[:, 0] = nxt                    # (position i + 1 of both id matrices is written by iteration i's pick)
        ext[:, 0] = nxt_ext
        for i in range(Lt):
            scores = side.scores(rows, dp.ptr_hyp, nxt, i, caches, dp.plan.seq_dec_incremental(i, Lt, dev), seq_cross)
            nxt_ext, nxt = ops.greedy_pick(scores, dp.ptr_hyp["row_c"], dp.x_hyp, 1, 0, UNK, append=(text, ext, i + 1) if i + 1 < Lt else None)
        return (text if cfg.model_mode == "video" else ext).unsqueeze(1), None, None

    @staticmethod
    def _greedy_rerun(model, dp, mem, bank, cx):
        """greedy, ``incremental=False``: every iteration re-runs all Lt positions, as the reference does (the parity tests' reference form)"""
        cfg = model.config
        mode, plan, T, Lt, dev = cfg.model_mode, dp.plan, dp.T, cfg.max_t_len, mem.device
        text = torch.full((T, Lt), PAD, dtype=torch.int32, device=dev)
        ext = torch.full((T, Lt), PAD, dtype=torch.int32, device=dev)
        nxt = torch.full((T,), BOS, dtype=torch.int32, device=dev)
        nxt_ext = nxt.clone()
        tmask = torch.zeros(T, Lt, dtype=torch.float32, device=dev)
        for i in range(Lt):
            text[:, i] = nxt
            ext[:, i] = nxt_ext
            tmask[:, i] = 1.0
            xt = model.text_embeddings.run(text.reshape(-1), Lt, cx)
            dec = model.decoder.run(xt, tmask.reshape(-1), mem, plan.seq_dec_self, plan.seq_dec_cross, None, cx)
            if mode == "video":
                scores = model.decoder_classifier.run(dec, cx.eps)          # raw logits (translator.py:159)
            else:
                scores, _ = model._lm_probs(dec, bank, dp.ptr_all, cx)
            nxt_ext, nxt = ops.greedy_pick(scores, dp.ptr_all["row_c"], dp.x_all, Lt, i, UNK)
        return (text if mode == "video" else ext).unsqueeze(1), None, None

    @staticmethod
    def _force_pass(model, dp, mem, bank, cx):
        """Forced scoring: ONE pass of the decoder side over the Lt positions of all T·K given captions (the all-positions form of
        ``_greedy_rerun``: causal ∧ pad mask, so position i sees positions 0 … i of its own caption), then ``ops.force_score`` over the
        (T·K·Lt, C) score matrix → a dict of flat device tensors (``score_captions``)."""
        text, tmask, tgt, length, fin = Translator._force_inputs(model, dp)
        scores = Translator._force_scores(model, dp, mem, bank, cx, text, tmask)
        return Translator._force_finish(model, dp, scores, tgt, length, fin, model.config.model_mode == "video")

    @staticmethod
    def _force_inputs(model, dp):
        """the given captions as the decoder takes them → (text, tmask, tgt, length, fin) (``ops.force_inputs``)"""
        return ops.force_inputs(dp.given, model.config.vocab_size, UNK, EOS, PAD, IGNORE)

    @staticmethod
    def _force_scores(model, dp, mem, bank, cx, text, tmask):
        """the (T·K·Lt, C) score matrix of one model over the given captions: raw logits in ``video`` mode, else the mixed probabilities"""
        cfg = model.config
        Lt = cfg.max_t_len
        xt = model.text_embeddings.run(text.reshape(-1), Lt, cx)
        dec = model.decoder.run(xt, tmask.reshape(-1), mem, dp.force_self, dp.force_cross, None, cx)
        logits = model.decoder_classifier.run(dec, cx.eps)
        if cfg.model_mode == "video":
            return logits                                     # raw logits: the step score is their log_softmax (translator.py:159)
        pl = dp.ptr_force
        pi = g = None
        if bank is not None:        # the K captions of a sentence read its bank: one launch per k, nothing replicated
            pi, g = ops.ptr_attn_gate_groups(dec, model.bank_projection(bank), bank, pl["step_ne"], Lt, dp.group_rows,
                                             model.pgen_linear[0].weight, model.pgen_linear[0].bias)
        labels = torch.full((dec.shape[0],), -1, dtype=torch.int32, device=dec.device)
        return ops.ptr_mix_loss(logits, g, pi, labels, pl["row_c"], pl["row_vid"], pl["csr_off"], pl["csr_ent"], pl["csr_id"],
                                pl["csr_w"], pl["c_max"], model.label_smoothing)[0]

    @staticmethod
    def _force_finish(model, dp, scores, tgt, length, fin, logits):
        """``ops.force_score`` over a (T·K·Lt, C) score matrix (logits when ``logits``) → the dict ``score_captions`` splits"""
        K, T, Lt = dp.width, dp.T, model.config.max_t_len
        r = ops.force_score(scores, dp.cap_c, tgt, length, logits, UNK, dp.unk, max_cols=max(dp.c_list))
        return dict(cum=r["cum"].view(T, K), length=length.view(T, K), finished=fin.view(T, K), n_scored=r["n_scored"].view(T, K),
                    step=r["step"].view(T, K, Lt - 1), rank=r["rank"].view(T, K, Lt - 1), top=r["top"].view(T, K, Lt - 1),
                    top_step=r["top_step"].view(T, K, Lt - 1))

    @staticmethod
    def _self_segs(dp, Lt, dev):
        """the self-attention segmentations of the T·width hypothesis rows: at iteration i every row over its i + 1 ancestry rows"""
        if dp.seq_self is None:
            dp.seq_self = [SeqInfo.uniform(dp.T * dp.width, 1, i + 1, dev) for i in range(Lt - 1)]
        return dp.seq_self

    def _beam_iterations(self, dp, side):
        """A beam decode over the T·B hypothesis rows of the whole batch → (ids (T, 1, Lt) int32, score (T, 1) fp32, None); with controls
        or n-best (``dp.ranked``) → (ids (T, B, Lt) int32, cum (T, B) fp32, len (T, B) int32) in final-key order; stochastic beam search
        → (ids, cum, len, G (T, B) float64, phi (T, B) float64) in the order drawn."""
        dev = side.wide[0].device
        if dp.stochastic is not None:          # this decode's seed, on the device, exactly as ``_sample_iterations`` takes it
            ops.sample_seed(dp.seed_src, self._seed_word_on(dev), dp.seed_used)
        return self._beam_search(dp, side, side.rows(), dp.T, dp.ptr_hyp, dp.x_hyp, side.caches(dp.T * dp.width),
                                 self._self_segs(dp, side.model.config.max_t_len, dev), side.seq_cross(dp))

    @staticmethod
    def _beam_search(dp, side, rows, n_sent, ptr, row_x, caches, seq_self, seq_cross, history=None):
        """The Lt − 1 selection steps of a beam decode over n_sent·B hypothesis rows, then the final pick.  The ping-pong (text ids,
        extended ids, KV-cache ancestry) pairs — children are written from their parents' rows — start with BOS and the row's own slot at
        position 0, cum with beam 0 alone.  ``history``: ``ops.beam_step``'s, of a paragraph round.  Diverse beam search (``dp.groups``):
        cum and the selection score aug start with row 0 of every group alone, the step is ``ops.beam_step_groups``, and the final
        order is taken per group (the n-best final pick over n_sent·G "sentences" of Bg rows) → the B rows group-major.  Constrained
        beam search (``dp.cons``): every row carries a tracker state (start 0), the step is ``ops.beam_step_cons`` and the final pick
        ``ops.beam_finalize_cons`` → (ids, cum, len, met).  Stochastic beam search (``dp.stochastic``): every row also carries phi
        and G (float64; start 0 on row 0, −inf on the dead rows 1 … B − 1, which start finished), the step is
        ``ops.stochastic_beam_step`` with the seed ``dp.seed_used`` holds, and there is no final pick: the rows are already in the order
        drawn → (ids, cum, len, G, phi)."""
        cfg = side.model.config
        B, Lt, dev = dp.width, cfg.max_t_len, side.wide[0].device
        TB = n_sent * B
        toks = [[torch.full((TB, Lt), PAD, dtype=torch.int32, device=dev) for _ in range(3)] for _ in range(2)]
        toks[0][0][:, 0] = BOS
        toks[0][1][:, 0] = BOS
        toks[0][2][:, 0] = torch.arange(TB, dtype=torch.int32, device=dev) * Lt
        G = dp.groups
        if G is None:
            cum = torch.zeros(n_sent, B, dtype=torch.float32, device=dev)
            cum[:, 1:] = float("-inf")                                         # the first step: beam 0 alone
        else:
            cum = torch.zeros(n_sent, G, B // G, dtype=torch.float32, device=dev)
            cum[:, :, 1:] = float("-inf")                                      # … row 0 of every group alone
        cum = cum.view(TB)
        aug = cum.clone() if G is not None else None
        cstate = torch.zeros(TB, dtype=torch.int32, device=dev) if dp.cons is not None else None
        fin = torch.zeros(TB, dtype=torch.int32, device=dev)
        nxt = torch.full((TB,), BOS, dtype=torch.int32, device=dev)
        length = torch.zeros(TB, dtype=torch.int32, device=dev) if dp.ranked or dp.stochastic is not None else None   # lengths tracked
        phi = gk = None
        if dp.stochastic is not None:
            phi = cum.to(torch.float64)
            gk = phi.clone()
            fin = torch.isinf(cum).to(torch.int32)
        ctl = dict(dp.controls, length=length, history=history) if dp.ranked else {}
        for i in range(Lt - 1):
            t_in, t_out = toks[i % 2], toks[(i + 1) % 2]
            scores = side.scores(rows, ptr, nxt, i, caches, seq_self[i], seq_cross, t_in[2], B)
            if phi is not None:
                _, _, nxt = ops.stochastic_beam_step(scores, ptr["row_c"], row_x, B, i, side.logits, UNK, EOS, PAD, cum, phi, gk,
                                                     fin, length, t_in, t_out, Lt, dp.seed_used, **dp.stochastic)
            elif cstate is not None:
                _, _, nxt = ops.beam_step_cons(scores, ptr["row_c"], row_x, B, i, side.logits, UNK, EOS, PAD, cum, cstate, fin,
                                               length, t_in, t_out, Lt, dp.cons, **dp.controls)
            elif G is None:
                _, _, nxt = ops.beam_step(scores, ptr["row_c"], row_x, B, i, side.logits, UNK, EOS, PAD, cum, fin, t_in, t_out, Lt,
                                          **ctl)
            else:
                _, _, nxt = ops.beam_step_groups(scores, ptr["row_c"], row_x, B, G, i, side.logits, UNK, EOS, PAD, cum, aug, fin,
                                                 length, t_in, t_out, Lt, dp.pen, **dp.controls)
        ext = toks[(Lt - 1) % 2][1]
        if phi is not None:      # no final re-ranking: selection order is descending G, the order drawn
            return ext.view(n_sent, B, Lt), cum.view(n_sent, B), length.view(n_sent, B), gk.view(n_sent, B), phi.view(n_sent, B)
        if cstate is not None:   # all B hypotheses: more constraints met first, then the final key
            return ops.beam_finalize_cons(cum, ext, B, B, cstate, length, dp.controls["lp"])
        if G is not None:    # every group's rows in final-key order
            ids, score, ln = ops.beam_finalize_nbest(cum, ext, B // G, B // G, length, dp.controls["lp"])
            return ids.view(n_sent, B, Lt), score.view(n_sent, B), ln.view(n_sent, B)
        if dp.ranked:        # all B hypotheses in final-key order: translate_batch_beam keeps row 0, translate_batch_nbest n_best rows
            return ops.beam_finalize_nbest(cum, ext, B, B, length, dp.controls["lp"])
        ids, score = ops.beam_finalize(cum, ext, B)
        return ids.unsqueeze(1), score.unsqueeze(1), None

    def _paragraph_iterations(self, dp, side):
        """A paragraph-scope beam decode: the Lt − 1 selection steps (svpc_beam_step_para) run once per round, round s over the N_s·B
        rows of sentence s of every video with S_b > s, reading the chosen captions of rounds 0 … s − 1 from the decode's (T, Lt) top-1
        matrix.  Each round gathers its sentences' rows of the memory K|V projection, the pointer bank and its projection; the per-layer
        KV caches are sized for the largest round and reused (a round reads only rows it wrote).  → (ids (T, B, Lt) int32, cum (T, B)
        fp32, len (T, B) int32) in final-key order, as ``_beam_iterations`` with controls."""
        B, T, Lt, dev = dp.width, dp.T, side.model.config.max_t_len, side.wide[0].device
        caches = side.caches(dp.rows_max)
        ids = torch.full((T, B, Lt), PAD, dtype=torch.int32, device=dev)
        cums = torch.empty(T, B, dtype=torch.float32, device=dev)
        lens = torch.empty(T, B, dtype=torch.int32, device=dev)
        top1 = torch.full((T, Lt), PAD, dtype=torch.int32, device=dev)        # the chosen captions: the later rounds' history
        for rd in dp.rounds:
            r_ids, r_cum, r_len = self._beam_search(dp, side, side.rows(rd), rd.n, rd.plb, rd.row_xb, [c[:rd.n * B * Lt] for c in caches],
                                                    rd.seq_self, rd.seq_cross, history=(top1, rd.desc, BOS))
            ids.index_copy_(0, rd.sent64, r_ids)
            cums.index_copy_(0, rd.sent64, r_cum)
            lens.index_copy_(0, rd.sent64, r_len)
            top1.index_copy_(0, rd.sent64, r_ids[:, 0])
        return ids, cums, lens

    def _sample_iterations(self, dp, side):
        """A sampling decode: the Lt − 1 steps over the T·R sample rows, every row alive at BOS and its own ancestry (``dp.key_rows``),
        one (text ids, extended ids) pair written in place by ``ops.sample_step`` → (ids (T, R, Lt) int32, cum (T, R) fp32, len (T, R)
        int32) in sample order."""
        cfg = side.model.config
        R, T, Lt, dev = dp.width, dp.T, cfg.max_t_len, side.wide[0].device
        n = T * R
        text = torch.full((n, Lt), PAD, dtype=torch.int32, device=dev)
        text[:, 0] = BOS
        ext = text.clone()
        cum = torch.zeros(n, dtype=torch.float32, device=dev)
        ops.sample_seed(dp.seed_src, self._seed_word_on(dev), dp.seed_used)
        fin = torch.zeros(n, dtype=torch.int32, device=dev)
        nxt = torch.full((n,), BOS, dtype=torch.int32, device=dev)
        length = torch.zeros(n, dtype=torch.int32, device=dev)
        caches, rows, seq_self, seq_cross = side.caches(n), side.rows(), self._self_segs(dp, Lt, dev), side.seq_cross(dp)
        for i in range(Lt - 1):
            scores = side.scores(rows, dp.ptr_hyp, nxt, i, caches, seq_self[i], seq_cross, dp.key_rows, R)
            if dp.truncation is None:
                _, nxt = ops.sample_step(scores, dp.ptr_hyp["row_c"], dp.x_hyp, i, side.logits, UNK, EOS, PAD, cum, fin, length,
                                         text, ext, dp.seed_used, **dp.sampling)
            else:
                _, nxt, _ = ops.sample_step_trunc(scores, dp.ptr_hyp["row_c"], dp.x_hyp, i, side.logits, UNK, EOS, PAD, cum, fin, length,
                                                  text, ext, dp.seed_used, kept=dp.kept[i], **dp.sampling, **dp.truncation)
        return ext.view(T, R, Lt), cum.view(T, R), length.view(T, R)

    @staticmethod
    def _contrastive_iterations(dp, side):
        """A contrastive search: Lt decoder passes over the T·k candidate rows — one more than the other loops, because a word is chosen
        by its own hidden state, so the word at position Lt − 1 needs a pass too (without the head: it expands nothing) — each followed
        by ``ops.contrastive_step``, which commits the winner of every sentence and hands its top-k continuations to the k rows.  Row 0
        of a sentence starts alone live on BOS (p 1, step score 0); the ping-pong pairs are the beam decode's; the state is per sentence.
        There is no final pick → (ids (T, 1, Lt) int32, cum (T, 1) fp32, len (T, 1) int32, pen (T, 1, Lt) fp32)."""
        cfg = side.model.config
        k, T, Lt, D, dev = dp.width, dp.T, cfg.max_t_len, cfg.hidden_size, side.wide[0].device
        R = T * k
        toks = [[torch.full((R, Lt), PAD, dtype=torch.int32, device=dev) for _ in range(3)] for _ in range(2)]
        toks[0][0][:, 0] = BOS
        toks[0][1][:, 0] = BOS
        toks[0][2][:, 0] = torch.arange(R, dtype=torch.int32, device=dev) * Lt
        cand_p = torch.zeros(T, k, dtype=torch.float32, device=dev)
        cand_p[:, 0] = 1.0                                                     # iteration 0: row 0 alone
        cand_score = torch.full((T, k), float("-inf"), dtype=torch.float32, device=dev)
        cand_score[:, 0] = 0.0
        cand_p, cand_score = cand_p.view(R), cand_score.view(R)
        ids = torch.full((T, Lt), PAD, dtype=torch.int32, device=dev)
        cum = torch.zeros(T, dtype=torch.float32, device=dev)
        length = torch.zeros(T, dtype=torch.int32, device=dev)
        pen = torch.zeros(T, Lt, dtype=torch.float32, device=dev)
        fin = torch.zeros(T, dtype=torch.int32, device=dev)
        hist = torch.zeros(T, Lt, D, dtype=torch.float32, device=dev)
        hist_n2 = torch.zeros(T, Lt, dtype=torch.float64, device=dev)
        nxt = torch.full((R,), BOS, dtype=torch.int32, device=dev)
        caches, rows, seq_cross = side.caches(R), side.rows(), side.seq_cross(dp)
        if dp.seq_self is None:        # this decode's own list: Lt entries, the last one over Lt keys
            dp.seq_self = [SeqInfo.uniform(R, 1, i + 1, dev) for i in range(Lt)]
        for i in range(Lt):
            t_in, t_out = toks[i % 2], toks[(i + 1) % 2]
            scores, x = side.scores(rows, dp.ptr_hyp, nxt, i, caches, dp.seq_self[i], seq_cross, t_in[2], k, hidden=True, head=i + 1 < Lt)
            _, _, _, nxt = ops.contrastive_step(scores, dp.ptr_hyp["row_c"], dp.x_hyp, k, i, side.logits, UNK, EOS, PAD, ops.to_f32(x),
                                                cand_p, cand_score, ids, cum, length, pen, fin, hist, hist_n2, t_in, t_out, Lt,
                                                **dp.contrastive)
        return ids.unsqueeze(1), cum.unsqueeze(1), length.unsqueeze(1), pen.unsqueeze(1)

    def _seed_word_on(self, dev):
        """the sampling decodes' seed word (int64 (1,) on ``dev``): drawn once from torch's default generator, then advanced on the device
        by every decode with seed=None; a captured graph holds its address"""
        if self._seed_word is None or self._seed_word.device != torch.device(dev):
            self._seed_word = torch.randint(0, 1 << 62, (1,), dtype=torch.int64).to(dev)
        return self._seed_word

    @torch.no_grad()
    def translate_batch_greedy(self, input_ids_list, video_features_list, input_masks_list, token_type_ids_list,
                               ingr_input_ids, ingr_masks, ingr_sep_masks, ingr_id_dict, oov_word_dict, alignments, actions,
                               batch_step_num, rt_model):
        return self._translate([input_ids_list, video_features_list, input_masks_list, token_type_ids_list, ingr_input_ids, ingr_masks,
                                ingr_sep_masks, ingr_id_dict, oov_word_dict, alignments, actions, batch_step_num], rt_model, decode=Decode())

    def _translate(self, model_inputs, model, decode):
        (input_ids_list, video_features_list, input_masks_list, token_type_ids_list, ingr_input_ids, ingr_masks,
         ingr_sep_masks, ingr_id_dict, oov_word_dict, alignments, actions, batch_step_num) = model_inputs
        dev = video_features_list[0].device
        if decode.kind == SAMPLE and dev.type != "cuda":
            raise RuntimeError("sampling decodes on the GPU only (no CPU fallback exists)")
        if decode.stochastic is not None and dev.type != "cuda":
            raise ops._lib.SvpcKernelError("stochastic beam search decodes on the GPU only (no CPU fallback exists)")
        if decode.contrastive is not None and dev.type != "cuda":
            raise ops._lib.SvpcKernelError("contrastive search decodes on the GPU only (no CPU fallback exists)")
        if decode.kind == FORCE and dev.type != "cuda":
            raise ops._lib.SvpcKernelError("forced scoring runs on the GPU only (no CPU fallback exists)")
        # the text half of every step's ids / masks is blanked in place, as the reference does (translator.py:205-228).  When the per-step
        # tensors are consecutive slices of one buffer (the usual collate output; model._stacked sees it) that is three launches on the
        # stacked views instead of three per step
        stk = None
        if isinstance(input_ids_list, list) and dev.type == "cuda":
            views = [model._stacked(l) for l in (input_ids_list, input_masks_list, token_type_ids_list)]
            if all(v.data_ptr() == l[0].data_ptr() for v, l in zip(views, (input_ids_list, input_masks_list, token_type_ids_list))):
                stk = views
        if stk is not None:
            self.prepare_video_only_inputs(*stk)
        else:
            input_ids_list, input_masks_list = self.prepare_video_only_inputs(input_ids_list, input_masks_list, token_type_ids_list)
        N, L, F = video_features_list[0].shape
        S_pad = len(input_ids_list)
        feats4 = model._stacked(video_features_list)                                             # (S, N, L, F): zero-copy for a stacked loader
        ids3 = (stk[0] if stk is not None else torch.stack(input_ids_list))                      # (S, N, L)
        masks3 = (stk[1] if stk is not None else torch.stack(input_masks_list))
        ingr_all = torch.as_tensor(ingr_input_ids).to(dev).to(torch.int32)                       # (N, Li)
        sep_all = torch.as_tensor(ingr_sep_masks)

        def part(lo, hi, stream=None):
            n = hi - lo
            dp = self._prepare(model, decode, list(batch_step_num[lo:hi]), sep_all[lo:hi], list(ingr_id_dict[lo:hi]),
                               list(oov_word_dict[lo:hi]), S_pad, n, L, dev)
            if dp.seed_src is not None:       # the seed source of this call: a captured input, like the batch tensors
                dp.seed_src.copy_(torch.tensor([0, 0] if decode.seed is None else [1, decode.seed], dtype=torch.int64))
            if dp.given is not None:          # the captions to score: a captured input too
                dp.given.copy_(decode.given.view(dp.given.shape))
            if dp.cons is not None:           # the constraint table: one host-to-device copy per call
                dp.cons.copy_(decode.cons)
            src = (feats4[:, lo:hi], ids3[:, lo:hi], masks3[:, lo:hi], ingr_all[lo:hi])
            if not self.graph or dev.type != "cuda" or dp.raw:       # (``teacher_scores`` runs eager: its matrix is the caller's)
                out = self._decode_core(model, dp, src[0].reshape(S_pad * n * L, F), src[1].reshape(-1).to(torch.int32),
                                        src[2].reshape(-1).float(), src[3].reshape(-1))
            else:
                out = self._decode_graphed(model, dp, src, (S_pad, n, L, F), stream)
            if dp.seed_used is not None:
                self.last_sample_seed = dp.seed_used.clone()
            if decode.kind == SAMPLE:         # (the plan's own buffer, not a copy: the next decode of this setting fills it again)
                self.last_sample_kept = dp.kept
            return dp.plan, out

        # Two halves on two streams: the encoder side of a batch is bound by the matrix cores, the Lt decoding
        # iterations are chains of small dependent launches that leave the chip idle — two independent chains interleave.  Videos are
        # independent (the reference decodes them one by one, translator.py:175-191), so the ids are those of the unsplit decode bit for
        # bit (tests/test_config5_gpu.py).  Two replayed graphs on two streams, not one forked graph.
        halves = [(0, N)]
        if self.graph and self.two_streams and decode.kind == GREEDY and dev.type == "cuda" and N >= 2 * self.min_half:
            halves = [(0, N // 2), (N // 2, N)]
        if len(halves) == 1:
            plans_outs = [part(0, N)]
        else:
            from .graph import ops_stream, ops_stream_b
            cur = torch.cuda.current_stream()
            sa = cur if cur != torch.cuda.default_stream() else ops_stream()
            sb = ops_stream_b()
            plans_outs = []
            for (lo, hi), st in zip(halves, (sa, sb)):
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    plans_outs.append(part(lo, hi, st))
            for st in (sa, sb):
                cur.wait_stream(st)
        if decode.kind == FORCE:            # (one part: the halves are greedy's) the flat result, ``score_captions`` splits it
            return plans_outs[0][1]
        # every strategy's result: ids (T, K, Lt), cum (T, K) or None, len (T, K) or None.  The call returns the first n_best of the K rows
        # per sentence, or (n_best 0) the chosen caption alone, without lengths
        k = decode.n_best
        res, scores, lens, mets, gums, logqs, pens = [], [], [], [], [], [], []
        for plan, out in plans_outs:
            ids, cum, length = out[:3]
            met = out[3][:, :k].to(torch.int64) if decode.constrained else None
            gum, logq = (out[3], out[4]) if decode.stochastic is not None else (None, None)
            pen = out[3][:, 0] if decode.contrastive is not None else None
            if decode.contrastive is not None:         # one caption per sentence, with its length
                ids, cum, length = ids[:, 0], cum[:, 0].contiguous(), length[:, 0].to(torch.int64)
            elif k and decode.groups is not None and k < decode.width // decode.groups[0]:      # the first k rows of every group
                G, Bg = decode.groups[0], decode.width // decode.groups[0]
                ids, cum, length = (v.reshape(v.shape[0], G, Bg, *v.shape[2:])[:, :, :k].reshape(v.shape[0], G * k, *v.shape[2:])
                                    for v in (ids, cum, length))
                length = length.to(torch.int64)
            elif k:
                if decode.groups is not None:
                    k = decode.width
                ids, cum, length = ids[:, :k], cum[:, :k], length[:, :k].to(torch.int64)
            else:
                ids, cum, length = ids[:, 0], cum[:, 0].contiguous() if cum is not None else None, None
            ids = ids.to(torch.int64)                  # (one cast per part: the per-video results are views of it)
            for b in range(plan.N):
                o, n_ = plan.h_step_off[b], plan.h_step_len[b]
                for lst, t in ((res, ids), (scores, cum), (lens, length), (mets, met), (gums, gum), (logqs, logq), (pens, pen)):
                    if t is not None:
                        lst.append(t[o:o + n_])
        if decode.contrastive is not None:
            return res, oov_word_dict, scores, lens, pens
        if decode.constrained:
            return res, oov_word_dict, scores, lens, mets
        if decode.stochastic is not None:
            return res, oov_word_dict, scores, lens, gums, logqs
        return (res, oov_word_dict, scores, lens) if scores else (res, oov_word_dict)

    def _decode_graphed(self, model, dp, src, shape, stream=None):
        """The ≈2,000 launches of a batch's decode (encoder side + Lt iterations × 6 layers) replayed as ONE hipGraph.  The graph
        is tied to the batch structure (step / ingredient / OOV counts: ``_prepare``'s key): the first batch of a structure runs
        eagerly twice (warm-up: index tables reach the device, kernels set their attributes) and is then captured; later batches of
        the same structure copy their tensors into the captured inputs and replay.  ``src``: (features (S, n, L, F), ids (S, n, L),
        masks (S, n, L), ingredient ids (n, Li)) — possibly strided views of the whole batch (the copy into the captured inputs gathers them)."""
        # a captured graph holds raw pointers: it is valid only while the parameters (and, on the bf16 path, their shadow) live where
        # they lived at capture time — a weight store built later (optimizer start, WeightStore.for_model) re-points them
        from . import ops as _ops
        from .optim import WEIGHTS_EPOCH
        # (epoch + the embedding parameters' version counters: the graph holds the address of the per-checkpoint text-embedding table,
        # which ``_text_table`` rebuilds — elsewhere — when either moves: load_state_dict / copy_ into the same tensors bump only the versions)
        S_pad, n, L, F = shape
        from .graph import ops_stream
        cur = torch.cuda.current_stream()
        side = stream if stream is not None else (cur if cur != torch.cuda.default_stream() else ops_stream())
        mods = self._members()           # (every model the decode reads: an ensemble's graph holds all its members' addresses)
        sig = (tuple(p.data_ptr() for m in mods for p in list(m.parameters())[:8]), _ops.get_precision(),
               tuple(id(getattr(m, "_svpc_weight_store", None)) for m in mods), WEIGHTS_EPOCH[0],
               tuple(p._version for m in mods for p in [m.text_embeddings.word_embeddings.weight] + list(m.text_embeddings.word_fc.parameters())),
               side.cuda_stream)
        gkey = side.cuda_stream                      # one graph per replay stream: two halves of ONE structure must not share captured buffers
        g = dp.graphs.get(gkey)
        if g is not None and g[3] != sig:
            g = None
            dp.graphs.pop(gkey, None)

        def flat(st):
            return (st[0].view(S_pad * n * L, F), st[1].view(-1), st[2].view(-1), st[3].view(-1))
        if g is None:
            static = [torch.empty(S_pad, n, L, F, dtype=torch.float32, device=src[0].device),
                      torch.empty(S_pad, n, L, dtype=torch.int32, device=src[0].device),
                      torch.empty(S_pad, n, L, dtype=torch.float32, device=src[0].device),
                      torch.empty(src[3].shape, dtype=torch.int32, device=src[0].device)]
            for dst, s_ in zip(static, src):
                dst.copy_(s_)
            # warm-up and capture on ONE stream per half (svpc_amd.graph.ops_stream / ops_stream_b): a fresh stream per batch
            # structure would pin another 256 MB kernel workspace each (ops._ws is per (device, stream))
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self._decode_core(model, dp, *flat(static))
                self._decode_core(model, dp, *flat(static))
            cur.wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            from .graph import capturing
            with capturing(graph, stream=side):
                out = self._decode_core(model, dp, *flat(static))
            g = dp.graphs[gkey] = (graph, static, out, sig)
        graph, static, out, _ = g
        for dst, s_ in zip(static, src):
            dst.copy_(s_)
        graph.replay()
        if isinstance(out, dict):
            return {k: v.clone() for k, v in out.items()}
        return tuple(o.clone() if o is not None else None for o in out)
