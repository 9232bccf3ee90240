"""Self-critical sequence training (Rennie et al. 2017) over sampled captions: the training-time counterpart of consensus selection
(DESIGN §11.10).  ``SelfCritical.step`` samples K captions per sentence, scores every candidate paragraph against the video's references
on the device (``Translator.caption_scores``), turns the rewards into per-caption weights (``ops.scst_weights``: greedy, leave-one-out
mean or no baseline) and returns the loss −Σ w·log p(caption) of a graded forced pass (``sequence_loss``; ``ops.seq_nll``).  The caller runs
``graph.backward_all(model, loss)`` and the optimizer.

Sharing over K.  The K captions of a sentence read ONE memory and ONE pointer bank.  The graded pass replicates the sentence's memory rows,
its bank and the bank's projection K times through a differentiable row gather (a broadcast view made contiguous: its backward is the sum
over K), so the T·K caption rows are T·K independent "sentences" for every training kernel — the fused cross-attention, the pointer
attention + gate and their backwards run as they do in the train step, and no attention segmentation shares key rows (which
``ops.attention`` refuses under grad)."""
from types import SimpleNamespace

import torch

from . import ops
from .ops_common import ACT_RELU, Idx, SeqInfo
from .synthetic import EOS, IGNORE, PAD, UNK


def _replicate(t, K):
    """(T, …) → (T·K, …): row t·K + k is row t; differentiable, the backward sums the K copies in a fixed order"""
    if K == 1:
        return t
    return t.unsqueeze(1).expand(t.shape[0], K, *t.shape[1:]).reshape(t.shape[0] * K, *t.shape[1:])


class _ForcePlan(object):
    """the tables of a graded forced pass over one batch structure with K captions per sentence (cached on the model's plan)"""

    def __init__(self, model, plan, K, dicts, c_list, dev):
        cfg = model.config
        Lt, n_mem, T = cfg.max_t_len, model._n_mem(), plan.T
        R = T * K
        self.seq_self = SeqInfo.uniform(R, Lt, Lt, dev)
        self.seq_cross = SeqInfo.uniform(R, Lt, n_mem, dev)
        self.cap_vid = [b for b in plan.step_vid.host for _ in range(K)]
        self.cap_c = Idx([c_list[b] for b in self.cap_vid])
        self.step_ne = Idx([n for n in plan.step_ne.host for _ in range(K)])
        self.ptr = model._ptr_plan(dicts, c_list, Lt, self.step_ne, Idx([b for b in self.cap_vid for _ in range(Lt)]), device=dev)


def _force_plan(model, plan, K, dicts, c_list, dev):
    key = (K, tuple(c_list), tuple(tuple((int(e), tuple(int(i) for i in lst)) for e, lst in d.items()) for d in dicts), str(dev))
    cache = plan.__dict__.setdefault("_scst_plans", {})
    fp = cache.get(key)
    if fp is None:
        if len(cache) > 8:
            cache.clear()
        fp = cache[key] = _ForcePlan(model, plan, K, dicts, c_list, dev)
    return fp


def fresh_inputs(model, inputs):
    """the inputs with copies of the ids and masks (slots 0 and 2): a decode or a forced pass blanks their text half in place"""
    dec_in = list(inputs)
    dec_in[0] = list(model._stacked(list(inputs[0])).clone().unbind(0))
    dec_in[2] = list(model._stacked(list(inputs[2])).clone().unbind(0))
    return dec_in


class eval_mode(object):
    """``models`` (a translator's ``_members()``, or its one model) in eval mode, and those it switched back in training mode afterwards,
    also when the body raises.  A member already in eval mode is left alone: walking a model's modules twice per member and step is host
    time the eager passes do not hide."""

    def __init__(self, models):
        self.models = list(models)

    def __enter__(self):
        self.was = [m for m in self.models if m.training]
        for m in self.was:
            m.eval()

    def __exit__(self, *exc):
        for m in self.was:
            m.train(True)
        return False


def frozen_scores(scorer, model_inputs, dec_seq_list, field):
    """``scorer.score_captions(model_inputs, dec_seq_list).<field>`` of a frozen scorer, any ``Translator``, as a tensor of its own:
    without gradients, its members in eval mode (``eval_mode``), on copies of the ids and masks (``fresh_inputs``).  The result is a
    clone: with ``graph=True`` the pass's own buffer belongs to a captured graph and the next replay overwrites it."""
    models = list(scorer._members())
    inputs = fresh_inputs(models[0], model_inputs)
    with eval_mode(models), torch.no_grad():
        return getattr(scorer.score_captions(inputs, dec_seq_list), field).clone()


def row_weights(weights):
    """a head's optional per-caption weights (T, K) or (T·K,) → fp32 (T·K,) without a gradient, or None"""
    return None if weights is None else weights.detach().reshape(-1).to(torch.float32).contiguous()


def loss_result(p, loss, cum, step, barred, **own):
    """what every head over ``graded_pass`` returns: ``sequence_loss``'s namespace in its (T, K) views plus the head's ``own`` fields"""
    return SimpleNamespace(loss=loss, cum=cum.view(p.T, p.K), step=step.view(p.T, p.K, p.Lt - 1), barred=barred.view(p.T, p.K),
                           length=p.length.view(p.T, p.K), **own)


def per_token(p, *coefficients):
    """c / n per coefficient as an fp32 (R,) vector, n = max(1, Σ len) formed on the device in fp64 and rounded once; no read-back"""
    n = p.length.sum(dtype=torch.int64).clamp_(min=1).to(torch.float64)
    R = p.length.shape[0]
    return tuple((c / n).to(torch.float32).expand(R).contiguous() for c in coefficients)


class PhaseEvents(object):
    """``phase_events``: None, or a list to which ``_stamp`` appends a HIP event at each phase boundary of a step (the tools/bench_*
    scripts time the phases with them)"""
    phase_events = None

    def _stamp(self):
        if self.phase_events is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.phase_events.append(e)


def graded_pass(translator, model_inputs, dec_seq_list, weights, head, who="sequence_loss"):
    """The graded forced pass up to the decoder's score matrix, then ``head``: the encoder side of the decode and the decoder once over all
    positions of the T·K given captions, with gradients.  ``head`` is called inside the pass's ``enable_grad`` with a namespace — ``scores``
    (T·K·Lt, ≥ C) fp32 (probabilities, or raw logits when ``logits``), ``cap_c`` the rows' column counts (an Idx), ``max_cols``, ``tgt``
    (R, Lt) / ``length`` / ``finished`` (R,) int32 (``ops.force_inputs``'), ``steps`` the videos' sentence counts, ``plan`` the batch structure's plan, ``T``, ``K``, ``Lt``, ``hidden`` (T·K·Lt, D) the decoder's last-layer
    output the scores are read from (the activation stream's storage: ``ops.to_f32`` makes it fp32) — and
    its result is returned.  ``weights``: what ``ops.check_scst`` is to check beside the captions (``sequence_loss``'s weights)."""
    (input_ids_list, video_features_list, input_masks_list, _tt, ingr_input_ids, _im, ingr_sep_masks, ingr_id_dict, oov_word_dict,
     _al, _ac, batch_step_num) = model_inputs
    ids, steps = ops.stack_captions(dec_seq_list)
    if ids.dim() == 2:
        ids = ids.unsqueeze(1)
    if steps != [int(s) for s in batch_step_num]:
        raise ValueError("%s: the captions' rows per video %r are not the batch's step counts %r" % (who, steps, list(batch_step_num)))
    _, _, K = ops.check_scst(ids, baseline="none", lt=translator.max_t_len, steps=steps, weights=weights)
    model = translator.model
    cfg = model.config
    mode = cfg.model_mode
    dev = video_features_list[0].device
    if dev.type != "cuda":
        raise ops._lib.SvpcKernelError("%s runs on the GPU only (no CPU fallback exists)" % who)
    N, L, F = video_features_list[0].shape
    S_pad = len(input_ids_list)
    Lt, D, V = cfg.max_t_len, cfg.hidden_size, cfg.vocab_size
    with torch.enable_grad():
        cx = model._cx(dev)
        if model.training:
            cx.rng.begin_step()
        sep = torch.as_tensor(ingr_sep_masks)
        spans = model._spans_for(sep) if sep.is_cuda else model.ingredient_embeddings.spans(sep)
        plan = model.plan_for([int(s) for s in batch_step_num], spans[3], S_pad, N, L, dev)
        T = plan.T
        dicts = list(ingr_id_dict) if mode != "video" else [{}] * N
        c_list = [V + (len(d) if mode != "video" else 0) for d in oov_word_dict]
        fp = _force_plan(model, plan, K, dicts, c_list, dev)

        # the encoder side of the decode (Translator._decode_core) with gradients: only the clip rows of the ids / masks are read
        feats = model._stacked(list(video_features_list)).reshape(S_pad * N * L, F)
        ids_src, masks_src = (model._stacked(list(l)).reshape(-1) for l in (input_ids_list, input_masks_list))
        ids_v, mask_v, ingr_ids = ops.gather_cast_multi([(ids_src, plan.video_rows, torch.int32), (masks_src, plan.video_rows, torch.float32),
                                                         (torch.as_tensor(ingr_input_ids).to(dev), None, torch.int32)])
        ents = model.ingredient_embeddings.run(ingr_ids, spans, cx)
        cls = model._encode_clips(feats, plan.video_rows, ids_v, mask_v, plan.seq_enc, cx, cls_only=(plan.cls_rows_dev, plan.seq_enc_cls))
        x = ops.span_mean(cls, plan.arange_T, plan.ones_T, add=model.step_positional_encoding.pe, add_idx=plan.step_idx)
        g = model.step_wise_encoder.run(x, plan.seq_step, None, cx)
        if mode in ("full", "reason_copy"):
            _, _, ebar, eall, fbar = model.reasoner.run(g, ents, plan.sim, cx)
            went = ops.linear(ebar, model.Went[0].weight, model.Went[0].bias, act=ACT_RELU)
            wac = ops.linear(fbar, model.Wac[0].weight, model.Wac[0].bias, act=ACT_RELU)
            mem = torch.stack([g, went, wac], 1)
            bank = eall
        elif mode == "copy":
            mean_ing = ops.span_mean(ents, plan.ent_off, plan.ent_len)
            mem = torch.stack([g, ops.take_rows(mean_ing, plan.step_vid_dev)], 1)
            bank = model._padded_bank(ents, plan)
        else:
            mem = g.unsqueeze(1)
            bank = None

        # the decoder side over the T·K caption rows, each with its own copy of the sentence's memory rows and bank
        text, tmask, tgt, length, _fin = ops.force_inputs(ids, V, UNK, EOS, PAD, IGNORE)
        R = T * K
        mem_r = _replicate(mem, K).reshape(R * mem.shape[1], D)
        xt = model.text_embeddings.run(text.reshape(-1), Lt, cx, out_bf16=model.decoder.streams_bf16(R * Lt, D))
        dec = model.decoder.run(xt, tmask.reshape(-1), mem_r, fp.seq_self, fp.seq_cross, None, cx)
        if mode == "video":
            scores = model.decoder_classifier.run(dec, cx.eps)       # raw logits: the step score is their log-softmax without UNK
        else:
            proj = None
            if bank is not None:
                proj = _replicate(model.bank_projection(bank), K).contiguous()
                bank = _replicate(bank, K).contiguous()
            scores = model._lm_probs(dec, bank, fp.ptr, cx, proj=proj)[0]
        return head(SimpleNamespace(scores=scores, cap_c=fp.cap_c, max_cols=max(c_list), logits=mode == "video", tgt=tgt, length=length,
                                    finished=_fin, steps=steps, plan=plan, T=T, K=K, Lt=Lt, hidden=dec))


def sequence_loss(translator, model_inputs, dec_seq_list, weights):
    """The graded forced pass: loss = −Σ_{(t,k) not barred} w[t,k] · cum[t,k], cum the model's log-probability of the given caption
    (``Translator.score_captions``'s ``cum`` under ``unk="bar"``), differentiable in every parameter the decode-conditions pass touches.
    ``model_inputs`` as ``translate_batch`` takes them (only the video half is read, so the caller's ids and masks are left as they
    are); ``dec_seq_list`` per video (S_b, K, Lt) or (S_b, Lt) int64 / int32 extended ids, 1 ≤ K ≤ 16; ``weights`` (T, K) or (T·K,)
    floating point on the device (rounded to fp32).  ``model.train()``: dropout is on (the model's own RNG, advanced once per call);
    ``model.eval()``: deterministic.  → a namespace: ``loss`` () fp32 (the only result with a gradient), ``cum`` (T, K) fp32, ``step``
    (T, K, Lt − 1) fp32, ``barred`` (T, K) int32, ``length`` (T, K) int32.  No host synchronisation beyond the batch structure's tables."""
    def head(p):
        return loss_result(p, *ops.seq_nll(p.scores, p.cap_c, p.tgt, p.length, row_weights(weights), p.logits, UNK, max_cols=p.max_cols))
    return graded_pass(translator, model_inputs, dec_seq_list, weights, head)


class SelfCritical(PhaseEvents):
    """One self-critical training step over a ``Translator``'s model.  ``corpus`` is the ``ReferenceCorpus`` the rewards are
    scored against (its idf is CIDEr's)."""

    def __init__(self, translator, corpus):
        self.translator = translator
        self.corpus = corpus
        self._row_vid = {}
        self.phase_events = None    # tools/bench_scst.py: a list → ``step`` appends HIP events: start, sampled, greedy, rewards, graded forward

    def step(self, model_inputs, videos, num_samples=4, baseline="greedy", utility="CIDEr", seed=None, **sampling_kw):
        """``model_inputs`` as ``translate_batch`` takes them, ``videos`` the batch's videos as ``corpus.plan`` takes them → a namespace:
        ``loss`` (), ``reward`` (N, K) float64, ``baseline`` (N,) float64 greedy rewards / (N, K) leave-one-out means / None,
        ``advantage`` (N, K) float64, ``weights`` (T, K) fp32, ``cum`` (T, K) fp32, ``barred`` (T, K) int32, ``dec_seq_list`` (the
        samples, per video (S_b, K, Lt) int64), ``oov_word_dict``.  The decodes run in eval mode without gradients on copies of the ids
        and masks (they blank the text half in place); the graded pass runs in the model's current mode.  No host synchronisation."""
        tr = self.translator
        rule, col, K = ops.check_scst(num_samples=num_samples, baseline=baseline, utility=utility)
        model = tr.model
        inputs = list(model_inputs)
        self._stamp()
        with eval_mode([model]):
            dec, oov, _, _ = tr.translate_batch_sample(fresh_inputs(model, inputs), num_samples=K, seed=seed, **sampling_kw)
            self._stamp()
            greedy = tr.translate_batch_greedy(*fresh_inputs(model, inputs), model)[0] if rule == 1 else None
            self._stamp()
        plan = self.corpus.plan(list(videos))
        reward = torch.stack([tr.caption_scores(dec, plan, row=k)[:, col] for k in range(K)], 1).contiguous()
        r_g = tr.caption_scores(greedy, plan)[:, col].contiguous() if rule == 1 else None
        steps = [int(s) for s in model_inputs[11]]
        row_vid = self._row_vid.get(tuple(steps))             # (one upload per batch structure)
        if row_vid is None:
            if len(self._row_vid) > 64:
                self._row_vid.clear()
            row_vid = self._row_vid[tuple(steps)] = Idx([b for b, s in enumerate(steps) for _ in range(s)])
        adv, w = ops.scst_weights(reward, row_vid, baseline, r_g)
        self._stamp()
        r = sequence_loss(tr, inputs, dec, w)
        self._stamp()
        base = r_g if rule == 1 else (reward - adv if rule == 2 else None)
        return SimpleNamespace(loss=r.loss, reward=reward, baseline=base, advantage=adv, weights=w.view(-1, K), cum=r.cum, barred=r.barred,
                               dec_seq_list=dec, oov_word_dict=oov)
