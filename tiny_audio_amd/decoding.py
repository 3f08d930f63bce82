"""Decoding on the LM's KV cache: greedy search / sampling, beam search and candidate scoring, the ``Qwen3MI355X`` methods of the same
names.  The drivers are built of three pieces, each of which exists once -- ``PromptPass`` (the bookkeeping from the attention mask, the
inference binding, ``ta_lm_prefill``), ``ProcessorChain`` (HF's logits processors in HF's order) and ``step_loop`` (eager, capture,
replay, poll) -- and keep what is their own: state buffers, what happens to the processed logits, what is returned."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, ops
from .ops import BF16, F32, ptr, stream

I32, I64 = torch.int32, torch.int64


def check_decay_window(min_new_tokens, exponential_decay_length_penalty):
    """ValueError when the min-new-tokens window reaches behind the start of the exponential-decay length penalty."""
    if min_new_tokens > int(exponential_decay_length_penalty[0]):
        raise ValueError(f"min_new_tokens ({min_new_tokens}) > exponential_decay_length_penalty start ({exponential_decay_length_penalty[0]}): "
                         "HF forms -inf + inf = NaN on the eos scores in that window; refused")


class PromptPass:
    """What every driver derives from (``input_ids``, ``attention_mask``) [B, L]: ``ids`` int64 and ``att`` int32, contiguous;
    ``pos_full`` (HF: position_ids from the mask); ``n_valid`` [B], the valid tokens of each clip = the position of its first new
    token; ``last_rows``, the flat row of each clip's last valid prompt token.  Building it binds the LM for inference (the trainable
    base's or the adapters' current images; ``lora_img`` is the adapters' scratch image or None)."""

    def __init__(self, lm, input_ids, attention_mask):
        dev = lm.device_
        B, L = input_ids.shape
        self.lm, self.B, self.L = lm, B, L
        att = torch.ones((B, L), dtype=I32, device=dev) if attention_mask is None else attention_mask.to(device=dev, dtype=I32)
        self.att = att.contiguous()
        self.pos_full = (att.cumsum(-1) - 1).clamp(min=0).to(I32).contiguous()
        self.n_valid = att.sum(-1).to(I32).contiguous()
        idx = torch.arange(L, device=dev, dtype=I32)[None, :].expand(B, L)
        self.last_rows = (torch.arange(B, device=dev, dtype=I32) * L + (idx * att).max(dim=-1).values.to(I32)).contiguous()
        self.ids = input_ids.to(device=dev, dtype=I64).contiguous()
        self.lora_img = None
        if lm.train_base:
            lm._bind_ft()
        if lm.lora_rank:
            lm._bind_lora()
            self.lora_img = torch.empty(_lib.lib().ta_lm_lora_image_bytes(C.byref(lm._w)), dtype=torch.uint8, device=dev)

    def cache(self, rows, length):
        """an uninitialised bf16 (K, V) cache of ``rows`` rows and ``length`` slots"""
        c = self.lm.config
        shape = (c.num_hidden_layers, rows, c.num_key_value_heads, length, c.head_dim)
        return torch.empty(shape, dtype=BF16, device=self.lm.device_), torch.empty(shape, dtype=BF16, device=self.lm.device_)

    def workspace(self, decode_rows=0):
        """uint8 scratch for the prompt pass and, with ``decode_rows``, for decode steps on that many rows"""
        L_, w = _lib.lib(), C.byref(self.lm._w)
        n = L_.ta_lm_prefill_workspace_bytes(w, self.B, self.L)
        if decode_rows:
            n = max(n, L_.ta_lm_decode_workspace_bytes(w, decode_rows))
        return torch.empty(n, dtype=torch.uint8, device=self.lm.device_)

    def prefill(self, src_row, audio, kc, vc, cache_len, logits, ws):
        """``ta_lm_prefill``: the B prompts into the cache (kc, vc) of ``cache_len`` slots per row, each clip's last-row logits into
        ``logits`` [B, vocab_pad]."""
        a = None if audio is None else audio.detach().to(F32).contiguous()
        _lib.check(_lib.lib().ta_lm_prefill(C.byref(self.lm._w), ptr(self.ids), ptr(src_row), ptr(a), ptr(self.att), ptr(self.pos_full),
                                            self.B, self.L, ptr(kc), ptr(vc), cache_len, ptr(self.last_rows), ptr(logits),
                                            ptr(self.lora_img), ptr(ws), ws.numel(), stream()), "ta_lm_prefill")


class ProcessorChain:
    """HF's logits processors in HF's order (TF:generation/utils.py _get_logits_processor) on ``rows`` rows.  The constructor validates
    the options, uploads their tables and lists the launches with their arguments, which never change; calling the object on a logits
    buffer [rows, vocab_pad] only launches (no allocation, upload or sync: it runs inside the captured step).  An option that is off
    launches and allocates nothing.  The processors' context is ``prompt_ids[:, :n_ctx]`` followed by the ``*step_dev`` tokens of
    ``history`` [rows, max_new]; ``n_ctx`` = 0 is what HF's processors see when generate() is given inputs_embeds WITHOUT input_ids
    (the reference's generate_streaming, tiny_audio/asr_modeling.py:723-729): the generated tokens only."""

    def __init__(self, lm, rows, prompt_ids, n_ctx, history, max_new, step_dev, eos, n_eos, repetition_penalty=1.0,
                 no_repeat_ngram_size=0, min_new_tokens=0, sequence_bias=None, bad_words=None, forced_eos_ids=None,
                 exponential_decay_length_penalty=None, suppress_tokens=None, begin_suppress_tokens=None):
        self.lib, self.vp, self.V, dev = _lib.lib(), lm.vocab_pad, lm.config.vocab_size, lm.device_
        V, step = self.V, ptr(step_dev)
        rep, ngram, min_new = float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens or 0)
        context = (ptr(prompt_ids), n_ctx, ptr(history), max_new, step, rows)
        self.launches = []                          # (entry point, its arguments between (logits, vocab_pad, V) and the stream)
        self.keep = [prompt_ids, history, step_dev, eos]            # the tensors those arguments point into
        add = lambda name, *args: self.launches.append((name, args))  # noqa: E731

        def add_bias(entries, what):
            tab = ops.build_sequence_table(entries or [], V, dev, what)
            if tab is not None:
                self.keep.append(tab)
                add("ta_logits_sequence_bias", *context, ptr(tab["tokens"]), ptr(tab["offsets"]), ptr(tab["bias"]), ptr(tab["groups"]),
                    tab["n_seq"], tab["n_groups"], tab["n_tokens"])

        add_bias(sequence_bias, "sequence_bias")    # HF SequenceBiasLogitsProcessor: first of all, so the repetition penalty sees it
        if rep != 1.0 or ngram > 0:                 # HF repetition penalty and no-repeat-ngram
            add("ta_logits_process", *context, rep, ngram)
        add_bias(bad_words, "bad_words_ids")        # HF NoBadWordsLogitsProcessor: the same kernel, every bias -inf
        if min_new > 0 and n_eos:                   # HF MinNewTokensLengthLogitsProcessor: no eos before min_new_tokens tokens exist
            add("ta_logits_suppress_until", ptr(eos), n_eos, min_new, step, rows)
        ids_of = lambda v, what: torch.tensor(ops.id_list(v, V, what), dtype=I64, device=dev) if v else None  # noqa: E731
        forced, sup = ids_of(forced_eos_ids, "forced_eos_token_id"), ids_of(suppress_tokens, "suppress_tokens")
        bsup = ids_of(begin_suppress_tokens, "begin_suppress_tokens")
        decay_start, decay_mult = 0, None
        if exponential_decay_length_penalty is not None and n_eos:
            check_decay_window(min_new, exponential_decay_length_penalty)
            decay_start, decay_mult = ops.decay_multipliers(exponential_decay_length_penalty, max_new)
            decay_mult = decay_mult.to(dev)
        n_of = lambda t: 0 if t is None else t.numel()  # noqa: E731
        if any(t is not None for t in (forced, decay_mult, sup, bsup)):      # HF forced eos, exponential decay, suppress, begin-suppress: one launch
            self.keep += [forced, decay_mult, sup, bsup]
            add("ta_logits_step_rules", rows, step, max_new, ptr(forced), n_of(forced), ptr(eos), n_eos if decay_mult is not None else 0,
                decay_start, ptr(decay_mult), ptr(sup), n_of(sup), ptr(bsup), n_of(bsup))

    def __call__(self, logits):
        for name, args in self.launches:
            _lib.check(getattr(self.lib, name)(ptr(logits), self.vp, self.V, *args, stream()), name)


def step_loop(step, max_new, alive, sync_every, poll_every_step, use_graph, dev):
    """Run ``step()`` for t = 1 .. max_new - 1 (step 0 is the prompt pass's) and yield t after each.  Before step t the host reads the
    device counter ``alive`` if ``poll_every_step`` or t % sync_every == 0, and stops at 0.  A decode step is ~340 tiny launches whose
    arguments never change (all per-step state is device-resident): the first runs eagerly, the second is captured into a hipGraph,
    which is replayed for it and the rest (``use_graph=False``, a CPU device, the dry run or max_new <= 3: eager steps)."""
    graph = None
    want_graph = use_graph and dev.type == "cuda" and not _lib.DRY_RUN and max_new > 3
    for t in range(1, max_new):
        if (poll_every_step or t % sync_every == 0) and int(alive.item()) == 0:
            return
        if graph is not None:
            graph.replay()
        elif want_graph and t == 2:
            torch.cuda.synchronize()
            graph = step.graph = torch.cuda.CUDAGraph()      # owned by the driver's ``step``: it outlives this loop, as the replays in flight do
            with torch.cuda.graph(graph):
                step()
            graph.replay()                          # capture records, it does not run
        else:
            step()
        yield t


# ---------------------------------------------------------------------- greedy search and sampling
@torch.no_grad()
def greedy_decode(lm, input_ids, src_row, audio, attention_mask=None, max_new_tokens=128, eos_ids=(), pad_id=0, sync_every=8,
                  use_graph=True, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, sampling=None, token_scores=False,
                  top_logprobs=0, **decode_options):
    """-> int64 [B, n_new], or with ``token_scores`` / ``top_logprobs`` the pair (that tensor, the scores dict); see
    ``greedy_decode_iter`` (this drains it, polling the device every ``sync_every`` steps only).  ``decode_options``: its
    decoding-option keywords (``sequence_bias`` ... ``warp_ext``)."""
    out = None
    for out in lm.greedy_decode_iter(input_ids, src_row, audio, attention_mask, max_new_tokens, eos_ids, pad_id, sync_every, use_graph,
                                     per_token=False, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                     min_new_tokens=min_new_tokens, sampling=sampling, token_scores=token_scores,
                                     top_logprobs=top_logprobs, **decode_options):
        pass
    return out


def greedy_decode_iter(lm, input_ids, src_row, audio, attention_mask=None, max_new_tokens=128, eos_ids=(), pad_id=0,
                       sync_every=8, use_graph=True, per_token=True, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0,
                       processors_see_prompt=True, sampling=None, token_scores=False, top_logprobs=0, sequence_bias=None,
                       bad_words=None, forced_eos_ids=None, exponential_decay_length_penalty=None, suppress_tokens=None,
                       begin_suppress_tokens=None, warp_ext=None):
    """HF greedy search with a KV cache (what ``language_model.generate`` does for the reference's generation
    config, tiny_audio/asr_config.py:103-111): prompt pass, then one token per clip per step until every clip has
    emitted an eos id or ``max_new_tokens`` is reached.  -> int64 [B, n_new] (prompt stripped; finished clips are
    padded with ``pad_id``).  All per-step state lives on the device; the host only polls the number of
    unfinished clips every ``sync_every`` steps.

    A generator: with ``per_token`` it yields the int64 [B] host tensor of every step's tokens as soon as that step
    has run (one device sync per token: the streaming mode of tiny_audio/asr_modeling.py:648-760) and stops when
    every clip is finished; the last item yielded is always the full [B, n_new] device tensor.

    Decoding scores (``token_scores`` and / or ``top_logprobs`` = k in [1, 8]; off by default, and then nothing below is launched or
    allocated): every step also runs ``ta_token_scores_f32`` on its PROCESSED logits (after the processors and warpers), between the
    selection and the bookkeeping, also inside the captured step.  The last item is then ``(sequences, scores)`` with scores =
    {``token_logprobs`` f32 [B, n_new], ``token_entropy`` f32 [B, n_new], ``top_token_ids`` int64 [B, n_new, k] or None,
    ``top_logprobs`` f32 [B, n_new, k] or None} (positions after a clip's eos: 0 / 0 / -1 / -inf), and with ``per_token`` every
    step yields ``(tokens [B], logprob [B])`` host tensors.

    Decoding options (all off by default, and then nothing below is launched or allocated), HF's processors in HF's order
    (``ProcessorChain``), device-side and inside the captured step; their tables are uploaded before the
    prompt pass.  ``sequence_bias`` / ``bad_words``: [(tuple of ids, bias)] in HF's order (``ops.normalize_sequence_bias`` /
    ``ops.normalize_bad_words``) -> ``ta_logits_sequence_bias`` before / after ``ta_logits_process``; their context is the prompt
    plus the generated tokens, or the generated tokens alone with ``processors_see_prompt=False``.  ``forced_eos_ids``,
    ``exponential_decay_length_penalty`` = (start, factor) (acts on ``eos_ids``), ``suppress_tokens``, ``begin_suppress_tokens`` ->
    one ``ta_logits_step_rules`` after the min-new-tokens rule.  ``warp_ext`` = (min_p, typical_p, epsilon_cutoff, eta_cutoff) with
    the off values (0, 1, 0, 0) -> ``ta_logits_warp_ext`` after ``ta_logits_warp``; it acts under ``sampling`` only, as HF's
    warpers do.  All run before the scores kernel: scores and alternatives are those of the fully processed row."""
    n_top = int(top_logprobs or 0)
    if not 0 <= n_top <= ops.MAX_TOP_LOGPROBS:
        raise ValueError(f"top_logprobs must be within [0, {ops.MAX_TOP_LOGPROBS}]; got {top_logprobs}")
    want_scores = bool(token_scores) or n_top > 0
    if lm._w is None:
        raise _lib.Ta355Error("LM weights not loaded")
    L_ = _lib.lib()
    dev, V, vp = lm.device_, lm.config.vocab_size, lm.vocab_pad
    B, L = input_ids.shape
    max_new = int(max_new_tokens)
    if max_new <= 0:
        seq = torch.empty((B, 0), dtype=I64, device=dev)
        e = torch.empty((B, 0), dtype=F32, device=dev)
        yield (seq, dict(token_logprobs=e, token_entropy=e.clone(),
                         top_token_ids=torch.empty((B, 0, n_top), dtype=I64, device=dev) if n_top else None,
                         top_logprobs=torch.empty((B, 0, n_top), dtype=F32, device=dev) if n_top else None)) if want_scores else seq
        return
    Lmax = L + max_new
    if Lmax > lm.config.max_position_embeddings:
        raise ValueError(f"prompt ({L}) + max_new_tokens ({max_new}) exceeds max_position_embeddings")
    pp = PromptPass(lm, input_ids, attention_mask)
    kmask = torch.zeros((B, Lmax), dtype=I32, device=dev)
    kmask[:, :L] = pp.att
    pos = pp.n_valid.clone()                        # position of the next token: ta_greedy_advance moves it on
    kc, vc = pp.cache(B, Lmax)
    ws = pp.workspace(decode_rows=B)
    logits = torch.empty((B, vp), dtype=F32, device=dev)
    amax, next_ids = torch.zeros(B, dtype=I64, device=dev), torch.zeros(B, dtype=I64, device=dev)
    finished = torch.zeros(B, dtype=I32, device=dev)
    out_seq = torch.full((B, max_new), int(pad_id), dtype=I64, device=dev)
    step_dev = torch.zeros(1, dtype=I32, device=dev)
    slot_dev = torch.full((1,), L, dtype=I32, device=dev)
    alive = torch.full((1,), B, dtype=I32, device=dev)
    eos = torch.tensor(list(eos_ids) or [-1], dtype=I64, device=dev)
    n_eos = len(list(eos_ids))
    sc_lp = sc_ent = sc_ids = sc_top = None
    if want_scores:                                 # one column per step, written on the device at *step_dev; never the [B, V] rows
        sc_lp, sc_ent = torch.zeros((B, max_new), dtype=F32, device=dev), torch.zeros((B, max_new), dtype=F32, device=dev)
        if n_top:
            sc_ids = torch.full((B, max_new, n_top), -1, dtype=I64, device=dev)
            sc_top = torch.full((B, max_new, n_top), float("-inf"), dtype=F32, device=dev)
    process = ProcessorChain(lm, B, pp.ids, L if processors_see_prompt else 0, out_seq, max_new, step_dev, eos, n_eos,
                             repetition_penalty, no_repeat_ngram_size, min_new_tokens, sequence_bias, bad_words, forced_eos_ids,
                             exponential_decay_length_penalty, suppress_tokens, begin_suppress_tokens)
    wx = None
    if warp_ext is not None and sampling is not None and tuple(float(x) for x in warp_ext) != (0.0, 1.0, 0.0, 0.0):
        wx = tuple(float(x) for x in warp_ext)

    def advance():
        process(logits)
        if sampling is not None:                    # do_sample: HF's warpers (temperature, top-k, top-p), then one multinomial draw per clip
            temp, top_k, top_p, seed = sampling
            _lib.check(L_.ta_logits_warp(ptr(logits), vp, V, B, float(temp), int(top_k), float(top_p), stream()), "ta_logits_warp")
            if wx is not None:                      # HF min-p, typical, epsilon, eta warpers
                _lib.check(L_.ta_logits_warp_ext(ptr(logits), vp, V, B, *wx, stream()), "ta_logits_warp_ext")
            _lib.check(L_.ta_sample_f32(ptr(logits), vp, V, B, int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(step_dev), ptr(amax), stream()),
                       "ta_sample_f32")
        else:
            _lib.check(L_.ta_argmax_f32(ptr(logits), vp, V, B, ptr(amax), stream()), "ta_argmax_f32")
        if want_scores:                             # before the bookkeeping: it reads *step_dev and `finished` as they stand for THIS step
            _lib.check(L_.ta_token_scores_f32(ptr(logits), vp, V, B, ptr(amax), ptr(finished), ptr(step_dev), max_new, n_top, ptr(sc_lp),
                                              ptr(sc_ent), ptr(sc_ids), ptr(sc_top), stream()), "ta_token_scores_f32")
        _lib.check(L_.ta_greedy_advance(ptr(amax), ptr(eos), n_eos, int(pad_id), ptr(finished), ptr(next_ids), ptr(out_seq), max_new,
                                        ptr(step_dev), ptr(slot_dev), ptr(pos), ptr(kmask), Lmax, B, ptr(alive), stream()),
                   "ta_greedy_advance")

    def step():                                     # step_loop hangs the captured graph on it (``step.graph``): it lives as long as this driver
        _lib.check(L_.ta_lm_decode_step(C.byref(lm._w), ptr(next_ids), ptr(pos), ptr(kmask), ptr(slot_dev), B, ptr(kc), ptr(vc), Lmax,
                                        ptr(logits), ptr(pp.lora_img), ptr(ws), ws.numel(), stream()), "ta_lm_decode_step")
        advance()

    item = lambda t: (out_seq[:, t].cpu(), sc_lp[:, t].cpu()) if want_scores else out_seq[:, t].cpu()  # noqa: E731
    pp.prefill(src_row, audio, kc, vc, Lmax, logits, ws)
    advance()
    if per_token:
        yield item(0)
    for t in step_loop(step, max_new, alive, sync_every, per_token, use_graph, dev):
        if per_token:
            yield item(t)
    seq = out_seq.cpu()
    # HF stops right after the step in which the last clip finished: trim the surplus (all-pad) columns
    n_new = max_new
    if n_eos:
        is_eos = torch.isin(seq, torch.tensor(list(eos_ids), dtype=I64))
        first = torch.where(is_eos.any(-1), is_eos.to(torch.int8).argmax(-1) + 1, torch.full((B,), max_new + 1))
        n_new = min(max_new, int(first.max()))
    if want_scores:
        yield out_seq[:, :n_new], dict(token_logprobs=sc_lp[:, :n_new], token_entropy=sc_ent[:, :n_new],
                                       top_token_ids=sc_ids[:, :n_new] if n_top else None,
                                       top_logprobs=sc_top[:, :n_new] if n_top else None)
        return
    yield out_seq[:, :n_new]


# ---------------------------------------------------------------------- beam search (csrc/beam.hip)
@torch.no_grad()
def beam_decode(lm, input_ids, src_row, audio, attention_mask=None, max_new_tokens=128, eos_ids=(), pad_id=0, num_beams=1,
                length_penalty=1.0, early_stopping=False, num_return_sequences=1, sync_every=8, use_graph=True,
                repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, sequence_bias=None, bad_words=None,
                forced_eos_ids=None, exponential_decay_length_penalty=None, suppress_tokens=None, begin_suppress_tokens=None,
                return_trace=False):
    """HF beam search (``GenerationMixin._beam_search``, do_sample False) with beams as rows: the prompt pass runs once on the B
    clips, ``ta_kv_beam_expand`` copies every clip's cache rows to its K = ``num_beams`` rows, and every step is the unchanged
    ``ta_lm_decode_step`` on R = B * K rows followed by ``ta_beam_logprobs_f32``, the greedy loop's logits processors on the
    log-probabilities (context: the replicated prompt ids and the running sequences), ``ta_beam_topk_f32``, ``ta_beam_advance`` and
    ``ta_kv_beam_reorder``.  As in the greedy loop all per-step state is device memory: the first step runs eagerly, the second is
    captured into a hipGraph and replayed, and the host polls the number of clips that are not done every ``sync_every`` steps.

    -> (sequences int64 [B * num_return_sequences, n_new], sequences_scores f32 [B * num_return_sequences]): the best finished
    sequences of every clip in descending score order, padded with ``pad_id``, cropped to the longest.  ``early_stopping``: False,
    True or "never", HF's three heuristics.  With ``return_trace`` a third item, a dict: per executed step ``cand_score`` /
    ``cand_flat`` [steps, B, M], ``running_sequences`` [steps, B, K, max_new] and ``running_scores`` [steps, B, K] as they stood
    BEFORE the step, ``parent`` [steps, B, K]; and the final ``pool`` (sequences, scores, lengths, finished), the final running
    state and the R-row ``cache``.  The trace buffers are written by ``ta_beam_advance`` at ``*step_dev``; without the switch
    nothing extra is allocated or launched."""
    if lm._w is None:
        raise _lib.Ta355Error("LM weights not loaded")
    L_ = _lib.lib()
    c, dev = lm.config, lm.device_
    B, L = input_ids.shape
    K, max_new, eos_ids = int(num_beams), int(max_new_tokens), [int(e) for e in eos_ids]
    n_eos, nrs = len(eos_ids), int(num_return_sequences)
    if not 1 <= K <= ops.MAX_BEAMS:
        raise ValueError(f"num_beams must be within [1, {ops.MAX_BEAMS}]; got {num_beams}")
    if n_eos > ops.MAX_BEAM_EOS:
        raise ValueError(f"beam search takes at most {ops.MAX_BEAM_EOS} eos ids (max(2, 1 + n_eos) * num_beams candidates, "
                         f"{ops.MAX_BEAM_CANDIDATES} at the most); got {n_eos}")
    if not 1 <= nrs <= K:
        raise ValueError(f"num_return_sequences ({nrs}) has to be within [1, num_beams = {K}]")
    if early_stopping not in (False, True, "never"):
        raise ValueError(f"early_stopping must be False, True or 'never'; got {early_stopping!r}")
    es = 2 if early_stopping == "never" else int(bool(early_stopping))
    lp = float(length_penalty)
    if max_new <= 0:
        out = torch.empty((B * nrs, 0), dtype=I64, device=dev), torch.full((B * nrs,), -1.0e9, dtype=F32, device=dev)
        return (*out, {}) if return_trace else out
    Lmax = L + max_new
    if Lmax > c.max_position_embeddings:
        raise ValueError(f"prompt ({L}) + max_new_tokens ({max_new}) exceeds max_position_embeddings")
    if K * max_new > 12288:
        raise ValueError(f"num_beams * max_new_tokens = {K * max_new} exceeds 12288 (the running sequences are staged in LDS)")
    M, R, V, vp = max(2, 1 + n_eos) * K, B * K, c.vocab_size, lm.vocab_pad
    pp = PromptPass(lm, input_ids, attention_mask)
    # per row: every beam of a clip starts from the clip's prompt (HF _expand_inputs_for_generation)
    kmask = torch.zeros((R, Lmax), dtype=I32, device=dev)
    kmask[:, :L] = pp.att.repeat_interleave(K, 0)
    pos = pp.n_valid.repeat_interleave(K).contiguous()
    ids_r = pp.ids.repeat_interleave(K, 0).contiguous()
    nl, hkv, hd = c.num_hidden_layers, c.num_key_value_heads, c.head_dim
    kc0, vc0 = pp.cache(B, L)                       # the prompt pass's B-row staging cache
    kc, vc = pp.cache(R, Lmax)
    ws = pp.workspace(decode_rows=R)
    tk_ws = torch.empty(max(L_.ta_beam_topk_workspace_bytes(B, K, V, M), 8), dtype=torch.uint8, device=dev)
    logits = torch.empty((R, vp), dtype=F32, device=dev)
    pre_logits = torch.empty((B, vp), dtype=F32, device=dev)
    run_seq = torch.full((R, max_new), int(pad_id), dtype=I64, device=dev)
    run_score = torch.tensor([0.0] + [-1.0e9] * (K - 1), dtype=F32, device=dev).repeat(B).contiguous()      # HF: only beam 0 is live at first
    parent, next_ids = torch.zeros(R, dtype=I32, device=dev), torch.zeros(R, dtype=I64, device=dev)
    pool_seq = torch.full((B, K, max_new), int(pad_id), dtype=I64, device=dev)
    pool_score = torch.full((B, K), -1.0e9, dtype=F32, device=dev)
    pool_len, pool_fin = torch.zeros((B, K), dtype=I32, device=dev), torch.zeros((B, K), dtype=I32, device=dev)
    heur, clip_done = torch.ones(B, dtype=I32, device=dev), torch.zeros(B, dtype=I32, device=dev)
    cand_score, cand_flat = torch.empty((B, M), dtype=F32, device=dev), torch.empty((B, M), dtype=I32, device=dev)
    step_dev = torch.zeros(1, dtype=I32, device=dev)
    slot_dev = torch.full((1,), L, dtype=I32, device=dev)
    alive = torch.full((1,), B, dtype=I32, device=dev)
    eos = torch.tensor(eos_ids or [-1], dtype=I64, device=dev)
    len_div = ops.beam_length_divisors(lp, max_new).to(dev)
    tr = None
    if return_trace:
        tr = dict(cand_score=torch.zeros((max_new, B, M), dtype=F32, device=dev), cand_flat=torch.zeros((max_new, B, M), dtype=I32, device=dev),
                  run_seq=torch.full((max_new, R, max_new), int(pad_id), dtype=I64, device=dev),
                  run_score=torch.zeros((max_new, R), dtype=F32, device=dev), parent=torch.zeros((max_new, R), dtype=I32, device=dev))
    tp = lambda k: None if tr is None else ptr(tr[k])  # noqa: E731
    # the logits processors of the greedy loop, on R rows of log-probabilities (HF runs them behind log_softmax)
    process = ProcessorChain(lm, R, ids_r, L, run_seq, max_new, step_dev, eos, n_eos, repetition_penalty, no_repeat_ngram_size,
                             min_new_tokens, sequence_bias, bad_words, forced_eos_ids, exponential_decay_length_penalty, suppress_tokens,
                             begin_suppress_tokens)

    def select():
        _lib.check(L_.ta_beam_logprobs_f32(ptr(logits), vp, V, R, stream()), "ta_beam_logprobs_f32")
        process(logits)
        _lib.check(L_.ta_beam_topk_f32(ptr(logits), vp, V, ptr(run_score), B, K, M, ptr(cand_score), ptr(cand_flat), ptr(tk_ws),
                                       tk_ws.numel(), stream()), "ta_beam_topk_f32")
        _lib.check(L_.ta_beam_advance(ptr(cand_score), ptr(cand_flat), B, K, M, V, ptr(eos), n_eos, int(pad_id), max_new, ptr(len_div),
                                      es, int(es == 2 and lp > 0.0), ptr(run_seq), ptr(run_score), ptr(parent), ptr(next_ids),
                                      ptr(pool_seq), ptr(pool_score), ptr(pool_len), ptr(pool_fin), ptr(heur), ptr(clip_done),
                                      ptr(step_dev), ptr(slot_dev), ptr(pos), ptr(kmask), Lmax, ptr(alive), tp("cand_score"),
                                      tp("cand_flat"), tp("run_seq"), tp("run_score"), tp("parent"), stream()), "ta_beam_advance")
        if K > 1:
            _lib.check(L_.ta_kv_beam_reorder(ptr(kc), ptr(vc), nl, B, K, hkv, L, Lmax, hd, max_new, ptr(parent), ptr(slot_dev),
                                             stream()), "ta_kv_beam_reorder")

    def step():                                     # step_loop hangs the captured graph on it (``step.graph``): it lives as long as this driver
        _lib.check(L_.ta_lm_decode_step(C.byref(lm._w), ptr(next_ids), ptr(pos), ptr(kmask), ptr(slot_dev), R, ptr(kc), ptr(vc), Lmax,
                                        ptr(logits), ptr(pp.lora_img), ptr(ws), ws.numel(), stream()), "ta_lm_decode_step")
        select()

    pp.prefill(src_row, audio, kc0, vc0, L, pre_logits, ws)
    _lib.check(L_.ta_kv_beam_expand(ptr(kc0), ptr(vc0), ptr(kc), ptr(vc), nl, B, K, hkv, L, L, Lmax, hd, stream()), "ta_kv_beam_expand")
    logits.view(B, K, vp).copy_(pre_logits[:, None, :])             # the prompt's logits row feeds the clip's K rows (all but beam 0 carry -1e9)
    del kc0, vc0
    select()
    n_steps = 1 + sum(1 for _ in step_loop(step, max_new, alive, sync_every, False, use_graph, dev))
    lens = pool_len[:, :nrs]
    n_new = int(lens.max().item()) if lens.numel() else 0
    seqs = pool_seq[:, :nrs, :n_new].reshape(B * nrs, n_new).contiguous()
    scores = pool_score[:, :nrs].reshape(B * nrs).contiguous()
    if not return_trace:
        return seqs, scores
    trace = dict(n_steps=n_steps, cand_score=tr["cand_score"][:n_steps], cand_flat=tr["cand_flat"][:n_steps],
                 running_sequences=tr["run_seq"][:n_steps].reshape(n_steps, B, K, max_new),
                 running_scores=tr["run_score"][:n_steps].reshape(n_steps, B, K), parent=tr["parent"][:n_steps].reshape(n_steps, B, K),
                 pool=dict(sequences=pool_seq, scores=pool_score, lengths=pool_len, finished=pool_fin),
                 final_running_sequences=run_seq.reshape(B, K, max_new), final_running_scores=run_score.reshape(B, K),
                 heuristic_unsatisfied=heur, clip_done=clip_done, cache=(kc, vc), prompt_len=L, n_candidates=M)
    return seqs, scores, trace


# ---------------------------------------------------------------------- candidate scoring (include/ta355.h ta_lm_score)
@torch.no_grad()
def score_candidates(lm, input_ids, src_row, audio, attention_mask, token_ids, n_tokens, candidate_clip, chunks=None):
    """Log-probability of given continuations of the prompts: the prompt pass runs ONCE over the B clips (as in ``greedy_decode``),
    then ``ta_lm_score`` appends every candidate's tokens to the cache of its clip.  ``token_ids`` int64 [R, T] (entries behind a
    row's end are ignored), ``n_tokens`` [R] (each within [1, T]), ``candidate_clip`` [R] (within [0, B)): the table of
    ``scoring.build_candidate_table``; ``chunks``: its row ranges (default: ``scoring.chunk_rows`` under the C limits), one
    ``ta_lm_score`` call each.  -> (token_logprobs f32 [R, T], exact 0 behind a row's end; scores f32 [R]) on the device.  Raw logits:
    no processor, no temperature; candidate token t sits at RoPE position (valid prompt tokens of its clip) + t."""
    from . import scoring
    if lm._w is None:
        raise _lib.Ta355Error("LM weights not loaded")
    L_ = _lib.lib()
    dev = lm.device_
    B, L = input_ids.shape
    token_ids = torch.as_tensor(token_ids, dtype=I64)
    n_host = [int(v) for v in torch.as_tensor(n_tokens).tolist()]
    clip_host = [int(v) for v in torch.as_tensor(candidate_clip).tolist()]
    R, T = token_ids.shape
    if len(n_host) != R or len(clip_host) != R:
        raise ValueError(f"n_tokens / candidate_clip must have one entry per row of token_ids ({R})")
    if any(not 1 <= n <= T for n in n_host) or any(not 0 <= b < B for b in clip_host):
        raise ValueError("n_tokens must lie within [1, T] and candidate_clip within [0, B)")
    if L + T > lm.config.max_position_embeddings:
        raise ValueError(f"prompt ({L}) + candidate tokens ({T}) exceeds max_position_embeddings")
    token_lp = torch.zeros((R, T), dtype=F32, device=dev)
    scores = torch.zeros(R, dtype=F32, device=dev)
    if R == 0:
        return token_lp, scores
    if chunks is None:
        chunks = scoring.chunk_rows(n_host, *scoring.limits())
    pp = PromptPass(lm, input_ids, attention_mask)
    kc, vc = pp.cache(B, L)                         # Lmax = L: nothing is appended to the cache
    logits = torch.empty((B, lm.vocab_pad), dtype=F32, device=dev)
    pp.prefill(src_row, audio, kc, vc, L, logits, pp.workspace())
    for r0, r1 in chunks:
        n, Tc = r1 - r0, max(n_host[r0:r1])
        need = L_.ta_lm_score_workspace_bytes(C.byref(lm._w), B, n, Tc)
        if need < 0:
            raise ValueError(f"{n} rows x {Tc} tokens is outside one scoring call's limits {scoring.limits()}")
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        cid = token_ids[r0:r1, :Tc].to(device=dev).contiguous()
        lens = torch.tensor(n_host[r0:r1], dtype=I32, device=dev)
        lens_host = (C.c_int * n)(*n_host[r0:r1])
        clip = torch.tensor(clip_host[r0:r1], dtype=I32, device=dev)
        lp = torch.empty((n, Tc), dtype=F32, device=dev)
        _lib.check(L_.ta_lm_score(C.byref(lm._w), ptr(cid), ptr(lens), lens_host, ptr(clip), ptr(pp.n_valid), B, n, Tc, ptr(kc), ptr(vc), L,
                                  ptr(pp.att), ptr(logits), ptr(pp.lora_img), ptr(lp), ptr(scores[r0:r1]), ptr(ws), ws.numel(),
                                  stream()), "ta_lm_score")
        token_lp[r0:r1, :Tc] = lp
    return token_lp, scores
