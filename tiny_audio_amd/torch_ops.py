"""``torch.ops.ta355.*``: the composites of libta355.so registered as PyTorch custom operators (torch.library).

north_star: "exposed as PyTorch-ROCm custom ops so ASRModel/ASRProcessor and scripts/train.py stay drop-in".  The
reference has no FFI; its seams are nn.Module boundaries, and each operator below sits on one:

    ta355::logmel              WhisperFeatureExtractor.__call__           scripts/train.py:327-333
    ta355::wave_augment        RIRAugmentation / NoiseAugmentation.__call__   tiny_audio/augmentation.py:71-223
    ta355::wave_augment_chain  the same seam, every member of the production chain   tiny_audio/augmentation.py:153-216
    ta355::ctc_align           ForcedAligner._get_trellis / ._backtrack   tiny_audio/alignment.py:47-152
    ta355::ctc_align_long      the same, for a whole recording against its whole transcript   tiny_audio/asr_pipeline.py:117-131
    ta355::text_align          jiwer.wer's edit distance and align_words_to_reference's LCS table
                               scripts/eval/evaluators/base.py:114,150, scripts/eval/evaluators/alignment.py:12-79
    ta355::wave_cut_cost, cut_plan, wave_windows   long-form transcription: where to cut a recording and the cut itself; the reference
                               keeps the first chunk only   tiny_audio/asr_pipeline.py:243-245
    ta355::vad                 TenVad.process, one 256-sample frame per call (a statistical detector of this project's own, not that
                               model)   tiny_audio/diarization.py:370-387
    ta355::spk_vote, spk_merge, spk_words   LocalSpeakerDiarizer._resample_vad / _postprocess_segments / _merge_short_segments /
                               assign_speakers_to_words, the host loops behind the cluster labels   tiny_audio/diarization.py:520-682
    ta355::wav2vec2_emissions  torchaudio WAV2VEC2_ASR_BASE_960H forward + log_softmax   tiny_audio/alignment.py:206-211
    ta355::wav2vec2_sln_emissions  the same seam with a layer-norm / stable wav2vec2 (large-lv60, XLSR-53, XLS-R 300M, MMS 300M), which
                               the reference's align(..., _language=...) placeholder stands for   tiny_audio/alignment.py:182-211
    ta355::ecapa_embeddings    SpeechBrain ECAPA-TDNN encode_batch, one call per window   tiny_audio/diarization.py:457-517
    ta355::spk_affinity        SpectralCluster.get_sim_mat / p_pruning / get_laplacian   tiny_audio/diarization.py:49-89
    ta355::spk_laplacian_matmul, spk_panel_gram / _update / _combine   the products scipy.linalg.eigh is replaced by
                               (block Lanczos, tiny_audio_amd/spectral.py)   tiny_audio/diarization.py:91-106
    ta355::token_scores        compute_transition_scores on one step's processed logits (TF:generation/utils.py); the reference
                               asks HF for no scores (tiny_audio/asr_modeling.py:631-637)
    ta355::logits_sequence_bias, logits_step_rules, logits_warp_ext   HF's remaining single-hypothesis logits processors, which the
                               reference reaches through **generate_kwargs (tiny_audio/asr_modeling.py:625-637); in place
    ta355::beam_logprobs, beam_topk, beam_advance, kv_beam_expand, kv_beam_reorder   one iteration of HF's _beam_search
                               (TF:generation/utils.py), which the reference reaches with num_beams > 1 (tiny_audio/asr_config.py:42)
    ta355::encoder_forward     model.audio_tower(input_features=...)      tiny_audio/asr_modeling.py:448-450
    ta355::encoder_forward_ragged   the same seam, every clip at its own length (opt-in; what the reference computes for a
                               clip encoded alone, tiny_audio/asr_modeling.py:198-200)
    ta355::whisper_encoder_forward  the same seam with a Whisper tower    tiny_audio/asr_modeling.py:203-237
    ta355::mlp_projector       MLPAudioProjector.forward   (+ autograd)   tiny_audio/projectors.py:57-71
    ta355::moe_projector       MoEAudioProjector.forward   (+ autograd)   tiny_audio/projectors.py:257-347
    ta355::lm_forward_loss     embed + masked_scatter + Qwen3ForCausalLM(labels=...)  (+ autograd: d audio rows, LoRA
                               adapters or the LM's own weights)          tiny_audio/asr_modeling.py:497-526

Operators take tensors and plain scalars only.  The frozen models' packed bf16 weight images live in the Python module
that owns them (they are derived state, rebuilt when a master changes), so every operator carries an integer ``handle``
naming that module (``register_module``); trainable parameters are passed as tensors so that autograd sees them.  Saved
state for backward (the kernels' tapes) is returned as extra outputs, as torch.library requires.  Each forward has a
``*_backward`` operator of its own, registered with ``register_autograd``; fake (meta) implementations give the output
shapes so that the operators trace.

There is no CPU implementation: the implementations call the C ABI, which raises without a GPU (the dry-run marshalling
mode of ``_lib`` used by the CPU test-suite aside).
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib
from .ops import BF16, F32, ptr, stream

_MODULES: "weakref.WeakValueDictionary[int, object]" = weakref.WeakValueDictionary()
_NEXT = [1]


def register_module(mod) -> int:
    """-> integer handle of a weight-owning module (feature extractor, encoder, projector, LM); idempotent.
    A handle names ONE object: ``copy.deepcopy`` / pickling duplicate the ``_ta355_handle`` attribute with the rest of
    ``__dict__``, so a module that arrives with a handle somebody else holds (an EMA or reference copy of a model) is given a
    fresh one instead of rebinding the original's -- a later backward of the original would otherwise resolve its handle to
    the copy's packed weights."""
    h = mod.__dict__.get("_ta355_handle")
    owner = _MODULES.get(h) if h is not None else None
    if h is None or (owner is not None and owner is not mod):
        h = _NEXT[0]
        _NEXT[0] += 1
        object.__setattr__(mod, "_ta355_handle", h)
    _MODULES[h] = mod
    return h


def module_of(handle: int):
    mod = _MODULES.get(int(handle))
    if mod is None:
        raise _lib.Ta355Error(f"ta355 operator called with a stale module handle ({handle})")
    return mod


def _empty(dev):
    return torch.empty(0, device=dev)


def _is_bf16_image(x) -> bool:
    return x.dtype == BF16 and x.is_contiguous()


def _bf16_image(x):
    """-> (the bf16 tensor the kernels read, what the operator returns as its "bf16 image of x" output).  An operator's outputs
    must not alias its inputs: when x already IS a contiguous bf16 tensor (the frozen encoder's output) the output is an empty
    placeholder and the autograd formula saves the INPUT instead -- no copy of [B, S, E] per step (41 MB at B = 32)."""
    xd = x.detach()
    if _is_bf16_image(xd):
        return xd, torch.empty(0, device=x.device, dtype=BF16)
    xb = xd.to(BF16).contiguous()
    return xb, xb


# ============================================================================ log-mel
@torch.library.custom_op("ta355::logmel", mutates_args=())
def logmel(wav: Tensor, lens: Tensor, handle: int) -> Tuple[Tensor, Tensor]:
    """wav f32 [B, Ls] (zero padded), lens i64 [B] -> (features f32 [B, n_mels, Ls // 160], frame mask i32 [B, Ls // 160])."""
    return module_of(handle)._extract(wav, lens)


@logmel.register_fake
def _(wav, lens, handle):
    B, Ls = wav.shape
    n = module_of(handle).feature_size
    return wav.new_empty((B, n, Ls // 160)), wav.new_empty((B, Ls // 160), dtype=torch.int32)


# ============================================================================ waveform augmentation
@torch.library.custom_op("ta355::wave_augment", mutates_args=())
def wave_augment(wav: Tensor, lens: Tensor, desc: Tensor, stages: int, seed: int, offset: int, handle: int) -> Tensor:
    """wav f32 [B, Ls] (zero padded), lens i64 [B], desc u8: the packed per-clip descriptor (``WaveAugmentPlan.pack``) -> the augmented
    f32 [B, Ls].  ``stages``: bit mask of the stages some clip uses; (seed, offset): the Philox triple of the Gaussian floor.  No
    autograd: the waveform is data."""
    return module_of(handle)._apply(wav, lens, desc, stages, seed, offset)


@wave_augment.register_fake
def _(wav, lens, desc, stages, seed, offset, handle):
    return torch.empty_like(wav)


@torch.library.custom_op("ta355::wave_augment_chain", mutates_args=())
def wave_augment_chain(wav: Tensor, lens: Tensor, desc: Tensor, stages: int, seed: int, offset: int, ev_stride: int, max_event_len: int,
                       handle: int) -> Tensor:
    """``wave_augment`` with the whole production chain: desc u8 is ``ProductionAugmentPlan.pack``'s image (the base image, then the
    cascades' float64 sections and the short-noise events, ``ev_stride`` per clip, none longer than ``max_event_len`` samples);
    ``stages`` adds 16 short noises, 32 EQ, 64 band-limit.  The handle names a ``DeviceProductionAugment``.  No autograd."""
    return module_of(handle)._apply_chain(wav, lens, desc, stages, seed, offset, ev_stride, max_event_len)


@wave_augment_chain.register_fake
def _(wav, lens, desc, stages, seed, offset, ev_stride, max_event_len, handle):
    return torch.empty_like(wav)


# ============================================================================ forced alignment
@torch.library.custom_op("ta355::ctc_align", mutates_args=())
def ctc_align(emission: Tensor, cu_frames: Tensor, tokens: Tensor, cu_tokens: Tensor, blank_id: int, max_frames: int, max_tokens: int,
              trellis_off: Optional[Tensor], trellis_numel: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """N ragged clips in one launch (``ops.ctc_align``): emission f32 [sum T_n, C] log-probabilities, cu_frames / cu_tokens i32 [N + 1],
    tokens i32 [sum J_n] -> (frames i32 [sum J_n]: the frame of every token, -1 in clips that did not align; score f32 [N] =
    trellis[T_n, J_n]; status i32 [N]: 0 aligned, 1 failed; the clips' trellises, flat f32 [trellis_numel] at the element offsets
    ``trellis_off`` i64 [N], or empty without ``trellis_off``).  No autograd: the path is integers."""
    from . import ops
    frames, score, status, trellis = ops.ctc_align(emission, cu_frames, tokens, cu_tokens, blank_id, max_frames, max_tokens,
                                                   trellis_off=trellis_off, trellis_numel=trellis_numel)
    return frames, score, status, trellis if trellis is not None else torch.empty(0, device=emission.device, dtype=F32)


@ctc_align.register_fake
def _(emission, cu_frames, tokens, cu_tokens, blank_id, max_frames, max_tokens, trellis_off, trellis_numel):
    N = cu_frames.shape[0] - 1
    return (tokens.new_empty(tokens.shape), emission.new_empty((N,)), tokens.new_empty((N,)),
            emission.new_empty((trellis_numel if trellis_off is not None else 0,)))


@torch.library.custom_op("ta355::ctc_align_long", mutates_args=("workspace",))
def ctc_align_long(emission: Tensor, cu_frames: Tensor, tokens: Tensor, cu_tokens: Tensor, blank_id: int, max_frames: int,
                   max_tokens: int, col_block: int, frame_block: int, trellis_off: Optional[Tensor], trellis_numel: int,
                   workspace: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``ctc_align`` beyond its envelope (``ops.ctc_align_long``, csrc/align_long.hip): the same inputs and the same four outputs,
    byte for byte, for up to 64 clips of up to 1 048 576 frames and 262 144 tokens, as a tiled wavefront of launches.  ``col_block``
    (a multiple of 64) x ``frame_block`` is the tile, 0 = the default; ``workspace``: u8 scratch of
    ``ta_ctc_align_long_workspace_bytes`` bytes whose contents do not matter (None: allocated here).  No autograd."""
    from . import ops
    frames, score, status, trellis = ops.ctc_align_long(emission, cu_frames, tokens, cu_tokens, blank_id, max_frames, max_tokens,
                                                        col_block=col_block, frame_block=frame_block, trellis_off=trellis_off,
                                                        trellis_numel=trellis_numel, workspace=workspace)
    return frames, score, status, trellis if trellis is not None else torch.empty(0, device=emission.device, dtype=F32)


@ctc_align_long.register_fake
def _(emission, cu_frames, tokens, cu_tokens, blank_id, max_frames, max_tokens, col_block, frame_block, trellis_off, trellis_numel,
      workspace):
    N = cu_frames.shape[0] - 1
    return (tokens.new_empty(tokens.shape), emission.new_empty((N,)), tokens.new_empty((N,)),
            emission.new_empty((trellis_numel if trellis_off is not None else 0,)))


# ============================================================================ text alignment
@torch.library.custom_op("ta355::text_align", mutates_args=("workspace",))
def text_align(ref: Tensor, cu_ref: Tensor, hyp: Tensor, cu_hyp: Tensor, max_n: int, max_m: int, mode: int, want_path: bool,
               col_block: int, row_block: int, workspace: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """N ragged pairs of int32 symbol ids (``ops.text_align``, csrc/text_align.hip): ref i32 [sum n_p], hyp i32 [sum m_p], cu_ref /
    cu_hyp i32 [N + 1]; mode 0 = edit distance (WER / CER counts), 1 = LCS (the reference evaluator's word matching) ->
    (dist i32 [N]; counts i32 [N, 4]: hits, substitutions, deletions, insertions; map i32 [sum n_p]: the hypothesis index matched to
    every reference position, -1 for none; status i32 [N]: 0 ok, 2 refused).  Without ``want_path`` counts is zero and map is empty.
    ``col_block`` x ``row_block``: the long kernel's tile, 0 = the default; ``workspace``: u8 scratch of
    ``ta_text_align_workspace_bytes`` bytes whose contents do not matter (None: sized from the pairs and allocated here).  No
    autograd: everything is integers."""
    from . import ops
    dist, counts, map_, status = ops.text_align(ref, cu_ref, hyp, cu_hyp, max_n, max_m, mode, want_path, col_block=col_block,
                                                row_block=row_block, workspace=workspace)
    return dist, counts, map_ if map_ is not None else torch.empty(0, device=ref.device, dtype=torch.int32), status


@text_align.register_fake
def _(ref, cu_ref, hyp, cu_hyp, max_n, max_m, mode, want_path, col_block, row_block, workspace):
    N = cu_ref.shape[0] - 1
    return (ref.new_empty((N,)), ref.new_empty((N, 4)), ref.new_empty(ref.shape if want_path else (0,)), ref.new_empty((N,)))


# ============================================================================ long-form segmentation
@torch.library.custom_op("ta355::wave_cut_cost", mutates_args=())
def wave_cut_cost(wav: Tensor, offsets: Tensor, max_samples: int, smooth_positions: int, cut_penalty: float) -> Tensor:
    """wav flat f32, offsets i64 [R + 1] -> cost f32 [R, ceil(max_samples / 160) + 1]: the cost of cutting recording r at each of its
    positions 0 .. T_r (smoothed short-time power + ``cut_penalty`` x its mean power; ``ops.wave_cut_cost``), NaN beyond T_r.  No
    autograd: the waveform is data."""
    from . import ops
    return ops.wave_cut_cost(wav, offsets, max_samples, smooth_positions, cut_penalty)


@wave_cut_cost.register_fake
def _(wav, offsets, max_samples, smooth_positions, cut_penalty):
    return wav.new_empty((offsets.shape[0] - 1, -(-max_samples // 160) + 1))


@torch.library.custom_op("ta355::cut_plan", mutates_args=())
def cut_plan(cost: Tensor, offsets: Tensor, max_samples: int, min_len: int, max_len: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The cheapest cuts with every window within [min_len, max_len] positions (``ops.cut_plan``) -> (cuts i32 [R, max_T // min_len + 2],
    n_seg i32 [R], dp_T f32 [R], back i32 [R, cost.shape[1]]).  No autograd: the plan is integers."""
    from . import ops
    return ops.cut_plan(cost, offsets, max_samples, min_len, max_len)


@cut_plan.register_fake
def _(cost, offsets, max_samples, min_len, max_len):
    R = offsets.shape[0] - 1
    i32 = torch.int32
    return (cost.new_empty((R, -(-max_samples // 160) // min_len + 2), dtype=i32), cost.new_empty((R,), dtype=i32), cost.new_empty((R,)),
            cost.new_empty((R, cost.shape[1]), dtype=i32))


@torch.library.custom_op("ta355::wave_windows", mutates_args=())
def wave_windows(wav: Tensor, start: Tensor, length: Tensor, Ls: int) -> Tuple[Tensor, Tensor]:
    """wav flat f32, start i64 [W], length i32 [W] -> (f32 [W, Ls]: the windows, zero padded; their lengths i64 [W]): the inputs of
    ``logmel`` (``ops.wave_windows``)."""
    from . import ops
    return ops.wave_windows(wav, start, length, Ls)


@wave_windows.register_fake
def _(wav, start, length, Ls):
    W = start.shape[0]
    return wav.new_empty((W, Ls)), start.new_empty((W,))


# ============================================================================ voice activity detection
@torch.library.custom_op("ta355::vad", mutates_args=())
def vad(wav: Tensor, offsets: Tensor, max_samples: int, smooth: int, noise_window: int, noise_bias: float, threshold: float,
        floor: float) -> Tuple[Tensor, Tensor, Tensor]:
    """wav flat f32, offsets i64 [R + 1] -> (stat f32 [R, F_max] = the band-wise likelihood-ratio statistic of every 256-sample frame
    against a minimum-statistics noise floor, flags u8 [R, F_max] = stat > threshold, n_frames i32 [R]) with F_max =
    (max_samples - 1) // 256 (0 up to 256 samples); zeros beyond a recording's own frames (``ops.vad``).  No autograd: the waveform
    is data."""
    from . import ops
    return ops.vad(wav, offsets, max_samples, smooth, noise_window, noise_bias, threshold, floor)


@vad.register_fake
def _(wav, offsets, max_samples, smooth, noise_window, noise_bias, threshold, floor):
    R, F = offsets.shape[0] - 1, (0 if max_samples <= 256 else (max_samples - 1) // 256)
    return wav.new_empty((R, F)), wav.new_empty((R, F), dtype=torch.uint8), wav.new_empty((R,), dtype=torch.int32)


# ============================================================================ speaker turns
@torch.library.custom_op("ta355::spk_vote", mutates_args=())
def spk_vote(first: Tensor, last: Tensor, label: Tensor, cu_win: Tensor, S: int, n_frames: Tensor, max_frames: int, vad: Tensor,
             n_vad: Tensor, cu_cap: Tensor, capacity: int, voting_rate: float, vad_frame_s: float, min_segment_s: float, short_gap_s: float,
             same_gap_s: float) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Windows (first, last, label i32 [sum Nw], cu_win i32 [R + 1]) vote on the frames of R voting grids; vad u8 [R, ld] with n_vad
    i32 [R] -> (run_spk, run_f0, run_f1 i32 [capacity] with recording r's runs at cu_cap[r] .., n_runs i32 [R], status i32 [R]);
    ``capacity`` is cu_cap[R] (``ops.spk_vote``).  Integers only: no autograd."""
    from . import ops
    return ops.spk_vote(first, last, label, cu_win, S, n_frames, max_frames, vad, n_vad, cu_cap,
                        (voting_rate, vad_frame_s, min_segment_s, short_gap_s, same_gap_s), capacity=capacity)


@spk_vote.register_fake
def _(first, last, label, cu_win, S, n_frames, max_frames, vad, n_vad, cu_cap, capacity, voting_rate, vad_frame_s, min_segment_s,
      short_gap_s, same_gap_s):
    R = cu_win.shape[0] - 1
    return (first.new_empty((capacity,)), first.new_empty((capacity,)), first.new_empty((capacity,)), first.new_empty((R,)),
            first.new_empty((R,)))


@torch.library.custom_op("ta355::spk_merge", mutates_args=())
def spk_merge(run_spk: Tensor, run_f0: Tensor, run_f1: Tensor, cu_run: Tensor, n_run: Optional[Tensor], voting_rate: float, vad_frame_s: float,
              min_segment_s: float, short_gap_s: float, same_gap_s: float) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Runs (speaker, f0, f1) i32 [sum runs] of R recordings -> (seg_spk, seg_f0, seg_f1 i32 [sum runs], n_seg i32 [R]): every
    recording's merged turns at cu_run[r] ..; n_run i32 [R] or None: how many positions of a recording's range hold runs
    (``ops.spk_merge``)."""
    from . import ops
    return ops.spk_merge(run_spk, run_f0, run_f1, cu_run, (voting_rate, vad_frame_s, min_segment_s, short_gap_s, same_gap_s), n_run=n_run)


@spk_merge.register_fake
def _(run_spk, run_f0, run_f1, cu_run, n_run, voting_rate, vad_frame_s, min_segment_s, short_gap_s, same_gap_s):
    return (run_spk.new_empty(run_spk.shape), run_spk.new_empty(run_spk.shape), run_spk.new_empty(run_spk.shape),
            run_spk.new_empty((cu_run.shape[0] - 1,)))


@torch.library.custom_op("ta355::spk_words", mutates_args=())
def spk_words(word_start: Tensor, word_end: Tensor, cu_word: Tensor, seg_start: Tensor, seg_end: Tensor, cu_seg: Tensor) -> Tensor:
    """Word and segment times f64, ragged over R recordings -> i32 [sum W]: every word's segment index within its recording, -1
    without segments (``ops.spk_words``)."""
    from . import ops
    return ops.spk_words(word_start, word_end, cu_word, seg_start, seg_end, cu_seg)


@spk_words.register_fake
def _(word_start, word_end, cu_word, seg_start, seg_end, cu_seg):
    return word_start.new_empty(word_start.shape, dtype=torch.int32)


# ============================================================================ decoding scores
@torch.library.custom_op("ta355::token_scores", mutates_args=())
def token_scores(logits: Tensor, chosen: Tensor, V: int, top_k: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """One step of f32 logits [B, ld] (V valid columns, -inf allowed) and the chosen ids i64 [B] -> (logprob f32 [B] = log softmax at the
    chosen id, entropy f32 [B], top_ids i64 [B, top_k], top_logprobs f32 [B, top_k]; ``ops.token_scores``).  The decode loop runs the
    same kernel inside its captured step (``ASRModel.generate(return_token_scores=True)``); this is for callers who hold their own
    logits.  No autograd."""
    from . import ops
    return ops.token_scores(logits, chosen, V, top_k)


@token_scores.register_fake
def _(logits, chosen, V, top_k):
    B = logits.shape[0]
    return (logits.new_empty((B,)), logits.new_empty((B,)), chosen.new_empty((B, top_k)), logits.new_empty((B, top_k)))


# ============================================================================ decoding options
@torch.library.custom_op("ta355::logits_sequence_bias", mutates_args=("logits",))
def logits_sequence_bias(logits: Tensor, V: int, context: Tensor, seq_tokens: Tensor, seq_offsets: Tensor, seq_bias: Tensor,
                         group_starts: Tensor) -> None:
    """SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor on f32 logits [B, ld] (V valid columns), IN PLACE, given the ids so far
    ``context`` i64 [B, n] and the four tensors of ``ops.build_sequence_table`` (tokens, offsets, bias, groups) on the same device."""
    from . import ops
    tab = dict(tokens=seq_tokens, offsets=seq_offsets, bias=seq_bias, groups=group_starts, n_seq=seq_bias.numel(),
               n_groups=group_starts.numel() - 1, n_tokens=seq_tokens.numel())
    ops.logits_sequence_bias(logits, V, context, tab)


@torch.library.custom_op("ta355::logits_step_rules", mutates_args=("logits",))
def logits_step_rules(logits: Tensor, V: int, step: int, max_new: int, forced_eos_ids: Sequence[int], eos_ids: Sequence[int],
                      decay_start: int, decay_factor: float, suppress_tokens: Sequence[int], begin_suppress_tokens: Sequence[int]) -> None:
    """ForcedEOSToken, ExponentialDecayLengthPenalty (``decay_start`` < 0 = off), SuppressTokens and SuppressTokensAtBegin on f32 logits
    [B, ld], IN PLACE, for step ``step`` (tokens generated so far) of ``max_new``; empty lists switch a rule off."""
    from . import ops
    ops.logits_step_rules(logits, V, step, max_new, list(forced_eos_ids), list(eos_ids),
                          None if decay_start < 0 else (decay_start, decay_factor), list(suppress_tokens), list(begin_suppress_tokens))


@torch.library.custom_op("ta355::logits_warp_ext", mutates_args=("logits",))
def logits_warp_ext(logits: Tensor, V: int, min_p: float, typical_p: float, epsilon_cutoff: float, eta_cutoff: float) -> None:
    """MinP, Typical, Epsilon and Eta warpers on f32 logits [B, ld], IN PLACE, in HF's order (off: 0, 1, 0, 0)."""
    from . import ops
    ops.logits_warp_ext(logits, V, min_p, typical_p, epsilon_cutoff, eta_cutoff)


# ============================================================================ beam search
@torch.library.custom_op("ta355::beam_logprobs", mutates_args=("logits",))
def beam_logprobs(logits: Tensor, V: int) -> None:
    """log_softmax over the first V columns of f32 logits [R, ld], IN PLACE (``ops.beam_logprobs``; HF _beam_search's first operation on a
    step's logits).  No autograd."""
    from . import ops
    ops.beam_logprobs(logits, V)


@torch.library.custom_op("ta355::beam_topk", mutates_args=())
def beam_topk(rows: Tensor, V: int, score: Tensor, M: int) -> Tuple[Tensor, Tensor]:
    """HF _get_top_k_continuations: f32 rows [B * K, ld] and running scores f32 [B, K] -> (cand_score f32 [B, M], cand_flat i32 [B, M]),
    descending, lowest flat index k * V + v on ties (``ops.beam_topk``)."""
    from . import ops
    return ops.beam_topk(rows, V, score, M)


@beam_topk.register_fake
def _(rows, V, score, M):
    return rows.new_empty((score.shape[0], M)), rows.new_empty((score.shape[0], M), dtype=torch.int32)


@torch.library.custom_op("ta355::beam_advance", mutates_args=("state",))
def beam_advance(cand_score: Tensor, cand_flat: Tensor, V: int, eos_ids: Sequence[int], pad_id: int, len_div: Tensor, early_stopping: int,
                 length_penalty: float, state: List[Tensor]) -> None:
    """One step of HF's beam bookkeeping (``ops.beam_advance``) on the 15 state tensors of ``ops.BEAM_STATE``, in that order, IN PLACE.
    ``early_stopping``: 0 False, 1 True, 2 "never"."""
    from . import ops
    ops.beam_advance(cand_score, cand_flat, V, list(eos_ids), pad_id, len_div, "never" if early_stopping == 2 else bool(early_stopping),
                     length_penalty, dict(zip(ops.BEAM_STATE, state)))


@torch.library.custom_op("ta355::kv_beam_expand", mutates_args=())
def kv_beam_expand(ksrc: Tensor, vsrc: Tensor, num_beams: int, Lmax: int) -> Tuple[Tensor, Tensor]:
    """The B-row prompt caches bf16 [layers, B, kv_heads, L, head_dim] -> caches [layers, B * num_beams, kv_heads, Lmax, head_dim] with
    every clip's slots [0, L) in its num_beams rows (``ops.kv_beam_expand``)."""
    from . import ops
    return ops.kv_beam_expand(ksrc, vsrc, num_beams, Lmax)


@kv_beam_expand.register_fake
def _(ksrc, vsrc, num_beams, Lmax):
    nl, B, h, _, d = ksrc.shape
    return ksrc.new_empty((nl, B * num_beams, h, Lmax, d)), ksrc.new_empty((nl, B * num_beams, h, Lmax, d))


@torch.library.custom_op("ta355::kv_beam_reorder", mutates_args=("kcache", "vcache"))
def kv_beam_reorder(kcache: Tensor, vcache: Tensor, num_beams: int, L: int, max_new: int, parent: Tensor, slot_dev: Tensor) -> None:
    """Slots [L, *slot_dev) of the num_beams rows of every clip permuted by ``parent`` i32 [R], IN PLACE, both caches, every layer
    (``ops.kv_beam_reorder``; HF's reorder_cache)."""
    from . import ops
    ops.kv_beam_reorder(kcache, vcache, num_beams, L, max_new, parent, slot_dev)


# ============================================================================ frozen encoder
@torch.library.custom_op("ta355::encoder_forward", mutates_args=())
def encoder_forward(input_features: Tensor, frame_keep: Optional[Tensor], handle: int, return_f32: bool) -> Tensor:
    """f32 [B, n_mels, T] -> last_hidden_state [B, (T-1)//2+1, H] (bf16, or f32 on request); ``frame_keep`` f32 [B*S] is the
    train-time whole-frame dropout mask fused into the final LayerNorm (tiny_audio/asr_modeling.py:458-479)."""
    return module_of(handle)._forward_impl(input_features, frame_keep, return_f32)


@encoder_forward.register_fake
def _(input_features, frame_keep, handle, return_f32):
    enc = module_of(handle)
    B, _, T = input_features.shape
    return input_features.new_empty((B, enc.output_length(T), enc.config.hidden_size), dtype=F32 if return_f32 else BF16)


@torch.library.custom_op("ta355::encoder_forward_ragged", mutates_args=())
def encoder_forward_ragged(input_features: Tensor, mel_lengths: List[int], frame_keep: Optional[Tensor], handle: int,
                           return_f32: bool) -> Tensor:
    """The GLM-ASR tower with every clip encoded at its own length (not in the reference's training forward; opt-in): rows
    [b, :S_b] = the encoder applied to ``input_features[b:b+1, :, :mel_lengths[b]]`` alone, rows [b, S_b:] and dropped frames exact
    zeros, the padded [B, (T-1)//2+1, H] layout of ``encoder_forward``.  The lengths are host integers: they size the launches."""
    return module_of(handle)._forward_ragged_impl(input_features, mel_lengths, frame_keep, return_f32)


@encoder_forward_ragged.register_fake
def _(input_features, mel_lengths, frame_keep, handle, return_f32):
    enc = module_of(handle)
    B, _, T = input_features.shape
    return input_features.new_empty((B, enc.output_length(T), enc.config.hidden_size), dtype=F32 if return_f32 else BF16)


@torch.library.custom_op("ta355::whisper_encoder_forward", mutates_args=())
def whisper_encoder_forward(input_features: Tensor, frame_keep: Optional[Tensor], handle: int, return_f32: bool) -> Tensor:
    """Whisper tower: f32 [B, n_mels, 2 * max_source_positions] -> last_hidden_state [B, max_source_positions, H] (bf16, or f32 on
    request); ``frame_keep`` as in ``encoder_forward``.  Replaces ``WhisperEncoder.forward`` (tiny_audio/asr_modeling.py:203-237)."""
    return module_of(handle)._forward_impl(input_features, frame_keep, return_f32)


@whisper_encoder_forward.register_fake
def _(input_features, frame_keep, handle, return_f32):
    enc = module_of(handle)
    B, _, T = input_features.shape
    return input_features.new_empty((B, enc.output_length(T), enc.config.hidden_size), dtype=F32 if return_f32 else BF16)


# ============================================================================ wav2vec2 acoustic model
@torch.library.custom_op("ta355::wav2vec2_emissions", mutates_args=())
def wav2vec2_emissions(waveforms: Tensor, lengths: List[int], handle: int) -> Tensor:
    """Frozen wav2vec2 CTC model (``Wav2Vec2CtcMI355X``): f32 [B, Ls] 16 kHz waveforms, clip b = its first ``lengths[b]`` samples
    (400 <= length <= Ls) -> log-softmax emissions f32 [sum T_b, n_classes], T_b = (lengths[b] - 400) // 320 + 1, on the device in
    the layout ``ctc_align`` takes.  Replaces the torchaudio forward of tiny_audio/alignment.py:206-211.  No autograd."""
    return module_of(handle)._forward_impl(waveforms, lengths)


@wav2vec2_emissions.register_fake
def _(waveforms, lengths, handle):
    from .wav2vec2 import frames_of
    return waveforms.new_empty((sum(frames_of(n) for n in lengths), module_of(handle).config.n_classes), dtype=F32)


@torch.library.custom_op("ta355::wav2vec2_sln_emissions", mutates_args=())
def wav2vec2_sln_emissions(waveforms: Tensor, lengths: List[int], normalized: bool, handle: int) -> Tensor:
    """``wav2vec2_emissions`` for the layer-norm / stable family (``Wav2Vec2CtcMI355X`` with ``feat_extract_norm="layer"``:
    wav2vec2-large-lv60, XLSR-53, XLS-R 300M, MMS 300M).  ``normalized``: the waveforms already have zero mean and unit variance,
    so a ``normalize_input`` model skips that step (``emissions_long`` applies the whole recording's statistics once).  Replaces
    ``Wav2Vec2ForCTC.forward`` of that configuration + ``log_softmax``.  No autograd."""
    return module_of(handle)._forward_impl(waveforms, lengths, None, normalized)


@wav2vec2_sln_emissions.register_fake
def _(waveforms, lengths, normalized, handle):
    from .wav2vec2 import frames_of
    return waveforms.new_empty((sum(frames_of(n) for n in lengths), module_of(handle).config.n_classes), dtype=F32)


# ============================================================================ ECAPA-TDNN speaker embeddings
@torch.library.custom_op("ta355::ecapa_embeddings", mutates_args=())
def ecapa_embeddings(audio: Tensor, starts: List[int], lengths: List[int], window_samples: int, handle: int) -> Tensor:
    """Frozen ECAPA-TDNN (``EcapaTdnnMI355X``): f32 [n] 16 kHz audio, window i = its samples ``starts[i] .. starts[i] + lengths[i]``
    reflect-padded on the right to ``window_samples`` -> embeddings f32 [N, lin_neurons] on the device.  Replaces the
    one-window-per-call SpeechBrain loop of tiny_audio/diarization.py:457-517.  No autograd."""
    return module_of(handle)._embed_impl(audio, starts, lengths, window_samples)


@ecapa_embeddings.register_fake
def _(audio, starts, lengths, window_samples, handle):
    return audio.new_empty((len(starts), module_of(handle).config.lin_neurons), dtype=F32)


# ============================================================================ speaker clustering
@torch.library.custom_op("ta355::spk_affinity", mutates_args=())
def spk_affinity(embeddings: Tensor, keep: int) -> Tuple[Tensor, Tensor, Tensor]:
    """f32 [N, D] window embeddings -> (W f32 [N, N]: cosine affinity, every row pruned to its ``keep`` largest entries, symmetrised,
    zero diagonal; deg f32 [N]: its row sums; the survivors per row before symmetrisation i32 [N]).  Replaces get_sim_mat / p_pruning
    / get_laplacian's host matrices (tiny_audio/diarization.py:49-89; ``ops.spk_affinity``).  No autograd."""
    from . import ops
    W, deg, kept = ops.spk_affinity(embeddings, keep, want_kept=True)
    return W, deg, kept


@spk_affinity.register_fake
def _(embeddings, keep):
    N = embeddings.shape[0]
    return embeddings.new_empty((N, N)), embeddings.new_empty((N,)), embeddings.new_empty((N,), dtype=torch.int32)


@torch.library.custom_op("ta355::spk_laplacian_matmul", mutates_args=())
def spk_laplacian_matmul(W: Tensor, deg: Tensor, X: Tensor) -> Tensor:
    """Y [N, p] = diag(deg) X - W X, p <= 32: the graph Laplacian of tiny_audio/diarization.py:87-89 applied without forming it."""
    from . import ops
    return ops.spk_laplacian_matmul(W, deg, X)


@spk_laplacian_matmul.register_fake
def _(W, deg, X):
    return X.new_empty(X.shape)


@torch.library.custom_op("ta355::spk_panel_gram", mutates_args=())
def spk_panel_gram(A: Tensor, B: Tensor) -> Tensor:
    """C [a, b] = A^T B for two panels of N rows, summed in a fixed order (``ops.spk_panel_gram``)."""
    from . import ops
    return ops.spk_panel_gram(A, B)


@spk_panel_gram.register_fake
def _(A, B):
    return A.new_empty((A.shape[1], B.shape[1]))


@torch.library.custom_op("ta355::spk_panel_update", mutates_args=())
def spk_panel_update(B: Tensor, A: Tensor, C: Tensor) -> Tensor:
    """B - A C for ``B`` [N, b <= 32], ``A`` [N, a], ``C`` [a, b] (``ops.spk_panel_update`` on a copy of B)."""
    from . import ops
    return ops.spk_panel_update(B.clone(memory_format=torch.contiguous_format), A, C)


@spk_panel_update.register_fake
def _(B, A, C):
    return B.new_empty(B.shape)


@torch.library.custom_op("ta355::spk_panel_combine", mutates_args=())
def spk_panel_combine(V: Tensor, Z: Tensor) -> Tensor:
    """Y [N, m <= 32] = V Z (``ops.spk_panel_combine``)."""
    from . import ops
    return ops.spk_panel_combine(V, Z)


@spk_panel_combine.register_fake
def _(V, Z):
    return V.new_empty((V.shape[0], Z.shape[1]))


# ============================================================================ MLP projector
@torch.library.custom_op("ta355::mlp_projector", mutates_args=())
def mlp_projector(x: Tensor, w1: Tensor, g1: Tensor, w2: Tensor, g2: Tensor, handle: int) -> Tuple[Tensor, Tensor, Tensor]:
    """x [B, S, E] -> (y f32 [B, N, D], bf16 image of x, tape).  w1 / g1 / w2 / g2 are the fp32 masters (autograd inputs);
    the kernels read the module's packed bf16 images of them."""
    mod = module_of(handle)
    B, S, _ = x.shape
    xb, xb_out = _bf16_image(x)
    wts = mod._packed_weights()
    L_ = _lib.lib()
    N = mod.get_output_length(S)
    tape = torch.empty(L_.ta_mlp_tape_bytes(C.byref(wts), B, S), device=x.device, dtype=torch.uint8)
    y = torch.empty((B, N, mod.llm_dim), device=x.device, dtype=F32)
    _lib.check(L_.ta_mlp_projector_forward(C.byref(wts), ptr(xb), B, S, ptr(y), ptr(tape), stream()), "ta_mlp_projector_forward")
    return y, xb_out, tape


@mlp_projector.register_fake
def _(x, w1, g1, w2, g2, handle):
    mod = module_of(handle)
    B, S, _ = x.shape
    n_tape = _lib.lib().ta_mlp_tape_bytes(C.byref(mod._packed_weights_meta()), B, S)        # host-only size query
    return (x.new_empty((B, mod.get_output_length(S), mod.llm_dim), dtype=F32),
            x.new_empty((0,) if _is_bf16_image(x) else x.shape, dtype=BF16), x.new_empty((n_tape,), dtype=torch.uint8))


@torch.library.custom_op("ta355::mlp_projector_backward", mutates_args=())
def mlp_projector_backward(dy: Tensor, xb: Tensor, tape: Tensor, handle: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (dW1, dg1, dW2, dg2) f32; no d x (the encoder is frozen)."""
    mod = module_of(handle)
    B, S, _ = xb.shape
    wts = mod._packed_weights()
    L_ = _lib.lib()
    dev = dy.device
    dy = dy.to(F32).contiguous()
    dW1 = torch.empty(mod.linear_1.weight.shape, device=dev, dtype=F32)
    dW2 = torch.empty(mod.linear_2.weight.shape, device=dev, dtype=F32)
    dg1 = torch.empty(mod.norm.weight.shape, device=dev, dtype=F32)
    dg2 = torch.empty(mod.norm_2.weight.shape, device=dev, dtype=F32)
    ws = torch.empty(L_.ta_mlp_bwd_workspace_bytes(C.byref(wts), B, S), device=dev, dtype=torch.uint8)
    _lib.check(L_.ta_mlp_projector_backward(C.byref(wts), ptr(xb), B, S, ptr(dy), ptr(tape), ptr(dW1), ptr(dg1), ptr(dW2),
                                            ptr(dg2), ptr(ws), ws.numel(), stream()), "ta_mlp_projector_backward")
    return dW1, dg1, dW2, dg2


@mlp_projector_backward.register_fake
def _(dy, xb, tape, handle):
    mod = module_of(handle)
    f = lambda p: dy.new_empty(p.shape, dtype=F32)
    return f(mod.linear_1.weight), f(mod.norm.weight), f(mod.linear_2.weight), f(mod.norm_2.weight)


def _mlp_setup(ctx, inputs, output):
    ctx.handle = inputs[5]
    ctx.module = module_of(ctx.handle)       # the graph keeps its module alive: the handle cannot go stale before the backward
    ctx.set_materialize_grads(False)         # or autograd zero-fills a gradient for the saved-state outputs (xb, tape) every step
    ctx.save_for_backward(output[1] if output[1].numel() else inputs[0], output[2])


def _mlp_bwd(ctx, dy, _dxb, _dtape):
    if dy is None:
        return (None,) * 6
    xb, tape = ctx.saved_tensors
    dW1, dg1, dW2, dg2 = torch.ops.ta355.mlp_projector_backward(dy, xb, tape, ctx.handle)
    return None, dW1, dg1, dW2, dg2, None


mlp_projector.register_autograd(_mlp_bwd, setup_context=_mlp_setup)


# ============================================================================ MoE projector
@torch.library.custom_op("ta355::moe_projector", mutates_args=())
def moe_projector(x: Tensor, noise: Optional[Tensor], params: Sequence[Tensor], handle: int,
                  training: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """x [B, S, E] -> (y f32 [B, N, D], aux f32 [], bf16 image of x, tape).  ``params``: norm.weight, router.weight, then
    fc1.weight, fc1.bias, fc2.weight, fc2.bias of routed experts 0..E-1 and of the shared expert (``_param_list``)."""
    mod = module_of(handle)
    B, S, _ = x.shape
    xb, xb_out = _bf16_image(x)
    wts = mod._packed_weights()
    L_ = _lib.lib()
    dev = x.device
    N = mod.get_output_length(S)
    tape = torch.empty(L_.ta_moe_tape_bytes(C.byref(wts), B, S), device=dev, dtype=torch.uint8)
    y = torch.empty((B, N, mod.llm_dim), device=dev, dtype=F32)
    aux = torch.zeros((), device=dev, dtype=F32)
    _lib.check(L_.ta_moe_projector_forward(C.byref(wts), ptr(xb), B, S, ptr(noise), int(training), ptr(y), ptr(aux), ptr(tape),
                                           stream()), "ta_moe_projector_forward")
    return y, aux, xb_out, tape


@moe_projector.register_fake
def _(x, noise, params, handle, training):
    mod = module_of(handle)
    B, S, _ = x.shape
    n_tape = _lib.lib().ta_moe_tape_bytes(C.byref(mod._packed_weights_meta()), B, S)
    return (x.new_empty((B, mod.get_output_length(S), mod.llm_dim), dtype=F32), x.new_empty((), dtype=F32),
            x.new_empty((0,) if _is_bf16_image(x) else x.shape, dtype=BF16), x.new_empty((n_tape,), dtype=torch.uint8))


@torch.library.custom_op("ta355::moe_projector_backward", mutates_args=())
def moe_projector_backward(dy: Tensor, d_aux: Tensor, xb: Tensor, noise: Optional[Tensor], tape: Tensor, handle: int,
                           training: bool) -> List[Tensor]:
    """Gradients of sum(dy * y) + d_aux * aux (d_aux: a DEVICE scalar) -> [d norm.weight, d router.weight, then one STACKED
    tensor per kind over the E routed experts + the shared expert: d fc1.weight [E+1, H, In], d fc1.bias [E+1, H],
    d fc2.weight [E+1, D, H], d fc2.bias [E+1, D]].  (Operator outputs may not alias one another, and the constant stride
    between the experts' buffers is what lets the library write them from one grouped launch.)"""
    mod = module_of(handle)
    B, S, _ = xb.shape
    wts = mod._packed_weights()
    L_ = _lib.lib()
    dev = dy.device
    dy = dy.to(F32).contiguous()
    E = mod.num_experts
    adapters = list(mod.experts) + [mod.shared_expert]
    f = lambda p: torch.empty(p.shape, device=dev, dtype=F32)
    g_norm, g_router = f(mod.norm.weight), f(mod.router.weight)
    # the adapters' gradients of one kind are slices of ONE tensor: a constant stride between the experts' buffers is what
    # lets the library write all per-expert weight gradients from one grouped launch
    stack = lambda ps: torch.empty((len(ps),) + tuple(ps[0].shape), device=dev, dtype=F32)
    GW1, Gb1 = stack([a.fc1.weight for a in adapters]), stack([a.fc1.bias for a in adapters])
    GW2, Gb2 = stack([a.fc2.weight for a in adapters]), stack([a.fc2.bias for a in adapters])
    gW1, gb1, gW2, gb2 = (list(t.unbind(0)) for t in (GW1, Gb1, GW2, Gb2))
    arr = lambda ts: (C.c_void_p * (E + 1))(*[t.data_ptr() for t in ts])
    ws = torch.empty(L_.ta_moe_bwd_workspace_bytes(C.byref(wts), B, S), device=dev, dtype=torch.uint8)
    da = d_aux.to(device=dev, dtype=F32).reshape(1).contiguous()
    _lib.check(L_.ta_moe_projector_backward_dev(C.byref(wts), ptr(xb), B, S, ptr(dy), ptr(da), ptr(noise), int(training),
                                                ptr(tape), ptr(g_norm), ptr(g_router), arr(gW1), arr(gb1), arr(gW2), arr(gb2),
                                                ptr(ws), ws.numel(), stream()), "ta_moe_projector_backward_dev")
    return [g_norm, g_router, GW1, Gb1, GW2, Gb2]


def moe_router_aux_grads(d_aux: Tensor, xb: Tensor, noise: Optional[Tensor], tape: Tensor, handle: int, training: bool):
    """d_aux * d(aux) / d(norm.weight), d(router.weight) alone (ta_moe_router_aux_grads): the part of those two gradients that must
    NOT be divided by the global token count."""
    mod = module_of(handle)
    B, S, _ = xb.shape
    wts = mod._packed_weights()
    L_ = _lib.lib()
    dev = xb.device
    sn = torch.empty(mod.norm.weight.shape, device=dev, dtype=F32)
    sr = torch.empty(mod.router.weight.shape, device=dev, dtype=F32)
    ws = torch.empty(L_.ta_moe_bwd_workspace_bytes(C.byref(wts), B, S), device=dev, dtype=torch.uint8)
    da = d_aux.to(device=dev, dtype=F32).reshape(1).contiguous()
    _lib.check(L_.ta_moe_router_aux_grads(C.byref(wts), ptr(xb), B, S, ptr(da), ptr(noise), int(training), ptr(tape), ptr(sn), ptr(sr),
                                          ptr(ws), ws.numel(), stream()), "ta_moe_router_aux_grads")
    return sn, sr


@moe_projector_backward.register_fake
def _(dy, d_aux, xb, noise, tape, handle, training):
    mod = module_of(handle)
    n = mod.num_experts + 1
    a = mod.shared_expert
    f = lambda *s: dy.new_empty(s, dtype=F32)
    return [f(*mod.norm.weight.shape), f(*mod.router.weight.shape), f(n, *a.fc1.weight.shape), f(n, *a.fc1.bias.shape),
            f(n, *a.fc2.weight.shape), f(n, *a.fc2.bias.shape)]


def _moe_setup(ctx, inputs, output):
    x, noise, params, handle, training = inputs
    ctx.handle, ctx.training, ctx.has_noise, ctx.n_params = handle, training, noise is not None, len(params)
    ctx.module = module_of(handle)
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(output[2] if output[2].numel() else x, output[3], *([noise] if noise is not None else []))


def _moe_bwd(ctx, dy, d_aux, _dxb, _dtape):
    if dy is None and d_aux is None:
        return None, None, [None] * ctx.n_params, None, None
    xb, tape, *rest = ctx.saved_tensors
    noise = rest[0] if ctx.has_noise else None
    if d_aux is None:
        d_aux = torch.zeros((), device=dy.device, dtype=F32)
    if dy is None:
        dy = torch.zeros((xb.shape[0], module_of(ctx.handle).get_output_length(xb.shape[1]), module_of(ctx.handle).llm_dim),
                         device=xb.device, dtype=F32)
    direct = getattr(ctx.module, "_grad_direct", None)
    if direct is not None and ctx.training:
        # ASRTrainer, one micro-batch per optimizer step: the library writes every gradient straight into its segment of the trainer's flat
        # buffer (the .grad views) -- no 22 temporaries, no 22 autograd accumulation launches.  The routed experts' segments sit at a
        # constant stride there as well (fc1.weight, fc1.bias, fc2.weight, fc2.bias per expert), so the grouped launches still apply.
        mod, L_ = ctx.module, _lib.lib()
        B, S, _ = xb.shape
        wts = mod._packed_weights()
        E = mod.num_experts
        g_norm, g_router = direct[0], direct[1]
        gW1, gb1, gW2, gb2 = ([direct[2 + 4 * i + j] for i in range(E + 1)] for j in range(4))
        arr = lambda ts: (C.c_void_p * (E + 1))(*[t.data_ptr() for t in ts])
        ws = torch.empty(L_.ta_moe_bwd_workspace_bytes(C.byref(wts), B, S), device=xb.device, dtype=torch.uint8)
        da = d_aux.to(device=xb.device, dtype=F32).reshape(1).contiguous()
        _lib.check(L_.ta_moe_projector_backward_dev(C.byref(wts), ptr(xb), B, S, ptr(dy.to(F32).contiguous()), ptr(da), ptr(noise), int(ctx.training),
                                                    ptr(tape), ptr(g_norm), ptr(g_router), arr(gW1), arr(gb1), arr(gW2), arr(gb2),
                                                    ptr(ws), ws.numel(), stream()), "ta_moe_projector_backward_dev")
        # more than one rank with one micro-batch per step: the gradients go straight to the flat buffer AND the auxiliary share of
        # the two router-path gradients goes to its shadow segment (this branch used to return before the shadow fill,
        # which left aux at weight 1 / N on N > 1 ranks)
        shadow = getattr(ctx.module, "_aux_shadow", None)
        if shadow is not None:
            sn, sr = moe_router_aux_grads(d_aux, xb, noise, tape, ctx.handle, ctx.training)
            shadow["norm.weight"].add_(sn)
            shadow["router.weight"].add_(sr)
        return None, None, [None] * ctx.n_params, None, None
    g_norm, g_router, GW1, Gb1, GW2, Gb2 = torch.ops.ta355.moe_projector_backward(dy, d_aux, xb, noise, tape, ctx.handle,
                                                                                   ctx.training)
    shadow = getattr(ctx.module, "_aux_shadow", None)         # (ASRTrainer: the auxiliary-loss share of the two router-path gradients)
    if shadow is not None and ctx.training:
        sn, sr = moe_router_aux_grads(d_aux, xb, noise, tape, ctx.handle, ctx.training)
        shadow["norm.weight"].add_(sn)
        shadow["router.weight"].add_(sr)
    grads = [g_norm, g_router]                                # the order of MoEAudioProjector._param_list()
    for i in range(GW1.shape[0]):
        grads += [GW1[i], Gb1[i], GW2[i], Gb2[i]]
    return None, None, grads, None, None


moe_projector.register_autograd(_moe_bwd, setup_context=_moe_setup)


# ============================================================================ LM + shifted cross-entropy
@torch.library.custom_op("ta355::lm_forward_loss", mutates_args=())
def lm_forward_loss(audio: Tensor, trainable: Sequence[Tensor], handle: int, input_ids: Tensor, src_row: Optional[Tensor],
                    kmask: Optional[Tensor], label_rows: Optional[Tensor], label_targets: Optional[Tensor], n_label_rows: int,
                    loss_scale: float, want_logits: bool, pos: Optional[Tensor], seg: Optional[Tensor] = None, lora_p: float = 0.0,
                    lora_seed: int = 0, lora_offset: int = 0, label_smoothing: float = 0.0,
                    z_loss: float = 0.0) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (loss f32 [], per-row nll f32 [max(n, 1)], logits bf16 [B*L, vocab_pad] or empty, tape, workspace).
    ``audio`` f32 [rows, D]: the projector's output rows that replace the <audio> positions (``src_row`` from
    ta_audio_index); ``trainable``: the LoRA masters or, with a trainable base LM, its fp32 masters (autograd inputs);
    ``pos`` int32 [B*L]: RoPE position of every token row (the reference's ``position_ids``; None = arange(L) per clip);
    ``seg`` int32 [2, B*L]: the table of ops.segment_table for packed rows (block-diagonal attention inside every row; None = one
    clip per row); ``lora_p``, ``lora_seed``, ``lora_offset``: LoRA dropout (peft lora_dropout p > 0, training forwards), the triple
    that names the Philox masks (include/ta355.h ta_lora_dropout); lora_p == 0 is "no dropout"; ``label_smoothing``, ``z_loss``: the
    loss options of the cross-entropy launch (include/ta355.h ta_ce_options; both 0 = the call without options): ``loss`` is then the
    objective, the per-row nll stays plain, and the backward is unchanged.  The autograd node keeps the table,
    the triple and the module's two stream modes and hands them to ITS backward, so gradient accumulation and backwards run out
    of order regenerate the right masks and read the tape as it was recorded."""
    lm = module_of(handle)
    a = audio.detach().to(F32).contiguous()
    loss, nll, logits, c = lm.forward_loss(input_ids, src_row, a, kmask, label_rows, label_targets, n_label_rows, loss_scale, want_logits,
                                           pos=pos, lora_dropout=(lora_p, lora_seed, lora_offset) if lora_p > 0 else None, seg=seg,
                                           **({"label_smoothing": label_smoothing, "z_loss": z_loss}
                                              if (label_smoothing > 0 or z_loss > 0) else {}))
    return loss.reshape(()), nll, (logits if logits is not None else _empty(a.device)), c["tape"], c["ws"]


@lm_forward_loss.register_fake
def _(audio, trainable, handle, input_ids, src_row, kmask, label_rows, label_targets, n_label_rows, loss_scale, want_logits, pos,
      seg=None, lora_p=0.0, lora_seed=0, lora_offset=0, label_smoothing=0.0, z_loss=0.0):
    lm = module_of(handle)
    B, L = input_ids.shape
    logits = audio.new_empty((B * L, lm.vocab_pad), dtype=BF16) if want_logits else audio.new_empty((0,))
    L_ = _lib.lib()
    n_tape = L_.ta_lm_tape_bytes(C.byref(lm._w), B, L, n_label_rows)
    n_ws = L_.ta_lm_workspace_bytes(C.byref(lm._w), B, L, n_label_rows)
    u8 = lambda n: audio.new_empty((n,), dtype=torch.uint8)
    return audio.new_empty((), dtype=F32), audio.new_empty((max(n_label_rows, 1),), dtype=F32), logits, u8(n_tape), u8(n_ws)


@torch.library.custom_op("ta355::lm_backward", mutates_args=())
def lm_backward(tape: Tensor, ws: Tensor, handle: int, input_ids: Tensor, src_row: Optional[Tensor], kmask: Optional[Tensor],
                label_rows: Optional[Tensor], n_label_rows: int, n_audio_rows: int, want_d_audio: bool,
                pos: Optional[Tensor], seg: Optional[Tensor] = None, lora_p: float = 0.0, lora_seed: int = 0, lora_offset: int = 0,
                res_f32: bool = False, dx_f32: bool = False) -> List[Tensor]:
    """loss.backward() through the LM for d(loss) = 1 -> [d_audio f32 [n_audio_rows, D] (or empty), then one gradient per
    tensor of ``trainable`` (empty tensors when the LM accumulates straight into Parameter.grad: ASRTrainer's mode)].
    ``seg``, ``lora_p``, ``lora_seed``, ``lora_offset``: what the forward was given; ``res_f32``, ``dx_f32``: the stream modes the
    forward recorded ``tape`` in."""
    lm = module_of(handle)
    B, L = input_ids.shape
    ctx = dict(tape=tape, ws=ws, B=B, L=L, src_row=src_row, kmask=kmask, pos=pos, label_rows=label_rows,
               n_label_rows=n_label_rows, ids=input_ids, lora_dropout=(lora_p, lora_seed, lora_offset) if lora_p > 0 else None, seg=seg,
               modes=(res_f32, dx_f32))
    d_audio, _, lg = lm.backward_from_ctx(ctx, n_audio_rows, want_d_audio=want_d_audio)
    dev = tape.device
    out = [d_audio if d_audio is not None else _empty(dev)]
    for g in (lg or []):
        out.append(g if g is not None else _empty(dev))
    return out


@lm_backward.register_fake
def _(tape, ws, handle, input_ids, src_row, kmask, label_rows, n_label_rows, n_audio_rows, want_d_audio, pos, seg=None, lora_p=0.0,
      lora_seed=0, lora_offset=0, res_f32=False, dx_f32=False):
    lm = module_of(handle)
    f = lambda *s: tape.new_empty(s, dtype=F32)
    ps = lm.lora_parameters() or lm.ft_parameters() or []
    return [f(n_audio_rows, lm.config.hidden_size) if want_d_audio else f(0)] + [f(*p.shape) for p in ps]


def _lm_setup(ctx, inputs, output):
    (audio, trainable, handle, input_ids, src_row, kmask, label_rows, _targets, n_label_rows, _scale, _want, pos, seg, *drop) = inputs
    ctx.handle, ctx.n_label_rows, ctx.n_audio, ctx.n_train = handle, n_label_rows, audio.shape[0], len(trainable)
    ctx.drop = tuple(drop[:3])                                # (behind the triple: the loss options, which the backward does not take)
    ctx.module = module_of(handle)
    # this runs on the forward's thread, directly behind the forward: the stream modes its tape was recorded in
    ctx.modes = (ctx.module.res_f32, ctx.module.dx_f32)
    ctx.want_d_audio = audio.requires_grad
    # without this autograd materialises ZERO gradients for the unused outputs on every backward -- the tape alone is
    # 8.9 GB at B = 32 (a 1.35 ms fill per step, measured), the workspace 1.2 GB
    ctx.set_materialize_grads(False)
    optional = (src_row, kmask, label_rows, pos, seg)
    ctx.present = [t is not None for t in optional]
    ctx.save_for_backward(output[3], output[4], input_ids, *[t for t in optional if t is not None])


def _lm_bwd(ctx, g_loss, _g_nll, _g_logits, _g_tape, _g_ws):
    # every input behind (audio, trainable), as many as this call was dispatched with: trailing arguments that equal their defaults
    # are not among them
    rest_none = (None,) * (len(ctx.needs_input_grad) - 2)
    if g_loss is None:                                        # the loss was not used
        return (None, [None] * ctx.n_train) + rest_none
    tape, ws, ids, *rest = ctx.saved_tensors
    it = iter(rest)
    src_row, kmask, label_rows, pos, seg = (next(it) if p else None for p in ctx.present)
    out = torch.ops.ta355.lm_backward(tape, ws, ctx.handle, ids, src_row, kmask, label_rows, ctx.n_label_rows, ctx.n_audio,
                                      ctx.want_d_audio, pos, seg, *ctx.drop, *ctx.modes)
    d_audio = out[0] * g_loss if ctx.want_d_audio else None
    # gradients of the trainable LM tensors: scaled by d(loss) -- except in accumulate_into_grad mode, where the kernels
    # have already added them to Parameter.grad (empty placeholders come back) and d(loss) is 1 by ASRTrainer's contract
    tg = [(g * g_loss if g.numel() else None) for g in out[1:]]
    tg += [None] * (ctx.n_train - len(tg))
    return (d_audio, tg[: ctx.n_train]) + rest_none


lm_forward_loss.register_autograd(_lm_bwd, setup_context=_lm_setup)


OPERATORS = ("logmel", "encoder_forward", "mlp_projector", "mlp_projector_backward", "moe_projector", "moe_projector_backward",
             "lm_forward_loss", "lm_backward", "whisper_encoder_forward", "wave_augment", "wave_augment_chain", "encoder_forward_ragged", "ctc_align",
             "token_scores", "wav2vec2_emissions", "ecapa_embeddings", "spk_affinity", "spk_laplacian_matmul", "spk_panel_gram",
             "spk_panel_update", "spk_panel_combine", "logits_sequence_bias", "logits_step_rules", "logits_warp_ext", "ctc_align_long", "beam_logprobs", "beam_topk",
             "beam_advance", "kv_beam_expand", "kv_beam_reorder", "wave_cut_cost", "cut_plan", "wave_windows", "text_align",
             "wav2vec2_sln_emissions", "vad", "spk_vote", "spk_merge", "spk_words")
