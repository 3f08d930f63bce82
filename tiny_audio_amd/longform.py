"""Long-form transcription: a whole recording -> text, in encoder-sized windows cut at pauses.

The reference stops at one encoder window: ``ASRPipeline.postprocess`` keeps the first chunk's output
(tiny_audio/asr_pipeline.py:243-245).  Here the recording is uploaded once; ``ta_wave_cut_cost_f32`` prices a cut at every 10 ms
position (smoothed short-time power, plus a small share of the recording's mean power so that fewer cuts win among equally quiet
ones), ``ta_cut_plan_f32`` picks the cheapest cuts that keep every window between ``min_window_s`` and ``max_window_s``, and
``ta_wave_windows_f32`` gathers the windows, longest first, into the padded batches that the unchanged feature extractor, encoder,
decode loop and aligner take (csrc/segment.hip; DESIGN.md section 3, "Long-form transcription").  Only the cut table (a few integers
per window) visits the host: the prompts are built from it.  With ``vad=`` (a ``vad.DeviceVAD``) the detector runs on the same
uploaded buffer, its flags are the one further read-back, and a window without speech is neither gathered nor decoded nor aligned.
With ``return_speakers=True`` the same flags feed the diarizer: the windows' embeddings are read from the uploaded buffer, and the
voting, the merging and the words' speakers of all recordings are one launch each (csrc/speaker_post.hip; DESIGN.md section 3,
"Speaker turns").
"""
from __future__ import annotations

from typing import NamedTuple, Sequence

import numpy as np
import torch

from . import _lib
from . import torch_ops  # noqa: F401  (registers torch.ops.ta355.wave_cut_cost / cut_plan / wave_windows)
from .ops import CUT_HOP, SEGMENT_LIMITS

SAMPLE_RATE = 16000
POSITIONS_PER_SECOND = SAMPLE_RATE // CUT_HOP           # 100
MIN_WINDOW_S = 0.1                                      # the smallest min_window_s: at most 104 858 planner steps at the cap
MIN_ALIGN_SAMPLES = 400                                 # one wav2vec2 frame (wav2vec2.MIN_SAMPLES)


class WindowPlan(NamedTuple):
    """One recording's windows: window i is samples [starts[i], starts[i] + lengths[i]) of the recording; ``cut_costs[i]`` is the cost
    at the cut between windows i and i + 1 (a value far above the recording's quiet level is a cut that had to fall inside speech)."""
    starts: list
    lengths: list
    cut_costs: list


def _device():
    return torch.device("cpu") if _lib.DRY_RUN else torch.device("cuda")


def window_positions(max_window_s: float, min_window_s: float) -> tuple[int, int]:
    """-> (min_len, max_len) in positions of 10 ms, checked against the planner's envelope."""
    max_window_s, min_window_s = float(max_window_s), float(min_window_s)
    if not min_window_s >= MIN_WINDOW_S:
        raise ValueError(f"min_window_s must be at least {MIN_WINDOW_S:g} s; got {min_window_s:g} (the planner runs one sequential step per "
                         "min_window_s of audio: a tiny minimum makes a long recording one very long kernel)")
    if 2 * min_window_s > max_window_s:
        raise ValueError(f"2 * min_window_s ({2 * min_window_s:g} s) > max_window_s ({max_window_s:g} s): no plan would exist for some "
                         "lengths; windows need room between the two bounds")
    max_len = int(np.floor(POSITIONS_PER_SECOND * max_window_s + 1e-9))
    min_len = int(np.ceil(POSITIONS_PER_SECOND * min_window_s - 1e-9))
    if max_len > SEGMENT_LIMITS["max_len"]:
        raise ValueError(f"max_window_s={max_window_s:g} is {max_len} positions, beyond the planner's limit of {SEGMENT_LIMITS['max_len']} "
                         f"({SEGMENT_LIMITS['max_len'] / POSITIONS_PER_SECOND:g} s)")
    if min_len < 1 or 2 * min_len > max_len:
        raise ValueError(f"min_window_s={min_window_s:g} and max_window_s={max_window_s:g} leave no whole 10 ms grid between them")
    return min_len, max_len


def upload(waves: Sequence, device=None):
    """A list of 1-D recordings (numpy arrays or tensors, host or device) -> (flat f32 device buffer, offsets int64 [R + 1] on the
    device, the lengths as a host list): the one upload.  Host arrays are checked for non-finite samples on the way."""
    dev = _device() if device is None else torch.device(device)
    if len(waves) == 0:
        raise ValueError("empty audio: no recording was given")
    if len(waves) > SEGMENT_LIMITS["recordings"]:
        raise ValueError(f"{len(waves)} recordings: the segmentation kernels take at most {SEGMENT_LIMITS['recordings']} per call")
    parts, lens = [], []
    for i, w in enumerate(waves):
        t = torch.as_tensor(np.ascontiguousarray(w)) if isinstance(w, np.ndarray) else torch.as_tensor(w)
        if t.dim() != 1:
            raise ValueError(f"recording {i} must be 1-D, got {tuple(t.shape)}")
        n = int(t.shape[0])
        if n == 0:
            raise ValueError(f"empty audio: recording {i} has no samples")
        if -(-n // CUT_HOP) > SEGMENT_LIMITS["positions"]:
            raise ValueError(f"recording {i} has {n} samples ({n / SAMPLE_RATE / 3600:.2f} h), beyond the cap of "
                             f"{SEGMENT_LIMITS['positions'] * CUT_HOP} samples ({SEGMENT_LIMITS['positions'] / POSITIONS_PER_SECOND / 3600:.1f} h)")
        t = t.detach().to(torch.float32)
        if not t.is_cuda and not bool(torch.isfinite(t).all()):
            raise ValueError(f"recording {i} holds non-finite samples")
        parts.append(t.to(dev))
        lens.append(n)
    flat = parts[0].contiguous() if len(parts) == 1 else torch.cat(parts)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return flat, torch.from_numpy(off).to(dev), lens


def plan_uploaded(flat, offsets, lens, min_len: int, max_len: int, smooth_positions: int = 10, cut_penalty: float = 0.05) -> list[WindowPlan]:
    """The two planning operators on an uploaded batch -> a ``WindowPlan`` per recording (one read-back of the cut table)."""
    max_n = max(lens)
    cost = torch.ops.ta355.wave_cut_cost(flat, offsets, max_n, int(smooth_positions), float(cut_penalty))
    cuts, n_seg, dp_T, _back = torch.ops.ta355.cut_plan(cost, offsets, max_n, int(min_len), int(max_len))
    if _lib.DRY_RUN:                                    # nothing was computed: the trivial plan keeps the plumbing going
        return [_plan_from_cuts(list(range(0, -(-n // CUT_HOP), max_len)) + [-(-n // CUT_HOP)], n, None) for n in lens]
    cuts_h, n_seg_h = cuts.cpu().numpy(), n_seg.cpu().tolist()
    # the mean-power term reaches every cost, so one non-finite sample anywhere shows in cost[r, 0] (and in dp[T] of a recording that is cut)
    finite = (torch.isfinite(cost[:, 0]) & torch.isfinite(dp_T)).cpu().tolist()
    plans = []
    for r, n in enumerate(lens):
        if not finite[r]:
            raise ValueError(f"recording {r} holds non-finite samples")
        if n_seg_h[r] < 1:
            raise _lib.Ta355Error(f"ta_cut_plan_f32 found no plan for recording {r} (n_seg {n_seg_h[r]}): non-finite samples?")
        c = cuts_h[r, :n_seg_h[r] + 1].astype(np.int64)
        inner = torch.from_numpy(c[1:-1]).to(cost.device)
        plans.append(_plan_from_cuts(c.tolist(), n, cost[r].index_select(0, inner).cpu().tolist()))
    return plans


def _plan_from_cuts(cuts, n, cut_costs) -> WindowPlan:
    starts = [CUT_HOP * c for c in cuts[:-1]]
    ends = [min(CUT_HOP * c, n) for c in cuts[1:]]
    return WindowPlan(starts, [e - s for s, e in zip(starts, ends)], [0.0] * (len(cuts) - 2) if cut_costs is None else cut_costs)


def plan_windows(waves, max_window_s: float = 28.0, min_window_s: float = 10.0, smooth_positions: int = 10,
                 cut_penalty: float = 0.05) -> list[WindowPlan]:
    """Where to cut every recording of ``waves`` (a list of 1-D 16 kHz arrays or tensors): windows of ``min_window_s`` ..
    ``max_window_s`` seconds (a recording shorter than the minimum is one window) whose cuts cost the least, the cost of a cut being
    the power around it smoothed over ``2 * smooth_positions + 1`` positions of 10 ms plus ``cut_penalty`` x the recording's mean
    power.  The defaults are design choices, not measurements.  -> per recording ``WindowPlan(starts, lengths, cut_costs)``."""
    min_len, max_len = window_positions(max_window_s, min_window_s)
    flat, offsets, lens = upload(waves)
    return plan_uploaded(flat, offsets, lens, min_len, max_len, smooth_positions, cut_penalty)


def group_windows(lengths: Sequence[int], batch_size: int) -> list[list[int]]:
    """Window indices ordered by length, longest first, ties in their given order, ``batch_size`` at a time."""
    order = sorted(range(len(lengths)), key=lambda i: -int(lengths[i]))        # sorted() is stable
    return [order[i:i + batch_size] for i in range(0, len(order), batch_size)]


def left_pad_prompts(prompts: Sequence[torch.Tensor], pad_id: int):
    """1-D prompts of different lengths -> (input_ids [B, L], attention_mask [B, L]) padded on the left, as the collator pads."""
    L = max(int(p.numel()) for p in prompts)
    ids = torch.full((len(prompts), L), int(pad_id), dtype=torch.int64)
    att = torch.zeros((len(prompts), L), dtype=torch.int64)
    for i, p in enumerate(prompts):
        k = int(p.numel())
        ids[i, L - k:] = p.reshape(-1).to(torch.int64)
        att[i, L - k:] = 1
    return ids, att


def join_texts(texts: Sequence[str]) -> str:
    return " ".join(t for t in texts if t)


def transcribe_long(model, audio, sample_rate: int = 16000, *, max_window_s: float = 28.0, min_window_s: float = 10.0, batch_size: int = 32,
                    return_timestamps: bool = False, acoustic_model=None, system_prompt=None, vad=None, min_speech_s: float = 0.0,
                    return_speakers: bool = False, speaker_model=None, num_speakers=None, min_speakers=None, max_speakers=None,
                    cluster_device=None, **generate_kwargs):
    """``ASRModel.transcribe_long`` (documented there)."""
    from .asr_processing import ASRProcessor
    from .eval_text import postprocess_tokens
    if sample_rate != SAMPLE_RATE:
        raise ValueError(f"transcribe_long takes {SAMPLE_RATE} Hz audio, got sample_rate={sample_rate}: resample first")
    if int(batch_size) < 1:
        raise ValueError(f"batch_size must be at least 1; got {batch_size}")
    if return_speakers:
        if acoustic_model is None:
            raise ValueError("return_speakers=True needs acoustic_model=... (a wav2vec2.Wav2Vec2CtcMI355X): speakers are assigned to "
                             "words, and word times come from forced alignment of every window")
        if speaker_model is None or not hasattr(speaker_model, "embed_windows"):
            raise ValueError("return_speakers=True needs speaker_model=... (an ecapa.EcapaTdnnMI355X): the windows' embeddings are read "
                             "from the uploaded buffer by its embed_windows")
        if vad is None:
            raise ValueError("return_speakers=True needs vad=... (a detector with run_uploaded, such as vad.DeviceVAD()): no default "
                             "detector is claimed")
        return_timestamps = True                        # as the reference's pipeline has it (tiny_audio/asr_pipeline.py:100-101)
    if return_timestamps and acoustic_model is None:
        raise ValueError("return_timestamps=True needs acoustic_model=... (a wav2vec2.Wav2Vec2CtcMI355X): word times come from forced "
                         "alignment of every window")
    min_speech_s = float(min_speech_s)
    if not 0.0 <= min_speech_s < float("inf"):
        raise ValueError(f"min_speech_s must be finite and >= 0; got {min_speech_s}")
    if vad is None and min_speech_s > 0.0:
        raise ValueError("min_speech_s needs vad=... (a vad.DeviceVAD): without one no window's speech is known")
    if vad is not None and not hasattr(vad, "run_uploaded"):
        raise ValueError("vad must have run_uploaded(flat, offsets, lens), as a vad.DeviceVAD has: the detector runs on the uploaded buffer")
    enc_cfg = model.audio_tower.config
    frames_cap = 2 * int(getattr(enc_cfg, "max_source_positions", None) or enc_cfg.max_position_embeddings)
    if int(np.floor(POSITIONS_PER_SECOND * float(max_window_s) + 1e-9)) > frames_cap:
        raise ValueError(f"max_window_s={float(max_window_s):g} is beyond the encoder's window of {frames_cap} mel frames "
                         f"({frames_cap / POSITIONS_PER_SECOND:g} s)")
    min_len, max_len = window_positions(max_window_s, min_window_s)
    if model.tokenizer is None:
        raise ValueError("transcribe_long needs a tokenizer: it builds every window's chat prompt and decodes its tokens")
    single = not isinstance(audio, (list, tuple))
    waves = [audio] if single else list(audio)
    flat, offsets, lens = upload(waves, None if _lib.DRY_RUN else model.device_)
    plans = plan_uploaded(flat, offsets, lens, min_len, max_len)
    off_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    win = [(r, i, int(off_h[r]) + s, n) for r, p in enumerate(plans) for i, (s, n) in enumerate(zip(p.starts, p.lengths))]
    speech = None                                       # seconds of speech per window; a window at or below min_speech_s is not decoded
    if vad is not None:                                 # the detector runs once: its flags serve speech_s, the skipping and the diarizer
        from .vad import speech_seconds_from_flags
        _stat, flags_d, n_vad_d = vad.run_uploaded(flat, offsets, lens)
        flags_h = flags_d.cpu().numpy() if isinstance(flags_d, torch.Tensor) else np.asarray(flags_d)
        speech = speech_seconds_from_flags(flags_h, lens, [(w[0], w[2] - int(off_h[w[0]]), w[3]) for w in win])
    keep = list(range(len(win))) if speech is None else [k for k in range(len(win)) if speech[k] > min_speech_s]
    dev = flat.device
    fe = model.feature_extractor
    kw = dict(generate_kwargs)
    eos = kw.get("eos_token_id")
    if eos is None:
        eos = [model.config.eos_token_id, model.config.pad_token_id]
    eos = [int(e) for e in (eos if isinstance(eos, (list, tuple)) else [eos]) if e is not None]
    pad_id = int(kw.get("pad_token_id", model.config.pad_token_id))
    decode = lambda ids: model.tokenizer.decode(ids, skip_special_tokens=True)  # noqa: E731
    sys_prompt = system_prompt or model.system_prompt
    prompt_cache: dict = {}
    texts, words = [""] * len(win), [[] for _ in win]
    for group in group_windows([win[k][3] for k in keep], int(batch_size)):
        group = [keep[j] for j in group]
        g_len = [win[k][3] for k in group]
        start = torch.tensor([win[k][2] for k in group], dtype=torch.int64).to(dev)
        length = torch.tensor(g_len, dtype=torch.int32).to(dev)
        Ls = int(fe.n_samples) if fe.padding == "max_length" else max(g_len)
        wav, wlens = torch.ops.ta355.wave_windows(flat, start, length, Ls)
        feats, mask = fe.extract(wav, wlens)
        counts = model.projector.get_output_length(model._compute_encoder_output_lengths(mask))
        prompts = []
        for c in [int(v) for v in torch.as_tensor(counts).reshape(-1).tolist()]:       # every window its own placeholder count
            if c not in prompt_cache:
                prompt_cache[c] = ASRProcessor.tokenize_messages(model.tokenizer, ASRProcessor.build_messages(c, None, sys_prompt),
                                                                 add_generation_prompt=True)[0]
            prompts.append(prompt_cache[c])
        ids, att = left_pad_prompts(prompts, pad_id)
        out = model.generate(input_ids=ids, input_features=feats, audio_attention_mask=mask, attention_mask=att, **kw)
        seq = out["sequences"] if isinstance(out, dict) else out
        rows = seq.cpu().tolist()
        for j, k in enumerate(group):
            texts[k] = postprocess_tokens(rows[j], eos + [pad_id], decode)
        if return_timestamps:
            from .alignment import ForcedAligner
            live = [j for j, k in enumerate(group) if g_len[j] >= MIN_ALIGN_SAMPLES and texts[k]]
            if live:
                clips = [flat[win[group[j]][2]:win[group[j]][2] + g_len[j]] for j in live]
                got = ForcedAligner.align_audio_batch(clips, [texts[group[j]] for j in live], acoustic_model)
                for j, ws in zip(live, got):
                    k = group[j]
                    t0 = (win[k][2] - int(off_h[win[k][0]])) / SAMPLE_RATE
                    words[k] = [{"word": w["word"], "start": w["start"] + t0, "end": w["end"] + t0} for w in ws]
    results = []
    for r, n in enumerate(lens):                        # back into time order: `win` is in time order per recording
        ks = [k for k, w in enumerate(win) if w[0] == r]
        t0 = int(off_h[r])
        chunks = [{"text": texts[k], "timestamp": ((win[k][2] - t0) / SAMPLE_RATE, (win[k][2] - t0 + win[k][3]) / SAMPLE_RATE)} for k in ks]
        if speech is not None:
            for c, k in zip(chunks, ks):
                c["speech_s"] = speech[k]
        res = {"text": join_texts([texts[k] for k in ks]), "chunks": chunks}
        if return_timestamps:
            res["words"] = [w for k in ks for w in words[k]]
        results.append(res)
    if return_speakers:
        _add_speakers(results, flat, off_h, lens, flags_h, flags_d, n_vad_d, speaker_model, num_speakers, min_speakers, max_speakers,
                      cluster_device)
    return results[0] if single else results


def _add_speakers(results, flat, off_h, lens, flags_h, flags_d, n_vad_d, speaker_model, num_speakers, min_speakers, max_speakers,
                  cluster_device):
    """``"speaker_segments"`` for every result and ``"speaker"`` for every word: the diarizer on the uploaded buffer and the detector's
    flags; one ``embed_windows`` call for all recordings' windows, clustering per recording as ``diarize`` does it, then one ``spk_vote``,
    one ``spk_merge`` and one ``spk_words`` launch for the whole call."""
    from .diarization import LocalSpeakerDiarizer, SpeakerClusterer
    from .ops import vad_frames
    from .vad import segments_from_flags
    dev = flat.device
    decisions = [np.asarray(flags_h[r, :vad_frames(n)]).astype(bool) for r, n in enumerate(lens)]
    embedded = LocalSpeakerDiarizer.extract_embeddings_uploaded(flat, off_h, lens, [segments_from_flags(f) for f in decisions], speaker_model)
    items = []
    for r, (embeddings, windows) in enumerate(embedded):
        labels = []
        if len(embeddings):
            labels = SpeakerClusterer(min_num_spks=min_speakers or 2, max_num_spks=max_speakers or 10, device=cluster_device)(embeddings,
                                                                                                                          num_speakers)
        items.append((windows if len(labels) else [], labels, lens[r] / SAMPLE_RATE, decisions[r].tolist()))
    if not isinstance(flags_d, torch.Tensor):
        flags_d, n_vad_d = torch.from_numpy(np.ascontiguousarray(flags_d, dtype=np.uint8)), torch.as_tensor(n_vad_d, dtype=torch.int32)
    turns = LocalSpeakerDiarizer.postprocess_batch(items, dev, vad_device=(flags_d.to(dev), n_vad_d.to(dev)))
    for res, t in zip(results, turns):
        res["speaker_segments"] = t
    LocalSpeakerDiarizer.assign_speakers_batch([(res["words"], res["speaker_segments"]) for res in results], dev)
