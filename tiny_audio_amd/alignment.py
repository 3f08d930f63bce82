"""Forced alignment for word-level timestamps: the host mirror of the reference's ``tiny_audio/alignment.py``.

Same class, method names, arguments and returns as the reference's ``ForcedAligner``.  What differs is where the work happens: the
reference builds the Viterbi trellis in a Python double loop over frames x tokens (tiny_audio/alignment.py:47-78, about 30 us per
cell) and backtracks on the host (:80-152); here both run in one HIP kernel (``torch.ops.ta355.ctc_align``, csrc/align.hip), for
any number of clips per launch.  The trellis is the reference's bit for bit and the path is identical, ties included
("Forced alignment"; tests/align_ref.py is the definition).

What stays in Python, because it is O(tokens) host work in Python float arithmetic: the tokenisation of the transcript, the uniform
fallback for a clip that cannot be aligned, and the grouping of characters into words (tiny_audio/alignment.py:213-286).

There is no CPU path for the trellis: without a HIP device the methods raise ``Ta355Error``, like the rest of the package.
The wav2vec2 acoustic model is part of this library as an opt-in: ``align(audio, text, acoustic_model=m)`` and
``align_audio_batch(audios, texts, m)`` take a ``wav2vec2.Wav2Vec2CtcMI355X`` and go waveform -> emissions -> trellis on the device
with no host round trip of the emissions.  ``align(..., emission=...)`` and ``align_batch`` take emissions computed elsewhere;
with neither, ``align`` runs torchaudio's bundle through PyTorch as the reference does, and needs torchaudio installed.

Those calls stop at 2048 tokens and 32768 frames per clip (one workgroup per clip).  A whole recording against its whole transcript
-- the call the reference's pipeline makes (tiny_audio/asr_pipeline.py:117-131) -- goes through the explicit long form,
``align_long`` / ``align_long_batch`` (``torch.ops.ta355.ctc_align_long``, csrc/align_long.hip: the same trellis as a tiled wavefront
of launches, the same bytes), with ``Wav2Vec2CtcMI355X.emissions_long`` for the emissions.  The short calls never dispatch to it.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import _lib
from . import torch_ops  # noqa: F401  (registers torch.ops.ta355.ctc_align)
from .ops import ALIGN_LIMITS, ALIGN_LONG_LIMITS

# torchaudio.pipelines.WAV2VEC2_ASR_BASE_960H.get_labels(): blank, the word separator, then the letters by frequency
LABELS = ("-", "|", "E", "T", "A", "O", "N", "I", "H", "S", "R", "D", "L", "U", "M", "W", "C", "F", "G", "Y", "P", "B", "V", "K", "'",
          "X", "J", "Q", "Z")
FRAME_STRIDE = 320          # samples per emission frame of wav2vec2 (20 ms at 16 kHz)
SAMPLE_RATE = 16000


def _device() -> torch.device:
    if torch.cuda.is_available():
        return torch.device("cuda")
    if _lib.DRY_RUN:                                    # test instrumentation only (see _lib.DRY_RUN)
        return torch.device("cpu")
    raise _lib.Ta355Error("forced alignment needs a HIP device: there is no CPU path for the trellis")


def _torchaudio():
    try:
        import torchaudio
    except ImportError as e:
        raise ImportError("torchaudio is not installed: ForcedAligner.align needs it to compute wav2vec2 emissions; "
                          "pass emission=... (or use align_batch) to align emissions computed elsewhere") from e
    return torchaudio


def _check_clip(emission: torch.Tensor, tokens: Sequence[int], blank_id: int) -> None:
    if emission.dim() != 2:
        raise ValueError(f"emission must be [frames, classes], got {tuple(emission.shape)}")
    T, C = emission.shape
    if not 1 <= C <= ALIGN_LIMITS["classes"]:
        raise ValueError(f"{C} classes: the alignment kernel takes 1 .. {ALIGN_LIMITS['classes']} classes")
    if T > ALIGN_LIMITS["frames"]:
        raise ValueError(f"{T} frames: the alignment kernel takes at most {ALIGN_LIMITS['frames']} frames per clip")
    if len(tokens) > ALIGN_LIMITS["tokens"]:
        raise ValueError(f"{len(tokens)} tokens: the alignment kernel takes at most {ALIGN_LIMITS['tokens']} tokens per clip")
    if not 0 <= int(blank_id) < C:
        raise ValueError(f"blank_id {blank_id} is outside [0, {C})")
    for i, tk in enumerate(tokens):
        if not 0 <= int(tk) < C:
            raise ValueError(f"token {i} has id {tk}, outside [0, {C})")


def _launch(emissions: Sequence[torch.Tensor], tokens: Sequence[Sequence[int]], blank_id: int, want_trellis: bool = False):
    """One launch for all clips -> (frames: list of int lists, score: list of floats, status: list of ints, trellises or None),
    everything back on the host."""
    N = len(emissions)
    if N != len(tokens):
        raise ValueError(f"{N} emission matrices but {len(tokens)} token sequences")
    if N > ALIGN_LIMITS["clips"]:
        raise ValueError(f"{N} clips: the alignment kernel takes at most {ALIGN_LIMITS['clips']} clips per launch")
    if N == 0:
        return [], [], [], ([] if want_trellis else None)
    for e, tk in zip(emissions, tokens):
        _check_clip(e, tk, blank_id)
    C = emissions[0].shape[1]
    if any(e.shape[1] != C for e in emissions):
        raise ValueError("every clip of a batch must have the same number of classes")
    dev = _device()
    em = [e.detach().to(device=dev, dtype=torch.float32) for e in emissions]
    em = em[0].contiguous() if N == 1 else torch.cat(em, dim=0)
    return _launch_flat(em, [e.shape[0] for e in emissions], tokens, blank_id, want_trellis)


def _launch_flat(em: torch.Tensor, Ts: Sequence[int], tokens: Sequence[Sequence[int]], blank_id: int, want_trellis: bool = False):
    """``_launch`` on emissions that already sit on the device as one f32 [sum T_n, C] tensor, clip n owning ``Ts[n]`` rows."""
    N, dev = len(Ts), em.device
    Js = [len(tk) for tk in tokens]
    cu_f, cu_t = np.zeros(N + 1, np.int32), np.zeros(N + 1, np.int32)
    cu_f[1:], cu_t[1:] = np.cumsum(Ts), np.cumsum(Js)
    flat = np.asarray([int(x) for tk in tokens for x in tk], np.int32)
    tr_off, tr_numel = None, 0
    if want_trellis:
        sizes = np.asarray([(t + 1) * (j + 1) for t, j in zip(Ts, Js)], np.int64)
        off = np.concatenate([[0], np.cumsum(sizes)])
        tr_off, tr_numel = torch.from_numpy(off[:-1].copy()).to(dev), int(off[-1])
    frames, score, status, trellis = torch.ops.ta355.ctc_align(
        em, torch.from_numpy(cu_f).to(dev), torch.from_numpy(flat).to(dev), torch.from_numpy(cu_t).to(dev), int(blank_id),
        max(Ts), max(Js), tr_off, tr_numel)
    frames, status, score = frames.cpu().tolist(), status.cpu().tolist(), score.cpu().tolist()
    if any(s not in (0, 1) for s in status) and not _lib.DRY_RUN:
        raise _lib.Ta355Error(f"ta_ctc_align_f32 refused a clip (status {status})")
    per_clip = [frames[cu_t[n]:cu_t[n + 1]] for n in range(N)]
    trs = None
    if want_trellis:
        tc = trellis.cpu()
        trs = [tc[off[n]:off[n + 1]].reshape(Ts[n] + 1, Js[n] + 1).clone() for n in range(N)]
    return per_clip, score, status, trs


def _check_clip_long(emission: torch.Tensor, tokens: Sequence[int], blank_id: int) -> None:
    """``_check_clip`` against the long form's envelope (``ops.ALIGN_LONG_LIMITS``)."""
    if emission.dim() != 2:
        raise ValueError(f"emission must be [frames, classes], got {tuple(emission.shape)}")
    T, C = emission.shape
    if not 1 <= C <= ALIGN_LONG_LIMITS["classes"]:
        raise ValueError(f"{C} classes: the long alignment kernel takes 1 .. {ALIGN_LONG_LIMITS['classes']} classes")
    if T > ALIGN_LONG_LIMITS["frames"]:
        raise ValueError(f"{T} frames: the long alignment kernel takes at most {ALIGN_LONG_LIMITS['frames']} frames per clip")
    if len(tokens) > ALIGN_LONG_LIMITS["tokens"]:
        raise ValueError(f"{len(tokens)} tokens: the long alignment kernel takes at most {ALIGN_LONG_LIMITS['tokens']} tokens per clip")
    if not 0 <= int(blank_id) < C:
        raise ValueError(f"blank_id {blank_id} is outside [0, {C})")
    tk = np.asarray(tokens, np.int64).reshape(-1)
    bad = np.flatnonzero((tk < 0) | (tk >= C))
    if bad.size:
        raise ValueError(f"token {int(bad[0])} has id {int(tk[bad[0]])}, outside [0, {C})")


def _check_tile(col_block: int, frame_block: int) -> None:
    if col_block < 0 or col_block % 64 or col_block > ALIGN_LONG_LIMITS["col_block"]:
        raise ValueError(f"col_block {col_block}: a multiple of 64 up to {ALIGN_LONG_LIMITS['col_block']}, or 0 for the default")
    if frame_block < 0:
        raise ValueError(f"frame_block {frame_block}: at least 1, or 0 for the default")


def _launch_long(emissions: Sequence[torch.Tensor], tokens: Sequence[Sequence[int]], blank_id: int, col_block: int = 0,
                 frame_block: int = 0):
    """``_launch`` through ``torch.ops.ta355.ctc_align_long`` -> (frames per clip, score, status) on the host."""
    N = len(emissions)
    if N != len(tokens):
        raise ValueError(f"{N} emission matrices but {len(tokens)} token sequences")
    if N > ALIGN_LONG_LIMITS["clips"]:
        raise ValueError(f"{N} clips: the long alignment kernel takes at most {ALIGN_LONG_LIMITS['clips']} clips per call")
    _check_tile(int(col_block), int(frame_block))
    if N == 0:
        return [], [], []
    for e, tk in zip(emissions, tokens):
        _check_clip_long(e, tk, blank_id)
    C = emissions[0].shape[1]
    if any(e.shape[1] != C for e in emissions):
        raise ValueError("every clip of a batch must have the same number of classes")
    dev = _device()
    em = [e.detach().to(device=dev, dtype=torch.float32) for e in emissions]
    em = em[0].contiguous() if N == 1 else torch.cat(em, dim=0)
    Ts, Js = [e.shape[0] for e in emissions], [len(tk) for tk in tokens]
    cu_f, cu_t = np.zeros(N + 1, np.int32), np.zeros(N + 1, np.int32)
    cu_f[1:], cu_t[1:] = np.cumsum(Ts), np.cumsum(Js)
    flat = np.concatenate([np.asarray(tk, np.int32).reshape(-1) for tk in tokens])
    frames, score, status, _ = torch.ops.ta355.ctc_align_long(
        em, torch.from_numpy(cu_f).to(dev), torch.from_numpy(flat).to(dev), torch.from_numpy(cu_t).to(dev), int(blank_id),
        max(Ts), max(Js), int(col_block), int(frame_block), None, 0, None)
    frames, status, score = frames.cpu().tolist(), status.cpu().tolist(), score.cpu().tolist()
    if any(s not in (0, 1) for s in status) and not _lib.DRY_RUN:
        raise _lib.Ta355Error(f"ta_ctc_align_long_f32 refused a clip (status {status})")
    return [frames[cu_t[n]:cu_t[n + 1]] for n in range(N)], score, status


def _uniform_spans(tokens: Sequence[int], num_frames: int) -> list[tuple[int, float, float]]:
    """The reference's fallback for a clip that cannot be aligned (tiny_audio/alignment.py:101-107), in Python floats."""
    frames_per_token = num_frames / len(tokens)
    return [(tokens[i], i * frames_per_token, (i + 1) * frames_per_token) for i in range(len(tokens))]


def _spans(tokens: Sequence[int], frames: Sequence[int], failed: bool, num_frames: int) -> list[tuple[int, float, float]]:
    """Token spans from the kernel's outputs: every token of an aligned clip sits on exactly one frame f and spans (f, f + 1)."""
    if not tokens:
        return []
    if failed:
        return _uniform_spans(tokens, num_frames)
    return [(tokens[i], float(frames[i]), float(frames[i]) + 1.0) for i in range(len(tokens))]


def _tokenize(text: str, dictionary: dict, as_written: bool = False) -> list[int]:
    """Characters -> class ids; a character the dictionary lacks is dropped, a space becomes the word separator.  ``as_written``
    (an acoustic model's own vocabulary, ``Wav2Vec2CtcMI355X.set_vocab``): a character is looked up as written, then upper-cased,
    then lower-cased -- HF vocabularies are lower-case, ``LABELS`` is upper-case -- instead of the whole text being upper-cased."""
    tokens = []
    if as_written:
        for char in text:
            for form in (char, char.upper(), char.lower()):
                if form in dictionary:
                    tokens.append(dictionary[form])
                    break
            else:
                if char == " ":
                    tokens.append(dictionary.get("|", dictionary.get(" ", 0)))
        return tokens
    for char in text.upper():
        if char in dictionary:
            tokens.append(dictionary[char])
        elif char == " ":
            tokens.append(dictionary.get("|", dictionary.get(" ", 0)))
    return tokens


def _vocab_of(acoustic_model, default_dictionary: dict, blank_id):
    """-> (dictionary, blank id, as_written): the acoustic model's own vocabulary when it carries one (``set_vocab``), else
    ``default_dictionary`` and blank 0 as ever.  An explicit ``blank_id`` wins."""
    d = getattr(acoustic_model, "dictionary", None)
    if d is None:
        return default_dictionary, (0 if blank_id is None else int(blank_id)), False
    return d, (int(acoustic_model.blank_id) if blank_id is None else int(blank_id)), True


def _group_words(text: str, spans, dictionary: dict, frame_duration: float, start_offset: float, end_offset: float) -> list[dict]:
    """Characters into words at the separator (tiny_audio/alignment.py:238-286).  The reference's quirks are kept: a separator with
    no open word is skipped, and the labels come from ``text.split()`` in order, so a word with no alignable character shifts the
    labels of the words after it."""
    words = text.split()
    out = []
    start = end = None
    word_idx = 0
    separator_id = dictionary.get("|", dictionary.get(" ", 0))

    def emit():
        out.append({"word": words[word_idx], "start": max(0.0, start * frame_duration - start_offset),
                    "end": max(0.0, end * frame_duration - end_offset)})

    for token_id, start_frame, end_frame in spans:
        if token_id == separator_id:
            if start is not None and end is not None and word_idx < len(words):
                emit()
                word_idx += 1
            start = end = None
        else:
            if start is None:
                start = start_frame
            end = end_frame
    if start is not None and end is not None and word_idx < len(words):
        emit()
    return out


class ForcedAligner:
    """Forced aligner for word-level timestamps from wav2vec2 CTC emissions; the trellis and its backtrack run on the device."""

    _bundle = None
    _model = None
    _labels = None
    _dictionary = None

    # Offset compensation for Wav2Vec2-BASE systematic bias (in seconds), the reference's calibration
    START_OFFSET = 0.06  # subtracted from start times
    END_OFFSET = -0.03  # subtracted from end times (shifts them later)

    @classmethod
    def get_instance(cls, device: str = "cuda"):
        """-> (model, labels, dictionary) of torchaudio's WAV2VEC2_ASR_BASE_960H bundle, loaded once."""
        if cls._model is None:
            torchaudio = _torchaudio()
            cls._bundle = torchaudio.pipelines.WAV2VEC2_ASR_BASE_960H
            cls._model = cls._bundle.get_model().to(device)
            cls._model.eval()
            cls._labels = cls._bundle.get_labels()
            cls._dictionary = {c: i for i, c in enumerate(cls._labels)}
        return cls._model, cls._labels, cls._dictionary

    @classmethod
    def _dict(cls) -> dict:
        return cls._dictionary if cls._dictionary is not None else {c: i for i, c in enumerate(LABELS)}

    @staticmethod
    def _get_trellis(emission: torch.Tensor, tokens: list[int], blank_id: int = 0) -> torch.Tensor:
        """-> the CPU float32 trellis [num_frames + 1, num_tokens + 1]: trellis[t, j] is the log probability of the best path
        that aligns the first j tokens to the first t frames.  ``emission``: log-softmax [num_frames, num_classes], any device."""
        return _launch([emission], [list(tokens)], blank_id, want_trellis=True)[3][0]

    @staticmethod
    def _backtrack(trellis: torch.Tensor, emission: torch.Tensor, tokens: list[int], blank_id: int = 0) -> list[tuple[int, float, float]]:
        """-> [(token_id, start_frame, end_frame)] per token.  ``trellis`` MUST be what ``_get_trellis`` returns for the same
        ``emission``, ``tokens`` and ``blank_id``: only trellis[T, J] is read from it (the reference's test for a failed alignment);
        the path itself is derived on the device from ``emission`` and ``tokens``, where the forward pass records every decision."""
        num_frames, num_tokens = emission.size(0), len(tokens)
        if num_tokens == 0:
            return []
        if trellis[num_frames, num_tokens] == -float("inf"):
            return _uniform_spans(list(tokens), num_frames)
        frames, _, status, _ = _launch([emission], [list(tokens)], blank_id)
        return _spans(list(tokens), frames[0], status[0] == 1, num_frames)

    @classmethod
    def _emission_of(cls, audio, sample_rate: int) -> tuple[torch.Tensor, dict, float]:
        """The reference's acoustic front end (tiny_audio/alignment.py:182-211): torchaudio's wav2vec2 through PyTorch."""
        torchaudio = _torchaudio()
        dev = str(_device())
        model, _labels, dictionary = cls.get_instance(dev)
        waveform = torch.from_numpy(audio.copy()).float() if isinstance(audio, np.ndarray) else audio.clone().float()
        if waveform.dim() == 1:
            waveform = waveform.unsqueeze(0)
        if sample_rate != cls._bundle.sample_rate:
            waveform = torchaudio.functional.resample(waveform, sample_rate, cls._bundle.sample_rate)
        with torch.inference_mode():
            emissions, _ = model(waveform.to(dev))
            emissions = torch.log_softmax(emissions, dim=-1)
        return emissions[0], dictionary, FRAME_STRIDE / cls._bundle.sample_rate

    @classmethod
    def align(cls, audio, text: str, sample_rate: int = 16000, _language: str = "eng", _batch_size: int = 16, *,
              emission: torch.Tensor | None = None, log_softmax: bool = False, acoustic_model=None) -> list[dict]:
        """Align transcript to audio -> [{'word', 'start', 'end'}] in seconds.

        ``emission`` [num_frames, num_classes]: the acoustic model's log-probabilities (or its logits, with ``log_softmax=True``)
        over ``LABELS``; with it ``audio`` is not read and no acoustic model is needed.
        ``acoustic_model``: a ``wav2vec2.Wav2Vec2CtcMI355X`` that computes the emissions of ``audio`` (16 kHz: resampling stays the
        caller's job) on the device instead of torchaudio's bundle; ignored when ``emission`` is given."""
        if emission is None and acoustic_model is not None:
            if sample_rate != SAMPLE_RATE:
                raise ValueError(f"acoustic_model takes {SAMPLE_RATE} Hz audio, got sample_rate={sample_rate}: resample first")
            return cls.align_audio_batch([audio], [text], acoustic_model)[0]
        if emission is None:
            emission, dictionary, frame_duration = cls._emission_of(audio, sample_rate)
        else:
            dictionary, frame_duration = cls._dict(), FRAME_STRIDE / SAMPLE_RATE
        return cls.align_batch([emission], [text], log_softmax=log_softmax, _dictionary=dictionary, _frame_duration=frame_duration)[0]

    @classmethod
    def align_audio_batch(cls, audios: Sequence, texts: Sequence[str], acoustic_model, *, blank_id: int | None = None) -> list[list[dict]]:
        """Waveforms -> words for a batch: ``acoustic_model`` (``wav2vec2.Wav2Vec2CtcMI355X``) turns the 16 kHz clips ``audios``
        (1-D arrays or tensors of any lengths >= 400 samples) into emissions in ONE call, and the trellis kernel reads them where
        they are: the emissions never visit the host.  Same words as ``align`` per clip.  A model that carries a vocabulary
        (``set_vocab``) is tokenised against it with its own blank id; otherwise ``LABELS`` and blank 0 (``blank_id`` overrides)."""
        if len(audios) != len(texts):
            raise ValueError(f"{len(audios)} clips but {len(texts)} texts")
        dictionary, blank_id, as_written = _vocab_of(acoustic_model, cls._dict(), blank_id)
        out: list[list[dict]] = [[] for _ in texts]
        if not len(texts):
            return out
        if len(texts) > ALIGN_LIMITS["clips"]:
            raise ValueError(f"{len(texts)} clips: the alignment kernel takes at most {ALIGN_LIMITS['clips']} clips per launch")
        tokens = [_tokenize(t, dictionary, as_written) for t in texts]
        em, Ts = acoustic_model(list(audios))
        for n, tk in enumerate(tokens):
            _check_clip(em[:Ts[n]], tk, blank_id)
        if not any(tokens):
            return out
        frames, _, status, _ = _launch_flat(em, Ts, tokens, blank_id)
        for n, tk in enumerate(tokens):
            if tk:
                spans = _spans(tk, frames[n], status[n] == 1, Ts[n])
                out[n] = _group_words(texts[n], spans, dictionary, FRAME_STRIDE / SAMPLE_RATE, cls.START_OFFSET, cls.END_OFFSET)
        return out

    @classmethod
    def align_batch(cls, emissions: Sequence[torch.Tensor], texts: Sequence[str], *, log_softmax: bool = False, blank_id: int = 0,
                    _dictionary: dict | None = None, _frame_duration: float = FRAME_STRIDE / SAMPLE_RATE) -> list[list[dict]]:
        """``align`` for a batch in ONE launch: ``emissions[n]`` [T_n, num_classes] against ``texts[n]`` -> a word list per clip."""
        if len(emissions) != len(texts):
            raise ValueError(f"{len(emissions)} emission matrices but {len(texts)} texts")
        dictionary = _dictionary if _dictionary is not None else cls._dict()
        tokens = [_tokenize(t, dictionary) for t in texts]
        live = [n for n, tk in enumerate(tokens) if tk]
        out: list[list[dict]] = [[] for _ in texts]
        if not live:
            return out
        em = [emissions[n] for n in live]
        if log_softmax:
            em = [torch.log_softmax(e.to(_device()).float(), dim=-1) for e in em]
        frames, _, status, _ = _launch(em, [tokens[n] for n in live], blank_id)
        for i, n in enumerate(live):
            spans = _spans(tokens[n], frames[i], status[i] == 1, em[i].shape[0])
            out[n] = _group_words(texts[n], spans, dictionary, _frame_duration, cls.START_OFFSET, cls.END_OFFSET)
        return out

    # ------------------------------------------------------------------ long form
    @classmethod
    def align_long_batch(cls, emissions: Sequence[torch.Tensor], texts: Sequence[str], *, log_softmax: bool = False, blank_id: int | None = None,
                         col_block: int = 0, frame_block: int = 0, acoustic_model=None) -> list[list[dict]]:
        """``align_batch`` beyond its envelope: up to 64 clips of up to 1 048 576 frames against up to 262 144 characters each, in one
        call of ``torch.ops.ta355.ctc_align_long``.  Same word lists (the reference's two quirks of ``_group_words`` included);
        ``col_block`` x ``frame_block`` is the trellis tile (0 = the default) and does not change the result.  ``acoustic_model``: the
        model the emissions came from; only its vocabulary and blank id are read (``set_vocab``), it is not run."""
        if len(emissions) != len(texts):
            raise ValueError(f"{len(emissions)} emission matrices but {len(texts)} texts")
        _check_tile(int(col_block), int(frame_block))
        dictionary, blank_id, as_written = _vocab_of(acoustic_model, cls._dict(), blank_id)
        tokens = [_tokenize(t, dictionary, as_written) for t in texts]
        live = [n for n, tk in enumerate(tokens) if tk]
        out: list[list[dict]] = [[] for _ in texts]
        if not live:
            return out
        em = [emissions[n] for n in live]
        if log_softmax:
            em = [torch.log_softmax(e.to(_device()).float(), dim=-1) for e in em]
        frames, _, status = _launch_long(em, [tokens[n] for n in live], blank_id, col_block, frame_block)
        for i, n in enumerate(live):
            spans = _spans(tokens[n], frames[i], status[i] == 1, em[i].shape[0])
            out[n] = _group_words(texts[n], spans, dictionary, FRAME_STRIDE / SAMPLE_RATE, cls.START_OFFSET, cls.END_OFFSET)
        return out

    @classmethod
    def align_long(cls, audio, text: str, sample_rate: int = 16000, *, emission: torch.Tensor | None = None, acoustic_model=None,
                   window_s: float = 30.0, context_s: float = 2.0) -> list[dict]:
        """``align`` for a whole recording against its whole transcript -> [{'word', 'start', 'end'}] in seconds.

        ``emission`` [num_frames, num_classes]: log-probabilities over ``LABELS`` computed elsewhere (``audio`` is then not read).
        ``acoustic_model``: a ``wav2vec2.Wav2Vec2CtcMI355X``; the emissions of the 16 kHz ``audio`` come from its ``emissions_long``
        in windows of ``window_s`` seconds with ``context_s`` seconds of context on both sides, and stay on the device.  One of the
        two is required: torchaudio's bundle is not run over a whole recording."""
        if emission is None:
            if acoustic_model is None:
                raise ValueError("align_long needs emission=... or acoustic_model=...")
            if sample_rate != SAMPLE_RATE:
                raise ValueError(f"acoustic_model takes {SAMPLE_RATE} Hz audio, got sample_rate={sample_rate}: resample first")
            dictionary, _, as_written = _vocab_of(acoustic_model, cls._dict(), None)
            n_tokens = len(_tokenize(text, dictionary, as_written))
            if n_tokens > ALIGN_LONG_LIMITS["tokens"]:                                  # before the acoustic model runs for nothing
                raise ValueError(f"{n_tokens} tokens: the long alignment kernel takes at most {ALIGN_LONG_LIMITS['tokens']} tokens "
                                 "per clip")
            emission = acoustic_model.emissions_long(audio, window_s=window_s, context_s=context_s)
            return cls.align_long_batch([emission], [text], acoustic_model=acoustic_model)[0]
        return cls.align_long_batch([emission], [text])[0]
