"""Speaker diarization: who spoke when.  Speech segments from a VAD (TEN-VAD, or ``vad.DeviceVAD`` on the device) -> ECAPA-TDNN
embeddings of sliding windows -> spectral clustering -> frame-level voting -> merged speaker segments.

This is the counterpart of the reference's ``tiny_audio/diarization.py`` (the module behind ``ASRPipeline(return_speakers=True)``,
tiny_audio/asr_pipeline.py:133-152): the same class names, class constants, arguments, return values and quirks, restated.  What
differs is the hot path.  The reference pushes every 0.75 s window through SpeechBrain's ``encode_batch`` one window per call
(tiny_audio/diarization.py:490-502); with ``speaker_model=`` (an ``EcapaTdnnMI355X``) every window of every segment goes through ONE
``embed_windows`` call on the device -- the audio is uploaded once and the windows are cut and reflect-padded by the feature kernel.
Voting and merging behind the ``[N, 192]`` embeddings are O(N) host arithmetic and stay in numpy, scipy and scikit-learn exactly as the
reference has them.  Spectral clustering is not: ``SpectralCluster`` restates the reference's dense float64 affinity, Laplacian and full
``scipy.linalg.eigh`` -- O(N^2) memory and O(N^3) time, seconds at N = 4 000 windows (10 minutes of speech) and tens of minutes at an
hour.  It stays the default; ``cluster_device=`` (``SpeakerClusterer(device=...)``) moves the affinity, the Laplacian and the few
eigenpairs that are read onto the device (``tiny_audio_amd/spectral.py``) and leaves the eigengap rule, k-means and merging here.

Third-party pieces that are not rebuilt: TEN-VAD itself (``ten_vad``, a compiled library and the default; ``vad=DeviceVAD()`` -- the
model-free detector of ``tiny_audio_amd/vad.py``, whose constants are not validated on real speech -- or ``speech_frames=`` do without
it), file reading and resampling (``librosa``), and -- only without ``speaker_model`` -- SpeechBrain.  Each raises ``ImportError``
where it is needed and absent.  With ``vad=DeviceVAD()``, ``speaker_model=`` and ``cluster_device=`` a waveform array is diarized with
nothing third-party on the hot path.
"""
from __future__ import annotations

import warnings

import numpy as np

VAD_HOP = 256                                   # samples per TEN-VAD frame


class SpectralCluster:
    """Spectral clustering on the unnormalised Laplacian of a pruned cosine-affinity matrix; the number of speakers is where the
    gap between consecutive eigenvalues is widest (tiny_audio/diarization.py:27-115)."""

    def __init__(self, min_num_spks: int = 1, max_num_spks: int = 15, pval: float = 0.06):
        self.min_num_spks, self.max_num_spks, self.pval = min_num_spks, max_num_spks, pval

    def __call__(self, embeddings: np.ndarray, oracle_num: int | None = None) -> np.ndarray:
        """embeddings [N, D] -> labels [N]; ``oracle_num`` fixes the number of clusters."""
        pruned = self.p_pruning(self.get_sim_mat(embeddings))
        lap = self.get_laplacian(0.5 * (pruned + pruned.T))
        emb, k = self.get_spec_embs(lap, oracle_num)
        return self.cluster_embs(emb, k)

    def get_sim_mat(self, embeddings: np.ndarray) -> np.ndarray:
        import sklearn.metrics.pairwise
        return sklearn.metrics.pairwise.cosine_similarity(embeddings, embeddings)

    def p_pruning(self, affinity: np.ndarray) -> np.ndarray:
        """Keeps the ``max(pval, 6 / n)`` largest entries of every row and zeroes the rest -- IN PLACE, as the reference does."""
        n = affinity.shape[0]
        keep = max(1, int(max(self.pval, 6.0 / n) * n))
        top = np.argpartition(affinity, -keep, axis=1)[:, -keep:]
        kept = np.zeros_like(affinity, dtype=bool)
        np.put_along_axis(kept, top, True, axis=1)
        affinity[~kept] = 0
        return affinity

    def get_laplacian(self, sim_mat: np.ndarray) -> np.ndarray:
        """Unnormalised graph Laplacian; the diagonal of ``sim_mat`` is zeroed in place first."""
        from scipy.sparse.csgraph import laplacian
        np.fill_diagonal(sim_mat, 0)
        return laplacian(sim_mat, normed=False)

    def get_spec_embs(self, laplacian: np.ndarray, k_oracle: int | None = None):
        import scipy.linalg
        lambdas, vecs = scipy.linalg.eigh(laplacian)
        if k_oracle is not None:
            k = k_oracle
        else:
            k = np.argmax(self.get_eigen_gaps(lambdas[self.min_num_spks - 1:self.max_num_spks + 1])) + self.min_num_spks
        return vecs[:, :k], k

    def cluster_embs(self, emb: np.ndarray, k: int) -> np.ndarray:
        from sklearn.cluster._kmeans import k_means
        return k_means(emb, k, n_init=10)[1]

    def get_eigen_gaps(self, eig_vals: np.ndarray) -> np.ndarray:
        return np.diff(eig_vals)


class SpeakerClusterer:
    """Spectral clustering of speaker embeddings, then -- without an oracle count -- speakers whose centroids are closer than
    ``merge_thr`` in cosine are merged (tiny_audio/diarization.py:118-218)."""

    def __init__(self, min_num_spks: int = 2, max_num_spks: int = 10, merge_thr: float = 0.90, device=None):
        """device: None -- the host ``SpectralCluster``, as in the reference; a torch device -- ``spectral.DeviceSpectralCluster`` on
        it (which still hands small or undecided inputs to the host class; see its ``last_info``)."""
        self.min_num_spks, self.max_num_spks, self.merge_thr, self.device = min_num_spks, max_num_spks, merge_thr, device
        self._spectral_cluster: SpectralCluster | None = None

    def _get_spectral_cluster(self) -> SpectralCluster:
        if self._spectral_cluster is None:
            if self.device is None:
                self._spectral_cluster = SpectralCluster(min_num_spks=self.min_num_spks, max_num_spks=self.max_num_spks)
            else:
                from .spectral import DeviceSpectralCluster
                self._spectral_cluster = DeviceSpectralCluster(min_num_spks=self.min_num_spks, max_num_spks=self.max_num_spks,
                                                               device=self.device)
        return self._spectral_cluster

    def __call__(self, embeddings: np.ndarray, num_speakers: int | None = None) -> np.ndarray:
        """embeddings [N, D] -> labels [N], numbered 0 .. in order of first appearance of their sorted values.  Fewer than six rows
        are one speaker."""
        if len(embeddings.shape) != 2:
            raise ValueError(f"Expected 2D array, got shape {embeddings.shape}")
        n = embeddings.shape[0]
        if n == 0:
            return np.array([], dtype=int)
        if n == 1:
            return np.array([0], dtype=int)
        if n < 6:
            return np.zeros(n, dtype=int)
        from sklearn.preprocessing import normalize
        embeddings = normalize(np.nan_to_num(embeddings, nan=0.0, posinf=0.0, neginf=0.0))
        spectral = self._get_spectral_cluster()
        if num_speakers is not None:                     # the oracle count narrows the shared clusterer for this call only
            spectral.min_num_spks = spectral.max_num_spks = num_speakers
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore", category=RuntimeWarning)
            labels = spectral(embeddings, oracle_num=num_speakers)
        if num_speakers is not None:
            spectral.min_num_spks, spectral.max_num_spks = self.min_num_spks, self.max_num_spks
        else:
            labels = self._merge_by_cos(labels, embeddings, self.merge_thr)
        return np.unique(labels, return_inverse=True)[1]

    def _merge_by_cos(self, labels: np.ndarray, embs: np.ndarray, cos_thr: float) -> np.ndarray:
        """Average-linkage clustering of the normalised centroids at cosine distance ``1 - cos_thr``."""
        from scipy.cluster.hierarchy import fcluster, linkage
        from scipy.spatial.distance import pdist
        from sklearn.preprocessing import normalize
        speakers = np.unique(labels)
        if len(speakers) <= 1:
            return labels
        centroids = normalize(np.array([embs[labels == s].mean(0) for s in speakers]))
        merged = fcluster(linkage(pdist(centroids, metric="cosine"), method="average"), t=1.0 - cos_thr, criterion="distance") - 1
        to = dict(zip(speakers, merged))
        return np.array([to[s] for s in labels])


def _span(start_frame: int, end_frame: int, frame_duration: float, sample_rate: int) -> dict:
    start, end = start_frame * frame_duration, end_frame * frame_duration
    return {"start": start, "end": end, "start_sample": int(start * sample_rate), "end_sample": int(end * sample_rate)}


class LocalSpeakerDiarizer:
    """TEN-VAD + ECAPA-TDNN + spectral clustering (tiny_audio/diarization.py:221-681).

    1. the VAD's per-256-sample decisions become speech segments (gaps up to VAD_MAX_GAP bridged, segments under VAD_MIN_DURATION
       dropped, the rest padded by VAD_PAD_ONSET / VAD_PAD_OFFSET);
    2. every segment is cut into WINDOW_SIZE windows STEP_SIZE apart, plus one flush with its end when more than
       TAIL_COVERAGE_RATIO of a window would be left over;
    3. one embedding per window, clustered by ``SpeakerClusterer``;
    4. every VOTING_RATE frame goes to the speaker most windows over it voted for -- silence where the VAD heard none;
    5. segments under MIN_SEGMENT_DURATION are absorbed or dropped, same-speaker neighbours closer than SAME_SPEAKER_GAP joined.
    """

    _ten_vad_model = None
    _ecapa_model = None
    _device = None

    WINDOW_SIZE = 0.75
    STEP_SIZE = 0.15
    TAIL_COVERAGE_RATIO = 0.1
    VAD_THRESHOLD = 0.25
    VAD_MIN_DURATION = 0.05
    VAD_MAX_GAP = 0.50
    VAD_PAD_ONSET = 0.05
    VAD_PAD_OFFSET = 0.05
    VOTING_RATE = 0.01
    MIN_SEGMENT_DURATION = 0.15
    SHORT_SEGMENT_GAP = 0.1
    SAME_SPEAKER_GAP = 0.5

    # ------------------------------------------------------------------ third-party models
    @classmethod
    def _get_ten_vad_model(cls):
        """The process-wide TEN-VAD instance; ``ImportError`` when ``ten_vad`` is not installed."""
        if cls._ten_vad_model is None:
            from ten_vad import TenVad
            cls._ten_vad_model = TenVad(hop_size=VAD_HOP, threshold=cls.VAD_THRESHOLD)
        return cls._ten_vad_model

    @classmethod
    def _get_device(cls):
        if cls._device is None:
            import torch
            cls._device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        return cls._device

    @classmethod
    def _get_ecapa_model(cls):
        """The process-wide SpeechBrain ``spkrec-ecapa-voxceleb`` classifier (the path without ``speaker_model``); ``ImportError``
        when ``speechbrain`` is not installed."""
        if cls._ecapa_model is None:
            with warnings.catch_warnings():
                warnings.filterwarnings("ignore", message="torchaudio._backend")
                from speechbrain.inference.speaker import EncoderClassifier
                cls._ecapa_model = EncoderClassifier.from_hparams(source="speechbrain/spkrec-ecapa-voxceleb",
                                                                  run_opts={"device": str(cls._get_device())})
        return cls._ecapa_model

    # ------------------------------------------------------------------ the pipeline
    @classmethod
    def diarize(cls, audio, sample_rate: int = 16000, num_speakers: int | None = None, min_speakers: int = 2, max_speakers: int = 10,
                *, speaker_model=None, speech_frames=None, vad=None, cluster_device=None, **_kwargs) -> list[dict]:
        """audio: a waveform array or the path of an audio file -> ``[{"speaker": "SPEAKER_k", "start": s, "end": s}, ...]``.

        cluster_device: a torch device for the spectral clustering (``SpeakerClusterer(device=...)``); None keeps it on the host.

        speaker_model: an ``EcapaTdnnMI355X``; every window of every segment goes through one ``embed_windows`` call.  Without it
            SpeechBrain runs through PyTorch one window per call, as in the reference.
        speech_frames: the VAD's decisions, one per 256 samples, instead of running a VAD.
        vad: an object with TEN-VAD's ``process(int16 frame) -> (probability, flag)`` instead of the process-wide TEN-VAD; or one with
            ``speech_frames(audio) -> one decision per 256 samples`` (a ``vad.DeviceVAD``), which is called once on the whole array."""
        if isinstance(audio, str):
            import librosa
            audio, sample_rate = librosa.load(audio, sr=16000)
        if sample_rate != 16000:
            import librosa
            audio = librosa.resample(audio, orig_sr=sample_rate, target_sr=16000)
            sample_rate = 16000
        audio = audio.astype(np.float32)
        total_duration = len(audio) / sample_rate
        segments, vad_frames = cls._get_speech_segments(audio, sample_rate, speech_frames=speech_frames, vad=vad)
        if not segments:
            return []
        embeddings, window_segments = cls._extract_embeddings(audio, segments, sample_rate, speaker_model=speaker_model)
        if len(embeddings) == 0:
            return []
        labels = SpeakerClusterer(min_num_spks=min_speakers, max_num_spks=max_speakers, device=cluster_device)(embeddings, num_speakers)
        return cls._postprocess_segments(window_segments, labels, total_duration, vad_frames)

    @classmethod
    def _get_speech_segments(cls, audio_array: np.ndarray, sample_rate: int = 16000, *, speech_frames=None, vad=None):
        """-> (speech segments after hysteresis, the raw per-frame decisions).  Frames start every 256 samples while a whole frame
        AND at least one further sample remain, as the reference's loop has it."""
        if speech_frames is None and vad is not None and hasattr(vad, "speech_frames"):     # a whole-recording detector: one call, no frame loop
            from .vad import segments_from_flags
            flags = np.asarray(vad.speech_frames(audio_array)).astype(bool).reshape(-1)
            return segments_from_flags(flags, sample_rate), flags.tolist()
        if speech_frames is not None:
            frames = [bool(f) for f in speech_frames]
        else:
            model = vad if vad is not None else cls._get_ten_vad_model()
            pcm = audio_array if audio_array.dtype == np.int16 else (np.clip(audio_array, -1.0, 1.0) * 32767).astype(np.int16)
            frames = [model.process(pcm[i:i + VAD_HOP])[1] for i in range(0, len(pcm) - VAD_HOP, VAD_HOP)]
        frame_duration = VAD_HOP / sample_rate
        segments, begun = [], None
        for i, speech in enumerate(frames):
            if speech and begun is None:
                begun = i
            elif not speech and begun is not None:
                segments.append(_span(begun, i, frame_duration, sample_rate))
                begun = None
        if begun is not None:
            segments.append(_span(begun, len(frames), frame_duration, sample_rate))
        return cls._apply_vad_hysteresis(segments, sample_rate), frames

    @classmethod
    def _apply_vad_hysteresis(cls, segments: list[dict], sample_rate: int = 16000) -> list[dict]:
        """Bridge gaps up to VAD_MAX_GAP, drop what stays shorter than VAD_MIN_DURATION, pad the rest."""
        if not segments:
            return segments
        ordered = sorted(segments, key=lambda s: s["start"])
        joined = [ordered[0].copy()]
        for seg in ordered[1:]:
            if seg["start"] - joined[-1]["end"] <= cls.VAD_MAX_GAP:
                joined[-1]["end"], joined[-1]["end_sample"] = seg["end"], seg["end_sample"]
            else:
                joined.append(seg.copy())
        kept = [s for s in joined if (s["end"] - s["start"]) >= cls.VAD_MIN_DURATION]
        for s in kept:
            s["start"] = max(0.0, s["start"] - cls.VAD_PAD_ONSET)
            s["end"] = s["end"] + cls.VAD_PAD_OFFSET
            s["start_sample"], s["end_sample"] = int(s["start"] * sample_rate), int(s["end"] * sample_rate)
        return kept

    @classmethod
    def _window_positions(cls, segments: list[dict], sample_rate: int):
        """-> (window_samples, [(start_sample, end_sample), ...]) over all segments: the reference's positions, tail rule included."""
        window, step = int(cls.WINDOW_SIZE * sample_rate), int(cls.STEP_SIZE * sample_rate)
        spans = []
        for seg in segments:
            lo, hi = seg["start_sample"], seg["end_sample"]
            if hi - lo <= window:
                spans.append((lo, hi))
                continue
            starts = list(range(lo, hi - window + 1, step))
            spans += [(s, s + window) for s in starts]
            if starts and starts[-1] + window < hi and hi - (starts[-1] + window) > window * cls.TAIL_COVERAGE_RATIO:
                spans.append((hi - window, hi))
        return window, spans

    @classmethod
    def _extract_embeddings(cls, audio_array: np.ndarray, segments: list[dict], sample_rate: int, *, speaker_model=None):
        """-> (row-normalised embeddings [N, D], [{"start": s, "end": s}] per kept window).  A window whose embedding is not finite
        or has a norm of at most 1e-8 is dropped."""
        from sklearn.preprocessing import normalize
        window, spans = cls._window_positions(segments, sample_rate)
        if speaker_model is not None and hasattr(speaker_model, "embed_windows"):
            raw = cls._embed_on_device(speaker_model, audio_array, spans, window)
        else:
            import torch
            model = speaker_model if speaker_model is not None else cls._get_ecapa_model()
            raw = []
            with torch.no_grad():
                for lo, hi in spans:
                    chunk = audio_array[lo:hi]
                    if len(chunk) < window:
                        chunk = np.pad(chunk, (0, window - len(chunk)), mode="reflect")
                    raw.append(model.encode_batch(torch.from_numpy(chunk).float().unsqueeze(0)).squeeze(0).squeeze(0).cpu().numpy())
        embeddings, windows = [], []
        for e, (lo, hi) in zip(raw, spans):
            if np.isfinite(e).all() and np.linalg.norm(e) > 1e-8:
                embeddings.append(e)
                windows.append({"start": lo / sample_rate, "end": hi / sample_rate})
        if embeddings:
            return normalize(np.array(embeddings)), windows
        return np.array([]), []

    @staticmethod
    def _embed_on_device(speaker_model, audio_array: np.ndarray, spans, window: int) -> np.ndarray:
        """All windows through one ``embed_windows`` call.  A chunk shorter than the window is reflected by the feature kernel while
        it is read; one too short for a single reflection (fewer than pad + 1 samples: ``np.pad`` then reflects repeatedly) is padded
        here and rides behind the audio in the same upload."""
        if not spans:
            return np.zeros((0, 0), np.float32)
        n = len(audio_array)
        starts, lengths, extra = [], [], []
        for lo, hi in spans:
            have = max(0, min(hi, n) - lo) if lo >= 0 else len(audio_array[lo:hi])
            if lo >= 0 and window - have <= have - 1:
                starts.append(lo)
                lengths.append(have)
            else:
                chunk = audio_array[lo:hi]
                extra.append(np.pad(chunk, (0, window - len(chunk)), mode="reflect"))
                starts.append(n + (len(extra) - 1) * window)
                lengths.append(window)
        buf = np.concatenate([audio_array] + extra) if extra else audio_array
        return speaker_model.embed_windows(buf, starts, lengths, window).cpu().numpy()

    @classmethod
    def _resample_vad(cls, vad_frames: list[bool], num_frames: int) -> np.ndarray:
        """The 16 ms VAD decisions on the VOTING_RATE grid: voting frame f takes VAD frame ``int(f * VOTING_RATE / 0.016)``, clipped."""
        if not vad_frames:
            return np.zeros(num_frames, dtype=bool)
        decisions = np.array(vad_frames)
        at = np.clip(((np.arange(num_frames) * cls.VOTING_RATE) / (VAD_HOP / 16000)).astype(int), 0, len(decisions) - 1)
        return decisions[at]

    @classmethod
    def _postprocess_segments(cls, window_segments: list[dict], labels: np.ndarray, total_duration: float, vad_frames: list[bool]):
        """Frame-level voting: every window votes for its speaker on the frames it covers; a frame without votes or without speech
        is silence; runs of one speaker become segments."""
        if not window_segments or len(labels) == 0:
            return []
        speakers = np.unique(labels)
        if len(speakers) == 0:
            return []
        index = {old: new for new, old in enumerate(speakers)}
        num_frames = int(np.ceil(total_duration / cls.VOTING_RATE)) + 1
        votes = np.zeros((num_frames, len(speakers)), dtype=np.float32)
        for win, lbl in zip(window_segments, labels):
            first, last = int(win["start"] / cls.VOTING_RATE), min(int(win["end"] / cls.VOTING_RATE), num_frames)
            if first < last:
                votes[first:last, index[lbl]] += 1.0
        winner, score = np.argmax(votes, axis=1), np.max(votes, axis=1)
        speech = cls._resample_vad(vad_frames, num_frames)
        out, current, since = [], -1, 0.0
        for f in range(num_frames):
            who = -1 if (score[f] == 0 or not speech[f]) else int(winner[f])
            if who != current:
                if current != -1:
                    out.append({"speaker": f"SPEAKER_{current}", "start": since, "end": f * cls.VOTING_RATE})
                current, since = who, f * cls.VOTING_RATE
        if current != -1:
            out.append({"speaker": f"SPEAKER_{current}", "start": since, "end": num_frames * cls.VOTING_RATE})
        return cls._merge_short_segments(out)

    @classmethod
    def _merge_short_segments(cls, segments: list[dict]) -> list[dict]:
        """A segment under MIN_SEGMENT_DURATION extends a same-speaker predecessor closer than SHORT_SEGMENT_GAP or is dropped; any
        other segment extends a same-speaker predecessor closer than SAME_SPEAKER_GAP or starts a new entry."""
        if not segments:
            return []
        out: list[dict] = []
        for seg in segments:
            short = seg["end"] - seg["start"] < cls.MIN_SEGMENT_DURATION
            near = cls.SHORT_SEGMENT_GAP if short else cls.SAME_SPEAKER_GAP
            if out and out[-1]["speaker"] == seg["speaker"] and seg["start"] - out[-1]["end"] < near:
                out[-1]["end"] = seg["end"]
            elif not short:
                out.append(seg)
        return out

    @classmethod
    def assign_speakers_to_words(cls, words: list[dict], speaker_segments: list[dict]) -> list[dict]:
        """Adds ``"speaker"`` to every word: the first segment that contains the word's midpoint, else the segment whose midpoint is
        nearest (the first of equals), else None."""
        for word in words:
            mid = (word["start"] + word["end"]) / 2
            speaker = next((s["speaker"] for s in speaker_segments if s["start"] <= mid <= s["end"]), None)
            if speaker is None and speaker_segments:
                speaker = min(speaker_segments, key=lambda s: abs(mid - (s["start"] + s["end"]) / 2))["speaker"]
            word["speaker"] = speaker
        return words


class SpeakerDiarizer:
    """The public face of ``LocalSpeakerDiarizer`` (tiny_audio/diarization.py:684-730).

        >>> for seg in SpeakerDiarizer.diarize(audio, speaker_model=ecapa):
        ...     print(seg["speaker"], seg["start"], seg["end"])
    """

    @classmethod
    def diarize(cls, audio, sample_rate: int = 16000, num_speakers: int | None = None, min_speakers: int | None = None,
                max_speakers: int | None = None, *, speaker_model=None, speech_frames=None, vad=None, cluster_device=None,
                **_kwargs) -> list[dict]:
        return LocalSpeakerDiarizer.diarize(audio, sample_rate=sample_rate, num_speakers=num_speakers, min_speakers=min_speakers or 2,
                                            max_speakers=max_speakers or 10, speaker_model=speaker_model, speech_frames=speech_frames,
                                            vad=vad, cluster_device=cluster_device)

    @classmethod
    def assign_speakers_to_words(cls, words: list[dict], speaker_segments: list[dict]) -> list[dict]:
        return LocalSpeakerDiarizer.assign_speakers_to_words(words, speaker_segments)
