"""Speaker diarization: who spoke when.  Speech segments from a VAD (TEN-VAD, or ``vad.DeviceVAD`` on the device) -> ECAPA-TDNN
embeddings of sliding windows -> spectral clustering -> frame-level voting -> merged speaker segments.

This is the counterpart of the reference's ``tiny_audio/diarization.py`` (the module behind ``ASRPipeline(return_speakers=True)``,
tiny_audio/asr_pipeline.py:133-152): the same class names, class constants, arguments, return values and quirks, restated.  What
differs is the hot path.  The reference pushes every 0.75 s window through SpeechBrain's ``encode_batch`` one window per call
(tiny_audio/diarization.py:490-502); with ``speaker_model=`` (an ``EcapaTdnnMI355X``) every window of every segment goes through ONE
``embed_windows`` call on the device -- the audio is uploaded once and the windows are cut and reflect-padded by the feature kernel.
Voting and merging behind the ``[N, 192]`` embeddings are host loops in numpy and plain Python exactly as the reference has them --
fine for a 30 s clip, a million interpreted steps at the long-form cap; ``post_device=`` (and ``device=`` of the three functions) runs
the same rules as HIP kernels for ragged batches of recordings, with the same lists as result (csrc/speaker_post.hip).  Spectral clustering is not: ``SpectralCluster`` restates the reference's dense float64 affinity, Laplacian and full
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
                *, speaker_model=None, speech_frames=None, vad=None, cluster_device=None, post_device=None, **_kwargs) -> list[dict]:
        """audio: a waveform array or the path of an audio file -> ``[{"speaker": "SPEAKER_k", "start": s, "end": s}, ...]``.

        cluster_device: a torch device for the spectral clustering (``SpeakerClusterer(device=...)``); None keeps it on the host.
        post_device: a torch device for the voting and the merging behind the labels (``spk_vote``, ``spk_merge``; the same lists);
            None keeps the reference's loops here.  With a ``vad.DeviceVAD`` its decisions stay on the device for the voting.

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
        if post_device is not None:
            return cls.diarize_batch([audio], sample_rate, num_speakers, min_speakers, max_speakers, speaker_model=speaker_model,
                                     speech_frames=None if speech_frames is None else [speech_frames], vad=vad,
                                     cluster_device=cluster_device, post_device=post_device)[0]
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
    def diarize_batch(cls, audios, sample_rate: int = 16000, num_speakers: int | None = None, min_speakers: int = 2, max_speakers: int = 10,
                      *, speaker_model=None, speech_frames=None, vad=None, cluster_device=None, post_device=None) -> list[list[dict]]:
        """``diarize`` of several 16 kHz waveform arrays -> one list of turns per recording.  VAD, embeddings and clustering run per
        recording as in ``diarize``; with ``post_device`` the voting and merging of ALL recordings is one ``spk_vote`` and one
        ``spk_merge`` launch, and a ``vad.DeviceVAD`` runs once on one upload of all recordings, its decisions staying on the device
        for the voting.  speech_frames: None, or one list of decisions per recording."""
        if sample_rate != 16000:
            raise ValueError(f"diarize_batch takes 16 kHz arrays, got sample_rate={sample_rate}: resample first")
        audios = [np.asarray(a).astype(np.float32) for a in audios]
        if speech_frames is not None and len(speech_frames) != len(audios):
            raise ValueError(f"speech_frames holds {len(speech_frames)} lists for {len(audios)} recordings")
        vad_device, flags_h = None, None
        if post_device is not None and speech_frames is None and vad is not None and hasattr(vad, "speech_frames_uploaded") and audios:
            from .longform import upload
            flat, offsets, lens = upload(audios, post_device)
            flags_h, flags_d, n_vad = vad.speech_frames_uploaded(flat, offsets, lens)
            vad_device = (flags_d, n_vad)
        items = []
        for r, audio in enumerate(audios):
            total_duration = len(audio) / sample_rate
            if flags_h is not None:
                from .vad import segments_from_flags
                segments, vad_frames = segments_from_flags(flags_h[r], sample_rate), flags_h[r].tolist()
            else:
                segments, vad_frames = cls._get_speech_segments(audio, sample_rate, vad=vad,
                                                                speech_frames=None if speech_frames is None else speech_frames[r])
            windows, labels = [], []
            if segments:
                embeddings, window_segments = cls._extract_embeddings(audio, segments, sample_rate, speaker_model=speaker_model)
                if len(embeddings):
                    labels = SpeakerClusterer(min_num_spks=min_speakers, max_num_spks=max_speakers, device=cluster_device)(embeddings,
                                                                                                                          num_speakers)
                    windows = window_segments
            items.append((windows, labels, total_duration, vad_frames))
        if post_device is None:
            return [cls._postprocess_segments(*it) for it in items]
        return cls.postprocess_batch(items, post_device, vad_device=vad_device)

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
    def extract_embeddings_uploaded(cls, flat, offsets, lens, segments_per_recording, speaker_model, sample_rate: int = 16000):
        """``_extract_embeddings`` of several recordings that lie in one uploaded buffer (``longform.upload``: recording r at
        ``flat[offsets[r] : offsets[r] + lens[r]]``) -> per recording (row-normalised embeddings [N, D], the kept windows).  Every
        window the feature kernel can reflect by itself is read from ``flat`` in ONE ``embed_windows`` call; the few chunks too short
        for a single reflection are fetched, padded here as ``np.pad`` pads them, and go through a second call."""
        from sklearn.preprocessing import normalize
        spans_of, where, starts, lengths, extra, window = [], [], [], [], [], int(cls.WINDOW_SIZE * sample_rate)
        for r, segs in enumerate(segments_per_recording):
            window, spans = cls._window_positions(segs, sample_rate)
            base, n = int(offsets[r]), int(lens[r])
            spans_of.append(spans)
            for lo, hi in spans:
                if lo < 0:
                    raise ValueError(f"recording {r}: a window starts at sample {lo}")
                have = max(0, min(hi, n) - lo)
                if window - have <= have - 1:
                    where.append((0, len(starts)))
                    starts.append(base + lo), lengths.append(have)
                else:
                    chunk = flat[base + lo:base + lo + have].detach().cpu().numpy()
                    where.append((1, len(extra)))
                    extra.append(np.pad(chunk, (0, window - len(chunk)), mode="reflect"))
        raw = [None, None]
        if starts:
            raw[0] = speaker_model.embed_windows(flat, starts, lengths, window).cpu().numpy()
        if extra:
            raw[1] = speaker_model.embed_windows(np.concatenate(extra), [i * window for i in range(len(extra))], [window] * len(extra),
                                                 window).cpu().numpy()
        out, k = [], 0
        for spans in spans_of:
            embeddings, windows = [], []
            for lo, hi in spans:
                e = raw[where[k][0]][where[k][1]]
                k += 1
                if np.isfinite(e).all() and np.linalg.norm(e) > 1e-8:
                    embeddings.append(e)
                    windows.append({"start": lo / sample_rate, "end": hi / sample_rate})
            out.append((normalize(np.array(embeddings)), windows) if embeddings else (np.array([]), []))
        return out

    @classmethod
    def _resample_vad(cls, vad_frames: list[bool], num_frames: int) -> np.ndarray:
        """The 16 ms VAD decisions on the VOTING_RATE grid: voting frame f takes VAD frame ``int(f * VOTING_RATE / 0.016)``, clipped."""
        if not vad_frames:
            return np.zeros(num_frames, dtype=bool)
        decisions = np.array(vad_frames)
        at = np.clip(((np.arange(num_frames) * cls.VOTING_RATE) / (VAD_HOP / 16000)).astype(int), 0, len(decisions) - 1)
        return decisions[at]

    @classmethod
    def _postprocess_segments(cls, window_segments: list[dict], labels: np.ndarray, total_duration: float, vad_frames: list[bool],
                              device=None):
        """Frame-level voting: every window votes for its speaker on the frames it covers; a frame without votes or without speech
        is silence; runs of one speaker become segments.  ``device``: a torch device -- the same lists from ``spk_vote`` and
        ``spk_merge`` (``postprocess_batch``); None -- the reference's loops over the frames and the runs, here."""
        if device is not None:
            return cls.postprocess_batch([(window_segments, labels, total_duration, vad_frames)], device)[0]
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
    def _merge_short_segments(cls, segments: list[dict], device=None) -> list[dict]:
        """A segment under MIN_SEGMENT_DURATION extends a same-speaker predecessor closer than SHORT_SEGMENT_GAP or is dropped; any
        other segment extends a same-speaker predecessor closer than SAME_SPEAKER_GAP or starts a new entry.  ``device``: ``spk_merge``
        on that device, which takes turns on the voting grid (what ``_postprocess_segments`` makes): every time is snapped to its
        frame f and stands for ``f * VOTING_RATE``; one further than a microsecond from the grid is a ``ValueError``."""
        if device is not None:
            return cls._merge_on_device(segments, device)
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
    def assign_speakers_to_words(cls, words: list[dict], speaker_segments: list[dict], device=None) -> list[dict]:
        """Adds ``"speaker"`` to every word: the first segment that contains the word's midpoint, else the segment whose midpoint is
        nearest (the first of equals), else None.  ``device``: one ``spk_words`` launch instead of words x segments steps here."""
        if device is not None:
            return cls.assign_speakers_batch([(words, speaker_segments)], device)[0]
        for word in words:
            mid = (word["start"] + word["end"]) / 2
            speaker = next((s["speaker"] for s in speaker_segments if s["start"] <= mid <= s["end"]), None)
            if speaker is None and speaker_segments:
                speaker = min(speaker_segments, key=lambda s: abs(mid - (s["start"] + s["end"]) / 2))["speaker"]
            word["speaker"] = speaker
        return words

    # ------------------------------------------------------------------ the same stage on the device (csrc/speaker_post.hip)
    @classmethod
    def spk_options(cls) -> tuple:
        """``ta_spk_post_options`` from the class attributes, so that a subclass that overrides them is honoured."""
        return (cls.VOTING_RATE, VAD_HOP / 16000, cls.MIN_SEGMENT_DURATION, cls.SHORT_SEGMENT_GAP, cls.SAME_SPEAKER_GAP)

    @classmethod
    def turns_from_frames(cls, spk, f0, f1, names) -> list[dict]:
        """Integer frames -> the reference's dicts: every time is ``f * VOTING_RATE``, formed here exactly as the frame loop forms it."""
        return [{"speaker": names[int(k)], "start": int(a) * cls.VOTING_RATE, "end": int(b) * cls.VOTING_RATE}
                for k, a, b in zip(spk, f0, f1)]

    @classmethod
    def vote_inputs(cls, window_segments, labels, total_duration):
        """One recording's windows on the voting grid -> (first int32 [Nw], last int32 [Nw], rank int32 [Nw], names, num_frames): the
        host's share of ``_postprocess_segments`` as one numpy expression each -- ``int(start / VOTING_RATE)``,
        ``min(int(end / VOTING_RATE), num_frames)`` and the rank of every label among ``np.unique(labels)``."""
        from .ops import SPK_LIMITS
        labels = np.asarray(labels)
        speakers = np.unique(labels)
        n = min(len(window_segments), len(labels))                  # zip() stops at the shorter
        num_frames = int(np.ceil(total_duration / cls.VOTING_RATE)) + 1
        if not 1 <= num_frames <= SPK_LIMITS["frames"]:
            raise ValueError(f"{total_duration} s are {num_frames} voting frames, beyond the limit of {SPK_LIMITS['frames']} per recording")
        if len(speakers) > SPK_LIMITS["speakers"]:
            raise ValueError(f"{len(speakers)} speakers, the voting kernel takes at most {SPK_LIMITS['speakers']}")
        start = np.array([w["start"] for w in window_segments[:n]], np.float64)
        end = np.array([w["end"] for w in window_segments[:n]], np.float64)
        if not (np.isfinite(start).all() and np.isfinite(end).all()):
            raise ValueError("a window's start or end is not finite")
        first = (start / cls.VOTING_RATE).astype(np.int64)
        last = np.minimum((end / cls.VOTING_RATE).astype(np.int64), num_frames)
        if (first < 0).any():
            raise ValueError("a window starts before 0 (first >= 0 is required: the reference's slice would wrap a negative start around "
                             "the grid, which is not rebuilt on the device)")
        first = np.minimum(first, num_frames)                       # a window beyond the grid votes nowhere; its start fits int32 this way
        last = np.maximum(last, -1)
        rank = np.searchsorted(speakers, labels[:n])
        return first.astype(np.int32), last.astype(np.int32), rank.astype(np.int32), [f"SPEAKER_{k}" for k in range(len(speakers))], num_frames

    @classmethod
    def postprocess_batch(cls, items, device, vad_device=None, return_frames: bool = False):
        """``_postprocess_segments`` of several recordings in ONE ``spk_vote`` and ONE ``spk_merge`` launch, and one read-back.
        items: per recording ``(window_segments, labels, total_duration, vad_frames)``.  vad_device: ``(flags uint8 [R, ld], n_vad
        int32 [R])`` already on the device, row r for items[r] (what ``DeviceVAD.run_uploaded`` returned): then ``vad_frames`` is read
        on the host only to bound the number of runs, and nothing is uploaded a second time.  -> the turns per recording (with
        ``return_frames`` the integer triples ``(spk, f0, f1)`` beside them)."""
        import torch
        from . import torch_ops  # noqa: F401  (registers torch.ops.ta355.spk_*)
        R = len(items)
        out = [[] for _ in range(R)]
        frames = [(np.zeros(0, np.int32),) * 3 for _ in range(R)]
        firsts, lasts, ranks, names, n_frames, n_win, caps, vads = [], [], [], [], [], [], [], []
        for wins, labels, total_duration, vad_frames in items:
            live = bool(wins) and len(labels) > 0
            f, l, k, nm, nf = cls.vote_inputs(wins if live else [], labels if live else [], total_duration)
            v = np.asarray(vad_frames if vad_frames is not None else [], dtype=bool).reshape(-1)
            firsts.append(f), lasts.append(l), ranks.append(k), names.append(nm), n_frames.append(nf), n_win.append(len(f)), vads.append(v)
            # an owner changes only where a window begins or ends or the VAD's decision changes: a bound on the runs, and never more than frames
            caps.append(0 if not live else min(2 * len(f) + int(np.count_nonzero(v[1:] != v[:-1])) + 2, nf))
        if R == 0 or not any(n_win):
            return (out, frames) if return_frames else out
        dev = torch.device(device)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)  # noqa: E731
        cu = lambda c: i32(np.concatenate([[0], np.cumsum(c)]))  # noqa: E731
        if vad_device is None:
            ld = max(1, max(len(v) for v in vads))
            flags_h = np.zeros((R, ld), np.uint8)
            for r, v in enumerate(vads):
                flags_h[r, :len(v)] = v
            flags, n_vad = torch.from_numpy(flags_h).to(dev), i32([len(v) for v in vads])
        else:
            flags, n_vad = vad_device
            flags = flags if flags.shape[1] > 0 else flags.new_zeros((R, 1))
        S = max(1, max(len(nm) for nm in names))
        opts = cls.spk_options()
        cap, cu_cap = int(sum(caps)), cu(caps)
        run_spk, run_f0, run_f1, n_runs, status = torch.ops.ta355.spk_vote(
            i32(np.concatenate(firsts)), i32(np.concatenate(lasts)), i32(np.concatenate(ranks)), cu(n_win), S, i32(n_frames),
            int(max(n_frames)), flags.contiguous(), n_vad.to(torch.int32).contiguous(), cu_cap, cap, *opts)
        seg_spk, seg_f0, seg_f1, n_seg = torch.ops.ta355.spk_merge(run_spk, run_f0, run_f1, cu_cap, n_runs, *opts)
        back = torch.cat([seg_spk, seg_f0, seg_f1, n_seg, status]).cpu().numpy()      # the one read-back
        spk_h, f0_h, f1_h, n_seg_h, status_h = back[:cap], back[cap:2 * cap], back[2 * cap:3 * cap], back[3 * cap:3 * cap + R], back[3 * cap + R:]
        if not _dry_run() and status_h.any():
            raise RuntimeError(f"spk_vote reported status {status_h.tolist()}: the runs did not fit their bound")
        o = np.concatenate([[0], np.cumsum(caps)])
        for r in range(R):
            sl = slice(int(o[r]), int(o[r]) + int(n_seg_h[r]))
            frames[r] = (spk_h[sl].copy(), f0_h[sl].copy(), f1_h[sl].copy())
            out[r] = cls.turns_from_frames(*frames[r], names[r])
        return (out, frames) if return_frames else out

    @classmethod
    def _merge_on_device(cls, segments: list[dict], device) -> list[dict]:
        import torch
        from . import torch_ops  # noqa: F401
        if not segments:
            return []
        names = list(dict.fromkeys(s["speaker"] for s in segments))
        t = np.array([[s["start"], s["end"]] for s in segments], np.float64)
        f = np.rint(t / cls.VOTING_RATE)
        if not np.isfinite(t).all() or (np.abs(f * cls.VOTING_RATE - t) > 1e-6).any() or (f < 0).any() or (f > 2 ** 31 - 1).any():
            raise ValueError("the device path merges turns on the voting grid: a start or an end lies more than a microsecond from a "
                             f"multiple of VOTING_RATE = {cls.VOTING_RATE}, or outside int32 frames")
        dev = torch.device(device)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)  # noqa: E731
        spk = i32([names.index(s["speaker"]) for s in segments])
        seg_spk, seg_f0, seg_f1, n_seg = torch.ops.ta355.spk_merge(spk, i32(f[:, 0]), i32(f[:, 1]), i32([0, len(segments)]), None,
                                                                   *cls.spk_options())
        n = int(n_seg.cpu()[0])
        return cls.turns_from_frames(seg_spk[:n].cpu().numpy(), seg_f0[:n].cpu().numpy(), seg_f1[:n].cpu().numpy(), names)

    @classmethod
    def assign_speakers_batch(cls, items, device) -> list:
        """``assign_speakers_to_words`` of several recordings in ONE ``spk_words`` launch.  items: per recording
        ``(words, speaker_segments)``; every word gains ``"speaker"`` in place, as the host function does it."""
        import torch
        from . import torch_ops  # noqa: F401
        from .ops import SPK_LIMITS
        ws = np.array([[w["start"], w["end"]] for words, _ in items for w in words], np.float64).reshape(-1, 2)
        ss = np.array([[s["start"], s["end"]] for _, segs in items for s in segs], np.float64).reshape(-1, 2)
        if not (np.isfinite(ws).all() and np.isfinite(ws.sum(1)).all()):
            raise ValueError("a word's start or end is not finite")
        if not (np.isfinite(ss).all() and np.isfinite(ss.sum(1)).all()):
            raise ValueError("a segment's start or end is not finite")
        for what, n in (("words", len(ws)), ("segments", len(ss))):
            if n > SPK_LIMITS["items"]:
                raise ValueError(f"{n} {what}, the kernel takes at most {SPK_LIMITS['items']} per call")
        if len(items) > SPK_LIMITS["recordings"]:
            raise ValueError(f"{len(items)} recordings, the kernel takes at most {SPK_LIMITS['recordings']} per call")
        if len(ws):
            dev = torch.device(device)
            f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
            cu = lambda c: torch.from_numpy(np.concatenate([[0], np.cumsum(c)]).astype(np.int32)).to(dev)  # noqa: E731
            idx = torch.ops.ta355.spk_words(f64(ws[:, 0]), f64(ws[:, 1]), cu([len(w) for w, _ in items]), f64(ss[:, 0]), f64(ss[:, 1]),
                                            cu([len(s) for _, s in items])).cpu().tolist()
        k = 0
        for words, segs in items:
            for w in words:
                g = idx[k] if segs else -1
                w["speaker"] = segs[g]["speaker"] if 0 <= g < len(segs) else None
                k += 1
        return [words for words, _ in items]


def _dry_run() -> bool:
    from . import _lib
    return _lib.DRY_RUN


class SpeakerDiarizer:
    """The public face of ``LocalSpeakerDiarizer`` (tiny_audio/diarization.py:684-730).

        >>> for seg in SpeakerDiarizer.diarize(audio, speaker_model=ecapa):
        ...     print(seg["speaker"], seg["start"], seg["end"])
    """

    @classmethod
    def diarize(cls, audio, sample_rate: int = 16000, num_speakers: int | None = None, min_speakers: int | None = None,
                max_speakers: int | None = None, *, speaker_model=None, speech_frames=None, vad=None, cluster_device=None,
                post_device=None, **_kwargs) -> list[dict]:
        return LocalSpeakerDiarizer.diarize(audio, sample_rate=sample_rate, num_speakers=num_speakers, min_speakers=min_speakers or 2,
                                            max_speakers=max_speakers or 10, speaker_model=speaker_model, speech_frames=speech_frames,
                                            vad=vad, cluster_device=cluster_device, post_device=post_device)

    @classmethod
    def diarize_batch(cls, audios, sample_rate: int = 16000, num_speakers: int | None = None, min_speakers: int | None = None,
                      max_speakers: int | None = None, **kwargs) -> list[list[dict]]:
        return LocalSpeakerDiarizer.diarize_batch(audios, sample_rate, num_speakers, min_speakers or 2, max_speakers or 10, **kwargs)

    @classmethod
    def assign_speakers_to_words(cls, words: list[dict], speaker_segments: list[dict], device=None) -> list[dict]:
        return LocalSpeakerDiarizer.assign_speakers_to_words(words, speaker_segments, device=device)
