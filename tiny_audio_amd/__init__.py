"""tiny_audio_amd -- the MI355X-native hot path of tiny-audio.  Submodules are imported where they are used; the names below (the
speaker-diarization entry points) resolve lazily so that importing the package stays free of torch and of the HIP library."""
_LAZY = {"EcapaConfig": "ecapa", "EcapaTdnnMI355X": "ecapa", "SpectralCluster": "diarization", "SpeakerClusterer": "diarization",
         "LocalSpeakerDiarizer": "diarization", "SpeakerDiarizer": "diarization", "DeviceSpectralCluster": "spectral"}
__all__ = sorted(_LAZY)


def __getattr__(name):
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
