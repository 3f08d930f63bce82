"""-m "not gpu": the host side of long-form transcription (tiny_audio_amd/longform.py, ASRModel.transcribe_long) -- the ABI additions,
the dry-run marshalling of the three new entry points, every refusal, and the bookkeeping around the decode loop: groups by length
with a stable order, every window its own left-padded prompt, results back in time order, text joining, word-time offsets.  The
kernels compute nothing here (``_lib.DRY_RUN``): the gather is played by tests/segment_ref.py and ``generate`` by a recorder; the
numerics are in tests/test_gpu_longform.py."""
import numpy as np
import pytest
import torch

from oracle import weights as OW
from tests import segment_ref as R
from tiny_audio_amd import _lib, longform, ops, torch_ops

AUDIO_ID, PAD_ID, EOS_ID = 999, 990, 991


@pytest.fixture()
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


class _Tok:
    """Prompt = [1, (7 with a system turn), <audio> x count, 2, 3]; decode = 't<id>' words."""

    def convert_tokens_to_ids(self, t):
        return AUDIO_ID

    def apply_chat_template(self, messages, tokenize=True, add_generation_prompt=False, **_):
        user = [m for m in messages if m["role"] == "user"][0]["content"]
        head = [1, 7] if any(m["role"] == "system" for m in messages) else [1]
        return torch.tensor([head + [AUDIO_ID] * user.count("<audio>") + [2, 3]])

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(f"t{i}" for i in ids)


class _Extractor:
    """Stands in for the log-mel kernel: the mask is the frames that start inside the clip, the 'features' carry each window's first
    sample so that the recorder can tell the windows apart."""
    padding = False
    n_samples = 480000

    def extract(self, wav, lens):
        T = wav.shape[1] // 160
        mask = (torch.arange(T)[None, :] * 160 < lens[:, None]).to(torch.int32)
        return wav[:, :1].reshape(-1, 1, 1).clone(), mask


def _model():
    from tiny_audio_amd.asr_config import ASRConfig
    from tiny_audio_amd.asr_modeling import ASRModel
    enc, lm = OW.enc_config(hidden=256, ffn=512, layers=1, heads=4), OW.lm_config(vocab=1000, hidden=256, ffn=512, layers=1, heads=4, kv_heads=2)
    cfg = ASRConfig(audio_config=enc, text_config=lm, projector_hidden_dim=128, audio_token_id=AUDIO_ID, pad_token_id=PAD_ID, eos_token_id=EOS_ID)
    m = ASRModel(cfg, device="cpu", init="none", tokenizer=_Tok())
    m.feature_extractor = _Extractor()
    return m


def _record(m, monkeypatch, texts_by_first_sample=None):
    """model.generate -> a recorder that answers [round(first sample), placeholder count, eos, pad] per row."""
    calls = []

    def generate(**kw):
        ids, att, feats = kw["input_ids"], kw["attention_mask"], kw["input_features"]
        calls.append(kw)
        rows = []
        for b in range(ids.shape[0]):
            rows.append([int(round(float(feats[b, 0, 0]))), int((ids[b] == AUDIO_ID).sum()), EOS_ID, PAD_ID])
            if texts_by_first_sample and rows[-1][0] in texts_by_first_sample:
                rows[-1] = texts_by_first_sample[rows[-1][0]]
        return torch.tensor(rows)

    monkeypatch.setattr(m, "generate", generate, raising=False)
    monkeypatch.setattr(ops, "wave_windows", lambda wav, start, length, Ls, out=None: tuple(
        torch.from_numpy(a) for a in R.gather(wav.numpy(), start.tolist(), length.tolist(), Ls)))
    return calls


def _plans(monkeypatch, *cuts_per_recording):
    def plan_uploaded(flat, offsets, lens, min_len, max_len, smooth_positions=10, cut_penalty=0.05):
        assert len(lens) == len(cuts_per_recording)
        return [longform._plan_from_cuts(list(c), n, [0.5] * (len(c) - 2)) for c, n in zip(cuts_per_recording, lens)]
    monkeypatch.setattr(longform, "plan_uploaded", plan_uploaded)


def _ramp(n, base):
    """Sample i of the recording = base + i / 160: a window's first sample names its first position."""
    return (base + np.arange(n) / 160.0).astype(np.float32)


def _count(m, n_samples):
    frames = torch.tensor(-(-n_samples // 160))
    return int(m.projector.get_output_length(m._compute_encoder_output_lengths(torch.ones(1, int(frames), dtype=torch.int32))))


# ----------------------------------------------------------------------------- the ABI and the operators
def test_header_sources_version_and_operators(dry):
    protos = _lib.parse_header()
    for name, nargs in (("ta_wave_cut_cost_workspace_bytes", 2), ("ta_wave_cut_cost_f32", 11), ("ta_cut_plan_f32", 13), ("ta_wave_windows_f32", 9)):
        assert name in protos and len(protos[name][1]) == nargs, name
    import ctypes as C
    assert protos["ta_wave_cut_cost_workspace_bytes"][0] is C.c_long
    assert "segment.hip" in _lib.SOURCES and _lib.lib().ta_version() == 4
    assert {"wave_cut_cost", "cut_plan", "wave_windows"} <= set(torch_ops.OPERATORS)
    for name in ("wave_cut_cost", "cut_plan", "wave_windows"):
        assert str(getattr(torch.ops.ta355, name).default._schema).startswith(f"ta355::{name}(")
    assert ops.cut_cost_K(10) == R.cost_K(10) == 65 and ops.cut_cost_K(40) == R.cost_K(40) == 105
    L = _lib.lib()
    assert L.ta_wave_cut_cost_workspace_bytes(1, 48017) == 4 * (302 + 3 + 1)          # pw row, 3 tiles of 128 positions, the penalty
    assert L.ta_wave_cut_cost_workspace_bytes(1, 160 * 1048576 + 1) == 0 and L.ta_wave_cut_cost_workspace_bytes(65, 1000) == 0


def test_dry_run_records_the_three_calls_and_fake_shapes(dry):
    wav, off = torch.zeros(1000), torch.tensor([0, 400, 1000])
    cost = torch.ops.ta355.wave_cut_cost(wav, off, 600, 10, 0.05)
    assert cost.shape == (2, 5)
    cuts, n_seg, dp_T, back = torch.ops.ta355.cut_plan(cost, off, 600, 1, 2)
    assert cuts.shape == (2, 6) and n_seg.shape == (2,) and dp_T.shape == (2,) and back.shape == (2, 5)
    out, lens = torch.ops.ta355.wave_windows(wav, torch.tensor([0, 10]), torch.tensor([5, 7], dtype=torch.int32), 8)
    assert out.shape == (2, 8) and lens.shape == (2,) and lens.dtype == torch.int64
    assert [c for c in dry.calls if "cut" in c or "windows" in c] == ["ta_wave_cut_cost_f32", "ta_cut_plan_f32", "ta_wave_windows_f32"]
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        w, o = torch.empty(1000), torch.empty(3, dtype=torch.int64)
        c = torch.ops.ta355.wave_cut_cost(w, o, 600, 10, 0.05)
        assert c.shape == (2, 5)
        assert [t.shape for t in torch.ops.ta355.cut_plan(c, o, 600, 1, 2)] == [(2, 6), (2,), (2,), (2, 5)]
        assert [t.shape for t in torch.ops.ta355.wave_windows(w, o[:2], torch.empty(2, dtype=torch.int32), 8)] == [(2, 8), (2,)]


def test_operator_argument_checks(dry):
    wav, off = torch.zeros(1000), torch.tensor([0, 1000])
    with pytest.raises(ValueError, match="smooth_positions"):
        ops.wave_cut_cost(wav, off, 1000, 65)
    with pytest.raises(ValueError, match="cut_penalty"):
        ops.wave_cut_cost(wav, off, 1000, 10, -1.0)
    with pytest.raises(ValueError, match="beyond the kernel's limit"):
        ops.wave_cut_cost(wav, off, 160 * 1048576 + 1)
    cost = torch.zeros(1, 8)
    for mn, mx in ((0, 4), (3, 5), (1500, 3001)):
        with pytest.raises(ValueError, match="2 \\* min_len <= max_len"):
            ops.cut_plan(cost, off, 1000, mn, mx)
    with pytest.raises(ValueError, match="cost is"):
        ops.cut_plan(torch.zeros(1, 7), off, 1000, 1, 2)
    big = torch.tensor([0, 160 * 1048576])
    with pytest.raises(ValueError, match="sequential steps"):                       # 1 048 576 positions in blocks of 7: 149 796 > 131 072
        ops.cut_plan(torch.zeros(1, 1048577), big, 160 * 1048576, 7, 14)
    ops.cut_plan(torch.zeros(1, 1048577), big, 160 * 1048576, 8, 16)
    with pytest.raises(ValueError, match="Ls"):
        ops.wave_windows(wav, torch.tensor([0]), torch.tensor([5], dtype=torch.int32), 0)


# ----------------------------------------------------------------------------- refusals of transcribe_long
def test_every_refusal(dry):
    m = _model()
    x = np.zeros(16000, np.float32)
    with pytest.raises(ValueError, match="resample first"):
        m.transcribe_long(x, 8000)
    with pytest.raises(ValueError, match="empty audio"):
        m.transcribe_long(np.zeros(0, np.float32))
    with pytest.raises(ValueError, match="empty audio"):
        m.transcribe_long([])
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[77] = bad
        with pytest.raises(ValueError, match="non-finite"):
            m.transcribe_long([x, y])
    with pytest.raises(ValueError, match="min_window_s"):
        m.transcribe_long(x, max_window_s=19.0, min_window_s=10.0)
    with pytest.raises(ValueError, match="beyond the encoder's window"):
        m.transcribe_long(x, max_window_s=30.01, min_window_s=10.0)            # 2 * max_source_positions = 3000 frames
    with pytest.raises(ValueError, match="batch_size"):
        m.transcribe_long(x, batch_size=0)
    with pytest.raises(ValueError, match="acoustic_model"):
        m.transcribe_long(x, return_timestamps=True)
    with pytest.raises(ValueError, match="beyond the cap"):
        m.transcribe_long(torch.empty(160 * 1048576 + 1, dtype=torch.int8))     # never touched: refused by its length alone
    with pytest.raises(ValueError, match="1-D"):
        m.transcribe_long(np.zeros((2, 100), np.float32))
    m.tokenizer = None
    with pytest.raises(ValueError, match="tokenizer"):
        m.transcribe_long(x)
    assert "ta_wave_cut_cost_f32" not in dry.calls, "every refusal comes before any device work"
    assert longform.window_positions(28.0, 10.0) == (1000, 2800) and longform.window_positions(2.0, 0.5) == (50, 200)
    assert longform.window_positions(0.3, 0.15) == (15, 30) and longform.window_positions(30.0, 0.1) == (10, 3000)
    for tiny in (0.0, -1.0, 0.09):
        with pytest.raises(ValueError, match="at least 0.1 s"):
            longform.window_positions(28.0, tiny)


# ----------------------------------------------------------------------------- the bookkeeping
def test_groups_prompts_time_order_and_joining(dry, monkeypatch):
    m = _model()
    n0, n1 = 160 * 1000 + 37, 160 * 800
    _plans(monkeypatch, [0, 300, 500, 900, 1001], [0, 400, 800])
    # window lengths, in time order: 48000, 32000, 64000, 16037 | 64000, 64000
    silent = {5300: [EOS_ID, PAD_ID, PAD_ID, PAD_ID]}                           # recording 0's window at position 300 says nothing
    calls = _record(m, monkeypatch, silent)
    res = m.transcribe_long([_ramp(n0, 5000), _ramp(n1, 7000)], batch_size=3, max_new_tokens=4, repetition_penalty=1.3, do_sample=False)
    assert longform.group_windows([48000, 32000, 64000, 16037, 64000, 64000], 3) == [[2, 4, 5], [0, 1, 3]]      # longest first, stable
    assert len(calls) == 2
    firsts = [[int(round(float(v))) for v in kw["input_features"][:, 0, 0]] for kw in calls]
    assert firsts == [[5500, 7000, 7400], [5000, 5300, 5900]]
    # every generate keyword passed through; every window its own placeholder count, left-padded
    for kw in calls:
        assert kw["max_new_tokens"] == 4 and kw["repetition_penalty"] == 1.3 and kw["do_sample"] is False
    lens = [[64000, 64000, 64000], [48000, 32000, 16037]]
    for kw, ls in zip(calls, lens):
        ids, att = kw["input_ids"], kw["attention_mask"]
        counts = [_count(m, n) for n in ls]
        L = 4 + max(counts)                                                     # the config's default system prompt adds a turn: [1, 7]
        assert ids.shape == att.shape == (3, L) and kw["input_features"].shape[0] == 3
        for b, c in enumerate(counts):
            want = [PAD_ID] * (L - 4 - c) + [1, 7] + [AUDIO_ID] * c + [2, 3]
            assert ids[b].tolist() == want and att[b].tolist() == [0] * (L - 4 - c) + [1] * (4 + c)
        assert kw["audio_attention_mask"].sum(-1).tolist() == [-(-n // 160) for n in ls]
    assert len({_count(m, n) for n in lens[1]}) == 3, "the test's windows must differ in their counts"
    # results: a list per recording, chunks in time order with their own times, the silent window kept as an empty chunk
    assert isinstance(res, list) and len(res) == 2
    c0 = res[0]["chunks"]
    assert [c["timestamp"] for c in c0] == [(0.0, 3.0), (3.0, 5.0), (5.0, 9.0), (9.0, n0 / 16000)]
    assert [c["text"] for c in c0] == [f"t5000 t{_count(m, 48000)}", "", f"t5500 t{_count(m, 64000)}", f"t5900 t{_count(m, 16037)}"]
    assert res[0]["text"] == " ".join(c["text"] for c in c0 if c["text"]) and "  " not in res[0]["text"]
    assert [c["timestamp"] for c in res[1]["chunks"]] == [(0.0, 4.0), (4.0, 8.0)]
    assert res[1]["text"] == f"t7000 t{_count(m, 64000)} t7400 t{_count(m, 64000)}" and "words" not in res[1]


def test_system_prompt_reaches_every_window(dry, monkeypatch):
    m = _model()
    m.system_prompt = None
    _plans(monkeypatch, [0, 100, 250])
    calls = _record(m, monkeypatch)
    m.transcribe_long(_ramp(160 * 250, 100), batch_size=8)
    res = m.transcribe_long(_ramp(160 * 250, 100), batch_size=8, system_prompt="be brief")
    assert isinstance(res, dict) and len(calls) == 2
    for kw, head in zip(calls, ([1, AUDIO_ID], [1, 7])):
        assert kw["input_ids"].shape[0] == 2
        for b in range(2):
            row = [v for v in kw["input_ids"][b].tolist() if v != PAD_ID]
            assert row[:2] == head and row[-2:] == [2, 3]


def test_one_short_recording_is_one_window(dry, monkeypatch):
    m = _model()
    calls = _record(m, monkeypatch)
    x = _ramp(16000 * 20 + 5, 42)                                               # 20 s < max_window_s: the dry-run plan is the trivial one
    res = m.transcribe_long(x)
    assert len(calls) == 1 and calls[0]["input_ids"].shape[0] == 1 and calls[0]["audio_attention_mask"].shape == (1, 2000)
    assert len(res["chunks"]) == 1 and res["chunks"][0]["timestamp"] == (0.0, len(x) / 16000) and res["text"] == res["chunks"][0]["text"]
    assert {"ta_wave_cut_cost_f32", "ta_cut_plan_f32"} <= set(dry.calls)


def test_whisper_padding_uses_the_extractors_window(dry, monkeypatch):
    m = _model()
    m.feature_extractor.padding = "max_length"                                 # what ASRModel sets for a Whisper tower
    _plans(monkeypatch, [0, 100, 250])
    calls = _record(m, monkeypatch)
    m.transcribe_long(_ramp(160 * 250, 0))
    assert calls[0]["audio_attention_mask"].shape == (2, 3000) and calls[0]["audio_attention_mask"].sum(-1).tolist() == [150, 100]


def test_word_times_are_shifted_by_the_window_start(dry, monkeypatch):
    from tiny_audio_amd.alignment import ForcedAligner
    m = _model()
    _plans(monkeypatch, [0, 300, 500, 502], [0, 200])
    calls = _record(m, monkeypatch, {5300: [EOS_ID, PAD_ID, PAD_ID, PAD_ID]})
    seen = []

    def align_audio_batch(audios, texts, acoustic_model, **kw):
        assert acoustic_model == "AM"
        seen.append(([int(a.shape[0]) for a in audios], [float(a[0]) for a in audios], list(texts)))
        return [[{"word": t.split()[0], "start": 0.25, "end": 0.5}, {"word": "x", "start": 1.0, "end": 1.5}] for t in texts]

    monkeypatch.setattr(ForcedAligner, "align_audio_batch", staticmethod(align_audio_batch))
    res = m.transcribe_long([_ramp(160 * 502, 5000), _ramp(160 * 200, 7000)], batch_size=2, return_timestamps=True, acoustic_model="AM")
    # groups by length: [48000 (r0 w0), 32000 (r0 w1, silent)], [32000 (r1 w0), 320 (r0 w2: below one acoustic frame)]
    assert seen == [([48000], [5000.0], [res[0]["chunks"][0]["text"]]), ([32000], [7000.0], [res[1]["chunks"][0]["text"]])]
    assert res[0]["words"] == [{"word": "t5000", "start": 0.25, "end": 0.5}, {"word": "x", "start": 1.0, "end": 1.5}]
    assert res[1]["words"] == [{"word": "t7000", "start": 0.25, "end": 0.5}, {"word": "x", "start": 1.0, "end": 1.5}]
    # a later window's words carry its start
    seen.clear()
    _record(m, monkeypatch)
    _plans(monkeypatch, [0, 300, 700])
    res = m.transcribe_long(_ramp(160 * 700, 5000), return_timestamps=True, acoustic_model="AM")
    assert [w["start"] for w in res["words"]] == [0.25, 1.0, 3.25, 4.0] and [w["end"] for w in res["words"]] == [0.5, 1.5, 3.5, 4.5]
    assert [w["word"] for w in res["words"]] == ["t5000", "x", "t5300", "x"]
