"""-m "not gpu": the long form of forced alignment off the device -- the header's limits against ``ops.ALIGN_LONG_LIMITS``, the workspace
query, every refusal (C ABI and Python), the operator's registration, the dry-run plumbing of ``align_long`` / ``align_long_batch``, and
the window table of ``Wav2Vec2CtcMI355X.emissions_long``.  The short form's own limits and wording (tests/test_alignment_host.py)
are not touched by any of it, which the last test pins."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tiny_audio_amd import _lib, alignment, ops
from tiny_audio_amd import wav2vec2 as W
from tiny_audio_amd.alignment import ForcedAligner

I32 = torch.int32


@pytest.fixture
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


def header_define(name):
    return int(re.search(rf"#define {name} (\d+)", open(_lib.HEADER).read()).group(1))


# ----------------------------------------------------------------------------- limits and workspace
def test_header_limits_and_python_limits_agree():
    want = {"clips": 64, "frames": 1048576, "tokens": 262144, "classes": 65536, "col_block": 2048}
    assert ops.ALIGN_LONG_LIMITS == want
    got = {k: header_define("TA_ALIGN_LONG_MAX_" + n) for k, n in (("clips", "CLIPS"), ("frames", "FRAMES"), ("tokens", "TOKENS"),
                                                                    ("classes", "CLASSES"), ("col_block", "COL_BLOCK"))}
    assert got == want
    cb, fb = header_define("TA_ALIGN_LONG_COL_BLOCK"), header_define("TA_ALIGN_LONG_FRAME_BLOCK")
    assert cb % 64 == 0 and 64 <= cb <= want["col_block"] and fb >= 1
    text = open(_lib.HEADER).read()
    assert "tiny_audio/asr_pipeline.py:117-131" in text and "0.016" in text          # the call it serves, and the f32 note
    protos = _lib.parse_header()
    assert len(protos["ta_ctc_align_long_f32"][1]) == 20 and len(protos["ta_ctc_align_long_workspace_bytes"][1]) == 5
    assert protos["ta_ctc_align_long_workspace_bytes"][0] is C.c_long
    # every size that can pass 2^31 is a long: the row stride and the workspace size
    assert protos["ta_ctc_align_long_f32"][1][1] is C.c_long and protos["ta_ctc_align_long_f32"][1][16] is C.c_long


def expected_ws(N, T, J, cb):
    """The decision bits (one 64-bit word per frame and 64 columns), the row carry [nCB][cb], the column carry [nCB][T], one flag a clip."""
    ncb = -(-(J + 1) // cb)
    return N * T * ((J >> 6) + 1) * 8 + N * ncb * (cb + T) * 4 + (N * 4 + 7) // 8 * 8


def test_workspace_arithmetic():
    q = _lib.lib().ta_ctc_align_long_workspace_bytes
    cb0 = header_define("TA_ALIGN_LONG_COL_BLOCK")
    assert q(3, 150, 97, 64, 8) == expected_ws(3, 150, 97, 64) == 3 * 150 * 2 * 8 + 3 * 2 * (64 + 150) * 4 + 16
    assert q(3, 150, 97, 64, 8) == q(3, 150, 97, 64, 1000)                 # the frame block moves no byte
    assert q(1, 150, 97, 0, 0) == expected_ws(1, 150, 97, cb0)             # 0 = the defaults
    big = q(1, 180000, 60000, 0, 0)                                        # an hour against its transcript
    assert big == expected_ws(1, 180000, 60000, cb0)
    assert 180000 * 938 * 8 == 1350720000 <= big < 1.2 * 1350720000        # the bits dominate: 1.35 GB
    two = q(2, 180000, 60000, 0, 0)                                        # two of them: beyond 2^31 bytes
    assert two == expected_ws(2, 180000, 60000, cb0) and two > 2 ** 31
    top = q(1, 1048576, 262144, 2048, 0)
    assert top == expected_ws(1, 1048576, 262144, 2048) and top > 34e9
    assert q(0, 10, 10, 0, 0) == 0 and q(2, 0, 10, 0, 0) == expected_ws(2, 0, 10, cb0)
    for bad in ((63, 0), (96, 0), (-64, 0), (2112, 0), (64, -1)):
        assert q(1, 10, 10, *bad) == -1, bad


def test_c_abi_refuses_outside_the_envelope():
    """Host-side argument checks return TA_ERR_ARG before anything is launched, so they run without a GPU."""
    L = _lib.lib()
    one = C.c_void_p(8)                                                    # never dereferenced: every call below is refused

    def call(ld=29, Cn=29, N=1, mT=10, mJ=5, blank=0, cb=0, fb=0, ws=one, ws_bytes=1 << 20, tr=None, tr_off=None, em=one):
        return L.ta_ctc_align_long_f32(em, ld, Cn, one, one, one, N, mT, mJ, blank, cb, fb, one, one, one, ws, ws_bytes, tr, tr_off, None)

    assert call(N=65) == 1 and call(mT=1048577) == 1 and call(mJ=262145) == 1 and call(Cn=65537, ld=65537) == 1
    assert call(N=-1) == 1 and call(mT=-1) == 1 and call(mJ=-1) == 1 and call(Cn=0) == 1
    assert call(blank=29) == 1 and call(blank=-1) == 1 and call(ld=28) == 1
    assert call(cb=63) == 1 and call(cb=65) == 1 and call(cb=-64) == 1 and call(cb=2048 + 64) == 1 and call(fb=-1) == 1
    assert call(ws_bytes=L.ta_ctc_align_long_workspace_bytes(1, 10, 5, 0, 0) - 1) == 1 and call(ws=None) == 1
    assert call(tr=one, tr_off=None) == 1 and call(em=None) == 1
    assert call(N=0) == 0                                                  # an empty batch is legal and launches nothing


def test_value_errors_name_the_long_limits():
    e = torch.zeros(4, 29)
    al = ForcedAligner.align_long_batch
    with pytest.raises(ValueError, match="at most 262144 tokens"):
        al([e], ["a" * 262145])
    with pytest.raises(ValueError, match="at most 1048576 frames"):
        al([torch.zeros(1048577, 1)[:, :1].expand(1048577, 2)], ["a"])
    with pytest.raises(ValueError, match="65536 classes"):
        al([torch.zeros(1, 65537)], ["a"])
    with pytest.raises(ValueError, match="at most 64 clips"):
        al([e] * 65, ["a"] * 65)
    with pytest.raises(ValueError, match="2 emission matrices but 1 texts"):
        al([e, e], ["a"])
    with pytest.raises(ValueError, match="same number of classes"):
        al([e, torch.zeros(4, 30)], ["a", "b"])
    with pytest.raises(ValueError, match=r"\[frames, classes\]"):
        al([torch.zeros(4)], ["a"])
    with pytest.raises(ValueError, match="col_block 96"):
        al([e], ["a"], col_block=96)
    with pytest.raises(ValueError, match="col_block 4096"):
        al([e], ["a"], col_block=4096)
    with pytest.raises(ValueError, match="frame_block -1"):
        al([e], ["a"], frame_block=-1)
    with pytest.raises(ValueError, match=r"blank_id 29 is outside \[0, 29\)"):
        al([e], ["a"], blank_id=29)
    with pytest.raises(ValueError, match=r"id 29, outside \[0, 29\)"):
        alignment._launch_long([e], [[1, 29]], 0)
    with pytest.raises(ValueError, match="resample first"):
        ForcedAligner.align_long(np.zeros(8000, np.float32), "hi", sample_rate=8000, acoustic_model=object())
    with pytest.raises(ValueError, match="emission=... or acoustic_model="):
        ForcedAligner.align_long(np.zeros(8000, np.float32), "hi")
    assert al([], []) == [] and al([e, e], ["", "7"]) == [[], []]          # nothing to align: no device needed


def test_ops_wrapper_refuses_before_the_library(dry):
    cu1 = torch.tensor([0, 4], dtype=I32)
    args = (torch.zeros(4, 29), cu1, torch.tensor([1], dtype=I32), torch.tensor([0, 1], dtype=I32), 0)
    dry.calls.clear()
    for kw, msg in ((dict(col_block=100), "multiple of 64"), (dict(col_block=2112), "multiple of 64"), (dict(frame_block=-2), "at least 1")):
        with pytest.raises(ValueError, match=msg):
            ops.ctc_align_long(*args, 4, 1, **kw)
    with pytest.raises(ValueError, match="limit of 262144"):
        ops.ctc_align_long(*args, 4, 262145)
    with pytest.raises(ValueError, match="limit of 1048576"):
        ops.ctc_align_long(*args, 1048577, 1)
    with pytest.raises(ValueError, match="limit of 64"):
        ops.ctc_align_long(torch.zeros(4, 29), torch.zeros(66, dtype=I32), torch.zeros(0, dtype=I32), torch.zeros(66, dtype=I32), 0, 4, 1)
    with pytest.raises(ValueError, match="cu_frames holds 2 entries but cu_tokens 3"):
        ops.ctc_align_long(torch.zeros(4, 29), cu1, torch.tensor([1], dtype=I32), torch.tensor([0, 1, 1], dtype=I32), 0, 4, 1)
    assert dry.calls == []


def test_no_cpu_path_for_the_long_trellis(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.Ta355Error, match="no CPU path"):
        ForcedAligner.align_long(None, "hi", emission=torch.zeros(4, 29))
    with pytest.raises(_lib.Ta355Error, match="no CPU path"):
        ops.ctc_align_long(torch.zeros(4, 29), torch.tensor([0, 4], dtype=I32), torch.tensor([1], dtype=I32),
                           torch.tensor([0, 1], dtype=I32), 0, 4, 1)


# ----------------------------------------------------------------------------- operator and plumbing
def test_operator_is_registered_with_a_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from tiny_audio_amd import torch_ops
    assert "ctc_align_long" in torch_ops.OPERATORS and "ctc_align" in torch_ops.OPERATORS
    s = str(torch.ops.ta355.ctc_align_long.default._schema)
    assert s.startswith("ta355::ctc_align_long(Tensor emission, Tensor cu_frames, Tensor tokens, Tensor cu_tokens, SymInt blank_id, "
                        "SymInt max_frames, SymInt max_tokens, SymInt col_block, SymInt frame_block, Tensor? trellis_off, "
                        "SymInt trellis_numel, Tensor(a11!)? workspace)"), s
    assert s.endswith("-> (Tensor, Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        a = (torch.empty(30, 29), torch.empty(4, dtype=I32), torch.empty(11, dtype=I32), torch.empty(4, dtype=I32), 0, 12, 5, 64, 8)
        fr, sc, st, tr = torch.ops.ta355.ctc_align_long(*a, None, 0, None)
        assert fr.shape == (11,) and fr.dtype == I32 and sc.shape == (3,) and sc.dtype == torch.float32
        assert st.shape == (3,) and st.dtype == I32 and tr.shape == (0,)
        tr = torch.ops.ta355.ctc_align_long(*a, torch.empty(3, dtype=torch.int64), 77, torch.empty(4096, dtype=torch.uint8))[3]
        assert tr.shape == (77,) and tr.dtype == torch.float32


def test_dry_run_launches_the_long_entry_point_once_and_never_the_short_one(dry):
    e = torch.zeros(70, 29)
    dry.calls.clear()
    out = ForcedAligner.align_long_batch([e, e[:0], e[:10]], ["hello world", "a b", ""], col_block=64, frame_block=8)
    assert dry.calls == ["ta_ctc_align_long_f32"] and len(out) == 3 and out[2] == []          # one call for the batch
    dry.calls.clear()
    ForcedAligner.align_long(None, "hi there", emission=e)
    assert dry.calls == ["ta_ctc_align_long_f32"]
    dry.calls.clear()
    text = "ab " * 1000                                                                       # 3000 tokens: beyond the short envelope
    ForcedAligner.align_long(None, text, emission=torch.zeros(4000, 29))
    assert dry.calls == ["ta_ctc_align_long_f32"]
    with pytest.raises(ValueError, match="at most 2048 tokens"):                              # the short form still refuses it ...
        ForcedAligner.align(None, text, emission=torch.zeros(4000, 29))
    assert dry.calls == ["ta_ctc_align_long_f32"]                                             # ... and does not dispatch to the long one
    # strided emission rows are passed by their stride, and a caller's workspace by its pointer
    dry.calls.clear()
    wide = torch.zeros(12, 40)
    need = dry.ta_ctc_align_long_workspace_bytes(1, 12, 2, 64, 4)
    fr, sc, st, trs = ops.ctc_align_long(wide[:, :29], torch.tensor([0, 12], dtype=I32), torch.tensor([3, 4], dtype=I32),
                                         torch.tensor([0, 2], dtype=I32), 0, 12, 2, col_block=64, frame_block=4,
                                         workspace=torch.zeros(need, dtype=torch.uint8))
    assert fr.tolist() == [-1, -1] and sc.shape == (1,) and st.shape == (1,) and trs is None and dry.calls == ["ta_ctc_align_long_f32"]
    with pytest.raises(AssertionError):
        ops.ctc_align_long(wide[:, :29], torch.tensor([0, 12], dtype=I32), torch.tensor([3, 4], dtype=I32),
                           torch.tensor([0, 2], dtype=I32), 0, 12, 2, workspace=torch.zeros(need - 1, dtype=torch.uint8))


class _FakeAcoustic:
    """Stands in for Wav2Vec2CtcMI355X in the plumbing test: records the call, returns zeros of the right length."""
    def __init__(self):
        self.calls = []

    def emissions_long(self, wave, window_s=30.0, context_s=2.0, batch_windows=16):
        self.calls.append((len(wave), window_s, context_s))
        return torch.zeros(W.frames_of(len(wave)), 29)


def test_align_long_with_an_acoustic_model_calls_emissions_long(dry):
    m = _FakeAcoustic()
    dry.calls.clear()
    ForcedAligner.align_long(np.zeros(48000, np.float32), "hi there", acoustic_model=m, window_s=20.0, context_s=1.0)
    assert m.calls == [(48000, 20.0, 1.0)] and dry.calls == ["ta_ctc_align_long_f32"]
    with pytest.raises(ValueError, match="at most 262144 tokens"):
        ForcedAligner.align_long(np.zeros(48000, np.float32), "a" * 262145, acoustic_model=m)
    assert len(m.calls) == 1                                               # refused before the acoustic model ran


# ----------------------------------------------------------------------------- the window table
def check_table(n, window, context):
    T = (n - 400) // 320 + 1
    tab = W.long_windows(n, window, context)
    wf, ctx = max(window // 320, 1), context // 320 * 320
    assert tab[0][2] == 0 and tab[-1][3] == T
    for (s0, s1, f0, f1), nxt in zip(tab, tab[1:] + [None]):
        assert f0 < f1 and (nxt is None or nxt[2] == f1)                   # the spans tile [0, T) exactly once, in order
        assert f0 % wf == 0 and (f0 * 320) % 320 == 0 and s0 % 320 == 0    # starts sit on the global frame grid
        assert 0 <= s0 <= f0 * 320 and (f1 - 1) * 320 + 400 <= s1 <= n     # the slice holds every sample its own frames read
        assert s0 == max(0, f0 * 320 - ctx) and s1 == min(n, (f1 - 1) * 320 + 400 + ctx)
        local = W.frames_of(s1 - s0)
        assert f1 - s0 // 320 <= local                                     # the kept frames exist in the slice's own output
    return tab


def test_long_windows_tile_the_recording():
    assert W.FRAME_HOP == 320 == int(np.prod(W.CONV_STRIDE))
    for n, window, context in ((1120000, 320000, 32000), (1120000, 480000, 0), (1120399, 320000, 32000), (100000, 3200, 640),
                               (100001, 3333, 700), (16000 * 60, 16000 * 30, 16000 * 2), (401 + 320 * 7, 320, 0)):
        check_table(n, window, context)
    # 70 s in windows of 20 s with 2 s of context: four windows, the last one of 10 s
    tab = check_table(1120000, 320000, 32000)
    assert tab == [(0, 320080 + 32000, 0, 1000), (288000, 640080 + 32000, 1000, 2000), (608000, 960080 + 32000, 2000, 3000),
                   (928000, 1120000, 3000, 3499)]
    # a recording of at most one window is the whole recording, whatever the context
    assert W.long_windows(320000, 320000, 32000) == [(0, 320000, 0, 999)]
    assert W.long_windows(320080, 320000, 32000) == [(0, 320080, 0, 1000)]
    assert W.long_windows(400, 480000, 32000) == [(0, 400, 0, 1)] and W.long_windows(399, 480000, 32000) == []
    # a last window with fewer than 400 samples of its own holds no frame and is merged into the one before it ...
    two = W.long_windows(2 * 320000 + 399, 320000, 3200)
    assert len(two) == 2 and two[-1] == (320000 - 3200, 2 * 320000 + 399, 1000, 2000)      # its samples: the right context of that one
    # ... and with 400 it is a window of one frame
    three = W.long_windows(2 * 320000 + 400, 320000, 3200)
    assert len(three) == 3 and three[-1] == (640000 - 3200, 640400, 2000, 2001)
    assert W.long_windows(2 * 320000 + 399, 320000, 0)[-1][1] == 640080    # without context the merged tail is simply never read


def test_emissions_long_refuses_what_forward_refuses():
    m = W.Wav2Vec2CtcMI355X(W.Wav2Vec2CtcConfig(hidden_size=256, num_attention_heads=4, intermediate_size=512, conv_dim=128,
                                                num_hidden_layers=1), device="cpu")
    with pytest.raises(ValueError, match="shorter than the 400 samples"):
        m.emissions_long(np.zeros(399, np.float32))
    with pytest.raises(ValueError, match="one 1-D recording"):
        m.emissions_long(np.zeros((2, 8000), np.float32))
    with pytest.raises(ValueError, match="window_s > 0"):
        m.emissions_long(np.zeros(8000, np.float32), window_s=0)


# ----------------------------------------------------------------------------- the short form is where it was
def test_the_short_form_keeps_its_envelope():
    assert ops.ALIGN_LIMITS == {"clips": 4096, "frames": 32768, "tokens": 2048, "classes": 65536}
    assert header_define("TA_ALIGN_MAX_TOKENS") == 2048 and header_define("TA_ALIGN_MAX_FRAMES") == 32768
    with pytest.raises(ValueError, match="at most 2048 tokens"):
        ForcedAligner.align_batch([torch.zeros(4, 29)], ["a" * 2049])
