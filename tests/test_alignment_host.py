"""-m "not gpu": forced alignment off the device.  tests/align_ref.py (the definition the kernel is held to) against the
reference's own outputs in tests/golden/alignment.npz, the host half of tiny_audio_amd/alignment.py (tokenisation, fallback, word
grouping) against the reference's word lists, and the library boundary: header, workspace query, refusals, operator, dry run."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import align_ref
from tiny_audio_amd import _lib, alignment, ops
from tiny_audio_amd.alignment import ForcedAligner

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = json.load(open(os.path.join(GOLDEN, "alignment.json")))
DICT = {c: i for i, c in enumerate(alignment.LABELS)}


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "alignment.npz"))


@pytest.fixture
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


def case(fx, name):
    return fx[name + ".emission"], fx[name + ".tokens"].tolist(), fx[name + ".trellis"], [tuple(r) for r in fx[name + ".spans"].tolist()]


# ----------------------------------------------------------------------------- the definition against the reference
def test_fixture_holds_the_cases():
    want = {"g_1x1", "g_3x3", "g_2x3", "g_0x2", "g_65x1", "g_64x64", "g_70x65", "g_300x130", "q_40x12", "q_70x65", "q_130x40",
            "inf_60x10", "dead_20x5"}
    assert set(META["cases"]) == want
    assert {w["key"] for w in META["words"]} == {"plain", "spaces", "edges", "apostrophe", "digits", "lower", "empty", "unalignable",
                                                 "only_separator", "fallback"}
    assert os.path.getsize(os.path.join(GOLDEN, "alignment.npz")) < 256 * 1024


@pytest.mark.parametrize("name", META["cases"])
def test_align_ref_equals_the_reference_bit_for_bit(fx, name):
    e, tokens, tr, sp = case(fx, name)
    assert tr.shape == (e.shape[0] + 1, len(tokens) + 1) and tr.dtype == np.float32 and tr[0, 0] == 0
    got = align_ref.align(e, tokens)
    assert got["trellis"].tobytes() == tr.tobytes()                       # every bit, the -inf pattern included
    fast = align_ref.align(e, tokens, fast=True)
    assert fast["trellis"].tobytes() == tr.tobytes() and fast["frames"] == got["frames"] and fast["status"] == got["status"]
    assert got["status"] == int(np.isneginf(tr[-1, -1]))
    spans = align_ref.spans(tokens, got["status"], got["frames"], e.shape[0])
    assert spans == [(int(a), b, c) for a, b, c in sp] and len(spans) == len(tokens)       # one span per token
    if got["status"] == 0 and tokens:
        f = got["frames"]
        assert all(b > a for a, b in zip(f, f[1:])) and 0 <= f[0] and f[-1] < e.shape[0]


def test_fixture_pins_the_tie_rule(fx):
    """Quantised emissions make exact ties; the path the reference took crosses some, so `move >= stay` (not `>`) is pinned."""
    met = {}
    for name in ("q_40x12", "q_70x65", "q_130x40"):
        e, tokens, tr, _ = case(fx, name)
        r = align_ref.align(e, tokens)
        ties = on_path = 0
        for t in range(e.shape[0]):
            for j in range(1, len(tokens) + 1):
                stay, move = np.float32(tr[t, j] + e[t, 0]), np.float32(tr[t, j - 1] + e[t, tokens[j - 1]])
                tie = np.isfinite(stay) and stay == move
                ties += tie
                on_path += tie and r["frames"][j - 1] == t       # a tie the walk meets is taken as a move: token j - 1 sits at t
        met[name] = (int(ties), int(on_path))
    assert all(v[0] >= 20 for v in met.values()), met
    assert met["q_40x12"][1] >= 1 and met["q_130x40"][1] >= 1, met


# ----------------------------------------------------------------------------- the host half of the module
@pytest.mark.parametrize("w", META["words"], ids=[w["key"] for w in META["words"]])
def test_words_equal_the_reference(fx, w):
    e = fx[w["emission"] + ".emission"]
    tokens = alignment._tokenize(w["text"], DICT)
    if not tokens:
        assert w["words"] == [] and ForcedAligner.align(None, w["text"], emission=torch.from_numpy(e)) == []
        return
    r = align_ref.align(e, tokens, fast=True)
    spans = alignment._spans(tokens, r["frames"], r["status"] == 1, e.shape[0])
    assert spans == align_ref.spans(tokens, r["status"], r["frames"], e.shape[0])
    got = alignment._group_words(w["text"], spans, DICT, 320 / 16000, ForcedAligner.START_OFFSET, ForcedAligner.END_OFFSET)
    assert got == w["words"]                                               # Python floats, exactly
    assert (r["status"] == 1) == (w["key"] == "fallback")


def test_tokenisation_quirks():
    assert alignment._tokenize("Ab c", DICT) == [DICT["A"], DICT["B"], DICT["|"], DICT["C"]]
    assert alignment._tokenize("a  b", DICT).count(DICT["|"]) == 2 and alignment._tokenize("42!!", DICT) == []
    assert alignment._tokenize("it's", DICT)[2] == DICT["'"]
    assert len(alignment.LABELS) == 29 and alignment.LABELS[:3] == ("-", "|", "E") and alignment.LABELS[-1] == "Z"
    assert ForcedAligner.START_OFFSET == 0.06 and ForcedAligner.END_OFFSET == -0.03
    # a word with no alignable character keeps its slot in text.split(): the labels after it shift
    spans = [(DICT["A"], 0.0, 1.0), (DICT["|"], 1.0, 2.0), (DICT["|"], 2.0, 3.0), (DICT["B"], 5.0, 6.0)]
    got = alignment._group_words("a 42 b", spans, DICT, 0.02, 0.06, -0.03)
    assert [g["word"] for g in got] == ["a", "42"] and got[1]["start"] == max(0.0, 5.0 * 0.02 - 0.06)


def test_reference_assertions_that_need_no_kernel():
    assert ForcedAligner._backtrack(torch.zeros(6, 1), torch.zeros(5, 29), []) == []              # empty tokens
    tr = torch.full((3, 4), -float("inf"))                                                         # T = 2 < J = 3: fallback
    got = ForcedAligner._backtrack(tr, torch.zeros(2, 29), [5, 6, 7])
    assert got == [(5, 0.0, 2 / 3), (6, 2 / 3, 2 * (2 / 3)), (7, 2 * (2 / 3), 3 * (2 / 3))]
    assert ForcedAligner._backtrack(torch.full((1, 3), -float("inf")), torch.zeros(0, 29), [1, 2]) == [(1, 0.0, 0.0), (2, 0.0, 0.0)]
    assert ForcedAligner.align(np.zeros(16000, np.float32), "", emission=torch.zeros(5, 29)) == []
    assert ForcedAligner.align_batch([], []) == []
    assert ForcedAligner.align_batch([torch.zeros(5, 29)] * 2, ["", "7"]) == [[], []]


def test_no_cpu_path_for_the_trellis(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.Ta355Error, match="no CPU path"):
        ForcedAligner._get_trellis(torch.zeros(4, 29), [1, 2])
    with pytest.raises(_lib.Ta355Error, match="no CPU path"):
        ForcedAligner.align(None, "hi", emission=torch.zeros(4, 29))
    with pytest.raises(_lib.Ta355Error):
        ops.ctc_align(torch.zeros(4, 29), torch.tensor([0, 4], dtype=torch.int32), torch.tensor([1], dtype=torch.int32),
                      torch.tensor([0, 1], dtype=torch.int32), 0, 4, 1)


def test_align_without_torchaudio_raises_import_error(monkeypatch):
    monkeypatch.setitem(sys.modules, "torchaudio", None)                   # "not installed", whatever the box has
    monkeypatch.setattr(ForcedAligner, "_model", None)
    with pytest.raises(ImportError, match="torchaudio is not installed"):
        ForcedAligner.align(np.zeros(16000, np.float32), "hello")
    with pytest.raises(ImportError, match="torchaudio is not installed"):
        ForcedAligner.get_instance("cpu")


# ----------------------------------------------------------------------------- refusals
def test_value_errors_name_the_limit():
    e = torch.zeros(4, 29)
    with pytest.raises(ValueError, match=r"id 29, outside \[0, 29\)"):
        ForcedAligner._get_trellis(e, [1, 29])
    with pytest.raises(ValueError, match=r"id -1, outside"):
        ForcedAligner._get_trellis(e, [-1])
    with pytest.raises(ValueError, match=r"blank_id 29 is outside \[0, 29\)"):
        ForcedAligner._get_trellis(e, [1], blank_id=29)
    with pytest.raises(ValueError, match="at most 2048 tokens"):
        ForcedAligner._get_trellis(e, [1] * 2049)
    with pytest.raises(ValueError, match="at most 32768 frames"):
        ForcedAligner._get_trellis(torch.zeros(32769, 2), [1])
    with pytest.raises(ValueError, match="65536 classes"):
        ForcedAligner._get_trellis(torch.zeros(1, 65537), [1])
    with pytest.raises(ValueError, match="at most 4096 clips"):
        ForcedAligner.align_batch([torch.zeros(1, 29)] * 4097, ["a"] * 4097)
    with pytest.raises(ValueError, match="2 emission matrices but 1 texts"):
        ForcedAligner.align_batch([e, e], ["a"])
    with pytest.raises(ValueError, match="same number of classes"):
        ForcedAligner.align_batch([e, torch.zeros(4, 30)], ["a", "b"])
    with pytest.raises(ValueError, match=r"\[frames, classes\]"):
        ForcedAligner._get_trellis(torch.zeros(4), [1])


def test_c_abi_refuses_outside_the_envelope():
    """Host-side argument checks return TA_ERR_ARG before anything is launched, so they run without a GPU."""
    L = _lib.lib()
    one = C.c_void_p(8)                                                    # never dereferenced: every call below is refused

    def call(ld=29, Cn=29, N=1, mT=10, mJ=5, blank=0, ws=one, ws_bytes=1 << 20, tr=None, tr_off=None, em=one):
        return L.ta_ctc_align_f32(em, ld, Cn, one, one, one, N, mT, mJ, blank, one, one, one, ws, ws_bytes, tr, tr_off, None)

    assert call(N=4097) == 1 and call(mT=32769) == 1 and call(mJ=2049) == 1 and call(Cn=65537, ld=65537) == 1
    assert call(N=-1) == 1 and call(mT=-1) == 1 and call(mJ=-1) == 1 and call(Cn=0) == 1
    assert call(blank=29) == 1 and call(blank=-1) == 1 and call(ld=28) == 1
    assert call(ws_bytes=L.ta_ctc_align_workspace_bytes(1, 10, 5) - 1) == 1 and call(ws=None) == 1
    assert call(tr=one, tr_off=None) == 1 and call(em=None) == 1
    assert call(N=0) == 0                                                  # an empty batch is legal and launches nothing


def test_header_and_workspace_query():
    text = open(_lib.HEADER).read()
    for d in ("#define TA_ALIGN_MAX_TOKENS 2048", "#define TA_ALIGN_MAX_FRAMES 32768", "#define TA_ALIGN_MAX_CLASSES 65536",
              "#define TA_ALIGN_MAX_CLIPS 4096", "tiny_audio/alignment.py:47-152", "tiny_audio/asr_pipeline.py:117-131"):
        assert d in text, d
    assert ops.ALIGN_LIMITS == {"clips": 4096, "frames": 32768, "tokens": 2048, "classes": 65536}
    protos = _lib.parse_header()
    assert len(protos["ta_ctc_align_f32"][1]) == 18 and protos["ta_ctc_align_workspace_bytes"][0] is C.c_long
    L = _lib.lib()
    assert L.ta_version() == 4
    q = L.ta_ctc_align_workspace_bytes
    # one 64-bit word of decision bits per frame and per 64 trellis columns (J + 1 of them)
    assert q(1, 1, 1) == 8 and q(1, 100, 62) == 800 and q(1, 100, 63) == 800 and q(1, 100, 64) == 1600
    assert q(32, 1499, 400) == 32 * 1499 * 7 * 8 and q(1, 32768, 2048) == 32768 * 33 * 8
    assert q(0, 10, 10) == 0 and q(3, 0, 10) == 0 and q(2, 10, 0) == 2 * 10 * 8


# ----------------------------------------------------------------------------- operator and plumbing
def test_operator_is_registered_with_a_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from tiny_audio_amd import torch_ops
    assert "ctc_align" in torch_ops.OPERATORS
    s = str(torch.ops.ta355.ctc_align.default._schema)
    assert s.startswith("ta355::ctc_align(Tensor emission, Tensor cu_frames, Tensor tokens, Tensor cu_tokens, SymInt blank_id, "
                        "SymInt max_frames, SymInt max_tokens, Tensor? trellis_off, SymInt trellis_numel)"), s
    assert s.endswith("-> (Tensor, Tensor, Tensor, Tensor)")
    i32 = torch.int32
    with FakeTensorMode():
        a = (torch.empty(30, 29), torch.empty(4, dtype=i32), torch.empty(11, dtype=i32), torch.empty(4, dtype=i32), 0, 12, 5)
        fr, sc, st, tr = torch.ops.ta355.ctc_align(*a, None, 0)
        assert fr.shape == (11,) and fr.dtype == i32 and sc.shape == (3,) and sc.dtype == torch.float32
        assert st.shape == (3,) and st.dtype == i32 and tr.shape == (0,)
        tr = torch.ops.ta355.ctc_align(*a, torch.empty(3, dtype=torch.int64), 77)[3]
        assert tr.shape == (77,) and tr.dtype == torch.float32


def test_dry_run_marshals_through_the_real_prototypes(dry, fx):
    e = torch.from_numpy(fx["g_70x65.emission"])
    tokens = fx["g_70x65.tokens"].tolist()
    dry.calls.clear()
    tr = ForcedAligner._get_trellis(e, tokens)
    assert tr.shape == (71, 66) and tr.dtype == torch.float32 and tr.device.type == "cpu"
    assert dry.calls == ["ta_ctc_align_f32"]
    dry.calls.clear()
    out = ForcedAligner.align_batch([e, e[:0], e[:10]], ["hello world", "a b", ""])
    assert dry.calls == ["ta_ctc_align_f32"] and len(out) == 3 and out[2] == []      # one launch for the batch
    dry.calls.clear()
    ForcedAligner.align(None, "hi there", emission=e, log_softmax=True)
    assert dry.calls == ["ta_ctc_align_f32"]
    # strided emission rows are passed by their stride, not copied
    wide = torch.zeros(12, 40)
    fr, sc, st, trs = ops.ctc_align(wide[:, :29], torch.tensor([0, 12], dtype=torch.int32), torch.tensor([3, 4], dtype=torch.int32),
                                    torch.tensor([0, 2], dtype=torch.int32), 0, 12, 2)
    assert fr.tolist() == [-1, -1] and sc.shape == (1,) and st.shape == (1,) and trs is None
