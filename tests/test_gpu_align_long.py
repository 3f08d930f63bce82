"""-m gpu: the long form of forced alignment (csrc/align_long.hip through torch.ops.ta355.ctc_align_long, ForcedAligner.align_long and
Wav2Vec2CtcMI355X.emissions_long) against tests/align_ref.py (``align(..., fast=True)``; tests/test_alignment_host.py pins
``trellis_fast`` to the literal loop and that to the reference's own outputs) and against the short kernel.  Everything is integers and
single f32 adds, so every comparison is equality of bytes: no tolerance anywhere in this file.

The small shapes are chosen around the two kinds of tile seam at col_block = 64, frame_block = 8: a column seam every 64 trellis
columns (J + 1 = 64, 65, 98), a frame seam every 8 frames (T = 8, 9, 64, 65, 150), the diagonal T == J running through the corners of
the tiles, and tiles that lie wholly above it."""
import numpy as np
import pytest
import torch

from tests import align_ref
from tests.golden import wav2vec2_recipe as R
from tiny_audio_amd import _lib, alignment, ops
from tiny_audio_amd import wav2vec2 as W
from tiny_audio_amd.alignment import ForcedAligner

pytestmark = pytest.mark.gpu

DEV = "cuda"
I32 = torch.int32
SENTINEL = -77
GUARD, FILL = 5, 123.0                  # elements between and after the trellises of a launch, and what the test writes there
CB, FB = 64, 8                          # the smallest tile: every seam within a few dozen cells
_CASES = {}


def ref_case(T, J, C, quantised=False, seed=None):
    """A clip and what tests/align_ref.py makes of it, computed once per shape and shared (never modified) between the tests."""
    key = (T, J, C, quantised, seed)
    if key not in _CASES:
        rng = np.random.default_rng(T * 1000 + J if seed is None else seed)
        if quantised:                                   # few distinct values: many exact ties between staying and moving
            e = (-0.5 * rng.integers(0, 7, (T, C))).astype(np.float32)
        else:
            x = rng.standard_normal((T, C)).astype(np.float32)
            e = (x - np.log(np.exp(x.astype(np.float64)).sum(-1, keepdims=True))).astype(np.float32)
        tokens = rng.integers(1, C, J).tolist()
        r = align_ref.align(e, tokens, fast=True)
        _CASES[key] = dict(e=e, tokens=tokens, trellis=r["trellis"], status=r["status"], frames=r["frames"], score=r["score"])
    return _CASES[key]


def tables(clips):
    Ts, Js = [c[0].shape[0] for c in clips], [len(c[1]) for c in clips]
    cu_f = torch.tensor(np.concatenate([[0], np.cumsum(Ts)]), dtype=I32, device=DEV)
    cu_t = torch.tensor(np.concatenate([[0], np.cumsum(Js)]), dtype=I32, device=DEV)
    tok = torch.tensor([x for c in clips for x in c[1]], dtype=I32, device=DEV)
    em = torch.from_numpy(np.concatenate([c[0] for c in clips], axis=0)).to(DEV)
    return Ts, Js, em, cu_f, tok, cu_t


def launch(clips, col_block=CB, frame_block=FB, blank=0, want_trellis=False, workspace=None, maxima=None, short=False):
    """clips: [(emission ndarray [T, C], tokens list)] -> (frames per clip, score, status, the trellis of every clip or None) on the
    host.  Through ops.ctc_align_long, which is what the operator calls, so that frames can be pre-filled with a sentinel and the
    trellis buffer with FILL; ``short=True`` runs the same tables through ops.ctc_align."""
    Ts, Js, em, cu_f, tok, cu_t = tables(clips)
    frames = torch.full((sum(Js),), SENTINEL, dtype=I32, device=DEV)
    off = buf = None
    numel = 0
    if want_trellis:                              # every trellis is followed by GUARD elements that must keep their fill
        sizes = [(t + 1) * (j + 1) for t, j in zip(Ts, Js)]
        starts = np.concatenate([[0], np.cumsum([s + GUARD for s in sizes])])
        off, numel = torch.tensor(starts[:-1], dtype=torch.int64, device=DEV), int(starts[-1])
        buf = torch.full((numel,), FILL, device=DEV)
    max_T, max_J = (max(Ts), max(Js)) if maxima is None else maxima
    if short:
        fr, sc, st, tr = ops.ctc_align(em, cu_f, tok, cu_t, blank, max_T, max_J, frames=frames, trellis_off=off, trellis_numel=numel,
                                       trellis=buf)
    else:
        fr, sc, st, tr = ops.ctc_align_long(em, cu_f, tok, cu_t, blank, max_T, max_J, col_block=col_block, frame_block=frame_block,
                                            frames=frames, trellis_off=off, trellis_numel=numel, trellis=buf, workspace=workspace)
    torch.cuda.synchronize()
    fr = fr.cpu().tolist()
    cu = np.concatenate([[0], np.cumsum(Js)])
    trs = None
    if want_trellis:
        flat, trs = tr.cpu().numpy(), []
        for n, size in enumerate(sizes):
            trs.append(flat[starts[n]:starts[n] + size].reshape(Ts[n] + 1, Js[n] + 1))
            assert (flat[starts[n] + size:starts[n + 1]] == FILL).all(), f"clip {n} wrote past its trellis"
    return [fr[cu[n]:cu[n + 1]] for n in range(len(clips))], sc.cpu().numpy(), st.cpu().tolist(), trs


def check_clip(got_frames, got_score, got_status, want):
    assert got_status == want["status"]
    assert got_score.tobytes() == np.float32(want["score"]).tobytes()
    assert got_frames == (want["frames"] if want["status"] == 0 else [SENTINEL] * len(want["tokens"]))
    if want["status"] == 0 and want["tokens"]:
        f = got_frames
        assert all(b > a for a, b in zip(f, f[1:])) and 0 <= f[0] and f[-1] < want["e"].shape[0]


# ----------------------------------------------------------------------------- 1. tile seams at the smallest shapes
SEAMS = [(150, 97), (64, 63), (65, 64), (8, 5), (9, 5),        # the issue's list: both seams, one short of them and one past them
         (64, 64), (97, 97), (130, 128),                       # T == J: the diagonal only (and two frames of slack across two seams)
         (30, 70), (63, 64), (0, 3),                           # T < J: status 1; the second one frame short, at the seam
         (20, 0), (1, 1)]                                      # J = 0: one column of blank sums; the smallest trellis


@pytest.mark.parametrize("quantised", [False, True], ids=["random", "ties"])
@pytest.mark.parametrize("T,J", SEAMS, ids=[f"{t}x{j}" for t, j in SEAMS])
def test_tile_seams(T, J, quantised):
    c = ref_case(T, J, 6 if quantised else 29, quantised)
    fr, sc, st, tr = launch([(c["e"], c["tokens"])], want_trellis=True)
    assert tr[0].tobytes() == c["trellis"].tobytes()
    check_clip(fr[0], sc[0], st[0], c)
    assert c["status"] == int(T < J)
    fr, sc, st, _ = launch([(c["e"], c["tokens"])])                        # and without the trellis output
    check_clip(fr[0], sc[0], st[0], c)


def test_the_quantised_cases_cross_ties_at_the_seams():
    """The ties the tie rule is about exist where the seams are: in the quantised (150, 97) case there are cells with move == stay in
    the first column of the second column block (its move operand comes through the column carry) and in the first frame of a frame
    block (both operands come through the row carry), and the path takes some tie."""
    c = ref_case(150, 97, 6, True)
    tr, e, tok = c["trellis"], c["e"], c["tokens"]
    col = row = on_path = 0
    for t in range(150):
        for j in range(1, 98):
            stay, move = np.float32(tr[t, j] + e[t, 0]), np.float32(tr[t, j - 1] + e[t, tok[j - 1]])
            if np.isfinite(stay) and stay == move:
                col += j == CB
                row += t % FB == 0
                on_path += c["frames"][j - 1] == t
    assert col >= 1 and row >= 5 and on_path >= 1, (col, row, on_path)


def test_a_token_id_outside_the_classes_is_refused_and_nothing_else_is_written():
    a = ref_case(150, 97, 29)
    neg = np.float32(-np.inf).tobytes()
    for bad_id, where in ((29, 80), (-1, 3), (29, 96)):                    # in the second column block, in the first, the last token
        bad = list(a["tokens"])
        bad[where] = bad_id
        fr, sc, st, tr = launch([(a["e"], a["tokens"]), (a["e"], bad), (a["e"], a["tokens"])], want_trellis=True)
        assert st == [0, 2, 0] and sc[1].tobytes() == neg and fr[1] == [SENTINEL] * 97 and (tr[1] == FILL).all()
        for n in (0, 2):
            check_clip(fr[n], sc[n], st[n], a)
            assert tr[n].tobytes() == a["trellis"].tobytes()
    # a clip beyond the maxima the caller declared (they size the workspace) is refused the same way
    b = ref_case(64, 63, 29)
    for maxima in ((64, 97), (150, 63)):
        fr, sc, st, tr = launch([(b["e"], b["tokens"]), (a["e"], a["tokens"]), (b["e"], b["tokens"])], want_trellis=True, maxima=maxima)
        assert st == [0, 2, 0] and sc[1].tobytes() == neg and fr[1] == [SENTINEL] * 97 and (tr[1] == FILL).all()
        for n in (0, 2):
            check_clip(fr[n], sc[n], st[n], b)
            assert tr[n].tobytes() == b["trellis"].tobytes()


# ----------------------------------------------------------------------------- 2. one tile == the short kernel
@pytest.mark.parametrize("T,J,C,quantised", [(150, 97, 29, False), (150, 97, 6, True), (300, 130, 29, False), (30, 70, 29, False)])
def test_one_tile_gives_the_short_kernels_bytes(T, J, C, quantised):
    c = ref_case(T, J, C, quantised)
    _, _, em, cu_f, tok, cu_t = tables([(c["e"], c["tokens"])])
    off, numel = torch.zeros(1, dtype=torch.int64, device=DEV), (T + 1) * (J + 1)
    short = torch.ops.ta355.ctc_align(em, cu_f, tok, cu_t, 0, T, J, off, numel)
    long_ = torch.ops.ta355.ctc_align_long(em, cu_f, tok, cu_t, 0, T, J, 2048, 512, off, numel, None)
    assert J + 1 <= 2048 and T <= 512
    for name, a, b in zip(("frames", "score", "status", "trellis"), short, long_):
        assert a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), name
    assert long_[3].cpu().numpy().tobytes() == c["trellis"].tobytes() and long_[2].tolist() == [c["status"]]


def test_operator_returns_fresh_outputs_and_passes_opcheck():
    c, d = ref_case(150, 97, 6, True), ref_case(8, 5, 6, True)
    Ts, Js, em, cu_f, tok, cu_t = tables([(c["e"], c["tokens"]), (d["e"][:3], d["tokens"])])          # the second one fails: T = 3 < 5
    args = (em, cu_f, tok, cu_t, 0, 150, 97, CB, FB)
    fr, sc, st, tr = torch.ops.ta355.ctc_align_long(*args, None, 0, None)
    assert fr.tolist() == c["frames"] + [-1] * 5 and st.tolist() == [0, 1] and tr.numel() == 0
    off = torch.tensor([0, 151 * 98], dtype=torch.int64, device=DEV)
    ws = torch.empty(_lib.lib().ta_ctc_align_long_workspace_bytes(2, 150, 97, CB, FB), dtype=torch.uint8, device=DEV)
    tr = torch.ops.ta355.ctc_align_long(*args, off, 151 * 98 + 4 * 6, ws)[3]
    assert tr[:151 * 98].cpu().numpy().tobytes() == c["trellis"].tobytes()
    torch.library.opcheck(torch.ops.ta355.ctc_align_long, (*args, None, 0, None), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.ta355.ctc_align_long, (*args, off, 151 * 98 + 24, ws), test_utils=("test_schema", "test_faketensor"))


# ----------------------------------------------------------------------------- 3. ragged batch
def test_ragged_batch_equals_the_clips_one_by_one():
    """Clips of 2 x 19, 1 x 1, 2 x 4 (fails), 3 x 38 and 1 x 3 (J = 0) tiles in one call: per clip the same outputs as alone; the frames
    slots of the failed clip keep the sentinel; the trellises land at their offsets and the guard elements keep their fill."""
    cs = [ref_case(150, 97, 29), ref_case(8, 5, 29), ref_case(30, 70, 29), ref_case(300, 130, 29), ref_case(20, 0, 29)]
    clips = [(c["e"], c["tokens"]) for c in cs]
    fr, sc, st, tr = launch(clips, want_trellis=True)
    assert st == [0, 0, 1, 0, 0]
    for n, c in enumerate(cs):
        check_clip(fr[n], sc[n], st[n], c)
        assert tr[n].tobytes() == c["trellis"].tobytes(), n
    fr, sc, st, _ = launch(clips[::-1])                                    # the other order, without the trellis
    for n, c in enumerate(cs[::-1]):
        check_clip(fr[n], sc[n], st[n], c)


# ----------------------------------------------------------------------------- 4. beyond the old envelope
def test_beyond_the_old_envelope_with_the_default_tiles():
    """T = 6000 frames against J = 3000 tokens, C = 32, the default tile: more tokens than ta_ctc_align_f32 takes."""
    c = ref_case(6000, 3000, 32)
    assert c["status"] == 0 and len(c["tokens"]) > ops.ALIGN_LIMITS["tokens"]
    fr, sc, st, _ = launch([(c["e"], c["tokens"])], col_block=0, frame_block=0)
    check_clip(fr[0], sc[0], st[0], c)
    with pytest.raises(ValueError, match="limit of 2048"):
        launch([(c["e"], c["tokens"])], short=True)


def test_decision_bits_beyond_two_gigabytes():
    """Eight clips whose decision bits take 8 x 1 000 000 x 47 words = 3.0 GB: every index into the last clip's bits lies past 2^31
    bytes.  Clip 0 is one trellis column over 1 000 000 frames (J = 0: its score is the sum of the blanks, multiples of 0.25 that f32
    adds exactly); clips 1 .. 6 are one frame; clip 7 is the 6 000 x 3 000 case, against align_ref."""
    rng = np.random.default_rng(5)
    e0 = np.full((1000000, 32), -1.0, np.float32)
    e0[:, 0] = -0.25 * rng.integers(1, 5, 1000000)
    c = ref_case(6000, 3000, 32)
    one = ref_case(1, 1, 29)["e"][:, :1].repeat(32, axis=1)
    clips = [(e0, [])] + [(one, [])] * 6 + [(c["e"], c["tokens"])]
    fr, sc, st, _ = launch(clips, col_block=256, frame_block=1024)
    assert st == [0] * 8 and float(sc[0]) == float(e0[:, 0].astype(np.float64).sum()) and fr[0] == []
    assert all(s.tobytes() == one[0, 0].tobytes() for s in sc[1:7])
    assert 7 * 1000000 * 47 * 8 > 2 ** 31 and _lib.lib().ta_ctc_align_long_workspace_bytes(8, 1000000, 3000, 256, 1024) > 3e9
    check_clip(fr[7], sc[7], st[7], c)


# ----------------------------------------------------------------------------- 5. trellis_out
def test_trellis_out_equals_the_reference_trellis():
    for quantised in (False, True):
        c = ref_case(150, 97, 6 if quantised else 29, quantised)
        for cb, fb in ((64, 8), (64, 1), (128, 7), (64, 150)):
            tr = launch([(c["e"], c["tokens"])], col_block=cb, frame_block=fb, want_trellis=True)[3]
            assert tr[0].shape == (151, 98) and tr[0].tobytes() == c["trellis"].tobytes(), (quantised, cb, fb)


# ----------------------------------------------------------------------------- 6. poisoned workspace and carries
@pytest.mark.parametrize("pattern", ["ff", "quiet_nan"])
def test_results_do_not_depend_on_what_the_workspace_held(pattern):
    """Every word of the workspace -- decision bits, both carries, the flags -- is a NaN bit pattern before the call (all ones, or
    f32's quiet NaN 0x7fc00000), and twice the needed size is handed over: the results are the reference's, and nothing behind the
    needed size is written."""
    cs = [ref_case(150, 97, 6, True), ref_case(30, 70, 29), ref_case(300, 130, 29)]
    cs[0] = dict(cs[0], e=np.concatenate([cs[0]["e"], np.zeros((150, 23), np.float32)], axis=1))      # C = 6 rides in the C = 29 batch
    need = _lib.lib().ta_ctc_align_long_workspace_bytes(3, 300, 130, CB, FB)
    assert need % 4 == 0
    if pattern == "ff":
        ws = torch.full((2 * need,), 0xFF, dtype=torch.uint8, device=DEV)
    else:
        ws = torch.full((need // 2,), float("nan"), dtype=torch.float32, device=DEV).view(torch.uint8)
    assert ws.numel() == 2 * need and torch.isnan(ws.view(torch.float32)).all()
    before = ws[need:].clone()
    fr, sc, st, tr = launch([(c["e"], c["tokens"]) for c in cs], want_trellis=True, workspace=ws)
    for n, c in enumerate(cs):
        check_clip(fr[n], sc[n], st[n], c)
        assert tr[n].tobytes() == c["trellis"].tobytes(), n
    assert torch.equal(ws[need:], before), "the call wrote past the workspace it asked for"


# ----------------------------------------------------------------------------- 7. two tilings of one input
def test_the_tiling_does_not_change_a_byte():
    c = ref_case(700, 300, 6, True)
    want = None
    for cb, fb in ((64, 8), (128, 100), (256, 33), (320, 700), (2048, 1), (0, 0)):
        fr, sc, st, tr = launch([(c["e"], c["tokens"])], col_block=cb, frame_block=fb, want_trellis=True)
        got = (fr[0], sc[0].tobytes(), st[0], tr[0].tobytes())
        want = want or got
        assert got == want, (cb, fb)
    check_clip(want[0], np.frombuffer(want[1], np.float32)[0], want[2], c)
    assert want[3] == c["trellis"].tobytes()


# ----------------------------------------------------------------------------- 8. end to end
def clip(n, seed):
    """A deterministic 16 kHz recording of n samples: two tones, noise and a DC offset."""
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.15 * np.sin(2 * np.pi * 220.0 * t + seed) + 0.07 * np.sin(2 * np.pi * 1900.0 * t) + 0.03 * g.standard_normal(n) + 0.02).astype(np.float32)


@pytest.fixture(scope="module")
def recording():
    m = W.Wav2Vec2CtcMI355X(W.Wav2Vec2CtcConfig(**R.GEOMS["a"], n_classes=29), device=DEV)
    m.load_state_dict_hf(R.weights("a"), labels="torchaudio")
    wave = clip(70 * 16000, 123)
    E = m.emissions_long(wave, window_s=20.0)
    torch.cuda.synchronize()
    return m, wave, E


def test_emissions_long_is_forward_on_the_windows(recording):
    m, wave, E = recording
    n = len(wave)
    T = (n - 400) // 320 + 1
    assert E.shape == (T, 29) and E.dtype == torch.float32 and E.is_cuda and T == 3499
    table = W.long_windows(n, 20 * 16000, 2 * 16000)
    assert len(table) == 4
    w = torch.from_numpy(wave)
    for group, got in ((16, E), (3, m.emissions_long(wave, window_s=20.0, batch_windows=3))):
        for i in range(0, 4, group):
            part = table[i:i + group]
            em, Ts = m([w[s0:s1] for s0, s1, _, _ in part])                # the same windows in the same grouping
            row = 0
            for (s0, s1, f0, f1), t in zip(part, Ts):
                assert t == W.frames_of(s1 - s0)
                lo = row + f0 - s0 // 320
                assert torch.equal(got[f0:f1], em[lo:lo + f1 - f0]), (group, f0)
                row += t
    assert torch.isfinite(E).all() and torch.allclose(E.exp().sum(-1), torch.ones(T, device=DEV), atol=1e-4)
    # a recording no longer than one window is one forward call: the same bytes
    short = wave[:5 * 16000 + 123]
    assert torch.equal(m.emissions_long(short, window_s=20.0), m([short])[0])
    assert torch.equal(m.emissions_long(wave[:20 * 16000], window_s=20.0), m([wave[:20 * 16000]])[0])


def test_align_long_end_to_end(recording):
    m, wave, E = recording
    rng = np.random.default_rng(9)
    letters = np.array(list("ETAOINSHRDLU'"))
    words = ["".join(rng.choice(letters, int(rng.integers(1, 9)))) for _ in range(520)]
    words[100] = "42"                                                      # no alignable character: the labels after it shift
    text = "  ".join(words[:3]) + " " + " ".join(words[3:]).lower()        # a doubled separator: skipped while no word is open
    dictionary = ForcedAligner._dict()
    tokens = alignment._tokenize(text, dictionary)
    assert 2048 < len(tokens) <= E.shape[0]
    r = align_ref.align(E.cpu().numpy(), tokens, fast=True)
    assert r["status"] == 0
    spans = alignment._spans(tokens, r["frames"], False, E.shape[0])
    want = alignment._group_words(text, spans, dictionary, 320 / 16000, ForcedAligner.START_OFFSET, ForcedAligner.END_OFFSET)
    got = ForcedAligner.align_long(None, text, emission=E)
    assert got == want and len(got) == 519 and all(g["end"] > g["start"] for g in got)
    assert ForcedAligner.align_long_batch([E.cpu(), E[:100]], [text, "it's short"], col_block=128, frame_block=50)[0] == want
    assert ForcedAligner.align_long(wave, text, acoustic_model=m, window_s=20.0) == want
    with pytest.raises(ValueError, match="at most 2048 tokens"):           # the short form refuses the same call, as before
        ForcedAligner.align(None, text, emission=E)
    # a clip that cannot be aligned falls back to uniform spans, as align_batch does
    few = ForcedAligner.align_long_batch([E[:5]], ["hello world"])[0]
    assert few == ForcedAligner.align_batch([E[:5]], ["hello world"])[0] and len(few) == 2
