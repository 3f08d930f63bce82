"""-m gpu: forced alignment on the device (csrc/align.hip through torch.ops.ta355.ctc_align and tiny_audio_amd/alignment.py) against
the reference's own outputs in tests/golden/alignment.npz and against tests/align_ref.py.  Everything is integers and single f32
adds, so every comparison is equality: no tolerance anywhere in this file."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import align_ref
from tiny_audio_amd import _lib, ops
from tiny_audio_amd.alignment import ForcedAligner

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = json.load(open(os.path.join(GOLDEN, "alignment.json")))
DEV = "cuda"
I32 = torch.int32
SENTINEL = -77
_HDR = open(_lib.HEADER).read()
THREADS, FRAME_BLOCK, STAGE = (int(re.search(rf"#define TA_ALIGN_{k} (\d+)", _HDR).group(1))
                               for k in ("THREADS", "FRAME_BLOCK", "STAGE_FLOATS"))       # the kernel's own constants
GUARD, FILL = 5, 123.0                  # elements between and after the trellises of a launch, and what the test writes there


def frame_block(J):
    """Frames staged per block for a clip of J tokens (csrc/align.hip)."""
    return min(FRAME_BLOCK, STAGE // (J + 1))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "alignment.npz"))


def case(fx, name):
    e, tokens, tr = fx[name + ".emission"], fx[name + ".tokens"].tolist(), fx[name + ".trellis"]
    spans = [tuple(r) for r in fx[name + ".spans"].tolist()]
    failed = bool(np.isneginf(tr[-1, -1]))
    frames = [] if failed else [int(s[1]) for s in spans]
    return dict(e=e, tokens=tokens, trellis=tr, spans=[(int(a), b, c) for a, b, c in spans], status=int(failed), frames=frames,
                score=tr[-1, -1])


def launch(clips, blank=0, want_trellis=False, emission=None, maxima=None):
    """clips: [(emission ndarray [T, C], tokens list)] -> the operator's outputs on the host (frames per clip, score, status, the
    trellis of every clip or None).  frames are pre-filled with a sentinel, the trellis buffer with FILL."""
    Ts, Js = [c[0].shape[0] for c in clips], [len(c[1]) for c in clips]
    cu_f = torch.tensor(np.concatenate([[0], np.cumsum(Ts)]), dtype=I32, device=DEV)
    cu_t = torch.tensor(np.concatenate([[0], np.cumsum(Js)]), dtype=I32, device=DEV)
    tok = torch.tensor([x for c in clips for x in c[1]], dtype=I32, device=DEV)
    if emission is None:
        emission = torch.from_numpy(np.concatenate([c[0] for c in clips], axis=0)).to(DEV)
    frames = torch.full((sum(Js),), SENTINEL, dtype=I32, device=DEV)
    off = buf = None
    numel = 0
    if want_trellis:                              # every trellis is followed by GUARD elements that must keep their fill
        sizes = [(t + 1) * (j + 1) for t, j in zip(Ts, Js)]
        starts = np.concatenate([[0], np.cumsum([s + GUARD for s in sizes])])
        off, numel = torch.tensor(starts[:-1], dtype=torch.int64, device=DEV), int(starts[-1])
        buf = torch.full((numel,), FILL, device=DEV)
    max_T, max_J = (max(Ts), max(Js)) if maxima is None else maxima
    fr, sc, st, tr = ops.ctc_align(emission, cu_f, tok, cu_t, blank, max_T, max_J, frames=frames, trellis_off=off,
                                   trellis_numel=numel, trellis=buf)
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


# ----------------------------------------------------------------------------- the reference's outputs, case by case
@pytest.mark.parametrize("name", META["cases"])
def test_trellis_equals_the_reference(fx, name):
    c = case(fx, name)
    tr = ForcedAligner._get_trellis(torch.from_numpy(c["e"]), c["tokens"])
    assert tr.device.type == "cpu" and tr.dtype == torch.float32 and tr.shape == c["trellis"].shape and tr[0, 0] == 0
    assert torch.equal(tr, torch.from_numpy(c["trellis"]))
    assert tr.numpy().tobytes() == c["trellis"].tobytes()                  # finite sums and -inf have one encoding each
    spans = ForcedAligner._backtrack(tr, torch.from_numpy(c["e"]).to(DEV), c["tokens"])
    assert spans == c["spans"] and len(spans) == len(c["tokens"])


@pytest.mark.parametrize("name", META["cases"])
def test_operator_equals_the_reference(fx, name):
    c = case(fx, name)
    fr, sc, st, _ = launch([(c["e"], c["tokens"])])
    check_clip(fr[0], sc[0], st[0], c)


def test_batch_equals_the_clips_one_by_one(fx):
    """All cases in one ragged launch, with a J = 0 clip in the middle: per clip the same outputs as alone; the frames slots of
    failed clips keep the sentinel; the trellises land at their offsets, and the guard elements that ``launch`` leaves after each
    of them keep their fill."""
    cs = [case(fx, n) for n in META["cases"]]
    e7 = fx["g_65x1.emission"][:7]                                        # J = 0: one trellis column of blank sums, status 0
    r = align_ref.align(e7, [])
    empty = dict(e=e7, tokens=[], trellis=r["trellis"], status=0, frames=[], score=r["score"])
    cs.insert(5, empty)
    def pad(e):                                   # the C = 6 cases ride in the C = 29 batch: classes no token names are never read
        return np.concatenate([e, np.full((e.shape[0], 29 - e.shape[1]), np.nan, np.float32)], axis=1)
    clips = [(pad(c["e"]), c["tokens"]) for c in cs]
    fr, sc, st, tr = launch(clips, want_trellis=True)
    assert len(cs) == 14 and st == [c["status"] for c in cs] and sorted(set(st)) == [0, 1]
    for n, c in enumerate(cs):
        check_clip(fr[n], sc[n], st[n], c)
        assert tr[n].tobytes() == c["trellis"].tobytes(), n


def test_operator_returns_fresh_outputs_and_passes_opcheck(fx):
    c, d = case(fx, "q_40x12"), case(fx, "g_2x3")
    e = torch.from_numpy(np.concatenate([c["e"][:, :6], d["e"][:, :6]])).to(DEV)
    tokens = c["tokens"] + [1, 2, 3]
    args = (e, torch.tensor([0, 40, 42], dtype=I32, device=DEV), torch.tensor(tokens, dtype=I32, device=DEV),
            torch.tensor([0, 12, 15], dtype=I32, device=DEV), 0, 40, 12)
    fr, sc, st, tr = torch.ops.ta355.ctc_align(*args, None, 0)
    assert fr.tolist() == c["frames"] + [-1, -1, -1] and st.tolist() == [0, 1] and tr.numel() == 0
    off = torch.tensor([0, 41 * 13], dtype=torch.int64, device=DEV)
    tr = torch.ops.ta355.ctc_align(*args, off, 41 * 13 + 3 * 4)[3]
    assert tr[:41 * 13].cpu().numpy().tobytes() == c["trellis"].tobytes()
    torch.library.opcheck(torch.ops.ta355.ctc_align, (*args, None, 0), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.ta355.ctc_align, (*args, off, 41 * 13 + 12), test_utils=("test_schema", "test_faketensor"))


def test_clips_are_isolated(fx):
    """NaN in the NEXT clip's emission rows (and a strided emission matrix whose padding columns are NaN) changes nothing."""
    a, b = case(fx, "g_70x65"), case(fx, "q_130x40")
    eb = np.full((130, 29), np.nan, np.float32)
    clips = [(a["e"], a["tokens"]), (eb, b["tokens"]), (a["e"], a["tokens"])]
    fr, sc, st, _ = launch(clips)
    check_clip(fr[0], sc[0], st[0], a)
    check_clip(fr[2], sc[2], st[2], a)
    wide = torch.full((70, 40), float("nan"), device=DEV)
    wide[:, :29] = torch.from_numpy(a["e"]).to(DEV)
    fr, sc, st, _ = launch([(a["e"], a["tokens"])], emission=wide[:, :29])
    check_clip(fr[0], sc[0], st[0], a)


# ----------------------------------------------------------------------------- shapes beyond the fixture, against align_ref
def ref_case(seed, T, J, C, quantised=False, spread=False):
    rng = np.random.default_rng(seed)
    if quantised:
        e = (-0.5 * rng.integers(0, 7, (T, C))).astype(np.float32)
    else:
        x = rng.standard_normal((T, C)).astype(np.float32)
        e = (x - np.log(np.exp(x.astype(np.float64)).sum(-1, keepdims=True))).astype(np.float32)
    tokens = (np.linspace(1, C - 1, J).astype(np.int64) if spread else rng.integers(1, C, J)).tolist()
    r = align_ref.align(e, tokens, fast=True)
    return dict(e=e, tokens=tokens, trellis=r["trellis"], status=r["status"], frames=r["frames"], score=r["score"])


@pytest.mark.parametrize("T,J,C,kw", [
    (THREADS + 40, THREADS - 1, 29, {}),                     # J + 1 columns = the workgroup exactly: one full pass, no second
    (THREADS + 40, THREADS, 29, {}),                         # one column above it: thread 0 alone owns a second column
    (THREADS + 40, THREADS + 1, 29, {}),                     # J one above the workgroup
    (FRAME_BLOCK + 1, 20, 29, {}),                           # T one above the full staging block (J + 1 <= STAGE / FRAME_BLOCK)
    (frame_block(2 * THREADS + 5) + 1, 2 * THREADS + 5, 6, dict(quantised=True)),      # T one above a CLAMPED block (T < J: fails)
    (40 * frame_block(2 * THREADS + 5) + 1, 2 * THREADS + 5, 6, dict(quantised=True)),  # the same 40 blocks on: ties, 3 columns a thread
    (100, 300, 4096, dict(spread=True)),                     # large C: the gather reaches across the vocabulary, T < J fails
    (400, 300, 4096, dict(spread=True)),                     # the same and it aligns
], ids=["J+1=threads", "J=threads", "J=threads+1", "T=block+1", "T=clamped_block+1", "ties_3cols", "C=4096_fails", "C=4096"])
def test_shapes_against_align_ref(T, J, C, kw):
    c = ref_case(T * 1000 + J, T, J, C, **kw)
    fr, sc, st, tr = launch([(c["e"], c["tokens"])], want_trellis=True)
    assert tr[0].tobytes() == c["trellis"].tobytes()
    check_clip(fr[0], sc[0], st[0], c)
    assert c["status"] == int(T < J)


def test_constants_sit_where_the_cases_assume():
    assert THREADS % 64 == 0 and frame_block(20) == FRAME_BLOCK and 1 <= frame_block(2 * THREADS + 5) < FRAME_BLOCK
    assert frame_block(ops.ALIGN_LIMITS["tokens"]) >= 1


def test_device_refuses_a_bad_clip_and_leaves_its_neighbours_alone(fx):
    """What the host wrappers of alignment.py refuse before a launch, the kernel refuses per clip when it is reached directly
    (ops.ctc_align / the C ABI): status 2, score -inf, no frames and no trellis written, the other clips of the launch as alone."""
    a, b = case(fx, "g_70x65"), case(fx, "q_40x12")
    neg = np.float32(-np.inf).tobytes()
    bad = list(a["tokens"])
    bad[40] = 29                                                            # one id == C, deep in the second ballot word
    fr, sc, st, tr = launch([(a["e"], a["tokens"]), (a["e"], bad), (a["e"], a["tokens"])], want_trellis=True)
    assert st == [0, 2, 0] and sc[1].tobytes() == neg and fr[1] == [SENTINEL] * 65 and (tr[1] == FILL).all()
    for n in (0, 2):
        check_clip(fr[n], sc[n], st[n], a)
        assert tr[n].tobytes() == a["trellis"].tobytes()
    bad[40] = -1
    assert launch([(a["e"], bad)])[2] == [2]
    # a clip beyond the maxima the caller declared (they size the workspace): 70 frames against max_frames 40, then 65 tokens
    # against max_tokens 12
    pad = np.concatenate([b["e"], np.full((40, 23), np.nan, np.float32)], axis=1)
    for maxima in ((40, 65), (70, 12)):
        fr, sc, st, tr = launch([(pad, b["tokens"]), (a["e"], a["tokens"]), (pad, b["tokens"])], want_trellis=True, maxima=maxima)
        assert st == [0, 2, 0] and sc[1].tobytes() == neg and fr[1] == [SENTINEL] * 65 and (tr[1] == FILL).all()
        for n in (0, 2):
            check_clip(fr[n], sc[n], st[n], b)
            assert tr[n].tobytes() == b["trellis"].tobytes()


def test_envelope_corner_runs():
    """J = 2048 (nine columns per thread, three-frame staging blocks) over a short clip and a longer one in one launch."""
    a, b = ref_case(1, 2100, 2048, 32, quantised=True), ref_case(2, 70, 2048, 32)
    fr, sc, st, _ = launch([(a["e"], a["tokens"]), (b["e"], b["tokens"])])
    check_clip(fr[0], sc[0], st[0], a)
    check_clip(fr[1], sc[1], st[1], b)
    assert st == [0, 1]


# ----------------------------------------------------------------------------- end to end
def test_align_and_align_batch_equal_the_reference_words(fx):
    ems = [torch.from_numpy(fx[w["emission"] + ".emission"]) for w in META["words"]]
    texts = [w["text"] for w in META["words"]]
    want = [w["words"] for w in META["words"]]
    assert ForcedAligner.align_batch(ems, texts) == want
    assert ForcedAligner.align_batch([e.to(DEV) for e in ems], texts) == want
    for e, text, w in zip(ems, texts, want):
        assert ForcedAligner.align(np.zeros(16000, np.float32), text, emission=e) == w
    # logits plus log_softmax=True: shifted log-probabilities are logits of the same distribution, up to rounding; the words hold
    got = ForcedAligner.align(None, texts[0], emission=ems[0] + 3.0, log_softmax=True)
    assert [g["word"] for g in got] == [g["word"] for g in want[0]]
