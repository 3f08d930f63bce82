"""-m gpu: text alignment on the device (csrc/text_align.hip through ops.text_align, torch.ops.ta355.text_align and
tiny_audio_amd/text_align.py) against tests/text_align_ref.py (tests/test_text_align_host.py pins its row scan to the cell-by-cell
definition and its LCS walk to the reference's own answers).  Everything is int32, so every comparison is equality: no tolerance
anywhere in this file.

The shapes sit around the seams: the wave word (63 / 64 / 65, 127 / 128 / 129 on either side), a column seam every 64 or 128 columns
and a row seam every 64 rows with the long kernel's smallest tiles, the default tile's seam at 256, the short kernel's envelope at
512 columns, and alphabets of 2 to 4 symbols, where equal-cost paths are everywhere and the tie rule decides every step."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import text_align_ref as R
from tiny_audio_amd import _lib, eval_text, ops, text_align

pytestmark = pytest.mark.gpu

DEV = "cuda"
I32 = torch.int32
SENTINEL = -77
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EDGES = (0, 1, 2, 63, 64, 65, 127, 128, 129)
MODES = pytest.mark.parametrize("mode", (R.EDIT, R.LCS), ids=("edit", "lcs"))
PATHS = pytest.mark.parametrize("want_path", (True, False), ids=("path", "dist"))
_REF = {}


def ref_of(key, r, h, mode):
    """The restatement's answer, computed once per (case, mode) and shared, never modified, between the tests."""
    if (key, mode) not in _REF:
        _REF[key, mode] = R.align(r, h, mode)
    return _REF[key, mode]


def header_define(name):
    return int(re.search(rf"#define {name} (\d+)", open(_lib.HEADER).read()).group(1))


def pair(n, m, alpha, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, alpha, n).astype(np.int32), rng.integers(0, alpha, m).astype(np.int32)


def run(refs, hyps, mode, want_path, cb=0, rb=0, max_n=None, max_m=None, guard=0, workspace=None):
    """Lists of id arrays -> (dist, counts, map, status) on the host, through ops.text_align (what the operator calls), so that map
    can be pre-filled with a sentinel; ``guard`` extra symbols and map entries lie beyond cu_ref[-1]."""
    r, cu_r = R.ragged(refs)
    h, cu_h = R.ragged(hyps)
    r = np.concatenate([r, np.full(guard, 3, np.int32)])
    t = lambda x: torch.from_numpy(x).to(DEV)                                                  # noqa: E731
    mp = torch.full((len(r),), SENTINEL, dtype=I32, device=DEV) if want_path else None
    max_n = max([len(x) for x in refs] + [0]) if max_n is None else max_n
    max_m = max([len(x) for x in hyps] + [0]) if max_m is None else max_m
    d, c, mp, st = ops.text_align(t(r), t(cu_r), t(h), t(cu_h), max_n, max_m, mode, want_path, col_block=cb, row_block=rb, map=mp,
                                  workspace=workspace)
    torch.cuda.synchronize()
    return d.cpu().numpy(), c.cpu().numpy(), (mp.cpu().numpy() if want_path else None), st.cpu().numpy()


def check_pair(key, r, h, mode, want_path, **kw):
    dist, counts, mp = ref_of(key, r, h, mode)
    d, c, m, st = run([r], [h], mode, want_path, **kw)
    assert st.tolist() == [0] and d.tolist() == [dist], (key, mode, d, dist)
    if want_path:
        assert c.tolist() == [list(counts)], (key, mode, c, counts)
        assert np.array_equal(m, mp), (key, mode)
    else:
        assert c.tolist() == [[0, 0, 0, 0]] and m is None


# ----------------------------------------------------------------------------- length edges, single pairs
@MODES
@PATHS
def test_length_edges(mode, want_path):
    for n in EDGES:
        for m in EDGES:
            r, h = pair(n, m, 2, 1000 * n + m)
            check_pair(("edge", n, m), r, h, mode, want_path)
    for n in (1, 64, 65, 129):
        same = pair(n, n, 2, n)[0]
        check_pair(("same", n), same, same.copy(), mode, want_path)                     # identical: all hits
        check_pair(("disjoint", n), np.zeros(n, np.int32), np.ones(n + 1, np.int32), mode, want_path)     # nothing in common
        wide = np.where(same == 0, -2 ** 31, 2 ** 31 - 1).astype(np.int32)                                # any int32 is a symbol
        check_pair(("wide", n), wide, wide[::-1].copy(), mode, want_path)
    if want_path and mode == R.EDIT:
        dist, counts, mp = _REF[("same", 129), mode]
        assert dist == 0 and counts == (129, 0, 0, 0) and mp.tolist() == list(range(129))
        dist, counts, mp = _REF[("disjoint", 64), mode]
        assert dist == 65 and counts == (0, 64, 0, 1) and mp.tolist() == list(range(1, 65))


# ----------------------------------------------------------------------------- tile edges on the long kernel
TILE_PAIRS = ((200, 300), (64, 64), (65, 64), (64, 65), (129, 257))


@MODES
@pytest.mark.parametrize("n,m", TILE_PAIRS, ids=[f"{n}x{m}" for n, m in TILE_PAIRS])
def test_tile_edges_every_kernel_the_same_bytes(mode, n, m):
    r, h = pair(n, m, 2, 77 * n + m)
    dist, counts, mp = ref_of(("tile", n, m), r, h, mode)
    cb0, rb0 = header_define("TA_TEXT_ALIGN_COL_BLOCK"), header_define("TA_TEXT_ALIGN_ROW_BLOCK")
    outs = {}
    for name, (cb, rb) in dict(short=(0, 0), t64=(64, 64), t128=(128, 64), t64x128=(64, 128), t512=(512, 64), default=(cb0, rb0),
                               default_cols=(0, 64)).items():
        outs[name] = run([r], [h], mode, True, cb=cb, rb=rb)
        d = run([r], [h], mode, False, cb=cb, rb=rb)
        assert d[0].tolist() == [dist] and d[3].tolist() == [0], name
    for name, (d, c, mpg, st) in outs.items():
        assert st.tolist() == [0] and d.tolist() == [dist] and c.tolist() == [list(counts)] and np.array_equal(mpg, mp), name
        for a, b in zip(outs["short"][:3], (d, c, mpg)):
            assert a.tobytes() == b.tobytes(), name


def test_the_short_kernel_up_to_its_last_column_and_the_long_one_beyond():
    """m = 512 is the short kernel's widest pair (8 columns a lane), m = 513 the first that the default choice sends to the tiles."""
    for m in (512, 513):
        r, h = pair(70, m, 3, m)
        for mode in (R.EDIT, R.LCS):
            check_pair(("envelope", m), r, h, mode, True)
            check_pair(("envelope", m), r, h, mode, True, cb=64, rb=64)


# ----------------------------------------------------------------------------- a ragged batch in one call
def ragged_batch():
    rng = np.random.default_rng(37)
    lens = [0, 1, 30, 700]
    refs, hyps = [], []
    for p in range(37):
        n = lens[p % 4] + (int(rng.integers(-3, 4)) if lens[p % 4] >= 30 else 0)
        m = lens[(p // 4 + p) % 4] + (int(rng.integers(-3, 4)) if lens[(p // 4 + p) % 4] >= 30 else 0)
        refs.append(rng.integers(0, 3, n).astype(np.int32))
        hyps.append(rng.integers(0, 3, m).astype(np.int32))
    refs[8] = rng.integers(0, 3, 900).astype(np.int32)                    # longer than the declared max_n of 750: refused
    return refs, hyps


@MODES
@PATHS
@pytest.mark.parametrize("kernel", ("long", "short"))
def test_ragged_batch_in_one_call(mode, want_path, kernel):
    refs, hyps = ragged_batch()
    if kernel == "short":                                                 # the pairs whose hypotheses fit one narrow tile
        keep = [p for p in range(37) if len(hyps[p]) <= 40]
        refs, hyps = [refs[p] for p in keep], [hyps[p] for p in keep]
        assert len(refs) >= 15 and any(len(x) == 900 for x in refs)
    cu = np.concatenate([[0], np.cumsum([len(x) for x in refs])])
    assert any(int(x) % 4 for x in cu[1:-1])                              # offsets that are no multiple of 4
    refused = next(p for p in range(len(refs)) if len(refs[p]) == 900)
    d, c, mp, st = run(refs, hyps, mode, want_path, max_n=750, max_m=max(len(x) for x in hyps), guard=11)
    for p, (r, h) in enumerate(zip(refs, hyps)):
        if p == refused:
            assert st[p] == 2 and d[p] == -1 and c[p].tolist() == [0, 0, 0, 0]
            if want_path:
                assert (mp[cu[p]:cu[p + 1]] == SENTINEL).all()
            continue
        dist, counts, want = ref_of(("ragged", kernel, p), r, h, mode)
        assert st[p] == 0 and d[p] == dist, p
        if want_path:
            assert c[p].tolist() == list(counts) and np.array_equal(mp[cu[p]:cu[p + 1]], want), p
    if want_path:
        assert len(mp) == cu[-1] + 11 and (mp[cu[-1]:] == SENTINEL).all()


def test_a_workspace_too_small_for_the_bits_refuses_the_pairs_that_do_not_fit():
    refs, hyps = [pair(70, 30, 2, 1)[0], pair(10, 5, 2, 2)[0], pair(200, 40, 2, 3)[0]], [pair(70, 30, 2, 1)[1], pair(10, 5, 2, 2)[1],
                                                                                       pair(200, 40, 2, 3)[1]]
    cu_r, cu_h = (torch.tensor(R.ragged(x)[1]) for x in (refs, hyps))
    fixed = ops.text_align_workspace_bytes(cu_r, cu_h, 200, 40, False)
    room = fixed + (30 * 2 + 5 * 1) * 16                                  # the bits of the first two pairs, not of the third
    assert ops.text_align_workspace_bytes(cu_r, cu_h, 200, 40, True) == room + 40 * 4 * 16
    ws = torch.empty(room, dtype=torch.uint8, device=DEV)
    d, c, mp, st = run(refs, hyps, R.EDIT, True, workspace=ws)
    assert st.tolist() == [0, 0, 2] and d[2] == -1 and (mp[80:] == SENTINEL).all()
    for p in range(2):
        dist, counts, want = R.align(refs[p], hyps[p], R.EDIT)
        assert d[p] == dist and c[p].tolist() == list(counts)
    assert run(refs, hyps, R.EDIT, False, workspace=ws)[3].tolist() == [0, 0, 0]      # distances need no bits


# ----------------------------------------------------------------------------- one mid-size pair
@MODES
def test_mid_size_pair_with_the_default_tiles(mode):
    r, h = pair(5000, 5200, 4, 5000)
    check_pair(("mid",), r, h, mode, True)
    check_pair(("mid",), r, h, mode, False)


# ----------------------------------------------------------------------------- determinism, the operator
def test_two_runs_give_identical_bytes_whatever_the_workspace_held():
    refs, hyps = ragged_batch()
    refs[8] = refs[8][:700]
    for mode in (R.EDIT, R.LCS):
        a = run(refs, hyps, mode, True)
        b = run(refs, hyps, mode, True)
        cu_r, cu_h = (torch.tensor(R.ragged(x)[1]) for x in (refs, hyps))
        need = ops.text_align_workspace_bytes(cu_r, cu_h, 703, 703, True)
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
        c = run(refs, hyps, mode, True, max_n=703, max_m=703, workspace=ws)
        for x, y, z in zip(a, b, c):
            assert x.tobytes() == y.tobytes() == z.tobytes()
        assert a[3].tolist() == [0] * 37


def test_operator_and_opcheck():
    refs, hyps = [pair(70, 65, 2, 5)[0], pair(3, 0, 2, 6)[0]], [pair(70, 65, 2, 5)[1], pair(3, 0, 2, 6)[1]]
    r, cu_r = (torch.from_numpy(x).to(DEV) for x in R.ragged(refs))
    h, cu_h = (torch.from_numpy(x).to(DEV) for x in R.ragged(hyps))
    for mode in (R.EDIT, R.LCS):
        dist, counts, mp = R.align_batch(refs, hyps, mode)
        d, c, m, st = torch.ops.ta355.text_align(r, cu_r, h, cu_h, 70, 65, mode, True, 0, 0, None)
        assert d.dtype == c.dtype == m.dtype == st.dtype == I32 and st.tolist() == [0, 0]
        assert d.tolist() == dist.tolist() and c.tolist() == counts.tolist() and m.tolist() == mp.tolist()
        d, c, m, st = torch.ops.ta355.text_align(r, cu_r, h, cu_h, 70, 65, mode, False, 64, 64, None)
        assert d.tolist() == dist.tolist() and m.shape == (0,) and not c.any()
    ws = torch.empty(ops.text_align_workspace_bytes(cu_r.cpu(), cu_h.cpu(), 70, 65, True, 64, 64), dtype=torch.uint8, device=DEV)
    torch.library.opcheck(torch.ops.ta355.text_align, (r, cu_r, h, cu_h, 70, 65, 0, True, 0, 0, None), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.ta355.text_align, (r, cu_r, h, cu_h, 70, 65, 1, True, 64, 64, ws), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.ta355.text_align, (r, cu_r, h, cu_h, 70, 65, 0, False, 0, 0, None), test_utils=("test_schema", "test_faketensor"))


# ----------------------------------------------------------------------------- the Python surface
REFS = ["the cat sat on the mat", "", "a a a b a", "Hello  World", "one", "the a the a the a the"]
HYPS = ["the cat sat on mat the", "uh", "a b a a", "hello world again", "", "a the a the a"]


@pytest.mark.parametrize("unit", ("word", "char"))
def test_error_counts_equal_the_restatement(unit):
    out = text_align.error_counts(REFS, HYPS, unit=unit, normalize=str.lower, return_map=True)
    r, cu_r, h, cu_h = text_align.encode(REFS, HYPS, unit, str.lower)
    tot = 0
    for p in range(len(REFS)):
        rp, hp = r[cu_r[p]:cu_r[p + 1]], h[cu_h[p]:cu_h[p + 1]]
        dist, (H, S, D, I), mp = R.align(rp, hp, R.EDIT)
        got = tuple(int(out[k][p]) for k in ("dist", "hits", "substitutions", "deletions", "insertions", "ref_len", "hyp_len"))
        assert got == (dist, H, S, D, I, len(rp), len(hp)), (p, got)
        assert np.array_equal(out["map"][p], mp)
        tot += dist
    assert out["cer" if unit == "char" else "wer"] == tot / int(cu_r[-1])
    assert out["dist"][1] == len(HYPS[1].split() if unit == "word" else HYPS[1])              # an empty reference: insertions only
    sub = text_align.error_counts(REFS, HYPS, unit=unit, normalize=str.lower, col_block=64, row_block=64)
    assert all(np.array_equal(sub[k], out[k]) for k in ("dist", "hits", "substitutions", "deletions", "insertions"))


class Lower:
    def normalize(self, text):
        return text.lower().strip()


def test_align_words_to_reference_equals_the_reference():
    for case in json.load(open(os.path.join(GOLDEN, "text_align.json")))["cases"]:
        pw = [dict(word=w, index=i) for i, w in enumerate(case["pred"])]
        rw = [dict(word=w, index=i) for i, w in enumerate(case["ref"])]
        got = text_align.align_words_to_reference(pw, rw, Lower(), device="cuda")
        assert [[p["index"], q["index"]] for p, q in got] == case["pairs"], case["name"]
        assert all(p is pw[p["index"]] and q is rw[q["index"]] for p, q in got)               # the caller's own dicts


def test_word_error_rate_on_the_device_is_the_host_value():
    host = eval_text.word_error_rate(REFS, HYPS, normalize=str.lower)
    assert eval_text.word_error_rate(REFS, HYPS, normalize=str.lower, device="cuda") == host
    assert eval_text.word_error_rate("a b c", "a c", device="cuda") == 1 / 3 == eval_text.word_error_rate("a b c", "a c")
    rng = np.random.default_rng(3)
    words = "the a of cat dog sat mat".split()
    refs = [" ".join(words[i] for i in rng.integers(0, 7, rng.integers(1, 60))) for _ in range(200)]
    hyps = [" ".join(words[i] for i in rng.integers(0, 7, rng.integers(0, 60))) for _ in range(200)]
    assert eval_text.word_error_rate(refs, hyps, device="cuda") == eval_text.word_error_rate(refs, hyps)
