"""-m "not gpu": text alignment off the device.  tests/text_align_ref.py (the definition the kernels are held to): its row-scan form
against its cell-by-cell form, the count identities, and the pairs the reference's own ``align_words_to_reference`` returned
(tests/golden/text_align.json); then the C ABI's declarations, workspace arithmetic and refusals, the operator's registration, the
dry-run plumbing of ``tiny_audio_amd.text_align``, and ``word_error_rate`` being where it was without ``device``."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import text_align_ref as R
from tiny_audio_amd import _lib, eval_text, ops, text_align

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIX = json.load(open(os.path.join(GOLDEN, "text_align.json")))["cases"]
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


class Lower:
    def normalize(self, text):
        return text.lower().strip()


# ----------------------------------------------------------------------------- the restatement
def random_pairs():
    rng = np.random.default_rng(7)
    for alpha in (2, 3, 50):
        for _ in range(40):
            n, m = rng.integers(0, 41, 2)
            yield rng.integers(0, alpha, n).astype(np.int32), rng.integers(0, alpha, m).astype(np.int32)
    for n, m in ((0, 0), (0, 7), (7, 0), (1, 1), (40, 40)):
        yield np.zeros(n, np.int32), np.ones(m, np.int32)                 # fully disjoint
        yield np.zeros(n, np.int32), np.zeros(m, np.int32)                # one repeated symbol


@pytest.mark.parametrize("mode", (R.EDIT, R.LCS))
def test_row_scan_equals_cell_by_cell(mode):
    k = 0
    for r, h in random_pairs():
        want = R.align_cells(r, h, mode)
        got = R.align(r, h, mode)
        assert got[0] == want[0] and tuple(got[1]) == tuple(want[1]) and np.array_equal(got[2], want[2]), (mode, r, h)
        assert R.align(r, h, mode, want_path=False) == (want[0], None, None)
        # every row of the scan, not only the last: the full tables
        table = (R.edit_table_cells if mode == R.EDIT else R.lcs_table_cells)(list(r), list(h))
        for i in range(len(r) + 1):
            last = (R.edit_rows if mode == R.EDIT else R.lcs_rows)(r[:i], h, want_bits=False)[0]
            assert last.tolist() == table[i]
        k += 1
    assert k >= 120


def test_count_identities():
    for r, h in random_pairs():
        n, m = len(r), len(h)
        dist, (H, S, D, I), mp = R.align(r, h, R.EDIT)
        assert S + D + I == dist and H + S + D == n and H + S + I == m
        assert (mp >= 0).sum() == H + S and (np.diff(mp[mp >= 0]) > 0).all()
        assert sum(int(r[i] == h[j]) for i, j in enumerate(mp) if j >= 0) == H
        pairs, (P, zero, dn, dm), mp = R.align(r, h, R.LCS)
        assert P == pairs and zero == 0 and dn == n - P and dm == m - P
        assert (mp >= 0).sum() == P and all(r[i] == h[j] for i, j in enumerate(mp) if j >= 0)
        assert dist <= n + m - 2 * pairs                                  # indel distance bounds Levenshtein from above


def test_batch_layout():
    refs = [np.array([1, 2, 3]), np.zeros(0, np.int64), np.array([5])]
    hyps = [np.array([1, 3]), np.array([4, 4]), np.array([5])]
    dist, counts, mp = R.align_batch(refs, hyps, R.EDIT)
    assert dist.tolist() == [1, 2, 0] and counts.tolist() == [[2, 0, 1, 0], [0, 0, 0, 2], [1, 0, 0, 0]] and mp.tolist() == [0, -1, 1, 0]
    assert dist.dtype == counts.dtype == mp.dtype == np.int32
    flat, cu = R.ragged(refs)
    assert flat.tolist() == [1, 2, 3, 5] and cu.tolist() == [0, 3, 3, 4] and flat.dtype == cu.dtype == np.int32


# ----------------------------------------------------------------------------- the reference's own answers
def fixture_ids(case):
    """What align_words_to_reference does on the host: skip <unk> (reference side) and empty-after-normalisation, number the words."""
    norm = Lower().normalize
    ref = [(norm(w), i) for i, w in enumerate(case["ref"]) if w != "<unk>" and norm(w)]
    pred = [(norm(w), i) for i, w in enumerate(case["pred"]) if norm(w)]
    table = {}
    r = [table.setdefault(w, len(table)) for w, _ in ref]
    h = [table.setdefault(w, len(table)) for w, _ in pred]
    return r, h, [i for _, i in ref], [i for _, i in pred]


def test_fixture_is_pinned():
    assert os.path.getsize(os.path.join(GOLDEN, "text_align.json")) < 64 * 1024
    names = [c["name"] for c in FIX]
    assert len(names) == 15 and {"repeats_ta", "repeats_at", "unk_and_empty", "disjoint", "no_pred", "random_0"} <= set(names)
    ta = next(c for c in FIX if c["name"] == "repeats_ta")
    assert ta["pred"][:4] == ["the", "a", "the", "a"] and len(ta["pairs"]) == 10     # repeated words: the tie rule decides
    assert sum(len(c["pairs"]) for c in FIX) == 226
    assert all(set(c) == {"name", "pred", "ref", "pairs"} for c in FIX)              # data only: words and indices


@pytest.mark.parametrize("case", FIX, ids=[c["name"] for c in FIX])
def test_restatement_reproduces_the_reference(case):
    r, h, ref_idx, pred_idx = fixture_ids(case)
    _, counts, mp = R.align(r, h, R.LCS) if r and h else (0, (0, 0, len(r), len(h)), np.full(len(r), -1, np.int32))
    got = [[pred_idx[j], ref_idx[i]] for i, j in enumerate(mp) if j >= 0]
    assert got == case["pairs"] and counts[0] == len(case["pairs"])
    if r and h:
        assert R.align_cells(r, h, R.LCS)[0] == len(case["pairs"])


# ----------------------------------------------------------------------------- the C ABI
def test_header_declares_the_entry_points():
    protos = _lib.parse_header()
    assert len(protos["ta_text_align_i32"][1]) == 18 and len(protos["ta_text_align_workspace_bytes"][1]) == 8
    assert protos["ta_text_align_workspace_bytes"][0] is C.c_long and protos["ta_text_align_i32"][0] is C.c_int
    assert protos["ta_text_align_i32"][1][16] is C.c_long                            # the workspace size can pass 2^31
    text = open(_lib.HEADER).read()
    assert "scripts/eval/evaluators/alignment.py:12-79" in text and "tests/text_align_ref.py" in text
    want = {"pairs": 65536, "length": 262144, "col_block": 512, "short_m": 512}
    assert ops.TEXT_ALIGN_LIMITS == want
    assert {k: header_define("TA_TEXT_ALIGN_" + n) for k, n in (("pairs", "MAX_PAIRS"), ("length", "MAX_LEN"), ("col_block", "MAX_COL_BLOCK"),
                                                               ("short_m", "SHORT_MAX_M"))} == want
    assert header_define("TA_TEXT_ALIGN_MAX_LEN") == header_define("TA_ALIGN_LONG_MAX_TOKENS")
    assert header_define("TA_TEXT_ALIGN_COL_BLOCK") in (64, 128, 256, 512) and header_define("TA_TEXT_ALIGN_ROW_BLOCK") % 64 == 0
    assert (header_define("TA_TEXT_ALIGN_EDIT"), header_define("TA_TEXT_ALIGN_LCS")) == (ops.TEXT_ALIGN_EDIT, ops.TEXT_ALIGN_LCS) == (0, 1)


def test_source_is_built_and_the_abi_version_stays():
    assert "text_align.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "text_align.hip"))
    L = _lib.lib()
    assert L.ta_version() == 4
    assert hasattr(L, "ta_text_align_i32") and hasattr(L, "ta_text_align_workspace_bytes")


def cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=I32)


def test_workspace_arithmetic():
    """A fixed part (a flag and an offset per pair; for the long kernel the two carries from the maxima), then the decision bits of
    the batch's ACTUAL pairs: m * ceil(n / 64) * 16 bytes each."""
    q = ops.text_align_workspace_bytes
    rb0 = header_define("TA_TEXT_ALIGN_ROW_BLOCK")

    def fixed(N, max_n, max_m, short, rb):
        carries = 0 if short else N * (max_m + max_n + -(-max_n // rb)) * 4
        return ((N * 4 + 7) // 8 * 8 + N * 8 + carries + 15) // 16 * 16

    def bits(ns, ms):
        return sum(m * -(-n // 64) * 16 for n, m in zip(ns, ms))

    ns, ms = [10, 0, 65, 700], [12, 5, 64, 3]
    a, b = cu(ns), cu(ms)
    assert q(a, b, 700, 64, True) == fixed(4, 700, 64, True, rb0) + bits(ns, ms)                   # the short kernel: no carries
    assert q(a, b, 700, 64, False) == fixed(4, 700, 64, True, rb0) == q(None, None, 700, 64, True, pairs=4) == 48
    assert q(None, None, 700, 64, False, 64, 64, pairs=4) == fixed(4, 700, 64, False, 64) == q(a, b, 700, 64, False, 64, 64) > 12000
    assert q(None, None, 700, 64, True, pairs=0) == 0
    assert q(a, b, 700, 64, True, 64, 128) == fixed(4, 700, 64, False, 128) + bits(ns, ms)         # a tiling asks for the long one
    assert q(a, b, 700, 64, True, 0, 128) == q(a, b, 700, 64, True, 512, 128)                      # the column block moves no byte
    assert q(a, b, 700, 513, True) == fixed(4, 700, 513, False, rb0) + bits(ns, ms)                # beyond one tile: the long kernel
    assert q(a, b, 64, 64, True) == fixed(4, 64, 64, True, rb0) + bits(ns[:2], ms[:2])             # refused pairs hold no bits
    # sized from the pairs, not N x max x max: 4096 short pairs and one declared maximum far beyond them
    many_n, many_m = [30] * 4096, [40] * 4096
    assert q(cu(many_n), cu(many_m), 262144, 512, True) == fixed(4096, 262144, 512, True, rb0) + 4096 * 40 * 16 < 4 << 20
    one = q(cu([32768]), cu([32768]), 32768, 32768, True)
    assert one == fixed(1, 32768, 32768, False, rb0) + 32768 * 512 * 16 and 268e6 < one < 270e6
    top = q(cu([262144]), cu([262144]), 262144, 262144, True)
    assert top == fixed(1, 262144, 262144, False, rb0) + 262144 * 4096 * 16 and top > 2 ** 34
    assert q(cu([262144]), cu([262144]), 262144, 262144, False) < 3 << 20                          # distance only: the carries
    for bad in ((63, 0), (96, 0), (-64, 0), (1024, 0), (64, -64), (64, 96), (0, 262144 + 64)):
        assert q(a, b, 700, 64, True, *bad) == -1, bad


def test_c_abi_refuses_before_any_launch():
    """Host-side argument checks return TA_ERR_ARG before anything is launched, so they run without a GPU."""
    L = _lib.lib()
    one = C.c_void_p(8)                                                    # never dereferenced: every call below is refused

    def call(N=1, mn=10, mm=5, mode=0, path=1, cb=0, rb=0, ref=one, hyp=one, cu_r=one, cu_h=one, dist=one, counts=one, mp=one,
             status=one, ws=one, ws_bytes=1 << 20):
        return L.ta_text_align_i32(ref, cu_r, hyp, cu_h, N, mn, mm, mode, path, cb, rb, dist, counts, mp, status, ws, ws_bytes, None)

    assert call(N=65537) == 1 and call(N=-1) == 1 and call(mn=262145) == 1 and call(mm=262145) == 1 and call(mn=-1) == 1 and call(mm=-1) == 1
    assert call(mode=2) == 1 and call(mode=-1) == 1 and call(path=2) == 1 and call(path=-1) == 1
    assert call(cb=63) == 1 and call(cb=192) == 1 and call(cb=1024) == 1 and call(cb=-64) == 1 and call(rb=-64) == 1 and call(rb=100) == 1
    assert call(cu_r=None) == 1 and call(cu_h=None) == 1 and call(dist=None) == 1 and call(status=None) == 1
    assert call(ref=None) == 1 and call(hyp=None) == 1 and call(counts=None) == 1 and call(mp=None) == 1
    assert call(ws=None) == 1 and call(ws_bytes=15) == 1                   # the fixed part of one pair is 16 bytes
    assert call(cb=64, ws_bytes=16 + (10 + 5 + 1) * 4 - 1) == 1            # ... and with the long kernel's carries 80
    assert call(N=0) == 0                                                  # an empty batch is legal and launches nothing


def test_ops_wrapper_refuses_before_the_library(dry):
    r, h = torch.zeros(4, dtype=I32), torch.zeros(3, dtype=I32)
    args = (r, cu([4]), h, cu([3]))
    dry.calls.clear()
    for kw, msg in ((dict(col_block=100), "64, 128, 256 or 512"), (dict(col_block=1024), "64, 128, 256 or 512"),
                    (dict(row_block=96), "multiple of 64"), (dict(row_block=-64), "multiple of 64")):
        with pytest.raises(ValueError, match=msg):
            ops.text_align(*args, 4, 3, 0, True, **kw)
    with pytest.raises(ValueError, match="limit of 262144"):
        ops.text_align(*args, 262145, 3, 0, True)
    with pytest.raises(ValueError, match="neither 0"):
        ops.text_align(*args, 4, 3, 2, True)
    with pytest.raises(ValueError, match="limit of 65536"):
        ops.text_align(r, torch.zeros(65538, dtype=I32), h, torch.zeros(65538, dtype=I32), 4, 3, 0, True)
    with pytest.raises(ValueError, match="cu_ref holds 2 entries but cu_hyp 3"):
        ops.text_align(r, cu([4]), h, cu([1, 2]), 4, 3, 0, True)
    # a path whose decision bits pass max_workspace_bytes is refused with the size in the message; distances alone are not
    big = (torch.zeros(40000, dtype=I32), cu([40000]), torch.zeros(30000, dtype=I32), cu([30000]), 40000, 30000, 0)
    need = ops.text_align_workspace_bytes(cu([40000]), cu([30000]), 40000, 30000, True)
    assert need > 30000 * 625 * 16
    with pytest.raises(ValueError, match=f"workspace of {need} bytes, beyond max_workspace_bytes = 1000000"):
        ops.text_align(*big, True, max_workspace_bytes=1000000)
    assert ops.TEXT_ALIGN_MAX_WORKSPACE == 8 << 30 and inspect.signature(ops.text_align).parameters["max_workspace_bytes"].default == 8 << 30
    assert dry.calls == []
    ops.text_align(*big, False, max_workspace_bytes=1000000)
    assert dry.calls == ["ta_text_align_i32"]


def test_the_wrapper_sizes_the_workspace_the_library_asks_for(dry, monkeypatch):
    """Whatever the kernel and the mode, the workspace the wrapper allocates is the query's size for the same arguments."""
    seen = []
    real = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (seen.append(a[0]) if k.get("dtype") == torch.uint8 else None, real(*a, **k))[1])
    r, h = torch.zeros(300, dtype=I32), torch.zeros(700, dtype=I32)
    a, b = cu([100, 0, 200]), cu([1, 699, 0])
    for path in (True, False):
        for cb, rb in ((0, 0), (64, 64), (0, 128), (512, 0)):
            seen.clear()
            ops.text_align(r, a, h, b, 200, 699, 0, path, col_block=cb, row_block=rb)
            need = ops.text_align_workspace_bytes(a, b, 200, 699, path, cb, rb)
            assert seen == [need] and need >= ((3 * 4 + 7) // 8 * 8 + 24 + 3 * (699 + 200 + 1) * 4), (path, cb, rb)
    seen.clear()
    ops.text_align(r, a, torch.zeros(60, dtype=I32), cu([20, 20, 20]), 200, 20, 0, False)      # the short kernel: no carries
    assert seen == [48]


def test_no_cpu_path(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.Ta355Error, match="no CPU path"):
        ops.text_align(torch.zeros(4, dtype=I32), cu([4]), torch.zeros(3, dtype=I32), cu([3]), 4, 3, 0, True)
    with pytest.raises(_lib.Ta355Error, match="no CPU path"):
        text_align.error_counts(["a b"], ["a"])
    with pytest.raises(_lib.Ta355Error, match="no CPU path"):
        text_align.error_counts(["a b"], ["a"], device="cpu")
    with pytest.raises(_lib.Ta355Error, match="no CPU path"):
        eval_text.word_error_rate(["a b"], ["a"], device="cuda")
    with pytest.raises(_lib.Ta355Error, match="no CPU path"):
        text_align.align_words_to_reference([dict(word="a")], [dict(word="a")], Lower())


# ----------------------------------------------------------------------------- operator and plumbing
def test_operator_is_registered_with_a_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from tiny_audio_amd import torch_ops
    assert "text_align" in torch_ops.OPERATORS
    s = str(torch.ops.ta355.text_align.default._schema)
    assert s.startswith("ta355::text_align(Tensor ref, Tensor cu_ref, Tensor hyp, Tensor cu_hyp, SymInt max_n, SymInt max_m, SymInt mode, "
                        "bool want_path, SymInt col_block, SymInt row_block, Tensor(a10!)? workspace)"), s
    assert s.endswith("-> (Tensor, Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        a = (torch.empty(30, dtype=I32), torch.empty(4, dtype=I32), torch.empty(11, dtype=I32), torch.empty(4, dtype=I32), 12, 5, 0)
        dist, counts, mp, st = torch.ops.ta355.text_align(*a, True, 0, 0, None)
        assert dist.shape == (3,) and counts.shape == (3, 4) and mp.shape == (30,) and st.shape == (3,)
        assert dist.dtype == counts.dtype == mp.dtype == st.dtype == I32
        assert torch.ops.ta355.text_align(*a, False, 64, 64, torch.empty(4096, dtype=torch.uint8))[2].shape == (0,)


def test_dry_run_plumbing(dry):
    dry.calls.clear()
    out = text_align.error_counts(["a b c", "", "x"], ["a c", "y", "x"], return_map=True)
    assert dry.calls == ["ta_text_align_i32"]                                                 # one call for the batch
    assert out["ref_len"].tolist() == [3, 0, 1] and out["hyp_len"].tolist() == [2, 1, 1] and len(out["map"]) == 3
    assert [len(x) for x in out["map"]] == [3, 0, 1] and set(out) >= {"dist", "hits", "substitutions", "deletions", "insertions", "wer"}
    dry.calls.clear()
    assert "cer" in text_align.error_counts(["ab"], ["b"], unit="char")
    eval_text.word_error_rate(["a b"], ["a"], device="cuda")
    words = [dict(word=w) for w in ("The", "<unk>", "cat")]
    assert text_align.align_words_to_reference(words, words, Lower()) == []                   # the stubs compute nothing: map stays -1
    assert text_align.align_words_to_reference([], words, Lower()) == []
    assert dry.calls == ["ta_text_align_i32"] * 3
    with pytest.raises(ValueError, match="empty reference"):
        text_align.error_counts(["", " "], ["a", "b"])
    with pytest.raises(ValueError, match="differ in length"):
        text_align.error_counts(["a"], ["a", "b"])
    with pytest.raises(ValueError, match="'word' or 'char'"):
        text_align.error_counts(["a"], ["a"], unit="phone")
    with pytest.raises(ValueError, match="at most 262144 per side"):
        text_align.error_counts(["a " * 262145], ["a"])
    # a caller's workspace goes by its pointer and its size; map is the caller's tensor
    dry.calls.clear()
    mp = torch.full((4,), 77, dtype=I32)
    d, c, m2, st = ops.text_align(torch.zeros(4, dtype=I32), cu([4]), torch.zeros(3, dtype=I32), cu([3]), 4, 3, 1, True, col_block=64,
                                  row_block=64, map=mp, workspace=torch.zeros(4096, dtype=torch.uint8))
    assert m2 is mp and mp.tolist() == [77] * 4 and d.shape == (1,) and c.shape == (1, 4) and st.shape == (1,)
    assert ops.text_align(torch.zeros(4, dtype=I32), cu([4]), torch.zeros(3, dtype=I32), cu([3]), 4, 3, 0, False)[2] is None
    assert dry.calls == ["ta_text_align_i32"] * 2


def test_encode():
    r, cu_r, h, cu_h = text_align.encode(["The cat  sat", "", "a"], ["the cat", "x y", "a"], normalize=str.lower)
    assert cu_r.tolist() == [0, 3, 3, 4] and cu_h.tolist() == [0, 2, 4, 5]
    assert r.dtype == cu_r.dtype == h.dtype == cu_h.dtype == np.int32
    assert r[0] == h[0] and r[1] == h[1] and r[3] == h[4] and len(set(r.tolist()) | set(h.tolist())) == 6     # one dictionary per call
    assert text_align.encode(["The"], ["the"])[0][0] != text_align.encode(["The"], ["the"])[2][0]             # no normaliser: distinct
    r, cu_r, h, cu_h = text_align.encode("héllo", "hello", unit="char")
    assert r.tolist() == [ord(c) for c in "héllo"] and h.tolist() == [ord(c) for c in "hello"] and cu_r.tolist() == [0, 5]


def test_word_error_rate_without_device_is_unchanged():
    """The default path is the host loop it was: the same value as the definition on text_post.json's strings, and no device call."""
    assert inspect.signature(eval_text.word_error_rate).parameters["device"].default is None
    g = json.load(open(os.path.join(GOLDEN, "text_post.json")))
    refs = [src for src, _ in g["truncate"]]
    hyps = [out for _, out in g["truncate"]]
    refs, hyps = [r for r in refs if r.split()] + ["a b c d"], [h for r, h in zip(refs, hyps) if r.split()] + ["a x d e"]
    assert len(refs) >= 10
    edits = total = 0
    table = {}
    for r, h in zip(refs, hyps):
        ri, hi = ([table.setdefault(w, len(table)) for w in t.split()] for t in (r, h))
        edits += R.edit_table_cells(ri, hi)[len(ri)][len(hi)]
        total += len(ri)
    assert edits > 0
    _lib.DRY_RUN = True                                                    # any call into the library would be recorded
    try:
        L = _lib.lib()
        L.calls.clear()
        assert eval_text.word_error_rate(refs, hyps) == edits / total
        assert eval_text.word_error_rate("a b c", "a c") == 1 / 3
        assert eval_text.word_error_rate(["A b"], ["a b"], normalize=str.lower) == 0.0
        assert L.calls == []
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None
    with pytest.raises(ValueError, match="empty reference"):
        eval_text.word_error_rate([""], ["a"])
