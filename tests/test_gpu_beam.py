"""-m gpu: beam search -- the kernels of csrc/beam.hip against float64 / numpy / tests/beam_ref.py (which tests/test_beam_ref.py pins to
HF's own beam search), and ``ASRModel.generate_beams`` end to end on the generate_small.npz model.  Every test fails on the parent,
where neither the symbols nor the method exist.

Gates.  ``ta_beam_logprobs_f32``: |x - ref| <= 5e-6 (1 + |ref|) against a float64 log-softmax, the project's bound for
log-probabilities (tests/test_gpu_scores.py).  ``ta_beam_topk_f32``, ``ta_beam_advance``, the cache kernels: exact.  End to end: the
device's candidates are the fp32 oracle's within the 0.12 the generation tests grant the bf16 model on near-ties; the restatement fed
the device's own candidates reproduces the device's state and output exactly; captured and eager runs agree bit for bit; the cache
rows of the final beams equal those of a teacher-forced pass of the final running sequences.
"""
import ctypes as C_

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import beam_ref as BR
from tests import decode_options_ref as R
from tests.test_gpu_decode_options import _oracle_last, ctx  # noqa: F401  (the generate_small.npz model, built once per module)

DEV = "cuda"
F32, I32, I64 = torch.float32, torch.int32, torch.int64
POISON = 7.0


def _bits():
    from tiny_audio_amd import _lib
    return _lib, _lib.lib(), (lambda t: None if t is None else C_.c_void_p(t.data_ptr())), C_.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device_rows(x, ld):
    buf = torch.full((x.shape[0], ld), POISON, dtype=F32, device=DEV)
    buf[:, :x.shape[1]] = torch.from_numpy(np.ascontiguousarray(x))
    return buf


# ============================================================================ ta_beam_logprobs_f32
@pytest.mark.parametrize("R_, V, ld", [(1, 1003, 1024), (5, 1003, 1024), (8, 151670, 151680)])
def test_logprobs_against_float64(R_, V, ld):
    from tiny_audio_amd import ops
    rng = np.random.default_rng(V + R_)
    x = (rng.standard_normal((R_, V)) * 4).astype(np.float32)
    x[:, rng.integers(0, V, 37)] = -np.inf
    x[-1, :] = -np.inf
    x[-1, V - 2] = 1.5                                                      # one row with a single finite entry
    buf = _device_rows(x, ld)
    ops.beam_logprobs(buf, V)
    got = buf.cpu().numpy()
    assert (got[:, V:] == POISON).all(), "columns >= V were written"
    x64 = x.astype(np.float64)
    m = x64.max(-1, keepdims=True)
    ref = (x64 - m) - np.log(np.exp(x64 - m).sum(-1, keepdims=True))
    got = got[:, :V]
    assert np.array_equal(np.isneginf(got), np.isneginf(x)) and not np.isnan(got).any()
    fin = np.isfinite(ref)
    err = np.abs(got[fin] - ref[fin]) / (1 + np.abs(ref[fin]))
    print(f"logprobs R={R_} V={V}: max scaled error {err.max():.3g}")
    assert err.max() <= 5e-6
    assert got[-1, V - 2] == 0.0


# ============================================================================ ta_beam_topk_f32
def _topk_case(B, K, V, M, seed):
    rng = np.random.default_rng(seed)
    rows = (rng.standard_normal((B * K, V)) * 3 - 8).astype(np.float32)
    score = -(rng.random((B, K)) * 5).astype(np.float32)
    # clip 0: M + 2 equal values, spread over beams with equal scores and adjacent inside one beam: ties in the top M and across its edge
    if K > 1:
        score[0, 1] = score[0, 0]
    cols = [3, 4, 5, 6, V - 1, V - 2, 517] + list(range(700, 700 + M))
    for n in range(M + 2):
        rows[(n % min(K, 2)), cols[n % len(cols)] + (n // len(cols))] = 40.0
    if B > 1:                                                               # clip 1: every winner in ONE beam, consecutive columns (one lane's float4s)
        k0 = K - 1
        rows[K + k0, 100:100 + M + 3] = 30.0 + rng.permutation(M + 3).astype(np.float32)
        rows[K + k0, V - 3:] += 60.0                                        # ... and in the last partial slice of the row
    if B > 2:                                                               # clip 2: fewer than M finite entries, and the first step's scores
        rows[2 * K:3 * K] = -np.inf
        rows[2 * K, [7, V - 1]] = [-1.0, -2.0]
        if K > 1:
            rows[2 * K + 1, 9] = 5.0
        score[2] = [0.0] + [-1.0e9] * (K - 1)
    return rows, score


@pytest.mark.parametrize("n_eos", [0, 1, 3])
@pytest.mark.parametrize("B, K, V, ld", [(1, 1, 1003, 1024), (2, 4, 1003, 1024), (3, 8, 1003, 1024), (2, 4, 151670, 151680)])
def test_topk_is_bit_exact(B, K, V, ld, n_eos):
    from tiny_audio_amd import ops
    M = BR.n_candidates(K, n_eos)
    rows, score = _topk_case(B, K, V, M, 11 * K + n_eos)
    cs, cf = ops.beam_topk(_device_rows(rows, ld), V, torch.from_numpy(score).to(DEV), M)
    acc = (rows.reshape(B, K, V) + score[:, :, None]).astype(np.float32).reshape(B, K * V)
    order = np.argsort(-acc, axis=-1, kind="stable")[:, :M]
    assert np.array_equal(cf.cpu().numpy(), order.astype(np.int32)), (cf.cpu().numpy(), order)
    assert np.array_equal(cs.cpu().numpy(), np.take_along_axis(acc, order, -1))


def test_library_refuses_shapes_outside_the_envelope():
    _lib, L_, ptr, st = _bits()
    x = torch.zeros((9, 128), dtype=F32, device=DEV)
    s = torch.zeros(9, dtype=F32, device=DEV)
    o, oi = torch.zeros(64, dtype=F32, device=DEV), torch.zeros(64, dtype=I32, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    assert L_.ta_beam_topk_f32(ptr(x), 128, 100, ptr(s), 1, 9, 18, ptr(o), ptr(oi), ptr(ws), ws.numel(), st) == 1       # K = 9
    assert L_.ta_beam_topk_f32(ptr(x), 128, 100, ptr(s), 1, 8, 40, ptr(o), ptr(oi), ptr(ws), ws.numel(), st) == 1       # M = 40
    assert L_.ta_kv_beam_reorder(ptr(x), ptr(x), 1, 1, 9, 1, 1, 2, 128, 1, ptr(oi), ptr(oi), st) == 1
    assert L_.ta_kv_beam_expand(ptr(x), ptr(x), ptr(x), ptr(x), 1, 1, 0, 1, 1, 1, 2, 128, st) == 1
    assert (o == 0).all() and (oi == 0).all()


# ============================================================================ ta_beam_advance
def _state(B, K, max_new, L, pad):
    R_, Lmax = B * K, L + max_new
    z = lambda *s, dt=I32: torch.zeros(s, dtype=dt, device=DEV)  # noqa: E731
    kmask = z(R_, Lmax)
    kmask[:, :L] = 1
    return dict(run_seq=torch.full((R_, max_new), pad, dtype=I64, device=DEV),
                run_score=torch.tensor([0.0] + [-1.0e9] * (K - 1), dtype=F32, device=DEV).repeat(B).contiguous(), parent=z(R_),
                next_ids=z(R_, dt=I64), pool_seq=torch.full((B, K, max_new), pad, dtype=I64, device=DEV),
                pool_score=torch.full((B, K), -1.0e9, dtype=F32, device=DEV), pool_len=z(B, K), pool_fin=z(B, K),
                heur=torch.ones(B, dtype=I32, device=DEV), clip_done=z(B), step_dev=z(1), slot_dev=torch.full((1,), L, dtype=I32, device=DEV),
                pos=torch.full((R_,), L, dtype=I32, device=DEV), kmask=kmask, n_unfinished=torch.full((1,), B, dtype=I32, device=DEV))


def _compare_state(s, st, t, L, where=""):
    """device state dict ``s`` against the BeamState ``st`` after step t (0-based)."""
    B, K, max_new = st.B, st.K, st.max_new
    g = {k: v.cpu().numpy() for k, v in s.items()}
    assert np.array_equal(g["run_seq"].reshape(B, K, max_new)[:, :, :t + 1], st.run_seq[:, :, :t + 1]), where
    assert np.array_equal(g["run_score"].reshape(B, K), st.run_score), (where, g["run_score"], st.run_score)
    assert np.array_equal(g["parent"].reshape(B, K), st.parent) and np.array_equal(g["next_ids"].reshape(B, K), st.next_ids), where
    fin = st.pool_fin
    assert np.array_equal(g["pool_fin"].astype(bool), fin), (where, g["pool_fin"], fin)
    assert np.array_equal(g["pool_score"][fin], st.pool_score[fin]) and np.array_equal(g["pool_len"][fin], st.pool_len[fin]), where
    assert np.array_equal(g["pool_seq"][fin], st.pool_seq[fin]), where
    assert np.array_equal(g["heur"].astype(bool), st.heur) and np.array_equal(g["clip_done"].astype(bool), st.done), (where, g["heur"], st.heur)
    assert int(g["step_dev"][0]) == t + 1 and int(g["slot_dev"][0]) == L + t and int(g["n_unfinished"][0]) == int((~st.done).sum()), where
    assert (g["pos"] == L + t).all(), where
    want = np.zeros_like(g["kmask"])
    want[:, :L + t + 1] = 1
    assert np.array_equal(g["kmask"], want), where


def _synthetic_candidates(t, B, K, M, V, eos, max_new, rng):
    """Descending scores and distinct flat indices for every clip; eos placement by clip and step (see the test's docstring)."""
    cs = -np.sort(rng.random((B, M)).astype(np.float32) * 3, axis=-1) - np.float32(1.5 * t)
    cs = np.sort(cs, axis=-1)[:, ::-1].copy()
    par = rng.integers(0, K, (B, M))
    tok = np.stack([rng.choice(np.arange(10, V - 10), M, replace=False) for _ in range(B)])
    e = lambda n: eos[n % len(eos)]  # noqa: E731
    if eos:
        if t == 1:
            tok[1 % B, 0] = e(0)                                            # eos at rank 0
            tok[2 % B, :K] = [e(i) for i in range(K)]                       # all top K eos: with early_stopping=True the clip is done
        if t == 2:
            tok[1 % B, K:] = [e(i) for i in range(M - K)]                   # eos only at ranks >= K: must not finish
        if t == 3:
            tok[1 % B, :K] = [e(i) for i in range(K)]
    # distinct flat indices: the same token under two parents is fine, the same (parent, token) is not
    for b in range(B):
        seen = set()
        for c in range(M):
            while (par[b, c], tok[b, c]) in seen:
                par[b, c] = (par[b, c] + 1) % K
                if (par[b, c], tok[b, c]) in seen and K == 1:
                    tok[b, c] = 5 + c
            seen.add((par[b, c], tok[b, c]))
    return cs, (par * V + tok).astype(np.int32)


@pytest.mark.parametrize("lp", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("es", [False, True, "never"])
@pytest.mark.parametrize("K, n_eos", [(4, 2), (1, 1), (3, 0)])
def test_advance_is_bit_exact(K, n_eos, es, lp):
    """max_new steps of synthetic candidate lists, device and restatement side by side from the same initial state: no eos (clip 0
    until the final step), eos at rank 0, eos only at ranks >= K, all top K eos, the final step (everything hits), and a clip that
    becomes done while the others continue (early_stopping=True).  Every state item is compared after every step."""
    from tiny_audio_amd import ops
    B, V, max_new, L, pad = 3, 1003, 6, 5, 990
    eos = [900, 901, 902][:n_eos]
    M = BR.n_candidates(K, n_eos)
    rng = np.random.default_rng(K * 100 + n_eos)
    s = _state(B, K, max_new, L, pad)
    st = BR.BeamState(B, K, max_new, eos_ids=eos, pad_id=pad, length_penalty=lp, early_stopping=es)
    div = ops.beam_length_divisors(lp, max_new).to(DEV)
    assert np.array_equal(div.cpu().numpy(), st.div)
    seen_done = set()
    for t in range(max_new):
        cs, cf = _synthetic_candidates(t, B, K, M, V, eos, max_new, rng)
        ops.beam_advance(torch.from_numpy(cs).to(DEV), torch.from_numpy(cf).to(DEV), V, eos, pad, div, es, lp, s)
        st.step(cs, cf, V)
        _compare_state(s, st, t, L, where=f"step {t}")
        seen_done.add(tuple(st.done.tolist()))
    assert st.done.all()                                                    # the final step ends every clip
    if es is True and n_eos and K > 1:
        assert any(any(d) and not all(d) for d in seen_done), "no step with one clip done and another running"
    assert st.pool_fin.all()


# ============================================================================ the cache kernels
@pytest.mark.parametrize("slot", [5, 6, 11])
def test_kv_expand_and_reorder_are_exact(slot):
    from tiny_audio_amd import ops
    nl, B, K, hkv, hd, L, Lmax = 2, 2, 4, 2, 128, 5, 12
    g = torch.Generator(device="cpu").manual_seed(slot)
    ksrc, vsrc = (torch.randn((nl, B, hkv, L, hd), generator=g).to(torch.bfloat16).to(DEV) for _ in range(2))
    kd, vd = ops.kv_beam_expand(ksrc, vsrc, K, Lmax)
    for dst, src in ((kd, ksrc), (vd, vsrc)):
        assert torch.equal(dst[:, :, :, :L], src.repeat_interleave(K, 1))
    parents = [[0, 1, 2, 3, 0, 1, 2, 3], [1, 2, 3, 0, 3, 0, 1, 2], [2, 2, 2, 2, 0, 0, 0, 0], [0, 1, 2, 3, 3, 3, 1, 0]]
    slot_dev = torch.tensor([slot], dtype=I32, device=DEV)
    for p in parents:
        kc, vc = (torch.randn((nl, B * K, hkv, Lmax, hd), generator=g).to(torch.bfloat16).to(DEV) for _ in range(2))
        k0, v0 = kc.clone(), vc.clone()
        par = torch.tensor(p, dtype=I32, device=DEV)
        ops.kv_beam_reorder(kc, vc, K, L, Lmax - L, par, slot_dev)
        src_row = (torch.arange(B * K, device=DEV) // K) * K + par.long()
        for got, old in ((kc, k0), (vc, v0)):
            want = old.clone()
            want[:, :, :, L:slot] = old[:, src_row][:, :, :, L:slot]
            assert torch.equal(got, want), (p, slot)                        # prompt slots and slots >= *slot_dev unchanged, the rest permuted


# ============================================================================ end to end
def _beams(ctx, K=4, max_new=8, eos=(), nrs=1, **opt):
    out, tr = ctx.m.generate_beams(**ctx.kw, max_new_tokens=max_new, eos_token_id=list(eos), num_beams=K, num_return_sequences=nrs,
                                   return_beam_trace=True, **opt)
    return out, tr


def _np(t):
    return t.detach().cpu().numpy()


def _check_candidates(ctx, tr, K, max_new, eos, tol=0.12, **opt):
    """(a): every candidate's step score is the oracle's processed log-probability of that token on the device's own prefix, within
    tol; no oracle continuation outside the device's set beats the device's M-th candidate by more than tol."""
    cs, cf = _np(tr["cand_score"]), _np(tr["cand_flat"]).astype(np.int64)
    rseq, rsc = _np(tr["running_sequences"]), _np(tr["running_scores"])
    n_steps, B, M = cs.shape
    V = ctx.V
    prompt = np.asarray(ctx.batch["input_ids"], np.int64)
    worst = 0.0
    for t in range(n_steps):
        lp = np.empty((B, K, V), np.float32)
        for k in range(K):
            if t == 0 and k > 0:
                lp[:, k] = lp[:, 0]
                continue
            tokens = rseq[t, :, k, :]
            x = _oracle_last(ctx, tokens, t).astype(np.float64)
            x = (x - x.max(-1, keepdims=True)) - np.log(np.exp(x - x.max(-1, keepdims=True)).sum(-1, keepdims=True))
            context = np.concatenate([prompt, tokens[:, :t]], axis=1)
            lp[:, k] = R.process(x.astype(np.float32), context, t, max_new, V, eos_ids=tuple(eos), **opt)
        for b in range(B):
            live = rsc[t, b] > -1.0e8
            acc = np.where(live[:, None], lp[b].astype(np.float64) + rsc[t, b][:, None], -np.inf)
            inset = np.zeros(K * V, bool)
            for c in range(M):
                if not np.isfinite(cs[t, b, c]):
                    continue
                k, v = divmod(int(cf[t, b, c]), V)
                assert live[k], (t, b, c)
                d = abs((float(cs[t, b, c]) - float(rsc[t, b, k])) - float(lp[b, k, v]))
                worst = max(worst, d)
                assert d < tol, (t, b, c, k, v, d)
                inset[cf[t, b, c]] = True
            rest = acc.reshape(-1)[~inset]
            assert rest.max() <= float(cs[t, b, M - 1]) + tol, (t, b, float(rest.max()), float(cs[t, b, M - 1]))
    print(f"candidate scores: largest deviation from the oracle {worst:.4f}")


def _check_replay(ctx, out, tr, K, max_new, eos, lp, es, nrs):
    """(b): beam_ref on the device's candidate lists reproduces the running state before every step, the final state and the output."""
    cs, cf = _np(tr["cand_score"]), _np(tr["cand_flat"])
    B = cs.shape[1]
    st = BR.BeamState(B, K, max_new, eos_ids=eos, pad_id=ctx.pad, length_penalty=lp, early_stopping=es)
    for t in range(cs.shape[0]):
        assert np.array_equal(_np(tr["running_sequences"])[t][:, :, :t], st.run_seq[:, :, :t]), t
        assert np.array_equal(_np(tr["running_scores"])[t], st.run_score), t
        st.step(cs[t], cf[t], ctx.V)
        assert np.array_equal(_np(tr["parent"])[t], st.parent), t
    n = cs.shape[0]
    assert np.array_equal(_np(tr["final_running_sequences"])[:, :, :n], st.run_seq[:, :, :n])
    assert np.array_equal(_np(tr["final_running_scores"]), st.run_score)
    assert np.array_equal(_np(tr["pool"]["finished"]).astype(bool), st.pool_fin)
    assert np.array_equal(_np(tr["clip_done"]).astype(bool), st.done)
    assert st.pool_fin[:, :nrs].all()
    seq, score = st.result(nrs)
    assert np.array_equal(_np(out.sequences), seq) and np.array_equal(_np(out.sequences_scores), score)
    return st


def test_e2e_beams_follow_the_oracle_and_the_restatement(ctx):
    K, N = 4, 8
    eos = [int(ctx.plain[0, 3])]
    out, tr = _beams(ctx, K, N, eos)
    assert out.sequences.dtype == torch.int64 and out.sequences_scores.dtype == F32 and out.sequences.shape[0] == ctx.plain.shape[0]
    _check_candidates(ctx, tr, K, N, eos)
    _check_replay(ctx, out, tr, K, N, eos, 1.0, False, 1)
    # (c) captured and eager runs agree bit for bit
    out2, tr2 = _beams(ctx, K, N, eos, use_graph=False)
    assert torch.equal(out.sequences, out2.sequences) and torch.equal(out.sequences_scores, out2.sequences_scores)
    n = min(tr["n_steps"], tr2["n_steps"])
    for k in ("cand_score", "cand_flat", "running_sequences", "running_scores", "parent"):
        assert torch.equal(tr[k][:n], tr2[k][:n]), k


def test_e2e_options_two_eos_and_n_best(ctx):
    K, N = 4, 8
    eos = [int(ctx.plain[0, 3]), int(ctx.plain[1 % ctx.plain.shape[0], 2])]
    opt = dict(bad_words_ids=[[int(ctx.plain[0, 0])]], repetition_penalty=1.3)
    out, tr = _beams(ctx, K, N, eos, nrs=K, length_penalty=2.0, early_stopping=True, **opt)
    assert tr["n_candidates"] == 3 * K
    _check_candidates(ctx, tr, K, N, eos, **opt)
    _check_replay(ctx, out, tr, K, N, eos, 2.0, True, K)
    sc = _np(out.sequences_scores).reshape(-1, K)
    assert (np.diff(sc, axis=-1) <= 0).all(), sc                            # n-best: descending per clip
    assert int(ctx.plain[0, 0]) not in _np(out.sequences)[:K]


def test_e2e_one_beam_is_greedy_and_the_cache_follows_the_beams(ctx):
    """(d): K = 1 with early_stopping=True returns the greedy tokens up to and including every clip's first eos; with K = 4 the
    final cache rows equal, over the generated slots, those of a teacher-forced pass of the final running sequences through the
    unchanged decode step (a wrong permutation of the cache cannot pass)."""
    N = 8
    eos = [int(ctx.plain[0, 3])]
    greedy = ctx.m.generate(**ctx.kw, max_new_tokens=N, eos_token_id=eos).cpu().numpy()
    out, _ = _beams(ctx, 1, N, eos, early_stopping=True)
    one = _np(out.sequences)
    for b in range(greedy.shape[0]):
        hit = np.isin(greedy[b], eos)
        n = int(hit.argmax()) + 1 if hit.any() else greedy.shape[1]
        assert np.array_equal(one[b, :n], greedy[b, :n]), (b, one[b], greedy[b])
    K = 4
    out, tr = _beams(ctx, K, N, [])
    kc, vc = tr["cache"]
    L, n_steps = tr["prompt_len"], tr["n_steps"]
    seq = tr["final_running_sequences"].reshape(-1, N)
    R_, Lmax = seq.shape[0], kc.shape[3]
    assert n_steps == N and (_np(tr["parent"])[1:] != np.arange(K)).any(), "the beams never switched parents: the check would be empty"
    _lib, L_, ptr, st = _bits()
    lm = ctx.m.language_model
    k2, v2 = torch.zeros_like(kc), torch.zeros_like(vc)
    k2[:, :, :, :L], v2[:, :, :, :L] = kc[:, :, :, :L], vc[:, :, :, :L]
    ws = torch.empty(L_.ta_lm_decode_workspace_bytes(C_.byref(lm._w), R_), dtype=torch.uint8, device=DEV)
    logits = torch.empty((R_, lm.vocab_pad), dtype=F32, device=DEV)
    kmask = torch.zeros((R_, Lmax), dtype=I32, device=DEV)
    kmask[:, :L] = 1
    for t in range(n_steps - 1):                                            # the decode steps the beam run executed: inputs = tokens 0 .. n_steps - 2
        kmask[:, L + t] = 1
        pos = torch.full((R_,), L + t, dtype=I32, device=DEV)
        slot = torch.tensor([L + t], dtype=I32, device=DEV)
        ids = seq[:, t].contiguous()
        _lib.check(L_.ta_lm_decode_step(C_.byref(lm._w), ptr(ids), ptr(pos), ptr(kmask), ptr(slot), R_, ptr(k2), ptr(v2), Lmax, ptr(logits),
                                        None, ptr(ws), ws.numel(), st), "ta_lm_decode_step")
    torch.cuda.synchronize()
    hi = L + n_steps - 1
    assert torch.equal(k2[:, :, :, L:hi], kc[:, :, :, L:hi]) and torch.equal(v2[:, :, :, L:hi], vc[:, :, :, L:hi])


# ============================================================================ the true vocabulary
def test_three_steps_at_the_true_vocabulary():
    """B = 2, K = 4, V = 151 670: random logits through log-softmax, a repetition penalty, top-k and the bookkeeping for three steps;
    the restatement ranks the device's own processed rows and must agree exactly at every step."""
    from tiny_audio_amd import ops
    _lib, L_, ptr, st_ = _bits()
    B, K, V, ld, max_new, L, pad = 2, 4, 151670, 151680, 4, 3, 0
    eos = [77]
    M = BR.n_candidates(K, 1)
    rng = np.random.default_rng(5)
    s = _state(B, K, max_new, L, pad)
    st = BR.BeamState(B, K, max_new, eos_ids=eos, pad_id=pad, length_penalty=1.0, early_stopping=False)
    div = ops.beam_length_divisors(1.0, max_new).to(DEV)
    prompt = torch.from_numpy(rng.integers(0, V, (B * K, L))).to(DEV)
    for t in range(3):
        x = (rng.standard_normal((B * K, V)) * 3).astype(np.float32)
        x[:, 77] += 9.0                                                     # eos among the likely tokens
        buf = _device_rows(x, ld)
        ops.beam_logprobs(buf, V)
        _lib.check(L_.ta_logits_process(ptr(buf), ld, V, ptr(prompt), L, ptr(s["run_seq"]), max_new, ptr(s["step_dev"]), B * K, 1.2, 0, st_),
                   "ta_logits_process")
        rows = buf.cpu().numpy()[:, :V]
        cs, cf = ops.beam_topk(buf, V, s["run_score"].reshape(B, K), M)
        ref_cs, ref_cf = BR.candidates(rows, st.run_score, M)
        assert np.array_equal(cf.cpu().numpy(), ref_cf.astype(np.int32)) and np.array_equal(cs.cpu().numpy(), ref_cs), t
        ops.beam_advance(cs, cf, V, eos, pad, div, False, 1.0, s)
        st.step(ref_cs, ref_cf, V)
        _compare_state(s, st, t, L, where=f"step {t}")
