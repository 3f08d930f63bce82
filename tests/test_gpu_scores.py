"""-m gpu: decoding scores -- ``ta_token_scores_f32`` (csrc/generate.hip) against the fp64 reference of tests/scores_ref.py, its column
addressing and finished rows, the true vocabulary width once, and ``ASRModel.generate(return_token_scores=True, top_logprobs=k)`` end
to end on the generate_small.npz model (steps 2.. run from the captured hipGraph).

Kernel gates (issue "Decoding scores"): |logprob - ref| <= 5e-6 (1 + |ref|), |entropy - ref| <= 2e-5, top_ids exact, top_logprobs held
to the logprob gate.  Origin: a float32 emulation of the one-pass (m, s, t) scheme (correctly rounded exp, 1024 lanes, tree merge) on these
value classes up to V = 151 670 gave at most 8e-8 (1 + |ref|) and 6.6e-7 against fp64; a fast __expf adds about
1.2e-7 sum p|z| + 2.4e-7 to log s and 1.2e-7 sum p z^2 to the entropy; the gates leave a factor 3 and 8 over that.

End-to-end gate against the fp32 oracle (teacher-forced on the device's own tokens): the difference is bf16 model arithmetic against
fp32, which cannot be derived; it was measured (profiles/decode_scores.md) and is gated at 3 x the recorded value, the recorded value
itself being far below the 0.12 logit gap the project accepts between the cache path and the full forward.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import weights as OW
from tests.golden import recipe as R
from tests.scores_ref import teacher_forced_logits, token_scores_ref

DEV = "cuda"
F32 = torch.float32

# max |device - oracle| over the unfinished positions as recorded in profiles/decode_scores.md (the same in the plain greedy run and the
# no_repeat_ngram run, which share the early step where it occurs; the same in two sessions)
REC_LOGPROB, REC_ENTROPY = 0.02702, 0.00192
GATE = 3.0


def _bits():
    from tiny_audio_amd import _lib
    return _lib, _lib.lib(), (lambda t: None if t is None else C.c_void_p(t.data_ptr())), C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rows(kinds, V, rng):
    """One row per entry of ``kinds`` (the issue's value classes, in its order), float32 [len(kinds), V]."""
    out = np.zeros((len(kinds), V), np.float32)
    for r, kind in enumerate(kinds):
        if kind == 0:
            out[r] = 2.5 * rng.standard_normal(V)
        elif kind == 1:
            out[r] = 0.0
        elif kind == 2:
            out[r] = 3e4
        elif kind == 3:
            out[r] = -3e4
        elif kind == 4:
            out[r] = 12.0 * rng.standard_normal(V)
        elif kind == 5:
            out[r, rng.randint(V)] = 80.0
        elif kind == 6:
            out[r] = -np.inf
            keep = rng.choice(V, min(6, V), replace=False)
            out[r, keep] = 3.0 * rng.standard_normal(keep.size)
        elif kind == 7:
            out[r] = -np.inf
            out[r, rng.randint(V)] = 1.5 * rng.standard_normal()
        else:                                                   # 8: five exact duplicates of the maximum
            out[r] = 2.5 * rng.standard_normal(V)
            out[r, rng.choice(V, min(5, V), replace=False)] = np.float32(out[r].max() + 1.25)
    return out


def _device_rows(x, ld):
    """x [B, V] -> device buffer [B, ld] whose columns >= V are half NaN, half +inf."""
    B, V = x.shape
    buf = torch.empty((B, ld), dtype=F32, device=DEV)
    pad = np.full((B, ld - V), np.nan, np.float32)
    pad[:, 1::2] = np.inf
    buf.copy_(torch.from_numpy(np.concatenate([x, pad], axis=1)))
    return buf


def _launch(buf, V, chosen, k, finished=None, step=None, max_new=1, out=None):
    _lib, L_, ptr, st = _bits()
    B, ld = buf.shape
    if out is None:
        out = (torch.empty((B, max_new), dtype=F32, device=DEV), torch.empty((B, max_new), dtype=F32, device=DEV),
               torch.empty((B, max_new, k), dtype=torch.int64, device=DEV), torch.empty((B, max_new, k), dtype=F32, device=DEV))
    lp, ent, ids, tl = out
    _lib.check(L_.ta_token_scores_f32(ptr(buf), ld, V, B, ptr(chosen), ptr(finished), ptr(step), max_new, k, ptr(lp), ptr(ent),
                                      ptr(ids) if k else None, ptr(tl) if k else None, st), "ta_token_scores_f32")
    return out


def _close_lp(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    inf = np.isneginf(ref)
    ok = np.array_equal(np.isneginf(got), inf) and not np.isnan(got).any()
    err = np.abs(np.where(inf, 0.0, got) - np.where(inf, 0.0, ref)) / (1.0 + np.abs(np.where(inf, 0.0, ref)))
    return ok and bool((err <= 5e-6).all()), float(err.max()) if err.size else 0.0


def _check(buf, x, V, chosen_np, k, ref, tag):
    """ref: token_scores_ref(x, V, chosen, 8); the first k alternatives of the top 8 are the top k."""
    chosen = torch.from_numpy(chosen_np).to(DEV)
    lp, ent, ids, tl = (t.cpu().numpy() for t in _launch(buf, V, chosen, k))
    rl, re, ri, rt = ref
    ok, e1 = _close_lp(lp[:, 0], rl)
    assert ok, (tag, "logprob", e1, lp[:, 0], rl)
    e2 = float(np.abs(ent[:, 0].astype(np.float64) - re).max())
    assert not np.isnan(ent).any() and e2 <= 2e-5, (tag, "entropy", e2)
    if k:
        assert np.array_equal(ids[:, 0], ri[:, :k]), (tag, "top_ids", ids[:, 0], ri[:, :k])
        ok, e3 = _close_lp(tl[:, 0], rt[:, :k])
        assert ok, (tag, "top_logprobs", e3)
        e1 = max(e1, e3)
    return e1, e2


# ============================================================================ (a) the kernel against the fp64 reference
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 1023, 1024, 1025, 4099])
def test_kernel_vs_fp64_reference(V):
    """Every value class x B in {1, 3, 33} x both row layouts (ld = V + 7: rows 1.. are not 16-byte aligned -> the scalar path; ld = V
    rounded up to 16 plus 16: the float4 path with a ragged tail) x top_k in {0, 1, 4, 8} x chosen = the argmax / the smallest finite
    entry.  Columns >= V hold NaN and +inf."""
    rng = np.random.RandomState(1000 + V)
    worst = [0.0, 0.0]
    for B in (1, 3, 33):
        for shift in (range(0, 9, B) if B < 9 else (0,)):                 # every class meets every B
            kinds = [(shift + r) % 9 for r in range(B)]
            x = _rows(kinds, V, rng)
            fin = np.isfinite(x)
            c_max = np.where(fin, x, -np.inf).argmax(-1)
            c_min = np.where(fin, x, np.inf).argmin(-1)
            refs = {n: token_scores_ref(x, V, c, 8) for n, c in (("max", c_max), ("min", c_min))}
            for ld in (V + 7, (V + 15) // 16 * 16 + 16):
                buf = _device_rows(x, ld)
                for k in (0, 1, 4, 8):
                    for n, c in (("max", c_max), ("min", c_min)):
                        e1, e2 = _check(buf, x, V, c, k, refs[n], (V, B, kinds[0], ld, k, n))
                        worst = [max(worst[0], e1), max(worst[1], e2)]
    print(f"V = {V}: worst logprob error {worst[0]:.2e} (1 + |ref|) (gate 5e-6), worst entropy error {worst[1]:.2e} (gate 2e-5)")


def test_a_chosen_minus_inf_is_minus_inf_not_nan():
    V, ld = 1025, 1032
    rng = np.random.RandomState(5)
    x = _rows([0, 6, 7], V, rng)
    x[0, 17] = -np.inf
    chosen = np.array([17, int(np.nonzero(~np.isfinite(x[1]))[0][3]), int(np.nonzero(~np.isfinite(x[2]))[0][0])])
    lp, ent, ids, tl = (t.cpu().numpy() for t in _launch(_device_rows(x, ld), V, torch.from_numpy(chosen).to(DEV), 4))
    assert np.isneginf(lp[:, 0]).all()
    rl, re, ri, rt = token_scores_ref(x, V, chosen, 4)
    assert np.isneginf(rl).all() and np.abs(ent[:, 0] - re).max() <= 2e-5 and np.array_equal(ids[:, 0], ri)
    assert 17 not in ids[0, 0] and (ids[2, 0, 1:] == -1).all() and np.isneginf(tl[2, 0, 1:]).all()
    _lib, L_, ptr, st = _bits()                                              # top_k outside [0, 8]: the library's argument error
    for bad in (9, -1):
        assert L_.ta_token_scores_f32(ptr(torch.zeros(1, 8, device=DEV)), 8, 8, 1, ptr(torch.zeros(1, dtype=torch.int64, device=DEV)), None, None, 1,
                                      bad, ptr(torch.zeros(1, device=DEV)), ptr(torch.zeros(1, device=DEV)), None, None, st) == 1


@pytest.mark.parametrize("B,V", [(3, 16383), (3, 16384), (3, 16389), (64, 16385), (65, 16385)])
def test_both_layouts_around_their_thresholds(B, V):
    """ta_token_scores_f32 splits a row over 8 workgroups (and a combine launch) from V = 16 384 on while B <= 64, and keeps one
    workgroup per row otherwise: both sides of both thresholds, every value class, both row alignments, slices that end inside a
    float4, finished rows and the device-side column in the split layout as well."""
    rng = np.random.RandomState(B * 100000 + V)
    worst = [0.0, 0.0]
    for shift in ((0, 3, 6) if B == 3 else (0,)):
        kinds = [(shift + r) % 9 for r in range(B)]
        x = _rows(kinds, V, rng)
        fin = np.isfinite(x)
        c_max, c_min = np.where(fin, x, -np.inf).argmax(-1), np.where(fin, x, np.inf).argmin(-1)
        refs = {n: token_scores_ref(x, V, c, 8) for n, c in (("max", c_max), ("min", c_min))}
        for ld in (V + 7, (V + 15) // 16 * 16 + 16):
            buf = _device_rows(x, ld)
            for k in (0, 1, 4, 8):
                for n, c in (("max", c_max), ("min", c_min)):
                    e1, e2 = _check(buf, x, V, c, k, refs[n], (V, B, kinds[0], ld, k, n))
                    worst = [max(worst[0], e1), max(worst[1], e2)]
    print(f"B = {B}, V = {V}: worst logprob error {worst[0]:.2e} (1 + |ref|), worst entropy error {worst[1]:.2e}")
    # column 2 of [B, 3] buffers from device memory, every other row finished
    SENT = -777.0
    out = (torch.full((B, 3), SENT, dtype=F32, device=DEV), torch.full((B, 3), SENT, dtype=F32, device=DEV),
           torch.full((B, 3, 4), -777, dtype=torch.int64, device=DEV), torch.full((B, 3, 4), SENT, dtype=F32, device=DEV))
    fins = (np.arange(B) % 2).astype(np.int32)
    _launch(buf, V, torch.from_numpy(c_max).to(DEV), 4, finished=torch.from_numpy(fins).to(DEV),
            step=torch.full((1,), 2, dtype=torch.int32, device=DEV), max_new=3, out=out)
    lp, ent, ids, tl = (t.cpu().numpy() for t in out)
    rl, re, ri, rt = refs["max"]
    assert (lp[:, :2] == SENT).all() and (ent[:, :2] == SENT).all() and (ids[:, :2] == -777).all() and (tl[:, :2] == SENT).all()
    dead = fins == 1
    assert (lp[dead, 2] == 0).all() and (ent[dead, 2] == 0).all() and (ids[dead, 2] == -1).all() and np.isneginf(tl[dead, 2]).all()
    assert _close_lp(lp[~dead, 2], rl[~dead])[0] and np.abs(ent[~dead, 2] - re[~dead]).max() <= 2e-5
    assert np.array_equal(ids[~dead, 2], ri[~dead, :4]) and _close_lp(tl[~dead, 2], rt[~dead, :4])[0]


# ============================================================================ (b) column addressing and finished rows
def test_column_addressing_and_finished_rows():
    B, V, ld, k, max_new = 5, 1025, 1040, 4, 4
    rng = np.random.RandomState(7)
    xs = [_rows([0, 4, 6, 8, 0], V, rng) for _ in range(3)]
    SENT = -777.0
    out = (torch.full((B, max_new), SENT, dtype=F32, device=DEV), torch.full((B, max_new), SENT, dtype=F32, device=DEV),
           torch.full((B, max_new, k), -777, dtype=torch.int64, device=DEV), torch.full((B, max_new, k), SENT, dtype=F32, device=DEV))
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    fins = [np.array([0, 0, 0, 0, 0], np.int32), np.array([0, 1, 0, 0, 0], np.int32), np.array([0, 1, 0, 1, 1], np.int32)]
    chosen = [np.where(np.isfinite(x), x, -np.inf).argmax(-1) for x in xs]
    for t in range(3):
        step.fill_(t)                                                         # the column comes from DEVICE memory
        _launch(_device_rows(xs[t], ld), V, torch.from_numpy(chosen[t]).to(DEV), k, finished=torch.from_numpy(fins[t]).to(DEV), step=step,
                max_new=max_new, out=out)
    lp, ent, ids, tl = (t.cpu().numpy() for t in out)
    assert (lp[:, 3] == SENT).all() and (ent[:, 3] == SENT).all() and (ids[:, 3] == -777).all() and (tl[:, 3] == SENT).all()
    for t in range(3):
        rl, re, ri, rt = token_scores_ref(xs[t], V, chosen[t], k)
        for b in range(B):
            if fins[t][b]:
                assert lp[b, t] == 0.0 and ent[b, t] == 0.0 and (ids[b, t] == -1).all() and np.isneginf(tl[b, t]).all(), (t, b)
            else:
                assert _close_lp(lp[b, t], rl[b])[0] and abs(ent[b, t] - re[b]) <= 2e-5 and np.array_equal(ids[b, t], ri[b]), (t, b)
                assert _close_lp(tl[b, t], rt[b])[0], (t, b)
    step.fill_(max_new)                                                       # a step past the buffers writes nothing
    before = [t.clone() for t in out]
    _launch(_device_rows(xs[0], ld), V, torch.from_numpy(chosen[0]).to(DEV), k, step=step, max_new=max_new, out=out)
    assert all(torch.equal(a, b) for a, b in zip(before, out))


# ============================================================================ (c) the true width once
def test_scores_at_the_true_vocabulary():
    """B = 32, V = 151 670, ld = 151 680, top_k = 8 under the same gates; the time per launch is printed next to ta_argmax_f32's at the
    same shape (parity test, not a benchmark: only the loose bound of test_logits_warp_and_sample_at_the_true_vocabulary is asserted)."""
    _lib, L_, ptr, st = _bits()
    B, V, ld = 32, 151670, 151680
    rng = np.random.RandomState(11)
    x = (2.5 * rng.standard_normal((B, V))).astype(np.float32)
    x[1] = (12.0 * rng.standard_normal(V)).astype(np.float32)
    x[2, rng.choice(V, V - 50, replace=False)] = -np.inf                     # a warped row: 50 survivors
    buf = _device_rows(x, ld)
    c = np.where(np.isfinite(x), x, -np.inf).argmax(-1)
    ref = token_scores_ref(x, V, c, 8)
    e1, e2 = _check(buf, x, V, c, 8, ref, "true width")
    chosen = torch.from_numpy(c).to(DEV)
    out = _launch(buf, V, chosen, 8)
    amax = torch.zeros(B, dtype=torch.int64, device=DEV)

    def timed(fn, n=20):
        fn(); torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) / n
    ms_s = timed(lambda: _launch(buf, V, chosen, 8, out=out))
    ms_0 = timed(lambda: _launch(buf, V, chosen, 0, out=out))
    ms_a = timed(lambda: _lib.check(L_.ta_argmax_f32(ptr(buf), ld, V, B, ptr(amax), st), "ta_argmax_f32"))
    assert np.array_equal(amax.cpu().numpy(), c)
    # the other layout (one workgroup per row at every shape) on the same rows: same gates, its time for the record
    import os
    os.environ["TA355_SCORES_SPLIT"] = "0"
    try:
        L_.ta_gemm_reload_knobs()
        d1, d2 = _check(buf, x, V, c, 8, ref, "true width, one workgroup per row")
        ms_d = timed(lambda: _launch(buf, V, chosen, 8, out=out))
        ms_d0 = timed(lambda: _launch(buf, V, chosen, 0, out=out))
    finally:
        del os.environ["TA355_SCORES_SPLIT"]
        L_.ta_gemm_reload_knobs()
    print(f"token scores at V = 151 670, B = 32, per call: top_k = 8 {ms_s * 1e3:.1f} us, top_k = 0 {ms_0 * 1e3:.1f} us (8 workgroups per row + "
          f"combine); one workgroup per row {ms_d * 1e3:.1f} / {ms_d0 * 1e3:.1f} us; ta_argmax_f32 {ms_a * 1e3:.1f} us (ratios {ms_s / ms_a:.2f}, "
          f"{ms_d / ms_a:.2f}); errors {e1:.2e} (1 + |ref|), {e2:.2e}; one workgroup per row {d1:.2e}, {d2:.2e}")
    assert ms_s < 3.0 and ms_d < 3.0


# ============================================================================ (d) end to end
class _Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(golden):
    from tests.test_gpu_parity import build_model
    g = golden("generate_small.npz")
    S = R.SMALL
    E, D, H = S["enc"]["hidden"], S["lm"]["hidden"], S["proj_hidden"]
    wE, wL, wP = OW.init_encoder(S["enc"], 0), R.gen_lm_weights(), OW.init_mlp_projector(E, D, H)
    c = _Ctx()
    c.m = build_model(S["enc"], S["lm"], H, wE, wL, wP, audio_token_id=S["audio_token_id"], pad_token_id=S["pad_id"], eos_token_id=S["eos_id"])
    c.kw = dict(input_ids=torch.from_numpy(g["input_ids"]), input_features=torch.from_numpy(g["input_features"]),
                audio_attention_mask=torch.from_numpy(g["audio_attention_mask"]), attention_mask=torch.ones(g["input_ids"].shape, dtype=torch.int64))
    c.W = dict(encoder=wE, lm=wL, projector=wP)
    c.cfg = dict(enc=S["enc"], lm=S["lm"], projector_type="mlp", k=S["k"], audio_token_id=S["audio_token_id"])
    c.batch = dict(input_ids=g["input_ids"], input_features=g["input_features"])
    c.pad, c.eos_b, c.V = S["pad_id"], int(g["eos_b"]), S["lm"]["vocab"]
    c.eos = [c.eos_b, c.pad]
    c.cache = {}
    return c


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _run_b(ctx):
    """The fixture's early-stopping run (clip 0 emits eos_b), scores and 4 alternatives on; shared by the tests below."""
    if "b" not in ctx.cache:
        ctx.cache["b"] = _np(ctx.m.generate(**ctx.kw, max_new_tokens=12, eos_token_id=ctx.eos, return_token_scores=True, top_logprobs=4))
    return ctx.cache["b"]


def _alive(seq, eos):
    """True where the clip had not finished BEFORE the step."""
    hit = np.isin(seq, eos)
    return np.concatenate([np.ones((seq.shape[0], 1), bool), np.cumsum(hit, axis=1)[:, :-1] == 0], axis=1)


def test_scores_do_not_change_the_tokens(ctx):
    for extra in (dict(), dict(do_sample=True, temperature=1.5, top_k=8, top_p=0.95, seed=11)):
        off = ctx.m.generate(**ctx.kw, max_new_tokens=12, eos_token_id=[], **extra)
        on = ctx.m.generate(**ctx.kw, max_new_tokens=12, eos_token_id=[], return_token_scores=True, top_logprobs=8, **extra)
        assert torch.is_tensor(off) and torch.equal(off, on.sequences), extra
        assert on.token_logprobs.shape == (2, 12) and on.top_logprobs.shape == (2, 12, 8)
        lp = on.token_logprobs.cpu().numpy()
        assert np.isfinite(lp).all() and (lp <= 0).all()
        if extra:                                           # a sampled token is one of the <= 8 survivors of the top-k cut
            ids, seq = on.top_token_ids.cpu().numpy(), on.sequences.cpu().numpy()
            assert (ids == seq[..., None]).any(-1).all()


def test_greedy_invariants_and_finished_positions(ctx):
    o = _run_b(ctx)
    seq, lp, ent, ids, tl = o["sequences"], o["token_logprobs"], o["token_entropy"], o["top_token_ids"], o["top_logprobs"]
    n = seq.shape[1]
    assert lp.shape == ent.shape == (2, n) and ids.shape == tl.shape == (2, n, 4)
    alive = _alive(seq, ctx.eos)
    assert not alive[0].all(), "the fixture's clip 0 stops early"
    assert (ids[..., 0][alive] == seq[alive]).all()
    assert (tl[..., 0][alive] == lp[alive]).all()
    assert (lp <= 0).all() and (ent >= 0).all() and np.isfinite(lp).all() and np.isfinite(ent).all()
    assert (np.diff(tl[alive], axis=-1) <= 0).all()
    dead = ~alive
    assert (lp[dead] == 0).all() and (ent[dead] == 0).all() and (ids[dead] == -1).all() and np.isneginf(tl[dead]).all()
    assert (seq[dead] == ctx.pad).all()


def test_graph_and_eager_steps_give_identical_scores(ctx):
    """Steps 2.. of generate() are replays of one captured step: a column index taken from the host would freeze there."""
    o = _run_b(ctx)
    ctx.m.eval()
    with torch.no_grad():
        args = ctx.m._prepare_generation(ctx.kw["input_ids"], ctx.kw["input_features"], ctx.kw["audio_attention_mask"], ctx.kw["attention_mask"],
                                         None, dict(max_new_tokens=12, eos_token_id=ctx.eos))
    seq, sc = ctx.m.language_model.greedy_decode(**args, token_scores=True, top_logprobs=4, use_graph=False)
    assert np.array_equal(seq.cpu().numpy(), o["sequences"])
    for k in ("token_logprobs", "token_entropy", "top_token_ids", "top_logprobs"):
        assert np.array_equal(sc[k].cpu().numpy(), o[k]), k


def test_top_k_1_sampling_is_certain(ctx):
    o = _np(ctx.m.generate(**ctx.kw, max_new_tokens=12, eos_token_id=[], do_sample=True, top_k=1, seed=7, return_token_scores=True, top_logprobs=2))
    assert (o["token_logprobs"] == 0).all() and (o["token_entropy"] == 0).all()
    assert (o["top_token_ids"][..., 0] == o["sequences"]).all() and (o["top_logprobs"][..., 0] == 0).all()
    assert (o["top_token_ids"][..., 1] == -1).all() and np.isneginf(o["top_logprobs"][..., 1]).all()


def _oracle_errors(ctx, o, eos, **proc):
    steps, alive = teacher_forced_logits(ctx.batch, ctx.W, ctx.cfg, o["sequences"], eos_ids=eos, **proc)
    assert np.array_equal(alive, _alive(o["sequences"], eos))
    B, n = o["sequences"].shape
    rl, re = np.zeros((B, n)), np.zeros((B, n))
    for t, last in enumerate(steps):
        rl[:, t], re[:, t], _, _ = token_scores_ref(last, ctx.V, o["sequences"][:, t], 0)
    d_lp = float(np.abs(o["token_logprobs"] - rl)[alive].max())
    d_ent = float(np.abs(o["token_entropy"] - re)[alive].max())
    return d_lp, d_ent, steps, alive


def test_scores_against_the_oracle(ctx):
    """Teacher-forced on the device's own tokens: bf16 model arithmetic against the fp32 oracle (recorded: profiles/decode_scores.md)."""
    d_lp, d_ent, _, _ = _oracle_errors(ctx, _run_b(ctx), ctx.eos)
    print(f"plain greedy: max |token_logprobs - oracle| = {d_lp:.5f}, max |token_entropy - oracle| = {d_ent:.5f} over unfinished positions")
    assert REC_LOGPROB <= 0.12 and REC_ENTROPY <= 0.12
    assert d_lp <= GATE * REC_LOGPROB and d_ent <= GATE * REC_ENTROPY


def test_no_repeat_ngram_scores_are_of_the_processed_logits(ctx):
    proc = dict(no_repeat_ngram_size=2)
    o = _np(ctx.m.generate(**ctx.kw, max_new_tokens=12, eos_token_id=[], return_token_scores=True, top_logprobs=8, **proc))
    d_lp, d_ent, steps, alive = _oracle_errors(ctx, o, [], **proc)
    print(f"no_repeat_ngram_size = 2: max |token_logprobs - oracle| = {d_lp:.5f}, max |token_entropy - oracle| = {d_ent:.5f}")
    assert d_lp <= GATE * REC_LOGPROB and d_ent <= GATE * REC_ENTROPY
    banned_seen = 0
    for t, last in enumerate(steps):
        for b in range(last.shape[0]):
            banned = np.nonzero(np.isneginf(last[b]))[0]
            banned_seen += banned.size
            fin = np.isfinite(o["top_logprobs"][b, t])
            assert not np.isin(o["top_token_ids"][b, t][fin], banned).any(), (b, t)
            assert o["sequences"][b, t] not in banned
    assert banned_seen > 0, "the run never banned a token: the case checks nothing"
