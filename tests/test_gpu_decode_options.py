"""-m gpu: the decoding options -- ``ta_logits_sequence_bias``, ``ta_logits_step_rules``, ``ta_logits_warp_ext`` (csrc/generate.hip)
against the numpy restatement of tests/decode_options_ref.py (pinned to HF's own outputs by tests/test_decode_options_host.py), and
``ASRModel.generate`` / ``generate_streaming`` with the options end to end on the generate_small.npz model.

Gates.  Bias and step rules: bit-identical to the restatement (float32, HF's operations in HF's order).  Warpers: against the float64
restatement -- every element outside its band agrees, every survivor keeps its value, nothing is NaN, columns >= V keep their poison;
inside the band an element may fall on either side.  The bands come from tests/golden/decode_options.npz: 4 x the largest relative
distance from the float64 threshold at which HF's own float32 warpers disagree with float64 on these very inputs (seeds 100..103, both
widths), floor 1e-5; at most max(2, V / 2000) elements per row may lie inside (a condition on the inputs, checked on the reference).
Like HF's TypicalLogitsWarper, typical_p keeps the element nearest the entropy and may remove the row maximum; the other three never
remove it.  End to end: every device decision is the processed fp32 argmax of the oracle on the device's own prefix, or within the
0.12 logit tolerance the existing generation tests accept for bf16 near-ties.
"""
import ctypes as C_

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import generate as OG
from oracle import qwen3 as OQ
from oracle import weights as OW
from tests import decode_options_ref as R
from tests.golden import recipe as RC

DEV = "cuda"
F32 = torch.float32
POISON = 7.0
CASES = R.CASES
SHAPES = ((1003, 1024), (151670, 151680))


def _bits():
    from tiny_audio_amd import _lib
    return _lib, _lib.lib(), (lambda t: None if t is None else C_.c_void_p(t.data_ptr())), C_.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device_rows(x, ld):
    """x [B, V] -> device buffer [B, ld] whose columns >= V hold the poison."""
    B, V = x.shape
    buf = torch.full((B, ld), POISON, dtype=F32, device=DEV)
    buf[:, :V] = torch.from_numpy(np.ascontiguousarray(x))
    return buf


def _back(buf, V):
    got = buf.cpu().numpy()
    assert (got[:, V:] == POISON).all(), "columns >= V were written"
    return got[:, :V]


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32), equal_nan=True)


@pytest.fixture(scope="module")
def bands(golden):
    g = golden("decode_options.npz")
    return {k[5:]: float(g[k]) for k in g.files if k.startswith("band_")}


# ============================================================================ (a) sequence bias / bad words
L_PROMPT, MAX_NEW = 40, 8
STEPS = (0, 1, MAX_NEW - 1)


def _bias_case(B, V, seed):
    """Rows 0, 2, 4 share row 0's ids, the others are random.  For every tested step t the entries hold a 2-token, a 4-token (its
    prefix straddles the prompt / generated boundary at t = 1) and a maximum-length sequence cut from row 0's context at that step."""
    from tiny_audio_amd import ops
    rng = np.random.RandomState(seed)
    x = (3.0 * rng.standard_normal((B, V))).astype(np.float32)
    x[:, 311] = -np.inf
    prompt = rng.randint(400, 1003, size=(B, L_PROMPT)).astype(np.int64)
    gen = rng.randint(400, 1003, size=(B, MAX_NEW)).astype(np.int64)
    prompt[2::2], gen[2::2] = prompt[0], gen[0]
    row0 = np.concatenate([prompt[0], gen[0]])
    entries = [((305,), 0.75)]
    for t in STEPS:
        n = L_PROMPT + t
        entries += [((int(row0[n - 1]), 200 + t), 1.5 + t), (tuple(int(v) for v in row0[n - 3:n]) + (210 + t,), -2.25),
                    (tuple(int(v) for v in row0[n - (ops.SEQ_BIAS_MAX_LEN - 1):n]) + (220 + t,), 4.0)]
    entries += [((300,), 1e8), ((int(row0[L_PROMPT]), 300), -1e8 + 1), ((int(row0[L_PROMPT - 1]), int(row0[L_PROMPT]), 300), 1.0),   # fire at t = 1
                ((int(row0[L_PROMPT]), 301), 1e8), ((int(row0[L_PROMPT - 1]), int(row0[L_PROMPT]), 301), -1e8 + 1),               # the issue's pair
                ((310,), float("-inf")), ((int(row0[L_PROMPT - 1]), 312), float("-inf")),           # -inf onto finite scores
                ((311,), 2.0),                                                                      # a finite bias onto -inf
                ((V - 1,), 0.5), ((int(row0[L_PROMPT - 1]), V - 1), 0.25)]                          # the last valid column
    assert max(len(k) for k, _ in entries) == ops.SEQ_BIAS_MAX_LEN
    return x, prompt, gen, entries


def _run_bias(x, ld, prompt, gen, entries, L, t):
    from tiny_audio_amd import ops
    _lib, L_, ptr, st = _bits()
    B, V = x.shape
    buf = _device_rows(x, ld)
    tab = ops.build_sequence_table(entries, V, DEV)
    p, g = torch.from_numpy(prompt).to(DEV), torch.from_numpy(gen).to(DEV)
    step = torch.tensor([t], dtype=torch.int32, device=DEV)
    _lib.check(L_.ta_logits_sequence_bias(ptr(buf), ld, V, ptr(p), L, ptr(g), gen.shape[1], ptr(step), B, ptr(tab["tokens"]), ptr(tab["offsets"]),
                                          ptr(tab["bias"]), ptr(tab["groups"]), tab["n_seq"], tab["n_groups"], tab["n_tokens"], st),
               "ta_logits_sequence_bias")
    return _back(buf, V)


@pytest.mark.parametrize("B", [1, 5])
def test_sequence_bias_is_bit_identical(B):
    V, ld = SHAPES[0]
    x, prompt, gen, entries = _bias_case(B, V, 7 + B)
    fired = set()
    for L in (L_PROMPT, 0):
        for t in STEPS:
            ctx = np.concatenate([prompt[:, :L], gen[:, :t]], axis=1)
            ref = R.sequence_bias(x, ctx, entries)
            got = _run_bias(x, ld, prompt[:, L_PROMPT - L:] if L else prompt, gen, entries, L, t)
            assert _same(got, ref), (L, t, np.argwhere(got != ref)[:5].tolist())
            fired |= {(L, t, int(c)) for c in np.nonzero(ref[0] != x[0])[0]}
    # the cases exist on the reference side: every kind fired where it should and nowhere else
    for t in STEPS:
        assert (L_PROMPT, t, 200 + t) in fired and (L_PROMPT, t, 210 + t) in fired and (L_PROMPT, t, 220 + t) in fired
    assert (0, 0, 200) not in fired and (0, 1, 211) not in fired and (0, MAX_NEW - 1, 210 + MAX_NEW - 1) in fired
    assert (0, MAX_NEW - 1, 220 + MAX_NEW - 1) not in fired                        # longer than the context: skipped
    ref1 = R.sequence_bias(x, np.concatenate([prompt, gen[:, :1]], axis=1), entries)
    assert ref1[0, 300] == np.float32(x[0, 300] + np.float32(1.0)) and np.isneginf(ref1[:, 310]).all() and np.isneginf(ref1[:, 311]).all()


def test_sequence_bias_and_bad_words_at_the_true_vocabulary():
    from tiny_audio_amd import ops
    V, ld = SHAPES[1]
    x, prompt, gen, entries = _bias_case(2, V, 3)
    for t in (1, MAX_NEW - 1):
        ctx = np.concatenate([prompt, gen[:, :t]], axis=1)
        assert _same(_run_bias(x, ld, prompt, gen, entries, L_PROMPT, t), R.sequence_bias(x, ctx, entries)), t
    words = [list(k) for k, _ in entries]
    bad = ops.normalize_bad_words(words, eos_ids=(305,))
    ctx = np.concatenate([prompt, gen[:, :1]], axis=1)
    ref = R.bad_words(x, ctx, words, eos_ids=(305,))
    assert _same(_run_bias(x, ld, prompt, gen, bad, L_PROMPT, 1), ref) and np.isfinite(ref[:, 305]).all() and np.isneginf(ref[:, 300]).all()


def test_sequence_bias_limits_are_checked_by_the_library():
    from tiny_audio_amd import ops
    _lib, L_, ptr, st = _bits()
    buf = _device_rows(np.zeros((1, 1003), np.float32), 1024)
    z = torch.zeros(8, dtype=torch.int64, device=DEV)
    zi = torch.zeros(8, dtype=torch.int32, device=DEV)
    args = lambda n_seq, n_groups, n_tok: (ptr(buf), 1024, 1003, ptr(z), 4, ptr(z), 4, ptr(zi), 1, ptr(z), ptr(zi), ptr(buf), ptr(zi),  # noqa: E731
                                           n_seq, n_groups, n_tok, st)
    assert L_.ta_logits_sequence_bias(*args(ops.SEQ_BIAS_MAX_SEQS + 1, 1, ops.SEQ_BIAS_MAX_SEQS + 1)) == 1
    assert L_.ta_logits_sequence_bias(*args(2, 1, 2 * ops.SEQ_BIAS_MAX_LEN + 1)) == 1
    assert L_.ta_logits_sequence_bias(*args(2, 3, 2)) == 1
    assert L_.ta_logits_sequence_bias(*args(0, 0, 0)) == 0                                    # nothing to do
    torch.cuda.synchronize()


# ============================================================================ (b) step rules
def _run_rules(x, ld, t, max_new, forced=None, eos=None, decay=None, sup=None, bsup=None):
    from tiny_audio_amd import ops
    _lib, L_, ptr, st = _bits()
    B, V = x.shape
    buf = _device_rows(x, ld)
    ten = lambda v: None if not v else torch.tensor(list(v), dtype=torch.int64, device=DEV)  # noqa: E731
    n = lambda v: 0 if not v else len(v)  # noqa: E731
    f_, e_, s_, b_ = ten(forced), ten(eos), ten(sup), ten(bsup)
    start, mult = 0, None
    if decay is not None and eos:
        start, mult = ops.decay_multipliers(decay, max_new)
        mult = mult.to(DEV)
    step = torch.tensor([t], dtype=torch.int32, device=DEV)
    _lib.check(L_.ta_logits_step_rules(ptr(buf), ld, V, B, ptr(step), max_new, ptr(f_), n(forced), ptr(e_), n(eos) if mult is not None else 0,
                                       start, ptr(mult), ptr(s_), n(sup), ptr(b_), n(bsup), st), "ta_logits_step_rules")
    return _back(buf, V)


RULES = dict(forced=(7, 12), eos=(7, 11, 7, 1002), decay=(0, 1.5), sup=(0, 1, 2, 500, 1002, 11), bsup=(4, 600, 1001))


@pytest.mark.parametrize("B", [1, 5])
def test_step_rules_are_bit_identical(B):
    V, ld = SHAPES[0]
    max_new = 6
    x = (3.0 * np.random.RandomState(20 + B).standard_normal((B, V))).astype(np.float32)
    x[:, 11] = -np.abs(x[:, 11])                                    # a negative eos score: the penalty is on |score|
    subsets = [RULES, dict(forced=RULES["forced"]), dict(eos=RULES["eos"], decay=RULES["decay"]), dict(sup=RULES["sup"]), dict(bsup=RULES["bsup"]),
               dict(eos=RULES["eos"], decay=(3, 1.1), bsup=RULES["bsup"]), dict(eos=RULES["eos"])]
    changed = set()
    for k, sub in enumerate(subsets):
        for t in (0, 1, max_new - 1):
            ref = R.step_rules(x, t, max_new, sub.get("forced"), sub.get("eos"), sub.get("decay"), sub.get("sup"), sub.get("bsup"))
            got = _run_rules(x, ld, t, max_new, **sub)
            assert _same(got, ref), (k, t, np.argwhere(got != ref)[:5].tolist())
            if not _same(ref, x):
                changed.add((k, t))
    assert {(1, 5), (2, 1), (2, 5), (3, 0), (3, 1), (4, 0), (5, 5)} <= changed and not {(1, 0), (2, 0), (4, 1), (5, 1), (6, 0), (6, 5)} & changed
    ref = R.step_rules(x, 1, max_new, None, RULES["eos"], RULES["decay"])
    assert ref[0, 7] == np.float32(x[0, 7] + np.float32(abs(x[0, 7]) * np.float32(0.5)))      # 1.5 ** 1 - 1, applied once to the repeated id


def test_step_rules_at_the_true_vocabulary():
    V, ld = SHAPES[1]
    max_new = 5
    x = (3.0 * np.random.RandomState(31).standard_normal((2, V))).astype(np.float32)
    rules = dict(forced=(151645, 151643), eos=(151645, 151643), decay=(1, 1.25), sup=(0, 151669, 75000), bsup=(151668, 3))
    for t in (0, 2, max_new - 1):
        ref = R.step_rules(x, t, max_new, rules["forced"], rules["eos"], rules["decay"], rules["sup"], rules["bsup"])
        assert _same(_run_rules(x, ld, t, max_new, **rules), ref), t


# ============================================================================ (c) warpers
WARPERS = (("min_p", dict(min_p_value=CASES.MIN_P)), ("typical_p", dict(typical_p=CASES.TYPICAL_P)), ("epsilon", dict(eps=CASES.EPSILON)),
           ("eta", dict(eta=CASES.ETA)),
           ("all", dict(min_p_value=CASES.MIN_P, typical_p=CASES.TYPICAL_P, eps=CASES.EPSILON, eta=CASES.ETA)))


def _run_warp(x, ld, min_p_value=None, typical_p=None, eps=None, eta=None):
    _lib, L_, ptr, st = _bits()
    B, V = x.shape
    buf = _device_rows(x, ld)
    _lib.check(L_.ta_logits_warp_ext(ptr(buf), ld, V, B, min_p_value or 0.0, 1.0 if typical_p is None else typical_p, eps or 0.0, eta or 0.0, st),
               "ta_logits_warp_ext")
    return _back(buf, V)


def _check_warp(x, ld, kw, bands, name):
    V = x.shape[1]
    ref, und = R.warp_ext(x, **kw, bands=bands)
    if len([v for v in kw.values() if v is not None]) > 1:
        # a chain: an element inside an earlier stage's band would change the later stages' distribution -- such inputs are unusable
        first, u1 = R.warp_ext(x, min_p_value=kw.get("min_p_value"), typical_p=kw.get("typical_p"), eps=kw.get("eps"), bands=bands)
        assert not u1.any(), "an element lies inside the band of a stage that is not the last: pick other inputs"
    got = _run_warp(x, ld, **kw)
    flips = R.check_warp(got, x, ref, und, V)
    removed = np.isneginf(got) & ~np.isneginf(x)
    assert removed.any(axis=1).all() and (~np.isneginf(got)).any(axis=1).all(), name
    if "typical_p" not in kw:                                       # (HF's typical warper may remove the maximum; the others never do)
        assert (got[np.arange(x.shape[0]), x.argmax(axis=1)] == x.max(axis=1)).all(), name
    else:
        p, logp = R._softmax64(x if name == "typical_p" else R.warp_ext(x, min_p_value=kw.get("min_p_value"))[0])
        s = np.abs(-logp - R._entropy64(p, logp))
        assert np.isfinite(got[np.arange(x.shape[0]), np.where(np.isfinite(s), s, np.inf).argmin(axis=1)]).all(), name
    return flips


@pytest.mark.parametrize("name, kw", WARPERS, ids=[w[0] for w in WARPERS])
def test_warpers_small_vocabulary(bands, name, kw):
    V, ld = SHAPES[0]
    for seed in CASES.WARP_SEEDS:
        x = R.warp_inputs(seed, V, 5)
        _check_warp(x, ld, kw, bands, name)
        _check_warp(x[:1], ld, kw, bands, name)                    # B = 1


@pytest.mark.parametrize("name, kw", WARPERS, ids=[w[0] for w in WARPERS])
def test_warpers_at_the_true_vocabulary(bands, name, kw):
    """V = 151 670: the typical-p bisection runs full-row passes first and narrows to the LDS candidate list."""
    V, ld = SHAPES[1]
    for seed in CASES.WARP_SEEDS:
        _check_warp(R.warp_inputs(seed, V, 2), ld, kw, bands, name)


def test_warpers_edge_rows(bands):
    V, ld = SHAPES[0]
    # all -inf but one; all -inf but two tied; everything -inf
    x = np.full((3, V), -np.inf, np.float32)
    x[0, 517], x[1, 3], x[1, 1002] = 1.5, -2.0, -2.0
    for name, kw in WARPERS:
        assert _same(_run_warp(x, ld, **kw), x), name
    # min_p = 1 keeps the maxima only; the off values leave the row alone
    y = R.warp_inputs(5, V, 2)
    y[1, 10] = y[1, 20] = y[1].max() + 0.5
    got = _run_warp(y, ld, min_p_value=1.0)
    assert _same(got, np.where(y >= y.max(axis=1, keepdims=True), y, -np.inf))
    assert _same(_run_warp(y, ld), y)
    # planted exact ties at the cut: rows of few distinct values, so every cut falls on a tied group.  The groups carry percents of the
    # mass and their boundaries stay 1e-4 of it away from the target, so no float32 rounding can move a cut across one: the float64 decisions are required exactly, and a tied group never splits
    q = (np.round(R.warp_inputs(6, V, 4) * 2.0) / 2.0).astype(np.float32)
    for name, kw in WARPERS[:4]:
        ref, und = R.warp_ext(q, **kw, bands=dict(bands, typical_s=0.0))      # (a tied group sits AT s_cut: the s band would hold it whole)
        if name == "typical_p":
            p, logp = R._softmax64(q)
            s = np.abs(-logp - R._entropy64(p, logp))
            for r in range(q.shape[0]):                              # the cumulative mass at every group boundary is far from the target
                o = np.argsort(s[r], kind="stable")
                cum, ends = np.cumsum(p[r, o]), np.nonzero(np.diff(s[r, o]) > 1e-9)[0]
                assert np.abs(cum[ends] / CASES.TYPICAL_P - 1.0).min() > 1e-4      # (f32 sums of ~1000 terms stray ~1e-6)
        else:
            assert not und.any()
        got = _run_warp(q, ld, **kw)
        assert _same(got, ref), name
        for r in range(q.shape[0]):
            for v in np.unique(q[r]):
                assert len(set(np.isneginf(got[r][q[r] == v]))) == 1, (name, r, float(v))


def test_warp_ext_argument_checks():
    _lib, L_, ptr, st = _bits()
    buf = _device_rows(np.zeros((1, 1003), np.float32), 1024)
    for a in ((1.5, 1.0, 0.0, 0.0), (-0.1, 1.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (0.0, 1.5, 0.0, 0.0), (0.0, 1.0, 1.0, 0.0), (0.0, 1.0, 0.0, 1.0),
              (0.0, 1.0, -0.5, 0.0)):
        assert L_.ta_logits_warp_ext(ptr(buf), 1024, 1003, 1, *a, st) == 1, a
    assert L_.ta_logits_warp_ext(ptr(buf), 1000, 1003, 1, 0.5, 1.0, 0.0, 0.0, st) == 1
    assert L_.ta_logits_step_rules(ptr(buf), 1024, 1003, 1, None, 4, None, 0, None, 0, 0, None, ptr(buf), 1, None, 0, st) == 1
    torch.cuda.synchronize()


def test_operators_on_the_device():
    from tiny_audio_amd import ops, torch_ops  # noqa: F401
    V, ld = SHAPES[0]
    x = CASES.scores()
    ctx = CASES.context()
    buf = _device_rows(x, ld)
    tab = ops.build_sequence_table(ops.normalize_sequence_bias(dict(CASES.SEQUENCE_BIAS)), V, DEV)
    torch.ops.ta355.logits_sequence_bias(buf, V, torch.from_numpy(ctx).to(DEV), tab["tokens"], tab["offsets"], tab["bias"], tab["groups"])
    ref = R.sequence_bias(x, ctx, CASES.SEQUENCE_BIAS)
    assert _same(_back(buf, V), ref)
    torch.ops.ta355.logits_step_rules(buf, V, 4, 8, list(CASES.FORCED), list(CASES.EOS), CASES.DECAY[0], CASES.DECAY[1], list(CASES.SUPPRESS),
                                      list(CASES.BEGIN_SUPPRESS))
    ref = R.step_rules(ref, 4, 8, CASES.FORCED, CASES.EOS, CASES.DECAY, CASES.SUPPRESS, CASES.BEGIN_SUPPRESS)
    assert _same(_back(buf, V), ref)
    buf2 = _device_rows(x[1:], ld)
    assert ops.logits_warp_ext(buf2, V, min_p=1.0) is buf2
    assert _same(_back(buf2, V), np.where(x[1:] >= x[1:].max(axis=1, keepdims=True), x[1:], -np.inf))


# ============================================================================ (d) end to end
class _Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(golden):
    from tests.test_gpu_parity import build_model
    g = golden("generate_small.npz")
    S = RC.SMALL
    E, D, H = S["enc"]["hidden"], S["lm"]["hidden"], S["proj_hidden"]
    wE, wL, wP = OW.init_encoder(S["enc"], 0), RC.gen_lm_weights(), OW.init_mlp_projector(E, D, H)
    c = _Ctx()
    c.m = build_model(S["enc"], S["lm"], H, wE, wL, wP, audio_token_id=S["audio_token_id"], pad_token_id=S["pad_id"], eos_token_id=S["eos_id"])
    c.g = g
    c.kw = dict(input_ids=torch.from_numpy(g["input_ids"]), input_features=torch.from_numpy(g["input_features"]),
                audio_attention_mask=torch.from_numpy(g["audio_attention_mask"]), attention_mask=torch.ones(g["input_ids"].shape, dtype=torch.int64))
    c.W = dict(encoder=wE, lm=wL, projector=wP)
    c.cfg = dict(enc=S["enc"], lm=S["lm"], projector_type="mlp", k=S["k"], audio_token_id=S["audio_token_id"])
    c.batch = dict(input_ids=g["input_ids"], input_features=g["input_features"])
    c.pad, c.eos_b, c.V = S["pad_id"], int(g["eos_b"]), S["lm"]["vocab"]
    c.N = 8
    c.plain = c.m.generate(**c.kw, max_new_tokens=c.N, eos_token_id=[]).cpu().numpy()
    c.logits = {}
    return c


def _oracle_last(ctx, tokens, t):
    """fp32 oracle logits [B, V] of step t on the prefix tokens[:, :t] (cached: the tests share prefixes)."""
    key = tokens[:, :t].tobytes()
    if key not in ctx.logits:
        x = OG.prompt_embeds(ctx.batch, ctx.W, ctx.cfg)
        embed = ctx.W["lm"]["model.embed_tokens.weight"]
        if t:
            x = np.concatenate([x, embed[tokens[:, :t]]], axis=1)
        logits, _ = OQ.lm_forward(x, np.ones(x.shape[:2], np.int64), ctx.W["lm"], ctx.cfg["lm"], keep_cache=False)
        ctx.logits[key] = logits[:, -1].astype(np.float32)
    return ctx.logits[key]


def _follow(ctx, tokens, max_new, eos_ids=(), see_prompt=True, tol=0.12, rows=None, **opt):
    """The prefix-following check of tests/test_gpu_parity.py with the new restatement on the oracle's logits: every decision of an
    unfinished clip is the processed fp32 argmax on the device's own prefix or within ``tol`` of it; finished clips emit pad."""
    B, n_new = tokens.shape
    unfinished = np.ones(B, bool)
    prompt = np.asarray(ctx.batch["input_ids"], np.int64)
    for t in range(n_new):
        assert unfinished.any(), "generation continued after every clip had finished"
        context = np.concatenate([prompt, tokens[:, :t]], axis=1) if see_prompt else tokens[:, :t]
        last = R.process(_oracle_last(ctx, tokens, t), context, t, max_new, ctx.V, eos_ids=tuple(eos_ids), **opt)
        for b in range(B):
            if not unfinished[b]:
                assert tokens[b, t] == ctx.pad
            elif rows is None or b in rows:
                assert np.isfinite(last[b, tokens[b, t]]) and last[b].max() - last[b, tokens[b, t]] < tol, \
                    (b, t, int(tokens[b, t]), int(last[b].argmax()))
        unfinished &= ~np.isin(tokens[:, t], list(eos_ids))


def _gen(ctx, max_new=None, eos=(), **opt):
    return ctx.m.generate(**ctx.kw, max_new_tokens=max_new or ctx.N, eos_token_id=list(eos), **opt).cpu().numpy()


def test_e2e_single_token_bad_word(ctx):
    """Fails on the parent, which ignores the argument."""
    t0 = int(ctx.plain[0, 0])
    out = _gen(ctx, bad_words_ids=[[t0]])
    assert t0 not in out[0] and not np.array_equal(out, ctx.plain)
    _follow(ctx, out, ctx.N, bad_words_ids=[[t0]])


def test_e2e_two_token_bad_word(ctx):
    row = ctx.plain[0]
    i = next(i for i in range(len(row) - 1) if row[i] != row[i + 1] and row[i] not in row[:i])
    a, b = int(row[i]), int(row[i + 1])
    out = _gen(ctx, bad_words_ids=[[a, b]])
    assert a in out[0]
    for k, r in enumerate(out):
        seq = [int(ctx.g["input_ids"][k, -1])] + [int(v) for v in r]
        assert (a, b) not in set(zip(seq[:-1], seq[1:]))
    assert not np.array_equal(out[0], ctx.plain[0])
    _follow(ctx, out, ctx.N, bad_words_ids=[[a, b]])


def test_e2e_sequence_bias(ctx):
    t = next(v for v in range(20, ctx.V) if v not in ctx.plain and v != ctx.pad)
    out = _gen(ctx, sequence_bias={(t,): 30.0})
    assert (out[:, 0] == t).all()
    _follow(ctx, out, ctx.N, sequence_bias_entries=[((t,), 30.0)])
    u = int(ctx.plain[0, 0])
    for form in ({(u, t): 30.0}, [[[u, t], 30.0]]):                 # both HF forms
        out = _gen(ctx, sequence_bias=form)
        assert out[0, 0] == u and out[0, 1] == t
        for r in out:
            for i in np.nonzero(r == t)[0]:
                assert i > 0 and r[i - 1] == u                     # fires only after its prefix
        _follow(ctx, out, ctx.N, sequence_bias_entries=[((u, t), 30.0)])


def test_e2e_suppress_begin_suppress_and_forced_eos(ctx):
    sup = sorted(set(int(v) for v in ctx.plain[0]))
    out = _gen(ctx, suppress_tokens=sup)
    assert not np.isin(out, sup).any()
    _follow(ctx, out, ctx.N, suppress_tokens=sup)
    # a token the plain run emits later but not first: suppressed at the first step only, the run must not change at all
    later = [int(v) for v in ctx.plain[:, 1:].ravel() if v not in ctx.plain[:, 0]]
    assert later
    out = _gen(ctx, begin_suppress_tokens=later[:1])
    assert np.array_equal(out, ctx.plain)
    first = [int(v) for v in ctx.plain[:, 0]]
    out = _gen(ctx, begin_suppress_tokens=first)
    assert not np.isin(out[:, 0], first).any()
    _follow(ctx, out, ctx.N, begin_suppress_tokens=first)
    forced = next(v for v in range(20, ctx.V) if v not in ctx.plain and v != ctx.pad)
    out = _gen(ctx, forced_eos_token_id=forced)
    assert (out[:, -1] == forced).all() and np.array_equal(out[:, :-1], ctx.plain[:, :-1]) and out.shape[1] == ctx.N
    _follow(ctx, out, ctx.N, forced_eos_ids=[forced])
    eos = [ctx.eos_b, ctx.pad]                                       # with eos ids: the last column of every unfinished row
    out = _gen(ctx, max_new=12, eos=eos, forced_eos_token_id=forced)
    done = np.isin(out, eos).any(axis=1)
    assert (out[~done, -1] == forced).all() and (out.shape[1] == 12 or done.all())


def test_e2e_exponential_decay_length_penalty(ctx):
    eos = [ctx.eos_b, ctx.pad]
    plain = _gen(ctx, max_new=12, eos=eos)
    out = _gen(ctx, max_new=12, eos=eos, exponential_decay_length_penalty=(2, 1.5))
    _follow(ctx, out, 12, eos_ids=eos, exponential_decay_length_penalty=(2, 1.5))
    length = lambda a: [int(np.nonzero(np.isin(r, eos))[0][0]) + 1 if np.isin(r, eos).any() else 13 for r in a]  # noqa: E731
    assert all(n <= p for n, p in zip(length(out), length(plain))), (length(out), length(plain))
    with pytest.raises(ValueError, match="NaN"):
        _gen(ctx, max_new=12, eos=eos, min_new_tokens=3, exponential_decay_length_penalty=(2, 1.5))


def _all_options(ctx):
    t0 = int(ctx.plain[0, 0])
    free = [v for v in range(20, ctx.V) if v not in ctx.plain and v != ctx.pad and v != ctx.eos_b]
    return dict(bad_words_ids=[[t0], [int(ctx.plain[0, 1]), int(ctx.plain[0, 2])]], sequence_bias={(free[0],): 1.5, (t0, free[1]): 2.0},
                suppress_tokens=free[2:6], begin_suppress_tokens=[int(ctx.plain[1, 0])], forced_eos_token_id=ctx.eos_b,
                exponential_decay_length_penalty=(3, 1.2), min_new_tokens=2, repetition_penalty=1.2, no_repeat_ngram_size=2)


def test_e2e_all_options_graph_and_eager_agree(ctx):
    """max_new_tokens = 8: steps 2.. replay the captured graph, whose launches read the step from device memory."""
    eos = [ctx.eos_b, ctx.pad]
    opt = _all_options(ctx)
    # greedy: also held to the oracle
    out = _gen(ctx, max_new=8, eos=eos, **opt)
    chk = dict(opt)
    chk["sequence_bias_entries"] = [(k, v) for k, v in chk.pop("sequence_bias").items()]
    chk["forced_eos_ids"] = [chk.pop("forced_eos_token_id")]
    _follow(ctx, out, 8, eos_ids=eos, **chk)
    assert (out[~np.isin(out[:, :-1], eos).any(axis=1), -1] == ctx.eos_b).all()
    # with the warpers on top
    samp = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.95, min_p=0.02, typical_p=0.95, epsilon_cutoff=3e-4, eta_cutoff=2e-3,
                renormalize_logits=True, seed=123)
    ctx.m.eval()
    res = {}
    for samp_kw in (dict(), samp):
        with torch.no_grad():
            args = ctx.m._prepare_generation(ctx.kw["input_ids"], ctx.kw["input_features"], ctx.kw["audio_attention_mask"],
                                             ctx.kw["attention_mask"], None, dict(max_new_tokens=8, eos_token_id=eos, **opt, **samp_kw))
        assert ("warp_ext" in args) == bool(samp_kw)
        for graph in (True, False):
            seq, sc = ctx.m.language_model.greedy_decode(**args, token_scores=True, top_logprobs=4, use_graph=graph)
            res[graph] = (seq.cpu().numpy(), {k: v.cpu().numpy() for k, v in sc.items()})
        assert np.array_equal(res[True][0], res[False][0])
        for k in res[True][1]:
            assert np.array_equal(res[True][1][k], res[False][1][k]), k
        if not samp_kw:
            assert np.array_equal(res[True][0], out)


def test_e2e_scores_are_of_the_processed_row(ctx):
    t0 = int(ctx.plain[0, 0])
    o = ctx.m.generate(**ctx.kw, max_new_tokens=ctx.N, eos_token_id=[], bad_words_ids=[[t0]], return_token_scores=True, top_logprobs=4)
    ids, lp, tl = o.top_token_ids.cpu().numpy(), o.token_logprobs.cpu().numpy(), o.top_logprobs.cpu().numpy()
    assert not (ids == t0).any() and np.isfinite(lp).all() and np.isfinite(tl).all()
    assert (ids[..., 0] == o.sequences.cpu().numpy()).all()
    plain = ctx.m.generate(**ctx.kw, max_new_tokens=ctx.N, eos_token_id=[], return_token_scores=True, top_logprobs=4)
    assert (plain.top_token_ids.cpu().numpy()[0, 0] == t0).any()


def test_e2e_streaming_context_is_the_generated_tokens_only(ctx):
    p, b = int(ctx.g["input_ids"][0, -1]), int(ctx.plain[0, 0])
    one = dict(input_features=ctx.kw["input_features"][:1], audio_attention_mask=ctx.kw["audio_attention_mask"][:1], input_ids=ctx.kw["input_ids"][:1])
    toks = list(ctx.m.generate_streaming(**one, return_token_ids=True, max_new_tokens=ctx.N, eos_token_id=[], bad_words_ids=[[p, b]]))
    assert toks[0] == b                                              # the prompt is not part of the streaming context: no match
    got = np.array(toks, np.int64)[None, :]
    one_batch = _Ctx()
    one_batch.__dict__.update(ctx.__dict__)
    one_batch.batch = dict(input_ids=ctx.g["input_ids"][:1], input_features=ctx.g["input_features"][:1])
    one_batch.logits = {}
    _follow(one_batch, got, ctx.N, see_prompt=False, bad_words_ids=[[p, b]])
    out = _gen(ctx, bad_words_ids=[[p, b]])
    assert out[0, 0] != b                                            # generate() hands the prompt ids over: it fires
    _follow(ctx, out, ctx.N, bad_words_ids=[[p, b]])
    # a bad word whose prefix is a generated token fires in the streaming mode too -- from the step at which the context is as long as
    # the word (HF skips a sequence longer than the context: [plain 0, plain 1] cannot fire at step 1, where the context holds one token)
    w1, w2 = [b, int(ctx.plain[0, 1])], [int(ctx.plain[0, 1]), int(ctx.plain[0, 2])]
    toks1 = list(ctx.m.generate_streaming(**one, return_token_ids=True, max_new_tokens=ctx.N, eos_token_id=[], bad_words_ids=[w1]))
    assert toks1[:2] == w1
    _follow(one_batch, np.array(toks1, np.int64)[None, :], ctx.N, see_prompt=False, bad_words_ids=[w1])
    toks2 = list(ctx.m.generate_streaming(**one, return_token_ids=True, max_new_tokens=ctx.N, eos_token_id=[], bad_words_ids=[w2]))
    assert toks2[:2] == [int(v) for v in ctx.plain[0, :2]] and toks2[2] != w2[1]
    _follow(one_batch, np.array(toks2, np.int64)[None, :], ctx.N, see_prompt=False, bad_words_ids=[w2])


def test_e2e_top_k_1_with_each_warper_is_greedy(ctx):
    for extra in (dict(min_p=0.3), dict(typical_p=0.5), dict(epsilon_cutoff=0.01), dict(eta_cutoff=0.01),
                  dict(min_p=0.3, typical_p=0.5, epsilon_cutoff=0.01, eta_cutoff=0.01)):
        out = _gen(ctx, do_sample=True, top_k=1, seed=5, **extra)
        assert np.array_equal(out, ctx.plain), extra
    assert np.array_equal(_gen(ctx, do_sample=True, min_p=1.0, seed=9), ctx.plain)
    # without do_sample HF builds no warper: neither do we
    assert np.array_equal(_gen(ctx, min_p=0.3, typical_p=0.5, epsilon_cutoff=0.01, eta_cutoff=0.01), ctx.plain)


def test_e2e_no_option_is_the_parents_path(ctx):
    a = _gen(ctx, max_new=12, eos=())
    assert np.array_equal(a[:, :ctx.N], ctx.plain) and (a[:, :3] == ctx.g["tokens_a"][:, :3]).all()
    off = _gen(ctx, max_new=12, bad_words_ids=None, sequence_bias=None, suppress_tokens=[], begin_suppress_tokens=None, forced_eos_token_id=None,
               exponential_decay_length_penalty=None, min_p=None, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, renormalize_logits=True)
    assert np.array_equal(off, a)
    with pytest.raises(NotImplementedError):
        ctx.m.generate(**ctx.kw, num_beams=4, bad_words_ids=[[5]])
