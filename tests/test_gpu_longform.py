"""-m gpu: long-form segmentation (csrc/segment.hip) and ``ASRModel.transcribe_long`` end to end.

Gates.  Cost: |device - float64| <= gamma_K * float64 per position, K = TA_CUT_COST_K(h) as the kernel states it (its longest chain
of additions + 3), gamma_K = K u / (1 - K u), u = 2^-24; zeros cost exactly 0; two runs give the same bits.  Plan: cuts, n_seg, dp[T]
and every back[] entry equal tests/segment_ref.py's float32 restatement on the device's own cost array, bit for bit.  Gather: an
exact copy and exact zeros.  End to end on the generate_small.npz model: the windows tile the recording within the bounds, every cut
lies in a silence, and every window's tokens are those of ``model.generate`` on host-sliced copies of the same windows in the same
groups with the same prompts.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import segment_ref as R

DEV = "cuda"
F32 = torch.float32


def _upload(waves):
    from tiny_audio_amd import longform
    return longform.upload(waves)


def _cost(waves, h=10, cp=0.05):
    flat, off, lens = _upload(waves)
    cost = torch.ops.ta355.wave_cut_cost(flat, off, max(lens), h, cp)
    return cost, off, lens


def _check_cost(waves, h=10, cp=0.05):
    cost, _, lens = _cost(waves, h, cp)
    got = cost.cpu().numpy()
    g = R.gamma(R.cost_K(h))
    assert got.shape == (len(waves), R.positions(max(lens)) + 1)
    worst = 0.0
    for r, x in enumerate(waves):
        T = R.positions(len(x))
        ref = R.cut_cost(x, h, cp)
        err = np.abs(got[r, :T + 1].astype(np.float64) - ref)
        worst = max(worst, float((err / np.maximum(ref, 1e-300)).max()))
        assert (err <= g * ref).all(), (r, len(x), int(np.argmax(err - g * ref)))
        assert np.isnan(got[r, T + 1:]).all(), "positions beyond T were written"
    print(f"cut cost: worst relative error {worst:.3g} against gamma_K {g:.3g} (K = {R.cost_K(h)})")
    return got


# ============================================================================ (a) the cost
@pytest.mark.parametrize("n", [1, 159, 160, 161, 400, 48017])
def test_cost_against_float64(n):
    rng = np.random.RandomState(n)
    x = (rng.standard_normal(n) * np.exp(rng.uniform(-6, 0, n))).astype(np.float32)
    _check_cost([x])
    _check_cost([x], h=0, cp=0.0)
    _check_cost([x], h=3, cp=1.5)


def test_cost_of_zeros_impulses_ragged_batch_and_bits():
    rng = np.random.RandomState(0)
    z = np.zeros(4000, np.float32)
    assert (_check_cost([z])[0] == 0.0).all(), "a recording of zeros must cost exactly 0"
    first, last = z.copy(), z.copy()
    first[0], last[-1] = 3.0, -2.0
    g0 = _check_cost([first], h=2)[0]
    assert g0[0] >= g0[3] > g0[4] > 0 and (g0[4:] == g0[4]).all()                 # sample 0 is in pw[0] and pw[1]: h = 2 carries it to 0 .. 3
    g1 = _check_cost([last], h=2)[0]
    assert g1[25] >= g1[22] > g1[21] > 0 and (g1[:22] == g1[0]).all()              # T = 25: sample n - 1 is in pw[24] and pw[25]: 22 .. 25
    # three ragged recordings in one call: the second and third start off a 16-byte boundary
    waves = [rng.standard_normal(n).astype(np.float32) for n in (161, 48017, 400)]
    got = _check_cost(waves)
    for r, x in enumerate(waves):                                                  # the same bits as the recording alone (aligned start)
        alone = _cost([x])[0].cpu().numpy()[0]
        T = R.positions(len(x))
        assert np.array_equal(got[r, :T + 1], alone[:T + 1]), r
    again = _cost(waves)[0].cpu().numpy()
    assert np.array_equal(got, again, equal_nan=True), "two runs must give the same bits"


# ============================================================================ (b) the plan
def _offsets(Ts):
    off = np.zeros(len(Ts) + 1, np.int64)
    off[1:] = np.cumsum([160 * T - 3 if T > 1 else 157 for T in Ts])              # ceil(n / 160) = T
    return torch.from_numpy(off).to(DEV), int(np.diff(off).max())


def _check_plan(cost_rows, Ts, min_len, max_len):
    """cost_rows: device f32 [R, >= max T + 1]; every output of the kernel against the restatement on those very costs."""
    off, max_n = _offsets(Ts)
    cuts, n_seg, dp_T, back = torch.ops.ta355.cut_plan(cost_rows, off, max_n, min_len, max_len)
    host = cost_rows.cpu().numpy()
    cuts, n_seg, dp_T, back = cuts.cpu().numpy(), n_seg.cpu().numpy(), dp_T.cpu().numpy(), back.cpu().numpy()
    out = []
    for r, T in enumerate(Ts):
        rc, rn, rdp, rback, _ = R.cut_plan(host[r], T, min_len, max_len)
        assert n_seg[r] == rn, (T, n_seg[r], rn)
        assert cuts[r, :rn + 1].tolist() == rc, (T, cuts[r, :rn + 1].tolist(), rc)
        assert (cuts[r, rn + 1:] == -1).all()
        assert np.float32(dp_T[r]).tobytes() == np.float32(rdp).tobytes(), (T, dp_T[r], rdp)
        assert np.array_equal(back[r, :T + 1], rback), (T, np.flatnonzero(back[r, :T + 1] != rback)[:5])
        out.append(rc)
    return out


def _device_costs(Ts, seed):
    """The cost kernel's own output for random bursts: rows of one [R, max T + 1] tensor."""
    rng = np.random.RandomState(seed)
    waves = []
    for T in Ts:
        n = 160 * T - 3 if T > 1 else 157
        env = np.repeat(np.exp(rng.uniform(-5, 0, n // 800 + 1)), 800)[:n]
        waves.append((rng.standard_normal(n) * env).astype(np.float32))
    return _cost(waves)[0]


@pytest.mark.parametrize("min_len,max_len", [(4, 8), (3, 7)])
def test_plan_small_grids_bit_for_bit(min_len, max_len):
    """(4, 8): T below, at and just past the bounds and 1000; (3, 7): a block of min_len positions straddles the window's chunks.
    R = 8 recordings of different T in one launch, then each alone."""
    Ts = [1, 3, 4, 8, 9, 16, 17, 1000]
    cost = _device_costs(Ts, 11)
    together = _check_plan(cost, Ts, min_len, max_len)
    for r, T in enumerate(Ts):
        assert _check_plan(cost[r:r + 1, :T + 1].contiguous(), [T], min_len, max_len)[0] == together[r]
    assert together[0] == [0, 1] and together[1] == [0, 3]                        # T < min_len: the single window


@pytest.mark.parametrize("min_len,max_len,T", [(4, 8, 1000), (3, 7, 200), (64, 200, 3000), (50, 200, 777)])
def test_plan_constant_cost_follows_the_tie_rule(min_len, max_len, T):
    cost = torch.full((1, T + 1), 0.25, device=DEV, dtype=F32)
    cuts = _check_plan(cost, [T], min_len, max_len)[0]
    assert len(cuts) - 1 == -(-T // max_len)                                       # the fewest cuts; which ones is the tie rule's choice


def test_plan_cuts_at_the_one_deep_pause():
    T = 900
    host = np.full((1, T + 1), 1.0, np.float32)
    host[0, 437] = 1.0 / 1024
    cuts = _check_plan(torch.from_numpy(host).to(DEV), [T], 100, 600)[0]
    assert cuts == [0, 437, 900]


def test_plan_production_bounds_and_three_recordings():
    """min_len = 500, max_len = 2800, T = 20 000 on the device's own costs (a ring of 3328 positions that wraps six times, 52 chunk minima in flight),
    with two shorter recordings in the same launch."""
    Ts = [20000, 2801, 499]
    cost = _device_costs(Ts, 3)
    cuts = _check_plan(cost, Ts, 500, 2800)
    assert all(500 <= b - a <= 2800 for a, b in zip(cuts[0][:-1], cuts[0][1:])) and cuts[2] == [0, 499]


def test_non_finite_samples_on_the_device_are_refused():
    """Host arrays are checked before the upload; a device tensor is caught on the plan's read-back: the mean-power term carries one
    bad sample into every cost.  A recording that is cut, and one too short to be cut."""
    from tiny_audio_amd import longform
    for n in (48017, 300):
        for bad in (float("nan"), float("inf")):
            x = torch.zeros(n, device=DEV)
            x[n // 3] = bad
            with pytest.raises(ValueError, match="recording 1 holds non-finite"):
                longform.plan_windows([torch.ones(5000, device=DEV), x], max_window_s=2.0, min_window_s=0.5)


# ============================================================================ (c) the gather
@pytest.mark.parametrize("Ls", [4096, 1000, 1027])
def test_gather_is_an_exact_copy_with_exact_zeros(Ls):
    """Ls a multiple of 4 (16-byte stores) and not (4-byte stores); starts at every residue mod 4; len = 1, len = Ls, a window ending at
    the buffer's last sample, len = 0."""
    from tiny_audio_amd import ops
    rng = np.random.RandomState(Ls)
    total = 3 * Ls + 11
    flat = rng.standard_normal(total).astype(np.float32)
    start = [0, 1, 2, 3, 4, Ls + 5, total - Ls, total - 1, 7, 2 * Ls]
    length = [Ls, Ls, 777, 1, Ls - 1, Ls, Ls, 1, 0, 5]
    out = torch.full((len(start), Ls), float("nan"), device=DEV, dtype=F32)
    got, lens = ops.wave_windows(torch.from_numpy(flat).to(DEV), torch.tensor(start, dtype=torch.int64, device=DEV),
                                 torch.tensor(length, dtype=torch.int32, device=DEV), Ls, out=out)
    ref, rlens = R.gather(flat, start, length, Ls)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert lens.cpu().tolist() == rlens.tolist()


def test_operators_pass_opcheck():
    x = torch.randn(5000, device=DEV)
    off = torch.tensor([0, 1700, 5000], device=DEV)
    utils = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.ta355.wave_cut_cost, (x, off, 3300, 10, 0.05), test_utils=utils)
    cost = torch.ops.ta355.wave_cut_cost(x, off, 3300, 10, 0.05)
    torch.library.opcheck(torch.ops.ta355.cut_plan, (cost, off, 3300, 4, 8), test_utils=utils)
    torch.library.opcheck(torch.ops.ta355.wave_windows, (x, torch.tensor([3, 1700], device=DEV),
                                                        torch.tensor([100, 64], dtype=torch.int32, device=DEV), 128), test_utils=utils)


# ============================================================================ (d) end to end
LETTERS = "ETAONIHSRDLU"
BURSTS = ((0.0, 0.9), (1.2, 2.3), (2.6, 3.5), (3.9, 4.8), (5.1, 6.0))           # seconds; the gaps are the silences


class _Tok:
    """The generation fixture's prompt shape (tests/golden/recipe.py) with one placeholder per projected frame; two-letter words."""

    def __init__(self, audio_id):
        self.audio_id = audio_id

    def convert_tokens_to_ids(self, t):
        return self.audio_id

    def apply_chat_template(self, messages, tokenize=True, add_generation_prompt=False, **_):
        user = [m for m in messages if m["role"] == "user"][0]["content"]
        return torch.tensor([[5, 6, 7] + [self.audio_id] * user.count("<audio>") + [40, 41, 42, 43]])

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(LETTERS[i % 12] + LETTERS[(i // 12) % 12] for i in ids)


def _recording():
    rng = np.random.RandomState(6)
    x = np.zeros(96000, np.float32)
    for a, b in BURSTS:
        x[int(a * 16000):int(b * 16000)] = 0.3 * rng.standard_normal(int(b * 16000) - int(a * 16000))
    return x


@pytest.fixture(scope="module")
def model():
    from oracle import weights as OW
    from tests.golden import recipe as RC
    from tests.test_gpu_parity import build_model
    S = RC.SMALL
    wE, wL, wP = OW.init_encoder(S["enc"], 0), RC.gen_lm_weights(), OW.init_mlp_projector(S["enc"]["hidden"], S["lm"]["hidden"], S["proj_hidden"])
    m = build_model(S["enc"], S["lm"], S["proj_hidden"], wE, wL, wP, audio_token_id=S["audio_token_id"], pad_token_id=S["pad_id"],
                    eos_token_id=S["eos_id"])
    m.tokenizer = _Tok(S["audio_token_id"])
    m.system_prompt = None
    return m


def test_end_to_end_windows_tokens_text_and_words(model):
    from tiny_audio_amd import longform, wav2vec2 as W
    from tiny_audio_amd.alignment import ForcedAligner
    from tiny_audio_amd.asr_processing import ASRProcessor
    from tiny_audio_amd.eval_text import postprocess_tokens
    m, x = model, _recording()
    n = len(x)
    plan = longform.plan_windows([x], max_window_s=2.0, min_window_s=0.5)[0]
    starts, lengths = plan.starts, plan.lengths
    # the windows tile [0, n) within the bounds, and every interior cut lies inside a silence
    assert starts[0] == 0 and starts[-1] + lengths[-1] == n and all(s + l == s2 for s, l, s2 in zip(starts, lengths, starts[1:]))
    assert all(8000 <= l <= 32000 for l in lengths) and len(lengths) >= 3
    silences = [(int(b * 16000), int(a2 * 16000)) for (_, b), (a2, _) in zip(BURSTS, BURSTS[1:])]
    for c in starts[1:]:
        assert any(lo < c < hi for lo, hi in silences), (c, silences)
        assert not x[c - 160:c + 160].any()
    # four cuts, one per silence (three cannot keep every window within 2 s), each where the cost is the bare penalty term
    assert len(lengths) == 5 and len(plan.cut_costs) == 4 and len(set(plan.cut_costs)) == 1 and plan.cut_costs[0] > 0

    calls = []
    real_generate = m.generate

    def spy(**kw):
        out = real_generate(**kw)
        calls.append((kw, out))
        return out

    m.generate = spy
    am = W.Wav2Vec2CtcMI355X(W.Wav2Vec2CtcConfig(hidden_size=256, num_attention_heads=4, intermediate_size=512, conv_dim=128,
                                                 num_hidden_layers=1), device=DEV).random_init(0)
    try:
        res = m.transcribe_long(x, max_window_s=2.0, min_window_s=0.5, batch_size=3, max_new_tokens=6, return_timestamps=True,
                                acoustic_model=am)
    finally:
        del m.generate
    groups = longform.group_windows(lengths, 3)
    assert len(calls) == len(groups) >= 2
    proc = ASRProcessor(m.feature_extractor, m.tokenizer, m.projector, m.config.encoder_conv_layers)
    eos = [m.config.eos_token_id, m.config.pad_token_id]
    texts, words = {}, {}
    for group, (kw, out) in zip(groups, calls):
        slices = [x[starts[k]:starts[k] + lengths[k]].copy() for k in group]                    # host-sliced copies, the usual front door
        f = m.feature_extractor(slices, sampling_rate=16000)
        assert torch.equal(f["input_features"], kw["input_features"]) and torch.equal(f["attention_mask"], kw["audio_attention_mask"])
        counts = proc.audio_token_counts(f["attention_mask"]).tolist()
        prompts = [ASRProcessor.tokenize_messages(m.tokenizer, ASRProcessor.build_messages(c, None, None), True)[0] for c in counts]
        ids, att = longform.left_pad_prompts(prompts, m.config.pad_token_id)
        assert torch.equal(ids, kw["input_ids"].cpu()) and torch.equal(att, kw["attention_mask"].cpu())
        want = real_generate(input_ids=ids, input_features=f["input_features"], audio_attention_mask=f["attention_mask"],
                             attention_mask=att, max_new_tokens=6)
        assert torch.equal(want, out), (group, want.tolist(), out.tolist())
        for j, k in enumerate(group):
            texts[k] = postprocess_tokens(want[j].tolist(), eos, lambda t: m.tokenizer.decode(t))
        live = [j for j, k in enumerate(group) if texts[k]]
        got = ForcedAligner.align_audio_batch([slices[j] for j in live], [texts[group[j]] for j in live], am)
        for j, ws in zip(live, got):
            t0 = starts[group[j]] / 16000
            words[group[j]] = [{"word": w["word"], "start": w["start"] + t0, "end": w["end"] + t0} for w in ws]
    chunks = res["chunks"]
    assert [c["timestamp"] for c in chunks] == [(s / 16000, (s + l) / 16000) for s, l in zip(starts, lengths)]
    assert [c["text"] for c in chunks] == [texts[k] for k in range(len(starts))]
    assert any(texts.values()) and res["text"] == " ".join(texts[k] for k in range(len(starts)) if texts[k])
    assert res["words"] == [w for k in range(len(starts)) for w in words.get(k, [])]
    assert res["words"] and all(w["end"] <= n / 16000 + 0.1 for w in res["words"])
