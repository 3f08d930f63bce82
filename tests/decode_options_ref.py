"""Reference for the decoding options (``ta_logits_sequence_bias``, ``ta_logits_step_rules``, ``ta_logits_warp_ext``).  TEST
INFRASTRUCTURE ONLY.

A numpy restatement of the rules of ``transformers/generation/logits_process.py`` (5.15) that ``oracle/generate.py`` does not know:

* bias, bad words and the step rules in float32, operation by operation as HF's torch code performs them, so that the results are
  bit-identical to HF's (tests/golden/decode_options.npz holds HF's own outputs);
* the four warpers in float64: every threshold is formed in float64, and each function returns the keep mask together with every
  element's relative distance from the threshold, so that a float32 implementation can be held to "agrees outside a band".

``process`` chains them in HF's order (TF:generation/utils.py _get_logits_processor) around the two existing rules of
``oracle.generate.apply_logits_processors``.
"""
import numpy as np

NEG = np.float32(-np.inf)


# ----------------------------------------------------------------------------- float32, bit for bit
def sequence_bias(scores, context, entries):
    """SequenceBiasLogitsProcessor.  scores f32 [B, V], context int [B, n], entries [(tuple of ids, bias)] in HF's (dict) order."""
    scores = np.asarray(scores, np.float32)
    context = np.asarray(context).reshape(scores.shape[0], -1)
    B, V = scores.shape
    n = context.shape[1]
    length_1 = np.zeros(V, np.float32)
    for ids, b in entries:
        if len(ids) == 1:
            length_1[ids[0]] = np.float32(b)
    bias = np.zeros((B, V), np.float32)
    with np.errstate(invalid="ignore"):
        bias += length_1
        for ids, b in entries:
            if len(ids) == 1 or len(ids) > n:
                continue
            pre = len(ids) - 1
            match = (context[:, n - pre:] == np.asarray(ids[:-1])[None, :]).all(axis=1)
            bias[:, ids[-1]] += np.where(match, np.float32(b), np.float32(0.0)).astype(np.float32)
        return (scores + bias).astype(np.float32)


def bad_words(scores, context, words, eos_ids=()):
    """NoBadWordsLogitsProcessor: ``[eos]``-only words dropped, the rest biased by -inf."""
    kept = [tuple(w) for w in words if all(list(w) != [int(e)] for e in eos_ids)]
    return sequence_bias(scores, context, [(w, float("-inf")) for w in dict.fromkeys(kept)])


def forced_eos(scores, t, max_new, ids):
    scores = np.asarray(scores, np.float32)
    if t != max_new - 1:
        return scores.copy()
    out = np.full_like(scores, NEG)
    out[:, list(ids)] = 0.0
    return out


def decay_multiplier(t, start, factor):
    """float32(factor ** (t - start) - 1): the Python scalar HF multiplies the f32 |score| with."""
    return np.float32(pow(float(factor), t - start) - 1)


def exponential_decay(scores, t, eos_ids, start, factor):
    scores = np.asarray(scores, np.float32)
    if not t > start:
        return scores.copy()
    eos = list(eos_ids)
    pen = np.zeros_like(scores)
    with np.errstate(invalid="ignore", over="ignore"):
        pen[:, eos] = (np.abs(scores[:, eos]) * decay_multiplier(t, start, factor)).astype(np.float32)
        return (scores + pen).astype(np.float32)


def suppress(scores, ids):
    out = np.asarray(scores, np.float32).copy()
    out[:, list(ids)] = NEG
    return out


def begin_suppress(scores, t, ids):
    return suppress(scores, ids) if t == 0 else np.asarray(scores, np.float32).copy()


def step_rules(scores, t, max_new, forced_eos_ids=None, eos_ids=None, exponential_decay_length_penalty=None, suppress_tokens=None,
               begin_suppress_tokens=None):
    """The four step-indexed rules in HF's order; t = tokens generated so far."""
    x = np.asarray(scores, np.float32).copy()
    if forced_eos_ids:
        x = forced_eos(x, t, max_new, forced_eos_ids)
    if exponential_decay_length_penalty is not None and eos_ids:
        x = exponential_decay(x, t, eos_ids, *exponential_decay_length_penalty)
    if suppress_tokens:
        x = suppress(x, suppress_tokens)
    if begin_suppress_tokens:
        x = begin_suppress(x, t, begin_suppress_tokens)
    return x


# ----------------------------------------------------------------------------- float64 warpers
def _softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = np.where(np.isneginf(x), 0.0, np.exp(x - m))
    z = e.sum(axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        logp = np.where(np.isneginf(x), -np.inf, x - m - np.log(z))
    return e / z, logp


def _entropy64(p, logp):
    return -np.where(p > 0, p * np.where(p > 0, logp, 0.0), 0.0).sum(axis=-1, keepdims=True)


def _threshold_warper(x, p, thr):
    """keep = p >= thr or the row maximum; dist = |p / thr - 1| (inf on entries that are -inf already)."""
    x = np.asarray(x)
    keep = (p >= thr) | (x >= x.max(axis=-1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        dist = np.where(np.isneginf(x), np.inf, np.abs(p / thr - 1.0))
    return keep & ~np.isneginf(x), dist


def min_p(x, value):
    p, _ = _softmax64(x)
    return _threshold_warper(x, p, value * p.max(axis=-1, keepdims=True))


def epsilon_cutoff(x, eps):
    p, _ = _softmax64(x)
    return _threshold_warper(x, p, np.full((p.shape[0], 1), float(eps)))


def eta_cutoff(x, eps):
    p, logp = _softmax64(x)
    H = _entropy64(p, logp)
    return _threshold_warper(x, p, np.minimum(float(eps), np.sqrt(float(eps)) * np.exp(-H)))


def typical(x, mass, band_s=0.0, band_mass=0.0):
    """TypicalLogitsWarper in float64 -> (keep, undecided).  keep: s_i <= s_cut (ties survive), s_cut the shifted score at which the
    cumulative probability in ascending s first reaches ``mass``.  undecided: the elements a float32 implementation may put on either
    side -- s_cut may be the shifted score at which the cumulative probability reaches anything within mass (1 +- band_mass), and an
    element within a relative band_s of that range of cuts is undecided (unless it is the cut element and stands there alone)."""
    x = np.asarray(x)
    p, logp = _softmax64(x)
    H = _entropy64(p, logp)
    with np.errstate(invalid="ignore"):
        s = np.where(np.isneginf(x), np.inf, np.abs(-logp - H))
    keep, undecided = np.zeros(x.shape, bool), np.zeros(x.shape, bool)
    for r in range(x.shape[0]):
        order = np.argsort(s[r], kind="stable")
        cum = np.cumsum(p[r, order])
        ss = s[r, order]
        cut = lambda m: ss[min(int((cum < m).sum()), x.shape[1] - 1)]  # noqa: E731
        s_cut, s_lo, s_hi = cut(mass), cut(mass * (1.0 - band_mass)), cut(mass * (1.0 + band_mass))
        keep[r] = s[r] <= s_cut
        undecided[r] = (s[r] >= s_lo * (1.0 - band_s)) & (s[r] <= s_hi * (1.0 + band_s)) & np.isfinite(s[r])
        if s_lo == s_hi and undecided[r].sum() == 1:
            # the cut element alone: nothing is near enough to change places with it and the cumulative probability passes the whole
            # mass band on it -- it is decided (kept)
            undecided[r] = False
    return keep & ~np.isneginf(x), undecided


def typical_distances(x, mass):
    """For the band measurement: per element (|s_i / s_cut - 1|, |cum_i / mass - 1|) with cum_i the nearer of the cumulative
    probabilities just before and just after the element in ascending s."""
    x = np.asarray(x)
    p, logp = _softmax64(x)
    H = _entropy64(p, logp)
    with np.errstate(invalid="ignore"):
        s = np.where(np.isneginf(x), np.inf, np.abs(-logp - H))
    ds, dm = np.full(x.shape, np.inf), np.full(x.shape, np.inf)
    for r in range(x.shape[0]):
        order = np.argsort(s[r], kind="stable")
        cum = np.cumsum(p[r, order])
        s_cut = s[r, order][min(int((cum < mass).sum()), x.shape[1] - 1)]
        with np.errstate(divide="ignore", invalid="ignore"):
            ds[r] = np.abs(s[r] / s_cut - 1.0)
        dm[r, order] = np.minimum(np.abs(cum / mass - 1.0), np.abs((cum - p[r, order]) / mass - 1.0))
    return ds, dm


def apply_keep(x, keep):
    return np.where(keep, np.asarray(x, np.float32), NEG).astype(np.float32)


def warp_ext(x, min_p_value=None, typical_p=None, eps=None, eta=None, bands=None):
    """The four warpers in HF's order on f32 rows -> (out f32, undecided): ``undecided`` marks every element that lay inside a band at
    the stage that decided it (bands: dict(min_p=, epsilon=, eta=, typical_s=, typical_mass=); None = zero bands)."""
    bands = bands or {}
    x = np.asarray(x, np.float32).copy()
    und = np.zeros(x.shape, bool)
    if min_p_value:
        k, d = min_p(x, min_p_value)
        und |= d <= bands.get("min_p", 0.0)
        x = apply_keep(x, k)
    if typical_p is not None and typical_p < 1.0:
        k, u = typical(x, typical_p, bands.get("typical_s", 0.0), bands.get("typical_mass", 0.0))
        und |= u
        x = apply_keep(x, k)
    if eps:
        k, d = epsilon_cutoff(x, eps)
        und |= d <= bands.get("epsilon", 0.0)
        x = apply_keep(x, k)
    if eta:
        k, d = eta_cutoff(x, eta)
        und |= d <= bands.get("eta", 0.0)
        x = apply_keep(x, k)
    return x, und


def check_warp(got, x, ref, undecided, V, cap=None):
    """The issue's warper gate.  got / x / ref f32 [B, >= V]: every element outside the band agrees with the float64 decision, every
    survivor keeps its value, nothing is NaN; at most max(2, V / 2000) undecided elements per row (a property of the INPUTS)."""
    got, x, ref = np.asarray(got)[:, :V], np.asarray(x)[:, :V], np.asarray(ref)[:, :V]
    cap = max(2, V // 2000) if cap is None else cap
    n_und = undecided.sum(axis=1)
    assert (n_und <= cap).all(), f"the inputs put {n_und.tolist()} elements inside the band (cap {cap}): pick other inputs"
    assert not np.isnan(got).any()
    removed_got, removed_ref = np.isneginf(got), np.isneginf(ref)
    wrong = (removed_got != removed_ref) & ~undecided
    assert not wrong.any(), f"{int(wrong.sum())} decisions outside the band differ, first at {np.argwhere(wrong)[:4].tolist()}"
    surv = ~removed_got
    assert np.array_equal(got[surv], x[surv]), "a survivor's value changed"
    return int((removed_got != removed_ref).sum())


# ----------------------------------------------------------------------------- HF's order
def process(scores, context, t, max_new, V, *, sequence_bias_entries=None, repetition_penalty=1.0, no_repeat_ngram_size=0,
            bad_words_ids=None, min_new_tokens=0, eos_ids=(), forced_eos_ids=None, exponential_decay_length_penalty=None,
            suppress_tokens=None, begin_suppress_tokens=None):
    """Every processor (no warper) on one step's scores f32 [B, >= V] in HF's order; context int [B, n] = the ids HF's processors see;
    t = tokens generated so far.  -> f32 [B, V]."""
    from oracle import generate as OG
    x = np.asarray(scores, np.float32)[:, :V].copy()
    context = np.asarray(context).reshape(x.shape[0], -1)
    if sequence_bias_entries:
        x = sequence_bias(x, context, sequence_bias_entries)
    if repetition_penalty != 1.0 or no_repeat_ngram_size > 0:
        x = np.asarray(OG.apply_logits_processors(x, context, repetition_penalty, no_repeat_ngram_size), np.float32)
    if bad_words_ids:
        x = bad_words(x, context, bad_words_ids, eos_ids)
    if min_new_tokens > 0 and len(eos_ids) and t < min_new_tokens:
        x[:, list(eos_ids)] = NEG
    return step_rules(x, t, max_new, forced_eos_ids, list(eos_ids), exponential_decay_length_penalty, suppress_tokens,
                      begin_suppress_tokens)


# ----------------------------------------------------------------------------- the cases shared by the fixture generator and the tests
def warp_inputs(seed, V, B):
    """The warper tests' rows: 3 * randn, float32 [B, V]."""
    return (3.0 * np.random.RandomState(seed).standard_normal((B, V))).astype(np.float32)


class CASES:
    V, L, N_CTX = 1003, 20, 24                      # the context: 20 prompt ids followed by 4 generated tokens
    EOS, FORCED, DECAY = (7, 11), (7,), (2, 1.5)
    SUPPRESS, BEGIN_SUPPRESS = (1, 2, 3, 500, 1002), (4, 600)
    MIN_P, TYPICAL_P, EPSILON, ETA = 0.05, 0.9, 3e-4, 2e-3
    WARP_SHAPES, WARP_SEEDS = ((1003, 5), (151670, 2)), (100, 101, 102, 103)
    # positions 19 .. 23 of the three rows (19 is the prompt's last token)
    TAILS = ((30, 31, 32, 40, 41), (30, 31, 32, 41, 40), (33, 31, 32, 40, 41))
    SEQUENCE_BIAS = (
        ((50,), 2.5), ((40, 41, 50), 3.0), ((41, 50), -1.5),                     # three entries add up on token 50 (rows 0, 2)
        ((60,), 1e8), ((41, 60), -1e8 + 1), ((40, 41, 60), 1.0),                 # (1e8 - 1e8) + 1 = 1 in f32; any other order gives 0
        ((31, 32, 40, 41, 70), 4.0),                                             # a prefix of 4: rows 0 and 2
        ((30, 31, 32, 40, 41, 71), 5.0),                                         # straddles the prompt / generated boundary: row 0 only
        (tuple(range(100, 125)) + (72,), 6.0),                                   # 26 tokens > the context: skipped
        ((80,), float("-inf")), ((41, 81), float("-inf")),                       # -inf onto finite scores
        ((90,), 2.0),                                                            # a finite bias onto the planted -inf score [0, 90]
    )
    SEQUENCE_BIAS_LIST_FORM = (((50,), 2.5), ((40, 41, 50), 3.0), ((41, 50), -1.5), ((80,), float("-inf")))
    BAD_WORDS = ((7,), (85,), (40, 41, 86), (41, 40, 87), (99, 88), (85,))      # [eos] is dropped, (85,) counts once, (99, 88) never fires
    CHAIN_POINTS = (("t0", 0, 8), ("t4", 4, 8), ("t4_last", 4, 5))               # (tag, tokens generated so far, max_new_tokens)

    @staticmethod
    def scores():
        x = (3.0 * np.random.RandomState(2024).standard_normal((3, CASES.V))).astype(np.float32)
        x[0, 90] = -np.inf
        return x

    @staticmethod
    def context():
        c = np.random.RandomState(2025).randint(120, CASES.V, size=(3, CASES.N_CTX)).astype(np.int64)
        c[:, 5], c[:, 12] = c[:, 2], c[:, 3]                                      # repeats, for the repetition penalty
        c[:, 8:10] = c[:, 15:17]                                                   # a repeated bigram ...
        for b, tail in enumerate(CASES.TAILS):
            c[b, 19:24] = tail
        c[:, 16] = 41                                                              # ... and an earlier 41, for the n-gram rule
        return c

    @staticmethod
    def chain_generation_kwargs(max_new):
        """GenerationConfig keywords with every processor option set (``max_length`` = L + max_new is the caller's)."""
        return dict(sequence_bias=CASES.SEQUENCE_BIAS, repetition_penalty=1.3, no_repeat_ngram_size=2,
                    bad_words_ids=[list(w) for w in CASES.BAD_WORDS], min_new_tokens=2, forced_eos_token_id=CASES.FORCED[0],
                    exponential_decay_length_penalty=CASES.DECAY, suppress_tokens=list(CASES.SUPPRESS),
                    begin_suppress_tokens=list(CASES.BEGIN_SUPPRESS), eos_token_id=list(CASES.EOS), pad_token_id=0)
