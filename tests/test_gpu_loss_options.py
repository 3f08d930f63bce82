"""-m gpu: the LM loss options (label smoothing eps, z-loss zc; include/ta355.h ``ta_ce_options``) -- the cross-entropy launch against
the float64 reference of tests/loss_options_ref.py under the gates of tests/rowwise_ref.py (buffers and checks are those of
tests/test_gpu_rowwise_grid.py, imported), then through ASRModel.forward and ASRTrainer against transformers in fp32 on the CPU with
seeded random weights (tiny Qwen3: the SMALL configuration, the one tests/golden/qwen3_small.npz was made with -- the fixture itself is
not read; tiny SmolLM3: the same widths without q/k-norm, last layer NoPE; both as tests/test_gpu_packing.py builds them).

Every kernel check prints ``ROWGRID ta_cross_entropy_opt <case> <tensor> e/m=<ratio> worst=<row>``; the model tests print their figures
behind ``[lossopt]``.  The measured table is profiles/loss_options.md."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import loss_options_ref as LO
from tests import rowwise_ref as R
from tests.test_gpu_rowwise_grid import Checks, Guarded, call, ptr, stream

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from tiny_audio_amd import _lib

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EP = "ta_cross_entropy_opt"
SCALE = 0.37
FULL_WIDTH = (151670, 151680)


# ----------------------------------------------------------------------------- the kernel
def _rows(n, R_):
    rows = [(7 * i + 3) % R_ for i in range(n)]
    if n > 5:
        rows[5] = rows[2]                                                   # non-monotonic, one row twice
    return rows


@functools.lru_cache(maxsize=None)
def _inputs(V, ldl, n, kind, bf16, with_rows):
    """Logits, row list, targets of one case -- made once, shared by every option setting and ldd."""
    rows = _rows(n, n + 13) if with_rows else None
    z = R.ce_logits(n if rows is None else max(rows) + 1, V, ldl, kind, bf16)
    t = R.ce_targets(n, V, ldl)
    if kind == "dominant_target":
        t = [i % V for i in range(n)]
    elif kind == "dominant_other":
        t = [(i + 1) % V for i in range(n)]
    return z, rows, t


@functools.lru_cache(maxsize=None)
def _reference(V, ldl, n, kind, bf16, with_rows, eps, zc):
    """(exact, model) at the widest ldd of the grid; a narrower dlogits is its leading columns (those >= V are zero)."""
    z, rows, t = _inputs(V, ldl, n, kind, bf16, with_rows)
    return tuple(LO.cross_entropy_opt(z, rows, t, V, SCALE, ldl + 8, eps, zc, model=mo) for mo in (False, True))


def run_opt(ck, case, key, ldd, eps, zc):
    V, ldl, n = key[0], key[1], key[2]
    z, rows, t = _inputs(*key)
    e, m = _reference(*key, eps, zc)
    zd, td = z.to(DEV), torch.tensor(t, dtype=torch.int64, device=DEV)
    rd = None if rows is None else torch.tensor(rows, dtype=torch.int32, device=DEV)
    nll, obj, dl, loss = Guarded(n), Guarded(n), Guarded(n, ldd, BF16), Guarded(1, None, F32, torch.zeros(1))
    opt = _lib.CeOptions(eps=eps, zc=zc, obj=obj.full.data_ptr())
    call(EP, ptr(zd), int(z.dtype == BF16), ldl, ptr(rd), ptr(td), n, V, SCALE, nll.p, loss.p, dl.p, ldd, C.byref(opt), stream())
    nll0, loss0 = Guarded(n), Guarded(1, None, F32, torch.zeros(1))
    call("ta_cross_entropy", ptr(zd), int(z.dtype == BF16), ldl, ptr(rd), ptr(td), n, V, SCALE, nll0.p, loss0.p, None, ldd, stream())
    bad = ~e["valid"]
    got = nll.get()
    ck.rows(case, "nll", got, e["nll"], m["nll"], n)
    ck.equal(case, "nll of invalid targets", not got[bad].any())
    ck.equal(case, "nll is the options-off nll, bit for bit", torch.equal(got.view(torch.int32), nll0.get().view(torch.int32)))
    got = obj.get()
    ck.rows(case, "obj", got, e["obj"], m["obj"], n)
    ck.equal(case, "obj of invalid targets", not got[bad].any())
    mo_l = float(torch.tensor(0.0, dtype=F32) + m["loss"].float())
    ck.scalar(case, "loss", float(loss.get()[0]), float(e["loss"]), mo_l)
    got = dl.get()
    ck.rows(case, "dlogits", got, e["dlogits"][:, :ldd], m["dlogits"][:, :ldd], ldd, bf16=True)
    ck.equal(case, "dlogits of invalid targets", not got[bad].float().any())
    ck.equal(case, "dlogits columns >= V", not got[:, V:].float().any())
    del zd, td, rd


def _grid(V, ldl, n):
    ck = Checks(EP)
    for bf in (False, True):
        for with_rows in (False, True):
            key = (V, ldl, n, "normal3", bf, with_rows)
            for eps, zc in LO.OPTIONS:
                for ldd in (ldl, (V + 3) // 4 * 4, ldl + 8):
                    case = f"V{V}-ldl{ldl}-{'bf16' if bf else 'f32'}-{'rows' if with_rows else 'norows'}-ldd{ldd}-eps{eps}-zc{zc}"
                    run_opt(ck, case, key, ldd, eps, zc)
    torch.cuda.synchronize()
    ck.done()


@pytest.mark.parametrize("V,ldl", R.CASES["cross_entropy"]["V_ldl"])
def test_options_kernel_shapes(V, ldl):
    _grid(V, ldl, R.CASES["cross_entropy"]["n"])


def test_options_kernel_full_width_rows():
    """One row block of the production width: 148 strided float4 (593 logits) per lane in both passes, the V % 4 tail and the padding
    behind it."""
    _grid(*FULL_WIDTH, 5)


def test_options_kernel_values():
    """The value edges of the existing grid at V = 1003; shift-3000 is the row whose mean a plain f32 sum would lose."""
    V, ldl, n, ck = 1003, 1024, 37, Checks(EP)
    for kind in R.CASES["cross_entropy"]["values"]:
        for eps, zc in LO.OPTIONS:
            run_opt(ck, f"{kind}-eps{eps}-zc{zc}", (V, ldl, n, kind, kind == "bf16x5", False), ldl, eps, zc)
    torch.cuda.synchronize()
    ck.done()


def test_options_loss_bits_repeat():
    """The objective is summed from its per-row buffer in index order: the same loss bits on every call (4096 row blocks finish in
    whatever order; a float atomic per row would not repeat)."""
    n, V, ldl = 4096, 255, 256
    g = torch.Generator().manual_seed(3)
    z = (torch.randn(n, ldl, generator=g) * 3).to(DEV)
    t = torch.randint(0, V, (n,), generator=g).to(DEV)
    bits = []
    for _ in range(3):
        obj, loss, dl = Guarded(n), Guarded(1, None, F32, torch.zeros(1)), Guarded(n, ldl, BF16)
        opt = _lib.CeOptions(eps=0.1, zc=1e-4, obj=obj.full.data_ptr())
        call(EP, ptr(z), 0, ldl, None, ptr(t), n, V, 1.0 / n, None, loss.p, dl.p, ldl, C.byref(opt), stream())
        bits.append((int(loss.get().view(torch.int32)[0]), obj.get().clone(), dl.get().clone()))
    assert bits[0][0] == bits[1][0] == bits[2][0], [b[0] for b in bits]
    assert torch.equal(bits[0][1], bits[1][1]) and torch.equal(bits[0][2].view(torch.int16), bits[1][2].view(torch.int16))
    assert np.isfinite(np.float32(bits[0][1].sum())) and float(bits[0][1].min()) > 0


def test_options_argument_errors():
    """eps outside [0, 1), zc < 0: TA_ERR_ARG, nothing written; NULL options and all-zero options without a buffer: the plain call."""
    n, ldl, V = 4, 8, 8
    z = torch.zeros(n, ldl, device=DEV)
    t = torch.zeros(n, dtype=torch.int64, device=DEV)
    nll, obj, loss, dl = Guarded(n), Guarded(n), Guarded(1, None, F32, torch.zeros(1)), Guarded(n, ldl, BF16)
    for eps, zc in ((1.0, 0.0), (-0.1, 0.0), (0.0, -1e-4), (float("nan"), 0.0)):
        opt = _lib.CeOptions(eps=eps, zc=zc, obj=obj.full.data_ptr())
        call(EP, ptr(z), 0, ldl, None, ptr(t), n, V, 1.0, nll.p, loss.p, dl.p, ldl, C.byref(opt), stream(), expect=1)
    assert float(loss.get()[0]) == 0.0
    for buf in (nll, obj):
        assert bool((buf.get().view(torch.int32) == -1).all())
    assert bool((dl.get().view(torch.int16) == -1).all())
    call(EP, ptr(z), 0, ldl, None, ptr(t), n, V, 1.0, nll.p, loss.p, None, ldl, None, stream())
    off = _lib.CeOptions(eps=0.0, zc=0.0, obj=None)
    call(EP, ptr(z), 0, ldl, None, ptr(t), n, V, 1.0, nll.p, loss.p, None, ldl, C.byref(off), stream())
    assert abs(float(loss.get()[0]) - 2 * n * 2.0794415) < 1e-4 and bool((obj.get().view(torch.int32) == -1).all())
    # all-zero options WITH a buffer: the objective is the nll
    on = _lib.CeOptions(eps=0.0, zc=0.0, obj=obj.full.data_ptr())
    call(EP, ptr(z), 0, ldl, None, ptr(t), n, V, 1.0, nll.p, loss.p, None, ldl, C.byref(on), stream())
    assert torch.equal(obj.get(), nll.get())


# ----------------------------------------------------------------------------- through the model
# Truth: transformers' Qwen3ForCausalLM / SmolLM3ForCausalLM in fp32 on the CPU (tests/test_gpu_packing.py builds them from the SMALL
# configuration, the one of tests/golden/qwen3_small.npz; SmolLM3: no q/k-norm, last layer NoPE), every clip as its own row, under
# functional_call + autograd of the float64 objective of tests/loss_options_ref.py.  Gates: the existing ones for the same quantities
# (loss 5e-3 relative, d(audio) cosine > 0.999, adapter gradients cosine > 0.998: tests/test_gpu_smollm3.py, tests/test_gpu_packing.py).
EPS, ZC = 0.1, 1e-4
GATE_DX, GATE_LORA = 0.999, 0.998
# On a random-weight LM the objective and the plain CE differ by 0.2 % and their gradients by a factor near 1 - eps in length, hardly at all
# in direction: neither the 5e-3 loss gate nor a cosine can tell whether the options were applied.  Two more checks can:
#   * adapter gradients also within relmax 6e-2 of the truth (the gate of tests/test_gpu_parity.py:356 and tests/test_gpu_packing.py:260),
#     which a gradient 10 % too long misses;
#   * (loss with options) - (loss without) against the same difference of the truth.  It is eps * mean_r (z_rt - mean_v z_rv) plus the
#     z-loss term, linear in the logits; the logits gate of these files allows an RMS error of 0.02 per logit, so the two logit terms
#     together move it by at most eps * 2 * 0.02 (the z-loss term moves by 2 zc lse * 0.02, two orders below).
GATE_RELMAX = 6e-2
DELTA_TOL = lambda eps: eps * 2 * 0.02


def _far(c):
    """A vector of the same length within cosine c of g lies within sqrt(2 (1 - c)) |g| of it: what a cosine gate of c forgives."""
    return float(np.sqrt(2.0 * (1.0 - c)))


def _reldiff(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


_TRUTH = {}


def _truth(kind, rows, eps, zc, lora=None, drop=None):
    """One clip per row on the CPU -> dict(loss, dx [R, Lp, D], grads {adapter matrix: d(loss)}) for the objective (eps, zc).
    ``lora``: the adapter matrices (default: oracle.weights.init_lora, rank 8).  ``drop`` = (p, seed, offset): LoRA dropout as peft's
    training-mode LoraLayer -- every adapted linear adds s B A (x * keep / (1 - p)) through a forward hook, keep being the numpy twin of
    the device masks (tiny_audio_amd.lora_dropout.keep_mask, pinned to the device by tests/test_gpu_lora_dropout.py) at the token's
    row of the [R * Lp] row space, as in that file's _torch_layer_ref.  Runs without ``lora`` and ``drop`` are computed once."""
    from torch.func import functional_call
    from tests import test_gpu_packing as P
    from oracle import weights as OW
    from tiny_audio_amd import lora_dropout as LD
    key = (kind, str(rows), eps, zc)
    if lora is None and drop is None and key in _TRUTH:
        return _TRUTH[key]
    cfg, w, model = P.small(kind, 4, 2 if kind == "qwen3" else 1)
    x, sid, lab, clips = P.packed_batch(rows, cfg["hidden"], cfg["vocab"])
    given = lora is not None or drop is not None
    lora = lora if lora is not None else OW.init_lora(cfg, rank=8)
    params = {k: v.detach() for k, v in model.named_parameters()}
    lo = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in lora.items()}
    n_tot = int((lab != -100).sum())
    out = dict(dx=np.zeros_like(x), grads={k: 0 for k in lo}, loss=0.0, x=x, sid=sid, lab=lab, clips=clips, cfg=cfg, w=w, lora=lora,
               model=model)
    Lp = x.shape[1]
    adapted = {name: mod for name, mod in model.named_modules() if isinstance(mod, torch.nn.Linear) and f"{name}.lora_A" in lo}
    assert len(adapted) * 2 == len(lo)
    keeps = {}
    if drop is not None:
        for name, mod in adapted.items():
            layer, j = int(name.split("layers.")[1].split(".")[0]), LD.PEFT_ORDER.index(name.rsplit(".", 1)[1])
            keeps[name] = torch.from_numpy(LD.keep_mask(*drop, layer, j, x.shape[0] * Lp, mod.in_features)).float() * float(LD.inv_keep(drop[0]))
    for (r, at, n) in clips:
        eff, hooks = dict(params), []
        for name, mod in adapted.items():
            A, Bm = lo[name + ".lora_A"], lo[name + ".lora_B"]
            if drop is None:                          # no dropout: the merged weight W + s B A
                eff[name + ".weight"] = params[name + ".weight"] + 4.0 * Bm @ A
            else:
                k = keeps[name][r * Lp + at:r * Lp + at + n]
                hooks.append(mod.register_forward_hook(
                    lambda mod_, inp, o, A=A, Bm=Bm, k=k: o + (4.0 * (((inp[0].reshape(n, -1) * k) @ A.t()) @ Bm.t())).reshape(o.shape)))
        xe = torch.from_numpy(x[r:r + 1, at:at + n]).requires_grad_(True)
        try:
            lg = functional_call(model, eff, args=(), kwargs=dict(inputs_embeds=xe, use_cache=False)).logits
        finally:
            for h in hooks:
                h.remove()
        s = LO.objective(lg, torch.from_numpy(lab[r:r + 1, at:at + n]), eps, zc, num_items=n_tot)
        names = list(lo)
        g = torch.autograd.grad(s, [xe] + [lo[k] for k in names])
        out["dx"][r, at:at + n] = g[0][0].numpy()
        for k, gg in zip(names, g[1:]):
            out["grads"][k] = out["grads"][k] + gg.numpy()
        out["loss"] += float(s.detach())
    if not given:
        _TRUTH[key] = out
    return out


def _asr_model(kind, ref, lora_dropout=0.0):
    """ASRModel around the tiny LM with rank-8 adapters; the projector's output is handed in by the test (``_feed``)."""
    from oracle import weights as OW
    from tiny_audio_amd.asr_config import ASRConfig
    from tiny_audio_amd.asr_modeling import ASRModel
    cfg = ref["cfg"]
    text = dict(ref["model"].config.to_dict()) if kind == "smollm3" else cfg
    enc = OW.enc_config(hidden=256, ffn=512, layers=1, heads=4)
    m = ASRModel(ASRConfig(audio_config=enc, text_config=text, projector_hidden_dim=128, audio_token_id=cfg["vocab"] - 1, pad_token_id=990,
                           eos_token_id=991, use_lora=True, freeze_projector=True, lora_dropout=lora_dropout), device=DEV, init="none")
    m.language_model.load_state_dict_hf(ref["w"])
    m.language_model.load_lora_state_dict(ref["lora"])
    return m


def _feed(m, ref, packed):
    """-> (the leaf standing for the projector's output, forward keyword arguments).  Every token is an <audio> placeholder, so the
    LM's inputs_embeds are the leaf's rows: [R, Lp, D] one clip per row (right padding), or [C, N, D] per clip for packed rows."""
    x, sid, lab, clips = ref["x"], ref["sid"], ref["lab"], ref["clips"]
    Rr, Lp, Dm = x.shape
    ids = torch.full((Rr, Lp), ref["cfg"]["vocab"] - 1, dtype=torch.int64)
    if packed:
        N = max(n for _, _, n in clips)
        y = np.zeros((len(clips), N, Dm), np.float32)
        for c, (r, at, n) in enumerate(clips):
            y[c, :n] = x[r, at:at + n]
        kw = dict(segment_ids=torch.from_numpy(sid).long(), audio_token_counts=torch.tensor([n for _, _, n in clips]))
    else:
        y = x
        kw = dict(attention_mask=torch.from_numpy((sid != 0).astype(np.int64)), audio_token_counts=torch.full((Rr,), Lp, dtype=torch.int64))
    leaf = torch.from_numpy(y).to(DEV).requires_grad_(True)
    m._encode_audio = lambda *a, **k: leaf                         # the frozen encoder + projector are not under test here
    kw.update(input_ids=ids, input_features=torch.zeros(y.shape[0], 128, 8), labels=torch.from_numpy(lab), return_logits=True)
    return leaf, kw


def _run(m, leaf, kw, ref, packed, **opts):
    """One forward + backward -> dict(loss, nll, logits [R, Lp, V] f64 on the host, dx in the layout of ref["dx"], grads by adapter)."""
    lm = m.language_model
    lm.lora_drop_offset = 0                                           # LoRA dropout: the same Philox offset, the same masks, in every run
    leaf.grad = None
    for p in lm.lora_parameters():
        p.grad = None
    out = m(**kw, **opts)
    out.loss.backward()
    torch.cuda.synchronize()
    g = leaf.grad.detach().float().cpu().numpy()
    dx = np.zeros_like(ref["dx"])
    if packed:
        for c, (r, at, n) in enumerate(ref["clips"]):
            dx[r, at:at + n] = g[c, :n]
    else:
        dx = g
    keep = [p.detach().clone() for p in lm.lora_parameters()]
    with torch.no_grad():
        for p in lm.lora_parameters():
            p.copy_(p.grad)
        grads = {k: v.detach().float().cpu().numpy() for k, v in lm.export_lora_state_dict(prefix="model.", suffix="").items()}
        for p, k in zip(lm.lora_parameters(), keep):
            p.copy_(k)
    return dict(loss=float(out.loss.detach()), loss_ce=float(out.loss_ce.detach()), nll=out.nll.detach().cpu(),
                logits=out.logits.detach().double().cpu(), dx=dx, grads=grads, loss_t=out.loss.detach().clone(),
                raw=[leaf.grad.detach().clone()] + [p.grad.detach().clone() for p in lm.lora_parameters()])


def _check_model(kind, rows, packed, tag, lora_dropout=0.0):
    """``lora_dropout`` > 0: the LM in training mode (the _ex call shape), every run at Philox offset 0, the truth under the same masks."""
    ref, ref0 = _truth(kind, rows, EPS, ZC), _truth(kind, rows, 0.0, 0.0)
    m = _asr_model(kind, ref, lora_dropout)
    m.train()
    if lora_dropout > 0.0:
        m.language_model.train(True)
        drop = (lora_dropout, m.language_model.lora_drop_seed, 0)
        ref, ref0 = _truth(kind, rows, EPS, ZC, drop=drop), _truth(kind, rows, 0.0, 0.0, drop=drop)
    leaf, kw = _feed(m, ref, packed)
    on = _run(m, leaf, kw, ref, packed, label_smoothing=EPS, z_loss_coef=ZC)
    off = _run(m, leaf, kw, ref, packed)
    real = ref["sid"] != 0
    lab = torch.from_numpy(ref["lab"])
    # the loss is the reference objective of the logits this forward returned, and of the truth's
    own = float(LO.objective(on["logits"], lab, R.f32v(EPS), R.f32v(ZC)))
    cs = P_cos(on["dx"][real], ref["dx"][real])
    worst = min(P_cos(on["grads"][k], ref["grads"][k]) for k in ref["grads"])
    d_dx, d_lo = _reldiff(on["dx"][real], off["dx"][real]), min(_reldiff(on["grads"][k], off["grads"][k]) for k in ref["grads"])
    print(f"[lossopt] {tag}: loss {on['loss']:.5f}, objective of its logits {own:.5f}, truth {ref['loss']:.5f} (options off {off['loss']:.5f}, truth "
          f"{ref0['loss']:.5f}); d(audio) cosine {cs:.6f}, worst adapter cosine {worst:.6f}; options on vs off: d(audio) moves by {d_dx:.4f}, "
          f"adapters by >= {d_lo:.4f} (a cosine gate forgives {_far(GATE_DX):.4f} / {_far(GATE_LORA):.4f})")
    assert abs(on["loss"] - own) < 5e-3 * own, tag
    assert abs(on["loss"] - ref["loss"]) < 5e-3 * ref["loss"], tag
    assert abs((on["loss"] - off["loss"]) - (ref["loss"] - ref0["loss"])) < DELTA_TOL(EPS), tag
    assert on["loss_ce"] == on["loss"]
    assert abs(off["loss"] - ref0["loss"]) < 5e-3 * ref0["loss"], tag
    assert set(on["grads"]) == set(ref["grads"])
    assert cs > GATE_DX, tag
    for k in ref["grads"]:
        assert P_cos(on["grads"][k], ref["grads"][k]) > GATE_LORA, (tag, k)
        assert _relmax(on["grads"][k], ref["grads"][k]) < GATE_RELMAX, (tag, k)
    assert not on["dx"][~real].any(), tag
    # the options reach the backward: the gradients moved by more than the gates above would forgive ...
    assert d_dx > _far(GATE_DX) and d_lo > _far(GATE_LORA), tag
    # ... while nll stays the plain one, bit for bit
    assert torch.equal(on["nll"], off["nll"]) and abs(float(on["nll"].sum()) / on["nll"].numel() - off["loss"]) < 1e-5 * off["loss"]
    # options off: omitting the arguments and passing the defaults are the same call -- the same bits in the loss and every gradient
    explicit = _run(m, leaf, kw, ref, packed, label_smoothing=0.0, z_loss_coef=0.0)
    assert torch.equal(off["loss_t"], explicit["loss_t"]) and all(torch.equal(a, b) for a, b in zip(off["raw"], explicit["raw"])), tag
    return m, leaf, kw, ref


def _relmax(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / (np.abs(b).max() + 1e-30))


def P_cos(a, b):
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))


@pytest.mark.parametrize("kind", ["qwen3", "smollm3"])
def test_model_forward_one_clip_per_row(kind):
    _check_model(kind, [[48], [40]], False, f"{kind} one clip per row")


def test_model_forward_packed_rows():
    _check_model("qwen3", [[30, 34], [40]], True, "qwen3 packed")


def test_model_forward_with_lora_dropout():
    """lora_dropout 0.1, the LM in training mode (the _ex call shape): the same checks, the truth carrying the numpy twin of the masks."""
    rows = [[48], [40]]
    m, leaf, kw, ref = _check_model("qwen3", rows, False, "qwen3 lora dropout 0.1", lora_dropout=0.1)
    on = _run(m, leaf, kw, ref, False, label_smoothing=EPS, z_loss_coef=ZC)
    again = _run(m, leaf, kw, ref, False, label_smoothing=EPS, z_loss_coef=ZC)
    assert torch.equal(on["loss_t"], again["loss_t"]) and all(torch.equal(a, b) for a, b in zip(on["raw"], again["raw"]))
    # the masks did something: the logits differ from the same model's without dropout, and so does the truth's loss
    m0 = _asr_model("qwen3", ref)
    m0.train()
    leaf0, kw0 = _feed(m0, ref, False)
    assert not torch.equal(on["logits"], _run(m0, leaf0, kw0, ref, False, label_smoothing=EPS, z_loss_coef=ZC)["logits"])
    assert abs(ref["loss"] - _truth("qwen3", rows, EPS, ZC)["loss"]) > 1e-6


def test_trainer_label_smoothing_factor():
    """ASRTrainer(label_smoothing_factor = 0.1) over two steps on the tiny Qwen3 with adapters: the logged loss is the objective, and the
    adapters move as torch.optim.AdamW moves them on the truth's gradients (clip at max_grad_norm 1, lr 1e-3; the tolerances are those of
    tests/test_gpu_parity.py::test_three_training_steps_vs_golden: losses 5e-3 relative, mean |weight difference| < 2e-4)."""
    from tiny_audio_amd.trainer import ASRTrainer, TrainingArguments
    rows, lr = [[48], [40]], 1e-3
    ref = _truth("qwen3", rows, EPS, 0.0)
    m = _asr_model("qwen3", ref)
    m.train()
    leaf, kw = _feed(m, ref, False)
    batch = {k: v for k, v in kw.items() if k != "return_logits"}
    with torch.no_grad():                                             # the plain CE of the first step's batch, by the same kernels
        plain = float(m(**kw).loss)
    tr = ASRTrainer(m, TrainingArguments(learning_rate=lr, weight_decay=0.0, max_grad_norm=1.0, label_smoothing_factor=EPS))
    # the truth: two AdamW steps on the adapter matrices
    lo = {k: torch.from_numpy(v).clone() for k, v in ref["lora"].items()}
    names = list(lo)
    opt = torch.optim.AdamW([lo[k] for k in names], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    want_losses, got_losses = [], []
    for step in range(2):
        t = _truth("qwen3", rows, EPS, 0.0, lora={k: v.detach().numpy().copy() for k, v in lo.items()})      # of THIS step's adapters
        want_losses.append(t["loss"])
        for k in names:
            lo[k].grad = torch.from_numpy(np.asarray(t["grads"][k], np.float32)).clone()
        torch.nn.utils.clip_grad_norm_([lo[k] for k in names], 1.0)
        opt.step()
        tr.training_step(batch)
        got_losses.append(tr.last_loss())
    print(f"[lossopt] trainer: logged losses {got_losses} vs objective {want_losses}")
    np.testing.assert_allclose(got_losses, want_losses, rtol=5e-3)
    # the logged loss is the objective, not the plain CE: their difference is the truth's (DELTA_TOL above)
    want_delta = want_losses[0] - _truth("qwen3", rows, 0.0, 0.0)["loss"]
    print(f"[lossopt] trainer: logged - plain {got_losses[0] - plain:.5f}, truth {want_delta:.5f}")
    assert abs((got_losses[0] - plain) - want_delta) < DELTA_TOL(EPS) < abs(want_delta)
    mine = m.language_model.export_lora_state_dict(prefix="model.", suffix="")
    moved = 0.0
    for k in names:
        d = np.abs(mine[k].detach().float().cpu().numpy() - lo[k].numpy())
        moved = max(moved, float(np.abs(lo[k].numpy() - ref["lora"][k]).mean()))
        assert d.mean() < 2e-4, (k, d.mean())
    assert moved > 5e-4                                               # two steps of lr 1e-3 did move the adapters
