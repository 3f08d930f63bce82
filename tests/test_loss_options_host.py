"""LM loss options (label smoothing, z-loss) without a GPU: the C header, the call sequence under DRY_RUN (the stubs of
tests/test_dryrun_plumbing.py: arguments are marshalled through the real ctypes prototypes, nothing is computed), the refusals, the
config round trip and the ISA of the four cross-entropy kernels."""
import json
import re

import pytest
import torch

from oracle import weights as OW
from tiny_audio_amd import _lib

ENC = OW.enc_config(hidden=256, ffn=512, layers=1, heads=4)
LM = OW.lm_config(vocab=1000, hidden=256, ffn=512, layers=2, heads=4, kv_heads=2)

# What one forward + backward launched before the options existed (recorded on the commit before them), per call shape.
BEFORE = {
    "plain": ["ta_encoder_forward", "ta_cast_f32_bf16", "ta_cast_f32_bf16", "ta_transpose_to_bf16", "ta_mlp_projector_forward",
              "ta_audio_index", "ta_lm_forward_loss", "ta_lm_backward", "ta_mlp_projector_backward"],
    "ex": ["ta_encoder_forward", "ta_cast_f32_bf16", "ta_cast_f32_bf16", "ta_transpose_to_bf16", "ta_mlp_projector_forward",
           "ta_audio_index", "ta_lm_forward_loss_ex", "ta_lm_backward_ex", "ta_mlp_projector_backward"],
    "seg": ["ta_segment_table", "ta_encoder_forward", "ta_cast_f32_bf16", "ta_cast_f32_bf16", "ta_transpose_to_bf16",
            "ta_mlp_projector_forward", "ta_audio_index_seg", "ta_label_rows", "ta_lm_forward_loss_seg", "ta_lm_backward_seg",
            "ta_mlp_projector_backward"],
}


@pytest.fixture()
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


def _model(**over):
    from tiny_audio_amd.asr_config import ASRConfig
    from tiny_audio_amd.asr_modeling import ASRModel
    cfg = ASRConfig(audio_config=ENC, text_config=LM, projector_hidden_dim=128, audio_token_id=999, **over)
    return ASRModel(cfg, device="cpu", init="random")


def _batch():
    ids, att, lab, counts = OW.synthetic_tokens(2, [12, 12], 1000, 999, 990, 991, n_text=10, n_suffix=4)
    meta = (torch.zeros(40, dtype=torch.int32), torch.zeros(40, dtype=torch.int64), 22)
    return dict(input_ids=torch.from_numpy(ids), input_features=torch.zeros(2, 128, 100), attention_mask=torch.from_numpy(att),
                labels=torch.from_numpy(lab), audio_token_counts=torch.from_numpy(counts), label_meta=meta)


def _packed_batch():
    """Two rows, three clips: [12 + 9 placeholders] and [12], 100 mel frames per clip (12 projector rows)."""
    A = 999
    seg = [[5, 6] + [A] * 12 + [7, 8, 9], [5] + [A] * 9 + [7, 8], [5, 6] + [A] * 12 + [7, 8, 9, 10]]
    L = len(seg[0]) + len(seg[1])
    ids = torch.zeros((2, L), dtype=torch.int64); sid = torch.zeros((2, L), dtype=torch.int64)
    ids[0, :17] = torch.tensor(seg[0]); ids[0, 17:29] = torch.tensor(seg[1]); sid[0, :17] = 1; sid[0, 17:29] = 2
    ids[1, :18] = torch.tensor(seg[2]); sid[1, :18] = 1
    lab = torch.where((ids != A) & (sid != 0), ids, torch.full_like(ids, -100))
    return dict(input_ids=ids, segment_ids=sid, attention_mask=(sid != 0).long(), labels=lab, input_features=torch.zeros(3, 128, 100),
                audio_token_counts=torch.tensor([12, 9, 12]))


def _shape(kind):
    """(model in training mode, batch) of one of the three call shapes: plain, LoRA dropout (_ex), packed (_seg)."""
    if kind == "plain":
        m, b = _model(), _batch()
    elif kind == "ex":
        m, b = _model(use_lora=True, freeze_projector=False, lora_dropout=0.1), _batch()
    else:
        m, b = _model(), _packed_batch()
    m.train()
    if kind == "ex":
        m.language_model.train(True)
    return m, b


class _Options:
    """Records the ta_ce_options (and whether a table / a dropout descriptor came along) of every ta_lm_forward_loss_opt call."""

    def __init__(self, dry, monkeypatch):
        self.seen = []
        stub = dry.ta_lm_forward_loss_opt

        def rec(*args):
            ce = args[20]._obj
            self.seen.append((round(ce.eps, 6), round(ce.zc, 8), bool(ce.obj), args[6] is not None, args[19] is not None))
            return stub(*args)
        monkeypatch.setattr(dry, "ta_lm_forward_loss_opt", rec, raising=False)


# ----------------------------------------------------------------------------- header
def test_header_declares_the_entry_points_and_keeps_the_abi_version():
    protos = _lib.parse_header()
    assert len(protos["ta_cross_entropy_opt"][1]) == len(protos["ta_cross_entropy"][1]) + 1
    assert len(protos["ta_lm_forward_loss_opt"][1]) == len(protos["ta_lm_forward_loss_seg"][1]) + 1
    text = open(_lib.HEADER).read()
    for name in ("ta_cross_entropy_opt", "ta_lm_forward_loss_opt"):
        before = text[:text.index(f"int {name}(")]
        note = before[before.rindex("/*"):]
        assert "TF:trainer_pt_utils.py LabelSmoother" in note and "TF:loss/loss_utils.py fixed_cross_entropy" in note, name
    assert re.search(r"typedef struct ta_ce_options \{\s*float eps;.*?float zc;.*?float\* obj;", text, flags=re.S)
    assert [f[0] for f in _lib.CeOptions._fields_] == ["eps", "zc", "obj"]
    L = _lib.lib()
    assert L.ta_version() == 4                                        # additive: the ABI version does not move
    for name in ("ta_cross_entropy_opt", "ta_lm_forward_loss_opt", "ta_cross_entropy", "ta_lm_forward_loss", "ta_lm_forward_loss_ex",
                 "ta_lm_forward_loss_seg"):
        assert getattr(L, name) is not None, name                     # exported: the old entry points next to the new ones


# ----------------------------------------------------------------------------- plumbing
@pytest.mark.parametrize("kind", ["plain", "ex", "seg"])
def test_options_off_launch_what_was_launched_before(dry, kind):
    """Options at 0 -- left out, passed as 0, or 0 in the config -- the three forwards and their backwards are the calls of BEFORE."""
    for how in ("omitted", "explicit", "config"):
        m, b = _shape(kind)
        if how == "config":
            m.config.label_smoothing, m.config.lm_z_loss_coef = 0.0, 0.0
        extra = dict(label_smoothing=0.0, z_loss_coef=0.0) if how == "explicit" else {}
        dry.calls.clear()
        m(**b, return_logits=False, **extra).loss.backward()
        assert list(dry.calls) == BEFORE[kind], (kind, how)


@pytest.mark.parametrize("kind", ["plain", "ex", "seg"])
def test_options_on_launch_the_new_entry_point_once(dry, monkeypatch, kind):
    rec = _Options(dry, monkeypatch)
    m, b = _shape(kind)
    fwd = {"plain": "ta_lm_forward_loss", "ex": "ta_lm_forward_loss_ex", "seg": "ta_lm_forward_loss_seg"}[kind]
    expect = [("ta_lm_forward_loss_opt" if c == fwd else c) for c in BEFORE[kind]]        # the backward is the one of the call shape
    # per-call override
    dry.calls.clear()
    m(**b, return_logits=False, label_smoothing=0.1, z_loss_coef=1e-4).loss.backward()
    assert list(dry.calls) == expect
    assert rec.seen == [(0.1, 1e-4, True, kind == "seg", kind == "ex")]
    # from the config; a call argument overrides one of the two
    m.config.label_smoothing, m.config.lm_z_loss_coef = 0.2, 1e-3
    rec.seen.clear(); dry.calls.clear()
    m(**b, return_logits=False)
    m(**b, return_logits=False, z_loss_coef=0.0)
    m(**b, return_logits=False, label_smoothing=0.0)
    assert [s[:2] for s in rec.seen] == [(0.2, 1e-3), (0.2, 0.0), (0.0, 1e-3)]
    assert dry.calls.count("ta_lm_forward_loss_opt") == 3 and fwd not in dry.calls
    # eval(): as in HF the options apply whenever labels are given ...
    m.eval()
    rec.seen.clear()
    with torch.no_grad():
        m(**b, return_logits=False)
    assert [s[:2] for s in rec.seen] == [(0.2, 1e-3)]
    # ... and not without labels
    rec.seen.clear(); dry.calls.clear()
    with torch.no_grad():
        m(**{k: v for k, v in b.items() if k not in ("labels", "label_meta")})
    assert rec.seen == [] and "ta_lm_forward_loss_opt" not in dry.calls


def test_trainer_hands_label_smoothing_factor_to_the_forward(dry, monkeypatch):
    from tiny_audio_amd.trainer import ASRTrainer, TrainingArguments
    rec = _Options(dry, monkeypatch)
    m, b = _shape("plain")
    m.config.lm_z_loss_coef = 1e-4
    tr = ASRTrainer(m, TrainingArguments(label_smoothing_factor=0.1))
    dry.calls.clear()
    tr.training_step(b)
    assert [s[:3] for s in rec.seen] == [(0.1, 1e-4, True)]
    assert dry.calls.count("ta_lm_forward_loss_opt") == 1 and "ta_lm_forward_loss" not in dry.calls and "ta_lm_backward" in dry.calls
    assert TrainingArguments().label_smoothing_factor == 0.0
    # factor 0: the config decides; both 0: the call as it was
    m2, b2 = _shape("plain")
    tr2 = ASRTrainer(m2, TrainingArguments())
    rec.seen.clear(); dry.calls.clear()
    tr2.training_step(b2)
    assert rec.seen == [] and "ta_lm_forward_loss" in dry.calls and "ta_lm_forward_loss_opt" not in dry.calls


def test_raw_forward_loss_and_operator_take_the_options(dry, monkeypatch):
    """Qwen3MI355X.forward_loss(label_smoothing=, z_loss=) and the trailing arguments of ta355::lm_forward_loss."""
    rec = _Options(dry, monkeypatch)
    m, b = _shape("plain")
    lm = m.language_model
    ids = b["input_ids"]
    B, L = ids.shape
    rows, tg = torch.zeros(B * L, dtype=torch.int32), torch.zeros(B * L, dtype=torch.int64)
    audio = torch.zeros(4, 256)
    loss, nll, logits, ctx = lm.forward_loss(ids, None, audio, None, rows, tg, 5, 0.2, label_smoothing=0.1, z_loss=1e-2)
    assert rec.seen == [(0.1, 1e-2, True, False, False)] and ctx["obj"].shape == (5,) and nll.shape == (5,)
    _, _, _, ctx0 = lm.forward_loss(ids, None, audio, None, rows, tg, 5, 0.2)
    assert "obj" not in ctx0 and dry.calls[-1] == "ta_lm_forward_loss"
    from tiny_audio_amd import torch_ops
    schema = str(torch.ops.ta355.lm_forward_loss.default._schema)
    assert schema.index("lora_offset") < schema.index("float label_smoothing=0.") < schema.index("float z_loss=0.")
    rec.seen.clear()
    torch.ops.ta355.lm_forward_loss(audio, [], torch_ops.register_module(lm), ids, None, None, rows, tg, 5, 0.2, False, None, None,
                                    0.0, 0, 0, 0.3, 0.0)
    assert rec.seen == [(0.3, 0.0, True, False, False)]
    from tiny_audio_amd import ops
    z, t = torch.zeros(3, 8), torch.zeros(3, dtype=torch.int64)
    assert len(ops.cross_entropy_opt(z, t, 7, 1.0, label_smoothing=0.1)) == 4 and dry.calls[-1] == "ta_cross_entropy_opt"
    assert len(ops.cross_entropy_opt(z, t, 7, 1.0)) == 4 and dry.calls[-1] == "ta_cross_entropy_opt"
    assert len(ops.cross_entropy(z, t, 7, 1.0)) == 3 and dry.calls[-1] == "ta_cross_entropy"


# ----------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("eps,zc", [(1.0, 0.0), (-0.1, 0.0), (0.0, -1e-4), (float("nan"), 0.0)])
def test_refusals(dry, eps, zc):
    from tiny_audio_amd import ops
    from tiny_audio_amd.asr_config import ASRConfig
    m, b = _shape("plain")
    dry.calls.clear()
    with pytest.raises(ValueError):
        m(**b, label_smoothing=eps, z_loss_coef=zc)
    with pytest.raises(ValueError):                                   # without labels too: refused, not ignored
        m(**{k: v for k, v in b.items() if k not in ("labels", "label_meta")}, label_smoothing=eps, z_loss_coef=zc)
    assert dry.calls == []                                            # refused before the encoder ran
    ids = b["input_ids"]
    with pytest.raises(ValueError):
        m.language_model.forward_loss(ids, None, torch.zeros(4, 256), None, None, None, 0, 1.0, label_smoothing=eps, z_loss=zc)
    with pytest.raises(ValueError):
        ops.cross_entropy_opt(torch.zeros(3, 8), torch.zeros(3, dtype=torch.int64), 7, 1.0, label_smoothing=eps, z_loss=zc)
    assert not any(c.startswith(("ta_lm_forward_loss", "ta_cross_entropy")) for c in dry.calls)
    with pytest.raises(ValueError):
        ASRConfig(audio_config=ENC, text_config=LM, label_smoothing=eps, lm_z_loss_coef=zc)


def test_lm_entry_point_refuses_options_without_objective_buffer():
    """ta_lm_forward_loss_opt with eps > 0 or zc > 0 and obj NULL: TA_ERR_ARG (the loss would be summed with one float atomic per row).
    The check stands in front of everything else, so the real library answers it on the host: B = 0, no launch either way."""
    import ctypes as C
    L, w, buf = _lib.lib(), _lib.LmWeights(), (C.c_float * 4)()
    call = lambda ce: L.ta_lm_forward_loss_opt(C.byref(w), None, None, None, None, None, None, 0, 0, None, None, 0, 1.0, None, None, None,
                                               None, None, 0, None, None if ce is None else C.byref(ce), None)
    assert call(_lib.CeOptions(eps=0.1, zc=0.0, obj=None)) == 1
    assert call(_lib.CeOptions(eps=0.0, zc=1e-4, obj=None)) == 1
    assert call(_lib.CeOptions(eps=1.0, zc=0.0, obj=C.addressof(buf))) == 1
    assert call(_lib.CeOptions(eps=0.1, zc=1e-4, obj=C.addressof(buf))) == 0
    assert call(_lib.CeOptions(eps=0.0, zc=0.0, obj=None)) == 0 and call(None) == 0


# ----------------------------------------------------------------------------- config
def test_config_round_trips(tmp_path):
    from tiny_audio_amd.asr_config import ASRConfig
    from tiny_audio_amd.asr_modeling import ASRModel
    c0 = ASRConfig(audio_config=ENC, text_config=LM)
    assert c0.label_smoothing == 0.0 and c0.lm_z_loss_coef == 0.0
    d0 = c0.to_dict()
    assert d0["label_smoothing"] == 0.0 and d0["lm_z_loss_coef"] == 0.0
    cfg = ASRConfig(audio_config=ENC, text_config=LM, projector_hidden_dim=128, audio_token_id=999, label_smoothing=0.1,
                    lm_z_loss_coef=1e-4)
    d = json.loads(json.dumps(cfg.to_dict()))
    assert d["label_smoothing"] == 0.1 and d["lm_z_loss_coef"] == 1e-4
    back = ASRConfig(**d)
    assert back.label_smoothing == 0.1 and back.lm_z_loss_coef == 1e-4
    m = ASRModel(cfg, device="cpu", init="random")
    m.save_pretrained(tmp_path / "ck")
    saved = json.load(open(tmp_path / "ck" / "config.json"))
    assert saved["label_smoothing"] == 0.1 and saved["lm_z_loss_coef"] == 1e-4
    b = ASRModel.from_pretrained(tmp_path / "ck", device="cpu", init="random", seed=3)
    assert b.config.label_smoothing == 0.1 and b.config.lm_z_loss_coef == 1e-4


# ----------------------------------------------------------------------------- ISA
def _kernarg_ranges(code):
    """Byte ranges [start, end) of the kernel-argument block that a kernel's scalar loads read.  The first scalar load of a kernel can
    only go through the kernel-argument pointer (no other address exists yet); every load through that register pair counts."""
    loads = re.findall(r"s_load_dword(x\d+)?\s+s\[?[\d:]+\]?, (s\[\d+:\d+\]), (0x[0-9a-f]+|\d+)", code)
    assert loads, "no scalar loads found"
    base = loads[0][1]
    return [(int(at, 0), int(at, 0) + 4 * int(width[1:] if width else 1)) for width, b, at in loads if b == base]


def test_options_off_kernels_never_read_the_options():
    """csrc/loss.hip: one kernel template, four instantiations, none with scratch.  The argument block is (logits, ldl, rows, targets, V,
    scale, nll, loss, dlogits, ldd) in bytes [0, 72), then eps, zc at [72, 80) and obj at [80, 88).  The OPT = false kernels read nothing
    at or behind byte 72 and keep the 32 B of LDS of the two reductions; their OPT = true twins read all three options and are longer.
    (That the OPT = false instruction stream EQUALS the one before the options needs the previous source: profiles/loss_options.md.)"""
    import os
    import subprocess
    src = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "loss.hip")
    out = os.path.join(os.path.dirname(src), "build", "loss_isa.s")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [_lib.hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "--cuda-device-only",
           "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    isa = open(out).read()
    body, scratch = {}, {}
    for m in re.finditer(r"^(_Z\w*ce_fwd_bwd_kernel\w+):[^\n]*\n(.*?); ScratchSize: (\d+)", isa, re.S | re.M):
        body[m.group(1)], scratch[m.group(1)] = m.group(2).split("s_endpgm")[0], int(m.group(3))
    assert len(body) == 4 and all(v == 0 for v in scratch.values()), scratch
    lds = {k: int(re.search(r"\.amdhsa_kernel " + k + r"\b.*?\.amdhsa_group_segment_fixed_size (\d+)", isa, re.S).group(1)) for k in body}
    count = lambda k: sum(1 for l in body[k].splitlines() if l.startswith("\t") and not l.strip().startswith((";", ".")))
    for ty in ("f", "t"):                                             # float, unsigned short (bf16 bits)
        off, on = (next(k for k in body if f"ce_fwd_bwd_kernelI{ty}Lb{b}EE" in k) for b in (0, 1))
        assert all(end <= 72 for _, end in _kernarg_ranges(body[off])), (off, _kernarg_ranges(body[off]))
        read = _kernarg_ranges(body[on])
        assert all(any(lo <= byte < hi for lo, hi in read) for byte in (72, 76, 80, 84)), (on, read)
        assert lds[off] == 32 and lds[on] > 32, lds
        assert count(off) < count(on), (count(off), count(on))
