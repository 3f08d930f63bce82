"""wav2vec2 acoustic model, host side (no GPU): weight packing and export, argument errors, the operator and its dry run, the header's
citations, and ``ForcedAligner.align`` unchanged without ``acoustic_model``."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

from tests.golden import wav2vec2_recipe as R
from tiny_audio_amd import _lib, ops, torch_ops
from tiny_audio_amd import wav2vec2 as W
from tiny_audio_amd.alignment import ForcedAligner


@pytest.fixture()
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


def _model(geom="a", n_classes=32, labels="hf"):
    m = W.Wav2Vec2CtcMI355X(W.Wav2Vec2CtcConfig(**R.GEOMS[geom], n_classes=n_classes), device="cpu")
    return m.load_state_dict_hf(R.weights(geom), labels=labels)


# ----------------------------------------------------------------------------- packing
def test_defaults_are_the_base_960h_geometry():
    c = W.Wav2Vec2CtcConfig()
    assert (c.hidden_size, c.num_attention_heads, c.intermediate_size, c.num_hidden_layers, c.conv_dim, c.n_classes) == (768, 12, 3072, 12, 512, 29)
    assert c.layer_norm_eps == 1e-5 and W.CONV_KERNEL == (10, 3, 3, 3, 3, 2, 2) and W.CONV_STRIDE == (5, 2, 2, 2, 2, 2, 2)


def test_packed_images():
    sd, cfg = R.weights("a"), W.Wav2Vec2CtcConfig(**R.GEOMS["a"], n_classes=32)
    b = W.pack_state_dict(sd, cfg)
    H, Cd, cg = 256, 128, 16
    assert b["conv0_w"].shape == (Cd, 10) and b["conv0_w"].dtype == torch.float32
    w3 = torch.from_numpy(sd["wav2vec2.feature_extractor.conv_layers.3.conv.weight"])
    assert b["conv3_w"].shape == (Cd, 3 * Cd) and b["conv3_w"].dtype == torch.bfloat16
    assert torch.equal(b["conv3_w"][5, 2 * Cd + 7], w3[5, 7, 2].bfloat16())                 # column = tap * C + cin
    assert b["conv5_w"].shape == (Cd, 2 * Cd)
    # positional conv: [16][NB * 16][128 * cg], column = tap * cg + cin, weight norm folded with g != ||v||
    pw = W.fold_weight_norm(sd["wav2vec2.encoder.pos_conv_embed.conv.parametrizations.weight.original0"],
                            sd["wav2vec2.encoder.pos_conv_embed.conv.parametrizations.weight.original1"])
    assert b["pos_w"].shape == (16, 16, 128 * cg)
    assert torch.equal(b["pos_w"][3, 5, 77 * cg + 9], pw[3 * cg + 5, 9, 77].bfloat16())
    # q rows and q bias carry head_dim^-0.5 log2 e; k keeps its bias
    p = "wav2vec2.encoder.layers.1.attention."
    wq, bk = torch.from_numpy(sd[p + "q_proj.weight"]), torch.from_numpy(sd[p + "k_proj.bias"])
    assert torch.equal(b["layers.1.wqkv_fa"][:H], (wq * W.Q_SCALE).bfloat16()) and torch.equal(b["layers.1.bqkv_fa"][H:2 * H], bk)
    assert abs(W.Q_SCALE - 0.125 * 1.4426950408889634) < 1e-12
    assert b["head_w"].shape == (W.HEAD_PAD, H) and not b["head_w"][32:].any() and b["head_b"].shape == (32,)


def test_pos_conv_image_pads_odd_group_widths_with_zero_rows():
    w = torch.randn(16 * 24, 24, 128)
    img = W.pack_pos_conv(w)
    assert img.shape == (16, 32, 128 * 24) and not img[:, 24:].any()
    assert torch.equal(img[15, 23, 127 * 24 + 23], w[15 * 24 + 23, 23, 127].bfloat16())


@pytest.mark.parametrize("form", ["parametrizations", "weight_g", "plain"])
def test_weight_norm_forms_pack_alike(form):
    sd = R.weights("a")
    pc = "wav2vec2.encoder.pos_conv_embed.conv."
    g, v = sd.pop(pc + "parametrizations.weight.original0"), sd.pop(pc + "parametrizations.weight.original1")
    if form == "parametrizations":
        sd[pc + "parametrizations.weight.original0"], sd[pc + "parametrizations.weight.original1"] = g, v
    elif form == "weight_g":
        sd[pc + "weight_g"], sd[pc + "weight_v"] = g, v
    else:
        sd[pc + "weight"] = W.fold_weight_norm(g, v).numpy()
    cfg = W.Wav2Vec2CtcConfig(**R.GEOMS["a"], n_classes=32)
    assert torch.equal(W.pack_state_dict(sd, cfg)["pos_w"], W.pack_state_dict(R.weights("a"), cfg)["pos_w"])


def test_export_round_trip():
    m = _model("a")
    sd = m.export_state_dict_hf()
    assert "wav2vec2.encoder.pos_conv_embed.conv.weight_g" in sd and sd["lm_head.weight"].shape == (32, 256)
    m2 = W.Wav2Vec2CtcMI355X(m.config, device="cpu").load_state_dict_hf(sd)
    assert m._bufs.keys() == m2._bufs.keys()
    for k in m._bufs:                                                                      # bf16 images are a fixed point
        if k in ("pos_w", "pos_w_plain") or k.endswith("wqkv_fa"):
            # refolded / rescaled from an exported bf16 value instead of the fp32 master: one more bf16 rounding (2^-8 relative)
            np.testing.assert_allclose(m2._bufs[k].float().numpy(), m._bufs[k].float().numpy(), rtol=2 ** -7, atol=0)
        else:
            assert torch.equal(m._bufs[k], m2._bufs[k]), k
    w = sd["wav2vec2.feature_extractor.conv_layers.2.conv.weight"]
    want = torch.from_numpy(R.weights("a")["wav2vec2.feature_extractor.conv_layers.2.conv.weight"]).bfloat16().float().numpy()
    np.testing.assert_array_equal(w, want)


def test_random_init_is_seeded():
    cfg = W.Wav2Vec2CtcConfig(**R.GEOMS["a"], n_classes=29)
    a, b, c = (W.Wav2Vec2CtcMI355X(cfg, device="cpu").random_init(s) for s in (0, 0, 1))
    assert torch.equal(a._bufs["pos_w"], b._bufs["pos_w"]) and not torch.equal(a._bufs["pos_w"], c._bufs["pos_w"])
    assert a._w.n_classes == 29 and a._w.conv_dim == 128 and a._w.res_f32 == 0
    a.res_f32 = True
    assert a._w.res_f32 == 1


# ----------------------------------------------------------------------------- argument errors
def test_config_refuses_what_the_kernels_cannot_run():
    ok = dict(R.GEOMS["a"])
    for bad in (dict(hidden_size=320, num_attention_heads=5), dict(num_attention_heads=2), dict(intermediate_size=500),
                dict(conv_dim=100), dict(n_classes=65), dict(n_classes=0)):
        with pytest.raises(ValueError):
            W.Wav2Vec2CtcConfig(**{**ok, **bad})


def test_forward_refuses_bad_clips_before_any_device_work():
    m = _model("a")
    with pytest.raises(ValueError, match="399 samples is shorter than the 400"):
        m([np.zeros(8000, np.float32), np.zeros(399, np.float32)])
    with pytest.raises(ValueError, match="1-D"):
        m([np.zeros((2, 800), np.float32)])
    with pytest.raises(ValueError, match="lengths"):
        m([np.zeros(800, np.float32)], lengths=[800])
    with pytest.raises(ValueError, match="2 lengths for 3 clips"):
        m(torch.zeros(3, 800), lengths=[800, 800])
    with pytest.raises(ValueError, match="exceeds the padded width"):
        m(torch.zeros(2, 800), lengths=[800, 801])
    assert m([])[1] == [] and m([])[0].shape == (0, 32)
    with pytest.raises(_lib.Ta355Error, match="not loaded"):
        W.Wav2Vec2CtcMI355X(m.config, device="cpu")._forward_impl(torch.zeros(1, 800), [800])
    with pytest.raises(ValueError, match="labels"):
        W.Wav2Vec2CtcMI355X(m.config, device="cpu").load_state_dict_hf(R.weights("a"), labels="fairseq")


def test_c_abi_refuses_outside_the_envelope():
    """Host-side argument checks return TA_ERR_ARG before anything is launched, so they run without a GPU."""
    L = _lib.lib()
    one = C.c_void_p(64)                                                   # never dereferenced: every call below is refused
    assert L.ta_w2v_pos_conv(one, 0, one, one, C.c_void_p(128), one, 1, 10, 16 * 12, None) == 1       # 12 channels per group
    assert L.ta_w2v_pos_conv(one, 0, one, one, C.c_void_p(128), one, 1, 10, 16 * 72, None) == 1       # 72 > 64
    assert L.ta_w2v_pos_conv(one, 0, one, one, C.c_void_p(128), one, 1, 10, 250, None) == 1           # not 16 groups
    assert L.ta_w2v_pos_conv(one, 0, one, one, one, one, 1, 10, 256, None) == 1                        # in place
    assert L.ta_w2v_pos_conv(one, 0, None, one, C.c_void_p(128), one, 1, 10, 256, None) == 1
    assert L.ta_w2v_pos_conv(one, 0, one, one, C.c_void_p(128), one, 0, 10, 256, None) == 0            # empty batch: nothing launched
    assert L.ta_w2v_head_logsoftmax(one, 64, one, 65, one, 4, None) == 1 and L.ta_w2v_head_logsoftmax(one, 64, one, 0, one, 4, None) == 1
    assert L.ta_w2v_head_logsoftmax(one, 28, one, 29, one, 4, None) == 1 and L.ta_w2v_head_logsoftmax(one, 64, one, 29, one, 0, None) == 0
    assert L.ta_w2v_conv0_gn_gelu(one, one, 1, 9, one, one, one, 128, 1e-5, one, 100, one, 1 << 20, None) == 1      # Ls < 10
    assert L.ta_w2v_conv0_gn_gelu(one, one, 1, 8000, one, one, one, 128, 1e-5, one, 1598, one, 1 << 30, None) == 1  # slab stride < T0
    assert L.ta_w2v_conv0_gn_gelu(one, one, 1, 8000, one, one, one, 128, 1e-5, one, 1599, one,
                                  L.ta_w2v_conv0_ws_bytes(1, 8000, 128) - 1, None) == 1
    assert L.ta_w2v_conv0_ws_bytes(2, 8000, 128) >= (2 * 7 * 128 * 2 + 2 * 128 * 2) * 4
    m = _model("a")
    lens = np.asarray([8000, 399], np.int32)
    fwd = lambda lens, B, Ls, ws_bytes=1 << 40, w=m._w: L.ta_wav2vec2_forward(C.byref(w), one, lens.ctypes.data_as(C.c_void_p), one, one,
                                                                             B, Ls, one, one, ws_bytes, None)
    assert fwd(lens, 2, 8000) == 1                                         # a clip with no frame
    assert fwd(np.asarray([8000, 8001], np.int32), 2, 8000) == 1           # a clip longer than the row
    ok = np.asarray([8000, 4000], np.int32)
    need = L.ta_wav2vec2_workspace_bytes(C.byref(m._w), 2, 8000, 24 + 12)
    assert need > 2 * 1599 * 128 * 2 and fwd(ok, 2, 8000, ws_bytes=need - 1) == 1
    assert fwd(ok, 0, 8000) == 0
    bad = _model("a")
    bad._w.n_classes = 65
    assert fwd(ok, 2, 8000, w=bad._w) == 1
    bad._w.n_classes, bad._w.heads = 32, 3
    assert fwd(ok, 2, 8000, w=bad._w) == 1


# ----------------------------------------------------------------------------- header, operator, dry run
def test_header_cites_what_the_entry_points_replace():
    text = open(_lib.HEADER).read()
    for cite in ("tiny_audio/alignment.py:206-211", "TF:models/wav2vec2/modeling_wav2vec2.py:1667-1700",
                 "TF:models/wav2vec2/modeling_wav2vec2.py:302-323", "TF:models/wav2vec2/modeling_wav2vec2.py:326-379",
                 "#define TA_W2V_HEAD_PAD 64"):
        assert cite in text, cite
    protos = _lib.parse_header()
    for name, nargs in (("ta_wav2vec2_forward", 11), ("ta_wav2vec2_workspace_bytes", 4), ("ta_w2v_conv0_gn_gelu", 14),
                        ("ta_w2v_conv0_ws_bytes", 3), ("ta_w2v_pos_conv", 10), ("ta_w2v_head_logsoftmax", 7)):
        assert name in protos and len(protos[name][1]) == nargs, name
    assert "wav2vec2.hip" in _lib.SOURCES and _lib.lib().ta_version() == 4
    assert W.HEAD_PAD == 64


def test_operator_is_registered_with_a_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "wav2vec2_emissions" in torch_ops.OPERATORS
    s = str(torch.ops.ta355.wav2vec2_emissions.default._schema)
    assert s.startswith("ta355::wav2vec2_emissions(Tensor waveforms, SymInt[] lengths, SymInt handle) -> Tensor"), s
    m = _model("a")
    h = torch_ops.register_module(m)
    with FakeTensorMode():
        e = torch.ops.ta355.wav2vec2_emissions(torch.empty(3, 43200), [8000, 24000, 43200], h)
        assert e.shape == (24 + 74 + 134, 32) and e.dtype == torch.float32


def test_dry_run_marshals_through_the_real_prototypes(dry):
    m = _model("a", n_classes=29, labels="torchaudio")
    waves = R.waves()
    dry.calls.clear()
    em, frames = m(waves)
    assert dry.calls == ["ta_wav2vec2_forward"] and frames == [25, 140] and em.shape == (165, 29) and em.dtype == torch.float32
    dry.calls.clear()
    em2, frames2 = m(torch.zeros(2, 9000), lengths=torch.tensor([9000, 500]))
    assert frames2 == [27, 1] and em2.shape == (28, 29) and dry.calls == ["ta_wav2vec2_forward"]
    dry.calls.clear()
    out = ForcedAligner.align_audio_batch(waves, ["hello world", ""], m)
    assert dry.calls == ["ta_wav2vec2_forward", "ta_ctc_align_f32"] and len(out) == 2 and out[1] == []
    dry.calls.clear()
    ForcedAligner.align(waves[0], "hi there", acoustic_model=m)
    assert dry.calls == ["ta_wav2vec2_forward", "ta_ctc_align_f32"]
    with pytest.raises(ValueError, match="resample first"):
        ForcedAligner.align(waves[0], "hi", sample_rate=8000, acoustic_model=m)
    with pytest.raises(ValueError, match="2 clips but 1 texts"):
        ForcedAligner.align_audio_batch(waves, ["a"], m)
    # the primitive wrappers
    dry.calls.clear()
    x = torch.zeros(10, 256, dtype=torch.bfloat16)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    assert ops.w2v_pos_conv(x, m._bufs["pos_w"], m._bufs["pos_b"], cu, 6).shape == (10, 256)
    assert ops.w2v_head_logsoftmax(torch.zeros(7, 64), m._bufs["head_b"], 29).shape == (7, 29)
    y = ops.w2v_conv0_gn_gelu(torch.zeros(2, 800), torch.tensor([800, 400], dtype=torch.int32), m._bufs["conv0_w"], m._bufs["gn_w"], m._bufs["gn_b"])
    assert y.shape == (2, 159, 128) and y.dtype == torch.bfloat16
    assert dry.calls == ["ta_w2v_pos_conv", "ta_w2v_head_logsoftmax", "ta_w2v_conv0_gn_gelu"]


# ----------------------------------------------------------------------------- the existing path
def test_align_without_acoustic_model_is_unchanged(monkeypatch, dry):
    import inspect
    sig = inspect.signature(ForcedAligner.align)
    assert list(sig.parameters)[:5] == ["audio", "text", "sample_rate", "_language", "_batch_size"]
    assert sig.parameters["acoustic_model"].default is None and sig.parameters["acoustic_model"].kind is inspect.Parameter.KEYWORD_ONLY
    monkeypatch.setitem(sys.modules, "torchaudio", None)                   # "not installed", whatever the box has
    monkeypatch.setattr(ForcedAligner, "_model", None)
    with pytest.raises(ImportError, match="torchaudio is not installed: ForcedAligner.align needs it to compute wav2vec2 emissions"):
        ForcedAligner.align(np.zeros(16000, np.float32), "hello")
    with pytest.raises(ImportError, match="torchaudio is not installed"):
        ForcedAligner.align(np.zeros(16000, np.float32), "hello", acoustic_model=None)
    dry.calls.clear()
    ForcedAligner.align(None, "hi there", emission=torch.zeros(30, 29), acoustic_model=_model("a"))     # emission wins: no acoustic model run
    assert dry.calls == ["ta_ctc_align_f32"]
