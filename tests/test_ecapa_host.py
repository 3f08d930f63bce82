"""ECAPA-TDNN speaker-embedding model, host side (no GPU): config validation, weight packing (the Res2Net image against an unpacked
definition, the BatchNorm fold), the state-dict round trip on SpeechBrain's names, envelope errors from Python and from C, the
operator and its dry run, the header's citations."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ecapa_ref as REF
from tests.golden import ecapa_recipe as R
from tiny_audio_amd import _lib, ops, torch_ops
from tiny_audio_amd import ecapa as E

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


@pytest.fixture()
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


@pytest.fixture(scope="module")
def model_a():
    return E.EcapaTdnnMI355X(E.EcapaConfig(**R.GEOMS["a"]), device="cpu").load_state_dict_speechbrain(R.weights("a"))


# ----------------------------------------------------------------------------- config
def test_defaults_are_the_checkpoint_geometry():
    c = E.EcapaConfig()
    assert (c.channels, c.se_channels, c.attention_channels, c.lin_neurons, c.dilations, c.width) == (1024, 128, 128, 192, (2, 3, 4), 128)
    assert (E.N_FFT, E.HOP, E.N_MELS, E.FEAT_STRIDE, E.SCALE) == (400, 160, 80, 128, 8) and c.bn_eps == 1e-5
    assert E.frames_of(12000) == 76 and E.frames_of(3333) == 21 and E.frames_of(640) == 5


def test_config_refuses_what_the_kernels_cannot_run():
    ok = dict(R.GEOMS["a"])
    for bad in (dict(channels=64), dict(channels=192), dict(channels=2048), dict(se_channels=0), dict(se_channels=257),
                dict(attention_channels=32), dict(attention_channels=96), dict(attention_channels=320), dict(lin_neurons=190),
                dict(lin_neurons=0), dict(dilations=(2, 3)), dict(dilations=(2, 3, 5)), dict(dilations=(0, 3, 4))):
        with pytest.raises(ValueError):
            E.EcapaConfig(**{**ok, **bad})
    E.EcapaConfig(**ok)


# ----------------------------------------------------------------------------- tables and packing
def test_filter_bank_tables_are_the_definition():
    win, tw, mel, rng = E.fbank_tables()
    assert win.dtype == tw.dtype == mel.dtype == np.float32 and rng.dtype == np.int32
    assert np.array_equal(win, REF.hamming_window().astype(np.float32)) and np.array_equal(mel, REF.mel_filterbank().astype(np.float32))
    j = np.arange(400)
    assert np.abs(tw[:, 0] - np.cos(2 * np.pi * j / 400)).max() < 1e-7 and np.abs(tw[:, 1] + np.sin(2 * np.pi * j / 400)).max() < 1e-7
    assert mel.shape == (201, 80) and rng.shape == (80, 2)
    for m in range(80):
        lo, hi = rng[m]
        assert 0 <= lo < hi <= 201 and not mel[:lo, m].any() and not mel[hi:, m].any() and mel[lo, m] > 0 and mel[hi - 1, m] > 0
    assert win[0] == np.float32(0.08) and abs(float(win[200]) - 1.0) < 1e-7            # periodic: the maximum sits at n = 200


def test_batchnorm_fold():
    g = torch.Generator().manual_seed(0)
    w, b, m, v = torch.randn(33, generator=g), torch.randn(33, generator=g), torch.randn(33, generator=g), 0.5 + torch.rand(33, generator=g)
    x = torch.randn(4, 33, 7, generator=g)
    bn = torch.nn.BatchNorm1d(33).eval()
    bn.load_state_dict({"weight": w, "bias": b, "running_mean": m, "running_var": v, "num_batches_tracked": torch.tensor(0)})
    s, t = E.fold_batchnorm(w, b, m, v, eps=1e-5)
    assert s.dtype == t.dtype == F32
    with torch.no_grad():
        assert (bn(x) - (x * s[None, :, None] + t[None, :, None])).abs().max() < 1e-5
    s64, t64 = REF.fold_bn({"weight": w, "bias": b, "running_mean": m, "running_var": v}, "")
    assert np.abs(s.double().numpy() - s64).max() <= 2.0 ** -24 * np.abs(s64).max() and np.abs(t.double().numpy() - t64).max() < 1e-6


@pytest.mark.parametrize("w", [16, 48, 128])
def test_res2net_image_against_an_unpacked_definition(w):
    """Row co of conv m, column tap * w + cin is weight[co, cin, tap]; K is rounded up to 32 with zero columns.  A product of the image's
    rows with the operand row [x[t - d] | x[t] | x[t + d] | 0 ...] is the convolution."""
    g = torch.Generator().manual_seed(w)
    ws = [torch.randn(w, w, 3, generator=g) for _ in range(7)]
    img = E.pack_res2net(ws)
    kp = (3 * w + 31) // 32 * 32
    assert img.shape == (7, w, kp) and img.dtype == BF16 and not img[:, :, 3 * w:].any()
    for m in (0, 6):
        for co, ci, tap in ((0, 0, 0), (w - 1, w - 1, 2), (3, 5, 1)):
            assert img[m, co, tap * w + ci] == ws[m][co, ci, tap].to(BF16)
    x = torch.randn(9, w, generator=g).to(BF16).to(F64)
    d, t = 2, 4
    row = torch.cat([x[t - d], x[t], x[t + d], torch.zeros(kp - 3 * w, dtype=F64)])
    want = REF.conv1d(x.numpy(), ws[2].to(BF16).to(F64).numpy(), None, d)[t]
    assert np.abs((img[2].to(F64) @ row).numpy() - want).max() < 1e-9
    with pytest.raises(ValueError):
        E.pack_res2net(ws[:6] + [torch.zeros(w, w, 5)])


def test_packed_images(model_a):
    sd, b = R.weights("a"), model_a._bufs
    Cc, w = 128, 16
    assert b["w0"].shape == (Cc, 640) and b["w0"].dtype == BF16
    w0 = b["w0"].float().reshape(Cc, 5, 128)
    assert not w0[:, :, 80:].any() and torch.equal(w0[:, :, :80], torch.from_numpy(sd["blocks.0.conv.conv.weight"]).to(BF16).float().permute(0, 2, 1))
    assert b["blk0.res_w"].shape == (7, w, 64) and b["blk0.res_b"].shape == (7 * w,) and b["blk2.w1"].shape == (Cc, Cc)
    assert torch.equal(b["blk1.se_w1t"], torch.from_numpy(sd["blocks.2.se_block.conv1.conv.weight"])[:, :, 0].t())
    assert b["blk1.se_w1t"].shape == (Cc, 32) and b["blk1.se_w2t"].shape == (32, Cc) and b["blk1.se_w2t"].dtype == F32
    wa = torch.from_numpy(sd["asp.tdnn.conv.conv.weight"])[:, :, 0].to(BF16)
    assert torch.equal(b["att_wh"], wa[:, :3 * Cc]) and torch.equal(b["att_wms"], wa[:, 3 * Cc:]) and b["att_wms"].shape == (64, 6 * Cc)
    assert b["att_conv_w"].shape == (3 * Cc, 64) and b["fc_w"].shape == (64, 6 * Cc) and b["aspbn_s"].shape == (6 * Cc,)
    s, t = REF.fold_bn(sd, "blocks.3.res2net_block.blocks.4.norm.norm.")
    assert np.abs(b["blk2.res_s"][4 * w:5 * w].double().numpy() - s).max() < 1e-6 and np.abs(b["blk2.res_t"][4 * w:5 * w].double().numpy() - t).max() < 1e-6
    assert [model_a._w.blocks[i].dilation for i in range(3)] == [2, 3, 4] and model_a._w.channels == Cc and model_a._w.emb_dim == 64
    assert model_a._w.blocks[1].w2 == b["blk1.w2"].data_ptr() and model_a._w.fc_b == b["fc_b"].data_ptr()


def test_state_dict_names_and_shape_errors():
    cfg = E.EcapaConfig(**R.GEOMS["a"])
    sd = R.weights("a")
    names = E.state_dict_names(cfg)
    assert set(names) == set(sd) and len(names) == len(set(names))
    for n in ("blocks.0.conv.conv.weight", "blocks.1.tdnn1.norm.norm.running_var", "blocks.3.res2net_block.blocks.6.conv.conv.bias",
              "blocks.2.se_block.conv1.conv.weight", "mfa.norm.norm.weight", "asp.tdnn.conv.conv.weight", "asp.conv.conv.bias",
              "asp_bn.norm.running_mean", "fc.conv.weight"):
        assert n in names, n
    assert set(E.random_state_dict(cfg, 0)) == set(names)
    bad = dict(sd)
    bad["blocks.2.tdnn1.conv.conv.weight"] = np.zeros((128, 64, 1), np.float32)
    with pytest.raises(ValueError, match="blocks.2.tdnn1.conv.conv.weight"):
        E.pack_state_dict(bad, cfg)
    del bad["fc.conv.bias"]
    with pytest.raises((KeyError, ValueError)):
        E.pack_state_dict(bad, cfg)


def test_export_round_trip(model_a):
    sd = model_a.export_state_dict_speechbrain()
    assert set(sd) == set(R.weights("a"))
    src = R.weights("a")
    for k in ("blocks.0.conv.conv.weight", "blocks.1.res2net_block.blocks.3.conv.conv.weight", "blocks.3.se_block.conv2.conv.weight",
              "asp.tdnn.conv.conv.weight", "fc.conv.weight", "mfa.conv.conv.weight"):
        assert sd[k].shape == src[k].shape, k
        want = src[k] if "se_block" in k else torch.from_numpy(src[k]).to(BF16).float().numpy()
        assert np.array_equal(sd[k], want), k
    assert np.array_equal(sd["blocks.2.tdnn2.conv.conv.bias"], src["blocks.2.tdnn2.conv.conv.bias"])
    again = E.EcapaTdnnMI355X(model_a.config, device="cpu").load_state_dict_speechbrain(sd)
    assert set(again._bufs) == set(model_a._bufs)
    for k, v in model_a._bufs.items():
        assert torch.equal(again._bufs[k], v), k


def test_random_init_is_seeded():
    cfg = E.EcapaConfig(**R.GEOMS["a"])
    a, b, c = (E.EcapaTdnnMI355X(cfg, device="cpu").random_init(s) for s in (0, 0, 1))
    assert torch.equal(a._bufs["blk0.res_w"], b._bufs["blk0.res_w"]) and not torch.equal(a._bufs["blk0.res_w"], c._bufs["blk0.res_w"])


# ----------------------------------------------------------------------------- envelope
def test_python_refuses_bad_windows_before_any_device_work(model_a, dry):
    audio = np.zeros(50000, np.float32)
    dry.calls.clear()
    for args, match in ((([0], [500], 500), "4 frames; the kernels take 5 .. 512 frames"),
                        (([0], [40000], 512 * 160), "513 frames"),
                        (([0], [1666], 3333), "cannot be reflect-padded to 3333"),
                        (([0], [3334], 3333), "does not fit a window of 3333"),
                        (([48000], [3333], 3333), "lies outside the 50000 samples"),
                        (([-1], [3333], 3333), "lies outside"),
                        (([0, 1], [3333], 3333), "2 starts for 1 lengths")):
        with pytest.raises(ValueError, match=match):
            model_a.embed_windows(audio, *args)
    with pytest.raises(ValueError, match="1-D"):
        model_a.embed_windows(np.zeros((2, 4000), np.float32), [0], [3333], 3333)
    with pytest.raises(ValueError, match="relative lengths"):
        model_a.encode_batch(np.zeros((2, 4000), np.float32), wav_lens=torch.tensor([1.0, 0.5]))
    with pytest.raises(_lib.Ta355Error, match="weights not loaded"):
        E.EcapaTdnnMI355X(model_a.config, device="cpu")._embed_impl(torch.zeros(4000), [0], [3333], 3333)
    assert dry.calls == []
    assert model_a.embed_windows(audio, [], [], 3333).shape == (0, 64)


def test_c_abi_refuses_outside_the_envelope(model_a):
    """Host-side argument checks return TA_ERR_ARG before anything is launched, so they run without a GPU."""
    L = _lib.lib()
    one, two = C.c_void_p(64), C.c_void_p(4096)                             # never dereferenced: every call below is refused
    r2n = lambda T, w, d, ldz=1024, rpw=400, z=one, y=two: L.ta_ecapa_res2net(z, ldz, rpw, one, one, one, one, one, one, y, ldz, rpw, 3, T, w, d, None)
    assert r2n(76, 24, 2) == 1 and r2n(76, 144, 2) == 1 and r2n(76, 0, 2) == 1            # w: a multiple of 16 up to 128
    assert r2n(76, 16, 0) == 1 and r2n(76, 16, 5) == 1 and r2n(4, 16, 2) == 1 and r2n(513, 16, 2, rpw=600) == 1
    assert r2n(76, 128, 2, ldz=1000) == 1 and r2n(76, 16, 2, ldz=132) == 1 and r2n(76, 16, 2, rpw=75) == 1
    assert r2n(76, 16, 2, y=one) == 1 and r2n(76, 16, 2, z=C.c_void_p(72)) == 1            # in place; unaligned
    assert L.ta_ecapa_res2net(one, 1024, 400, one, one, one, one, one, one, two, 1024, 400, 0, 76, 16, 2, None) == 0
    assert L.ta_ecapa_fbank(one, 1000, one, one, 2, 639, one, one, one, one, one, one, None) == 1                # 4 frames
    assert L.ta_ecapa_fbank(one, 1000, one, one, 2, 513 * 160, one, one, one, one, one, one, None) == 1
    assert L.ta_ecapa_fbank(one, 1000, one, None, 2, 3333, one, one, one, one, one, one, None) == 1
    assert L.ta_ecapa_relu_bn(one, one, one, one, None, None, 3, 76, 127, None) == 1 and L.ta_ecapa_relu_bn(one, one, one, one, None, None, 3, 4, 128, None) == 1
    assert L.ta_ecapa_se_residual(one, one, one, one, one, one, one, one, 128, one, 384, 3, 76, 128, 257, one, None) == 1
    assert L.ta_ecapa_se_residual(one, one, one, one, one, one, one, one, 126, one, 384, 3, 76, 128, 32, one, None) == 1
    assert L.ta_ecapa_se_residual(one, one, one, one, one, one, one, one, 128, one, 384, 3, 76, 2048, 32, one, None) == 1
    assert L.ta_ecapa_attn_act(one, one, one, one, one, 3, 600, 64, None) == 1 and L.ta_ecapa_asp_pool(one, one, one, one, None, None, None, 3, 76, 384, None) == 1
    assert L.ta_ecapa_se_ws_floats(3, 128) == 768 and L.ta_ecapa_se_ws_floats(0, 128) == 0
    w = model_a._w
    st, ln = np.asarray([0, 100], np.int32), np.asarray([3333, 3333], np.int32)
    fwd = lambda st, ln, N, L_, chunk=8, n_audio=10000, ws_bytes=1 << 40, w=w: L.ta_ecapa_forward(
        C.byref(w), one, n_audio, st.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p), one, one, N, L_, chunk, one, one, ws_bytes, None)
    assert fwd(st, ln, 2, 500) == 1 and fwd(st, ln, 2, 513 * 160) == 1                     # T outside 5 .. 512
    assert fwd(st, np.asarray([3333, 1666], np.int32), 2, 3333) == 1                       # pad 1667 > len - 1
    assert fwd(st, np.asarray([3333, 3334], np.int32), 2, 3333) == 1
    assert fwd(np.asarray([0, 7000], np.int32), ln, 2, 3333) == 1                          # past the end of the audio
    assert fwd(np.asarray([0, -1], np.int32), ln, 2, 3333) == 1
    assert fwd(st, ln, 2, 3333, chunk=0) == 1 and fwd(st, ln, 0, 3333) == 0
    need = L.ta_ecapa_workspace_bytes(C.byref(w), 2, 21)
    assert need > 2 * 21 * (3 * 128 * 4 + 3 * 128 * 2 * 2) and fwd(st, ln, 2, 3333, ws_bytes=need - 1) == 1
    assert L.ta_ecapa_workspace_bytes(C.byref(w), 1, 21) < need and L.ta_ecapa_workspace_bytes(C.byref(w), 2, 4) == 0
    bad = E.EcapaTdnnMI355X(model_a.config, device="cpu").load_state_dict_speechbrain(R.weights("a"))
    bad._w.channels = 192
    assert fwd(st, ln, 2, 3333, w=bad._w) == 1 and L.ta_ecapa_workspace_bytes(C.byref(bad._w), 2, 21) == 0
    bad._w.channels, bad._w.blocks[1].dilation = 128, 5
    assert fwd(st, ln, 2, 3333, w=bad._w) == 1
    bad._w.blocks[1].dilation, bad._w.attn_channels = 3, 96
    assert fwd(st, ln, 2, 3333, w=bad._w) == 1


# ----------------------------------------------------------------------------- header, operator, dry run
def test_header_cites_what_the_entry_points_replace():
    text = open(_lib.HEADER).read()
    for cite in ("tiny_audio/diarization.py:457-517", "tiny_audio/diarization.py:490-502", "tiny_audio/diarization.py:484-488",
                 "#define TA_ECAPA_MAX_T 512", "#define TA_ECAPA_MIN_T 5", "#define TA_ECAPA_FEAT_STRIDE 128"):
        assert cite in text, cite
    protos = _lib.parse_header()
    for name, nargs in (("ta_ecapa_forward", 14), ("ta_ecapa_workspace_bytes", 3), ("ta_ecapa_fbank", 13), ("ta_ecapa_res2net", 17),
                        ("ta_ecapa_relu_bn", 10), ("ta_ecapa_se_residual", 17), ("ta_ecapa_se_ws_floats", 2), ("ta_ecapa_attn_act", 9),
                        ("ta_ecapa_asp_pool", 11)):
        assert name in protos and len(protos[name][1]) == nargs, name
    assert "ecapa.hip" in _lib.SOURCES and _lib.lib().ta_version() == 4
    assert (E.MIN_T, E.MAX_T, E.MAX_DILATION, E.MAX_CHANNELS, E.MAX_SE, E.MAX_ATTN, E.MAX_EMB) == (5, 512, 4, 1024, 256, 256, 1024)
    for name, v in (("MAX_DILATION", 4), ("MAX_CHANNELS", 1024), ("MAX_SE", 256), ("MAX_ATTN", 256), ("MAX_EMB", 1024), ("SCALE", 8), ("N_MELS", 80)):
        assert f"#define TA_ECAPA_{name} {v}" in text, name
    assert C.sizeof(_lib.EcapaBlock) == 17 * 8 and C.sizeof(_lib.EcapaWeights) == 16 + 8 * 8 + 3 * 17 * 8 + 15 * 8


def test_operator_is_registered_with_a_fake_kernel(model_a):
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "ecapa_embeddings" in torch_ops.OPERATORS
    s = str(torch.ops.ta355.ecapa_embeddings.default._schema)
    assert s.startswith("ta355::ecapa_embeddings(Tensor audio, SymInt[] starts, SymInt[] lengths, SymInt window_samples, SymInt handle) -> Tensor"), s
    h = torch_ops.register_module(model_a)
    with FakeTensorMode():
        e = torch.ops.ta355.ecapa_embeddings(torch.empty(50000), [0, 10, 20], [3333] * 3, 3333, h)
        assert e.shape == (3, 64) and e.dtype == torch.float32


def test_package_exports_the_new_names():
    import tiny_audio_amd
    assert tiny_audio_amd.EcapaConfig is E.EcapaConfig and tiny_audio_amd.EcapaTdnnMI355X is E.EcapaTdnnMI355X
    with pytest.raises(AttributeError):
        tiny_audio_amd.no_such_name


def test_dry_run_marshals_through_the_real_prototypes(model_a, dry):
    audio = np.zeros(50000, np.float32)
    dry.calls.clear()
    e = model_a.embed_windows(audio, [0, 100, 46000], [3333, 3333, 3000], 3333)
    assert dry.calls == ["ta_ecapa_forward"] and e.shape == (3, 64) and e.dtype == F32
    dry.calls.clear()
    e = model_a.encode_batch(torch.zeros(4, 12000))
    assert dry.calls == ["ta_ecapa_forward"] and e.shape == (4, 1, 64)
    assert model_a.encode_batch(np.zeros(640, np.float32)).shape == (1, 1, 64)
    dry.calls.clear()
    N, T, Cc = 3, 21, 128
    tabs = tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in E.fbank_tables())
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    feat, slab = ops.ecapa_fbank(torch.zeros(20000), i32([0, 5000, 9000]), i32([3333] * 3), 3333, tabs)
    assert feat.shape == (N, T, 80) and slab.shape == (N, T + 4, 128) and slab.dtype == BF16
    b = model_a._bufs
    y = torch.zeros(N, T, Cc, dtype=BF16)
    ops.ecapa_res2net(torch.zeros(N, T, Cc, dtype=BF16), b["blk0.bn1_s"], b["blk0.bn1_t"], b["blk0.res_w"], b["blk0.res_b"], b["blk0.res_s"],
                      b["blk0.res_t"], T, 16, 2, y)
    z = torch.zeros(N * T, Cc, dtype=BF16)
    assert ops.ecapa_relu_bn(z, b["bn0_s"], b["bn0_t"], N, T).shape == (N * T, Cc)
    out, sf, sb = ops.ecapa_relu_bn(torch.zeros(N * T, 3 * Cc, dtype=BF16), b["mfa_s"], b["mfa_t"], N, T, want_stats=True)
    assert sf.shape == (N, 6 * Cc) and sb.dtype == BF16
    cat = torch.zeros(N * T, 3 * Cc, dtype=BF16)
    ops.ecapa_se_residual(z, b["blk0.bn2_s"], b["blk0.bn2_t"], b["blk0.se_w1t"], b["blk0.se_b1"], b["blk0.se_w2t"], b["blk0.se_b2"], z, cat, 128, N, T)
    assert ops.ecapa_attn_act(torch.zeros(N * T, 64), torch.zeros(N, 64), b["att_s"], b["att_t"], N, T).dtype == BF16
    o, aw, p = ops.ecapa_asp_pool(torch.zeros(N * T, 3 * Cc), torch.zeros(N * T, 3 * Cc, dtype=BF16), b["aspbn_s"], b["aspbn_t"], N, T)
    assert o.shape == (N, 6 * Cc) and aw.shape == (N * T, 3 * Cc) and p.dtype == F32
    assert dry.calls == ["ta_ecapa_fbank", "ta_ecapa_res2net", "ta_ecapa_relu_bn", "ta_ecapa_relu_bn", "ta_ecapa_se_residual",
                         "ta_ecapa_attn_act", "ta_ecapa_asp_pool"]
