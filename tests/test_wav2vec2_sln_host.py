"""Layer-norm / stable wav2vec2 family and the aligner's vocabularies, host side (no GPU): config fields and refusals, ``from_hf``,
weight packing and export, ``set_vocab``, the tokeniser's case rule, the aligner reading the model's dictionary and blank id (and
behaving as ever without one), the C ABI's argument checks, the struct against the header, the operator and its dry run."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests.golden import wav2vec2_recipe as RB
from tests.golden import wav2vec2_sln_recipe as R
from tiny_audio_amd import _lib, alignment, ops, torch_ops
from tiny_audio_amd import wav2vec2 as W
from tiny_audio_amd.alignment import LABELS, ForcedAligner


@pytest.fixture()
def dry():
    _lib.DRY_RUN = True
    try:
        yield _lib.lib()
    finally:
        _lib.DRY_RUN = False
        _lib._LIB = None


def _config(geom="c", n_classes=32, **kw):
    return W.Wav2Vec2CtcConfig(**R.GEOMS[geom], n_classes=n_classes, **{**R.FAMILY, **kw})


def _model(geom="c", n_classes=32, **kw):
    return W.Wav2Vec2CtcMI355X(_config(geom, n_classes, **kw), device="cpu").load_state_dict_hf(R.weights(geom))


# 40 classes, lower-case letters, blank NOT at 0, a delimiter that is not "|": what an XLSR fine-tune's vocab.json looks like
VOCAB = {t: i for i, t in enumerate(["<s>", "</s>", "<unk>", "<pad>", " "] + list("abcdefghijklmnopqrstuvwxyz") + list("äöüß'") + ["é", "ñ", "ç", "-"])}


# ----------------------------------------------------------------------------- config
def test_defaults_are_still_the_base_model():
    c = W.Wav2Vec2CtcConfig()
    assert (c.feat_extract_norm, c.conv_bias, c.do_stable_layer_norm, c.normalize_input, c.sln) == ("group", False, False, None, False)
    c = _config(normalize_input="hf")
    assert c.sln and c.conv_bias and c.do_stable_layer_norm and W.INPUT_NORM_EPS == {"hf": 1e-7, "torchaudio": 1e-5}


def test_config_refuses_by_name_what_is_not_built():
    ok = dict(R.GEOMS["c"], **R.FAMILY)
    for bad, match in ((dict(do_stable_layer_norm=False), "mixed configuration"),
                       (dict(feat_extract_norm="group", conv_bias=False), "mixed configuration"),
                       (dict(conv_bias=False), "conv_bias=False is not built"),
                       (dict(feat_extract_norm="batch"), "feat_extract_norm must be"),
                       (dict(normalize_input="fairseq"), "normalize_input must be"),
                       (dict(hidden_size=1280, num_attention_heads=16), "head_dim 64"),           # XLS-R 1B: head_dim 80
                       (dict(n_classes=65), "above 64 classes"),
                       (dict(conv_dim=192), "conv_dim must be one of")):
        with pytest.raises(ValueError, match=match):
            W.Wav2Vec2CtcConfig(**{**ok, **bad})
    with pytest.raises(ValueError, match='built for feat_extract_norm="layer"'):
        W.Wav2Vec2CtcConfig(normalize_input="hf")


def test_from_hf():
    d = R.hf_config_dict("d")
    c = W.Wav2Vec2CtcConfig.from_hf(d)
    assert (c.hidden_size, c.num_attention_heads, c.intermediate_size, c.num_hidden_layers, c.conv_dim, c.n_classes) == (1024, 16, 4096, 2, 512, 32)
    assert c.sln and c.normalize_input == "hf" and c.layer_norm_eps == 1e-5
    assert W.Wav2Vec2CtcConfig.from_hf(d, n_classes=40, normalize_input="torchaudio").normalize_input == "torchaudio"
    assert W.Wav2Vec2CtcConfig.from_hf(d, normalize_input=None).normalize_input is None
    base = W.Wav2Vec2CtcConfig.from_hf(dict(vocab_size=32))                    # transformers' own defaults: wav2vec2-base
    assert base == W.Wav2Vec2CtcConfig(n_classes=32) and not base.sln
    from transformers import Wav2Vec2Config
    assert W.Wav2Vec2CtcConfig.from_hf(Wav2Vec2Config(**d).to_dict()) == c
    for bad, match in ((dict(adapter_attn_dim=16), "adapter_attn_dim"), (dict(hidden_size=1280), "head_dim 64"),
                       (dict(vocab_size=154), "above 64 classes"), (dict(do_stable_layer_norm=False), "mixed configuration"),
                       (dict(conv_dim=(512,) * 6 + (256,)), "one width"), (dict(conv_stride=(5, 2, 2, 2, 2, 2, 1)), "conv_kernel / conv_stride"),
                       (dict(num_conv_pos_embedding_groups=8), "16 groups"), (dict(add_adapter=True), "add_adapter")):
        with pytest.raises(ValueError, match=match):
            W.Wav2Vec2CtcConfig.from_hf({**d, **bad})


# ----------------------------------------------------------------------------- packing
def test_packed_images_and_struct_fields():
    sd = R.weights("c")
    m = _model("c", normalize_input="torchaudio")
    b = m._bufs
    fe = "wav2vec2.feature_extractor.conv_layers."
    assert "gn_w" not in b and b["conv0_w"].shape == (128, 10)
    for i in range(7):
        for f, k in (("b", "conv.bias"), ("ln_w", "layer_norm.weight"), ("ln_b", "layer_norm.bias")):
            assert torch.equal(b[f"conv{i}_{f}"], torch.from_numpy(sd[fe + f"{i}.{k}"])) and b[f"conv{i}_{f}"].dtype == torch.float32
    assert torch.equal(b["conv3_w"][5, 2 * 128 + 7], torch.from_numpy(sd[fe + "3.conv.weight"])[5, 7, 2].bfloat16())
    w = m._w
    assert isinstance(w, _lib.Wav2Vec2SlnWeights) and abs(w.input_norm_eps - 1e-5) < 1e-12 and w.conv_dim == 128 and w.n_classes == 32
    assert [w.conv_b[i] for i in range(7)] == [b[f"conv{i}_b"].data_ptr() for i in range(7)]
    assert [w.conv_ln_w[i] for i in range(7)] == [b[f"conv{i}_ln_w"].data_ptr() for i in range(7)]
    assert w.conv_w[5] == b["conv6_w"].data_ptr() and w.enc_ln_b == b["enc_ln_b"].data_ptr() and w.head_b == b["head_b"].data_ptr()
    m.res_f32 = True
    assert w.res_f32 == 1
    assert isinstance(W.Wav2Vec2CtcMI355X(W.Wav2Vec2CtcConfig(**RB.GEOMS["a"], n_classes=32), device="cpu")
                      .load_state_dict_hf(RB.weights("a"))._w, _lib.Wav2Vec2Weights)
    missing = dict(sd)
    del missing[fe + "4.conv.bias"]
    with pytest.raises(ValueError, match="needs conv_layers.4.conv.bias"):
        W.pack_state_dict(missing, _config())
    with pytest.raises(ValueError, match="conv_bias=True checkpoints are not supported"):
        W.pack_state_dict(sd, W.Wav2Vec2CtcConfig(**R.GEOMS["c"], n_classes=32))


def test_export_round_trip():
    m = _model("c")
    sd = m.export_state_dict_hf()
    for k in R.weights("c"):
        if "pos_conv_embed.conv.parametrizations" not in k:
            assert k in sd, k
    m2 = W.Wav2Vec2CtcMI355X(m.config, device="cpu").load_state_dict_hf(sd)
    assert m._bufs.keys() == m2._bufs.keys()
    for k in m._bufs:
        if k in ("pos_w", "pos_w_plain") or k.endswith("wqkv_fa"):         # refolded / rescaled from a bf16 value: one more rounding
            np.testing.assert_allclose(m2._bufs[k].float().numpy(), m._bufs[k].float().numpy(), rtol=2 ** -7, atol=0)
        else:
            assert torch.equal(m._bufs[k], m2._bufs[k]), k


def _to_torchaudio(sd):
    out = {}
    for k, v in sd.items():
        if k.startswith("lm_head."):
            out["aux." + k[len("lm_head."):]] = v
            continue
        k = k[len("wav2vec2."):]
        k = k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v")
        if k.startswith("feature_projection."):
            k = "encoder." + k
        elif k.startswith("encoder."):
            k = "encoder.transformer." + k[len("encoder."):]
        out[k] = v
    return out


def test_torchaudio_names_of_the_family_round_trip():
    sd = R.weights("c")
    ta = _to_torchaudio(sd)
    for name in ("feature_extractor.conv_layers.5.layer_norm.weight", "feature_extractor.conv_layers.0.conv.bias",
                 "encoder.transformer.layer_norm.bias", "encoder.transformer.layers.1.final_layer_norm.weight", "aux.bias"):
        assert name in ta, name
    a = W.pack_state_dict(sd, _config())
    b = W.Wav2Vec2CtcMI355X(_config(), device="cpu").load_state_dict_torchaudio(ta)._bufs
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_random_init_of_the_family_is_seeded_and_leaves_the_base_draws_alone():
    a, b, c = (W.Wav2Vec2CtcMI355X(_config(n_classes=29), device="cpu").random_init(s) for s in (0, 0, 1))
    assert torch.equal(a._bufs["conv4_b"], b._bufs["conv4_b"]) and not torch.equal(a._bufs["conv4_b"], c._bufs["conv4_b"])
    assert a._bufs["conv0_b"].abs().max() > 0 and (a._bufs["conv6_ln_w"] - 1).abs().max() > 0
    base = W.Wav2Vec2CtcConfig(**R.GEOMS["c"], n_classes=29)
    sb, ss = W.random_state_dict(base, 0), W.random_state_dict(_config(n_classes=29), 0)
    k = "wav2vec2.feature_extractor.conv_layers.6.conv.weight"                 # drawn before the family's extras in both
    assert torch.equal(sb[k], ss[k]) and set(ss) - set(sb) and not set(sb) - set(ss)


# ----------------------------------------------------------------------------- vocabulary
def test_set_vocab():
    m = W.Wav2Vec2CtcMI355X(_config(n_classes=40), device="cpu")
    assert m.dictionary is None and m.labels is None and m.blank_id == 0
    assert m.set_vocab(VOCAB, blank_token="<pad>", word_delimiter=" ") is m
    assert m.blank_id == 3 and m.labels[3] == "<pad>" and m.labels[5] == "a" and len(m.labels) == 40
    assert m.dictionary["a"] == 5 and m.dictionary["|"] == 4 and m.dictionary[" "] == 4 and m.dictionary["ß"] == VOCAB["ß"]
    with pytest.raises(ValueError, match="blank_token"):
        m.set_vocab(VOCAB, blank_token="[PAD]", word_delimiter=" ")
    with pytest.raises(ValueError, match="word_delimiter"):
        m.set_vocab(VOCAB)                                                      # "|" is not in this vocabulary
    with pytest.raises(ValueError, match="0 .. 39"):
        m.set_vocab({k: v for k, v in VOCAB.items() if v < 39}, word_delimiter=" ")
    with pytest.raises(ValueError, match="0 .. 39"):
        m.set_vocab({**VOCAB, "a": 6}, word_delimiter=" ")                      # id 6 twice, id 5 missing


def test_tokeniser_case_rule():
    d = dict(VOCAB)
    d["|"] = d[" "]
    tok = lambda t, dic=d: alignment._tokenize(t, dic, True)
    assert tok("ab c") == [5, 6, 4, 7]
    assert tok("AB C") == [5, 6, 4, 7]                                          # not as written, not upper: lower-cased
    assert tok("Straße ÄÖ") == [d[c] for c in "straße"] + [4] + [d["ä"], d["ö"]]
    assert tok("a1b!") == [5, 6]                                                # absent characters are dropped
    up = {c: i for i, c in enumerate(LABELS)}
    assert alignment._tokenize("it's", up, True) == alignment._tokenize("it's", up) == [up[c] for c in "IT'S"]      # upper-cased
    mixed = {"<pad>": 0, "|": 1, "a": 2, "A": 3}
    assert alignment._tokenize("aA a", mixed, True) == [2, 3, 1, 2]            # as written wins over both cases
    # without a vocabulary the old rule, whole-text upper-casing, is what runs: 'ß' becomes 'SS' there and two tokens
    assert alignment._tokenize("ß", up) == [up["S"], up["S"]] and alignment._tokenize("ß", up, True) == []


def _capture_launch(monkeypatch):
    seen = {}

    def fake(em, Ts, tokens, blank_id, want_trellis=False):
        seen.update(Ts=list(Ts), tokens=[list(t) for t in tokens], blank_id=blank_id, classes=em.shape[1])
        return [[min(j, Ts[n] - 1) for j in range(len(tk))] for n, tk in enumerate(tokens)], [0.0] * len(Ts), [0] * len(Ts), None
    monkeypatch.setattr(alignment, "_launch_flat", fake)
    return seen


def test_aligner_uses_the_models_dictionary_and_blank_id(monkeypatch, dry):
    sd = R.weights("c")
    g = np.random.default_rng(0)
    sd["lm_head.weight"], sd["lm_head.bias"] = g.standard_normal((40, 256)).astype(np.float32), g.standard_normal(40).astype(np.float32)
    m = W.Wav2Vec2CtcMI355X(_config(n_classes=40, normalize_input="hf"), device="cpu").load_state_dict_hf(sd)
    m.set_vocab(VOCAB, word_delimiter=" ")
    seen = _capture_launch(monkeypatch)
    waves = R.waves()
    out = ForcedAligner.align_audio_batch(waves, ["Grüße dich", "no"], m)
    want = [[VOCAB[c] for c in "grüße"] + [4] + [VOCAB[c] for c in "dich"], [VOCAB["n"], VOCAB["o"]]]
    assert seen["tokens"] == want and seen["blank_id"] == 3 and seen["classes"] == 40 and seen["Ts"] == [25, 140]
    assert [w["word"] for w in out[0]] == ["Grüße", "dich"] and [w["word"] for w in out[1]] == ["no"]
    ForcedAligner.align_audio_batch(waves, ["a", "b"], m, blank_id=7)          # an explicit blank id still wins
    assert seen["blank_id"] == 7
    assert ForcedAligner.align(waves[0], "Grüße dich", acoustic_model=m) == out[0]
    # the long form: tokens counted and aligned against the same dictionary, blank id passed down
    long_seen = {}

    def fake_long(em, tokens, blank_id, col_block=0, frame_block=0):
        long_seen.update(tokens=[list(t) for t in tokens], blank_id=blank_id)
        return [list(range(len(tk))) for tk in tokens], [0.0], [0]
    monkeypatch.setattr(alignment, "_launch_long", fake_long)
    words = ForcedAligner.align_long(waves[1], "Grüße dich", acoustic_model=m)
    assert long_seen["tokens"] == [want[0]] and long_seen["blank_id"] == 3 and [w["word"] for w in words] == ["Grüße", "dich"]
    ForcedAligner.align_long_batch([torch.zeros(30, 40)], ["ab"], acoustic_model=m)
    assert long_seen["tokens"] == [[5, 6]] and long_seen["blank_id"] == 3
    # _language stays accepted and unused
    assert ForcedAligner.align(waves[0], "Grüße dich", 16000, "deu", acoustic_model=m) == out[0]


def test_aligner_without_a_vocabulary_is_as_before(monkeypatch, dry):
    """A model that carries no vocabulary (the base model, or a family model before ``set_vocab``): LABELS, whole-text upper-casing,
    blank 0 -- in align_audio_batch, align_long and align_long_batch, with and without the model argument."""
    up = {c: i for i, c in enumerate(LABELS)}
    old = lambda t: [up[c] if c != " " else up["|"] for c in t.upper() if c in up or c == " "]
    seen = _capture_launch(monkeypatch)
    base = W.Wav2Vec2CtcMI355X(W.Wav2Vec2CtcConfig(**RB.GEOMS["a"], n_classes=29), device="cpu").load_state_dict_hf(RB.weights("a"), labels="torchaudio")
    fam = W.Wav2Vec2CtcMI355X(_config(n_classes=29), device="cpu").random_init(0)
    for m in (base, fam):
        out = ForcedAligner.align_audio_batch(R.waves(), ["Hello wörld", "Straße"], m)
        assert seen["tokens"] == [old("Hello wörld"), old("Straße")] and seen["blank_id"] == 0
        assert [w["word"] for w in out[0]] == ["Hello", "wörld"]
    assert old("Straße") == [up[c] for c in "STRASSE"]
    long_seen = {}

    def fake_long(em, tokens, blank_id, col_block=0, frame_block=0):
        long_seen.update(tokens=[list(t) for t in tokens], blank_id=blank_id)
        return [list(range(len(tk))) for tk in tokens], [0.0], [0]
    monkeypatch.setattr(alignment, "_launch_long", fake_long)
    ForcedAligner.align_long_batch([torch.zeros(30, 29)], ["Hi you"])
    assert long_seen == dict(tokens=[old("Hi you")], blank_id=0)
    ForcedAligner.align_long(R.waves()[0], "Hi you", acoustic_model=base)
    assert long_seen == dict(tokens=[old("Hi you")], blank_id=0)


# ----------------------------------------------------------------------------- C ABI
def _struct_fields_from_header(name):
    """[(field, ctypes type)] of a ``typedef struct { ... } name;`` in the header: int / float scalars, pointers (``const T* a, *b``,
    ``const T *a, *b``) and arrays of pointers (``const T* a[7]``)."""
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", text).group(1)
    out = []
    for decl in (" ".join(d.split()) for d in body.split(";")):
        if not decl:
            continue
        ty, rest = re.match(r"(?:const )?(\w+)\s*(.*)", decl).groups()
        for item in rest.split(","):
            item = item.strip()
            pointer, ident = "*" in item, item.replace("*", "").strip()
            base = (C.POINTER(_lib.EncLayer) if ty == "ta_enc_layer" else C.c_void_p) if pointer else {"int": C.c_int, "float": C.c_float}[ty]
            am = re.fullmatch(r"(\w+)\[(\d+)\]", ident)
            out.append((am.group(1), base * int(am.group(2))) if am else (ident, base))
    return out


def test_struct_mirrors_the_header():
    want = _struct_fields_from_header("ta_wav2vec2_sln_weights")
    got = list(_lib.Wav2Vec2SlnWeights._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, a), (_, b) in zip(got, want):
        assert a is b or (issubclass(a, C.Array) and issubclass(b, C.Array) and a._type_ is b._type_ and a._length_ == b._length_) \
            or (a._type_ is b._type_), (n, a, b)
    # the parser is right about a struct that has been bound for long
    assert [n for n, _ in _struct_fields_from_header("ta_wav2vec2_weights")] == [n for n, _ in _lib.Wav2Vec2Weights._fields_]
    assert [n for n, _ in _lib.Wav2Vec2Weights._fields_][:8] == ["hidden", "ffn", "n_layers", "heads", "conv_dim", "n_classes", "ln_eps", "conv0_w"]


def test_header_declares_and_cites_the_new_entry_points():
    text = open(_lib.HEADER).read()
    for cite in ("Wav2Vec2LayerNormConvLayer", "Wav2Vec2EncoderStableLayerNorm", "Wav2Vec2EncoderLayerStableLayerNorm",
                 "zero_mean_unit_var_norm", "tests/wav2vec2_sln_ref.py"):
        assert cite in text, cite
    protos = _lib.parse_header()
    for name, nargs in (("ta_wav2vec2_sln_forward", 11), ("ta_wav2vec2_sln_workspace_bytes", 4), ("ta_wav2vec2_sln_ws_offsets", 6),
                        ("ta_w2v_conv0_ln_gelu", 13), ("ta_w2v_input_norm", 9), ("ta_w2v_input_norm_ws_bytes", 2),
                        ("ta_layernorm_gelu_bf16", 8)):
        assert name in protos and len(protos[name][1]) == nargs, name
    assert len(protos["ta_wav2vec2_forward"][1]) == 11 and len(protos["ta_w2v_conv0_gn_gelu"][1]) == 14       # untouched


def test_c_abi_refuses_outside_the_envelope():
    """Host-side argument checks return TA_ERR_ARG before anything is launched, so they run without a GPU."""
    L = _lib.lib()
    one, two = C.c_void_p(64), C.c_void_p(128)                                 # never dereferenced: every call below is refused
    conv0 = lambda Ls=8000, Cd=128, rpb=1599, w=one, B=1: L.ta_w2v_conv0_ln_gelu(one, one, B, Ls, w, one, one, one, Cd, 1e-5, one, rpb, None)
    assert conv0(Ls=9) == 1 and conv0(rpb=1598) == 1 and conv0(Cd=192) == 1 and conv0(Cd=1024) == 1 and conv0(w=None) == 1 and conv0(B=0) == 0
    norm = lambda Ls=8000, eps=1e-7, ws=1 << 20, B=1: L.ta_w2v_input_norm(one, one, B, Ls, eps, two, one, ws, None)
    assert norm(Ls=0) == 1 and norm(eps=0.0) == 1 and norm(ws=L.ta_w2v_input_norm_ws_bytes(1, 8000) - 1) == 1 and norm(B=0) == 0
    assert L.ta_w2v_input_norm_ws_bytes(2, 480000) >= 2 * 118 * 2 * 4
    assert L.ta_layernorm_gelu_bf16(one, one, one, one, 4, 512, 1e-5, None) == 1                           # in place
    assert L.ta_layernorm_gelu_bf16(one, one, one, two, 4, 510, 1e-5, None) == 1                           # H % 4
    assert L.ta_layernorm_gelu_bf16(one, None, one, two, 4, 512, 1e-5, None) == 1 and L.ta_layernorm_gelu_bf16(one, one, one, two, 0, 512, 1e-5, None) == 0
    m = _model("c")
    fwd = lambda lens, B, Ls, ws_bytes=1 << 40, w=None: L.ta_wav2vec2_sln_forward(C.byref(w if w is not None else m._w), one,
                                                                                  lens.ctypes.data_as(C.c_void_p), one, one, B, Ls, one, one, ws_bytes, None)
    ok = np.asarray([8000, 4000], np.int32)
    assert fwd(np.asarray([8000, 399], np.int32), 2, 8000) == 1 and fwd(np.asarray([8000, 8001], np.int32), 2, 8000) == 1
    need = L.ta_wav2vec2_sln_workspace_bytes(C.byref(m._w), 2, 8000, 24 + 12)
    assert need > 2 * 1599 * 128 * 2 + 2 * 8000 * 4 and fwd(ok, 2, 8000, ws_bytes=need - 1) == 1 and fwd(ok, 0, 8000) == 0
    for field, value in (("n_classes", 65), ("heads", 3), ("conv_dim", 192), ("input_norm_eps", -1.0)):
        bad = _model("c")
        setattr(bad._w, field, value)
        assert fwd(ok, 2, 8000, w=bad._w) == 1, field
    bad = _model("c")
    bad._w.conv_ln_b[6] = None
    assert fwd(ok, 2, 8000, w=bad._w) == 1
    f, s = C.c_long(-1), C.c_long(-1)
    assert L.ta_wav2vec2_sln_ws_offsets(C.byref(m._w), 2, 8000, 36, C.byref(f), C.byref(s)) == 0 and 0 < f.value < s.value < need
    assert f.value % 256 == 0 and s.value % 256 == 0


# ----------------------------------------------------------------------------- operator, dry run
def test_operator_is_registered_with_a_fake_kernel_and_the_old_schema_stays():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "wav2vec2_sln_emissions" in torch_ops.OPERATORS and "wav2vec2_emissions" in torch_ops.OPERATORS
    s = str(torch.ops.ta355.wav2vec2_sln_emissions.default._schema)
    assert s.startswith("ta355::wav2vec2_sln_emissions(Tensor waveforms, SymInt[] lengths, bool normalized, SymInt handle) -> Tensor"), s
    s = str(torch.ops.ta355.wav2vec2_emissions.default._schema)
    assert s.startswith("ta355::wav2vec2_emissions(Tensor waveforms, SymInt[] lengths, SymInt handle) -> Tensor"), s
    m = _model("c")                                                            # (the registry holds modules weakly)
    h = torch_ops.register_module(m)
    with FakeTensorMode():
        e = torch.ops.ta355.wav2vec2_sln_emissions(torch.empty(3, 43200), [8000, 24000, 43200], False, h)
        assert e.shape == (24 + 74 + 134, 32) and e.dtype == torch.float32


def test_dry_run_marshals_through_the_real_prototypes(dry):
    m = _model("c", normalize_input="hf")
    waves = R.waves()
    dry.calls.clear()
    em, frames = m(waves)
    assert dry.calls == ["ta_wav2vec2_sln_forward"] and frames == [25, 140] and em.shape == (165, 32) and em.dtype == torch.float32
    assert abs(m._w.input_norm_eps - 1e-7) < 1e-12
    m(waves, normalized=True)
    assert m._w.input_norm_eps == 0.0
    # one window: forward itself; three windows: the whole recording's statistics once, then pre-normalised windows
    dry.calls.clear()
    one = m.emissions_long(waves[1], window_s=30.0)
    assert dry.calls == ["ta_wav2vec2_sln_forward"] and one.shape == (140, 32)
    dry.calls.clear()
    three = m.emissions_long(waves[1], window_s=1.0, context_s=0.2, batch_windows=2)
    assert dry.calls == ["ta_w2v_input_norm", "ta_wav2vec2_sln_forward", "ta_wav2vec2_sln_forward"] and three.shape == (140, 32)
    assert m._w.input_norm_eps == 0.0
    raw = _model("c")                                                          # no normalisation: no statistics pass
    dry.calls.clear()
    raw.emissions_long(waves[1], window_s=1.0, context_s=0.2)
    assert dry.calls == ["ta_wav2vec2_sln_forward"]
    assert m.state_of_last_call("feat").shape[1] == 128 and m.state_of_last_call("stream").shape[1] == 256
    # the primitive wrappers
    dry.calls.clear()
    b = m._bufs
    y = ops.w2v_conv0_ln_gelu(torch.zeros(2, 800), torch.tensor([800, 400], dtype=torch.int32), b["conv0_w"], b["conv0_b"], b["conv0_ln_w"], b["conv0_ln_b"])
    assert y.shape == (2, 159, 128) and y.dtype == torch.bfloat16
    assert ops.w2v_input_norm(torch.zeros(2, 800), torch.tensor([800, 400], dtype=torch.int32), 1e-7).shape == (2, 800)
    assert ops.layernorm_gelu(torch.zeros(9, 128, dtype=torch.bfloat16), b["conv1_ln_w"], b["conv1_ln_b"]).shape == (9, 128)
    assert dry.calls == ["ta_w2v_conv0_ln_gelu", "ta_w2v_input_norm", "ta_layernorm_gelu_bf16"]
    # the base model still goes through its own entry point and operator
    base = W.Wav2Vec2CtcMI355X(W.Wav2Vec2CtcConfig(**RB.GEOMS["a"], n_classes=32), device="cpu").load_state_dict_hf(RB.weights("a"))
    dry.calls.clear()
    base(waves)
    assert dry.calls == ["ta_wav2vec2_forward"]
