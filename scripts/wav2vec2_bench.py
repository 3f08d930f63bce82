"""wav2vec2 CTC acoustic model: device time of one ``Wav2Vec2CtcMI355X`` forward at the base-960h geometry, of its new kernels alone,
and of the same network in bf16 through PyTorch (transformers' ``Wav2Vec2ForCTC``, where transformers is importable).

    python scripts/wav2vec2_bench.py [--arch base|large-lv60] [--layers N] [--repeats 10] [--out FILE.json]

``--arch large-lv60``: the layer-norm / stable family at its true geometry (H 1024, 16 heads, ffn 4096, 24 layers, conv 512,
normalised input).  Its conv0 column is ta_w2v_conv0_ln_gelu (one launch); two more columns time the input normalisation alone and
the six LayerNorm + GELU passes behind conv layers 1 .. 6 alone (ta_layernorm_gelu_bf16 at each layer's slab rows).

Shapes: B = 32 clips of 10 s (499 frames each) and 1 clip of 30 s (1499 frames), random weights (timing does not depend on them).
  * model:      waveforms on the device -> emissions, ``_forward_impl`` (one ta_wav2vec2_forward + the two small length tables);
  * conv0:      ta_w2v_conv0_gn_gelu alone (statistics, merge, apply) at the same waveforms;
  * pos_conv:   ta_w2v_pos_conv alone at the model's row count; FLOPs = 2 * rows * H * (H / 16) * 128;
  * attention:  ``--layers`` launches of ta_attention_enc_fwd_varlen at the same rows (what the issue compares the positional conv with);
  * hf_bf16:    ``Wav2Vec2ForCTC(...).to(bfloat16)`` + log_softmax on the same device, eager attention, the batch as one padded call.
Every time is HIP events around ``--inner`` back-to-back calls after ``--warmup`` calls, median (min, max) of ``--repeats``.
Results: profiles/wav2vec2.md.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tiny_audio_amd import ops  # noqa: E402
from tiny_audio_amd import wav2vec2 as W  # noqa: E402


def time_events(fn, warmup, repeats, inner):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def hf_model(cfg):
    try:
        from transformers import Wav2Vec2Config, Wav2Vec2ForCTC
    except ImportError:
        return None
    c = Wav2Vec2Config(vocab_size=32, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                       num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                       conv_dim=(cfg.conv_dim,) * 7, feat_extract_norm=cfg.feat_extract_norm, conv_bias=cfg.conv_bias,
                       do_stable_layer_norm=cfg.do_stable_layer_norm, attn_implementation="eager")
    return Wav2Vec2ForCTC(c).eval().to(device="cuda", dtype=torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", choices=("base", "large-lv60"), default="base")
    ap.add_argument("--layers", type=int, default=None, help="default: 12 (base), 24 (large-lv60)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--no-hf", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    large = a.arch == "large-lv60"
    if a.layers is None:
        a.layers = 24 if large else 12
    if large:
        cfg = W.Wav2Vec2CtcConfig(hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_hidden_layers=a.layers,
                                  conv_dim=512, n_classes=32, feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True,
                                  normalize_input="hf")
    else:
        cfg = W.Wav2Vec2CtcConfig(num_hidden_layers=a.layers)
    m = W.Wav2Vec2CtcMI355X(cfg, device="cuda").random_init(0)
    hf = None if a.no_hf else hf_model(cfg)
    H, cg = cfg.hidden_size, cfg.hidden_size // 16
    res = dict(device=torch.cuda.get_device_name(0), arch=a.arch, layers=a.layers, warmup=a.warmup, repeats=a.repeats, inner=a.inner, rows=[])
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    t = lambda fn: time_events(fn, a.warmup, a.repeats, a.inner)
    for B, seconds in ((32, 10), (1, 30)):
        Ls = seconds * 16000
        g = torch.Generator().manual_seed(B)
        wav = (0.1 * torch.randn(B, Ls, generator=g)).cuda()
        lens = [Ls] * B
        T = W.frames_of(Ls)
        rows = B * T
        em = m._forward_impl(wav, lens)
        torch.cuda.synchronize()
        assert em.shape == (rows, cfg.n_classes) and bool(torch.isfinite(em).all())
        assert float((em.double().exp().sum(-1) - 1).abs().max()) < 1e-4
        row = dict(B=B, seconds=seconds, frames=T, rows=rows)
        row["model_ms"] = t(lambda: m._forward_impl(wav, lens))
        lens_dev = torch.tensor(lens, dtype=torch.int32, device="cuda")
        T0 = (Ls - 10) // 5 + 1
        c0 = torch.empty((B, T0, cfg.conv_dim), dtype=torch.bfloat16, device="cuda")
        bufs = m._bufs
        if large:
            row["conv0_ms"] = t(lambda: ops.w2v_conv0_ln_gelu(wav, lens_dev, bufs["conv0_w"], bufs["conv0_b"], bufs["conv0_ln_w"],
                                                              bufs["conv0_ln_b"], out=c0))
            wn = torch.empty_like(wav)
            row["input_norm_ms"] = t(lambda: ops.w2v_input_norm(wav, lens_dev, 1e-7, out=wn))
            Tl, n = [], Ls                                     # frames behind each conv layer
            for k, s_ in zip(W.CONV_KERNEL, W.CONV_STRIDE):
                n = (n - k) // s_ + 1
                Tl.append(n)
            slabs = [torch.randn(B * Tl[l], cfg.conv_dim, device="cuda").to(torch.bfloat16) for l in range(1, 7)]
            outs = [torch.empty_like(v) for v in slabs]

            def ln_gelu():
                for l in range(6):
                    ops.layernorm_gelu(slabs[l], bufs[f"conv{l + 1}_ln_w"], bufs[f"conv{l + 1}_ln_b"], out=outs[l])
            row["ln_gelu_six_ms"] = t(ln_gelu)
        else:
            row["conv0_ms"] = t(lambda: ops.w2v_conv0_gn_gelu(wav, lens_dev, bufs["conv0_w"], bufs["gn_w"], bufs["gn_b"], out=c0))
        cu = (torch.arange(B + 1, dtype=torch.int32) * T).cuda()
        x = torch.randn(rows, H, generator=g).to(torch.bfloat16).cuda()
        y = torch.empty_like(x)
        row["pos_conv_ms"] = t(lambda: ops.w2v_pos_conv(x, m._bufs["pos_w"], m._bufs["pos_b"], cu, T, out=y))
        row["pos_conv_tflops"] = 2.0 * rows * H * cg * 128 / (row["pos_conv_ms"]["median"] * 1e-3) / 1e12
        qkv = torch.randn(rows, 3 * H, generator=g).to(torch.bfloat16).cuda()
        ao = torch.empty((rows, H), dtype=torch.bfloat16, device="cuda")

        def attn():
            for _ in range(a.layers):
                ops.attention_enc_fwd_varlen(qkv, cu, cfg.num_attention_heads, T, out=ao)
        row["attention_all_layers_ms"] = t(attn)
        for k in ("conv0", "pos_conv", "attention_all_layers") + (("input_norm", "ln_gelu_six") if large else ()):
            row[k + "_share"] = row[k + "_ms"]["median"] / row["model_ms"]["median"]
        if hf is not None:
            wb = wav.to(torch.bfloat16)
            with torch.inference_mode():
                row["hf_bf16_ms"] = time_events(lambda: torch.log_softmax(hf(wb).logits.float(), -1), 2, max(3, a.repeats // 2), 1)
            row["speedup_vs_hf_bf16"] = row["hf_bf16_ms"]["median"] / row["model_ms"]["median"]
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
