"""Device-event timing of the Whisper audio tower next to the GLM-ASR tower at the same shapes (one process, one GPU).

    python scripts/whisper_encoder_bench.py [--batch 32] [--iters 20] [--warmup 5] [--out profiles/whisper_encoder.json]

Rows: the Whisper tower at large-v3 geometry (1280 / 20 / 5120 / 32 layers / 128 mel) and the GLM-ASR tower (same widths: the same GEMM
shapes and attention, rotary epilogue instead of the position add) at B x 3000 frames, both residual-stream modes, timed in ALTERNATION
so that drift of the box hits all of them alike; whisper-small geometry (768 / 12 / 3072 / 12 / 80 mel); and the log-mel front end at
80 and 128 bins on B clips of 30 s.  Times are per forward, from hipEvent pairs around each call; "spread" is (max - min) / median of
the timed iterations of one row.  There is no fallback: without a GPU the script fails.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tiny_audio_amd.asr_config import EncoderConfig, WhisperEncoderConfig  # noqa: E402
from tiny_audio_amd.asr_processing import LogMelFeatureExtractor  # noqa: E402
from tiny_audio_amd.encoder import GlmAsrEncoderMI355X  # noqa: E402
from tiny_audio_amd.whisper_encoder import WhisperEncoderMI355X  # noqa: E402

T = 3000


def timed(fns, iters, warmup):
    """fns: {name: callable}; the callables run round-robin -> {name: [ms per call]}."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); f(); b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return out


def row(name, ms):
    ms = np.asarray(ms)
    return dict(name=name, median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()),
                spread=float((ms.max() - ms.min()) / np.median(ms)), n=int(ms.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "whisper_encoder_bench needs a GPU"
    dev, B = "cuda", a.batch
    rows = []
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    x128 = torch.randn(B, 128, T, device=dev, generator=gen) * 0.6
    wh = WhisperEncoderMI355X(WhisperEncoderConfig(d_model=1280, encoder_attention_heads=20, encoder_ffn_dim=5120,
                                                   encoder_layers=a.layers, num_mel_bins=128), dev).random_init(0)
    glm = GlmAsrEncoderMI355X(EncoderConfig(num_hidden_layers=a.layers), dev).random_init(0)

    def run(enc, f32):
        def f():
            enc.res_f32 = f32
            enc._forward_impl(x128)
        return f
    t = timed({"whisper large-v3 bf16 stream": run(wh, False), "glm-asr bf16 stream": run(glm, False),
               "whisper large-v3 fp32 stream": run(wh, True), "glm-asr fp32 stream": run(glm, True)}, a.iters, a.warmup)
    rows += [row(f"{k}, B={B}, T={T}, {a.layers} layers", v) for k, v in t.items()]
    del wh, glm
    torch.cuda.empty_cache()
    x80 = torch.randn(B, 80, T, device=dev, generator=gen) * 0.6
    sm = WhisperEncoderMI355X(WhisperEncoderConfig(d_model=768, encoder_attention_heads=12, encoder_ffn_dim=3072, encoder_layers=12,
                                                   num_mel_bins=80), dev).random_init(0)
    t = timed({"whisper-small bf16 stream": lambda: sm._forward_impl(x80)}, a.iters, a.warmup)
    rows += [row(f"{k}, B={B}, T={T}, 12 layers", v) for k, v in t.items()]
    wav = torch.randn(B, 480000, device=dev, generator=gen) * 0.1
    lens = torch.full((B,), 480000, device=dev, dtype=torch.int64)
    fe80, fe128 = LogMelFeatureExtractor(80, dev), LogMelFeatureExtractor(128, dev)
    t = timed({"log-mel 80 bins": lambda: fe80._extract(wav, lens), "log-mel 128 bins": lambda: fe128._extract(wav, lens)}, a.iters, a.warmup)
    for k, v in t.items():
        r = row(f"{k}, {B} clips of 30 s", v)
        r["us_per_clip"] = 1000.0 * r["median_ms"] / B
        rows.append(r)
    print("| row | median ms | min | max | spread |\n|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['name']} | {r['median_ms']:.3f} | {r['min_ms']:.3f} | {r['max_ms']:.3f} | {100 * r['spread']:.1f} % |")
    print(json.dumps({"rows": rows}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
