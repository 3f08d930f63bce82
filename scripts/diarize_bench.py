"""Speaker-embedding hot path of diarization: device time of ``EcapaTdnnMI355X.embed_windows`` at the checkpoint's geometry, of its
kernels alone, and of the same network in bf16 through PyTorch on the same device, batched and one window per call.

    python scripts/diarize_bench.py [--windows 4000] [--per-call-windows 200] [--repeats 7] [--out FILE.json]

Workload: ``--windows`` windows of 0.75 s (12 000 samples, 76 frames) every 0.15 s of one audio buffer -- ten minutes of speech at the
reference's 80 % overlap -- random weights (timing does not depend on them).
  * device:     audio on the device -> embeddings, ``_embed_impl`` (one ta_ecapa_forward, chunks of ``--chunk`` windows);
  * kernels at one chunk's shape, alone: the filter bank, the Res2Net chain (FLOPs = 2 * rows * 7 * w * 3w), the C x C and 3C x 3C
    GEMMs (the in-situ GEMM rate the Res2Net kernel is compared with), SE + residual, ReLU + BatchNorm + statistics, the pooling;
  * torch_bf16: the composition of torch modules the fixtures are made with (tests/golden/ecapa_recipe.torch_model) in bfloat16 on
    the same device behind torch.stft features, windows batched ``--torch-batch`` at a time;
  * per_call:   the same modules, one window per call -- the reference's calling pattern (tiny_audio/diarization.py:490-502) -- timed
    on ``--per-call-windows`` windows only and scaled to ``--windows``.
Every time is HIP events around ``--inner`` back-to-back calls after ``--warmup`` calls, median (min, max) of ``--repeats``.
Results: profiles/diarization.md.
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

from tiny_audio_amd import ecapa as E  # noqa: E402
from tiny_audio_amd import ops  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32


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


def torch_legs(sd, audio, starts, L, batch, per_call, warmup, repeats):
    from tests import ecapa_ref as REF
    from tests.golden import ecapa_recipe as R
    m = R.torch_model("full", {k: v.numpy() for k, v in sd.items()}).to(device="cuda", dtype=BF16)
    win = torch.from_numpy(REF.hamming_window()).float().cuda()
    mel = torch.from_numpy(REF.mel_filterbank()).float().cuda()
    idx = torch.arange(L, device="cuda")[None, :]

    def embed(st):
        x = audio[torch.as_tensor(st, device="cuda")[:, None] + idx]                                  # [n, L]
        spec = torch.stft(x, 400, hop_length=160, win_length=400, window=win, center=True, pad_mode="constant", return_complex=True)
        db = 10.0 * torch.log10(torch.clamp((spec.real ** 2 + spec.imag ** 2).transpose(1, 2) @ mel, min=1e-10))
        db = torch.maximum(db, db.amax((1, 2), keepdim=True) - 80.0)
        return m((db - db.mean(1, keepdim=True)).transpose(1, 2).to(BF16))["emb"]

    def batched():
        return torch.cat([embed(starts[i:i + batch]) for i in range(0, len(starts), batch)])

    def one_by_one():
        return [embed(starts[i:i + 1]) for i in range(per_call)]

    with torch.inference_mode():
        e = batched()
        torch.cuda.synchronize()
        return e.float(), time_events(batched, warmup, repeats, 1), time_events(one_by_one, 1, max(3, repeats // 2), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4000)
    ap.add_argument("--chunk", type=int, default=E.DEFAULT_CHUNK)
    ap.add_argument("--torch-batch", type=int, default=256)
    ap.add_argument("--per-call-windows", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = E.EcapaConfig()
    sd = E.random_state_dict(cfg, 0)
    m = E.EcapaTdnnMI355X(cfg, device="cuda").load_state_dict_speechbrain(sd)
    m.chunk_windows = a.chunk
    L, step = 12000, 2400
    T, C, w = E.frames_of(L), cfg.channels, cfg.width
    N = a.windows
    g = torch.Generator().manual_seed(0)
    audio = (0.1 * torch.randn((N - 1) * step + L, generator=g)).cuda()
    starts, lens = [i * step for i in range(N)], [L] * N
    res = dict(device=torch.cuda.get_device_name(0), windows=N, chunk=a.chunk, frames=T, warmup=a.warmup, repeats=a.repeats, inner=a.inner,
               gflop_per_window=None)
    t = lambda fn: time_events(fn, a.warmup, a.repeats, a.inner)
    emb = m._embed_impl(audio, starts, lens, L)
    torch.cuda.synchronize()
    assert emb.shape == (N, cfg.lin_neurons) and bool(torch.isfinite(emb).all())
    res["device_ms"] = t(lambda: m._embed_impl(audio, starts, lens, L))
    A, D = cfg.attention_channels, cfg.lin_neurons
    flop = 2.0 * T * (C * 640 + 3 * (2 * C * C + 7 * w * 3 * w) + 9 * C * C + 3 * C * A * 2) + 2.0 * (6 * C * A + 6 * C * D)
    res["gflop_per_window"] = flop / 1e9
    res["device_tflops"] = flop * N / (res["device_ms"]["median"] * 1e-3) / 1e12
    res["workspace_mb"] = m._ws.numel() / 2 ** 20

    # the kernels alone at one chunk's shape
    nw = min(a.chunk, N)
    R = nw * T
    b = m._bufs
    st_dev, ln_dev = torch.tensor(starts[:nw], dtype=torch.int32, device="cuda"), torch.tensor(lens[:nw], dtype=torch.int32, device="cuda")
    tabs = (b["fb_window"], b["fb_twiddle"], b["fb_mel"], b["fb_mel_range"])
    k = {}
    k["fbank_ms"] = t(lambda: ops.ecapa_fbank(audio, st_dev, ln_dev, L, tabs))
    z = torch.randn(nw, T, C, generator=g).to(BF16).cuda()
    y = torch.empty_like(z)
    k["res2net_ms"] = t(lambda: ops.ecapa_res2net(z, b["blk0.bn1_s"], b["blk0.bn1_t"], b["blk0.res_w"], b["blk0.res_b"], b["blk0.res_s"],
                                                  b["blk0.res_t"], T, w, cfg.dilations[0], y))
    k["res2net_tflops"] = 2.0 * R * 7 * w * 3 * w / (k["res2net_ms"]["median"] * 1e-3) / 1e12
    z2, o2 = z.reshape(R, C), torch.empty((R, C), dtype=BF16, device="cuda")
    k["gemm_cc_ms"] = t(lambda: ops.gemm_nt(z2, b["blk0.w1"], out=o2, bias=b["blk0.b1"]))
    k["gemm_cc_tflops"] = 2.0 * R * C * C / (k["gemm_cc_ms"]["median"] * 1e-3) / 1e12
    z3 = torch.randn(R, 3 * C, generator=g).to(BF16).cuda()
    o3 = torch.empty_like(z3)
    k["gemm_mfa_ms"] = t(lambda: ops.gemm_nt(z3, b["mfa_w"], out=o3, bias=b["mfa_b"]))
    k["gemm_mfa_tflops"] = 2.0 * R * 9 * C * C / (k["gemm_mfa_ms"]["median"] * 1e-3) / 1e12
    k["se_residual_ms"] = t(lambda: ops.ecapa_se_residual(z2, b["blk0.bn2_s"], b["blk0.bn2_t"], b["blk0.se_w1t"], b["blk0.se_b1"], b["blk0.se_w2t"],
                                                          b["blk0.se_b2"], o2, o3, C, nw, T))
    k["relu_bn_stats_ms"] = t(lambda: ops.ecapa_relu_bn(z3, b["mfa_s"], b["mfa_t"], nw, T, want_stats=True))
    k["relu_bn_stats_gbs"] = 3.0 * R * 3 * C * 2 / (k["relu_bn_stats_ms"]["median"] * 1e-3) / 1e9          # read twice, written once
    lg = torch.randn(R, 3 * C, generator=g).cuda()
    k["asp_pool_ms"] = t(lambda: ops.ecapa_asp_pool(lg, z3, b["aspbn_s"], b["aspbn_t"], nw, T))
    res["kernels_at_one_chunk"] = dict(windows=nw, rows=R, **k)
    print(json.dumps(res), flush=True)

    if not a.no_torch:
        et, res["torch_bf16_ms"], pc = torch_legs(sd, audio, starts, L, a.torch_batch, min(a.per_call_windows, N), a.warmup, max(3, a.repeats // 2))
        res["per_call_ms"] = dict(windows=min(a.per_call_windows, N), **pc)
        res["per_call_scaled_ms"] = pc["median"] * N / min(a.per_call_windows, N)
        res["device_over_torch_bf16"] = res["torch_bf16_ms"]["median"] / res["device_ms"]["median"]
        res["device_over_per_call"] = res["per_call_scaled_ms"] / res["device_ms"]["median"]
        cos = torch.nn.functional.cosine_similarity(emb, et, dim=1)
        res["cosine_device_vs_torch_bf16"] = dict(min=float(cos.min()), median=float(cos.median()))
        print(json.dumps({kk: res[kk] for kk in ("torch_bf16_ms", "per_call_ms", "per_call_scaled_ms", "device_over_torch_bf16",
                                                 "device_over_per_call", "cosine_device_vs_torch_bf16")}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
