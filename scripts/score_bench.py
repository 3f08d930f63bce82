#!/usr/bin/env python3
"""Candidate-scoring timing at full model size, the LM part only (synthetic ids and audio embeddings, as gen_bench.py).
B = 32 clips, prompt L = 3 + 125 <audio> + 32 tokens = 160, K candidates of T tokens per clip, for (K, T) in {4, 8} x {4, 32}.  Per shape,
alternating in one process:
  shared    ``Qwen3MI355X.score_candidates``: one prompt pass over [B, L] plus one ``ta_lm_score`` over [B*K, T] rows;
  prefill   the same call with one one-token candidate per clip (the prompt pass, the per-clip log-sum-exp and the row kernel: no
            decoder layer runs for the candidates), so shared - prefill is the extend layers + head + cross-entropy;
  repeated  the only route without ``ta_lm_score``: ``forward_loss`` (no backward) over [B*K, L + T] rows with the prompt repeated per
            candidate and labels on the candidate positions.
Times are host clocks around work that ends in a device synchronise, the median of ``--iters`` (default 7) after 2 warm-up calls.
One JSON line per shape, and the largest |score - repeated-route score| as a consistency figure.
``score_bench.py [--iters N] [--B n]``"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tiny_audio_amd.asr_config import ASRConfig
from tiny_audio_amd.asr_modeling import ASRModel

iters, B = 7, 32
it = iter(sys.argv[1:])
for a in it:
    if a == "--iters":
        iters = int(next(it))
    elif a == "--B":
        B = int(next(it))
cfg = ASRConfig()
m = ASRModel(cfg, device="cuda", init="random", seed=0)
lm = m.language_model
dev, D, V = "cuda", cfg.text_config.hidden_size, cfg.text_config.vocab_size
N_AUDIO = 125
prompt = [5, 6, 7] + [cfg.audio_token_id] * N_AUDIO + list(range(100, 132))
L = len(prompt)
ids = torch.tensor([prompt] * B, device=dev)
g = torch.Generator(device="cpu").manual_seed(0)
audio = (torch.randn(B * N_AUDIO, D, generator=g) * 0.02).to(dev)
src_row = torch.full((B, L), -1, dtype=torch.int32)
src_row[:, 3:3 + N_AUDIO] = torch.arange(B * N_AUDIO, dtype=torch.int32).reshape(B, N_AUDIO)
att = torch.ones((B, L), dtype=torch.int32, device=dev)


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2] * 1e3


for K in (4, 8):
    for T in (4, 32):
        R = B * K
        cand = torch.randint(0, V - 1000, (R, T), generator=g)
        n_tok = torch.full((R,), T, dtype=torch.int64)
        clip = torch.arange(B).repeat_interleave(K)
        # the repeated-prompt batch: row (b, k) = prompt of b followed by candidate k; label row L - 1 + t predicts token t
        ids_rep = torch.cat([ids.repeat_interleave(K, 0), cand.to(dev)], 1).contiguous()
        src_rep = torch.cat([src_row.repeat_interleave(K, 0), torch.full((R, T), -1, dtype=torch.int32)], 1).to(dev).contiguous()
        att_rep = torch.ones((R, L + T), dtype=torch.int32, device=dev)
        rows = (torch.arange(R, dtype=torch.int32)[:, None] * (L + T) + L - 1 + torch.arange(T, dtype=torch.int32)[None, :]).reshape(-1).to(dev)
        targets = cand.reshape(-1).to(dev)
        src_dev = src_row.to(dev)

        shared = lambda: lm.score_candidates(ids, src_dev, audio, att, cand, n_tok, clip)  # noqa: E731
        one = torch.zeros((B, 1), dtype=torch.int64)
        prefill = lambda: lm.score_candidates(ids, src_dev, audio, att, one, torch.ones(B, dtype=torch.int64), torch.arange(B))  # noqa: E731
        repeated = lambda: lm.forward_loss(ids_rep, src_rep, audio, att_rep, rows, targets, R * T, 1.0)  # noqa: E731
        t_sh, t_rep, t_pre = timed(shared), timed(repeated), timed(prefill)
        t_sh2, t_rep2 = timed(shared), timed(repeated)                   # the pair again: the spread of the same command
        _, sc = shared()
        _, nll, _, _ = repeated()
        gap = float((sc.double() + nll.double().reshape(R, T).sum(-1)).abs().max())
        print(json.dumps({"B": B, "K": K, "T": T, "L": L, "rows_shared": B * L + R * T, "rows_repeated": R * (L + T),
                          "shared_ms": round(t_sh, 2), "shared_ms_again": round(t_sh2, 2), "prefill_ms": round(t_pre, 2),
                          "extend_head_ce_ms": round(t_sh - t_pre, 2), "repeated_ms": round(t_rep, 2), "repeated_ms_again": round(t_rep2, 2),
                          "speedup": round(t_rep / t_sh, 2), "max_abs_score_gap": round(gap, 4)}), flush=True)
