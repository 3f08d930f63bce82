#!/usr/bin/env python
"""Sequence packing against padding on one ragged batch: 32 synthetic clips with seeded durations uniform in 2-20 s, Qwen3-0.6B widths,
MLP projector, full training steps (forward, backward, optimizer) timed with device events.

    python scripts/packing_bench.py --mode padded                 # one clip per row, padded to the longest (today's batch)
    python scripts/packing_bench.py --mode packed --pack-to 512   # DataCollator(pack_to=512)'s layout

One process per configuration, one JSON line each: ms per step (median, min, max over the timed steps), LM rows per step and row
utilisation (real tokens / rows).  TA355_LIB=<older libta355.so> runs the padded mode on another build of the library (the packed mode
needs the _seg entry points).  profiles/packing.md holds the numbers of one session."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def clip_sequences(durations, audio_id, rng):
    """Per clip: chat prefix, one <audio> per projector frame, prompt, then the labelled transcript (~2.5 tokens per second) + eos."""
    seqs, labs, counts, mels = [], [], [], []
    for d in durations:
        mel = int(round(d * 100))
        n = (((mel - 1) // 2 + 1) - 4) // 4 + 1
        text = rng.randint(10, 5000, int(2.5 * d) + 3)
        ids = np.concatenate([rng.randint(10, 5000, 8), np.full(n, audio_id), rng.randint(10, 5000, 12), text]).astype(np.int64)
        lab = np.full(ids.size, -100, np.int64); lab[-text.size:] = text
        seqs.append(ids); labs.append(lab); counts.append(n); mels.append(mel)
    return seqs, labs, counts, mels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["padded", "packed"], required=True)
    ap.add_argument("--pack-to", type=int, default=512)
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from tiny_audio_amd.asr_config import ASRConfig
    from tiny_audio_amd.asr_modeling import ASRModel
    from tiny_audio_amd.collator import pack_sequences
    from tiny_audio_amd.trainer import ASRTrainer, TrainingArguments
    rng = np.random.RandomState(a.seed)
    dur = rng.uniform(2.0, 20.0, a.clips)
    cfg = ASRConfig(projector_hidden_dim=1024)
    m = ASRModel(cfg, device="cuda:0", init="random", seed=1)
    seqs, labs, counts, mels = clip_sequences(dur, m.audio_token_id, rng)
    T = max(mels)
    feats = torch.randn((a.clips, 128, T), generator=torch.Generator().manual_seed(a.seed)) * 0.5
    amask = torch.zeros((a.clips, T), dtype=torch.int64)
    for i, t in enumerate(mels):
        amask[i, :t] = 1; feats[i, :, t:] = 0
    if a.mode == "packed":
        batch, order = pack_sequences(seqs, labs, a.pack_to, pad_id=0)
        order = torch.tensor(order)
        batch.update(input_features=feats[order], audio_attention_mask=amask[order], audio_token_counts=torch.tensor(counts)[order])
    else:
        L = max(s.size for s in seqs)
        ids = torch.zeros((a.clips, L), dtype=torch.int64); lab = torch.full((a.clips, L), -100, dtype=torch.int64)
        att = torch.zeros((a.clips, L), dtype=torch.int64)
        for i, (s, l) in enumerate(zip(seqs, labs)):
            ids[i, :s.size] = torch.from_numpy(s); lab[i, :s.size] = torch.from_numpy(l); att[i, :s.size] = 1
            lab[i, 0] = -100
        batch = dict(input_ids=ids, labels=lab, attention_mask=att, input_features=feats, audio_attention_mask=amask,
                     audio_token_counts=torch.tensor(counts))
    batch = {k: v.to("cuda:0") for k, v in batch.items()}
    tr = ASRTrainer(m, TrainingArguments(learning_rate=1e-5))
    m.train()
    for _ in range(a.warmup):
        tr.training_step(batch)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); loss = tr.training_step(batch); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    rows, Lp = batch["input_ids"].shape
    real = int(sum(s.size for s in seqs))
    print(json.dumps(dict(mode=a.mode, pack_to=a.pack_to if a.mode == "packed" else None, lib=os.environ.get("TA355_LIB") or "tree",
                          ms_median=round(float(np.median(ms)), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), steps=a.steps,
                          lm_rows=rows, row_len=Lp, lm_token_rows=rows * Lp, real_tokens=real, utilisation=round(real / (rows * Lp), 4),
                          loss_sum=round(float(loss), 4))))


if __name__ == "__main__":
    main()
