#!/usr/bin/env python
"""The ragged encoder against the padded one, on the batch of scripts/packing_bench.py (32 synthetic clips, seeded durations uniform in
2-20 s, seed 0) or on an equal-length batch (32 x 10 s, bench.py's shape), timed with device events.

    python scripts/ragged_encoder_bench.py --mode encoder --leg padded                 # the 32-layer tower alone, padded to the longest clip
    python scripts/ragged_encoder_bench.py --mode encoder --leg ragged                 # ... every clip at its own length
    python scripts/ragged_encoder_bench.py --mode encoder --leg ragged --batch equal   # what the extra kernels cost when nothing is saved
    python scripts/ragged_encoder_bench.py --mode step --leg padded                    # whole ASRTrainer.training_step
    python scripts/ragged_encoder_bench.py --mode step --leg ragged
    python scripts/ragged_encoder_bench.py --mode step --leg ragged --pack-to 512      # ... with DataCollator(pack_to=512)'s LM layout

One process per configuration, one JSON line each: ms per call (median, min, max over the timed calls) and the row ratios
sum S_b / (B S_max) and sum S_b^2 / (B S_max^2).  TA355_LIB=<older libta355.so> runs a padded leg on another build of the library (the
ragged legs need the new entry points).  profiles/ragged_encoder.md holds the numbers of one session."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from scripts.packing_bench import clip_sequences  # noqa: E402  (the same clips, token sequences and mel lengths)


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["encoder", "step"], required=True)
    ap.add_argument("--leg", choices=["padded", "ragged"], required=True)
    ap.add_argument("--batch", choices=["ragged", "equal"], default="ragged")
    ap.add_argument("--pack-to", type=int, default=0, help="step mode: > 0 packs the LM rows (DataCollator(pack_to=...)'s layout)")
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
    dur = rng.uniform(2.0, 20.0, a.clips) if a.batch == "ragged" else np.full(a.clips, 10.0)
    m = ASRModel(ASRConfig(projector_hidden_dim=1024), device="cuda:0", init="random", seed=1, ragged_encoder=a.leg == "ragged")
    seqs, labs, counts, mels = clip_sequences(dur, m.audio_token_id, rng)
    T = max(mels)
    feats = torch.randn((a.clips, 128, T), generator=torch.Generator().manual_seed(a.seed)) * 0.5
    amask = torch.zeros((a.clips, T), dtype=torch.int64)
    for i, t in enumerate(mels):
        amask[i, :t] = 1; feats[i, :, t:] = 0
    S = np.asarray([(t - 1) // 2 + 1 for t in mels], np.float64)
    info = dict(mode=a.mode, leg=a.leg, batch=a.batch, pack_to=a.pack_to or None, lib=os.environ.get("TA355_LIB") or "tree", clips=a.clips,
                T=T, rows=int(S.sum()), padded_rows=int(a.clips * S.max()), row_ratio=round(float(S.sum() / (a.clips * S.max())), 4),
                row_sq_ratio=round(float((S ** 2).sum() / (a.clips * S.max() ** 2)), 4))
    if a.mode == "encoder":
        x = feats.to("cuda:0")
        lens = mels if a.leg == "ragged" else None       # host ints: no sync inside the timed region
        ms = timed(lambda: m.audio_tower(x, mel_lengths=lens) if lens is not None else m.audio_tower(x), a.warmup, a.steps)
    else:
        if a.pack_to > 0:
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
        # the audio mask stays on the host, where the collators leave it: the ragged switch reads its row sums there (no sync)
        batch = {k: (v if k == "audio_attention_mask" else v.to("cuda:0")) for k, v in batch.items()}
        tr = ASRTrainer(m, TrainingArguments(learning_rate=1e-5))
        m.train()
        last = {}
        ms = timed(lambda: last.update(loss=tr.training_step(batch)), a.warmup, a.steps)
        info.update(lm_rows=int(batch["input_ids"].shape[0]), row_len=int(batch["input_ids"].shape[1]), loss_sum=round(float(last["loss"]), 4))
    info.update(ms_median=round(float(np.median(ms)), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), steps=a.steps)
    print(json.dumps(info))


if __name__ == "__main__":
    main()
