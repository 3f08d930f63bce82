"""Device-event timing of the text tower at SmolLM3-3B widths next to Qwen3-1.7B (one process, one GPU).

    python scripts/smollm3_bench.py [--batch 32] [--seq-len 192] [--iters 10] [--warmup 3] [--only smollm3|qwen3] [--no-decode]
                                    [--out profiles/smollm3.json]

Rows, per tower: one LM training step of the frozen-LM recipe -- ta_lm_forward_loss + ta_lm_backward down to d(audio embeddings), the
share of a stage-1 step that the text tower owns (encoder, projector and optimizer do not depend on the tower) -- at B x L tokens, the two
towers timed in ALTERNATION; and greedy decoding per generated token at B = 8 and B = 32 (prompt of 64 tokens; the difference of a 36-token
and a 4-token generation divided by 32, so the prompt pass and the hipGraph capture cancel).  SmolLM3-3B: 36 layers, D 2048, F 11008,
16 / 4 heads, V 128 257, every 4th layer NoPE, no q/k-norm.  Qwen3-1.7B: 28 layers, D 2048, F 6144, 16 / 8 heads, V 151 670.
Weights are random (the times do not depend on them).  ``--only`` runs one tower alone (for a rocprofv3 --kernel-trace --stats run);
``--layers N`` cuts both towers to N layers.  There is no fallback: without a GPU the script fails.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tiny_audio_amd import ops  # noqa: E402
from tiny_audio_amd.asr_config import LMConfig  # noqa: E402
from tiny_audio_amd.language_model import Qwen3MI355X  # noqa: E402

TOWERS = {
    "smollm3": dict(model_type="smollm3", vocab_size=128257, max_position_embeddings=4096),     # SmolLM3Config() + the <audio> row
    "qwen3": dict(model_type="qwen3", vocab_size=151670, hidden_size=2048, intermediate_size=6144, num_hidden_layers=28,
                  num_attention_heads=16, num_key_value_heads=8),                                 # Qwen3-1.7B
}


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
    ap.add_argument("--seq-len", type=int, default=192)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=0, help="cut both towers to this many layers (0 = their own depth)")
    ap.add_argument("--only", choices=sorted(TOWERS), default=None)
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "smollm3_bench needs a GPU"
    dev, B, L = "cuda", a.batch, a.seq_len
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    lms = {}
    for name, src in TOWERS.items():
        if a.only in (None, name):
            cfg = LMConfig(dict(src, **({"num_hidden_layers": a.layers} if a.layers else {})))
            lms[name] = Qwen3MI355X(cfg, dev).random_init(1)
    rows = []

    def step_fn(lm):
        c = lm.config
        ids = torch.full((B, L), c.vocab_size - 1, dtype=torch.int64, device=dev)
        ids[:, L // 2:] = torch.randint(0, c.vocab_size - 1, (B, L - L // 2), device=dev, generator=gen)     # half <audio> rows, half text
        n_audio = B * (L // 2)
        src_row = torch.full((B, L), -1, dtype=torch.int32, device=dev)
        src_row[:, :L // 2] = torch.arange(n_audio, dtype=torch.int32, device=dev).view(B, L // 2)
        src_row = src_row.reshape(-1).contiguous()
        audio = torch.randn(n_audio, c.hidden_size, device=dev, generator=gen)
        lab = torch.full((B, L), -100, dtype=torch.int64, device=dev)
        lab[:, L - 32:] = ids[:, L - 32:]
        rows_, tg, n = ops.label_rows(lab)
        n = int(n.item())
        att = torch.ones((B, L), dtype=torch.int32, device=dev)

        def f():
            _, _, _, ctx = lm.forward_loss(ids, src_row, audio, att, rows_, tg, n, 1.0 / n)
            lm.backward_from_ctx(ctx, n_audio)
        return f

    t = timed({k: step_fn(lm) for k, lm in lms.items()}, a.iters, a.warmup)
    for k, v in t.items():
        c = lms[k].config
        r = row(f"{k} LM step (forward + loss + backward to d(audio)), B={B}, L={L}, {c.num_hidden_layers} layers", v)
        r["attention_path"] = "fused" if (c.num_attention_heads // c.num_key_value_heads) * ((L + 31) // 32) <= 12 and L <= 192 else "two-kernel"
        rows.append(r)

    if not a.no_decode:
        for Bd in (8, 32):
            for k, lm in lms.items():
                c = lm.config
                Lp = 64
                ids = torch.randint(0, c.vocab_size - 1, (Bd, Lp), device=dev, generator=gen)

                def gen_n(n_new):
                    return lambda: lm.greedy_decode(ids, None, None, None, max_new_tokens=n_new, eos_ids=(), pad_id=0)
                t = timed({"n4": gen_n(4), "n36": gen_n(36)}, max(3, a.iters // 2), 1)
                per = (np.median(t["n36"]) - np.median(t["n4"])) / 32.0
                rows.append(dict(name=f"{k} greedy decoding, B={Bd}, prompt {Lp}", ms_per_token=float(per), median_ms_36=float(np.median(t["n36"])),
                                 median_ms_4=float(np.median(t["n4"]))))
    print("| row | median ms | min | max | spread |\n|---|---|---|---|---|")
    for r in rows:
        if "ms_per_token" in r:
            print(f"| {r['name']} | {r['ms_per_token']:.3f} per token | | | |")
        else:
            print(f"| {r['name']} ({r['attention_path']} attention) | {r['median_ms']:.3f} | {r['min_ms']:.3f} | {r['max_ms']:.3f} | {100 * r['spread']:.1f} % |")
    print(json.dumps({"rows": rows}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
