"""Cost of LoRA dropout on the configs[4] step (stage 2: frozen MLP projector, LoRA r = 8 / alpha = 32 on q, k, v, o, gate, up, down):
the bench.py step at B = 32, L = 192, timed at lora_dropout = 0 and at p (default 0.05) in ONE process on one model, legs interleaved
(A B A B ...) so that clock and thermal drift fall on both.  Prints one JSON line.

    python scripts/lora_dropout_bench.py [--steps 10] [--warmup 3] [--rounds 3] [--p 0.05] [--only-p]

``--only-p``: run only the p > 0 leg (for a kernel trace: rocprofv3 --kernel-trace --stats -- python scripts/lora_dropout_bench.py --only-p).
The LM is put in training mode explicitly: ASRModel.train() keeps the frozen LM, and with it peft's dropout, in eval mode.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq-len", type=int, default=192)
    ap.add_argument("--p", type=float, default=0.05)
    ap.add_argument("--only-p", action="store_true")
    a = ap.parse_args()
    from tiny_audio_amd import ops
    from tiny_audio_amd.asr_config import ASRConfig
    from tiny_audio_amd.asr_modeling import ASRModel
    from tiny_audio_amd.asr_processing import LogMelFeatureExtractor
    from tiny_audio_amd.synthetic import token_batch
    from tiny_audio_amd.trainer import ASRTrainer, TrainingArguments

    dev = torch.device("cuda", 0)
    cfg = ASRConfig(model_dtype="float32", audio_token_dropout=0.10, use_lora=True, freeze_projector=True, lora_dropout=a.p)
    torch.manual_seed(0)
    model = ASRModel(cfg, device=dev, init="random", seed=0)
    model.train()
    lm = model.language_model
    lm.train(True)
    fe = LogMelFeatureExtractor(128, dev)
    trainer = ASRTrainer(model, TrainingArguments(learning_rate=1e-3, weight_decay=0.0, max_grad_norm=1.0, warmup_steps=500,
                                                  max_steps=50000, lr_scheduler_type="polynomial", lr_scheduler_kwargs={"power": 0.5}))
    B, L, n_samples = a.batch, a.seq_len, 160000
    g = torch.Generator(device=dev); g.manual_seed(1234)
    wav = 0.1 * torch.randn(B, n_samples, device=dev, generator=g)
    lens = torch.full((B,), n_samples, device=dev, dtype=torch.int64)
    n_audio = int(model.projector.get_output_length(n_samples // 320))
    ids, att, lab, counts, n_lab = token_batch(B, n_audio, cfg.text_config.vocab_size, cfg.audio_token_id, cfg.pad_token_id,
                                               cfg.eos_token_id, L=L)
    ids_d, att_d, lab_d = (torch.from_numpy(x).to(dev) for x in (ids, att, lab))
    counts_d = torch.from_numpy(counts).to(dev)

    def step():
        feats, _ = fe.extract(wav, lens)
        rows, tg, _n = ops.label_rows(lab_d)
        trainer.training_step(dict(input_ids=ids_d, input_features=feats, attention_mask=att_d, labels=lab_d, audio_token_counts=counts_d,
                                   label_meta=(rows, tg, n_lab)))

    def leg(p):
        lm.lora_dropout = p
        for _ in range(a.warmup):
            step()
        trainer.flush(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        trainer.flush(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3

    import gc
    gc.collect(); gc.freeze()
    legs = {0.0: [], a.p: []}
    for _ in range(a.rounds):
        for p in ((a.p,) if a.only_p else (0.0, a.p)):
            legs[p].append(leg(p))
    res = {"config": "configs[4] step, B=%d L=%d, fp32 streams" % (B, L), "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "p": a.p, "ms_per_step_p": [round(v, 3) for v in legs[a.p]], "loss": float(trainer.last_loss())}
    if not a.only_p:
        m0, m1 = min(legs[0.0]), min(legs[a.p])
        res.update(ms_per_step_p0=[round(v, 3) for v in legs[0.0]], best_p0=round(m0, 3), best_p=round(m1, 3), delta_ms=round(m1 - m0, 3))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
