#!/usr/bin/env python3
"""Greedy-generation timing at full model size (secondary metric: the WER loop's inference side).
B clips of 10 s, prompt = 3 + 125 <audio> + 24 tokens, N new tokens; reports prompt-pass and per-token latency.
``gen_bench.py [B [N]] [--scores] [--top-logprobs K]``: the same loop with the decoding scores on (token log-probability and entropy,
K alternatives per step).  Decoding options: ``--bad-words`` (256 two-token entries), ``--suppress`` (64 suppressed ids), ``--min-p P`` and
``--typical-p P`` (both switch sampling on: HF's warpers act under do_sample only); ``--options-sweep`` measures none, each of the four alone
and all of them in one process, one JSON line each.
``--num-beams K [--length-penalty P]``: beam search (``generate_beams``) on B clips x K beams, and in the same process greedy decoding at
B * K rows, so that the difference of the two per-step figures is the beam machinery (log-softmax, top-k, bookkeeping, cache reorder)."""
import sys, os, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from tiny_audio_amd.asr_config import ASRConfig
from tiny_audio_amd.asr_modeling import ASRModel

argv, scores, top_lp = [], False, 0
bad_words, suppress, min_p, typical_p, sweep = False, False, None, None, False
num_beams, length_penalty = 0, 1.0
it = iter(sys.argv[1:])
for a in it:
    if a == "--scores":
        scores = True
    elif a == "--top-logprobs":
        top_lp = int(next(it))
    elif a == "--bad-words":
        bad_words = True
    elif a == "--suppress":
        suppress = True
    elif a == "--min-p":
        min_p = float(next(it))
    elif a == "--typical-p":
        typical_p = float(next(it))
    elif a == "--num-beams":
        num_beams = int(next(it))
    elif a == "--length-penalty":
        length_penalty = float(next(it))
    elif a == "--options-sweep":
        sweep = True
    else:
        argv.append(a)
B = int(argv[0]) if len(argv) > 0 else (8 if num_beams else 32)
N = int(argv[1]) if len(argv) > 1 else 64
cfg = ASRConfig()
m = ASRModel(cfg, device="cuda", init="random", seed=0)
feats = torch.randn(B, 128, 1000, device="cuda") * 0.5
amask = torch.ones(B, 1000, dtype=torch.int64)
ids = torch.tensor([[5, 6, 7] + [cfg.audio_token_id] * 125 + list(range(100, 124))] * B)
kw = dict(input_ids=ids, input_features=feats, audio_attention_mask=amask, attention_mask=torch.ones_like(ids), eos_token_id=[])
if scores or top_lp:
    kw.update(return_token_scores=scores, top_logprobs=top_lp)


def option_kwargs(bad_words, suppress, min_p, typical_p):
    o = {}
    if bad_words:       # 256 two-token entries over 16 last tokens: groups of 16 sequences
        o["bad_words_ids"] = [[2000 + i, 3000 + i % 16] for i in range(256)]
    if suppress:
        o["suppress_tokens"] = list(range(4000, 4064))
    if min_p is not None or typical_p is not None:
        o.update(do_sample=True, seed=0)
        if min_p is not None:
            o["min_p"] = min_p
        if typical_p is not None:
            o["typical_p"] = typical_p
    return o


def measure(options, gen=None, kw=kw):
    gen = gen or m.generate
    res = {}
    for n in (1, N):
        gen(**kw, **options, max_new_tokens=n); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            gen(**kw, **options, max_new_tokens=n)
        torch.cuda.synchronize()
        res[n] = (time.perf_counter() - t0) / 3
    return res


if num_beams:
    K = num_beams
    r = measure(dict(num_beams=K, length_penalty=length_penalty), m.generate_beams)
    rows = B * K                      # greedy at the same number of rows: what the decode step itself costs
    kw_g = dict(kw, input_ids=ids[:1].expand(rows, -1).contiguous(), input_features=feats[:1].expand(rows, -1, -1).contiguous(),
                audio_attention_mask=amask[:1].expand(rows, -1).contiguous(), attention_mask=torch.ones(rows, ids.shape[1], dtype=torch.int64))
    g = measure({}, kw=kw_g)
    beam_ms, greedy_ms = (r[N] - r[1]) / (N - 1) * 1e3, (g[N] - g[1]) / (N - 1) * 1e3
    print(json.dumps({"B": B, "num_beams": K, "rows": rows, "length_penalty": length_penalty, "new_tokens": N,
                      "prompt_pass_ms": round(r[1] * 1e3, 2), "per_step_ms": round(beam_ms, 3),
                      "greedy_rows": rows, "greedy_prompt_pass_ms": round(g[1] * 1e3, 2), "greedy_per_token_ms": round(greedy_ms, 3),
                      "beam_machinery_ms_per_step": round(beam_ms - greedy_ms, 3)}))
    sys.exit(0)


if sweep:
    for name, o in (("none", option_kwargs(False, False, None, None)), ("sampling only", dict(do_sample=True, seed=0)),
                    ("bad_words", option_kwargs(True, False, None, None)), ("suppress", option_kwargs(False, True, None, None)),
                    ("min_p", option_kwargs(False, False, 0.05, None)), ("typical_p", option_kwargs(False, False, None, 0.9)),
                    ("all", option_kwargs(True, True, 0.05, 0.9))):
        r = measure(o)
        print(json.dumps({"B": B, "new_tokens": N, "options": name, "prompt_pass_ms": round(r[1] * 1e3, 2),
                          "per_token_ms": round((r[N] - r[1]) / (N - 1) * 1e3, 3)}), flush=True)
    sys.exit(0)
options = option_kwargs(bad_words, suppress, min_p, typical_p)
res = measure(options)
per_tok = (res[N] - res[1]) / (N - 1)
# decode roofline: a step streams every LM weight once (bf16 linears of all layers + the tied lm_head) and the KV cache of the
# positions so far (prompt 152 + on average N / 2 generated); HBM peak 8 TB/s (MI355X_MICROARCH.md)
t = cfg.text_config
D, F, nl = t.hidden_size, t.intermediate_size, t.num_hidden_layers
nq, nkv, hd = t.num_attention_heads, t.num_key_value_heads, t.head_dim
vocab_pad = (t.vocab_size + 127) // 128 * 128
w_bytes = 2 * (nl * (D * (nq + 2 * nkv) * hd + nq * hd * D + 3 * D * F) + vocab_pad * D)
kv_bytes = 2 * 2 * nl * B * nkv * hd * (ids.shape[1] + N // 2)
floor_ms = (w_bytes + kv_bytes) / 8e12 * 1e3
print(json.dumps({"B": B, "new_tokens": N, "prompt_pass_ms": round(res[1] * 1e3, 2), "per_token_ms": round(per_tok * 1e3, 3),
                  "tokens_per_s": round(B / per_tok, 1), "total_ms": round(res[N] * 1e3, 1),
                  "rtf_audio_s_per_s": round(B * 10.0 / res[N], 1),
                  "roofline": {"bound": "hbm", "weight_bytes": w_bytes, "kv_cache_bytes": kv_bytes, "peak": 8000.0, "unit": "GB/s",
                               "achieved": round((w_bytes + kv_bytes) / per_tok / 1e9, 1),
                               "frac": round(floor_ms / (per_tok * 1e3), 4), "floor_ms_per_token": round(floor_ms, 4),
                               "frac_weights_only": round(w_bytes / 8e12 / per_tok, 4)},
                  "fused": os.environ.get("TA355_DECODE_FUSED", "1") != "0", "token_scores": bool(scores or top_lp), "top_logprobs": top_lp,
                  "options": sorted(k for k in options if k not in ("do_sample", "seed"))}))
