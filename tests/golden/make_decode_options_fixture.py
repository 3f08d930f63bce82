"""Writes tests/golden/decode_options.npz from the logits processors of the installed ``transformers`` (5.15) on the CPU:

    python tests/golden/make_decode_options_fixture.py

* inputs: scores 3 * randn f32 [3, 1003], context ids [3, 24] (20 prompt + 4 generated tokens) with planted repeats and tails;
* every processor's output alone (float32, HF's own arithmetic);
* the output of the ``LogitsProcessorList`` that ``GenerationMixin._get_logits_processor`` builds for a ``GenerationConfig`` with every
  processor option set (a tiny Qwen3 on the CPU), at three (step, max_new) points so that every step-indexed rule fires once -- this
  pins HF's order -- and the class names of the list with ``do_sample=True``, which pins the warpers' order;
* the bands of the four threshold warpers: over the device tests' own inputs (``decode_options_ref.warp_inputs``, seeds 100..103,
  V = 1003 and V = 151 670) the largest relative distance from the float64 threshold of any element on which HF's float32 result
  disagrees with the float64 decision; band = 4 x that with a floor of 1e-5 (the device sums f32 in another order at the same
  precision).  The measured strays are stored next to the bands.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import decode_options_ref as R      # noqa: E402
C = R.CASES

from transformers import GenerationConfig, Qwen3Config, Qwen3ForCausalLM      # noqa: E402
from transformers.generation import logits_process as LP      # noqa: E402


def main():
    out = {}
    scores, ctx = C.scores(), C.context()
    out["scores"], out["context"] = scores, ctx
    ts, ti = torch.from_numpy(scores), torch.from_numpy(ctx)
    run = lambda proc, ids=ti: proc(ids, ts.clone()).numpy().astype(np.float32)  # noqa: E731

    out["sequence_bias"] = run(LP.SequenceBiasLogitsProcessor(dict(C.SEQUENCE_BIAS)))
    out["sequence_bias_list_form"] = run(LP.SequenceBiasLogitsProcessor([[list(k), v] for k, v in C.SEQUENCE_BIAS_LIST_FORM]))
    out["sequence_bias_generated_only"] = run(LP.SequenceBiasLogitsProcessor(dict(C.SEQUENCE_BIAS)), ti[:, C.L:])
    out["bad_words"] = run(LP.NoBadWordsLogitsProcessor([list(w) for w in C.BAD_WORDS], eos_token_id=list(C.EOS)))
    out["forced_eos_last"] = run(LP.ForcedEOSTokenLogitsProcessor(C.L + 5, list(C.FORCED)))           # context 24 = max_length - 1
    out["forced_eos_before"] = run(LP.ForcedEOSTokenLogitsProcessor(C.L + 8, list(C.FORCED)))
    out["exponential_decay"] = run(LP.ExponentialDecayLengthPenalty(C.DECAY, list(C.EOS), C.L))        # t = 4 > start = 2
    out["exponential_decay_before"] = run(LP.ExponentialDecayLengthPenalty((4, C.DECAY[1]), list(C.EOS), C.L))
    out["suppress"] = run(LP.SuppressTokensLogitsProcessor(list(C.SUPPRESS)))
    out["begin_suppress_t0"] = run(LP.SuppressTokensAtBeginLogitsProcessor(list(C.BEGIN_SUPPRESS), C.L), ti[:, :C.L])
    out["begin_suppress_t4"] = run(LP.SuppressTokensAtBeginLogitsProcessor(list(C.BEGIN_SUPPRESS), C.L))
    out["min_p"] = run(LP.MinPLogitsWarper(C.MIN_P))
    out["typical_p"] = run(LP.TypicalLogitsWarper(C.TYPICAL_P))
    out["epsilon_cutoff"] = run(LP.EpsilonLogitsWarper(C.EPSILON))
    out["eta_cutoff"] = run(LP.EtaLogitsWarper(C.ETA))

    # HF's own list, from a GenerationConfig with everything set
    model = Qwen3ForCausalLM(Qwen3Config(vocab_size=C.V, hidden_size=16, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2,
                                         num_key_value_heads=1, head_dim=8, max_position_embeddings=64))
    names = None
    for tag, t, max_new in C.CHAIN_POINTS:
        kw = dict(C.chain_generation_kwargs(max_new))
        kw["sequence_bias"] = dict(kw["sequence_bias"])
        gc = GenerationConfig(**kw, max_length=C.L + max_new, do_sample=False)
        model._prepare_special_tokens(gc, True, device=torch.device("cpu"))
        procs = model._get_logits_processor(gc, input_ids_seq_length=C.L, encoder_input_ids=None, prefix_allowed_tokens_fn=None,
                                            logits_processor=LP.LogitsProcessorList(), device="cpu", model_kwargs={})
        out[f"chain_{tag}"] = procs(ti[:, :C.L + t], ts.clone()).numpy().astype(np.float32)
        names = [type(p).__name__ for p in procs]
    gc = GenerationConfig(**{**C.chain_generation_kwargs(8), "sequence_bias": dict(C.SEQUENCE_BIAS)}, max_length=C.L + 8, do_sample=True,
                          temperature=0.7, top_k=50, top_p=0.9, min_p=C.MIN_P, typical_p=C.TYPICAL_P, epsilon_cutoff=C.EPSILON,
                          eta_cutoff=C.ETA, renormalize_logits=True)
    model._prepare_special_tokens(gc, True, device=torch.device("cpu"))
    procs = model._get_logits_processor(gc, input_ids_seq_length=C.L, encoder_input_ids=None, prefix_allowed_tokens_fn=None,
                                        logits_processor=LP.LogitsProcessorList(), device="cpu", model_kwargs={})
    order = dict(processors=names, with_do_sample=[type(p).__name__ for p in procs])
    out["hf_order_json"] = np.frombuffer(json.dumps(order).encode(), dtype=np.uint8)

    # bands
    stray = dict(min_p=0.0, epsilon=0.0, eta=0.0, typical_s=0.0, typical_mass=0.0)
    none = torch.zeros((1, 0), dtype=torch.int64)
    for V, B in C.WARP_SHAPES:
        for seed in C.WARP_SEEDS:
            x = R.warp_inputs(seed, V, B)
            tx = torch.from_numpy(x)
            for name, hf, ref in (("min_p", LP.MinPLogitsWarper(C.MIN_P), lambda a: R.min_p(a, C.MIN_P)),
                                  ("epsilon", LP.EpsilonLogitsWarper(C.EPSILON), lambda a: R.epsilon_cutoff(a, C.EPSILON)),
                                  ("eta", LP.EtaLogitsWarper(C.ETA), lambda a: R.eta_cutoff(a, C.ETA))):
                removed = torch.isneginf(hf(none, tx.clone())).numpy()
                keep, dist = ref(x)
                bad = removed == keep
                if bad.any():
                    stray[name] = max(stray[name], float(dist[bad].max()))
            removed = torch.isneginf(LP.TypicalLogitsWarper(C.TYPICAL_P)(none, tx.clone())).numpy()
            keep, _ = R.typical(x, C.TYPICAL_P)
            bad = removed == keep
            if bad.any():
                ds, dm = R.typical_distances(x, C.TYPICAL_P)
                on_s = ds[bad] <= dm[bad]                 # every disagreement is charged to the nearer of the two thresholds
                if on_s.any():
                    stray["typical_s"] = max(stray["typical_s"], float(ds[bad][on_s].max()))
                if (~on_s).any():
                    stray["typical_mass"] = max(stray["typical_mass"], float(dm[bad][~on_s].max()))
            print(V, seed, {k: f"{v:.3g}" for k, v in stray.items()}, flush=True)
    for k, v in stray.items():
        out[f"stray_{k}"] = np.float64(v)
        out[f"band_{k}"] = np.float64(max(4.0 * v, 1e-5))
    path = os.path.join(ROOT, "tests", "golden", "decode_options.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", order)
    print({k: float(out[k]) for k in out if k.startswith(("stray_", "band_"))})


if __name__ == "__main__":
    main()
