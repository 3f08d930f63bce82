"""Writes tests/golden/beam_search.npz from the beam search of the installed ``transformers`` (5.15) on the CPU.

A tiny random ``Qwen3ForCausalLM`` (V = 1003, the geometry of make_decode_options_fixture.py) decodes B = 2 prompts with
``generate(..., num_beams=K, output_scores=True, return_dict_in_generate=True)`` for the runs of ``RUNS`` below: K in {1, 2, 4},
length_penalty in {0, 1, 2}, early_stopping in {False, True, "never"}, none / one / two eos ids, num_return_sequences in {1, K}, one
run with repetition_penalty and min_new_tokens.  With K = 1 HF runs greedy search: those runs store log_softmax of its scores and no
sequence scores, and a one-beam search with early_stopping=True must return the greedy tokens up to and including the first eos.
The eos ids are tokens the beams of an eos-free run pass through early, so some beams finish early while others run to the maximum
length.

Stored per run: HF's ``sequences`` (generated part), ``sequences_scores``, ``beam_indices``, and every step's processed ``scores``
rows of the running beams -- as each row's M largest entries (value, index), which is all a clip's top M can draw from; the test
rebuilds the rows with -inf elsewhere.  tests/test_beam_ref.py feeds them to tests/beam_ref.py and requires HF's sequences and scores
exactly.  Condition, checked here: no exact tie among the M + 1 largest finite accumulated values of any clip and step (torch.topk
promises no order among ties); the model seed is advanced until it holds and recorded in the file.

    python tests/golden/make_beam_fixture.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import beam_ref as BR      # noqa: E402

from transformers import Qwen3Config, Qwen3ForCausalLM      # noqa: E402

V, L, B, MAX_NEW, PAD = 1003, 5, 2, 6, 990
# (K, length_penalty, early_stopping, n_eos, num_return_sequences, extra generate kwargs)
RUNS = [(1, 1.0, True, 1, 1, {}), (1, 0.0, True, 2, 1, {}), (2, 0.0, True, 1, 2, {}), (2, 2.0, "never", 2, 1, {}),
        (2, 1.0, False, 0, 2, {}), (4, 1.0, False, 1, 4, {}), (4, 0.0, "never", 1, 1, {}), (4, 2.0, True, 2, 4, {}),
        (4, 2.0, False, 1, 1, {}), (4, 1.0, True, 2, 1, dict(repetition_penalty=1.3, min_new_tokens=2))]


def build(seed):
    torch.manual_seed(seed)
    model = Qwen3ForCausalLM(Qwen3Config(vocab_size=V, hidden_size=16, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2,
                                         num_key_value_heads=1, head_dim=8, max_position_embeddings=64)).eval()
    with torch.no_grad():                               # sharper than the default init: a few tokens stand out, as in a trained model
        for p in model.parameters():
            p.mul_(6.0)
    ids = torch.from_numpy(np.random.default_rng(seed).integers(1, 900, size=(B, L)).astype(np.int64))
    return model, ids


def generate(model, ids, K, lp, es, eos, nrs, extra):
    with torch.no_grad():
        return model.generate(ids, attention_mask=torch.ones_like(ids), max_new_tokens=MAX_NEW, num_beams=K, length_penalty=lp,
                              early_stopping=es, num_return_sequences=nrs, eos_token_id=list(eos) or None, pad_token_id=PAD,
                              do_sample=False, output_scores=True, return_dict_in_generate=True, **extra)


def attempt(seed):
    model, ids = build(seed)
    free = generate(model, ids, 4, 1.0, False, (), 4, {})
    gen = free.sequences[:, L:].numpy()
    # eos ids: the second token of clip 0's best beam and the third token of clip 1's second beam
    eos2 = [int(gen[0, 1]), int(gen[5, 2])]
    if eos2[0] == eos2[1] or PAD in eos2:
        return None
    out = dict(seed=np.int64(seed), input_ids=ids.numpy())
    meta = []
    for i, (K, lp, es, n_eos, nrs, extra) in enumerate(RUNS):
        eos = eos2[:n_eos]
        o = generate(model, ids, K, lp, es, eos, nrs, extra)
        M = BR.n_candidates(K, n_eos)
        if K == 1:                                      # HF runs greedy search and scores logits: log_softmax gives what a one-beam search ranks
            rows = [torch.log_softmax(s.float(), -1).numpy() for s in o.scores]
        else:
            rows = [s.numpy().astype(np.float32) for s in o.scores]
        st = BR.BeamState(B, K, MAX_NEW, eos_ids=eos, pad_id=PAD, length_penalty=lp, early_stopping=es)
        for r in rows:                                  # the no-tie condition, on the accumulated values HF ranked
            acc = (r.reshape(B, K, V) + st.run_score[:, :, None]).astype(np.float32).reshape(B, K * V)
            top = -np.sort(-acc, axis=-1)[:, :M + 1]
            top = np.where(np.isfinite(top), top, np.arange(M + 1)[None, :] * -1.0e30)
            if (np.diff(top, axis=-1) == 0).any():
                return None
            if st.step_rows(r) == 0:
                break
        tv = np.stack([-np.sort(-r, axis=-1)[:, :M] for r in rows])
        ti = np.stack([np.argsort(-r, axis=-1, kind="stable")[:, :M] for r in rows]).astype(np.int32)
        out[f"r{i}_sequences"] = o.sequences[:, L:].numpy()
        if K == 1:                                      # no sequence scores from greedy search; lengths = up to and including the first eos
            g = out[f"r{i}_sequences"]
            is_eos = np.isin(g, eos)
            lens = np.where(is_eos.any(-1), is_eos.argmax(-1) + 1, g.shape[1])
            out[f"r{i}_sequences_scores"] = np.zeros(0, np.float32)
            out[f"r{i}_beam_indices"] = np.where(np.arange(g.shape[1])[None, :] < lens[:, None], 0, -1).astype(np.int32)
        else:
            out[f"r{i}_sequences_scores"] = o.sequences_scores.numpy().astype(np.float32)
            out[f"r{i}_beam_indices"] = o.beam_indices.numpy().astype(np.int32)
        out[f"r{i}_top_val"], out[f"r{i}_top_idx"] = tv, ti
        meta.append(dict(K=K, length_penalty=lp, early_stopping=es, eos=eos, num_return_sequences=nrs, extra=extra))
        n_fin = int(np.isin(out[f"r{i}_sequences"], eos).any(-1).sum()) if eos else 0
        print(f"run {i}: K={K} lp={lp} es={es} eos={eos} nrs={nrs} steps={len(rows)} n_new={out[f'r{i}_sequences'].shape[1]} "
              f"returned with eos: {n_fin}/{B * nrs}", flush=True)
    out["meta"] = np.array(json.dumps(dict(V=V, L=L, B=B, max_new=MAX_NEW, pad=PAD, runs=meta)))
    return out


def main():
    for seed in range(64):
        out = attempt(seed)
        if out is not None:
            break
        print(f"seed {seed}: a tie or an unusable eos choice, next", flush=True)
    else:
        raise SystemExit("no seed without ties")
    path = os.path.join(ROOT, "tests", "golden", "beam_search.npz")
    np.savez_compressed(path, **out)
    print(f"seed {int(out['seed'])} -> {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
