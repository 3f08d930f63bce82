"""Generates tests/golden/lora_dropout_small.npz: stage-2 LoRA with peft's ``lora_dropout`` p > 0 on the SMALL LM config.

peft is not installed offline, so (as ``make_golden.gen_lora``) the adapters are applied to transformers' Qwen3 functionally --
but they cannot be merged into the weights: every targeted Linear j of layer l adds  s * ((x * K_j / (1 - p)) @ A_j^T) @ B_j^T
(peft LoraLayer.forward in training mode) through a forward hook, with the keep masks K_j of the numpy twin
tiny_audio_amd/lora_dropout.py (row m = b * L + t of the [B*L] row space).  torch autograd gives d loss / d inputs_embeds and the
adapter gradients.  lora_B is initialised NON-zero so that dA and the masked d(x) term are not trivially zero.

Run from the repository root on the build machine:  python tests/golden/make_lora_dropout_fixture.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_golden import build_lm, save, t  # noqa: E402
from tests.golden.recipe import SMALL, lm_input  # noqa: E402
from tiny_audio_amd import lora_dropout as LD  # noqa: E402

# (prefix, rank, alpha, targets (None = all 7), p, seed, offset)
CASES = (("c0", 8, 32, None, 0.1, 1234, 5),
         ("c1", 4, 16, ("q_proj", "v_proj"), 0.3, 0x9E3779B97F4A7C15 & 0x7FFFFFFFFFFFFFFF, (3 << 32) + 2))


def adapters(cfg, rank, targets):
    """oracle init_lora's A, and a deterministic NON-zero B (tests/test_gpu_lora_dropout.py rebuilds the same)."""
    from oracle import weights as OW
    lo = OW.init_lora(cfg, rank=rank, seed=4, targets=targets)
    for i, k in enumerate(sorted(lo)):
        if k.endswith(".lora_B"):
            lo[k] = (np.random.RandomState(100 + i).standard_normal(lo[k].shape) * 0.05).astype(np.float32)
    return lo


def run_case(m, cfg, rank, alpha, targets, p, seed, offset):
    lo = {k: t(v).requires_grad_(True) for k, v in adapters(cfg, rank, targets).items()}
    s = float(alpha) / rank
    x, att, lab = lm_input()
    B, L, _ = x.shape
    hooks = []
    for name, mod in m.named_modules():
        if not isinstance(mod, torch.nn.Linear) or f"{name}.lora_A" not in lo:
            continue
        layer = int(name.split("layers.")[1].split(".")[0])
        j = LD.PEFT_ORDER.index(name.rsplit(".", 1)[1])
        A, Bm = lo[f"{name}.lora_A"], lo[f"{name}.lora_B"]
        keep = torch.from_numpy(LD.keep_mask(p, seed, offset, layer, j, B * L, mod.in_features).astype(np.float32))
        scale = float(LD.inv_keep(p))

        def hook(mod_, inp, out, A=A, Bm=Bm, keep=keep, scale=scale):
            xin = inp[0].reshape(B * L, -1)
            return out + (s * (((xin * keep * scale) @ A.t()) @ Bm.t())).reshape(out.shape)
        hooks.append(mod.register_forward_hook(hook))
    xt = t(x).requires_grad_(True)
    out = m(inputs_embeds=xt, attention_mask=t(att), labels=t(lab))
    out.loss.backward()
    for h in hooks:
        h.remove()
    keep_keys = [k for k in lo if ".layers.0." in k or ".layers.1.self_attn" in k or ".layers.1.mlp.down_proj" in k]
    return out.loss.detach().numpy(), xt.grad.numpy(), {k: lo[k].grad.numpy() for k in keep_keys}


def main():
    from oracle import weights as OW
    cfg = SMALL["lm"]
    m = build_lm(cfg, OW.init_lm(cfg, seed=1))
    m.requires_grad_(False)
    arrays = {}
    for pre, rank, alpha, targets, p, seed, offset in CASES:
        loss, dx, grads = run_case(m, cfg, rank, alpha, targets, p, seed, offset)
        arrays.update({f"{pre}.loss": loss, f"{pre}.dx": dx, f"{pre}.p": np.float32(p), f"{pre}.seed": np.uint64(seed),
                       f"{pre}.offset": np.uint64(offset), f"{pre}.rank": np.int64(rank), f"{pre}.alpha": np.int64(alpha)})
        arrays.update({f"{pre}.g.{k}": v for k, v in grads.items()})
    save("lora_dropout_small.npz", **arrays)


if __name__ == "__main__":
    main()
