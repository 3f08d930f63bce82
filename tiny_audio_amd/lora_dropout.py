"""LoRA dropout masks (peft ``LoraLayer`` with ``lora_dropout = p > 0``): the numpy twin of the device definition in
csrc/philox.h / include/ta355.h (``ta_lora_dropout``).

The keep decision of element (m, c) of linear j (peft order q, k, v, o, gate, up, down = 0..6) in decoder layer l is a pure
function of (seed, offset, l, j, m, c): Philox4x32-10 with counter ((8 l + j) << 20 | c >> 3, m, lo32(offset), hi32(offset)) and
key (lo32(seed), hi32(seed)); the 16-bit half (c & 1) of output word (c & 7) >> 1 is compared with round(p * 65536).  The drop
probability is therefore p rounded to a multiple of 2^-16; kept values are scaled by 1 / (1 - p) with p as given.
"""
from __future__ import annotations

import numpy as np

PEFT_ORDER = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over broadcastable uint32 arrays -> (w0, w1, w2, w3) uint32."""
    c = [np.asarray(v, dtype=np.uint32) for v in (c0, c1, c2, c3)]
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    c0, c1, c2, c3 = (v.copy() for v in (c0, c1, c2, c3))
    k0, k1 = np.uint32(k0), np.uint32(k1)
    lo = np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = _M0 * c0.astype(np.uint64)
            p1 = _M1 * c2.astype(np.uint64)
            n0 = (p1 >> np.uint64(32)).astype(np.uint32) ^ c1 ^ k0
            n1 = (p1 & lo).astype(np.uint32)
            n2 = (p0 >> np.uint64(32)).astype(np.uint32) ^ c3 ^ k1
            n3 = (p0 & lo).astype(np.uint32)
            c0, c1, c2, c3 = n0, n1, n2, n3
            k0 = np.uint32((int(k0) + int(_W0)) & 0xFFFFFFFF)
            k1 = np.uint32((int(k1) + int(_W1)) & 0xFFFFFFFF)
    return c0, c1, c2, c3


def threshold(p: float) -> int:
    """Drop iff the 16-bit draw is below this (p as the float32 the descriptor carries)."""
    return min(65535, int(float(np.float32(p)) * 65536.0 + 0.5))


def inv_keep(p: float) -> np.float32:
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


def keep_mask(p: float, seed: int, offset: int, layer: int, linear: int, M: int, n: int) -> np.ndarray:
    """bool [M, n]: True = element kept (every element when p == 0)."""
    if not float(np.float32(p)) > 0.0:
        return np.ones((M, n), dtype=bool)
    c8 = np.arange((n + 7) // 8, dtype=np.uint32)
    m = np.arange(M, dtype=np.uint32)[:, None]
    lj = np.uint32(8 * layer + linear)
    w = philox4x32_10((lj << np.uint32(20)) | c8[None, :], m, offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF,
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    words = np.stack(w, axis=-1)                                               # [M, n8, 4]
    halves = np.stack([words & np.uint32(0xFFFF), words >> np.uint32(16)], axis=-1).reshape(M, -1)   # [M, n8 * 8], column order
    return (halves >= threshold(p))[:, :n]
