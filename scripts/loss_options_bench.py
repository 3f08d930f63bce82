"""Cost of the LM loss options in the cross-entropy launch at the benchmarked shape: bf16 logits, V = 151 936, the label rows of the
bench.py step (--batch clips x --labels-per-clip label positions), nll + loss + bf16 dlogits written.  ``ta_cross_entropy`` (options
off) against ``ta_cross_entropy_opt`` with --eps / --zc and the per-row objective buffer, in ONE process, device events around each call
(the row kernel and the ordered sum), legs alternating with the order swapped every pair.  Prints one JSON line.

    python scripts/loss_options_bench.py [--pairs 40] [--warmup 5] [--batch 32] [--labels-per-clip 36] [--eps 0.1] [--zc 1e-4]

The other half of profiles/loss_options.md, options off against the previous library, needs no script: build the previous commit,
then run ``bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs DIR`` (compare the four .npy files) and
``bench.py --gpus 1 --steps 20 --warmup 5`` (alternating) once as they are and once with ``TA355_LIB=<the previous libta355.so>``.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--labels-per-clip", type=int, default=36)
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--zc", type=float, default=1e-4)
    a = ap.parse_args()
    from tiny_audio_amd import _lib
    from tiny_audio_amd.ops import ptr, stream

    dev = torch.device("cuda", 0)
    n, V = a.batch * a.labels_per_clip, a.vocab
    g = torch.Generator(device=dev).manual_seed(0)
    z = (torch.randn(n, V, device=dev, generator=g) * 3).to(torch.bfloat16)
    t = torch.randint(0, V, (n,), device=dev, generator=g)
    nll, obj, loss = torch.empty(n, device=dev), torch.empty(n, device=dev), torch.zeros(1, device=dev)
    dl = torch.empty(n, V, device=dev, dtype=torch.bfloat16)
    L = _lib.lib()
    opt = _lib.CeOptions(eps=a.eps, zc=a.zc, obj=obj.data_ptr())

    def off():
        _lib.check(L.ta_cross_entropy(ptr(z), 1, V, None, ptr(t), n, V, 1.0 / n, ptr(nll), ptr(loss), ptr(dl), V, stream()), "ta_cross_entropy")

    def on():
        _lib.check(L.ta_cross_entropy_opt(ptr(z), 1, V, None, ptr(t), n, V, 1.0 / n, ptr(nll), ptr(loss), ptr(dl), V, C.byref(opt), stream()),
                   "ta_cross_entropy_opt")

    for _ in range(a.warmup):
        off(); on()
    torch.cuda.synchronize()
    times = {"off": [], "on": []}
    for rep in range(a.pairs):
        for name, fn in ((("off", off), ("on", on)) if rep % 2 == 0 else (("on", on), ("off", off))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    nbytes = n * V * 2 * 3                                            # the logits read twice, dlogits written once
    out = {"n_rows": n, "V": V, "bytes": nbytes, "eps": a.eps, "zc": a.zc}
    for k, v in times.items():
        v = np.array(v)
        out[k] = dict(median_us=float(np.median(v)), min_us=float(v.min()), p10_us=float(np.percentile(v, 10)),
                      p90_us=float(np.percentile(v, 90)), gbps_median=float(nbytes / np.median(v) / 1e3))
    out["on_over_off_median"] = out["on"]["median_us"] / out["off"]["median_us"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
