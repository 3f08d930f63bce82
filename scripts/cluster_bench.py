#!/usr/bin/env python
"""Spectral clustering of N window embeddings: the host ``SpectralCluster`` (the reference's dense float64 chain, unchanged) against
``DeviceSpectralCluster`` on the GPU, run alternately in one process on the same seeded embeddings.

    python scripts/cluster_bench.py --sizes 2048 4000 8000 16000 --reps 3 --skip-host-above 8000 --markdown out.md

Per N it prints one JSON line:
  host_s           wall time of ``SpectralCluster.__call__`` (affinity, pruning, Laplacian, eigh, k-means), every repetition
  device_s         wall time of ``DeviceSpectralCluster.__call__`` ending in a device synchronise -- upload, kernels, the host's
                   Cholesky factors, Rayleigh-Ritz and k-means included --, every repetition after one warm-up call
  phases_ms        HIP events around ``spk_affinity`` phase 1 (normalise + cosine), 2 (threshold and cut), 4 (symmetrise + degrees);
                   the Lanczos steps and the Rayleigh-Ritz checks from the driver's host clocks (both end in synchronisations)
  lapmul           the Laplacian product on a 16-column block alone: HIP events around 20 launches; bytes = the one pass over W
                   (4 N^2) it needs, GB/s against the 8 TB/s HBM figure the project uses.  W at N <= 8000 fits the 256 MB Infinity
                   Cache, so only the largest sizes say anything about HBM
  same_partition   the two label vectors are the same partition (where the host ran)
It needs a GPU: there is no CPU path to time."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBPS = 8.0


def embeddings(n, speakers=6, noise=1.6, seed=0, dim=192):
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((speakers, dim))
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    x = cent[rng.integers(0, speakers, size=n)] + noise * rng.standard_normal((n, dim)) / np.sqrt(dim)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def events_ms(fn, reps=1):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4000, 8000, 16000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-host-above", type=int, default=8000, help="the host leg passes a minute beyond this")
    ap.add_argument("--markdown", default=None, help="also write the table here")
    args = ap.parse_args()
    import torch
    from tiny_audio_amd import ops
    from tiny_audio_amd.diarization import SpectralCluster
    from tiny_audio_amd.spectral import DeviceSpectralCluster
    if not torch.cuda.is_available():
        raise SystemExit("cluster_bench.py measures on a GPU; none is visible")
    rows = []
    for n in args.sizes:
        E = embeddings(n, seed=n)
        E64 = E.astype(np.float64)
        dev = DeviceSpectralCluster(2, 10, device="cuda", min_rows=0)
        host = SpectralCluster(2, 10)
        dev(E64)                                                               # warm-up: code objects, allocator
        torch.cuda.synchronize()
        host_s, device_s, infos, same = [], [], [], None
        for _ in range(args.reps):
            t = time.perf_counter()
            ld = dev(E64)
            torch.cuda.synchronize()
            device_s.append(time.perf_counter() - t)
            infos.append(dict(dev.last_info))
            if n <= args.skip_host_above:
                t = time.perf_counter()
                lh = host(E64.copy())
                host_s.append(time.perf_counter() - t)
                same = bool(same_partition(ld, lh)) if same is None else (same and bool(same_partition(ld, lh)))
        e = torch.from_numpy(E).cuda()
        keep = ops.spk_keep(n, 0.06)
        W, deg, _ = ops.spk_affinity(e, keep)
        ph = {"affinity": events_ms(lambda: ops.spk_affinity(e, keep, out=W, deg=deg, phases=1)),
              "threshold": events_ms(lambda: ops.spk_affinity(e, keep, out=W, deg=deg, phases=2)),
              "symmetrise": events_ms(lambda: ops.spk_affinity(e, keep, out=W, deg=deg, phases=4))}
        X = torch.randn(n, 16, device="cuda")
        Y = torch.empty_like(X)
        ops.spk_laplacian_matmul(W, deg, X, out=Y)
        lap_ms = events_ms(lambda: ops.spk_laplacian_matmul(W, deg, X, out=Y), reps=20)
        best = int(np.argmin(device_s))
        info = infos[best]
        ph["lanczos_steps"] = 1e3 * info.get("t_steps", float("nan"))
        ph["ritz"] = 1e3 * info.get("t_ritz", float("nan"))
        row = dict(N=n, keep=keep, host_s=host_s, device_s=device_s, path=info.get("path"), reason=info.get("reason"), k=info.get("k"),
                   blocks=info.get("blocks"), max_residual=info.get("max_residual"), tol=info.get("tol"), phases_ms=ph,
                   lapmul=dict(ms=lap_ms, gbps=4.0 * n * n / (lap_ms * 1e-3) / 1e9, frac_of_hbm=4.0 * n * n / (lap_ms * 1e-3) / (HBM_TBPS * 1e12)),
                   same_partition=same)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write("| N | host s (min) | device s (min) | speed-up | path | blocks | affinity ms | threshold ms | symmetrise ms | Lanczos steps ms | Ritz ms | "
                    "L X (p = 16) ms | GB/s | of 8 TB/s | same partition |\n|" + "---:|" * 15 + "\n")
            for r in rows:
                h = min(r["host_s"]) if r["host_s"] else None
                d = min(r["device_s"])
                p = r["phases_ms"]
                f.write(f"| {r['N']} | {'not run' if h is None else f'{h:.2f}'} | {d:.3f} | {'-' if h is None else f'{h / d:.1f}x'} | {r['path']} | "
                        f"{r['blocks']} | {p['affinity']:.3f} | {p['threshold']:.3f} | {p['symmetrise']:.3f} | {p['lanczos_steps']:.1f} | {p['ritz']:.1f} | "
                        f"{r['lapmul']['ms']:.4f} | {r['lapmul']['gbps']:.0f} | {r['lapmul']['frac_of_hbm']:.2f} | {r['same_partition']} |\n")


if __name__ == "__main__":
    main()
