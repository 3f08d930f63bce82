"""Forced alignment: device time of one ta_ctc_align_f32 launch against the two things it replaces or competes with.

    python scripts/align_bench.py [--T 1499 --J 400 --C 29] [--out FILE.json]

For N = 1 and N = 32 clips of (T, J, C) -- a 30 s clip of wav2vec2 frames against about 400 characters:
  * kernel:   one launch (trellis + backtrack) through ops.ctc_align; HIP events around --inner back-to-back launches, divided by
              --inner; median of --repeats such measurements after --warmup launches.  Also with --inner 1 (one launch alone between
              the events, the launch latency and the wrapper's host work included);
  * torch:    the obvious device formulation, one shifted ``maximum`` per frame over a [N, J + 1] row (T x a few launches), trellis
              only, no backtrack -- the bar the kernel has to beat, since it makes one launch against thousands;
  * loop:     tests/align_ref.py's literal double loop for ONE clip on this box's CPU: the stand-in for the reference's Python loop.
The kernel's frames and score are checked against align_ref before anything is timed.  Results: profiles/forced_alignment.md.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import align_ref  # noqa: E402
from tiny_audio_amd import ops  # noqa: E402


def make(N, T, J, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    e = torch.log_softmax(torch.randn(N * T, C, generator=g), dim=-1)
    tok = torch.randint(1, C, (N * J,), generator=g, dtype=torch.int32)
    cu_f = torch.arange(N + 1, dtype=torch.int32) * T
    cu_t = torch.arange(N + 1, dtype=torch.int32) * J
    return e, tok, cu_f, cu_t


def time_events(fn, warmup, repeats, inner=1):
    """Median / min / max ms of one ``fn()``; ``inner`` calls sit between the two events so that the queue stays full and the host's
    share of a call (the wrapper allocates the workspace, score and status with torch.empty) is hidden behind the device's."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return statistics.median(ms), min(ms), max(ms)


def torch_trellis(e, tok, N, T, J):
    """[N, T, C] emissions, [N, J] tokens -> the last trellis row [N, J + 1]; T steps of gather + add + add + maximum."""
    e3 = e.view(N, T, -1)
    idx = tok.view(N, J).long()
    row = torch.full((N, J + 1), -float("inf"), device=e.device)
    row[:, 0] = 0
    neg = torch.full((N, 1), -float("inf"), device=e.device)
    for t in range(T):
        et = e3[:, t]
        stay = row + et[:, :1]
        move = torch.cat([neg, row[:, :-1] + et.gather(1, idx)], dim=1)
        row = torch.maximum(stay, move)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1499)
    ap.add_argument("--J", type=int, default=400)
    ap.add_argument("--C", type=int, default=29)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--torch-repeats", type=int, default=5)
    ap.add_argument("--no-loop", action="store_true", help="skip the CPU loop of align_ref")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T, J, C = a.T, a.J, a.C
    res = dict(T=T, J=J, C=C, device=torch.cuda.get_device_name(0), kernel_warmup=a.warmup, kernel_repeats=a.repeats, kernel_inner=a.inner,
               torch_warmup=1, torch_repeats=a.torch_repeats, rows=[])
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    for N in (1, 32):
        e, tok, cu_f, cu_t = (x.cuda() for x in make(N, T, J, C))
        fr, sc, st, _ = ops.ctc_align(e, cu_f, tok, cu_t, 0, T, J)
        ref = align_ref.align(e[:T].cpu().numpy(), tok[:J].cpu().tolist(), fast=True)
        assert st.tolist() == [0] * N and fr[:J].tolist() == ref["frames"] and sc[0].item() == float(ref["score"])
        frames = torch.empty_like(fr)
        k = time_events(lambda: ops.ctc_align(e, cu_f, tok, cu_t, 0, T, J, frames=frames), a.warmup, a.repeats, a.inner)
        k1 = time_events(lambda: ops.ctc_align(e, cu_f, tok, cu_t, 0, T, J, frames=frames), 0, a.repeats)
        last = torch_trellis(e, tok, N, T, J)
        assert torch.equal(last[:, J], sc), "the torch formulation computes the same scores"
        tt = time_events(lambda: torch_trellis(e, tok, N, T, J), 1, a.torch_repeats)
        row = dict(N=N, kernel_ms=dict(median=k[0], min=k[1], max=k[2]), kernel_single_launch_ms=dict(median=k1[0], min=k1[1], max=k1[2]),
                   torch_ms=dict(median=tt[0], min=tt[1], max=tt[2]),
                   cells=N * T * (J + 1), kernel_ns_per_frame=k[0] * 1e6 / T, speedup_vs_torch=tt[0] / k[0])
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    if not a.no_loop:
        e, tok, _, _ = make(1, T, J, C)
        t0 = time.perf_counter()
        align_ref.align(e.numpy(), tok.tolist())
        res["cpu_literal_loop_s"] = time.perf_counter() - t0
        print(json.dumps(dict(cpu_literal_loop_s=res["cpu_literal_loop_s"])), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
