"""Forced alignment: device time of one ta_ctc_align_f32 launch against the two things it replaces or competes with.

    python scripts/align_bench.py [--T 1499 --J 400 --C 29] [--out FILE.json]
    python scripts/align_bench.py --long [--tiles 256x256,512x512] [--out FILE.json]      (the long form: see long_main)

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
from tiny_audio_amd import _lib, ops  # noqa: E402


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


LONG_SHAPES = ((180000, 60000, 32), (32768, 2048, 32))      # an hour against its transcript; the corner of the short kernel's envelope
LONG_TILES = "128x128,128x256,192x128,256x64,256x96,256x128,256x256,256x512,512x256,512x512,1024x512,1024x1024,2048x1024"


def long_main(a):
    """--long: device time of one ops.ctc_align_long call (every launch of the wavefront plus the walk) for one clip at LONG_SHAPES, for
    every tile col_block x frame_block of --tiles and for the library's default (0x0).  HIP events around one call, workspace and
    frames allocated once outside; --warmup calls, then the median of --repeats.  At the corner of the old envelope the short kernel
    runs in the same process on the same inputs, and both are checked against align_ref; at the long shape, which the host cannot
    check in reasonable time, every tiling must give the first one's frames and score."""
    tiles = [tuple(int(x) for x in t.split("x")) for t in a.tiles.split(",")] + [(0, 0)]
    res = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, repeats=a.repeats, rows=[])
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    for T, J, C in LONG_SHAPES:
        e, tok, cu_f, cu_t = (x.cuda() for x in make(1, T, J, C))
        inside = T <= ops.ALIGN_LIMITS["frames"] and J <= ops.ALIGN_LIMITS["tokens"]
        want = None
        if inside:
            ref = align_ref.align(e.cpu().numpy(), tok.cpu().tolist(), fast=True)
            fr, sc, st, _ = ops.ctc_align(e, cu_f, tok, cu_t, 0, T, J)
            assert st.tolist() == [0] and fr.tolist() == ref["frames"] and sc[0].item() == float(ref["score"])
            want = (fr.clone(), sc.clone())
            frames = torch.empty_like(fr)
            k = time_events(lambda: ops.ctc_align(e, cu_f, tok, cu_t, 0, T, J, frames=frames), a.warmup, a.repeats)
            row = dict(T=T, J=J, C=C, kernel="ta_ctc_align_f32", ms=dict(median=k[0], min=k[1], max=k[2]))
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        for cb, fb in tiles:
            n = _lib.lib().ta_ctc_align_long_workspace_bytes(1, T, J, cb, fb)
            ws = torch.empty(n, dtype=torch.uint8, device="cuda")
            frames = torch.full((J,), -1, dtype=torch.int32, device="cuda")
            call = lambda: ops.ctc_align_long(e, cu_f, tok, cu_t, 0, T, J, col_block=cb, frame_block=fb, frames=frames, workspace=ws)
            _, sc, st, _ = call()
            if want is None:
                want = (frames.clone(), sc.clone())
            assert st.tolist() == [0] and torch.equal(frames, want[0]) and torch.equal(sc, want[1]), (T, J, cb, fb)
            k = time_events(call, a.warmup, a.repeats)
            row = dict(T=T, J=J, C=C, kernel="ta_ctc_align_long_f32", col_block=cb, frame_block=fb, workspace_bytes=n,
                       ms=dict(median=k[0], min=k[1], max=k[2]), ns_per_cell=k[0] * 1e6 / (T * (J + 1)))
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            del ws
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--long", action="store_true", help="time ta_ctc_align_long_f32 over --tiles at LONG_SHAPES instead")
    ap.add_argument("--tiles", default=LONG_TILES, help="col_block x frame_block tiles of --long, comma separated")
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
    if a.long:
        return long_main(a)
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
