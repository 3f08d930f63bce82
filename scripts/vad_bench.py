"""Voice activity detection on a synthetic hour: what the two launches of ``ta_vad_f32`` cost, next to the numpy restatement on the host.

    python scripts/vad_bench.py [--minutes 60] [--snr 10] [--iters 20] [--warmup 5] [--no-host]

Workload: one synthetic minute (tests/vad_ref.synth: harmonic bursts in white noise at ``--snr`` dB) repeated ``--minutes`` times, one
recording, uploaded once.  Printed, one JSON object per line:
  * the device: HIP events around each of ``--iters`` calls of ``ta_vad_f32`` (both launches: band energies, then the fused statistic)
    on preallocated outputs and workspace after ``--warmup`` calls; median, min, max in ms; frames per second; the audio read per
    second (4 n bytes over the median);
  * the host: tests/vad_ref.py's float32 restatement, one run (numpy, as many threads as its BLAS takes), and the device's distance
    from the float64 reference on the same hour: the largest |L_dev - L64| / (L64 + theta), the frames inside the decision band, and
    the flags that differ outside it.
There is no counterpart in the parent commit: the time is reported (profiles/vad.md), not gated.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import vad_ref as R  # noqa: E402
from tiny_audio_amd import _lib, longform, ops  # noqa: E402
from tiny_audio_amd.vad import DeviceVAD  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=int, default=60)
    ap.add_argument("--snr", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    x = np.tile(R.synth(0, 60.0, a.snr, "white")[0], a.minutes)
    n, F = len(x), R.frames_of(len(x))
    vad = DeviceVAD()
    h, W, beta, theta, e0 = vad.options()
    flat, off, lens = longform.upload([x])
    L = _lib.lib()
    ws_bytes = L.ta_vad_workspace_bytes(1, n)
    ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
    stat = torch.zeros((1, F), device="cuda")
    flags = torch.zeros((1, F), device="cuda", dtype=torch.uint8)
    nf = torch.zeros(1, device="cuda", dtype=torch.int32)
    opt = _lib.VadOptions(h, W, beta, theta, e0)

    def call():
        _lib.check(L.ta_vad_f32(ops.ptr(flat), ops.ptr(off), 1, n, C.byref(opt), ops.ptr(stat), ops.ptr(flags), F, ops.ptr(nf), ops.ptr(ws),
                                ws_bytes, ops.stream()), "ta_vad_f32")

    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        call()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    med = statistics.median(ms)
    res = dict(device=torch.cuda.get_device_name(0), minutes=a.minutes, samples=n, frames=F, options=dict(h=h, W=W, beta=beta, theta=theta, e0=e0),
               vad_ms=dict(median=med, min=min(ms), max=max(ms)), iters=a.iters, warmup=a.warmup, frames_per_s=F / (med * 1e-3),
               audio_tb_per_s=4.0 * n / (med * 1e-3) / 1e12, audio_hours_per_s=n / 16000 / 3600 / (med * 1e-3), workspace_mb=ws_bytes / 2 ** 20,
               speech_frames=int(flags.sum()))
    print(json.dumps(res), flush=True)
    if a.no_host:
        return
    t0 = time.perf_counter()
    L32 = R.statistic(x, h, W, beta, theta, e0, dtype=np.float32)
    host_s = time.perf_counter() - t0
    L64 = R.statistic(x, h, W, beta, theta, e0)
    Ld, fd = stat[0].cpu().numpy().astype(np.float64), flags[0].cpu().numpy().astype(bool)
    band = R.in_band(L64, theta)
    print(json.dumps(dict(host_float32_restatement_s=host_s, host_over_device=host_s / (med * 1e-3),
                          device_error=float(np.max(np.abs(Ld - L64) / (L64 + theta))), e32=float(np.max(np.abs(L32 - L64) / (L64 + theta))),
                          frames_in_band=int(band.sum()), flags_differing_outside_band=int(((fd != R.flags_of(L64, theta)) & ~band).sum()),
                          n_frames=int(nf[0]))), flush=True)


if __name__ == "__main__":
    main()
