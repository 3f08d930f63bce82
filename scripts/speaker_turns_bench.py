"""Speaker turns on a synthetic meeting: what ``spk_vote``, ``spk_merge`` and ``spk_words`` cost, next to the host functions they restate.

    python scripts/speaker_turns_bench.py [--hours 1.0] [--iters 20] [--warmup 5] [--no-host] [--cap]

Workload: ``--hours`` of two to four speakers in turns of 2 to 20 s with pauses of 0.2 to 2 s (seeded); windows of 0.75 s at 0.15 s
steps inside every turn, labelled with the truth; VAD decisions from the truth (speech inside the turns); about 2.5 words of 0.3 s per
second of speech.  Printed, one JSON object per line:
  * the device: for each of the three entry points, HIP events around 20 back-to-back calls on preallocated buffers, ``--iters`` times
    after ``--warmup`` calls; median, min and max per call in ms (``spk_vote`` is one memset and three launches, the other two one launch each), and whether the
    turns and the words' speakers equal the host's (``--no-host`` skips the host and the comparison);
  * the host: ``LocalSpeakerDiarizer._postprocess_segments`` and ``assign_speakers_to_words`` as they are, one run each, seconds;
  * ``--cap``: the same device calls on a recording at the 2.9 h cap (1 048 577 voting frames), device only.
There is no device counterpart in the parent commit: the times are reported (profiles/speaker_turns.md), not gated.
"""
import argparse
import copy
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

from tiny_audio_amd import _lib, ops  # noqa: E402
from tiny_audio_amd.diarization import LocalSpeakerDiarizer as L  # noqa: E402

DEV = "cuda"


def meeting(seconds: float, seed: int = 0):
    """-> (window dicts, labels, total duration, vad decisions, word dicts)."""
    rng = np.random.default_rng(seed)
    n_spk = int(rng.integers(2, 5))
    turns, t = [], 0.3
    while True:
        d = float(rng.uniform(2.0, 20.0))
        if t + d > seconds - 0.3:
            break
        turns.append((int(rng.integers(0, n_spk)), t, t + d))
        t += d + float(rng.uniform(0.2, 2.0))
    wins, labels, words = [], [], []
    for k, a, b in turns:
        s = np.arange(a, b - 0.75, 0.15)
        wins += [{"start": float(x), "end": float(x + 0.75)} for x in s]
        labels += [k] * len(s)
        w = np.arange(a + 0.05, b - 0.35, 0.4)
        words += [{"word": "w", "start": float(x), "end": float(x + 0.3)} for x in w]
    mid = (np.arange(int(seconds * 16000 - 1) // 256) * 256 + 128) / 16000
    starts, ends = np.array([a for _, a, _ in turns]), np.array([b for _, _, b in turns])
    i = np.searchsorted(starts, mid, side="right") - 1
    vad = (i >= 0) & (mid < ends[np.maximum(i, 0)])
    return wins, np.array(labels), float(seconds), vad.tolist(), words


def timed(call, iters, warmup, reps=20):
    """HIP events around ``reps`` back-to-back calls, ``iters`` times after ``warmup`` calls -> ms per call: median, min, max."""
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            call()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1) / reps)
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def device_side(wins, labels, duration, vad, words, iters, warmup):
    """The three entry points of the C ABI on preallocated buffers (no Python-side check or read-back inside the timed window)."""
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)  # noqa: E731
    f64 = lambda a: torch.tensor(a, dtype=torch.float64, device=DEV)  # noqa: E731
    lib, ptr, st = ops.lib(), ops.ptr, ops.stream
    first, last, rank, names, n_frames = L.vote_inputs(wins, labels, duration)
    v = np.asarray(vad, bool)
    cap = min(2 * len(first) + int(np.count_nonzero(v[1:] != v[:-1])) + 2, n_frames)
    opt = _lib.SpkPostOptions(*L.spk_options())
    S, nw = len(names), len(first)
    first_d, last_d, rank_d, cu_win, nf_d = i32(first), i32(last), i32(rank), i32([0, nw]), i32([n_frames])
    vad_d, n_vad, cu_cap = torch.from_numpy(v.astype(np.uint8)[None]).to(DEV).contiguous(), i32([len(v)]), i32([0, cap])
    runs = tuple(torch.zeros(cap, dtype=torch.int32, device=DEV) for _ in range(3))
    segs = tuple(torch.zeros(cap, dtype=torch.int32, device=DEV) for _ in range(3))
    n_runs, status, n_seg = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(3))
    ws_bytes = lib.ta_spk_post_workspace_bytes(1, S, n_frames, nw)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)

    def vote():
        _lib.check(lib.ta_spk_vote_i32(ptr(first_d), ptr(last_d), ptr(rank_d), ptr(cu_win), nw, 1, S, ptr(nf_d), n_frames, ptr(vad_d), len(v),
                                       ptr(n_vad), C.byref(opt), ptr(cu_cap), ptr(runs[0]), ptr(runs[1]), ptr(runs[2]), ptr(n_runs), ptr(status),
                                       ptr(ws), ws_bytes, st()), "ta_spk_vote_i32")

    def merge():
        _lib.check(lib.ta_spk_merge_i32(ptr(runs[0]), ptr(runs[1]), ptr(runs[2]), ptr(cu_cap), ptr(n_runs), 1, C.byref(opt), ptr(segs[0]),
                                        ptr(segs[1]), ptr(segs[2]), ptr(n_seg), st()), "ta_spk_merge_i32")

    out = dict(spk_vote_ms=timed(vote, iters, warmup), spk_merge_ms=timed(merge, iters, warmup))
    k = int(n_seg.cpu()[0])
    turns = L.turns_from_frames(segs[0][:k].cpu().numpy(), segs[1][:k].cpu().numpy(), segs[2][:k].cpu().numpy(), names)
    ws_d, we_d, cu_w = f64([w["start"] for w in words]), f64([w["end"] for w in words]), i32([0, len(words)])
    ss_d, se_d, cu_s = f64([s["start"] for s in turns]), f64([s["end"] for s in turns]), i32([0, len(turns)])
    idx = torch.zeros(len(words), dtype=torch.int32, device=DEV)

    def assign():
        _lib.check(lib.ta_spk_words_f64(ptr(ws_d), ptr(we_d), ptr(cu_w), ptr(ss_d), ptr(se_d), ptr(cu_s), 1, len(words), ptr(idx), st()),
                   "ta_spk_words_f64")

    out["spk_words_ms"] = timed(assign, iters, warmup)
    out.update(windows=nw, voting_frames=n_frames, vad_frames=len(v), runs=int(n_runs.cpu()[0]), turns=k, words=len(words), speakers=S,
               status=int(status.cpu()[0]), workspace_mb=ws_bytes / 2 ** 20)
    return out, turns, [turns[g]["speaker"] if g >= 0 else None for g in idx.cpu().tolist()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--cap", action="store_true")
    a = ap.parse_args()
    case = meeting(a.hours * 3600.0)
    dev, turns, speakers = device_side(*case, a.iters, a.warmup)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), hours=a.hours, iters=a.iters, warmup=a.warmup, **dev)), flush=True)
    if not a.no_host:
        wins, labels, duration, vad, words = case
        t0 = time.perf_counter()
        host_turns = L._postprocess_segments(wins, labels, duration, vad)
        t1 = time.perf_counter()
        host_words = L.assign_speakers_to_words(copy.deepcopy(words), host_turns)
        t2 = time.perf_counter()
        print(json.dumps(dict(host_postprocess_s=t1 - t0, host_assign_words_s=t2 - t1, turns_equal=host_turns == turns,
                              words_equal=[w["speaker"] for w in host_words] == speakers,
                              host_over_device=(t2 - t0) / (1e-3 * (dev["spk_vote_ms"]["median"] + dev["spk_merge_ms"]["median"] + dev["spk_words_ms"]["median"])))),
              flush=True)
    if a.cap:
        cap_s = (ops.SPK_LIMITS["frames"] - 1) * L.VOTING_RATE - 0.005
        dev, _, _ = device_side(*meeting(cap_s, seed=1), a.iters, a.warmup)
        print(json.dumps(dict(at_the_cap=True, seconds=cap_s, **dev)), flush=True)


if __name__ == "__main__":
    main()
