"""Text alignment: device time of ta_text_align_i32 on the three scales it is meant for.

    python scripts/text_align_bench.py [--workloads utterances,hour,limit] [--tiles 256x256,512x512] [--mode edit|lcs] [--out FILE.json]

  * utterances: 4 096 pairs of 10 to 60 words, with paths -- an evaluation set in one call (the short kernel);
  * hour:       one 32 768 x 32 768 pair, with path -- a 2.9 h transcript (the long kernel; every tile of --tiles and the default 0x0);
  * limit:      one 262 144 x 262 144 pair, distance only -- the envelope (the same tiles).
A hypothesis is its reference with about one word in ten substituted, dropped or followed by an extra one, over a vocabulary of 5 000
ids.  HIP events around one ops.text_align call, the workspace and map allocated once outside; --warmup calls, then the median of
--repeats (7).  Reported: ms and cells/s (sum of n x m over the pairs / time).  For the first two workloads the wall time of
tests/text_align_ref.py's numpy row scan on the same inputs is reported next to it (utterances: with the walk, every pair checked
against it; hour: the distance alone -- two boolean planes of 1 GiB are not kept -- and the device's counts are checked by their
identities); every tiling must give the first one's bytes.  Results: profiles/text_align.md.
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

from tests import text_align_ref as R  # noqa: E402
from tiny_audio_amd import ops  # noqa: E402

VOCAB = 5000


def noisy_copy(rng, ref, rate=0.1):
    """About ``rate`` of the words substituted, dropped, or followed by an inserted one (a third each)."""
    kind = rng.random(len(ref))
    out = []
    for w, k in zip(ref.tolist(), kind):
        if k < rate / 3:
            out.append(int(rng.integers(0, VOCAB)))
        elif k < 2 * rate / 3:
            continue
        elif k < rate:
            out += [w, int(rng.integers(0, VOCAB))]
        else:
            out.append(w)
    return np.asarray(out, np.int32)


def make_pairs(rng, lens):
    refs = [rng.integers(0, VOCAB, n).astype(np.int32) for n in lens]
    return refs, [noisy_copy(rng, r) for r in refs]


def square_pair(rng, n):
    """One n x n pair: the noisy copy cut or padded to n symbols, so that both sides sit exactly at the size under test."""
    r = rng.integers(0, VOCAB, n).astype(np.int32)
    h = noisy_copy(rng, r)
    h = np.concatenate([h, rng.integers(0, VOCAB, max(0, n - len(h))).astype(np.int32)])[:n]
    return [r], [h]


def time_events(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def device_batch(refs, hyps):
    r, cu_r = R.ragged(refs)
    h, cu_h = R.ragged(hyps)
    t = lambda x: torch.from_numpy(x).cuda()                                                   # noqa: E731
    return t(r), t(cu_r), t(h), t(cu_h), torch.from_numpy(cu_r), torch.from_numpy(cu_h)


def bench(name, refs, hyps, mode, want_path, tiles, a, res):
    r, cu_r, h, cu_h, cu_r_host, cu_h_host = device_batch(refs, hyps)
    max_n, max_m = max(len(x) for x in refs), max(len(x) for x in hyps)
    cells = sum(len(x) * len(y) for x, y in zip(refs, hyps))
    first = None
    for cb, rb in tiles:
        need = ops.text_align_workspace_bytes(cu_r_host, cu_h_host, max_n, max_m, want_path, cb, rb)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        mp = torch.full((r.numel(),), -1, dtype=torch.int32, device="cuda") if want_path else None
        call = lambda: ops.text_align(r, cu_r, h, cu_h, max_n, max_m, mode, want_path, col_block=cb, row_block=rb, map=mp,   # noqa: E731
                                      workspace=ws)
        dist, counts, _, st = call()
        got = (dist.cpu().numpy(), counts.cpu().numpy(), mp.cpu().numpy() if want_path else None)
        assert not st.any(), (name, cb, rb)
        if first is None:
            first = got
        assert all(x is None or x.tobytes() == y.tobytes() for x, y in zip(got, first)), (name, cb, rb)
        k = time_events(call, a.warmup, a.repeats)
        row = dict(workload=name, pairs=len(refs), max_n=max_n, max_m=max_m, mode=("edit", "lcs")[mode], want_path=want_path, col_block=cb,
                   row_block=rb, workspace_bytes=need, cells=cells, ms=dict(median=k[0], min=k[1], max=k[2]), cells_per_s=cells / (k[0] * 1e-3))
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        del ws
    return first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="utterances,hour,limit")
    ap.add_argument("--tiles", default="128x128,256x256,512x256,512x512,512x1024", help="col_block x row_block tiles of the long kernel")
    ap.add_argument("--mode", default="edit", choices=("edit", "lcs"))
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-ref", action="store_true", help="skip the numpy row scan of tests/text_align_ref.py")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mode = R.EDIT if a.mode == "edit" else R.LCS
    tiles = [tuple(int(x) for x in t.split("x")) for t in a.tiles.split(",") if t] + [(0, 0)]
    res = dict(device=torch.cuda.get_device_name(0), warmup=a.warmup, repeats=a.repeats, rows=[])
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    rng = np.random.default_rng(0)
    work = a.workloads.split(",")
    if "utterances" in work:
        refs, hyps = make_pairs(rng, rng.integers(10, 61, 4096))
        dist, counts, mp = bench("utterances", refs, hyps, mode, True, [(0, 0)], a, res)
        if not a.no_ref:
            t0 = time.perf_counter()
            want = R.align_batch(refs, hyps, mode)
            row = dict(workload="utterances", numpy_row_scan_s=time.perf_counter() - t0)
            assert all(np.array_equal(x, y) for x, y in zip((dist, counts, mp), want))
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    if "hour" in work:
        refs, hyps = square_pair(rng, 32768)
        dist, counts, mp = bench("hour", refs, hyps, mode, True, tiles, a, res)
        H, S, D, I = counts[0].tolist()
        assert H + S + D == 32768 and H + S + I == 32768 and (mode == R.LCS or S + D + I == dist[0]) and (mp >= 0).sum() == H + S
        if not a.no_ref:
            t0 = time.perf_counter()
            want = R.align(refs[0], hyps[0], mode, want_path=False)[0]
            row = dict(workload="hour", numpy_row_scan_distance_only_s=time.perf_counter() - t0)
            assert want == dist[0]
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    if "limit" in work:
        refs, hyps = square_pair(rng, 262144)
        bench("limit", refs, hyps, mode, False, tiles, a, res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
