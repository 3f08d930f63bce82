"""Per-stage cost of the device-side waveform augmentation at the production batch: B = 32 clips of 10 s, impulse responses of 1 s
and 2 s, every stage on for every clip, then each stage alone, then all stages off (the copy); then the three members that
``DeviceProductionAugment`` adds (short noises, EQ, band-limit) each alone on every clip, the whole chain on every clip, and the whole
chain with each stage drawn at the production recipe's probability (configs/training/production.yaml:67-140).  The cascade kernel is also
timed by itself (after a copy of the batch, which is timed beside it) in its time-parallel form and in the one-thread-per-clip form of
the same kernel (chunk length = the clip).  Device events around ``--iters``
calls after ``--warmup`` calls; the log-mel of the same batch is timed the same way beside it.  ``--cpu``: the same chain in float32
scipy / numpy on this process's CPUs (one clip per worker thread), the yardstick for "what the host would pay".

    python scripts/wave_augment_bench.py [--iters 50] [--warmup 5] [--cpu] [--out profiles/wave_augment.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pools(rng, sr=16000):
    irs = [(rng.standard_normal(n) * np.exp(-np.arange(n) / (n / 6.0))).astype(np.float32) for n in (sr, 2 * sr)]
    noises = [rng.standard_normal(n).astype(np.float32) * 0.1 for n in (5 * sr, 30 * sr)]
    return irs, noises


def cpu_chain(clips, irs, noises, plan, threads):
    import scipy.signal
    from concurrent.futures import ThreadPoolExecutor

    def one(b):
        x = clips[b]
        n = len(x)
        if plan.ir_idx[b] >= 0:
            y = scipy.signal.fftconvolve(x, irs[plan.ir_idx[b]])
            x = (y * np.float32(0.5 / max(float(np.abs(y).max()), 1e-30)))[:n]
        if plan.noise_idx[b] >= 0:
            v = noises[plan.noise_idx[b]]
            w = v[(plan.noise_start[b] + np.arange(n)) % len(v)]
            x = x + np.float32(np.sqrt(np.mean(x * x)) / 10 ** (plan.noise_snr_db[b] / 20) / np.sqrt(np.mean(w * w))) * w
        if np.isfinite(plan.gauss_snr_db[b]):
            x = x + np.float32(np.sqrt(np.mean(x * x)) / 10 ** (plan.gauss_snr_db[b] / 20)) * np.random.default_rng(b).standard_normal(n).astype(np.float32)
        if plan.clip_pct[b] > 0:
            lo, hi = np.percentile(x, [plan.clip_pct[b] // 2, 100 - plan.clip_pct[b] // 2])
            x = np.clip(x, lo, hi)
        return x
    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(one, range(len(clips))))
        return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16")))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from tiny_audio_amd.asr_processing import LogMelFeatureExtractor
    from tiny_audio_amd.augmentation import DeviceProductionAugment
    if not torch.cuda.is_available():
        raise SystemExit("wave_augment_bench.py measures on the GPU; none found")
    rng = np.random.default_rng(0)
    B, n = a.batch, int(a.seconds * 16000)
    irs, noises = pools(rng)
    clips = [rng.standard_normal(n).astype(np.float32) * 0.1 for _ in range(B)]
    wav = torch.from_numpy(np.stack(clips)).cuda()
    lens = torch.full((B,), n, dtype=torch.int64, device="cuda")
    events = [(rng.standard_normal(m) * np.exp(-np.arange(m) / (m / 4.0))).astype(np.float32) for m in (8000, 24000, 64000)]
    every = dict(rir_pool=irs, noise_pool=noises, short_noises_pool=events, gaussian_min_snr_db=20.0, gaussian_max_snr_db=40.0, device="cuda", seed=0)
    aug = DeviceProductionAugment(rir_prob=1.0, prob=1.0, clipping_prob=1.0, short_noises_prob=1.0, eq_prob=1.0, bandlimit_prob=1.0, **every)
    full = aug.plan([n] * B)
    full.ir_idx[:] = np.arange(B) % 2                    # half the clips the 1 s response, half the 2 s one

    def only(**keep):
        p = aug.plan([n] * B)
        p.ir_idx[:] = full.ir_idx if keep.get("rir") else -1
        p.ir_idx[:] = keep["rir_idx"] if "rir_idx" in keep else p.ir_idx
        p.noise_idx[:] = full.noise_idx if keep.get("bg") else -1
        p.gauss_snr_db[:] = full.gauss_snr_db if keep.get("gauss") else np.nan
        p.clip_pct[:] = full.clip_pct if keep.get("clip") else 0
        p.ev_count[:] = full.ev_count if keep.get("events") else 0
        p.eq_nsec[:] = full.eq_nsec if keep.get("eq") else 0
        p.bl_nsec[:] = full.bl_nsec if keep.get("bl") else 0
        for f in ("ev_pool", "ev_off", "ev_len", "ev_t0", "ev_fade_in", "ev_fade_out", "ev_snr_db", "eq_sos", "bl_sos"):
            getattr(p, f)[:] = getattr(full, f)
        return p

    fe = LogMelFeatureExtractor(128, "cuda")
    four = dict(rir=True, bg=True, gauss=True, clip=True)
    recipe = DeviceProductionAugment(rir_prob=0.5, prob=0.6, clipping_prob=0.1, short_noises_prob=0.5, eq_prob=0.5, bandlimit_prob=0.3, **every)
    drawn = recipe.plan([n] * B)
    cases = {"all stages": only(**four), "rir only (1 s + 2 s)": only(rir=True), "rir only, 1 s": only(rir_idx=0), "rir only, 2 s": only(rir_idx=1),
             "background only": only(bg=True), "gaussian only": only(gauss=True), "clipping only (every clip)": only(clip=True),
             "all off (copy)": only(), "short noises only (every clip)": only(events=True), "eq only (every clip)": only(eq=True),
             "band-limit only (every clip)": only(bl=True), "all seven stages, every clip": full,
             "production chain at the recipe's probabilities": drawn}

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    res = {"batch": B, "seconds": a.seconds, "iters": a.iters, "us": {}}
    for name, plan in cases.items():
        desc = torch.from_numpy(plan.pack()).cuda()
        st, E, ml = plan.stages(), plan.ev_stride(), plan.max_event_len()
        res["us"][name] = timed(lambda: aug._apply_chain(wav, lens, desc, st, plan.seed, plan.offset, E, ml))
    res["drawn"] = {"events": int(drawn.ev_count.sum()), "clips with events": int((drawn.ev_count > 0).sum()), "eq": int((drawn.eq_nsec > 0).sum()),
                    "band-limit": int((drawn.bl_nsec > 0).sum()), "rir": int((drawn.ir_idx >= 0).sum()),
                    "background": int((drawn.noise_idx >= 0).sum()), "clipped": int((drawn.clip_pct > 0).sum())}
    res["events in 'every clip'"] = int(full.ev_count.sum())
    res["us"]["logmel"] = timed(lambda: fe._extract(wav, lens))
    # the cascade kernel by itself: seven EQ sections on every clip, after a copy of the batch (timed alone beside it)
    buf = torch.empty_like(wav)
    nsec, sos = torch.from_numpy(full.eq_nsec).cuda(), torch.from_numpy(full.eq_sos).cuda()
    res["us"]["copy_ (torch)"] = timed(lambda: buf.copy_(wav))
    res["us"]["copy_ + sos, 7 sections, time-parallel (chunk 256)"] = timed(lambda: (buf.copy_(wav), aug._sos(buf, lens, nsec, sos)))
    seq = (n + 31) // 32 * 32
    a.iters, keep = max(a.iters // 10, 3), a.iters
    res["us"]["copy_ + sos, 7 sections, one thread per clip (chunk = the clip)"] = timed(lambda: (buf.copy_(wav), aug._sos(buf, lens, nsec, sos, seq)))
    a.iters = keep
    if a.cpu:
        cpu_chain(clips[:a.threads], irs, noises, full, a.threads)
        res["us"][f"cpu float32 scipy chain, {a.threads} threads"] = min(cpu_chain(clips, irs, noises, full, a.threads) for _ in range(3))
    for k, v in res["us"].items():
        print(f"{k:45s} {v:12.1f} us")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
