"""Long-form transcription on a synthetic hour: what the planning kernels cost, how many windows they make, and what the whole of
``ASRModel.transcribe_long`` takes with and without the length sort.

    python scripts/longform_bench.py [--minutes 60] [--batch-size 32] [--max-new-tokens 48] [--rounds 5] [--small]
                                     [--plan-sizes 360000,1048576]

Workload: ``--minutes`` of speech-like bursts (noise under a 4 Hz syllable envelope, 1 - 7 s each) separated by pauses of 0.2 - 1.5 s,
from a seed; the model is the default ``ASRConfig`` with random weights (``--small``: the tests' small model, for a rehearsal) and a
stub tokenizer -- the weights matter to the timing only through the step at which the random LM happens to emit an end token
(at most ``--max-new-tokens`` steps per group).  Printed, one JSON object per line:
  * planning: ``ta_wave_cut_cost_f32`` (its three launches; bytes/s = 4 n over the time), ``ta_cut_plan_f32`` and one
    ``ta_wave_windows_f32`` gather of ``--batch-size`` windows, HIP events around ``--inner`` calls, median of ``--repeats``;
  * the plan kernel alone at every T of ``--plan-sizes`` (min_len 1000, max_len 2800, random costs) next to tests/segment_ref.py's
    numpy restatement on the host, one run of each;
  * the number of windows, their length statistics, the share of cuts above twice the recording's quietest cut cost;
  * transcribe_long: total wall time (host clock around a device synchronise; median, min, max of ``--rounds``) and audio seconds
    per second with longest-first groups and with the same windows grouped in time order, the two alternating.
Results: profiles/longform.md.
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

from tiny_audio_amd import longform, ops  # noqa: E402


def synth(minutes, seed=0):
    rng = np.random.RandomState(seed)
    n = int(minutes * 60 * 16000)
    x = np.zeros(n, np.float32)
    at = 0
    while at < n:
        burst = int(rng.uniform(1.0, 7.0) * 16000)
        end = min(at + burst, n)
        t = np.arange(end - at) / 16000.0
        env = 0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t + rng.uniform(0, 6.28))
        x[at:end] = (0.1 * rng.uniform(0.3, 1.0)) * env * rng.standard_normal(end - at)
        at = end + int(rng.uniform(0.2, 1.5) * 16000)
    return x


def time_events(fn, warmup, repeats, inner):
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
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


class StubTokenizer:
    def __init__(self, audio_id):
        self.audio_id = audio_id

    def convert_tokens_to_ids(self, t):
        return self.audio_id

    def apply_chat_template(self, messages, tokenize=True, add_generation_prompt=False, **_):
        user = [m for m in messages if m["role"] == "user"][0]["content"]
        return torch.tensor([[5, 6, 7] + [self.audio_id] * user.count("<audio>") + [40, 41, 42, 43]])

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(f"w{i}" for i in ids)


def build_model(small):
    from tiny_audio_amd.asr_config import ASRConfig
    from tiny_audio_amd.asr_modeling import ASRModel
    if small:
        from oracle import weights as OW
        cfg = ASRConfig(audio_config=OW.enc_config(hidden=256, ffn=512, layers=2, heads=4),
                        text_config=OW.lm_config(vocab=1024, hidden=256, ffn=512, layers=2, heads=4, kv_heads=2, head_dim=128),
                        projector_hidden_dim=128, audio_token_id=1023, pad_token_id=1000, eos_token_id=1001)
    else:
        cfg = ASRConfig()
    m = ASRModel(cfg, device="cuda", init="random", seed=0)
    m.tokenizer = StubTokenizer(int(m.audio_token_id))
    return m


def plan_alone(T, repeats):
    from tests import segment_ref as R
    rng = np.random.RandomState(T % 9973)
    host = (rng.rand(T + 1) ** 4).astype(np.float32)
    cost = torch.from_numpy(host[None]).cuda()
    off = torch.tensor([0, 160 * T], device="cuda")
    dev = time_events(lambda: ops.cut_plan(cost, off, 160 * T, 1000, 2800), 1, repeats, 1)
    cuts, n_seg, dp_T, _ = ops.cut_plan(cost, off, 160 * T, 1000, 2800)
    t0 = time.perf_counter()
    rc, rn, rdp, _, _ = R.cut_plan(host, T, 1000, 2800)
    host_s = time.perf_counter() - t0
    same = int(n_seg[0]) == rn and cuts[0, :rn + 1].cpu().tolist() == rc and float(dp_T[0]) == float(rdp)
    return dict(T=T, hours=T / 360000.0, plan_kernel_ms=dev, segment_ref_host_s=host_s, same_plan=bool(same), windows=rn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--max-new-tokens", type=int, default=48)
    ap.add_argument("--max-window-s", type=float, default=28.0)
    ap.add_argument("--min-window-s", type=float, default=10.0)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--plan-sizes", default="360000,1048576")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-decode", action="store_true")
    a = ap.parse_args()
    x = synth(a.minutes)
    n = len(x)
    min_len, max_len = longform.window_positions(a.max_window_s, a.min_window_s)
    flat, off, lens = longform.upload([x])
    t = lambda fn: time_events(fn, a.warmup, a.repeats, a.inner)  # noqa: E731
    res = dict(device=torch.cuda.get_device_name(0), minutes=a.minutes, samples=n, positions=-(-n // 160) + 1)
    res["cut_cost_ms"] = t(lambda: ops.wave_cut_cost(flat, off, n))
    res["cut_cost_tb_per_s"] = 4.0 * n / (res["cut_cost_ms"]["median"] * 1e-3) / 1e12
    cost = ops.wave_cut_cost(flat, off, n)
    res["cut_plan_ms"] = t(lambda: ops.cut_plan(cost, off, n, min_len, max_len))
    plan = longform.plan_uploaded(flat, off, lens, min_len, max_len)[0]
    W = len(plan.starts)
    order = longform.group_windows(plan.lengths, a.batch_size)[0]
    st = torch.tensor([plan.starts[k] for k in order], dtype=torch.int64, device="cuda")
    ln = torch.tensor([plan.lengths[k] for k in order], dtype=torch.int32, device="cuda")
    Ls = max(plan.lengths[k] for k in order)
    res["gather_ms"] = t(lambda: ops.wave_windows(flat, st, ln, Ls))
    res["gather_windows"], res["gather_tb_per_s"] = len(order), 2 * 4.0 * len(order) * Ls / (res["gather_ms"]["median"] * 1e-3) / 1e12
    quiet = min(plan.cut_costs) if plan.cut_costs else 0.0
    res["windows"] = W
    res["window_s"] = dict(min=min(plan.lengths) / 16000, median=statistics.median(plan.lengths) / 16000, max=max(plan.lengths) / 16000)
    res["cuts_above_twice_the_quietest"] = sum(c > 2 * quiet for c in plan.cut_costs)
    print(json.dumps(res), flush=True)
    for T in [int(v) for v in a.plan_sizes.split(",") if v]:
        print(json.dumps(plan_alone(T, 3)), flush=True)
    if a.no_decode:
        return
    m = build_model(a.small)
    kw = dict(max_window_s=a.max_window_s, min_window_s=a.min_window_s, batch_size=a.batch_size, max_new_tokens=a.max_new_tokens)
    m.transcribe_long(x[:16000 * 120], **kw)                                  # warm-up: code objects, the decode graph
    torch.cuda.synchronize()
    sorted_groups = longform.group_windows
    runs = {"longest_first": sorted_groups,
            "time_order": lambda lengths, bs: [list(range(i, min(i + bs, len(lengths)))) for i in range(0, len(lengths), bs)]}
    out, walls = {}, {name: [] for name in runs}
    try:
        for _ in range(a.rounds):                                               # the two orders alternate: other work shares the host
            for name, fn in runs.items():
                longform.group_windows = fn
                t0 = time.perf_counter()
                r = m.transcribe_long(x, **kw)
                torch.cuda.synchronize()
                walls[name].append(time.perf_counter() - t0)
                out[name] = dict(chunks=len(r["chunks"]), words_of_text=len(r["text"].split()))
    finally:
        longform.group_windows = sorted_groups
    for name, w in walls.items():
        out[name].update(wall_s=dict(median=statistics.median(w), min=min(w), max=max(w)), audio_s_per_s=n / 16000 / statistics.median(w))
    out["time_order_over_longest_first"] = out["time_order"]["wall_s"]["median"] / out["longest_first"]["wall_s"]["median"]
    print(json.dumps(dict(transcribe_long=out, batch_size=a.batch_size, max_new_tokens=a.max_new_tokens, small_model=a.small)), flush=True)


if __name__ == "__main__":
    main()
