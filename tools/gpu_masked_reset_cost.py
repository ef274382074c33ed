#!/usr/bin/env python3
"""Measurement: what a masked reset (reset_torch(mask=...), sg_reset_masked_device) costs.  GoalContinuous3P-v0 and
KeplerRandomOrbits-v0 at 65 536 and 1 048 576 envs; four masks -- empty, the done row of a real step (auto-reset on, after 300
steps: ~2 % of the envs), 10 % random, all ones -- against the full reset_torch() and a one-launch-per-step step_torch; and the
per-step time of the loop "auto_reset off, step_torch + reset_torch(mask=done)" against "auto_reset on, step_torch".  Stream
events around back-to-back calls (median over the repetitions, per call).  One JSON line per (id, batch).  At 65 536 envs the
calls are bound by the host side of a call (~7 us with an empty mask); --kernel-trace only issues, per id at 65 536 envs, 200
masked resets with the done row and 200 full resets, to be run under `rocprofv3 --kernel-trace --stats` for the kernels' own
durations.
    python tools/gpu_masked_reset_cost.py [out.jsonl]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_masked_reset_cost.py --kernel-trace"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402


def timed(fn, reps, per):
    """median over `reps` timings of `per` back-to-back calls of fn(k), in microseconds per call"""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(per):
            fn(k)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / per)
    return float(np.median(out))


def measure(env_id, B):
    dev = torch.device("cuda", 0)
    on = sg.make_vec(env_id, B, device=0, seed=0, auto_reset=True)
    off = sg.make_vec(env_id, B, device=0, seed=0, auto_reset=False)
    T = 64
    acts = torch.rand((T, B, 2), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2 - 1
    on.reset_torch(); off.reset_torch()
    for t in range(300):
        on.step_torch(acts[t % T])
    _, _, done, _ = on.step_torch(acts[0])
    masks = {"empty": torch.zeros(B, dtype=torch.uint8, device=dev), "done_row": done.clone(),
             "random_10pct": (torch.rand(B, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) < 0.1).view(torch.uint8),
             "all_ones": torch.ones(B, dtype=torch.uint8, device=dev)}
    torch.cuda.synchronize()
    reps, per = (15, 50) if B <= 65536 else (9, 20)
    res = dict(env=env_id, batch=B, device=torch.cuda.get_device_name(0),
               mask_bits={k: int(m.sum().item()) for k, m in masks.items()})
    obs = off.reset_torch()
    for _ in range(3):  # warm
        off.reset_torch(); off.reset_torch(mask=masks["done_row"]); on.step_torch(acts[0])
    res["masked_reset_us"] = {k: timed(lambda _k, m=m: off.reset_torch(out=obs, mask=m), reps, per) for k, m in masks.items()}
    res["full_reset_us"] = timed(lambda _k: off.reset_torch(out=obs), reps, per)
    res["step_torch_us"] = timed(lambda k: on.step_torch(acts[k % T]), reps, per)
    # the training loops, from the same state
    on.reset_torch(); off.reset_torch()
    for t in range(300):
        on.step_torch(acts[t % T])
        _, _, d, _ = off.step_torch(acts[t % T])
        off.reset_torch(mask=d)
    torch.cuda.synchronize()

    def off_loop(k):
        _, _, d, _ = off.step_torch(acts[k % T])
        off.reset_torch(mask=d)
    res["loop_auto_reset_on_us"] = timed(lambda k: on.step_torch(acts[k % T]), reps, per)
    res["loop_auto_reset_off_masked_us"] = timed(off_loop, reps, per)
    res["done_row_below_full_reset"] = res["masked_reset_us"]["done_row"] < res["full_reset_us"]
    on.check_status(); off.check_status()
    on.close(); off.close()
    return res


def kernel_trace_phase():
    dev = torch.device("cuda", 0)
    for env_id in ("GoalContinuous3P-v0", "KeplerRandomOrbits-v0"):
        B = 65536
        on = sg.make_vec(env_id, B, device=0, seed=0, auto_reset=True)
        off = sg.make_vec(env_id, B, device=0, seed=0, auto_reset=False)
        acts = torch.rand((B, 2), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2 - 1
        on.reset_torch(); off.reset_torch()
        for _ in range(300):
            on.step_torch(acts)
        done = on.step_torch(acts)[2].clone()
        obs = off.reset_torch()
        for _ in range(200):
            off.reset_torch(out=obs, mask=done)
        for _ in range(200):
            off.reset_torch(out=obs)
        torch.cuda.synchronize()
        print(env_id, "done-row bits", int(done.sum().item()), flush=True)
        on.close(); off.close()


def main():
    if "--kernel-trace" in sys.argv:
        return kernel_trace_phase()
    lines = []
    for env_id in ("GoalContinuous3P-v0", "KeplerRandomOrbits-v0"):
        for B in (65536, 1048576):
            line = json.dumps(measure(env_id, B))
            print(line, flush=True)
            lines.append(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
