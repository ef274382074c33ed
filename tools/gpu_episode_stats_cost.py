#!/usr/bin/env python3
"""Measurement: what the episode-statistics pass (episode_stats_kernel) adds to a stepping call.  GoalContinuous3P-v0,
65 536 envs, two handles with the same seed, statistics off / on, timed alternately with stream events around each call
(median over the repetitions): the 20-step rollout launch, a 1000-step rollout, one launch per step (step_torch).  Run under
`rocprofv3 --kernel-trace --stats` for the kernel's own duration.
    python tools/gpu_episode_stats_cost.py [out.json]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402


def main():
    B, env_id = 65536, "GoalContinuous3P-v0"
    dev = torch.device("cuda", 0)
    envs = {m: sg.make_vec(env_id, B, device=0, seed=0, episode_statistics=(m == "on")) for m in ("off", "on")}
    Kmax = 1000
    acts = torch.rand((Kmax, B, 2), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2 - 1
    obs = torch.empty((Kmax, B, envs["on"].obs_dim), device=dev); rew = torch.empty((Kmax, B), device=dev)
    done = torch.empty((Kmax, B), dtype=torch.uint8, device=dev); trunc = torch.empty_like(done)
    el = envs["on"].episode_list_torch(B * 64)
    rows = dict(r=torch.empty(B, dtype=torch.float64, device=dev), l=torch.empty(B, dtype=torch.int32, device=dev))
    for e in envs.values():
        e.reset_torch()
        for _ in range(3):
            e.rollout_torch(acts[:200], obs[:200], rew[:200], done[:200], trunc[:200])
    torch.cuda.synchronize()

    def rollout(m, K):
        if m == "on":
            envs[m].rollout_torch(acts[:K], obs[:K], rew[:K], done[:K], trunc[:K], episodes=el)
        else:
            envs[m].rollout_torch(acts[:K], obs[:K], rew[:K], done[:K], trunc[:K])

    def steps(m, n):
        for t in range(n):
            if m == "on":
                envs[m].step_torch(acts[t], episodes=rows)
            else:
                envs[m].step_torch(acts[t])

    def timed(fn, reps, per=1):
        out = {"off": [], "on": []}
        for r in range(reps):
            for m in (("off", "on") if r % 2 == 0 else ("on", "off")):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); fn(m); b.record()
                torch.cuda.synchronize()
                out[m].append(a.elapsed_time(b) * 1000.0 / per)
        res = {m: float(np.median(v)) for m, v in out.items()}
        res["added_us"] = res["on"] - res["off"]
        res["added_pct"] = 100.0 * res["added_us"] / res["off"]
        return res

    result = dict(env=env_id, batch=B, device=torch.cuda.get_device_name(0))
    for _ in range(2):  # warm
        rollout("on", 20); rollout("off", 20); steps("on", 20); steps("off", 20)
    result["rollout_k20_us"] = timed(lambda m: rollout(m, 20), 200)
    result["rollout_k1000_us"] = timed(lambda m: rollout(m, 1000), 12)
    result["step_per_launch_us"] = timed(lambda m: steps(m, 200), 10, per=200)
    for e in envs.values():
        e.check_status()
        e.close()
    line = json.dumps(result)
    print(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
