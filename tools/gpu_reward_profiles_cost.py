#!/usr/bin/env python3
"""Measurement: what reward profiles cost.  GoalContinuous3P-v0 and KeplerCircleOrbit-v0, a handle with 8 profiles and random
per-env indices against one without: one step_torch launch per step at 65 536 and 1 048 576 envs (each step plan: the wave-pair
and the one-wave step kernels, SPACEGYM_STEP_KERNEL), and rollout_torch of 20 and 1000 steps at 65 536 envs (the wave-pair K-step
kernels, *_pair_rollout_profiled_kernel against *_pair_rollout_kernel).  Then large tables: GoalContinuous4P-v0 (the one-wave
step kernel with the most static LDS) at 1 048 576 envs with 8, 48, 64 and 256 profiles, one-wave plan.  Stream events around
back-to-back calls, the two handles alternated, median over the repetitions.  One JSON line per (id, batch).
    python tools/gpu_reward_profiles_cost.py [out.jsonl]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402

PROFILES = {"goal": [dict(survival_reward_scale=0.05 * k, goal_vel_reward_scale=0.5 + 0.1 * k, danger_zone=0.1 + 0.02 * k)
                     for k in range(8)],
            "kepler": [dict(numerator_C=0.01 + 0.005 * k, rad_penalty_C=1.0 + 0.25 * k) for k in range(8)]}


def timed_pair(fa, fb, reps, per):
    """medians (us per call) of `per` back-to-back calls of fa and of fb, alternated `reps` times"""
    out = ([], [])
    for _ in range(reps):
        for j, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(per):
                fn(k)
            b.record()
            torch.cuda.synchronize()
            out[j].append(a.elapsed_time(b) * 1000.0 / per)
    return float(np.median(out[0])), float(np.median(out[1]))


def pair(env_id, B, plan, n_prof=8):
    """a handle without profiles and one with n_prof and random indices, same seed; plan: SPACEGYM_STEP_KERNEL ("": chosen by size)"""
    os.environ["SPACEGYM_STEP_KERNEL"] = plan
    fam = "goal" if env_id.startswith("Goal") else "kepler"
    plain = sg.make_vec(env_id, B, device=0, seed=0)
    profs = [PROFILES[fam][k % 8] for k in range(n_prof)]
    prof = sg.make_vec(env_id, B, device=0, seed=0, reward_profiles=profs)
    prof.set_env_profiles(np.random.default_rng(0).integers(0, n_prof, B))
    os.environ.pop("SPACEGYM_STEP_KERNEL")
    plain.reset_torch(); prof.reset_torch()
    return plain, prof


def measure(env_id, B):
    dev = torch.device("cuda", 0)
    T = 64
    acts = torch.rand((T, B, 2), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2 - 1
    res = dict(env=env_id, batch=B, device=torch.cuda.get_device_name(0), profiles=8)
    reps, per = (15, 50) if B <= 65536 else (9, 20)
    for plan in ("pair", "single"):
        plain, prof = pair(env_id, B, plan)
        for t in range(100):  # warm, and into steady state (episodes ending)
            plain.step_torch(acts[t % T]); prof.step_torch(acts[t % T])
        torch.cuda.synchronize()
        a, b = timed_pair(lambda k: plain.step_torch(acts[k % T]), lambda k: prof.step_torch(acts[k % T]), reps, per)
        res[f"step_{plan}_us"] = dict(plain=a, profiled=b, ratio=b / a)
        plain.check_status(); prof.check_status()
        plain.close(); prof.close()
    if B == 65536:
        plain, prof = pair(env_id, B, "")  # (the default plans)
        for K, (r, p) in ((20, (9, 10)), (1000, (5, 1))):
            a_k = torch.rand((K, B, 2), device=dev, generator=torch.Generator(device=dev).manual_seed(K)) * 2 - 1
            outs = [(torch.empty((K, B, plain.obs_dim), device=dev), torch.empty((K, B), device=dev),
                     torch.empty((K, B), dtype=torch.uint8, device=dev), torch.empty((K, B), dtype=torch.uint8, device=dev))
                    for _ in range(2)]
            plain.rollout_torch(a_k, *outs[0]); prof.rollout_torch(a_k, *outs[1])  # warm
            torch.cuda.synchronize()
            a, b = timed_pair(lambda k: plain.rollout_torch(a_k, *outs[0]), lambda k: prof.rollout_torch(a_k, *outs[1]), r, p)
            res[f"rollout_{K}_us_per_step"] = dict(plain=a / K, profiled=b / K, ratio=b / a,
                                                   plain_kernel=plain.rollout_kernel(K), profiled_kernel=prof.rollout_kernel(K))
        plain.check_status(); prof.check_status()
        plain.close(); prof.close()
    return res


def large_tables(env_id="GoalContinuous4P-v0", B=1048576):
    """the one-wave step kernel with n profiles in LDS: past what two workgroups per CU hold, one per CU"""
    T = 16
    dev = torch.device("cuda", 0)
    acts = torch.rand((T, B, 2), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2 - 1
    res = dict(env=env_id, batch=B, device=torch.cuda.get_device_name(0), plan="single", step_us={})
    for n in (8, 48, 64, 256):
        plain, prof = pair(env_id, B, "single", n)
        for t in range(50):
            plain.step_torch(acts[t % T]); prof.step_torch(acts[t % T])
        torch.cuda.synchronize()
        a, b = timed_pair(lambda k: plain.step_torch(acts[k % T]), lambda k: prof.step_torch(acts[k % T]), 9, 20)
        res["step_us"][str(n)] = dict(plain=a, profiled=b, ratio=b / a)
        plain.check_status(); prof.check_status()
        plain.close(); prof.close()
    return res


def main():
    lines = []
    for env_id in ("GoalContinuous3P-v0", "KeplerCircleOrbit-v0"):
        for B in (65536, 1048576):
            line = json.dumps(measure(env_id, B))
            print(line, flush=True)
            lines.append(line)
    line = json.dumps(large_tables())
    print(line, flush=True)
    lines.append(line)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
