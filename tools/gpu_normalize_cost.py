#!/usr/bin/env python3
"""Measurement: what running normalization (sg_set_normalize: norm_moments_kernel, norm_merge_kernel, norm_apply_kernel)
adds to a stepping call, and what the same rules cost as eager torch ops -- what a user has without it.  GoalContinuous3P-v0,
65 536 envs, two handles with the same seed, normalization off / on (observations and rewards), timed alternately with
stream events around each call (median over the repetitions): the 20-step rollout launch, a 1000-step rollout, one launch per
step (step_torch).  The baseline normalizes the off handle's K-step output step by step with torch float64 ops (the running
statistics after each step's update, as the rules require).  Run under `rocprofv3 --kernel-trace --stats` for the kernels'
own durations.
    python tools/gpu_normalize_cost.py [out.json]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402


class TorchNormalize:
    """gym NormalizeObservation + NormalizeReward as eager torch ops on device tensors: one update per step row"""

    def __init__(self, B, D, dev, gamma=0.99, eps=1e-8):
        f = dict(dtype=torch.float64, device=dev)
        self.om, self.ov, self.oc = torch.zeros(D, **f), torch.ones(D, **f), 1e-4
        self.rm, self.rv, self.rc = torch.zeros((), **f), torch.ones((), **f), 1e-4
        self.ret = torch.zeros(B, **f)
        self.gamma, self.eps = gamma, eps

    @staticmethod
    def _update(mean, var, count, x):
        bm, bv, n = x.mean(0), x.var(0, unbiased=False), x.shape[0]
        delta = bm - mean
        tot = count + n
        mean = mean + delta * n / tot
        var = (var * count + bv * n + delta * delta * count * n / tot) / tot
        return mean, var, tot

    def step(self, obs, rew, done):
        x = obs.double()
        self.om, self.ov, self.oc = self._update(self.om, self.ov, self.oc, x)
        obs.copy_((x - self.om) / torch.sqrt(self.ov + self.eps))
        self.ret = self.ret * self.gamma + rew.double()
        self.rm, self.rv, self.rc = self._update(self.rm, self.rv, self.rc, self.ret)
        rew.copy_(rew.double() / torch.sqrt(self.rv + self.eps))
        self.ret.masked_fill_(done.bool(), 0.0)


def main():
    B, env_id = 65536, "GoalContinuous3P-v0"
    dev = torch.device("cuda", 0)
    envs = {m: sg.make_vec(env_id, B, device=0, seed=0, normalize_obs=(m == "on"), normalize_reward=(m == "on"))
            for m in ("off", "on")}
    D = envs["on"].obs_dim
    Kmax = 1000
    acts = torch.rand((Kmax, B, 2), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2 - 1
    obs = torch.empty((Kmax, B, D), device=dev); rew = torch.empty((Kmax, B), device=dev)
    done = torch.empty((Kmax, B), dtype=torch.uint8, device=dev); trunc = torch.empty_like(done)
    for e in envs.values():
        e.reset_torch()
        for _ in range(3):
            e.rollout_torch(acts[:200], obs[:200], rew[:200], done[:200], trunc[:200])
        e.rollout_torch(acts[:Kmax], obs[:Kmax], rew[:Kmax], done[:Kmax], trunc[:Kmax])  # (scratch for 1000 steps)
    torch.cuda.synchronize()
    tn = TorchNormalize(B, D, dev)

    def rollout(m, K):
        envs["off" if m == "torch" else m].rollout_torch(acts[:K], obs[:K], rew[:K], done[:K], trunc[:K])
        if m == "torch":
            for t in range(K):
                tn.step(obs[t], rew[t], done[t])

    def steps(m, n):
        for t in range(n):
            envs[m].step_torch(acts[t])

    def timed(fn, reps, per=1, modes=("off", "on")):
        out = {m: [] for m in modes}
        for r in range(reps):
            for m in (modes if r % 2 == 0 else modes[::-1]):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); fn(m); b.record()
                torch.cuda.synchronize()
                out[m].append(a.elapsed_time(b) * 1000.0 / per)
        res = {m: float(np.median(v)) for m, v in out.items()}
        for m in modes[1:]:
            res[f"added_us_{m}"] = res[m] - res["off"]
            res[f"added_pct_{m}"] = 100.0 * (res[m] - res["off"]) / res["off"]
        return res

    bytes_per_env_step = 193  # moments: obs 60 + reward 4 + done 1; apply: obs 60 + 60, reward 4 + 4
    result = dict(env=env_id, batch=B, device=torch.cuda.get_device_name(0), bytes_per_env_step=bytes_per_env_step)
    for _ in range(2):  # warm
        rollout("on", 20); rollout("off", 20); rollout("torch", 20); steps("on", 20); steps("off", 20)
    result["rollout_k20_us"] = timed(lambda m: rollout(m, 20), 100, modes=("off", "on", "torch"))
    result["rollout_k1000_us"] = timed(lambda m: rollout(m, 1000), 8)
    result["rollout_k1000_torch_us"] = timed(lambda m: rollout(m, 1000), 2, modes=("off", "torch"))
    result["step_per_launch_us"] = timed(lambda m: steps(m, 200), 10, per=200)
    for K, key in ((20, "rollout_k20_us"), (1000, "rollout_k1000_us")):
        bound_us = bytes_per_env_step * B * K / 8e12 * 1e6
        result[key]["hbm_bound_us"] = bound_us
        result[key]["share_of_hbm_bound"] = bound_us / max(result[key]["added_us_on"], 1e-9)
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
