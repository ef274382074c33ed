#!/usr/bin/env python3
"""Measurement: what acting costs in a closed-loop rollout at 65 536 envs of GoalContinuous3P-v0 with an actor and a critic of two
hidden layers of 64 (tanh) -- policy_act_torch / rollout_policy_torch against the same computation in eager torch.
  * act_kernel:    policy_act_torch (one launch: both nets, the draw, the log-prob)
  * act_eager:     two nn.Sequential forwards, Normal.sample and log_prob(...).sum(-1), the way a learner writes it
  * step:          step_torch alone (the baseline the acting surrounds)
  * rollout:       rollout_policy_torch(K = 128), per step
  * eager_loop:    K iterations of the eager forward + sample + log_prob + step_torch, per step
Stream events around back-to-back calls after a warm-up; median, 10th and 90th percentile over the repetitions, microseconds, the
host side of every call included (that is the point: the eager path is about ten launches per step).  One JSON line.
    python tools/gpu_policy_cost.py [out.jsonl]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_policy_cost.py --kernel-trace"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402

ENV_ID, B, K, HIDDEN = "GoalContinuous3P-v0", 65536, 128, 64


def timed(fn, reps, inner, per=1):
    """microseconds per `per`-th of a call: (median, p10, p90) over reps repetitions of `inner` back-to-back calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / (inner * per))
    return [round(float(x), 2) for x in (np.median(out), np.percentile(out, 10), np.percentile(out, 90))]


def main():
    trace = "--kernel-trace" in sys.argv
    paths = [a for a in sys.argv[1:] if not a.startswith("--")]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    env = sg.make_vec(ENV_ID, B, device=0, seed=1)
    D = env.obs_dim

    def net(out):
        return torch.nn.Sequential(torch.nn.Linear(D, HIDDEN), torch.nn.Tanh(), torch.nn.Linear(HIDDEN, HIDDEN), torch.nn.Tanh(),
                                   torch.nn.Linear(HIDDEN, out)).to(dev)
    actor, critic = net(2), net(1)
    log_std = torch.nn.Parameter(torch.full((2,), -0.5, device=dev))
    linears = lambda m: [(l.weight, l.bias) for l in m if isinstance(l, torch.nn.Linear)]  # noqa: E731
    pol = env.policy_torch(actor=linears(actor), critic=linears(critic), log_std=log_std)
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)  # noqa: E731
    buf = dict(obs=z(K + 1, B, D), action=z(K, B, 2), logp=z(K, B), value=z(K + 1, B), reward=z(K, B), done=z(K, B, dtype=torch.uint8),
               trunc=z(K, B, dtype=torch.uint8))
    buf["obs"][0].copy_(env.reset_torch())
    obs = buf["obs"][0]
    out = dict(action=buf["action"][0], logp=buf["logp"][0], value=buf["value"][0])

    def eager(o):
        with torch.no_grad():
            dist = torch.distributions.Normal(actor(o), log_std.exp())
            a = dist.sample()
            return a, dist.log_prob(a).sum(-1), critic(o)[:, 0]

    def eager_loop():
        for t in range(K):
            a, lp, v = eager(buf["obs"][t])
            buf["logp"][t], buf["value"][t] = lp, v
            env.step_torch(a, out=dict(obs=buf["obs"][t + 1], reward=buf["reward"][t], done=buf["done"][t], trunc=buf["trunc"][t]))

    # the two paths compute the same thing: mean, value and the log-prob of the kernel's own action
    a, lp, v = env.policy_act_torch(pol, obs, seed=3, step=0)
    with torch.no_grad():
        dist = torch.distributions.Normal(actor(obs), log_std.exp())
        agree = dict(value=float((critic(obs)[:, 0] - v).abs().max()), logp=float((dist.log_prob(a).sum(-1) - lp).abs().max()),
                     mean=float((env.policy_act_torch(pol, obs, deterministic=True)[0] - actor(obs)).abs().max()))
    reps, inner = (2, 5) if trace else (15, 50)
    rec = dict(env_id=ENV_ID, num_envs=B, hidden=HIDDEN, n_hidden=2, K=K, max_abs_diff_vs_eager=agree,
               act_kernel_us=timed(lambda: env.policy_act_torch(pol, obs, seed=3, step=0, out=out), reps, inner),
               act_eager_us=timed(lambda: eager(obs), reps, inner),
               step_us=timed(lambda: env.step_torch(buf["action"][0]), reps, inner),
               rollout_us_per_step=timed(lambda: env.rollout_policy_torch(pol, seed=3, **buf), max(2, reps // 3), 2, per=K),
               eager_loop_us_per_step=timed(eager_loop, max(2, reps // 3), 2, per=K))
    env.check_status()
    line = json.dumps(rec)
    print(line, flush=True)
    for p in paths:
        with open(p, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
