#!/usr/bin/env python3
"""Measurement: what the SAC actor costs at GoalContinuous3P-v0 with two hidden layers of 64 (relu), n = 4 096 and n = 65 536 envs /
rows -- the engine's kernels against the same computation in eager torch (nn.Sequential, torch.clamp, torch.tanh, autograd).
  * act:     squashed_act_torch (one launch: forward, Philox noise, tanh, logp)      / eager: forward, randn, tanh, logp under no_grad
  * sample:  squashed_sample_raw_torch with the caller's eps                         / eager: the same under no_grad with the same eps
  * grad:    squashed_grad_torch with g_action and g_logp                            / eager: forward with grad + autograd.grad
  * step:    one closed-loop step: squashed_act_torch + step_torch                   / eager act + step_torch
Stream events around back-to-back calls after a warm-up; median, 10th and 90th percentile over the repetitions, microseconds, the
host side of every call included.  Each n runs in a child process of its own under a time limit.  One JSON line per n.
    python tools/gpu_squashed_cost.py [out.jsonl]"""
import json
import math
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ENV_ID, HIDDEN, LIMIT_S = "GoalContinuous3P-v0", 64, 240
BOUNDS = (-20.0, 2.0)


def measure(n):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import torch
    import space_gym_amd as sg
    from gpu_policy_cost import timed

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    env = sg.make_vec(ENV_ID, n, device=0, seed=1)
    D = env.obs_dim
    actor = torch.nn.Sequential(torch.nn.Linear(D, HIDDEN), torch.nn.ReLU(), torch.nn.Linear(HIDDEN, HIDDEN), torch.nn.ReLU(),
                                torch.nn.Linear(HIDDEN, 4)).to(dev)
    params = list(actor.parameters())
    sp = env.squashed_policy_torch(actor=[(l.weight, l.bias) for l in actor if isinstance(l, torch.nn.Linear)], log_std_bounds=BOUNDS,
                                   activation="relu")
    obs = env.reset_torch().clone()
    eps = torch.randn((n, 2), device=dev)
    ga, gl = torch.randn((n, 2), device=dev), torch.randn(n, device=dev)
    out = dict(action=torch.empty((n, 2), device=dev), logp=torch.empty(n, device=dev))
    step_out = dict(obs=torch.empty((n, D), device=dev), reward=torch.empty(n, device=dev), done=torch.empty(n, dtype=torch.uint8, device=dev),
                    trunc=torch.empty(n, dtype=torch.uint8, device=dev))
    grads = env.squashed_grad_torch(sp, obs, eps, ga, gl)

    def eager(e):
        head = actor(obs)
        ls = head[:, 2:].clamp(*BOUNDS)
        u = head[:, :2] + ls.exp() * e
        a = torch.tanh(u)
        lp = (-0.5 * e * e - ls - 0.5 * math.log(2 * math.pi) - 2.0 * (math.log(2.0) - u - torch.nn.functional.softplus(-2.0 * u))).sum(-1)
        return a, lp

    def eager_act():
        with torch.no_grad():
            return eager(torch.randn((n, 2), device=dev))

    def eager_sample():
        with torch.no_grad():
            return eager(eps)

    def eager_grad():
        a, lp = eager(eps)
        return torch.autograd.grad((ga * a).sum() + (gl * lp).sum(), params)

    def fused_step():
        env.squashed_act_torch(sp, obs, seed=1, step=0, out=out)
        env.step_torch(out["action"], out=step_out)

    def eager_step():
        env.step_torch(eager_act()[0], out=step_out)

    mine = [t for pair in grads["actor"] for t in pair]
    agree = max(float((a - b).abs().max()) for a, b in zip(mine, eager_grad()))
    a_f, lp_f = env.squashed_sample_raw_torch(sp, obs, eps)
    a_e, lp_e = eager_sample()
    reps, inner = 15, 20
    rec = dict(env_id=ENV_ID, n=n, hidden=HIDDEN, n_hidden=2, max_abs_grad_diff_vs_eager=agree,
               max_abs_action_diff_vs_eager=float((a_f - a_e).abs().max()), max_abs_logp_diff_vs_eager=float((lp_f - lp_e).abs().max()),
               act_us=timed(lambda: env.squashed_act_torch(sp, obs, seed=1, step=0, out=out), reps, inner),
               eager_act_us=timed(eager_act, reps, inner),
               sample_us=timed(lambda: env.squashed_sample_raw_torch(sp, obs, eps, out=out), reps, inner),
               eager_sample_us=timed(eager_sample, reps, inner),
               grad_us=timed(lambda: env.squashed_grad_torch(sp, obs, eps, ga, gl, out=grads), reps, inner),
               eager_grad_us=timed(eager_grad, reps, inner),
               step_us=timed(fused_step, reps, inner), eager_step_us=timed(eager_step, reps, inner))
    env.check_status()
    env.close()
    return rec


def main():
    if "--n" in sys.argv:  # the child: one n
        print(json.dumps(measure(int(sys.argv[sys.argv.index("--n") + 1]))), flush=True)
        return 0
    paths = [a for a in sys.argv[1:] if not a.startswith("--")]
    for n in (4096, 65536):
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--n", str(n)], stdout=subprocess.PIPE, text=True, timeout=LIMIT_S)
        if done.returncode != 0:  # nothing more is started on the device after a failure
            print(f"n = {n}: the measurement ended with status {done.returncode}", file=sys.stderr)
            return 1
        line = done.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        for p in paths:
            with open(p, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
