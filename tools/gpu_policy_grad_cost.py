#!/usr/bin/env python3
"""Measurement: what a minibatch of an on-policy update costs at GoalContinuous3P-v0 with an actor and a critic of two hidden layers of
64 (tanh), n = 4 096 and n = 65 536 rows -- the engine's evaluate / grad kernels against the same computation in eager torch.
  * evaluate:        policy_evaluate_raw_torch (one launch: both nets, log-prob, entropy, value)
  * grad:            policy_grad_torch (the backward launch with the forward recomputed inside, and the reduction of the partials)
  * fused_update:    policy_evaluate_torch + a clipped-PPO loss + backward()
  * eager_update:    two nn.Sequential forwards, Normal.log_prob / entropy, the same loss, backward()
  * act_kernel:      policy_act_torch on the same rows, for scale
Stream events around back-to-back calls after a warm-up; median, 10th and 90th percentile over the repetitions, microseconds, the
host side of every call included.  One JSON line per n.
    python tools/gpu_policy_grad_cost.py [out.jsonl]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402
from gpu_policy_cost import timed  # noqa: E402

ENV_ID, HIDDEN = "GoalContinuous3P-v0", 64


def loss_fn(logp, entropy, value, old_logp, adv, ret):
    ratio = torch.exp(logp - old_logp)
    return (-torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv).mean() - 0.01 * entropy.mean() + 0.5 * ((value - ret) ** 2).mean())


def measure(n):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    env = sg.make_vec(ENV_ID, n, device=0, seed=1)
    D = env.obs_dim

    def net(out):
        return torch.nn.Sequential(torch.nn.Linear(D, HIDDEN), torch.nn.Tanh(), torch.nn.Linear(HIDDEN, HIDDEN), torch.nn.Tanh(),
                                   torch.nn.Linear(HIDDEN, out)).to(dev)
    actor, critic = net(2), net(1)
    log_std = torch.nn.Parameter(torch.full((2,), -0.5, device=dev))
    params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
    linears = lambda m: [(l.weight, l.bias) for l in m if isinstance(l, torch.nn.Linear)]  # noqa: E731
    pol = env.policy_torch(actor=linears(actor), critic=linears(critic), log_std=log_std)
    obs = env.reset_torch().clone()
    action, old_logp, _ = env.policy_act_torch(pol, obs, seed=3, step=0)
    old_logp = old_logp + 0.1 * torch.randn(n, device=dev)
    adv, ret = torch.randn(n, device=dev), torch.randn(n, device=dev)
    g = [torch.randn(n, device=dev) for _ in range(3)]
    fwd = {k: torch.empty(n, device=dev) for k in ("logp", "entropy", "value")}
    grads = env.policy_grad_torch(pol, obs, action, *g)

    def clear():
        for p in params:
            p.grad = None

    def fused():
        clear()
        loss_fn(*env.policy_evaluate_torch(pol, obs, action), old_logp, adv, ret).backward()

    def eager():
        clear()
        dist = torch.distributions.Normal(actor(obs), log_std.exp())
        loss_fn(dist.log_prob(action).sum(-1), dist.entropy().sum(-1), critic(obs)[:, 0], old_logp, adv, ret).backward()

    fused()
    mine = [p.grad.clone() for p in params]
    eager()
    agree = max(float((a - p.grad).abs().max()) for a, p in zip(mine, params))
    reps, inner = 15, 20
    rec = dict(env_id=ENV_ID, n=n, hidden=HIDDEN, n_hidden=2, max_abs_grad_diff_vs_eager=agree,
               evaluate_us=timed(lambda: env.policy_evaluate_raw_torch(pol, obs, action, out=fwd), reps, inner),
               grad_us=timed(lambda: env.policy_grad_torch(pol, obs, action, *g, out=grads), reps, inner),
               fused_update_us=timed(fused, reps, inner), eager_update_us=timed(eager, reps, inner),
               act_kernel_us=timed(lambda: env.policy_act_torch(pol, obs, seed=3, step=0), reps, inner))
    env.check_status()
    env.close()
    return rec


def main():
    paths = [a for a in sys.argv[1:] if not a.startswith("--")]
    for n in (4096, 65536):
        line = json.dumps(measure(n))
        print(line, flush=True)
        for p in paths:
            with open(p, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
