#!/usr/bin/env python3
"""Measurement: what one PPO minibatch update costs at GoalContinuous3P-v0 with an actor and a critic of two hidden layers of 64 (tanh),
n = 4 096 and n = 65 536 rows -- ppo_grad_torch against the update composed from the calls that were there before it, in the same run,
on the same rows, with the same objective (clip 0.2, value clip 0.2, ent_coef 0.01, vf_coef 0.5, normalised advantages):
  * fused:     ppo_grad_torch(policy, batch, index): advantage statistics, the backward with the loss inside, the reduction
  * composed:  six index_select gathers, policy_evaluate_torch (policy_evaluate_raw_torch forward), the loss in torch, backward()
               (policy_grad_torch): about twenty launches
  * grad:      policy_grad_torch alone on gathered rows, for scale
Expectation, stated before the first run: the fused call costs about the grad kernel plus a few microseconds (one more small launch, the
index loads, the statistics sums), so clearly less than the composed update, which adds the evaluate launch, the gathers and the loss's
elementwise launches to the same grad kernel.

Stream events around back-to-back calls after a warm-up of every timed shape; the two updates are timed in alternating windows of the same
run; median, 10th and 90th percentile over the windows, microseconds, the host side of every call included.  Writes the text profile
(default profiles/ppo_cost.txt) and prints one JSON line per n.
    python tools/gpu_ppo_cost.py [profile.txt]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402

ENV_ID, HIDDEN = "GoalContinuous3P-v0", 64
CLIP, CLIP_VF, ENT, VF = 0.2, 0.2, 0.01, 0.5
REPS, INNER = 20, 50


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / INNER


def alternating(fns):
    """{name: [median, p10, p90]} microseconds per call, the functions timed in alternating windows after a warm-up of each"""
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            out[k].append(window(fn))
    return {k: [round(float(x), 2) for x in (np.median(v), np.percentile(v, 10), np.percentile(v, 90))] for k, v in out.items()}


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
    action, logp, value = env.policy_act_torch(pol, obs, seed=3, step=0)
    batch = dict(obs=obs, action=action, logp=logp + 0.1 * torch.randn(n, device=dev), value=value + 0.1 * torch.randn(n, device=dev),
                 advantage=torch.randn(n, device=dev), ret=value + torch.randn(n, device=dev))
    index = torch.randperm(n, device=dev)
    grads, stats = env.ppo_grad_torch(pol, batch, index, clip_range=CLIP, clip_range_vf=CLIP_VF, ent_coef=ENT, vf_coef=VF)

    def fused():
        env.ppo_grad_torch(pol, batch, index, clip_range=CLIP, clip_range_vf=CLIP_VF, ent_coef=ENT, vf_coef=VF, out=grads, stats=stats)

    def composed():
        for p in params:
            p.grad = None
        o, a, old, adv, ret, ov = (batch[k].index_select(0, index) for k in ("obs", "action", "logp", "advantage", "ret", "value"))
        lp, ent, v = env.policy_evaluate_torch(pol, o, a)
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        ratio = torch.exp(lp - old)
        pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - CLIP, 1 + CLIP)).mean()
        vl = 0.5 * torch.max((v - ret) ** 2, (ov + torch.clamp(v - ov, -CLIP_VF, CLIP_VF) - ret) ** 2).mean()
        (pg - ENT * ent.mean() + VF * vl).backward()

    obs_g, action_g = obs.index_select(0, index), action.index_select(0, index)
    g = [torch.randn(n, device=dev) / n for _ in range(3)]
    alone = env.policy_grad_torch(pol, obs_g, action_g, *g)
    composed()
    flat = [t for pair in grads["actor"] + grads["critic"] for t in pair] + [grads["log_std"]]
    fused()
    agree = max(float((a - p.grad).abs().max()) for a, p in zip(flat, params))
    top = max(float(p.grad.abs().max()) for p in params)
    us = alternating(dict(fused=fused, composed=composed, grad=lambda: env.policy_grad_torch(pol, obs_g, action_g, *g, out=alone)))
    rec = dict(env_id=ENV_ID, n=n, hidden=HIDDEN, n_hidden=2, fused_us=us["fused"], composed_us=us["composed"], grad_us=us["grad"],
               fused_over_composed=round(us["fused"][0] / us["composed"][0], 3), fused_minus_grad_us=round(us["fused"][0] - us["grad"][0], 2),
               max_abs_grad_diff_vs_composed=agree, max_abs_grad=top, loss=float(stats[0]))
    env.check_status()
    env.close()
    return rec


def main():
    paths = [a for a in sys.argv[1:] if not a.startswith("--")] or [os.path.join(ROOT, "profiles", "ppo_cost.txt")]
    lines = ["Cost of one PPO minibatch update: ppo_grad_torch (fused) against the update composed of six gathers, policy_evaluate_torch, the loss in",
             "torch and backward() through policy_grad_torch -- the same rows, index and objective, timed in alternating windows of one run.",
             "%s, tools/gpu_ppo_cost.py; stream events around %d back-to-back calls after a warm-up, %d windows each; microseconds:"
             % (torch.cuda.get_device_name(0), INNER, REPS),
             "median [p10, p90], the host side of every call included.",
             "Expected before the run: fused = about the grad kernel plus a few microseconds, clearly under the composed update.", "",
             "%s, actor and critic of two hidden layers of %d" % (ENV_ID, HIDDEN)]
    row = lambda name, v: "  %-48s %8.2f  [%8.2f, %8.2f]" % (name, *v)  # noqa: E731
    for n in (4096, 65536):
        rec = measure(n)
        print(json.dumps(rec), flush=True)
        verdict = "faster" if rec["fused_over_composed"] < 1 else "NOT faster"
        lines += ["", "n = %d rows" % n, row("ppo_grad_torch (fused, two or three launches)", rec["fused_us"]),
                  row("composed update (gathers + evaluate + loss + grad)", rec["composed_us"]),
                  row("policy_grad_torch alone (two launches)", rec["grad_us"]),
                  "  fused / composed = %.3f (the fused call is %s); fused - grad alone = %.2f us"
                  % (rec["fused_over_composed"], verdict, rec["fused_minus_grad_us"]),
                  "  largest difference of a parameter gradient between the two updates: %.2g (largest gradient entry %.2g)"
                  % (rec["max_abs_grad_diff_vs_composed"], rec["max_abs_grad"])]
    for p in paths:
        os.makedirs(os.path.dirname(os.path.abspath(p)), exist_ok=True)
        with open(p, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
