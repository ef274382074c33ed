#!/usr/bin/env python3
"""Measurement: what a population of P small actor-critics costs per call at 65 536 envs of GoalContinuous3P-v0 -- actor and critic of
two hidden layers of 64 (tanh), P in {1, 4, 16, 64, 256}, member m on the env block [m B / P, (m + 1) B / P).
  * act:       population_act_torch (one launch for all members)
  * step:      a closed-loop step, rollout_population_torch(K = 32) per step, without and with the dense terminal_value (one more
               critic-only launch per step); rollout_policy_torch of ONE policy per step beside them
  * evaluate:  population_evaluate_raw_torch at n = 65 536 / P rows per member
  * grad:      population_grad_torch at the same n, all three g given
Baselines, both of them what the engine offered before the population calls:
  * single x P: policy_act_torch on the whole [B, D] batch (a member's block cannot be had for less), policy_evaluate_raw_torch and
    policy_grad_torch of one member on its n rows -- one call measured, multiplied by P;
  * eager: torch.baddbmm over the stacked tensors, Normal.sample / log_prob / entropy, autograd.grad for the gradients.

EXPECTATION, written down before the first run (a net call's time is one workgroup's chain of staged layers whatever
the batch up to 65 536 rows):
  * act and evaluate at ANY P cost what P = 1 costs -- the same number of workgroups, each running the same chain, plus P weight sets
    (2 x 5.3 k floats each: 10.9 MB at P = 256, resident in L2) instead of one;
  * P = 1 costs what policy_act_torch / policy_evaluate_raw_torch cost (the same kernel body plus one multiply per pointer);
  * grad at P = 1 equals policy_grad_torch (the same grouping: 256 workgroups); at larger P each member has 256 / P workgroups
    for 65 536 / P rows, so every workgroup still takes the same number of row tiles and the time should stay P = 1's too;
  * so the population call is ~P x cheaper than "single x P", and ~4.6 x cheaper than eager (section 17's figure) at any P;
  * the dense terminal_value adds one critic-only launch per step: about half an act launch (one net of the two).
Every figure is reported against these; one that contradicts them is reported as such.

Stream events around back-to-back calls after a warm-up; median, 10th and 90th percentile over the repetitions, microseconds, the host
side of every call included.  One JSON line per P, and the report.
    python tools/gpu_population_cost.py [report.txt]        (default: profiles/population_cost.txt)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import space_gym_amd as sg  # noqa: E402

ENV_ID, B, K, HIDDEN = "GoalContinuous3P-v0", 65536, 32, 64
MEMBERS = (1, 4, 16, 64, 256)


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


def stacked_net(P, D, out, dev, gen):
    dims = [D, HIDDEN, HIDDEN, out]
    u = lambda *shape, fan: (torch.rand(shape, device=dev, generator=gen) * 2 - 1) / fan ** 0.5  # noqa: E731
    return [(u(P, o, i, fan=i), u(P, o, fan=i)) for i, o in zip(dims[:-1], dims[1:])]


def forward(layers, x):
    """[P, n, in] -> [P, n, out]: one baddbmm per layer over the stacked tensors"""
    h = x
    for l, (W, b) in enumerate(layers):
        h = torch.baddbmm(b[:, None, :], h, W.transpose(1, 2))
        if l < len(layers) - 1:
            h = torch.tanh(h)
    return h


def measure(env, P, dev, gen, reps, inner):
    D, n = env.obs_dim, B // P
    actor, critic = stacked_net(P, D, 2, dev, gen), stacked_net(P, D, 1, dev, gen)
    log_std = torch.full((P, 2), -0.5, device=dev)
    pop = env.policy_population_torch(P, actor=actor, critic=critic, log_std=log_std)
    one = env.population_member_torch(pop, 0)
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)  # noqa: E731
    buf = dict(obs=z(K + 1, B, D), action=z(K, B, 2), logp=z(K, B), value=z(K + 1, B), reward=z(K, B), done=z(K, B, dtype=torch.uint8),
               trunc=z(K, B, dtype=torch.uint8))
    buf["obs"][0].copy_(env.reset_torch())
    dense = z(K, B)
    obs = buf["obs"][0]
    out = dict(action=buf["action"][0], logp=buf["logp"][0], value=buf["value"][0])
    rows = obs.view(P, n, D)
    act_rows = torch.randn((P, n, 2), device=dev, generator=gen)
    g = [torch.randn((P, n), device=dev, generator=gen) for _ in range(3)]
    ev_out = {k: z(P, n) for k in ("logp", "entropy", "value")}
    ev_one = {k: z(n) for k in ("logp", "entropy", "value")}
    grads = env.population_grad_torch(pop, rows, act_rows, *g)
    grads_one = env.policy_grad_torch(one, rows[0], act_rows[0], *[x[0] for x in g])
    params = [t for pair in actor + critic for t in pair] + [log_std]

    def eager_act():
        with torch.no_grad():
            dist = torch.distributions.Normal(forward(actor, rows), log_std.exp()[:, None, :])
            a = dist.sample()
            return a, dist.log_prob(a).sum(-1), forward(critic, rows)[..., 0]

    def eager_scores():
        dist = torch.distributions.Normal(forward(actor, rows), log_std.exp()[:, None, :])
        return dist.log_prob(act_rows).sum(-1), dist.entropy().sum(-1), forward(critic, rows)[..., 0]

    def eager_evaluate():
        with torch.no_grad():
            return eager_scores()

    def eager_grad():
        for t in params:
            t.requires_grad_(True)
        logp, ent, value = eager_scores()
        res = torch.autograd.grad((g[0] * logp + g[1] * ent + g[2] * value).sum(), params)
        for t in params:
            t.requires_grad_(False)
        return res

    # the paths compute the same thing
    lp, en, v = env.population_evaluate_raw_torch(pop, rows, act_rows, out=ev_out)
    elp, een, ev = eager_evaluate()
    eg = eager_grad()
    agree = dict(logp=float((lp - elp).abs().max()), value=float((v - ev).abs().max()),
                 grad_rel=max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
                              for a, b in zip([t for pair in grads["actor"] + grads["critic"] for t in pair] + [grads["log_std"]], eg)))
    k_reps = max(3, reps // 3)
    rec = dict(
        members=P, rows_per_member=n, max_abs_diff_vs_eager=agree,
        act_us=timed(lambda: env.population_act_torch(pop, obs, seed=3, step=0, out=out), reps, inner),
        act_single_us=timed(lambda: env.policy_act_torch(one, obs, seed=3, step=0, out=out), reps, inner),
        act_eager_us=timed(eager_act, reps, inner),
        step_us=timed(lambda: env.rollout_population_torch(pop, seed=3, **buf), k_reps, 2, per=K),
        step_dense_tv_us=timed(lambda: env.rollout_population_torch(pop, seed=3, terminal_value=dense, **buf), k_reps, 2, per=K),
        step_single_us=timed(lambda: env.rollout_policy_torch(one, seed=3, **buf), k_reps, 2, per=K),
        evaluate_us=timed(lambda: env.population_evaluate_raw_torch(pop, rows, act_rows, out=ev_out), reps, inner),
        evaluate_single_us=timed(lambda: env.policy_evaluate_raw_torch(one, rows[0], act_rows[0], out=ev_one), reps, inner),
        evaluate_eager_us=timed(eager_evaluate, reps, inner),
        grad_us=timed(lambda: env.population_grad_torch(pop, rows, act_rows, *g, out=grads), reps, inner),
        grad_single_us=timed(lambda: env.policy_grad_torch(one, rows[0], act_rows[0], *[x[0] for x in g], out=grads_one), reps, inner),
        grad_eager_us=timed(eager_grad, reps, max(1, inner // 5)),
        grad_workspace_bytes=int(pop.workspace.numel()))
    env.check_status()
    return rec


def report(recs, reps, inner):
    f = lambda t: "%8.2f [%7.2f, %7.2f]" % tuple(t)  # noqa: E731
    lines = [
        "Cost of a population of P actor-critics per call: population_act_torch / rollout_population_torch / population_evaluate_raw_torch /",
        "population_grad_torch (sg_policy_population_*) against P single-policy calls and against eager torch.baddbmm on the stacked",
        "tensors.  MI355X, tools/gpu_population_cost.py, one run; stream events around back-to-back calls after a warm-up, %d repetitions" % reps,
        "of %d calls (rollouts: K = %d, per step); microseconds: median [p10, p90], the host side of every call included." % (inner, K),
        "",
        "%s, %d envs, actor and critic of two hidden layers of %d, tanh; member m on env block m; n = %d / P rows per member" % (ENV_ID, B, HIDDEN, B),
        "",
        "Expectation written into the tool before the run: act and evaluate at any P cost what P = 1 costs, and P = 1 what the single-policy",
        "call costs; grad at P = 1 equals policy_grad_torch and stays there; 'single x P' is P times one single call.",
        ""]
    for r in recs:
        P = r["members"]
        lines += [
            "P = %d  (n = %d rows per member, gradient workspace %.1f MB)" % (P, r["rows_per_member"], r["grad_workspace_bytes"] / 1e6),
            "  act       population %s   one policy_act_torch on [B, D] %s  (x P = %9.1f)   eager bmm %s" % (
                f(r["act_us"]), f(r["act_single_us"]), P * r["act_single_us"][0], f(r["act_eager_us"])),
            "  step      population %s   with dense terminal_value %s   rollout_policy_torch, one policy %s" % (
                f(r["step_us"]), f(r["step_dense_tv_us"]), f(r["step_single_us"])),
            "  evaluate  population %s   one member's n rows         %s  (x P = %9.1f)   eager bmm %s" % (
                f(r["evaluate_us"]), f(r["evaluate_single_us"]), P * r["evaluate_single_us"][0], f(r["evaluate_eager_us"])),
            "  grad      population %s   one member's n rows         %s  (x P = %9.1f)   eager bmm + autograd %s" % (
                f(r["grad_us"]), f(r["grad_single_us"]), P * r["grad_single_us"][0], f(r["grad_eager_us"])),
            "  agreement with eager (max abs logp %.1e, value %.1e; max relative gradient difference %.1e)" % (
                r["max_abs_diff_vs_eager"]["logp"], r["max_abs_diff_vs_eager"]["value"], r["max_abs_diff_vs_eager"]["grad_rel"]),
            ""]
    base = recs[0]
    lines.append("Against the expectation (ratios of medians):")
    for r in recs:
        lines.append("  P = %3d: act %.2f x P = 1's, evaluate %.2f x, grad %.2f x; dense terminal_value adds %.1f us per step; population act / "
                     "single act %.2f, evaluate / (P x single) %.3f, grad / (P x single) %.3f" % (
                         r["members"], r["act_us"][0] / base["act_us"][0], r["evaluate_us"][0] / base["evaluate_us"][0],
                         r["grad_us"][0] / base["grad_us"][0], r["step_dense_tv_us"][0] - r["step_us"][0], r["act_us"][0] / r["act_single_us"][0],
                         r["evaluate_us"][0] / (r["members"] * r["evaluate_single_us"][0]), r["grad_us"][0] / (r["members"] * r["grad_single_us"][0])))
    return "\n".join(lines) + "\n"


def main():
    paths = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = paths[0] if paths else os.path.join(ROOT, "profiles", "population_cost.txt")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    env = sg.make_vec(ENV_ID, B, device=0, seed=1)
    reps, inner = 15, 50
    recs = []
    for P in MEMBERS:
        recs.append(measure(env, P, dev, gen, reps, inner))
        print(json.dumps(recs[-1]), flush=True)
    env.close()
    text = report(recs, reps, inner)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
