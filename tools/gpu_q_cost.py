#!/usr/bin/env python3
"""Measurement: what the off-policy learner's nets cost at GoalContinuous3P-v0 with two Q critics and an actor of two hidden layers of
64 (relu), n = 4 096 and n = 65 536 rows -- the engine's kernels against the same computation in eager torch (nn.Sequential on
torch.cat([obs, action], 1), autograd).
  * q_evaluate:          q_evaluate_raw_torch (one launch, both critics)            / eager: the two forwards under no_grad
  * q_grad:              q_grad_torch with params and the action gradient           / eager: autograd.grad to the parameters and the action
  * q_grad_action_only:  q_grad_torch(params=False, action_grad=True)               / eager: autograd.grad to the action alone
  * update:              the TD3 critic step and actor step through q_evaluate_torch / policy_action_torch and backward()
                                                                                    / eager: the same two losses on the modules
Stream events around back-to-back calls after a warm-up; median, 10th and 90th percentile over the repetitions, microseconds, the
host side of every call included.  Each n runs in a child process of its own under a time limit.  One JSON line per n.
    python tools/gpu_q_cost.py [out.jsonl]"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ENV_ID, HIDDEN, LIMIT_S = "GoalContinuous3P-v0", 64, 240


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

    def net(inp, out):
        return torch.nn.Sequential(torch.nn.Linear(inp, HIDDEN), torch.nn.ReLU(), torch.nn.Linear(HIDDEN, HIDDEN), torch.nn.ReLU(),
                                   torch.nn.Linear(HIDDEN, out)).to(dev)
    c1, c2, actor = net(D + 2, 1), net(D + 2, 1), net(D, 2)
    log_std = torch.nn.Parameter(torch.full((2,), -0.5, device=dev))
    c_params = list(c1.parameters()) + list(c2.parameters())
    a_params = list(actor.parameters()) + [log_std]
    linears = lambda m: [(l.weight, l.bias) for l in m if isinstance(l, torch.nn.Linear)]  # noqa: E731
    q = env.q_torch(critics=[linears(c1), linears(c2)], activation="relu")
    pol = env.policy_torch(actor=linears(actor), log_std=log_std, activation="relu")
    obs = env.reset_torch().clone()
    action = torch.randn((n, 2), device=dev).clamp(-1, 1)
    y = torch.randn(n, device=dev)
    g1, g2 = torch.randn(n, device=dev), torch.randn(n, device=dev)
    fwd = dict(q1=torch.empty(n, device=dev), q2=torch.empty(n, device=dev))
    full = env.q_grad_torch(q, obs, action, g1, g2, action_grad=True)
    only = env.q_grad_torch(q, obs, action, g1, g2, params=False, action_grad=True)

    def clear():
        for p in c_params + a_params:
            p.grad = None

    def eager_q(a):
        x = torch.cat([obs, a], 1)
        return c1(x)[:, 0], c2(x)[:, 0]

    def eager_forward():
        with torch.no_grad():
            eager_q(action)

    def eager_grad(with_params):
        a = action.detach().requires_grad_()
        q1, q2 = eager_q(a)
        torch.autograd.grad((g1 * q1).sum() + (g2 * q2).sum(), (c_params if with_params else []) + [a])

    def fused_update():
        clear()
        q1, q2 = env.q_evaluate_torch(q, obs, action)
        ((q1 - y).square().mean() + (q2 - y).square().mean()).backward()
        q1pi, _ = env.q_evaluate_torch(q, obs, env.policy_action_torch(pol, obs))
        (-q1pi.mean()).backward()

    def eager_update():
        clear()
        q1, q2 = eager_q(action)
        ((q1 - y).square().mean() + (q2 - y).square().mean()).backward()
        (-c1(torch.cat([obs, actor(obs)], 1))[:, 0].mean()).backward()

    fused_update()
    mine = [p.grad.clone() for p in c_params + a_params[:-1]]
    eager_update()
    agree = max(float((a - p.grad).abs().max()) for a, p in zip(mine, c_params + a_params[:-1]))
    reps, inner = 15, 20
    rec = dict(env_id=ENV_ID, n=n, hidden=HIDDEN, n_hidden=2, n_critics=2, max_abs_grad_diff_vs_eager=agree,
               q_evaluate_us=timed(lambda: env.q_evaluate_raw_torch(q, obs, action, out=fwd), reps, inner),
               eager_q_evaluate_us=timed(eager_forward, reps, inner),
               q_grad_us=timed(lambda: env.q_grad_torch(q, obs, action, g1, g2, action_grad=True, out=full), reps, inner),
               eager_q_grad_us=timed(lambda: eager_grad(True), reps, inner),
               q_grad_action_only_us=timed(lambda: env.q_grad_torch(q, obs, action, g1, g2, params=False, action_grad=True, out=only), reps, inner),
               eager_q_grad_action_only_us=timed(lambda: eager_grad(False), reps, inner),
               update_us=timed(fused_update, reps, inner), eager_update_us=timed(eager_update, reps, inner))
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
