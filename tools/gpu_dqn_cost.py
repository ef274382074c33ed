#!/usr/bin/env python3
"""Measurement: what the DQN head costs at GoalDiscrete3-v0 with two hidden layers of 64 (relu), n = 4 096 and n = 65 536 envs / rows --
the engine's kernels against the same computation in eager torch (nn.Sequential, argmax, gather, autograd), and the act against
policy_act_torch of a discrete actor of the same shape without a critic.
  * act:      dqn_act_torch with a per-env epsilon tensor (one launch)            / eager: forward, argmax, rand, randint, where, gather
  * step:     one closed-loop step: dqn_act_torch + step_torch                    / eager act + step_torch
  * evaluate: dqn_evaluate_raw_torch, all four outputs                            / eager: forward, gather, max under no_grad
  * grad:     dqn_grad_torch with g_taken and g_all                               / eager: forward with grad + autograd.grad
  * update:   a Double DQN update through autograd: argmax of the online net and q_taken of the target net on next_obs under no_grad,
              Huber loss on dqn_evaluate_torch's q_taken, backward()              / the same in eager torch
Stream events around back-to-back calls after a warm-up; median, 10th and 90th percentile over the repetitions, microseconds, the
host side of every call included.  Each n runs in a child process of its own under a time limit.  One JSON line per n.

Expected, written down before the first run: the act and the evaluate kernel have squashed_act_kernel's shape (the same policy_net, a
head padded to 8), so both should cost about what squashed_act_torch costs at this shape -- 39 us at either n
(profiles/squashed_cost.txt); grad is squashed_grad_torch's two launches with another dz at the head: about 334 us at 65 536 rows and
146 us at 4 096.
    python tools/gpu_dqn_cost.py [out.jsonl]"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ENV_ID, HIDDEN, LIMIT_S = "GoalDiscrete3-v0", 64, 300
EXPECTED_US = {"act": 39.0, "evaluate": 39.0, "grad": {65536: 334.0, 4096: 146.0}}


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
    mlp = lambda: torch.nn.Sequential(torch.nn.Linear(D, HIDDEN), torch.nn.ReLU(), torch.nn.Linear(HIDDEN, HIDDEN), torch.nn.ReLU(),
                                      torch.nn.Linear(HIDDEN, 6)).to(dev)
    pairs = lambda net: [(l.weight, l.bias) for l in net if isinstance(l, torch.nn.Linear)]
    online, target, actor = mlp(), mlp(), mlp()
    for p in target.parameters():
        p.requires_grad_(False)
    params = list(online.parameters())
    ho, ht = env.dqn_torch(net=pairs(online)), env.dqn_torch(net=pairs(target))
    pol = env.policy_torch(actor=pairs(actor), activation="relu")
    obs = env.reset_torch().clone()
    next_obs = obs + 0.01 * torch.randn_like(obs)
    action = torch.randint(0, 6, (n,), device=dev, dtype=torch.int32)
    action64 = action.long()
    reward, discount = torch.randn(n, device=dev), torch.full((n,), 0.99, device=dev)
    gt, ga = torch.randn(n, device=dev), torch.randn((n, 6), device=dev)
    eps = torch.full((n,), 0.1, device=dev)
    out = dict(action=torch.empty(n, dtype=torch.int32, device=dev), q=torch.empty(n, device=dev))
    pol_out = dict(action=torch.empty(n, dtype=torch.int32, device=dev), logp=torch.empty(n, device=dev), value=None)
    ev_out = dict(q_all=torch.empty((n, 6), device=dev), q_taken=torch.empty(n, device=dev), q_max=torch.empty(n, device=dev),
                  argmax=torch.empty(n, dtype=torch.int32, device=dev))
    step_out = dict(obs=torch.empty((n, D), device=dev), reward=torch.empty(n, device=dev), done=torch.empty(n, dtype=torch.uint8, device=dev),
                    trunc=torch.empty(n, dtype=torch.uint8, device=dev))
    grads = env.dqn_grad_torch(ho, obs, action, gt, ga)
    huber = torch.nn.functional.smooth_l1_loss

    def eager_act():
        with torch.no_grad():
            q = online(obs)
            a = torch.where(torch.rand(n, device=dev) < eps, torch.randint(0, 6, (n,), device=dev), q.argmax(1))
            return a.to(torch.int32), q.gather(1, a[:, None])[:, 0]

    def eager_evaluate():
        with torch.no_grad():
            q = online(obs)
            mx = q.max(1)
            return q, q.gather(1, action64[:, None])[:, 0], mx.values, mx.indices

    def eager_grad():
        q = online(obs)
        return torch.autograd.grad((gt * q.gather(1, action64[:, None])[:, 0]).sum() + (ga * q).sum(), params)

    def fused_step():
        env.dqn_act_torch(ho, obs, seed=1, step=0, epsilon=eps, out=out)
        env.step_torch(out["action"], out=step_out)

    def eager_step():
        env.step_torch(eager_act()[0], out=step_out)

    def fused_update():
        for p in params:
            p.grad = None
        with torch.no_grad():
            a2 = env.dqn_evaluate_raw_torch(ho, next_obs, out=dict(argmax=ev_out["argmax"]))[3]
            t = reward + discount * env.dqn_evaluate_raw_torch(ht, next_obs, a2, out=dict(q_taken=ev_out["q_taken"]))[1]
        huber(env.dqn_evaluate_torch(ho, obs, action)[1], t).backward()

    def eager_update():
        for p in params:
            p.grad = None
        with torch.no_grad():
            a2 = online(next_obs).argmax(1)
            t = reward + discount * target(next_obs).gather(1, a2[:, None])[:, 0]
        huber(online(obs).gather(1, action64[:, None])[:, 0], t).backward()

    mine = [t for pair in grads["net"] for t in pair]
    agree = max(float((a - b).abs().max()) for a, b in zip(mine, eager_grad()))
    q_f = env.dqn_evaluate_raw_torch(ho, obs, action)
    q_e = eager_evaluate()
    fused_update()
    upd = [p.grad.clone() for p in params]
    eager_update()
    agree_update = max(float((a - p.grad).abs().max()) for a, p in zip(upd, params))
    reps, inner = 15, 20
    rec = dict(env_id=ENV_ID, n=n, hidden=HIDDEN, n_hidden=2, max_abs_grad_diff_vs_eager=agree, max_abs_update_grad_diff_vs_eager=agree_update,
               max_abs_q_diff_vs_eager=float((q_f[0] - q_e[0]).abs().max()), argmax_disagreements_vs_eager=int((q_f[3] != q_e[3]).sum()),
               act_us=timed(lambda: env.dqn_act_torch(ho, obs, seed=1, step=0, epsilon=eps, out=out), reps, inner),
               eager_act_us=timed(eager_act, reps, inner),
               policy_act_us=timed(lambda: env.policy_act_torch(pol, obs, seed=1, step=0, out=pol_out), reps, inner),
               step_us=timed(fused_step, reps, inner), eager_step_us=timed(eager_step, reps, inner),
               evaluate_us=timed(lambda: env.dqn_evaluate_raw_torch(ho, obs, action, out=ev_out), reps, inner),
               eager_evaluate_us=timed(eager_evaluate, reps, inner),
               grad_us=timed(lambda: env.dqn_grad_torch(ho, obs, action, gt, ga, out=grads), reps, inner),
               eager_grad_us=timed(eager_grad, reps, inner),
               update_us=timed(fused_update, reps, inner), eager_update_us=timed(eager_update, reps, inner),
               expected_us=dict(act=EXPECTED_US["act"], evaluate=EXPECTED_US["evaluate"], grad=EXPECTED_US["grad"][n]))
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
