#!/usr/bin/env python3
"""Measurement: what the fused actor update (q_actor_grad_torch: sg_q_actor_squashed_grad_device, two launches) costs at
GoalContinuous3P-v0 with a squashed actor and twin critics of two hidden layers of 64 (relu), n = 4 096 and n = 65 536 rows, in SAC's
form (alpha 0.2, the minimum of the two critics), against two compositions of existing calls on the same batch:
  * fused:     q_actor_grad_torch(sp, q, obs, eps), no per-row outputs
  * fused_rows the same with all eight per-row outputs
  * raw:       squashed_sample_raw_torch; q_evaluate_raw_torch; the selection and the loss gradients in torch; q_grad_torch(params=False,
               action_grad=True), which runs both critics' forwards again; squashed_grad_torch, which runs the actor's forward again
  * autograd:  squashed_sample_torch, q_evaluate_torch, (alpha logp - minimum(q1, q2)).mean().backward()
  * learner:   q_actor_update_torch: fused_rows' call and adam_step_torch
ROUNDS rounds alternate the forms; within a round every figure is the median over 15 repetitions of 20 back-to-back calls between
stream events after a warm-up, the host side of every call included.  Reported per n: the median over the rounds and the spread over
the rounds (largest minus smallest round median) of each, microseconds, and whether fused is under raw by more than either form's
spread.  fused's and raw's gradients are compared to the bit (raw feeds squashed_grad_torch the g_action it formed itself, so the two
agree only if every step before agrees too); both and autograd's are held to the float64 model of tests/q_actor_model.py under the
project's rule, 8 x max|G32seq - G64| + 1e-6 (1 + max|G64|) per tensor.  Each n runs in a child process of its own under a time limit.
One JSON line per n; the exit status is 2 when the fused call is not under raw by more than either spread at a size, or the gradients'
bits or the rule fail.

Expected, written down before the first run, from the parts' own profiles (profiles/squashed_cost.txt, profiles/q_cost.txt); the sums
are arithmetic on those figures, nobody has measured them: raw is 38 + 89 + about 40 of elementwise launches + 188 + 146, about 500 us
at 4 096 rows, and 39 + 90 + 40 + 375 + 334, about 880 us at 65 536.  The fused kernel with a forward-only first step would be a forward
at 50, then the critics' walk and the actor's backward, about 385 / 810 us; its first step is a whole policy_grad_net with a zero dz (the
forward half as a function of its own changed the registers of the existing grad kernels), whose walk down without the MFMA costs about
what the forward does: about 425 us at 4 096 rows and 900 us at 65 536 -- under raw at the small size, and at the large one within
run-to-run spread of it, over rather than under.  autograd runs raw's launches and a few more elementwise ones: about 520 / 900 us.
    python tools/gpu_q_actor_cost.py [out.jsonl]"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ENV_ID, HIDDEN, LIMIT_S, ROUNDS, ALPHA = "GoalContinuous3P-v0", 64, 400, 5, 0.2
EXPECTED_US = {"fused": {4096: 425.0, 65536: 900.0}, "raw": {4096: 500.0, 65536: 880.0}, "autograd": {4096: 520.0, 65536: 900.0}}


def measure(n):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import space_gym_amd as sg
    from gpu_policy_cost import timed
    import q_actor_model

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    env = sg.make_vec(ENV_ID, n, device=0, seed=1)
    D = env.obs_dim
    mlp = lambda i, o: torch.nn.Sequential(torch.nn.Linear(i, HIDDEN), torch.nn.ReLU(), torch.nn.Linear(HIDDEN, HIDDEN), torch.nn.ReLU(),
                                           torch.nn.Linear(HIDDEN, o)).to(dev)
    pairs = lambda net: [(l.weight, l.bias) for l in net if isinstance(l, torch.nn.Linear)]
    actor, critics = mlp(D, 4), [mlp(D + 2, 1), mlp(D + 2, 1)]
    for net in critics:
        for p in net.parameters():
            p.requires_grad_(False)
    params = list(actor.parameters())
    sp = env.squashed_policy_torch(actor=pairs(actor), activation="relu")
    q = env.q_torch(critics=[pairs(m) for m in critics], activation="relu")
    obs = env.reset_torch().clone()
    eps = torch.randn((n, 2), device=dev)
    rows = {k: torch.empty((n, 2) if c == 2 else (n,), device=dev) for k, c in env._Q_ACTOR_ROWS.items()}
    grads, stats = env.q_actor_grad_torch(sp, q, obs, eps, alpha=ALPHA)

    def fused():
        env.q_actor_grad_torch(sp, q, obs, eps, alpha=ALPHA, out=grads, stats=stats)

    def fused_rows():
        env.q_actor_grad_torch(sp, q, obs, eps, alpha=ALPHA, rows=rows, out=grads, stats=stats)

    sample = dict(action=torch.empty((n, 2), device=dev), logp=torch.empty(n, device=dev))
    fwd = dict(q1=torch.empty(n, device=dev), q2=torch.empty(n, device=dev))
    back = dict(critics=None, action=torch.empty((n, 2), device=dev))
    raw_grads = env.squashed_grad_torch(sp, obs, eps, g_action=back["action"], g_logp=sample["logp"])
    g_logp = torch.full((n,), ALPHA, device=dev) / n

    def raw():  # the step the README gave before this call existed
        a, logp = env.squashed_sample_raw_torch(sp, obs, eps, out=sample)
        q1, q2 = env.q_evaluate_raw_torch(q, obs, a, out=fwd)
        sel2 = q2 < q1
        g1, g2 = torch.where(sel2, 0.0, -1.0 / n), torch.where(sel2, -1.0 / n, 0.0)
        env.q_grad_torch(q, obs, a, g_q1=g1, g_q2=g2, params=False, action_grad=True, out=back)
        env.squashed_grad_torch(sp, obs, eps, g_action=back["action"], g_logp=g_logp, out=raw_grads)
        return (ALPHA * logp - torch.where(sel2, q2, q1)).mean()

    def autograd():
        for p in params:
            p.grad = None
        a, logp = env.squashed_sample_torch(sp, obs, eps)
        q1, q2 = env.q_evaluate_torch(q, obs, a)
        loss = (ALPHA * logp - torch.minimum(q1, q2)).mean()
        loss.backward()
        return loss

    loss_raw, loss_auto = raw(), autograd()
    fused()
    torch.cuda.synchronize()
    flat_grads = [t for pair in grads["actor"] for t in pair]
    flat_raw = [t for pair in raw_grads["actor"] for t in pair]
    # (raw forms g_action as g_qc dQ_c / da with g_qc = -1 / n where the kernel divides -dQ_c / da by n: the same value where 1 / n is
    # exact, else one rounding apart; so the bits are compared on the fused call's own g_action as well)
    env.q_actor_grad_torch(sp, q, obs, eps, alpha=ALPHA, rows=rows, out=grads, stats=stats)
    exact = env.squashed_grad_torch(sp, obs, eps, g_action=rows["g_action"], g_logp=g_logp)
    torch.cuda.synchronize()
    equal_bits = all(torch.equal(a, b) for a, b in zip(flat_grads, [t for pair in exact["actor"] for t in pair]))
    raw_equal_bits = all(torch.equal(a, b) for a, b in zip(flat_grads, flat_raw))
    raw_diff = max(float((a - b).abs().max()) for a, b in zip(flat_grads, flat_raw))
    auto_diff = max(float((g - p.grad).abs().max()) for g, p in zip(flat_grads, params))
    loss_diff = max(abs(float(stats[0]) - float(loss_raw)), abs(float(stats[0]) - float(loss_auto)))
    host = lambda t: t.detach().cpu().numpy()
    nets = lambda m: [(host(w), host(b)) for w, b in pairs(m)]
    m64, m32 = (q_actor_model.actor_grad(nets(actor), [nets(m) for m in critics], host(obs), host(eps), alpha=ALPHA, form="squashed",
                                         bounds=sp.log_std_bounds, activation="relu", dtype=dt) for dt in (np.float64, np.float32))
    g64, g32 = q_actor_model.flat(m64), q_actor_model.flat(m32)
    worst = {"fused": 0.0, "raw": 0.0, "autograd": 0.0}
    for (name, ref), g, r, p in zip(g64.items(), flat_grads, flat_raw, params):
        tol = 8.0 * float(np.abs(g32[name].astype(np.float64) - ref).max()) + 1e-6 * (1.0 + float(np.abs(ref).max()))
        for form, t in (("fused", g), ("raw", r), ("autograd", p.grad)):
            worst[form] = max(worst[form], float(np.abs(host(t).astype(np.float64) - ref).max()) / tol)
    opt = env.adam_torch(sp, lr=1e-4)  # the learner step moves the parameters: measured last

    def learner():
        env.q_actor_update_torch(sp, q, opt, obs, eps, alpha=ALPHA, rows=rows, grads=grads, stats=stats)

    reps, inner = 15, 20
    rounds = {"fused": [], "raw": [], "autograd": [], "fused_rows": []}
    for _ in range(ROUNDS):
        for name, fn in (("fused", fused), ("raw", raw), ("autograd", autograd), ("fused_rows", fused_rows)):
            rounds[name].append(timed(fn, reps, inner)[0])
    rec = dict(env_id=ENV_ID, n=n, hidden=HIDDEN, n_hidden=2, n_critics=2, rounds=ROUNDS, gradients_equal_the_composed_calls_bits=bool(equal_bits),
               gradients_equal_raws_bits=bool(raw_equal_bits),
               max_abs_grad_diff_vs_raw=raw_diff, max_abs_grad_diff_vs_autograd=auto_diff, loss_diff_vs_compositions=loss_diff,
               worst_grad_error_over_tolerance=worst, gradients_within_the_rule=bool(max(worst.values()) <= 1.0))
    for name, v in rounds.items():
        rec[name + "_us"] = round(float(np.median(v)), 2)
        rec[name + "_spread_us"] = round(float(max(v) - min(v)), 2)
        rec[name + "_rounds_us"] = v
    rec["learner_us"] = round(float(timed(learner, reps, inner)[0]), 2)
    rec["saved_us"] = round(rec["raw_us"] - rec["fused_us"], 2)
    rec["under_raw_by_more_than_either_spread"] = bool(rec["raw_us"] - rec["fused_us"] > max(rec["raw_spread_us"], rec["fused_spread_us"]))
    rec["expected_us"] = {k: v[n] for k, v in EXPECTED_US.items()}
    rec["expectation_error"] = {k: round(rec[k + "_us"] / EXPECTED_US[k][n] - 1.0, 3) for k in EXPECTED_US}
    env.check_status()
    env.close()
    return rec


def main():
    if "--n" in sys.argv:  # the child: one n
        print(json.dumps(measure(int(sys.argv[sys.argv.index("--n") + 1]))), flush=True)
        return 0
    paths = [a for a in sys.argv[1:] if not a.startswith("--")]
    missed = []
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
        rec = json.loads(line)
        missed += [(n, k) for k in ("under_raw_by_more_than_either_spread", "gradients_equal_the_composed_calls_bits", "gradients_equal_raws_bits",
                                    "gradients_within_the_rule") if not rec[k]]
    for n, k in missed:  # every size is measured and written first; a missed requirement then fails the run
        print(f"n = {n}: {k} is false", file=sys.stderr)
    return 2 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
