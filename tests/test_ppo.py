"""CPU tests of the fused PPO minibatch update (sg_ppo_grad_device / ppo_grad_torch): the declarations, the NumPy model
(tests/ppo_model.py) against torch.autograd on float64 modules with the loss written in plain torch, the branch coverage of the fixed
cases, the bad-index rule, and the Python argument checks with the native calls stubbed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from policy_grad_model import flat
from policy_model import random_policy
from ppo_model import STATS, ppo
from test_episode_stats import _fake_cuda, _stub_env
from test_policy import _params, _torch_net
from test_snapshot_device import _header_args

D, ROWS = 13, 96
VARIANTS = {  # keyword arguments of the model and of the torch loss; index: a minibatch with repeats, else all rows
    "plain": dict(),
    "vclip": dict(clip_range_vf=0.2, ent_coef=0.01),
    "inf": dict(clip_range=float("inf"), ent_coef=0.01, vf_coef=1.0),
    "nocritic": dict(ent_coef=0.02),
    "index": dict(clip_range_vf=0.2, ent_coef=0.01, vf_coef=0.25),
    "raw_adv": dict(normalize_advantage=False, clip_range_vf=0.2),
}


def test_entry_points_and_structs_are_declared_with_the_header_arguments():
    from space_gym_amd import _native, build
    from space_gym_amd.vector_env import SpaceGymVectorEnv
    assert _header_args("sg_ppo_grad_device") == [
        "sg_env *env", "const sg_policy *policy", "const sg_ppo_config *cfg", "const sg_ppo_batch *batch", "int64_t rows", "int64_t n",
        "const sg_policy_grads *grads", "float *stats_out", "const sg_ppo_rows *row_out", "void *workspace", "size_t workspace_bytes",
        "void *hip_stream"]
    assert _header_args("sg_ppo_grad_workspace_bytes", "size_t") == ["sg_env *env", "const sg_policy *policy", "int64_t n"]
    assert _header_args("sg_ppo_config_init", "void") == ["sg_ppo_config *cfg"]
    vp, P = C.c_void_p, C.POINTER
    assert _native.SYMBOLS["sg_ppo_grad_device"] == (C.c_int, [vp, P(_native.SgPolicy), P(_native.SgPpoConfig), P(_native.SgPpoBatch), C.c_int64,
                                                              C.c_int64, P(_native.SgPolicyGrads), vp, P(_native.SgPpoRows), vp, C.c_size_t, vp])
    assert _native.SYMBOLS["sg_ppo_grad_workspace_bytes"] == (C.c_size_t, [vp, P(_native.SgPolicy), C.c_int64])
    header = open(os.path.join(ROOT, "include", "spacegym.h")).read()
    for name, cls, size in (("sg_ppo_config", _native.SgPpoConfig, 32), ("sg_ppo_batch", _native.SgPpoBatch, 56), ("sg_ppo_rows", _native.SgPpoRows, 32)):
        body = re.sub(r"/\*.*?\*/", "", header[header.index("typedef struct %s {" % name):header.index("} %s;" % name)], flags=re.S)
        names = [d.split()[-1].lstrip("*") for d in body.replace("typedef struct %s {" % name, "").split(";") if d.strip()]
        assert names == [f for f, _ in cls._fields_] and C.sizeof(cls) == size, name
    src = open(os.path.join(build.CSRC, "sg_engine.hip")).read()
    assert "sg_ppo.inc" in build.HEADERS and '#include "sg_ppo.inc"' in src
    inc = open(os.path.join(build.CSRC, "sg_ppo.inc")).read()
    assert "policy_grad_net<NT>" in inc and "policy_score(" in inc and "policy_grad_reduce_element(" in inc and "atomic" not in re.sub(r"//.*", "", inc).lower()
    assert SpaceGymVectorEnv.ppo_stats_names == STATS and len(STATS) == 12


def _case(continuous, critic=True, seed=0, rows=ROWS, hidden=33, n_hidden=2):
    """a policy and a flattened rollout whose stored logp / value lie around the current ones, so that both branches of both max occur"""
    from policy_grad_model import evaluate
    rng = np.random.default_rng(seed)
    pol = random_policy(rng, D, hidden, n_hidden, 2 if continuous else 6, critic=critic, continuous=continuous)
    obs = rng.standard_normal((rows, D)).astype(np.float32)
    action = rng.standard_normal((rows, 2)).astype(np.float32) if continuous else rng.integers(0, 6, rows).astype(np.int32)
    return pol, rng, obs, action, evaluate


def _batch(pol, rng, obs, action, evaluate, activation):
    now = evaluate(pol, obs, action, activation=activation, grads=False)
    rows = obs.shape[0]
    batch = dict(obs=obs, action=action, logp=(now["logp"] + 0.3 * rng.standard_normal(rows)).astype(np.float32),
                 advantage=(0.5 + 2.0 * rng.standard_normal(rows)).astype(np.float32))
    if pol["critic"] is not None:
        batch["value"] = (now["value"] + 0.3 * rng.standard_normal(rows)).astype(np.float32)
        batch["ret"] = (now["value"] + rng.standard_normal(rows)).astype(np.float32)
    return batch


def _torch_ppo(pol, batch, index, activation, clip_range=0.2, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True):
    """the loss in plain torch on float64 modules and distributions; an index outside the rows is a row whose terms are masked out and
    whose advantage is 0, the means dividing by n.  Returns (statistics by name, gradients by name)"""
    import torch
    rows = batch["obs"].shape[0]
    idx = np.arange(rows) if index is None else np.asarray(index, np.int64)
    n = len(idx)
    good = (idx >= 0) & (idx < rows)
    r = np.clip(idx, 0, rows - 1)
    t = lambda a: torch.from_numpy(np.asarray(a)[r].astype(np.float64))
    mask = torch.from_numpy(good.astype(np.float64))
    actor = _torch_net(pol["actor"], activation)
    critic = _torch_net(pol["critic"], activation) if pol["critic"] is not None else None
    x = t(batch["obs"])
    head = actor(x)
    if pol["log_std"] is not None:
        ls = torch.from_numpy(pol["log_std"].astype(np.float64)).requires_grad_()
        dist = torch.distributions.Normal(head, ls.exp().expand_as(head))
        logp, ent = dist.log_prob(t(batch["action"])).sum(1), dist.entropy().sum(1)
    else:
        ls = None
        dist = torch.distributions.Categorical(logits=head)
        logp, ent = dist.log_prob(torch.from_numpy(batch["action"][r].astype(np.int64))), dist.entropy()
    lr = logp - t(batch["logp"])
    ratio = lr.exp()
    adv = t(batch["advantage"]) * mask
    mean, std = adv.mean(), adv.std()
    if normalize_advantage:
        adv = (adv - mean) / (std + 1e-8)
    pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range))
    avg = lambda v: (v * mask).sum() / n
    loss = avg(pg) - ent_coef * avg(ent)
    vl = torch.zeros(())
    if critic is not None:
        value, ret = critic(x)[:, 0], t(batch["ret"])
        v = 0.5 * (value - ret) ** 2
        if clip_range_vf is not None:
            ov = t(batch["value"])
            v = 0.5 * torch.max((value - ret) ** 2, (ov + torch.clamp(value - ov, -clip_range_vf, clip_range_vf) - ret) ** 2)
        vl = avg(v)
        loss = loss + vf_coef * vl
    loss.backward()
    lin = lambda net: [m for m in net if isinstance(m, torch.nn.Linear)]
    grads = flat(dict(actor=[(m.weight.grad.numpy(), m.bias.grad.numpy()) for m in lin(actor)],
                      critic=[(m.weight.grad.numpy(), m.bias.grad.numpy()) for m in lin(critic)] if critic is not None else None,
                      log_std=ls.grad.numpy() if ls is not None else None))
    with torch.no_grad():
        stats = dict(loss=loss, policy_loss=avg(pg), value_loss=vl, entropy=avg(ent), approx_kl=avg((ratio - 1) - lr), old_approx_kl=avg(-lr),
                     clip_fraction=avg(((ratio - 1).abs() > clip_range).double()), adv_mean=mean if normalize_advantage else 0.0,
                     adv_std=std if normalize_advantage else 0.0, bad_rows=float((~good).sum()), reserved0=0.0, reserved1=0.0)
    return {k: float(v.detach()) if isinstance(v, torch.Tensor) else float(v) for k, v in stats.items()}, grads


def _assert_equal_to_torch(got, stats, grads, what):
    rel = lambda a, b: float(np.abs(a - b).max()) / max(1e-300, float(np.abs(b).max()))
    for k, name in enumerate(STATS):
        assert abs(float(got["stats"][k]) - stats[name]) <= 1e-10 * abs(stats[name]), (what, name, float(got["stats"][k]), stats[name])
    mine = flat(got)
    assert set(mine) == set(grads), what
    for k in grads:
        assert mine[k].shape == grads[k].shape and np.abs(grads[k]).max() > 0 and rel(mine[k], grads[k]) <= 1e-10, (what, k, rel(mine[k], grads[k]))


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("activation", ["tanh", "relu"])
@pytest.mark.parametrize("continuous", [True, False])
def test_model_equals_torch_autograd_in_float64(continuous, activation, variant):
    kw = VARIANTS[variant]
    pol, rng, obs, action, evaluate = _case(continuous, critic=variant != "nocritic", seed=11)
    batch = _batch(pol, rng, obs, action, evaluate, activation)
    index = rng.integers(0, ROWS, 70) if variant == "index" else None
    got = ppo(pol, batch, index, activation=activation, **kw)
    stats, grads = _torch_ppo(pol, batch, index, activation, **kw)
    _assert_equal_to_torch(got, stats, grads, (continuous, activation, variant))
    assert got["stats"].dtype == np.float64 and got["stats"][9] == 0
    # the fixed cases take both branches of both max: at least 10 % of the rows each (seed 11, chosen on the model alone)
    if np.isfinite(kw.get("clip_range", 0.2)):
        assert 0.1 <= got["pg_unclipped"].mean() <= 0.9, got["pg_unclipped"].mean()
    else:
        assert got["pg_unclipped"].all()
    if "clip_range_vf" in kw:
        assert 0.1 <= got["v_unclipped"].mean() <= 0.9, got["v_unclipped"].mean()
    if variant == "nocritic":
        assert got["critic"] is None and got["stats"][2] == 0 and got["rows"]["value"] is None


def test_per_row_derivatives_are_the_stated_ones():
    """g_logp, g_value of the model against autograd of the torch loss by the three [n] outputs"""
    import torch
    pol, rng, obs, action, evaluate = _case(True, seed=5)
    batch = _batch(pol, rng, obs, action, evaluate, "tanh")
    got = ppo(pol, batch, clip_range_vf=0.2, ent_coef=0.01, normalize_advantage=False)
    now = evaluate(pol, obs, action, grads=False)
    logp, value = [torch.from_numpy(now[k]).requires_grad_() for k in ("logp", "value")]
    t = lambda k: torch.from_numpy(batch[k].astype(np.float64))
    ratio, adv, ov, ret = (logp - t("logp")).exp(), t("advantage"), t("value"), t("ret")
    loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 0.8, 1.2)).mean()
    loss = loss + 0.5 * (0.5 * torch.max((value - ret) ** 2, (ov + torch.clamp(value - ov, -0.2, 0.2) - ret) ** 2)).mean()
    loss.backward()
    assert np.allclose(got["rows"]["g_logp"], logp.grad.numpy(), rtol=1e-12, atol=0) and (got["rows"]["g_logp"] == 0).mean() >= 0.1
    assert np.allclose(got["rows"]["g_value"], value.grad.numpy(), rtol=1e-12, atol=0) and (got["rows"]["g_value"] == 0).mean() >= 0.1


@pytest.mark.parametrize("continuous", [True, False])
def test_an_index_outside_the_rows_changes_nothing_but_the_count(continuous):
    pol, rng, obs, action, evaluate = _case(continuous, seed=3)
    batch = _batch(pol, rng, obs, action, evaluate, "tanh")
    kw = dict(clip_range_vf=0.2, ent_coef=0.01)
    index = rng.integers(0, ROWS, 60)
    where = [0, 7, 31, 59]
    results = []
    for bad in ((-1, ROWS, -1, ROWS), (ROWS, -1, ROWS + 10 ** 12, -2 ** 62)):
        idx = index.copy()
        idx[where] = bad
        results.append(ppo(pol, batch, idx, **kw))
        stats, grads = _torch_ppo(pol, batch, idx, "tanh", **kw)  # the masked loss: zero terms, advantage 0, means over n
        _assert_equal_to_torch(results[-1], stats, grads, (continuous, bad))
        assert results[-1]["stats"][9] == 4
        for k in ("g_logp", "g_value"):
            assert not results[-1]["rows"][k][where].any() and results[-1]["rows"][k].any()
    a, b = results
    assert a["stats"].tobytes() == b["stats"].tobytes()  # which way an index is outside, and how far, is all the same
    for k, v in flat(a).items():
        assert v.tobytes() == flat(b)[k].tobytes(), k
    # the same rows without the bad entries' terms, summed by hand: the entries add nothing, the divisor stays n
    keep = np.delete(index, where)
    alone = ppo(pol, batch, keep, normalize_advantage=False, **kw)
    idx = index.copy()
    idx[where] = -1
    full = ppo(pol, batch, idx, normalize_advantage=False, **kw)
    for k, v in flat(alone).items():
        assert np.allclose(flat(full)[k] * 60, v * 56, rtol=1e-12, atol=1e-300), k
    assert np.allclose(full["stats"][1:7] * 60, alone["stats"][1:7] * 56, rtol=1e-12, atol=0) and alone["stats"][9] == 0


def test_float32_mode_is_float32_and_close():
    from policy_grad_model import grad_tolerances
    pol, rng, obs, action, evaluate = _case(True, seed=8, rows=300)
    batch = _batch(pol, rng, obs, action, evaluate, "tanh")
    kw = dict(clip_range_vf=0.2, ent_coef=0.01)
    m64, m32 = ppo(pol, batch, **kw), ppo(pol, batch, dtype=np.float32, **kw)
    g64, g32 = flat(m64), flat(m32)
    tol = grad_tolerances(g32, g64)
    for k in g64:
        assert g32[k].dtype == np.float32 and g64[k].dtype == np.float64
        assert 0 < np.abs(g32[k] - g64[k]).max() < tol[k] <= 0.01 * np.abs(g64[k]).max(), k
    assert m32["stats"].dtype == np.float32 and m32["rows"]["g_logp"].dtype == np.float32
    for k in range(10):
        assert abs(float(m32["stats"][k]) - m64["stats"][k]) <= 1e-4 * (1 + abs(m64["stats"][k])), STATS[k]


def _ppo_args(n=24, rows=40, discrete=False):
    import torch
    z = lambda *shape, dtype=torch.float32: _fake_cuda(torch.zeros(shape, dtype=dtype))
    batch = dict(obs=z(rows, D), action=z(rows, dtype=torch.int32) if discrete else z(rows, 2), logp=z(rows), advantage=z(rows), ret=z(rows),
                 value=z(rows))
    return batch, z(n, dtype=torch.int64), z


def test_ppo_grad_torch_checks_its_arguments_before_the_native_call():
    import torch
    env = _stub_env()
    pol, pol_nc = env.policy_torch(**_params()), env.policy_torch(**_params(critic=None))
    batch, index, z = _ppo_args()
    n = 24
    refused = [
        ("handle policy_torch returns", lambda: env.ppo_grad_torch(_params(), batch, index)),
        ("batch: expected a dict", lambda: env.ppo_grad_torch(pol, [batch["obs"]], index)),
        (r"batch\['obs'\]", lambda: env.ppo_grad_torch(pol, dict(batch, obs=z(40, 14)), index)),
        (r"batch\['obs'\]", lambda: env.ppo_grad_torch(pol, dict(batch, obs=z(0, 13)), index)),
        (r"batch\['action'\]", lambda: env.ppo_grad_torch(pol, dict(batch, action=z(39, 2)), index)),
        (r"batch\['action'\]", lambda: env.ppo_grad_torch(pol, dict(batch, action=z(40, dtype=torch.int32)), index)),
        (r"batch\['logp'\]", lambda: env.ppo_grad_torch(pol, dict(batch, logp=z(41)), index)),
        (r"batch\['advantage'\]: missing", lambda: env.ppo_grad_torch(pol, {k: v for k, v in batch.items() if k != "advantage"}, index)),
        (r"batch\['ret'\]: missing", lambda: env.ppo_grad_torch(pol, {k: v for k, v in batch.items() if k != "ret"}, index)),
        (r"batch\['value'\]: missing \(clip_range_vf", lambda: env.ppo_grad_torch(pol, dict(batch, value=None), index, clip_range_vf=0.2)),
        ("index", lambda: env.ppo_grad_torch(pol, batch, z(n, dtype=torch.int32))),
        ("index", lambda: env.ppo_grad_torch(pol, batch, z(n, 1, dtype=torch.int64))),
        ("index", lambda: env.ppo_grad_torch(pol, batch, z(0, dtype=torch.int64))),
        ("clip_range: expected", lambda: env.ppo_grad_torch(pol, batch, index, clip_range=0.0)),
        ("clip_range: expected", lambda: env.ppo_grad_torch(pol, batch, index, clip_range=float("nan"))),
        ("clip_range_vf: expected", lambda: env.ppo_grad_torch(pol, batch, index, clip_range_vf=-0.1)),
        ("ent_coef", lambda: env.ppo_grad_torch(pol, batch, index, ent_coef=-1e-3)),
        ("vf_coef", lambda: env.ppo_grad_torch(pol, batch, index, vf_coef=float("nan"))),
        ("normalize_advantage: needs n >= 2", lambda: env.ppo_grad_torch(pol, batch, z(1, dtype=torch.int64))),
        (r"stats", lambda: env.ppo_grad_torch(pol, batch, index, stats=z(11))),
        (r"rows\['g_logp'\]", lambda: env.ppo_grad_torch(pol, batch, index, rows=dict(g_logp=z(n + 1)))),
        (r"rows\['ratio'\]", lambda: env.ppo_grad_torch(pol, batch, index, rows=dict(ratio=z(n)))),
        (r"rows\['value'\]: the policy has no critic", lambda: env.ppo_grad_torch(pol_nc, batch, index, rows=dict(value=z(n)))),
    ]
    pairs = lambda p: [(z(*w.shape), z(*b.shape)) for w, b in p]
    par = _params()
    good = dict(actor=pairs(par["actor"]), critic=pairs(par["critic"]), log_std=z(2))
    refused += [
        (r"out\['actor'\]: expected 3", lambda: env.ppo_grad_torch(pol, batch, index, out={**good, "actor": good["actor"][:2]})),
        (r"out\['critic'\]: the policy has a critic", lambda: env.ppo_grad_torch(pol, batch, index, out={**good, "critic": None})),
        (r"out\['critic'\]: the policy has no critic", lambda: env.ppo_grad_torch(pol_nc, batch, index, out=good)),
        (r"out\['log_std'\]", lambda: env.ppo_grad_torch(pol, batch, index, out={**good, "log_std": None})),
    ]
    for match, call in refused:
        with pytest.raises(ValueError, match=match):
            call()
    assert [c for c in env._lib.names() if c != "sg_ppo_config_init"] == []
    env.discrete = True
    pol_d = env.policy_torch(**_params(head=6, log_std=None))
    with pytest.raises(ValueError, match="the discrete ids have none"):
        env.ppo_grad_torch(pol_d, _ppo_args(discrete=True)[0], index, out={**good, "actor": pairs(_params(head=6)["actor"])})
    assert [c for c in env._lib.names() if c != "sg_ppo_config_init"] == []


def test_the_call_passes_the_columns_and_the_configuration():
    """with the workspace query stubbed to a size, the native call receives the batch's pointers, rows and n, and the configuration"""
    import torch
    from space_gym_amd import _native
    env = _stub_env()
    pol = env.policy_torch(**_params())
    batch, index, z = _ppo_args()
    pol.workspace = _fake_cuda(torch.zeros(64, dtype=torch.uint8))
    lib = env._lib
    real = lib.__getattr__

    class Sized(type(lib)):
        def __getattr__(self, name):
            if name == "sg_ppo_grad_workspace_bytes":
                return lambda *a: 64
            return real(name)
    env._lib = Sized()
    env._lib.calls = lib.calls
    rows = dict(g_logp=z(24), value=z(24))
    grads, stats = env.ppo_grad_torch(pol, batch, index, clip_range=0.1, clip_range_vf=0.3, ent_coef=0.01, vf_coef=0.25, normalize_advantage=False,
                                      rows=rows)
    name, args = lib.calls[-1]
    assert name == "sg_ppo_grad_device" and args[4] == 40 and args[5] == 24 and args[10] == 64
    cfg, b, r = args[2]._obj, args[3]._obj, args[8]._obj
    assert isinstance(cfg, _native.SgPpoConfig) and abs(cfg.clip_range - 0.1) < 1e-7 and abs(cfg.clip_range_vf - 0.3) < 1e-7
    assert abs(cfg.ent_coef - 0.01) < 1e-8 and cfg.vf_coef == 0.25 and cfg.normalize_advantage == 0 and cfg.reserved == 0
    assert (b.obs, b.action, b.old_logp, b.advantage, b.ret, b.old_value, b.index) == tuple(
        t.data_ptr() for t in (batch["obs"], batch["action"], batch["logp"], batch["advantage"], batch["ret"], batch["value"], index))
    assert (r.logp, r.value, r.g_logp, r.g_value) == (None, rows["value"].data_ptr(), rows["g_logp"].data_ptr(), None)
    assert stats.shape == (12,) and len(grads["actor"]) == 3 and len(grads["critic"]) == 3 and grads["log_std"].shape == (2,)
    # without value clipping old_value stays NULL; without an index n = rows
    env.ppo_grad_torch(pol, batch, normalize_advantage=False)
    args = lib.calls[-1][1]
    assert args[3]._obj.old_value is None and args[3]._obj.index is None and args[4] == args[5] == 40 and args[8] is None
    # the helper hands the tensors to the parameters
    env.ppo_assign_grads(pol, grads)
    flat_grads = [t for pair in grads["actor"] + grads["critic"] for t in pair] + [grads["log_std"]]
    assert all(p.grad is g for p, g in zip(pol.tensors, flat_grads))


def test_the_multi_device_front_ends_refuse_the_calls():
    from space_gym_amd.multi_device import MultiDeviceVectorEnv
    from space_gym_amd.sharded import ShardedVectorEnv
    for cls in (MultiDeviceVectorEnv, ShardedVectorEnv):
        for name in ("ppo_grad_torch", "ppo_assign_grads"):
            with pytest.raises(NotImplementedError, match="single-device front end only"):
                getattr(cls, name)(object.__new__(cls))
