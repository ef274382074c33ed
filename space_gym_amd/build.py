"""Builds libspacegym_hip.so (HIP kernels for gfx950 + the C ABI of include/spacegym.h) in-tree with hipcc."""
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIB_DIR, "libspacegym_hip.so")
SOURCES = ["sg_engine.hip"]
HEADERS = ["sg_device.hpp", "sg_host_config.hpp", "sg_config.h", "sg_goal_pair_rollout.inc", "sg_kepler_pair_rollout.inc", "sg_gae.inc", "sg_returns.inc", "sg_retrace.inc", "sg_replay.inc", "sg_sequence.inc", "sg_her.inc", "sg_priority.inc", "sg_policy.inc", "sg_policy_grad.inc", "sg_qnet.inc", "sg_squashed.inc", "sg_q_td.inc", "sg_q_actor.inc", "sg_dqn.inc", "sg_dqn_td.inc", "sg_population.inc", "sg_ppo.inc", "sg_adam.inc", "sg_pbt.inc", "sg_minibatch.inc", os.path.join(ROOT, "include", "spacegym.h")]
ARCH = "gfx950"


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the engine is HIP-only and cannot be built without ROCm")
    return exe


def flags(extra=()):
    # -ffp-contract=on: a*b+c fuses per source expression, identically in every kernel that inlines the same device
    # function (the default, fast, fuses across statements depending on context, so the per-step kernel and the fused
    # rollout kernel would round differently)
    return ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-shared", "-fno-gpu-rdc", "-ffp-contract=on",
            "-I", os.path.join(ROOT, "include"), "-I", CSRC, *extra]


def is_stale(target=LIB):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    deps = [os.path.join(CSRC, f) for f in SOURCES] + [f if os.path.isabs(f) else os.path.join(CSRC, f) for f in HEADERS]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False, extra=(), out=None):
    """out=None builds the product library; a different `out` (with e.g. extra=("-DSG_STAMPS",)) a diagnostic one."""
    if out is None and not force and not is_stale():
        return LIB
    os.makedirs(LIB_DIR, exist_ok=True)
    out = out or LIB
    cmd = [hipcc(), *flags(extra), "-o", out, *[os.path.join(CSRC, f) for f in SOURCES]]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return out


def device_asm(force=False):
    """One device-only compile for the tests and tools that inspect the code: (assembly, the compiler's resource remarks), kept
    until a source is newer.  Both are written under temporary names and renamed at the end: a file that is there is whole."""
    out = [os.path.join(LIB_DIR, "sg_engine.s"), os.path.join(LIB_DIR, "sg_engine.remarks.txt")]
    if not force and not any(is_stale(f) for f in out):
        return tuple(out)
    os.makedirs(LIB_DIR, exist_ok=True)
    tmp = ["%s.%d.tmp" % (f, os.getpid()) for f in out]
    cmd = [hipcc(), *[f for f in flags() if f not in ("-shared", "-fPIC")], "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-o", tmp[0], *[os.path.join(CSRC, f) for f in SOURCES]]
    try:
        with open(tmp[1], "w") as err:
            failed = subprocess.call(cmd, stderr=err)
        if failed:
            raise RuntimeError("device-only compile failed:\n" + open(tmp[1]).read()[-4000:])
        for t, f in zip(tmp, out):
            os.replace(t, f)
    finally:
        for t in filter(os.path.exists, tmp):
            os.remove(t)
    return tuple(out)


def resource_report(remarks_path=None):
    """One dict per kernel of the compiler's resource remarks: `name` (mangled) and the remark keys ("VGPRs", ...) as strings."""
    rows, cur = [], None
    for line in open(remarks_path or device_asm()[1]):
        m = re.search(r"remark: \s*(.+?)\s*\[-Rpass-analysis", line)
        if not m:
            continue
        k, _, v = m.group(1).partition(":")
        if k.strip() == "Function Name":
            cur = {"name": v.strip()}
            rows.append(cur)
        elif cur is not None:
            cur[k.strip()] = v.strip()
    return rows


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True,
                extra=("-Rpass-analysis=kernel-resource-usage",) if "--usage" in sys.argv else ()))
