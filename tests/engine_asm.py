"""The engine's device assembly and resource report for the tests that inspect them (no GPU needed): build.device_asm() compiles
them once and keeps them beside the library; here they are read and searched once per session."""
import functools
import os
import re
import shutil

import pytest


@functools.lru_cache(maxsize=None)
def _artefacts():
    from space_gym_amd import build
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    return build.device_asm()


@functools.lru_cache(maxsize=None)
def text():
    return open(_artefacts()[0]).read()


def resource_rows():
    """the compiler's resource remarks: one dict per kernel, `name` and the remark keys"""
    from space_gym_amd import build
    return build.resource_report(_artefacts()[1])


def descriptors(pattern):
    """[(mangled name, {field: int})] of the kernel descriptors whose name matches `pattern` (no capturing group in it)"""
    found = re.findall(r"\.amdhsa_kernel (" + pattern + r")\n(.*?)\.end_amdhsa_kernel", text(), flags=re.S)
    return [(name, {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)", body)}) for name, body in found]


def spill_counts(pattern, kind="vgpr"):
    """[(mangled name, spilled registers)] from the code object's metadata, for the kernels whose name matches `pattern`"""
    found = re.findall(r"\.name:\s+(" + pattern + r")(?:(?!\.name:).)*?\." + kind + r"_spill_count:\s+(\d+)", text(), flags=re.S)
    return [(name, int(n)) for name, n in found]


def function(name):
    """the assembly of one function, from its label to its .Lfunc_end"""
    st = text().index("\n" + name + ":")
    return text()[st:text().index(".Lfunc_end", st)]


def instructions(fn_text):
    """the instructions of a function's text: no comments, labels or directives"""
    ins = [l.split(";")[0].strip() for l in fn_text.splitlines()]
    return [l for l in ins if l and not l.startswith(".") and not l.endswith(":")]


def assert_no_memory_wait_behind_dma(label_regex, n_kernels, min_dma):
    """In each of the `n_kernels` functions whose label line matches: at least `min_dma` global_load_lds, behind the last of them
    300 instructions without an `s_waitcnt vmcnt`, and none between the loads of its group (those within 120 instructions)."""
    labels = [m.group(0)[:-1] for m in re.finditer(label_regex, text(), flags=re.M)]
    assert len(labels) == n_kernels, (len(labels), n_kernels, labels)  # (written out: pytest rewrites asserts in test files only)
    for label in labels:
        ins = instructions(function(label))
        dma = [k for k, l in enumerate(ins) if l.startswith("global_load_lds")]
        assert len(dma) >= min_dma, (label, len(dma), min_dma)
        last = dma[-1]
        nxt = next((k for k in range(last + 1, len(ins)) if ins[k].startswith("s_waitcnt") and "vmcnt" in ins[k]), len(ins))
        assert nxt - last >= 300, (label, nxt - last)
        first = next(k for k in dma if last - k < 120)
        assert not any(l.startswith("s_waitcnt") and "vmcnt" in l for l in ins[first:last]), label


def function_body(src, signature):
    """the C++ source of one function, from `signature` to its closing brace"""
    start = src.index(signature)
    depth, k = 0, src.index("{", start)
    for k in range(k, len(src)):
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        if depth == 0:
            return src[start:k + 1]
    raise AssertionError(signature)
