"""The argument heads of the struct-argument kernels arrive in preloaded SGPRs (no GPU): tools/kernarg_preload_report.py on conv_cb.hip.

The compiler preloads leading scalar / pointer kernel parameters only and stops at a by-value struct, so a kernel whose first parameter is
its argument block gets nothing (syncfusion_amd/csrc/Makefile).  conv_cb.hip is the cheapest of the hot sources to
compile (about a minute); profiles/kernarg_preload.txt records the other families.
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "kernarg_preload_report.py")
BUDGET = 14   # 16 user SGPRs less the two of the kernarg segment pointer


def _hipcc():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernarg_preload_report as rep
    finally:
        sys.path.pop(0)
    hipcc, _ = rep.makefile_vars()
    return hipcc if (os.path.exists(hipcc) or shutil.which(hipcc)) else None


@pytest.fixture(scope="module")
def conv_cb_rows():
    if _hipcc() is None:
        pytest.skip("hipcc is not installed: nothing to compile the kernels with")
    r = subprocess.run([sys.executable, TOOL, "conv_cb.hip"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = []
    for line in r.stdout.splitlines():
        f = line.split("\t")
        assert len(f) == 4, line
        rows.append((f[3], int(f[1]), int(f[2])))
    return rows


def test_every_conv_cb_instantiation_has_a_preloaded_head(conv_cb_rows):
    inst = [r for r in conv_cb_rows if "conv_cb_kernel<" in r[0]]
    assert len(inst) >= 16, [r[0] for r in conv_cb_rows]   # bf16 and fp16: MT 1-4 x prologue x KB forms and the direct epilogues
    for name, user, pre in inst:
        print(f"{user:3d} {pre:3d} {name}")
        assert pre > 0, f"no kernel argument is preloaded: {name}"
        assert user == pre + 2, f"user SGPRs {user} != kernarg pointer + {pre} preloaded dwords: {name}"


def test_no_kernel_reports_more_than_the_budget(conv_cb_rows):
    assert conv_cb_rows
    for name, user, pre in conv_cb_rows:
        assert 0 <= pre <= BUDGET, f"{pre} preloaded dwords: {name}"
