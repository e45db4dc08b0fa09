"""CPU: what plan_fwd plans is what the forward kernels walk.  tests/fwd_sched_check.cpp calls the
real plan_fwd (fmha_launch.h) over a grid of (b x kv heads, row blocks, slots, fwd_order, item
counter, fwd_xcdq, FwdQueue) and walks every workgroup of the planned grid with the pure schedule
functions fwd_walk is built from (fmha_fwd_sched.h): every (unit, row block) exactly once, nothing
out of range, pairs on steps 2j / 2j + 1 of one workgroup, the queues' orders, workgroup w on
queue w % 8.  Odd unit and row-block counts included, which the GPU tests' even shapes miss."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_planned_grids_walk_every_item_once(tmp_path):
    exe = tmp_path / "fwd_sched_check"
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17",
                    "-I", os.path.join(ROOT, "xf_flash_attention_cutlass_amd", "csrc"),
                    os.path.join(ROOT, "tests", "fwd_sched_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert r.stdout.strip().endswith("2880 cases, 0 failures"), r.stdout[-500:]
