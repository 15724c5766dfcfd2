"""What GridIndex::build() decides before it launches anything (csrc/grid_plan.h: plan_build, commit_build) is a pure host function:
host/index_plan_check.cpp holds it to cases worked out by hand from the measured rules and to invariants over a sweep of sizes, capacities
and hints (bins and LDS within their bounds, a layout only with a reused header, only variants that are built).  No GPU: the program is built by
g++ alone, which is also what keeps the header free of the device toolchain."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "simpleslam_amd", "lib", "index_plan_check")


def test_index_plan_check_program():
    assert os.path.exists(EXE), "index_plan_check not built (run __graft_entry__.build())"
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert out.stdout.strip() == "index_plan_check ok"

