"""Who walks a ray of the merged record walk (IntegratorPlan::touch_in_merge, COX_TOUCH in coxgraph_amd/csrc/cox_plan.hpp) for every
method, voxel size and queue budget -- no GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_touch_smoke(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_touch") / "plan_touch_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "plan_touch_smoke.cpp")])
    return exe


def test_touch_in_merge_follows_the_rule_and_the_switch(plan_touch_smoke):
    """simple / merged / fast at 10, 5, 2 and 1 cm on budgets of 1..5, 8, 16 queues and none: the bundle merge walks the rays exactly
    where the walk is on the ray-generation lanes with the small axis cap; COX_TOUCH=merge|kernel wins there and changes nothing
    elsewhere; no other plan field changes with the switch."""
    out = subprocess.run([plan_touch_smoke], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
