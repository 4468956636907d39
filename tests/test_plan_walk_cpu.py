"""Where the merged record walk runs (IntegratorPlan::walk_on_raygen, COX_WALK in coxgraph_amd/csrc/cox_plan.hpp) for every method,
voxel size and queue budget -- no GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plan_walk_smoke(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_walk") / "plan_walk_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "plan_walk_smoke.cpp")])
    return exe


def test_walk_placement_follows_the_rule_and_the_switch(plan_walk_smoke):
    """simple / merged / fast at 10, 5, 2 and 1 cm on budgets of 1..5, 8, 16 queues and none: the walk is on the ray-generation lanes
    exactly where T, R and U share a stream beside two lanes; COX_WALK=raygen|update wins wherever merged walks records (never with
    stage graphs); no other plan field changes with the switch."""
    out = subprocess.run([plan_walk_smoke], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
