"""The queue budget of the integrator's plan (coxgraph_amd/csrc/cox_plan.hpp): which streams an integrator gets when the process has
1, 2, 3, 4, 5, 8 or 16 hardware queues, or when nobody says -- no GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "coxgraph_amd", "csrc")


@pytest.fixture(scope="module")
def plan_queues_smoke(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_queues") / "plan_queues_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "plan_queues_smoke.cpp")])
    return exe


def test_plans_fit_the_queue_budget(plan_queues_smoke):
    """simple / merged / fast at 10, 5, 2 and 1 cm: no budget and 16 queues give today's plans, a tight budget never more streams
    than it has queues beside the null stream's, explicit switches win, COX_QUEUES is the argument, malformed values are ignored."""
    out = subprocess.run([plan_queues_smoke], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_the_engine_takes_the_budget_from_one_helper():
    """The integrator hands resolve_plan the environment and the queue count of cox_internal_hw_queues(); the runtime's variable is
    read in cox_layer.hip only, beside cox_runtime_prepare(), and the plan stays a pure function (no getenv in cox_plan.hpp)."""
    integ = open(os.path.join(CSRC, "cox_integrator.hip")).read()
    assert re.search(r"resolve_plan\([^;]*cox_internal_hw_queues\(\)|hw_queues = cox_internal_hw_queues\(\);[^;]*resolve_plan\([^;]*hw_queues\)", integ)
    assert "GPU_MAX_HW_QUEUES" not in integ
    assert "getenv" not in open(os.path.join(CSRC, "cox_plan.hpp")).read()
    layer = open(os.path.join(CSRC, "cox_layer.hip")).read()
    assert re.search(r"int cox_internal_hw_queues\(\)\s*\{[^}]*GPU_MAX_HW_QUEUES", layer)
    assert "int cox_internal_hw_queues();" in open(os.path.join(CSRC, "cox_internal.hpp")).read()
    for name in os.listdir(CSRC):  # nothing in the engine sets the variable but cox_runtime_prepare()
        src = open(os.path.join(CSRC, name)).read()
        assert len(re.findall(r"setenv\(\"GPU_MAX_HW_QUEUES\"", src)) == (1 if name == "cox_layer.hip" else 0), name
