"""The integrator's plan (coxgraph_amd/csrc/cox_plan.hpp): every creation-time decision resolved by a pure function -- no GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "coxgraph_amd", "csrc")


@pytest.fixture(scope="module")
def plan_smoke(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_smoke")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "plan_smoke.cpp")])
    return exe


def test_plans_are_what_the_integrator_used_to_decide(plan_smoke):
    """Defaults of simple / merged / fast at 10, 5, 2 and 1 cm, every environment the GPU tests parametrise, malformed values."""
    out = subprocess.run([plan_smoke], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


def test_switch_table_is_the_documented_one(plan_smoke):
    """DESIGN.md section 5's table lists exactly the switches of the plan's table."""
    table = subprocess.run([plan_smoke, "--switches"], capture_output=True, text=True, check=True).stdout.split()
    assert len(table) == len(set(table)) and all(n.startswith("COX_") for n in table)
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    start = text.index("Environment switches (all read when an integrator is created")
    rows = [l for l in text[start:].split("\n\n", 2)[1].splitlines() if l.startswith("|")]
    documented = set()
    for row in rows[2:]:  # the first column of every row below the header
        documented.update(re.findall(r"`(COX_[A-Z0-9_]+)`", row.split("|")[1]))
    assert documented == set(table), (sorted(documented - set(table)), sorted(set(table) - documented))


def test_the_integrator_reads_the_environment_in_one_place():
    src = open(os.path.join(CSRC, "cox_integrator.hip")).read()
    assert len(re.findall(r"getenv", src)) == 1
    assert re.search(r"resolve_plan\([^;]*std::getenv\)", src)
    for header in ("cox_frame.hpp", "cox_raygen.hpp", "cox_walk.hpp", "cox_frontend.hpp", "cox_threads.hpp", "cox_plan.hpp"):
        assert "getenv" not in open(os.path.join(CSRC, header)).read(), header
