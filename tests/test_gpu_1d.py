"""dim = 1 on the device: the checks of tests/test_1d_emu.py through librmh.so (one lane per element, remhos_amd/csrc/rmh_1d.hpp),
the reference's three 1-D regression runs in full (autotest/out_baseline.dat 'Transport per-1D': 1000 steps on 32 segments, the
printed ten digits) through rmhd_run, and the shipped binary on the reference's command line."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

from tests import test_1d_emu as t1

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "remhos_amd", "remhos_amd_run")
KAT1 = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kat_1d.json")))


@pytest.fixture(scope="module")
def dev():
    yield t1.Backend(True)
    t1.report()


def sig10(x):
    return float(f"{x:.10g}")


# ---- one stage, every entry point; conditions; order rules; refusals -------------------------------------------------------
@pytest.mark.parametrize("p,lo,mv", t1.STAGE_CASES, ids=[f"p{p}-lo{lo}-{'moving' if mv else 'fixed'}" for p, lo, mv in t1.STAGE_CASES])
def test_stage_parity(dev, p, lo, mv):
    for lattice in t1.LATTICES:
        t1.check_stage(dev, p, lo, mv, t1.PER3_P1 if (p == 1 and lattice[0] == "per3") else lattice)


def test_rd_order_conditions(dev):
    t1.check_rd_order_conditions(dev)


def test_refused_entries(dev):
    t1.check_refused_entries(dev)


def test_refused_options(dev):
    t1.check_refused_options(dev)


def test_pa_is_ignored(dev, capfd):
    t1.check_pa_is_ignored(dev, capfd)


@pytest.mark.parametrize("kw", t1.RUNS, ids=t1.RUN_IDS)
def test_runs_against_oracle(dev, kw):
    t1.check_run(dev, kw)


# ---- the reference's own answers -----------------------------------------------------------------------------------------
def run_kat(dev, case, fused):
    from remhos_amd.case import RmhdResult, make_config

    c = KAT1["common"]
    cfg = make_config(mesh=c["mesh"], rs=c["rs"], order=c["order"], problem=c["problem"], dt=c["dt"], t_final=c["t_final"],
                      lo_type=case["lo"], ho_type=case["ho"], pa=case["pa"], fct_type=c["fct"], fused=fused)
    res = RmhdResult()
    assert dev.lib.rmhd_run(C.byref(cfg), C.byref(res)) == 0, dev.lib.rmhd_last_error().decode()
    assert res.steps == 1000 and res.global_dofs == 32 * (c["order"] + 1)
    return res


@pytest.mark.parametrize("case", KAT1["cases"], ids=[c["name"] for c in KAT1["cases"]])
def test_reference_answers(dev, case):
    """autotest/out_baseline.dat:52-54, 89-91, 126-128 through rmhd_run, one kernel per stage"""
    res = run_kat(dev, case, 1)
    assert sig10(res.final_mass) == case["final_mass"]
    assert sig10(res.max_value) == case["max_value"]


def test_reference_answer_granular(dev):
    """the lo 4 run once more through the solver classes (fused = 0)"""
    case = KAT1["cases"][0]
    res = run_kat(dev, case, 0)
    assert sig10(res.final_mass) == case["final_mass"]
    assert sig10(res.max_value) == case["max_value"]


# ---- the binary ------------------------------------------------------------------------------------------------------------
def run_binary(args):
    assert os.path.exists(EXE), "remhos_amd/remhos_amd_run is not built (python -c 'import __graft_entry__ as g; g.build()')"
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def printed(out, label):
    m = re.search(rf"^{re.escape(label)}\s*([-+0-9.eE]+)\s*$", out, re.M)
    assert m, (label, out)
    return float(m.group(1))


def test_binary_reference_command_line(dev):
    """autotest/test.sh's 1-D line through the shipped binary: the printed digits are rmhd_run's and the reference's; -vb runs clean
    with the same values; -ps is refused naming dim = 1"""
    case = KAT1["cases"][0]
    args = ["-m", "data/periodic-segment.mesh", "-p", 0, "-rs", 3, "-o", 3, "-dt", 0.001, "-tf", 1, "-ho", 3, "-lo", 4, "-fct", 2]
    res = run_kat(dev, case, 1)
    for extra in ([], ["-vb"]):
        p = run_binary(args + extra)
        assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        assert printed(p.stdout, "Final mass u:") == sig10(res.final_mass) == case["final_mass"]
        assert printed(p.stdout, "Max value u:") == sig10(res.max_value) == case["max_value"]
        assert int(re.search(r"Number of unknowns: (\d+)", p.stdout).group(1)) == 128
    p = run_binary(args + ["-ps", "-s", 13])
    assert p.returncode != 0 and "dim = 1" in p.stderr, (p.returncode, p.stderr)
