"""NeumannHOSolver (-ho 1) on the MI355X: the kernels of remhos_amd/csrc/rmh_neumann.hpp against the restatement of
tests/neumann_oracle.py on the cases and with the checks of tests/test_neumann_emu.py, the reference's four `-ho 1 -lo 2 -fct 2`
known answers (autotest/out_baseline.dat:5-7, 10-12, 25-27, 30-32; tests/golden/reference_kat_pdu.json) through rmhd_run, one
3-D run beside -lo 5 and beside -fct 4, and the shipped executable."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import layout_from_oracle
from tests.test_neumann_emu import CASES, IDS, check_case_condition, check_ho1, driver_vs_oracle, oracle_ho1

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "remhos_amd", "remhos_amd_run")
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kat_pdu.json")))["autotest"]


@pytest.fixture(scope="module")
def lib():
    import torch

    from remhos_amd.capi import load_library
    from remhos_amd.case import bind_driver

    assert torch.cuda.is_available()
    return bind_driver(load_library())


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()  # (a copy: the shared oracle arrays are read-only)


def _context(lib, r, p, t):
    import torch

    from remhos_amd.capi import Context

    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=p, exec_mode=r.exec_mode, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.setup(t)
    return ctx


@pytest.mark.parametrize("mesh,rs,p,prob,t,pert,stop", CASES, ids=IDS)
def test_ho_neumann_gpu(lib, mesh, rs, p, prob, t, pert, stop):
    import torch

    r, uh, keep = oracle_ho1(mesh, rs, p, prob, t, pert)
    check_case_condition(keep, stop)
    ctx = _context(lib, r, p, t)
    u = _dev(uh)
    du, du2, du3 = (torch.full_like(u, float("nan")) for _ in range(3))
    ctx.ho_neumann(u, du)
    updates, norms = ctx.last_neumann()
    ctx.ho_neumann(u, du2)
    assert ctx.last_neumann()[0] == updates
    ctx.ho_apply(u, du3)
    torch.cuda.synchronize()
    ctx.close()
    check_ho1(keep, du.cpu().numpy(), du2.cpu().numpy(), updates, norms, du3.cpu().numpy(), "MI355X")


def test_ho_neumann_follows_the_moved_mesh_gpu(lib):
    import torch

    r, uh, keep = oracle_ho1("cube01_hex", 0, 3, 10, 0.3)
    ctx = _context(lib, r, 3, 0.0)
    u = _dev(uh)
    du = torch.zeros_like(u)
    ctx.ho_neumann(u, du)
    torch.cuda.synchronize()
    ctx.close()
    assert _rel(du.cpu().numpy(), keep["du"]) > 1e-6


@pytest.mark.parametrize("mesh,p,prob", [("cube01_hex", 2, 10), ("inline-quad", 3, 14)])
def test_ho_neumann_zero_input_gpu(lib, mesh, p, prob):
    import torch

    r, uh, keep = oracle_ho1(mesh, 0 if mesh == "cube01_hex" else 1, p, prob, 0.3)
    ctx = _context(lib, r, p, 0.3)
    u = torch.zeros_like(_dev(uh))
    du = torch.full_like(u, float("nan"))
    ctx.ho_neumann(u, du)
    updates, norms = ctx.last_neumann()
    ctx.close()
    assert bool((du == 0.0).all()) and updates == 0 and norms[0] == 0.0 and np.isnan(norms[1:]).all()


@pytest.mark.parametrize("e", KAT, ids=[e["name"] for e in KAT])
def test_reference_known_answers_ho1_lo2_fct2(lib, e):
    """the reference's first regression method through rmhd_run: its printed digits"""
    from remhos_amd.case import RmhdResult, make_config

    assert e["ho"] == 1 and e["lo"] == 2 and e["fct"] == 2
    cfg = make_config(e["mesh"], e["rs"], e["order"], e["problem"], e["dt"], e["t_final"], lo_type=2, fused=0, fct_type=2, ho_type=1)
    res = RmhdResult()
    assert lib.rmhd_run(C.byref(cfg), C.byref(res)) == 0, lib.rmhd_last_error()
    print(e["name"], "mass", res.final_mass, "max", res.max_value, "steps", res.steps)
    assert f"{res.final_mass:.10g}" == f"{e['mass']:.10g}"
    assert f"{res.max_value:.10g}" == f"{e['max']:.10g}"


@pytest.mark.parametrize("lo,fct", [(5, 2), (2, 4)])
def test_ho1_beside_other_solvers_3d(lib, lo, fct):
    """cube01_hex -rs 1 -o 2 -p 10 -dt 0.02 -tf 0.7, three steps of -ho 1 beside -lo 5 and beside -fct 4, against the restatement"""
    driver_vs_oracle(lib, "cube01_hex", 1, 2, 10, 0.02, 0.7, 3, lo, fct)


def _printed(out, label):
    m = re.search(rf"^{re.escape(label)}\s*([-+0-9.eE]+)\s*$", out, re.M)
    assert m, (label, out)
    return float(m.group(1))


def test_binary_ho1(lib):
    """remhos_amd_run -ho 1 -lo 2 -fct 2 -vb as a child process: rc 0, the printed mass is rmhd_run's"""
    from remhos_amd.case import RmhdResult, make_config

    args = ["-m", "data/cube01_hex.mesh", "-p", "10", "-rs", "1", "-o", "2", "-dt", "0.02", "-tf", "0.7", "-ms", "3", "-ho", "1",
            "-lo", "2", "-fct", "2"]
    p = subprocess.run([EXE] + args + ["-vb"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    cfg = make_config("cube01_hex", 1, 2, 10, 0.02, 0.7, max_steps=3, lo_type=2, fused=0, fct_type=2, ho_type=1)
    res = RmhdResult()
    assert lib.rmhd_run(C.byref(cfg), C.byref(res)) == 0, lib.rmhd_last_error()
    assert _printed(p.stdout, "Final mass u:") == float(f"{res.final_mass:.10g}")
    q = subprocess.run([EXE] + args + ["-pa"], capture_output=True, text=True, timeout=60)
    assert q.returncode == 2 and "-ho 1" in q.stderr and "-pa" in q.stderr
    # the front end never leaves its one-kernel default silently: -lo 5 needs -unfused beside -ho 1
    lo5 = args[:-4] + ["-lo", "5", "-fct", "2"]
    q = subprocess.run([EXE] + lo5, capture_output=True, text=True, timeout=60)
    assert q.returncode == 1 and "-ho 1" in q.stderr and "-unfused" in q.stderr
    q = subprocess.run([EXE] + lo5 + ["-unfused"], capture_output=True, text=True, timeout=600)
    assert q.returncode == 0, (q.returncode, q.stdout[-2000:], q.stderr[-2000:])
