"""GPU twin of tests/test_product2d_emu.py: product-field remap (-ps) on quadrilateral lattices on the MI355X -- the three
kernels of remhos_amd/csrc/rmh_product2d.hpp against the oracle on identical inputs (orders 1, 2, 3, 6: 4, 9, 16 and 49 of a
wavefront's 64 lanes), whole runs of every IDP solver through rmhd_run_state, the shipped binary, the refusals, and one 3-D
run that must be what it was."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_product2d_emu import DT, check_kernels, check_refusals, check_run, oracle_vb_counts, product2d_case, run_kernels

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "remhos_amd", "remhos_amd_run")


@pytest.fixture(scope="module")
def lib():
    import torch

    assert torch.cuda.is_available()
    from remhos_amd.capi import load_library
    from remhos_amd.case import bind_driver

    return bind_driver(load_library())


# (n = 8: inline-quad -rs 1, n = 16: -rs 2 = 64 workgroups; n = 5: 25 elements, the last workgroup holds one)
@pytest.mark.parametrize("p,n", [(1, 8), (2, 8), (3, 8), (6, 8), (3, 16), (1, 5), (2, 5), (6, 5)])
def test_product2d_kernels_gpu(lib, p, n):
    import torch

    c = product2d_case(p, n)
    dev = torch.device("cuda:0")
    o = run_kernels(c, lib, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev), lambda t: t.cpu().numpy(), p)
    check_kernels(c, o, p, "gpu")


@pytest.mark.parametrize("p,ode,pa,fused", [(3, 11, 0, 1), (3, 12, 0, 0), (3, 13, 0, 1), (3, 13, 1, 0), (2, 12, 0, 1)])
def test_product2d_run_gpu(lib, p, ode, pa, fused):
    """inline-quad -rs 1 -p 14 -dt 0.005, 6 steps: -o 3 with -s 11, 12, 13, -s 13 with -pa, and -o 2 with -s 12; the u block
    through the fused limiter kernel (fused = 1) and through the granular sequence (fused = 0)"""
    res = check_run(lib, p, ode, pa, fused)
    assert res.fom_wall > 0


def test_product2d_refusals_gpu(lib):
    check_refusals(lib)


def _printed(out, label):
    m = re.search(rf"^{re.escape(label)}\s*([-+0-9.eE]+)\s*$", out, re.M)
    assert m, (label, out)
    return float(m.group(1))


def test_product2d_binary(lib):
    """remhos_amd_run -m data/inline-quad.mesh -p 14 ... -ps -s 12 as a child process: the three us lines, the mass of us that
    rmhd_run gives (ten printed digits), and -vb on a run whose updates the oracle keeps inside their bounds"""
    from remhos_amd.case import RmhdResult, make_config

    args = ["-m", "data/inline-quad.mesh", "-p", "14", "-rs", "1", "-o", "3", "-dt", str(DT), "-tf", "0.5", "-ms", "6", "-ho", "3",
            "-lo", "5", "-fct", "2", "-ps", "-s", "12"]
    p = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    cfg = make_config("inline-quad", 1, 3, 14, DT, 0.5, max_steps=6, ps=1, ode_solver=12)
    res = RmhdResult()
    assert lib.rmhd_run(C.byref(cfg), C.byref(res)) == 0, lib.rmhd_last_error()
    assert _printed(p.stdout, "Final mass us:") == float(f"{res.final_mass_us:.10g}")
    assert _printed(p.stdout, "Max value s:") == float(f"{res.s_max:.10g}")
    assert _printed(p.stdout, "Mass loss us:") == float(f"{res.mass_loss_us:.6g}")
    # -vb: on the pacman field the mass-based average itself leaves the overlap bounds of u (the oracle's LO update does, at
    # every order and step tried: the reference's guard aborts on its LO check there), so the guarded run is the smooth field
    # of problem 10 at a step short enough that the oracle's LO, limited and product updates of all six stages stay inside
    assert oracle_vb_counts(14, 3, 12, DT, 6)["LO u"] > 0 and oracle_vb_counts(14, 3, 12, DT, 6)["FCT us"] == 0
    assert oracle_vb_counts(10, 3, 12, 0.001, 3) == {"LO u": 0, "FCT u": 0, "FCT us": 0}
    smooth = ["-m", "data/inline-quad.mesh", "-p", "10", "-rs", "1", "-o", "3", "-dt", "0.001", "-tf", "0.5", "-ms", "3", "-ho", "3",
              "-lo", "5", "-fct", "2", "-ps", "-s", "12"]
    w = subprocess.run([EXE] + smooth, capture_output=True, text=True, timeout=600)
    assert w.returncode == 0, (w.returncode, w.stdout[-2000:], w.stderr[-2000:])
    v = subprocess.run([EXE] + smooth + ["-vb"], capture_output=True, text=True, timeout=600)
    assert v.returncode == 0, (v.returncode, v.stdout[-2000:], v.stderr[-2000:])
    for label in ("Final mass u:", "Final mass us:", "Max value s:"):
        assert _printed(v.stdout, label) == _printed(w.stdout, label)


def test_product3d_unchanged(lib):
    """cube01_hex -rs 0 -o 2 -ps -s 12, 2 steps: the final masses are the oracle's, as before"""
    from oracle.remhos_oracle import Config, Remhos
    from remhos_amd.case import RmhdResult, make_config

    out = Remhos(Config(mesh="cube01_hex", rs=0, order=2, problem=10, dt=0.02, t_final=0.5, lo=5, fct=2, ps=True, ode=12, max_steps=2)).run()
    cfg = make_config("cube01_hex", 0, 2, 10, 0.02, 0.5, max_steps=2, ps=1, ode_solver=12)
    res = RmhdResult()
    assert lib.rmhd_run(C.byref(cfg), C.byref(res)) == 0, lib.rmhd_last_error()
    assert abs(res.final_mass - out["mass"]) <= 1e-12 * abs(out["mass"])
    assert abs(res.final_mass_us - out["mass_us"]) <= 1e-12 * abs(out["mass_us"])
