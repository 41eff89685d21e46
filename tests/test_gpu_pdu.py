"""Preconditioned DiscreteUpwind (-lo 2) on the MI355X: lo_upwind_prec_kernel (remhos_amd/csrc/rmh_pdu.hpp) against the
restatement of tests/pdu_oracle.py on identical inputs (the per-case bound of tests/test_pdu_emu.py, conservation, run-to-run bit
identity), one whole run beside each limiter through rmhd_run_state, and the shipped executable.  CPU twins:
tests/test_pdu_emu.py, tests/test_pdu_oracle.py (the reference's four `-ho 1 -lo 2 -fct 2` known answers)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import layout_from_oracle
from tests.pdu_oracle import Config, PduRemhos
from tests.test_pdu_emu import check_lo2, oracle_lo2, stage_tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "remhos_amd", "remhos_amd_run")

# the cases of tests/test_pdu_emu.py, 3-D on -rs 1 (64 workgroups)
CASES = [("cube01_hex", 1, 1, 10, 0.3), ("cube01_hex", 1, 2, 10, 0.3), ("cube01_hex", 1, 3, 10, 0.3), ("periodic-cube", 1, 3, 0, 0.0),
         ("inline-quad", 1, 1, 14, 0.3), ("inline-quad", 1, 3, 14, 0.3), ("inline-quad", 1, 6, 14, 0.3),
         ("periodic-square", 1, 3, 5, 0.0)]


@pytest.fixture(scope="module")
def lib():
    import torch

    from remhos_amd.capi import load_library
    from remhos_amd.case import bind_driver

    assert torch.cuda.is_available()
    return bind_driver(load_library())


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("mesh,rs,p,prob,t", CASES)
def test_lo_upwind_prec_gpu(lib, mesh, rs, p, prob, t):
    import torch

    from remhos_amd.capi import Context

    r, cfg, uh, keep = oracle_lo2(mesh, rs, p, prob, t)
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=p, exec_mode=r.exec_mode, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.setup(t)
    u = torch.from_numpy(np.ascontiguousarray(uh, dtype=np.float64)).cuda()
    lo, lo2 = torch.full_like(u, float("nan")), torch.full_like(u, float("nan"))
    ctx.lo_upwind_prec(u, lo)
    ctx.lo_upwind_prec(u, lo2)
    torch.cuda.synchronize()
    ctx.close()
    check_lo2(r, uh, keep, lo.cpu().numpy(), lo2.cpu().numpy(), "MI355X")


@pytest.mark.parametrize("fct", [1, 2, 4])
def test_lo2_beside_each_limiter_3d(lib, fct):
    """cube01_hex -rs 1 -o 2 -p 10 -dt 0.02 -tf 0.7, three steps, -lo 2 beside every limiter, against the restatement"""
    from remhos_amd.case import RmhdResult, make_config

    mesh, rs, p, prob, dt, tf, ms = "cube01_hex", 1, 2, 10, 0.02, 0.7, 3
    r = PduRemhos(Config(mesh=mesh, rs=rs, order=p, problem=prob, dt=dt, t_final=tf, lo=2, fct=fct, max_steps=ms))
    out = r.run()
    tol = 10.0 * stage_tol(r)
    cfg = make_config(mesh, rs, p, prob, dt, tf, max_steps=ms, lo_type=2, fused=0, fct_type=fct)
    res = RmhdResult()
    uf = np.zeros_like(r.u)
    assert lib.rmhd_run_state(C.byref(cfg), C.byref(res), uf.ctypes.data, None) == 0, lib.rmhd_last_error()
    print("mass", res.final_mass, out["mass"], "field", _rel(uf, r.u), "bound", tol)
    assert res.steps == out["steps"] == ms
    assert abs(res.final_mass - out["mass"]) <= 1e-12 * abs(out["mass"])
    assert _rel(uf, r.u) <= tol


def _printed(out, label):
    m = re.search(rf"^{re.escape(label)}\s*([-+0-9.eE]+)\s*$", out, re.M)
    assert m, (label, out)
    return float(m.group(1))


def test_binary_lo2(lib):
    """remhos_amd_run -ho 3 -lo 2 -fct 2 -vb as a child process: rc 0, the printed mass is rmhd_run's"""
    from remhos_amd.case import RmhdResult, make_config

    args = ["-m", "data/cube01_hex.mesh", "-p", "10", "-rs", "1", "-o", "2", "-dt", "0.02", "-tf", "0.7", "-ms", "3", "-ho", "3",
            "-lo", "2", "-fct", "2"]
    p = subprocess.run([EXE] + args + ["-vb"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    cfg = make_config("cube01_hex", 1, 2, 10, 0.02, 0.7, max_steps=3, lo_type=2, fused=0, fct_type=2)
    res = RmhdResult()
    assert lib.rmhd_run(C.byref(cfg), C.byref(res)) == 0, lib.rmhd_last_error()
    assert _printed(p.stdout, "Final mass u:") == float(f"{res.final_mass:.10g}")
