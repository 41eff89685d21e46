"""DiscreteUpwind (-lo 1) and FluxBasedFCT (-fct 1) on the MI355X: lo_upwind_kernel and fct_fluxbased_kernel
(remhos_amd/csrc/rmh_upwind.hpp) against the restatement of tests/upwind_oracle.py on identical inputs, the reference's four
`-ho 3 -lo 1 -fct 1` known answers (autotest/out_baseline.dat:150-180) through rmhd_run, one mixed combination per new solver,
and the shipped executable.  CPU twins: tests/test_upwind_emu.py, tests/test_upwind_oracle.py."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import layout_from_oracle
from tests.test_upwind_emu import check_fct_properties, check_lo_conservation, oracle_stage
from tests.upwind_oracle import Config, UpwindRemhos

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "remhos_amd", "remhos_amd_run")
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kat_upwind.json")))["autotest"]

# 3-D at p = 1 ... 6 (rs 1 at p <= 3: 64 workgroups), remap at t != 0 and transport; 2-D at several orders
CASES = [
    ("cube01_hex", 1, 1, 10, 0.3), ("cube01_hex", 1, 2, 10, 0.3), ("cube01_hex", 1, 3, 10, 0.3), ("cube01_hex", 0, 4, 10, 0.3),
    ("cube01_hex", 0, 5, 10, 0.3), ("cube01_hex", 0, 6, 10, 0.3), ("periodic-cube", 0, 3, 0, 0.0),
    ("inline-quad", 1, 3, 14, 0.3), ("periodic-square", 1, 3, 5, 0.0), ("inline-quad", 1, 1, 14, 0.3), ("inline-quad", 1, 2, 14, 0.3),
    ("inline-quad", 1, 6, 14, 0.3),
]


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

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


@pytest.mark.parametrize("mesh,rs,p,prob,t", CASES)
def test_upwind_kernels_gpu(lib, mesh, rs, p, prob, t):
    import torch

    from remhos_amd.capi import Context

    r, cfg, uh, keep = oracle_stage(mesh, rs, p, prob, t)
    cs = r.clip_scale(uh, keep["m"], keep["du_ho"], keep["du_lo"], keep["umin"], keep["umax"], cfg.dt)
    assert _rel(cs, keep["du"]) > 1e-4  # (the inputs tell the two limiters apart)
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=p, exec_mode=r.exec_mode, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.setup(t)
    u, m, dh, dl, umin, umax = (_dev(keep[k] if k != "u" else uh) for k in ("u", "m", "du_ho", "du_lo", "umin", "umax"))
    lo, lo2, du, du2 = (torch.full_like(u, float("nan")) for _ in range(4))
    ctx.lo_upwind(u, lo)
    ctx.lo_upwind(u, lo2)
    ctx.fct_fluxbased(u, m, dh, dl, umin, umax, cfg.dt, du)
    ctx.fct_fluxbased(u, m, dh, dl, umin, umax, cfg.dt, du2)
    torch.cuda.synchronize()
    ctx.close()
    glo, gdu = lo.cpu().numpy(), du.cpu().numpy()
    e_lo, e_du = _rel(glo, keep["du_lo"]), _rel(gdu, keep["du"])
    print("max|du_lo - oracle| / max|oracle| =", e_lo, "  max|du - oracle| / max|oracle| =", e_du)
    assert e_lo <= 1e-12 and e_du <= 1e-12
    check_lo_conservation(keep["m"], glo, keep)
    check_fct_properties(uh, keep["m"], gdu, keep, cfg.dt)
    assert np.array_equal(glo, lo2.cpu().numpy()) and np.array_equal(gdu, du2.cpu().numpy())


@pytest.mark.parametrize("e", KAT, ids=[e["name"] for e in KAT])
def test_reference_known_answers_lo1_fct1(lib, e):
    """autotest/out_baseline.dat:150-180 through rmhd_run: the reference's printed digits"""
    from remhos_amd.case import RmhdResult, make_config

    cfg = make_config(e["mesh"], e["rs"], e["order"], e["problem"], e["dt"], e["t_final"], lo_type=1, fused=0, fct_type=1)
    res = RmhdResult()
    assert lib.rmhd_run(C.byref(cfg), C.byref(res)) == 0, lib.rmhd_last_error()
    print(e["name"], "mass", res.final_mass, "max", res.max_value, "steps", res.steps)
    assert f"{res.final_mass:.10g}" == f"{e['mass']:.10g}"
    assert f"{res.max_value:.10g}" == f"{e['max']:.10g}"


@pytest.mark.parametrize("lo,fct", [(1, 2), (4, 1)])
def test_mixed_combinations_3d(lib, lo, fct):
    """cube01_hex -rs 1 -o 2 -p 10 -dt 0.02 -tf 0.7, three steps: each new solver beside an existing one, against the restatement"""
    from remhos_amd.case import RmhdResult, make_config

    mesh, rs, p, prob, dt, tf, ms = "cube01_hex", 1, 2, 10, 0.02, 0.7, 3
    r = UpwindRemhos(Config(mesh=mesh, rs=rs, order=p, problem=prob, dt=dt, t_final=tf, lo=lo, fct=fct, max_steps=ms))
    out = r.run()
    cfg = make_config(mesh, rs, p, prob, dt, tf, max_steps=ms, lo_type=lo, fused=0, fct_type=fct)
    res = RmhdResult()
    uf = np.zeros_like(r.u)
    assert lib.rmhd_run_state(C.byref(cfg), C.byref(res), uf.ctypes.data, None) == 0, lib.rmhd_last_error()
    print("mass", res.final_mass, out["mass"], "field", _rel(uf, r.u))
    assert res.steps == out["steps"] == ms
    assert abs(res.final_mass - out["mass"]) <= 1e-12 * abs(out["mass"])
    assert _rel(uf, r.u) < 1e-11


def _printed(out, label):
    m = re.search(rf"^{re.escape(label)}\s*([-+0-9.eE]+)\s*$", out, re.M)
    assert m, (label, out)
    return float(m.group(1))


def test_binary_lo1_fct1(lib):
    """remhos_amd_run -lo 1 -fct 1 -vb as a child process: rc 0, the printed mass is rmhd_run's; -ho 1 is still refused"""
    from remhos_amd.case import RmhdResult, make_config

    args = ["-m", "data/cube01_hex.mesh", "-p", "10", "-rs", "1", "-o", "2", "-dt", "0.02", "-tf", "0.7", "-ms", "3", "-ho", "3",
            "-lo", "1", "-fct", "1"]
    p = subprocess.run([EXE] + args + ["-vb"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    cfg = make_config("cube01_hex", 1, 2, 10, 0.02, 0.7, max_steps=3, lo_type=1, fused=0, fct_type=1)
    res = RmhdResult()
    assert lib.rmhd_run(C.byref(cfg), C.byref(res)) == 0, lib.rmhd_last_error()
    assert _printed(p.stdout, "Final mass u:") == float(f"{res.final_mass:.10g}")
    q = subprocess.run([EXE] + args[:-6] + ["-ho", "1", "-lo", "1", "-fct", "1"], capture_output=True, text=True, timeout=60)
    assert q.returncode == 1 and "implements" in q.stderr
