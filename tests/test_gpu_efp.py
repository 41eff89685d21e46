"""ElementFCTProjection (-fct 4) on the MI355X: fct_projection_kernel (remhos_amd/csrc/rmh_efp.hpp) against the oracle on
identical inputs and on the device's own stage vectors, the reference's two -fct 4 known answers (autotest/out_baseline.dat:
203-210) and a 3-D whole run through the driver, and the shipped executable.  CPU twins: tests/test_efp_emu.py."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from oracle.remhos_oracle import Config, Remhos
from tests.helpers import check_rel, layout_from_oracle
from tests.test_efp_emu import check_properties, oracle_stage

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "remhos_amd", "remhos_amd_run")
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kat.json")))

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
def test_projection_kernel_gpu(lib, mesh, rs, p, prob, t):
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
    du, du2 = torch.full_like(u, float("nan")), torch.full_like(u, float("nan"))
    ctx.fct_projection(u, m, dh, dl, umin, umax, cfg.dt, du)
    ctx.fct_projection(u, m, dh, dl, umin, umax, cfg.dt, du2)
    torch.cuda.synchronize()
    got = du.cpu().numpy()
    err = _rel(got, keep["du"])
    print("identical inputs: max|du - du_oracle| / max|du_oracle| =", err)
    assert err <= 1e-12
    check_properties(uh, keep["m"], got, keep, cfg.dt)
    assert np.array_equal(got, du2.cpu().numpy())
    # the device's own stage vectors: HO kernel, mass-based average, bounds, projection
    z = lambda: torch.zeros_like(u)  # noqa: E731
    k, dulo, bmin, bmax, dud = (z() for _ in range(5))
    xmn, xmx = _dev(np.zeros(r.lat.ne)), _dev(np.zeros(r.lat.ne))
    ctx.ho_apply(u, k)
    ctx.lo_massavg(u, k, cfg.dt, dulo)
    ctx.elem_minmax(u, xmn, xmx)
    ctx.bounds(xmn, xmx, bmin, bmax)
    ctx.fct_projection(u, ctx.lumped_mass_ptr(), k, dulo, bmin, bmax, cfg.dt, dud)
    torch.cuda.synchronize()
    ctx.close()
    check_rel(p, _rel(dud.cpu().numpy(), keep["du"]), f"efp stage {mesh} p{p}")


def _kat(prefix):
    return next(a for a in KAT["autotest"] if a["name"].startswith(prefix) and a.get("fct") == 4)


@pytest.mark.parametrize("prefix", ["periodic-square auto-dt", "inline-quad pacman auto-dt"])
def test_reference_known_answers_fct4(lib, prefix):
    """autotest/out_baseline.dat:203-210 through rmhd_run: the reference's printed digits, and the oracle's run of the same
    options with the criteria of tests/test_2d.py::test_2d_cpp_driver_bounds_type_1_and_dt_control_gpu"""
    from remhos_amd.case import RmhdResult, make_config

    e = _kat(prefix)
    assert (e["lo"], e["bounds_type"], e["dt_control"]) == (5, 1, 1)
    cfg = make_config(e["mesh"], e["rs"], e["order"], e["problem"], e["dt"], e["t_final"], lo_type=5, fused=0, bounds_type=1,
                      dt_control=1, fct_type=4)
    res = RmhdResult()
    assert lib.rmhd_run(C.byref(cfg), C.byref(res)) == 0, lib.rmhd_last_error()
    print(e["name"], "mass", res.final_mass, "max", res.max_value, "loss", res.mass_loss, "steps", res.steps, res.repeats)
    assert f"{res.final_mass:.10g}" == f"{e['mass']:.10g}"
    if "max" in e:
        assert f"{res.max_value:.10g}" == f"{e['max']:.10g}"
    if "mass_loss" in e:
        assert f"{res.mass_loss:.6g}" == f"{e['mass_loss']:.6g}"
    r = Remhos(Config(mesh=e["mesh"], rs=e["rs"], order=e["order"], problem=e["problem"], dt=e["dt"], t_final=e["t_final"], lo=5,
                      fct=4, bounds_type=1, dt_control=1))
    out = r.run()
    assert (res.steps, res.repeats) == (out["steps"], r.repeats), (res.steps, res.repeats, out["steps"], r.repeats)
    assert abs(res.dt - out["dt"]) <= 1e-12 * out["dt"]
    assert abs(res.final_mass - out["mass"]) <= 1e-12 * abs(out["mass"]) and abs(res.max_value - out["max"]) <= 1e-10


def test_whole_run_3d_fct4(lib):
    """cube01_hex -rs 1 -o 2 -p 10 -dt 0.02 -tf 0.7 -lo 5 -fct 4, six steps, against the oracle"""
    from remhos_amd.case import RmhdResult, make_config

    mesh, rs, p, prob, dt, tf, ms = "cube01_hex", 1, 2, 10, 0.02, 0.7, 6
    r = Remhos(Config(mesh=mesh, rs=rs, order=p, problem=prob, dt=dt, t_final=tf, lo=5, fct=4, max_steps=ms))
    out = r.run()
    cfg = make_config(mesh, rs, p, prob, dt, tf, max_steps=ms, lo_type=5, fused=0, fct_type=4)
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


def test_binary_fct4(lib):
    """remhos_amd_run -fct 4 as a child process: the printed mass is rmhd_run's; -fct 3 is refused with the usage text;
    -vb with -fct 4 passes on a run whose LO update keeps the bounds (the limiter keeps them too, the guard is live)"""
    from remhos_amd.case import RmhdResult, make_config

    args = ["-m", "data/inline-quad.mesh", "-p", "14", "-rs", "1", "-o", "3", "-dt", "0.002", "-tf", "0.5", "-ms", "3", "-ho", "3",
            "-lo", "5"]
    p = subprocess.run([EXE] + args + ["-fct", "4"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    cfg = make_config("inline-quad", 1, 3, 14, 0.002, 0.5, max_steps=3, lo_type=5, fused=0, fct_type=4)
    res = RmhdResult()
    from remhos_amd.case import Case

    n = Case(lib, cfg)
    uf, u2 = np.zeros((n.ne_owned, n.ndof)), np.zeros((n.ne_owned, n.ndof))
    assert lib.rmhd_run_state(C.byref(cfg), C.byref(res), uf.ctypes.data, None) == 0, lib.rmhd_last_error()
    assert _printed(p.stdout, "Final mass u:") == float(f"{res.final_mass:.10g}")
    cfg2 = make_config("inline-quad", 1, 3, 14, 0.002, 0.5, max_steps=3, lo_type=5, fused=0)
    res2 = RmhdResult()
    assert lib.rmhd_run_state(C.byref(cfg2), C.byref(res2), u2.ctypes.data, None) == 0
    assert _rel(u2, uf) > 1e-6  # (not the clip-and-scale run)
    q = subprocess.run([EXE] + args + ["-fct", "3"], capture_output=True, text=True, timeout=60)
    assert q.returncode != 0 and "implements" in q.stderr and "-fct 2|4" in q.stderr
    # -vb: with -lo 5 the mass-based average itself leaves the overlap bounds on this case (the oracle's LO update does, by
    # 1.7e-5 -- the reference's guard would abort on the LO check too); with -lo 4 the oracle's LO and limited updates of all
    # nine stages stay inside, so the guard has to pass
    lo4 = [a for a in args[:-1]] + ["4"]
    w = subprocess.run([EXE] + lo4 + ["-fct", "4"], capture_output=True, text=True, timeout=600)
    assert w.returncode == 0, (w.returncode, w.stdout[-2000:], w.stderr[-2000:])
    v = subprocess.run([EXE] + lo4 + ["-fct", "4", "-vb"], capture_output=True, text=True, timeout=600)
    assert v.returncode == 0, (v.returncode, v.stdout[-2000:], v.stderr[-2000:])
    assert _printed(v.stdout, "Final mass u:") == _printed(w.stdout, "Final mass u:")
