"""NeumannHOSolver (-ho 1; remhos_ho.cpp:131-187) under the host emulation: the kernels of remhos_amd/csrc/rmh_neumann.hpp
(rmh_ho_neumann, rmh_last_neumann) against the restatement of tests/neumann_oracle.py on identical inputs -- the number of
updates, the residual norm of every check, du, run-to-run bit identity, the dependence on the pseudo-time, that it is not -ho 3 --
and the driver's ho_type = 1 path with its refusals.  GPU twins: tests/test_gpu_neumann.py.

The solver is crude by design (it usually runs out its 20 updates far from M^-1 rhs), so what is compared is the reference's
stopping iteration; every case keeps its norms at least 1e-6 (relative) away from the threshold 1e-4, and the test asserts that.
The bound on du is computed per case from the ORACLE's element mass matrices:
    tol = max(1e-12, 256 * amp * 2^-53),   amp = max_e sum_{k<20} ||(I - M_L^-1 M_e)^k||_inf     relative to max|du|."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.helpers import emu_library_path, layout_from_oracle, perturbed
from tests.neumann_oracle import MAX_UPDATES, TOL, Config, NeumannRemhos, neumann_tol

# (mesh, rs, p, problem, t, perturbed input, the check at which the oracle stops -- 0: it runs out its 20 updates)
CASES = [("cube01_hex", 0, 1, 10, 0.3, True, 0), ("cube01_hex", 0, 3, 10, 0.3, True, 0), ("periodic-cube", 0, 3, 0, 0.0, True, 0),
         ("periodic-cube", 0, 6, 0, 0.0, True, 0), ("inline-quad", 1, 3, 14, 0.3, True, 0), ("inline-quad", 1, 6, 14, 0.3, True, 0),
         ("periodic-square", 1, 3, 5, 0.0, True, 0), ("cube01_hex", 1, 2, 10, 0.3, True, 19), ("cube01_hex", 1, 3, 10, 0.3, True, 12),
         ("inline-quad", 1, 1, 14, 0.3, False, 15)]
IDS = [f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{c[4]}" + ("" if c[5] else "-unperturbed") for c in CASES]


@pytest.fixture(scope="module")
def lib():
    from remhos_amd.capi import load_library
    from remhos_amd.case import bind_driver

    return bind_driver(load_library(emu_library_path()))


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@functools.lru_cache(maxsize=None)
def oracle_ho1(mesh, rs, p, prob, t, pert=True):
    """inputs and the result of one -ho 1 solve of the restatement at the geometry of time t (computed once per session)"""
    dim2 = mesh in ("inline-quad", "periodic-square")
    cfg = Config(mesh=mesh, rs=rs, order=p, problem=prob, dt=0.004 if dim2 else 0.02, t_final=0.7, lo=2, fct=2)
    r = NeumannRemhos(cfg)
    u = perturbed(r.u) if pert else r.u.copy()
    if r.exec_mode == 1:
        r.update_geometry(t)
    du, updates, norms = r.calc_ho_neumann_info(u)
    assert np.array_equal(du, r.calc_ho_neumann(u))  # (the helper restates tests/pdu_oracle.py operation by operation)
    keep = dict(du=du, updates=updates, norms=norms, tol=neumann_tol(r), amp=r.amplification(), du3=r.calc_ho(u))
    for a in (u, du, norms, keep["du3"]):
        a.setflags(write=False)
    return r, u, keep


def check_case_condition(keep, stop):
    """the case itself: every norm the oracle evaluated is at least 1e-6 (relative) away from the threshold, and the oracle
    stops where the case table says"""
    gap = float(np.abs(keep["norms"] - TOL).min() / TOL)
    print(f"oracle: updates = {keep['updates']}, checks = {len(keep['norms'])}, smallest |norm - 1e-4| / 1e-4 = {gap:.3e}, amp = {keep['amp']:.4g}")
    assert gap >= 1e-6
    if stop:
        assert keep["updates"] == stop - 1 and len(keep["norms"]) == stop and keep["norms"][-1] <= TOL
    else:
        assert keep["updates"] == MAX_UPDATES and len(keep["norms"]) == MAX_UPDATES


def check_ho1(keep, du, du_again, updates, norms, du3, where):
    nk = len(keep["norms"])
    norms = np.asarray(norms)
    assert updates == keep["updates"], (updates, keep["updates"], norms, keep["norms"])
    nerr = float(np.abs(norms[:nk] / keep["norms"] - 1.0).max()) if keep["norms"].min() > 0 else float(np.abs(norms[:nk] - keep["norms"]).max())
    assert np.isnan(norms[nk:]).all()  # (checks that were not evaluated)
    err, tol = _rel(du, keep["du"]), keep["tol"]
    print(f"{where}: updates = {updates}   max rel. error of the norms = {nerr:.3e}   max|du - oracle| / max|oracle| = {err:.3e}   bound = {tol:.3e}"
          f"   (amp = {keep['amp']:.4g})")
    assert nerr <= 1e-10
    assert err <= tol
    assert np.array_equal(du, du_again)
    # the inputs tell -ho 1 from -ho 3, in the restatement and in the library
    assert _rel(keep["du"], keep["du3"]) > 1e-3
    assert _rel(du, du3) > 1e-3


@pytest.mark.parametrize("mesh,rs,p,prob,t,pert,stop", CASES, ids=IDS)
def test_ho_neumann_vs_oracle(lib, mesh, rs, p, prob, t, pert, stop):
    from remhos_amd.capi import Context

    r, u, keep = oracle_ho1(mesh, rs, p, prob, t, pert)
    check_case_condition(keep, stop)
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=p, exec_mode=r.exec_mode, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    ctx.setup(t)
    du, du2, du3 = np.full_like(u, np.nan), np.full_like(u, np.nan), np.full_like(u, np.nan)
    ctx.ho_neumann(u, du)
    updates, norms = ctx.last_neumann()
    ctx.ho_neumann(u, du2)
    assert ctx.last_neumann()[0] == updates
    ctx.ho_apply(u, du3)
    ctx.close()
    check_ho1(keep, du, du2, updates, norms, du3, "emulation")


def test_ho_neumann_leaves_the_lumped_mass(lib):
    """rmh_ho_neumann forms the context's lumped mass and leaves it current: rmh_lo_massavg, which refuses to run without it,
    follows it and gives the restatement's mass-based average of the Neumann rate"""
    from remhos_amd.capi import Context

    r, u, keep = oracle_ho1("inline-quad", 1, 3, 14, 0.3)
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=3, exec_mode=1, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    ctx.setup(0.3)
    du, lo = np.zeros_like(u), np.zeros_like(u)
    ctx.ho_neumann(u, du)
    ctx.lo_massavg(u, du, 0.004, lo)
    ctx.close()
    assert _rel(lo, r.calc_lo_massavg(u, keep["du"], 0.004)) <= 10.0 * keep["tol"]


def test_ho_neumann_follows_the_moved_mesh(lib):
    """the same inputs at another pseudo-time give another answer: the geometry of rmh_setup(t) is what the kernels use"""
    from remhos_amd.capi import Context

    r, u, keep = oracle_ho1("cube01_hex", 0, 3, 10, 0.3)
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=3, exec_mode=1, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    du = np.zeros_like(u)
    ctx.setup(0.0)
    ctx.ho_neumann(u, du)
    ctx.close()
    assert _rel(du, keep["du"]) > 1e-6


@pytest.mark.parametrize("mesh,p,prob", [("cube01_hex", 2, 10), ("inline-quad", 3, 14)])
def test_ho_neumann_zero_input(lib, mesh, p, prob):
    """u = 0: the first check passes (norm 0), no update is applied, du is exactly zero"""
    from remhos_amd.capi import Context

    r, u, keep = oracle_ho1(mesh, 0 if mesh == "cube01_hex" else 1, p, prob, 0.3)
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=p, exec_mode=1, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    ctx.setup(0.3)
    du = np.full_like(u, np.nan)
    ctx.ho_neumann(np.zeros_like(u), du)
    updates, norms = ctx.last_neumann()
    ctx.close()
    assert np.all(du == 0.0) and updates == 0 and norms[0] == 0.0 and np.isnan(norms[1:]).all()


def test_ho_neumann_refuses_ghosts(lib):
    from remhos_amd.capi import Context
    from remhos_amd.case import Case, make_config

    c = Case(lib, make_config("cube01_hex", 1, 1, 10, -1.0, 0.5, part=(2, 1, 1), rank=0))
    assert c.ne_ghost > 0
    ctx = Context(lib, order=1, exec_mode=c.exec_mode, x0=c.x0, vel=c.vel, face_nbr=c.face_nbr, stencil27=c.stencil27,
                  ne_ghost=c.ne_ghost)
    ctx.setup(0.0)
    u = np.ascontiguousarray(c.u0, dtype=np.float64)
    du = np.zeros_like(u)
    assert lib.rmh_ho_neumann(ctx.h, u.ctypes.data, du.ctypes.data) != 0
    msg = lib.rmh_last_error()
    ctx.close()
    assert b"-ho 1" in msg and b"ghost" in msg


def driver_vs_oracle(lib, mesh, rs, p, prob, dt, tf, ms, lo, fct):
    """ms steps of ho_type = 1 through rmhd_run_state against the restatement's run; returns (field of the run, restatement)"""
    from remhos_amd.case import RmhdResult, make_config

    r = NeumannRemhos(Config(mesh=mesh, rs=rs, order=p, problem=prob, dt=dt, t_final=tf, lo=lo, fct=fct, max_steps=ms))
    out = r.run()
    tol = 10.0 * neumann_tol(r)
    cfg = make_config(mesh, rs, p, prob, dt, tf, max_steps=ms, lo_type=lo, fused=0, fct_type=fct, ho_type=1)
    res = RmhdResult()
    uf = np.zeros_like(r.u)
    assert lib.rmhd_run_state(C.byref(cfg), C.byref(res), uf.ctypes.data, None) == 0, lib.rmhd_last_error()
    assert res.steps == out["steps"] == ms
    print("mass", res.final_mass, out["mass"], "field", _rel(uf, r.u), "bound", tol)
    assert abs(res.final_mass - out["mass"]) <= 1e-12 * abs(out["mass"])
    assert _rel(uf, r.u) <= tol
    return uf, r


def test_driver_ho1_vs_oracle(lib):
    from remhos_amd.case import RmhdResult, make_config

    mesh, rs, p, prob, dt, tf, ms = "inline-quad", 1, 3, 14, 0.002, 0.5, 2
    uf, r = driver_vs_oracle(lib, mesh, rs, p, prob, dt, tf, ms, 2, 2)
    # and it is not the -ho 3 run
    res3 = RmhdResult()
    u3 = np.zeros_like(uf)
    cfg3 = make_config(mesh, rs, p, prob, dt, tf, max_steps=ms, lo_type=2, fused=0, fct_type=2, ho_type=3)
    assert lib.rmhd_run_state(C.byref(cfg3), C.byref(res3), u3.ctypes.data, None) == 0
    assert _rel(u3, uf) > 1e-6


def test_driver_ho1_refusals(lib):
    from remhos_amd.case import RmhdResult, make_config

    base = dict(mesh="cube01_hex", rs=0, order=2, problem=10, dt=0.02, t_final=0.7, max_steps=1, lo_type=5, ho_type=1)

    def refused(call, **kw):
        res = RmhdResult()
        cfg = make_config(**{**base, **kw})
        assert call(cfg, res) != 0
        msg = lib.rmhd_last_error()
        assert msg
        return msg

    run = lambda cfg, res: lib.rmhd_run(C.byref(cfg), C.byref(res))  # noqa: E731
    part = lambda cfg, res: lib.rmhd_run_partitioned(C.byref(cfg), None, 0, C.byref(res))  # noqa: E731
    msg = refused(run, fused=1)
    assert b"-ho 1" in msg and b"fused" in msg
    msg = refused(run, fused=0, pa=1)
    assert b"-ho 1" in msg and b"-pa" in msg and b"PA for DG is not supported" in msg
    msg = refused(run, fused=0, ps=1, ode_solver=11)
    assert b"-ho 1" in msg and b"-ps" in msg
    for call, kw in ((part, dict(fused=1)), (run, dict(fused=0))):
        msg = refused(call, part=(2, 1, 1), **kw)
        assert b"-ho 1" in msg and b"partitioned" in msg
    msg = refused(run, fused=0, ho_type=7)
    assert b"ho_type" in msg and b"7" in msg
    msg = refused(run, fused=1, ho_type=7)  # (no value falls through to the local inverse, whatever the path)
    assert b"ho_type" in msg and b"7" in msg


def test_stepper_refuses_ho1():
    """the one-kernel stage of remhos_amd/stepper.py has the local inverse built in: ho_type = 1 raises before anything runs"""
    import types

    from remhos_amd.stepper import Stepper

    case = types.SimpleNamespace(cfg=types.SimpleNamespace(lo_type=5, ho_type=1), peers=[])
    with pytest.raises(ValueError, match="-ho 1"):
        Stepper(None, case, device="cpu")
