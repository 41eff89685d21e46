"""Preconditioned DiscreteUpwind (-lo 2; remhos.cpp:749-771, 937-942, remhos_tools.cpp:975-1031) under the host emulation:
lo_upwind_prec_kernel of remhos_amd/csrc/rmh_pdu.hpp (rmh_lo_upwind_prec) against the restatement of tests/pdu_oracle.py on
identical inputs, conservation, run-to-run bit identity, its dependence on the pseudo-time, and the driver's lo_type = 2 path
with its refusals.  GPU twins: tests/test_gpu_pdu.py.

The tolerance of a stage is computed per case from the ORACLE's dense element mass:
    tol = max(1e-12, 16 * max_e cond_2(M_e) * 2^-53)     relative to max|du_lo|
-- the backward-error amplification of a Cholesky solve, with a margin for the different summation order."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import emu_library_path, layout_from_oracle, perturbed
from tests.pdu_oracle import Config, PduRemhos
from tests.test_upwind_emu import check_lo_conservation

# moved mesh + boundary faces in 3-D at every supported order; periodic neighbours, transport; 2-D at the lowest, a middle and the
# highest order; 2-D periodic transport
CASES = [("cube01_hex", 0, 1, 10, 0.3), ("cube01_hex", 0, 2, 10, 0.3), ("cube01_hex", 0, 3, 10, 0.3), ("periodic-cube", 0, 3, 0, 0.0),
         ("inline-quad", 1, 1, 14, 0.3), ("inline-quad", 1, 3, 14, 0.3), ("inline-quad", 1, 6, 14, 0.3),
         ("periodic-square", 1, 3, 5, 0.0)]


@pytest.fixture(scope="module")
def lib():
    from remhos_amd.capi import load_library
    from remhos_amd.case import bind_driver

    return bind_driver(load_library(emu_library_path()))


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def stage_tol(r):
    return max(1e-12, 16.0 * r.mass_cond() * 2.0**-53)


def oracle_lo2(mesh, rs, p, prob, t):
    """inputs and the result of one -lo 2 solve of the restatement on a perturbed field, at the geometry of time t"""
    dim2 = mesh in ("inline-quad", "periodic-square")
    cfg = Config(mesh=mesh, rs=rs, order=p, problem=prob, dt=0.004 if dim2 else 0.02, t_final=0.7, lo=2, fct=2)
    r = PduRemhos(cfg)
    u = perturbed(r.u)
    if r.exec_mode == 1:
        r.update_geometry(t)
    keep = {}
    keep["du_lo"] = r.calc_lo_upwind_prec(u, keep)  # (+ conv = K u of the preconditioned matrix, face = the lumped face fluxes)
    keep["m"] = r.m.copy()
    return r, cfg, u, keep


def check_lo2(r, u, keep, lo, lo_again, where):
    err, tol = _rel(lo, keep["du_lo"]), stage_tol(r)
    print(f"{where}: max|du_lo - oracle| / max|oracle| = {err:.3e}   bound = {tol:.3e}   (cond_2(M_e) = {r.mass_cond():.4g})")
    assert err <= tol
    assert _rel(r.calc_lo_upwind(u), keep["du_lo"]) > 1e-4  # (the inputs tell -lo 2 from -lo 1)
    check_lo_conservation(keep["m"], lo, keep)
    assert np.array_equal(lo, lo_again)


@pytest.mark.parametrize("mesh,rs,p,prob,t", CASES)
def test_lo_upwind_prec_vs_oracle(lib, mesh, rs, p, prob, t):
    from remhos_amd.capi import Context

    r, cfg, u, keep = oracle_lo2(mesh, rs, p, prob, t)
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=p, exec_mode=r.exec_mode, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    ctx.setup(t)
    lo, lo2 = np.full_like(u, np.nan), np.full_like(u, np.nan)
    ctx.lo_upwind_prec(u, lo)
    ctx.lo_upwind_prec(u, lo2)
    ctx.close()
    check_lo2(r, u, keep, lo, lo2, "emulation")


def test_lo_upwind_prec_follows_the_moved_mesh(lib):
    """the same inputs at another pseudo-time give another answer: the geometry of rmh_setup(t) is what the kernel uses"""
    from remhos_amd.capi import Context

    r, cfg, u, keep = oracle_lo2("cube01_hex", 0, 2, 10, 0.3)
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=2, exec_mode=1, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    lo = np.zeros_like(u)
    ctx.setup(0.0)
    ctx.lo_upwind_prec(u, lo)
    ctx.close()
    assert _rel(lo, keep["du_lo"]) > 1e-6


def test_lo_upwind_prec_refuses_3d_order_4(lib):
    from remhos_amd.capi import Context

    r = PduRemhos(Config(mesh="cube01_hex", rs=0, order=4, problem=10, dt=0.02, t_final=0.7, lo=5, fct=2))
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=4, exec_mode=1, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    ctx.setup(0.0)
    lo = np.zeros_like(r.u)
    assert lib.rmh_lo_upwind_prec(ctx.h, r.u.ctypes.data, lo.ctypes.data) != 0
    msg = lib.rmh_last_error()
    ctx.close()
    assert b"-lo 2" in msg and b"order 4" in msg


def test_driver_lo2_vs_oracle(lib):
    from remhos_amd.case import RmhdResult, make_config

    mesh, rs, p, prob, dt, tf, ms = "inline-quad", 1, 3, 14, 0.002, 0.5, 2
    r = PduRemhos(Config(mesh=mesh, rs=rs, order=p, problem=prob, dt=dt, t_final=tf, lo=2, fct=2, max_steps=ms))
    out = r.run()
    tol = 10.0 * stage_tol(r)
    cfg = make_config(mesh, rs, p, prob, dt, tf, max_steps=ms, lo_type=2, fused=0, fct_type=2, ho_type=3)
    res = RmhdResult()
    uf = np.zeros_like(r.u)
    assert lib.rmhd_run_state(C.byref(cfg), C.byref(res), uf.ctypes.data, None) == 0, lib.rmhd_last_error()
    assert res.steps == out["steps"] == ms
    print("mass", res.final_mass, out["mass"], "field", _rel(uf, r.u), "bound", tol)
    assert abs(res.final_mass - out["mass"]) <= 1e-12 * abs(out["mass"])
    assert _rel(uf, r.u) <= tol
    # and it is not the -lo 1 run
    res1 = RmhdResult()
    u1 = np.zeros_like(r.u)
    cfg1 = make_config(mesh, rs, p, prob, dt, tf, max_steps=ms, lo_type=1, fused=0, fct_type=2, ho_type=3)
    assert lib.rmhd_run_state(C.byref(cfg1), C.byref(res1), u1.ctypes.data, None) == 0
    assert _rel(u1, uf) > 1e-6


def test_driver_lo2_refusals(lib):
    from remhos_amd.case import RmhdResult, make_config

    base = dict(mesh="cube01_hex", rs=0, order=2, problem=10, dt=0.02, t_final=0.7, max_steps=1, lo_type=2)

    def refused(call, **kw):
        res = RmhdResult()
        cfg = make_config(**{**base, **kw})
        assert call(cfg, res) != 0
        msg = lib.rmhd_last_error()
        assert msg
        return msg

    run = lambda cfg, res: lib.rmhd_run(C.byref(cfg), C.byref(res))  # noqa: E731
    part = lambda cfg, res: lib.rmhd_run_partitioned(C.byref(cfg), None, 0, C.byref(res))  # noqa: E731
    assert b"fused" in refused(run, fused=1)
    assert b"ps" in refused(run, fused=0, ps=1, ode_solver=11)
    assert b"partitioned" in refused(part, fused=1, part=(2, 1, 1))
    assert b"partitioned" in refused(run, fused=0, part=(2, 1, 1))
    msg = refused(run, fused=0, order=4)
    assert b"-lo 2" in msg and b"order 4" in msg
