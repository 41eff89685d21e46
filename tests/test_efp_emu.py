"""ElementFCTProjection (-fct 4; remhos_fct.cpp:613-731) under the host emulation: the kernel of remhos_amd/csrc/rmh_efp.hpp
(rmh_fct_projection) against the oracle's restatement on identical inputs, its own conservation / bounds properties, run-to-run
bit identity, and the driver's -fct 4 path (rmhd_config.fct_type) with its refusals.  GPU twins: tests/test_gpu_efp.py."""
import ctypes as C

import numpy as np
import pytest

from oracle.remhos_oracle import Config, Remhos
from tests.helpers import emu_library_path, layout_from_oracle, perturbed

# (mesh, rs, order, problem, t): remap cases at t != 0 prove that the mass matrix is built on the moved mesh and, in 3-D, that
# the hierarchical nodes are undone correctly
CASES = [
    ("inline-quad", 1, 3, 14, 0.3), ("periodic-square", 1, 3, 5, 0.0), ("inline-quad", 1, 1, 14, 0.3), ("inline-quad", 1, 2, 14, 0.3),
    ("cube01_hex", 0, 2, 10, 0.3), ("cube01_hex", 0, 3, 10, 0.3), ("periodic-cube", 0, 3, 0, 0.0), ("cube01_hex", 0, 6, 10, 0.3),
    ("cube01_hex", 0, 1, 10, 0.3), ("cube01_hex", 0, 4, 10, 0.3), ("cube01_hex", 0, 5, 10, 0.3),
]


@pytest.fixture(scope="module")
def lib():
    from remhos_amd.capi import load_library
    from remhos_amd.case import bind_driver

    return bind_driver(load_library(emu_library_path()))


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def oracle_stage(mesh, rs, p, prob, t, dt=None):
    """inputs and result of one -fct 4 stage of the oracle on a perturbed field"""
    dim2 = mesh in ("inline-quad", "periodic-square")
    dt = dt if dt is not None else (0.004 if dim2 else 0.02)
    cfg = Config(mesh=mesh, rs=rs, order=p, problem=prob, dt=dt, t_final=0.7, lo=5, fct=4)
    r = Remhos(cfg)
    r.refine_steps = 2
    u = perturbed(r.u)
    keep = {}
    r.stage(u, t, cfg.dt, keep)
    return r, cfg, u, keep


def check_properties(u, m, du, keep, dt):
    """conservation per element and the -vb bounds, on the library's own result with the oracle's lumped mass"""
    defect = np.abs((m * (du - keep["du_lo"])).sum(axis=1))
    scale = np.abs(m * du).sum(axis=1)
    print("conservation defect / scale (worst):", float((defect / np.maximum(scale, 1e-300)).max()))
    assert (defect <= 1e-12 * scale).all()
    un = u + dt * du
    print("bounds: undershoot", float((keep["umin"] - un).max()), "overshoot", float((un - keep["umax"]).max()))
    assert (un >= keep["umin"] - 1e-12).all() and (un <= keep["umax"] + 1e-12).all()


@pytest.mark.parametrize("mesh,rs,p,prob,t", CASES)
def test_projection_kernel_vs_oracle(lib, mesh, rs, p, prob, t):
    from remhos_amd.capi import Context

    r, cfg, u, keep = oracle_stage(mesh, rs, p, prob, t)
    # the inputs tell the two limiters apart (from the oracle alone)
    cs = r.clip_scale(u, keep["m"], keep["du_ho"], keep["du_lo"], keep["umin"], keep["umax"], cfg.dt)
    assert _rel(cs, keep["du"]) > 1e-4
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=p, exec_mode=r.exec_mode, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    ctx.setup(t)
    du, du2 = np.full_like(u, np.nan), np.full_like(u, np.nan)
    args = (u, keep["m"], keep["du_ho"], keep["du_lo"], keep["umin"], keep["umax"], cfg.dt)
    ctx.fct_projection(*args, du)
    ctx.fct_projection(*args, du2)
    ctx.close()
    err = _rel(du, keep["du"])
    print("max|du - du_oracle| / max|du_oracle| =", err)
    assert err <= 1e-12
    check_properties(u, keep["m"], du, keep, cfg.dt)
    assert np.array_equal(du, du2)


def test_projection_follows_the_moved_mesh(lib):
    """the same inputs at another pseudo-time give another answer: the geometry of rmh_setup(t) is what the kernel uses"""
    from remhos_amd.capi import Context

    r, cfg, u, keep = oracle_stage("cube01_hex", 0, 2, 10, 0.3)
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=2, exec_mode=1, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    du = np.zeros_like(u)
    ctx.setup(0.0)
    ctx.fct_projection(u, keep["m"], keep["du_ho"], keep["du_lo"], keep["umin"], keep["umax"], cfg.dt, du)
    ctx.close()
    assert _rel(du, keep["du"]) > 1e-6


def test_driver_fct4_vs_oracle(lib):
    from remhos_amd.case import RmhdResult, make_config

    mesh, rs, p, prob, dt, tf, ms = "inline-quad", 1, 3, 14, 0.002, 0.5, 2
    r = Remhos(Config(mesh=mesh, rs=rs, order=p, problem=prob, dt=dt, t_final=tf, lo=5, fct=4, max_steps=ms))
    out = r.run()
    cfg = make_config(mesh, rs, p, prob, dt, tf, max_steps=ms, lo_type=5, fused=0, fct_type=4)
    res = RmhdResult()
    uf = np.zeros_like(r.u)
    assert lib.rmhd_run_state(C.byref(cfg), C.byref(res), uf.ctypes.data, None) == 0, lib.rmhd_last_error()
    assert res.steps == out["steps"] == ms
    print("mass", res.final_mass, out["mass"], "field", _rel(uf, r.u))
    assert abs(res.final_mass - out["mass"]) <= 1e-12 * abs(out["mass"])
    assert _rel(uf, r.u) < 1e-10
    # and it is not the clip-and-scale run
    res2 = RmhdResult()
    u2 = np.zeros_like(r.u)
    cfg2 = make_config(mesh, rs, p, prob, dt, tf, max_steps=ms, lo_type=5, fused=0)
    assert lib.rmhd_run_state(C.byref(cfg2), C.byref(res2), u2.ctypes.data, None) == 0
    assert _rel(u2, uf) > 1e-6


def test_driver_fct4_refusals(lib):
    from remhos_amd.case import RmhdResult, make_config

    base = dict(mesh="cube01_hex", rs=0, order=2, problem=10, dt=0.02, t_final=0.7, max_steps=1, lo_type=5)

    def refused(call, **kw):
        res = RmhdResult()
        cfg = make_config(**{**base, **kw})
        assert call(cfg, res) != 0
        msg = lib.rmhd_last_error()
        assert msg
        return msg

    run = lambda cfg, res: lib.rmhd_run(C.byref(cfg), C.byref(res))  # noqa: E731
    part = lambda cfg, res: lib.rmhd_run_partitioned(C.byref(cfg), None, 0, C.byref(res))  # noqa: E731
    assert b"fused" in refused(run, fct_type=4, fused=1)
    assert b"ps" in refused(run, fct_type=4, fused=0, ps=1, ode_solver=11)
    assert b"fct" in refused(run, fct_type=3, fused=0)
    assert b"fct" in refused(part, fct_type=4, fused=1, part=(2, 1, 1))
    assert b"fct" in refused(part, fct_type=4, fused=0, part=(2, 1, 1))
