"""DiscreteUpwind (-lo 1; remhos_lo.cpp:31-100) and FluxBasedFCT (-fct 1; remhos_fct.cpp:155-181, 295-446) under the host emulation:
the kernels of remhos_amd/csrc/rmh_upwind.hpp (rmh_lo_upwind, rmh_fct_fluxbased) against the restatement of tests/upwind_oracle.py
on identical inputs, their conservation / bounds properties, run-to-run bit identity, and the driver's -lo 1 / -fct 1 path with
its refusals.  GPU twins: tests/test_gpu_upwind.py."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import emu_library_path, layout_from_oracle, perturbed
from tests.test_efp_emu import CASES as EFP_CASES
from tests.upwind_oracle import Config, UpwindRemhos

# the list of tests/test_efp_emu.py (3-D p = 1..6 on cube01_hex -rs 0 at t = 0.3 and periodic-cube -rs 0, 2-D p = 1..3) + 2-D p = 6
CASES = list(EFP_CASES) + [("inline-quad", 1, 6, 14, 0.3)]


@pytest.fixture(scope="module")
def lib():
    from remhos_amd.capi import load_library
    from remhos_amd.case import bind_driver

    return bind_driver(load_library(emu_library_path()))


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def oracle_stage(mesh, rs, p, prob, t, dt=None):
    """inputs and results of one -lo 1 -fct 1 stage of the restatement on a perturbed field"""
    dim2 = mesh in ("inline-quad", "periodic-square")
    dt = dt if dt is not None else (0.004 if dim2 else 0.02)
    cfg = Config(mesh=mesh, rs=rs, order=p, problem=prob, dt=dt, t_final=0.7, lo=1, fct=1)
    r = UpwindRemhos(cfg)
    r.refine_steps = 2
    u = perturbed(r.u)
    keep = {}
    r.stage(u, t, cfg.dt, keep)
    r.calc_lo_upwind(u, keep)  # (+ the face-flux sums)
    keep["conv"] = r.conv_apply(u)
    return r, cfg, u, keep


def check_lo_conservation(m, du_lo, keep):
    """the diffusive part d_ij (u_j - u_i) moves mass between the dofs of an element only: sum_i m_i du_lo_i equals the sums of
    the convective term and the lumped face fluxes"""
    want = (keep["conv"] + keep["face"]).sum(axis=1)
    got = (m * du_lo).sum(axis=1)
    scale = np.abs(m * du_lo).sum(axis=1)
    print("LO conservation defect / scale (worst):", float((np.abs(got - want) / np.maximum(scale, 1e-300)).max()))
    assert (np.abs(got - want) <= 1e-12 * scale).all()


def check_fct_properties(u, m, du, keep, dt):
    """conservation per element and the bounds, on the library's own result"""
    defect = np.abs((m * (du - keep["du_lo"])).sum(axis=1))
    scale = np.abs(m * du).sum(axis=1)
    print("FCT conservation defect / scale (worst):", float((defect / np.maximum(scale, 1e-300)).max()))
    assert (defect <= 1e-12 * scale).all()
    un = u + dt * du
    print("bounds: undershoot", float((keep["umin"] - un).max()), "overshoot", float((un - keep["umax"]).max()))
    assert (un >= keep["umin"] - 1e-12).all() and (un <= keep["umax"] + 1e-12).all()


@pytest.mark.parametrize("mesh,rs,p,prob,t", CASES)
def test_upwind_kernels_vs_oracle(lib, mesh, rs, p, prob, t):
    from remhos_amd.capi import Context

    r, cfg, u, keep = oracle_stage(mesh, rs, p, prob, t)
    cs = r.clip_scale(u, keep["m"], keep["du_ho"], keep["du_lo"], keep["umin"], keep["umax"], cfg.dt)
    assert _rel(cs, keep["du"]) > 1e-4  # (the inputs tell the two limiters apart)
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=p, exec_mode=r.exec_mode, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    ctx.setup(t)
    lo, lo2, du, du2 = (np.full_like(u, np.nan) for _ in range(4))
    ctx.lo_upwind(u, lo)
    ctx.lo_upwind(u, lo2)
    args = (u, keep["m"], keep["du_ho"], keep["du_lo"], keep["umin"], keep["umax"], cfg.dt)
    ctx.fct_fluxbased(*args, du)
    ctx.fct_fluxbased(*args, du2)
    ctx.close()
    e_lo, e_du = _rel(lo, keep["du_lo"]), _rel(du, keep["du"])
    print("max|du_lo - oracle| / max|oracle| =", e_lo, "  max|du - oracle| / max|oracle| =", e_du)
    assert e_lo <= 1e-12 and e_du <= 1e-12
    check_lo_conservation(keep["m"], lo, keep)
    check_fct_properties(u, keep["m"], du, keep, cfg.dt)
    assert np.array_equal(lo, lo2) and np.array_equal(du, du2)


def test_upwind_follows_the_moved_mesh(lib):
    """the same inputs at another pseudo-time give another answer: the geometry of rmh_setup(t) is what the kernels use"""
    from remhos_amd.capi import Context

    r, cfg, u, keep = oracle_stage("cube01_hex", 0, 2, 10, 0.3)
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=2, exec_mode=1, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    lo, du = np.zeros_like(u), np.zeros_like(u)
    ctx.setup(0.0)
    ctx.lo_upwind(u, lo)
    ctx.fct_fluxbased(u, keep["m"], keep["du_ho"], keep["du_lo"], keep["umin"], keep["umax"], cfg.dt, du)
    ctx.close()
    assert _rel(lo, keep["du_lo"]) > 1e-6 and _rel(du, keep["du"]) > 1e-6


def test_driver_lo1_fct1_vs_oracle(lib):
    from remhos_amd.case import RmhdResult, make_config

    mesh, rs, p, prob, dt, tf, ms = "inline-quad", 1, 3, 14, 0.002, 0.5, 2
    r = UpwindRemhos(Config(mesh=mesh, rs=rs, order=p, problem=prob, dt=dt, t_final=tf, lo=1, fct=1, max_steps=ms))
    out = r.run()
    cfg = make_config(mesh, rs, p, prob, dt, tf, max_steps=ms, lo_type=1, fused=0, fct_type=1)
    res = RmhdResult()
    uf = np.zeros_like(r.u)
    assert lib.rmhd_run_state(C.byref(cfg), C.byref(res), uf.ctypes.data, None) == 0, lib.rmhd_last_error()
    assert res.steps == out["steps"] == ms
    print("mass", res.final_mass, out["mass"], "field", _rel(uf, r.u))
    assert abs(res.final_mass - out["mass"]) <= 1e-12 * abs(out["mass"])
    assert _rel(uf, r.u) < 1e-10
    # and it is not the -lo 5 -fct 2 run
    res2 = RmhdResult()
    u2 = np.zeros_like(r.u)
    cfg2 = make_config(mesh, rs, p, prob, dt, tf, max_steps=ms, lo_type=5, fused=0)
    assert lib.rmhd_run_state(C.byref(cfg2), C.byref(res2), u2.ctypes.data, None) == 0
    assert _rel(u2, uf) > 1e-6


def test_driver_upwind_refusals(lib):
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
    assert b"fused" in refused(run, fct_type=1, fused=1)
    assert b"fused" in refused(run, lo_type=1, fused=1)
    assert b"ps" in refused(run, fct_type=1, fused=0, ps=1, ode_solver=11)
    assert b"ps" in refused(run, lo_type=1, fused=0, ps=1, ode_solver=11)
    assert b"Flux-based FCT and PA are incompatible." in refused(run, fct_type=1, fused=0, pa=1)  # remhos.cpp:1088
    assert b"partitioned" in refused(part, fct_type=1, fused=0, part=(2, 1, 1))
    assert b"partitioned" in refused(part, lo_type=1, fused=1, part=(2, 1, 1))
    assert b"partitioned" in refused(run, lo_type=1, fused=0, part=(2, 1, 1))
    assert b"fct" in refused(run, fct_type=3, fused=0)  # (-fct 3 stays refused)
