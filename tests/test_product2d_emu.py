"""Product-field remap (-ps) on quadrilateral lattices (rmh_layout.dim = 2, remhos_amd/csrc/rmh_product2d.hpp): the three
product kernels behind rmh_product_ratio, rmh_elem_minmax_masked and rmh_fct_product against the oracle's restatement of
remhos_sync.cpp / remhos_fct.cpp:26-153, 543-566 ON IDENTICAL INPUTS, whole -ps runs through rmhd_run_state against
Remhos(Config(ps=True, ode=11|12|13)) (pinned by the reference's "Product remap 2D IDP3" known answer,
tests/test_oracle_kat.py::test_product_remap_idp3), and the refusals.  CPU: the g++ emulation build of the same kernel
sources; the GPU twin, tests/test_gpu_product2d.py, runs the same checks on the device."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle.remhos_oracle import (Config, Lattice, Remhos, compute_bool_indicators, compute_ratio, elem_minmax_masked,
                                  fct_product)
from tests.helpers import check_rel, layout_from_oracle

VEC_TOL = 1e-12   # the relative tolerance of the 3-D kernels (tests/test_gpu_product.py: check_product(..., 1e-12))
CONS_TOL = 1e-13  # conservation of sum m us per element, tests/test_product_remap.py::check_product
T_STAGE, DT = 0.3, 0.005


@functools.lru_cache(maxsize=None)
def product2d_case(p, n=8):
    """Inputs and the oracle's outputs of the second block of AdvectionOperator::LimitMult (remhos.cpp:1848-1915) on
    inline-quad (n = 8: -rs 1, n = 16: -rs 2; n = 5: the same square cut into 5 x 5 elements, a count that is no multiple of
    the four elements of a workgroup), problem 14 (the pacman field: regions of exact zero), mesh of pseudo-time 0.3, after
    one IDP stage; us = u s0(x) with a non-constant s0.  Computed once per (p, n) and never modified."""
    lat = Lattice(2, (n, n), False, [np.linspace(0.0, 1.0, n + 1) for _ in range(2)], 2)
    r = Remhos(Config(mesh="inline-quad", rs=1, order=p, problem=14, dt=DT, t_final=0.5, lo=5, fct=2, ps=True, ode=11), lat)
    r.refine_steps = 2 if p >= 4 else 0
    # one IDP (forward Euler) stage of the pacman field
    du, dus = r.mult_unlimited(r.u, r.us, T_STAGE)
    du, dus = r.limit_mult(r.u, r.us, du, dus, DT)
    u = r.u + DT * du
    x = np.einsum("an,enc->eac", r.T.PsiCU, r.X0)
    s0 = 2.0 + 0.9 * np.sin(7.0 * x[..., 0] + 1.0) * np.cos(5.0 * x[..., 1])
    us = u * s0
    # the stage on (u, us): HO rates, the limited rate of u, then the product block piece by piece
    du_ho, dus_ho = r.mult_unlimited(u, us, T_STAGE)
    du, _ = r.limit_mult(u, None, du_ho, None, DT)
    s, el, dofs = compute_ratio(us, u)
    xe_lo, xe_hi = elem_minmax_masked(s, el, dofs)
    smin, smax = r.bounds_from_extrema(xe_lo, xe_hi)
    u_new = u + DT * du
    el2, dofs2 = compute_bool_indicators(u_new)
    rec = {}

    def clip_scale(us_, m_, dho_, dlo_, lo_, hi_, dt_):  # (the default solver of fct_product, with its inputs kept)
        rec.update(d_us_lo=dlo_.copy(), us_min=lo_.copy(), us_max=hi_.copy())
        return Remhos.clip_scale(us_, m_, dho_, dlo_, lo_, hi_, dt_)

    d_us, smin_out, smax_out = fct_product(us, r.m, dus_ho, smin, smax, u_new, el2, dofs2, DT, fct=clip_scale)
    assert np.array_equal(d_us, fct_product(us, r.m, dus_ho, smin, smax, u_new, el2, dofs2, DT)[0])
    m = r.m
    f = m * (dus_ho - rec["d_us_lo"])
    us_lo = us + DT * rec["d_us_lo"]
    f = np.minimum(m / DT * (rec["us_max"] - us_lo), np.maximum(m / DT * (rec["us_min"] - us_lo), f))
    c = dict(r=r, u=u, us=us, m=m.copy(), dus_ho=dus_ho, s=s, el=el, dofs=dofs, xe_lo=xe_lo, xe_hi=xe_hi, smin=smin, smax=smax,
             u_new=u_new, el2=el2, dofs2=dofs2, d_us=d_us, smin_out=smin_out, smax_out=smax_out, d_us_lo=rec["d_us_lo"],
             new_mass=f.sum(1))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def assert_not_vacuous(c, both_branches=True):
    """the five conditions on the oracle's data without which the comparison would show little (both_branches = False: the
    5 x 5 cases at p >= 2, which are there for the wavefronts past the last element, have no element on the negative
    scaling branch; the 8 x 8 and 16 x 16 cases of every order and the 5 x 5 case at p = 1 meet all five)"""
    for el, dofs in ((c["el"], c["dofs"]), (c["el2"], c["dofs2"])):
        assert (~el).any(), "no empty element"
        assert (el & ~dofs.all(1)).any(), "no element with both active and inactive dofs"
        assert dofs.all(1).any(), "no full element"
    with np.errstate(invalid="ignore"):
        widened = ((c["smin_out"] != c["smin"]) | (c["smax_out"] != c["smax"])).any(1)
    assert widened.any(), "fct_product widens no bound"
    assert (c["new_mass"][c["el2"]] > 1e-15).any(), "the positive scaling branch is not taken"
    assert not both_branches or (c["new_mass"][c["el2"]] < -1e-15).any(), "the negative scaling branch is not taken"


def run_kernels(c, lib, as_dev, to_np, p):
    """the three entry points on the oracle's inputs; every output starts as NaN (flags: 7), so an entry nobody wrote shows"""
    from remhos_amd.capi import Context

    r = c["r"]
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=p, exec_mode=1, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    assert ctx.dim == 2
    ne, nd = c["u"].shape
    nan = lambda *sh: as_dev(np.full(sh, np.nan))  # noqa: E731
    flag = lambda n: as_dev(np.full(n, 7, dtype=np.uint8))  # noqa: E731
    dev = {k: as_dev(np.ascontiguousarray(c[k])) for k in ("u", "us", "m", "dus_ho", "s", "u_new")}
    o = {}
    ctx.setup(T_STAGE)
    for rep in (0, 1):  # twice: the second call must give the same bits
        s, el, dofs = nan(ne, nd), flag(ne), flag(ne * nd)
        ctx.product_ratio(dev["us"], dev["u"], s, el, dofs)
        el_i, dofs_i = flag(ne), flag(ne * nd)
        ctx.product_ratio(None, dev["u_new"], None, el_i, dofs_i)  # the indicator-only call
        xe_lo, xe_hi = nan(ne), nan(ne)
        ctx.elem_minmax_masked(dev["s"], as_dev(c["el"].astype(np.uint8)), as_dev(c["dofs"].astype(np.uint8).ravel()), xe_lo, xe_hi)
        smin, smax = as_dev(c["smin"].copy()), as_dev(c["smax"].copy())
        d_us = nan(ne, nd)
        ctx.fct_product(dev["us"], dev["m"], dev["dus_ho"], smin, smax, dev["u_new"], as_dev(c["el2"].astype(np.uint8)),
                        as_dev(c["dofs2"].astype(np.uint8).ravel()), DT, d_us)
        o[rep] = dict(s=to_np(s).copy(), el=to_np(el).copy(), dofs=to_np(dofs).copy().reshape(ne, nd), el_i=to_np(el_i).copy(),
                      dofs_i=to_np(dofs_i).copy().reshape(ne, nd), xe_lo=to_np(xe_lo).copy(), xe_hi=to_np(xe_hi).copy(),
                      smin=to_np(smin).copy(), smax=to_np(smax).copy(), d_us=to_np(d_us).copy())
    ctx.close()
    return o


def check_kernels(c, o, p, where):
    assert_not_vacuous(c, both_branches=len(c["el"]) != 25 or p == 1)
    a, b = o[0], o[1]
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), ("two calls differ", k)
    # flags, exactly (0 / 1 bytes)
    assert np.array_equal(a["el"], c["el"].astype(np.uint8)) and np.array_equal(a["dofs"], c["dofs"].astype(np.uint8))
    assert np.array_equal(a["el_i"], c["el2"].astype(np.uint8)) and np.array_equal(a["dofs_i"], c["dofs2"].astype(np.uint8))
    err = {}
    err["s"] = np.abs(a["s"] - c["s"]).max() / np.abs(c["s"]).max()
    assert np.array_equal(a["s"][~c["el"]], np.zeros_like(a["s"][~c["el"]]))
    # masked extrema of the oracle's s: the same numbers, +-inf included
    assert np.array_equal(a["xe_lo"], c["xe_lo"]) and np.array_equal(a["xe_hi"], c["xe_hi"])
    assert np.isposinf(a["xe_lo"][~c["el"]]).all() and np.isneginf(a["xe_hi"][~c["el"]]).all()
    for k in ("smin", "smax"):
        ref = c[k + "_out"]
        fin = np.isfinite(ref)
        assert np.array_equal(a[k][~fin], ref[~fin])
        err[k] = np.abs(a[k][fin] - ref[fin]).max() / np.abs(ref[fin]).max()
    scale = np.abs(c["d_us"]).max()
    err["d_us"] = np.abs(a["d_us"] - c["d_us"]).max() / scale
    assert not np.isnan(a["d_us"]).any() and not np.isnan(a["s"]).any()
    assert (a["d_us"][~c["el2"]] == 0.0).all()  # exactly 0 on empty elements
    act = c["el2"]
    lhs = (c["m"] * a["d_us"]).sum(1)[act]
    rhs = (c["m"] * c["d_us_lo"]).sum(1)[act]
    err["cons"] = np.abs(lhs - rhs).max() / np.abs(c["m"] * (c["us"] / DT + c["dus_ho"])).sum(1)[act].max()
    print(where, "p", p, "ne", len(c["el"]), " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    for k in ("s", "smin", "smax", "d_us"):
        assert err[k] <= VEC_TOL, (k, err[k])
    # sum m d_us = sum m d_us_LO per element: as sum m (us + dt d_us) against sum m (us + dt d_us_HO), the 3-D test's form
    assert err["cons"] <= CONS_TOL, err["cons"]
    return err


def oracle_vb_counts(problem, p, ode, dt, steps):
    """The three in-loop checks of -vb (remhos.cpp:1824-1837: LO and limited update of u; remhos_fct.cpp:568-610: the product
    update against the scaled bounds, eps = 1e-12) at every stage of a -ps run of the oracle: dofs out of bounds per check."""
    from oracle.remhos_oracle import check_violation

    r = Remhos(Config(mesh="inline-quad", rs=1, order=p, problem=problem, dt=dt, t_final=0.5, lo=5, fct=2, ps=True, ode=ode, max_steps=steps))
    bad = {"LO u": 0, "FCT u": 0, "FCT us": 0}
    limit_mult = r.limit_mult

    def checked(u, us, du_ho, dus_ho, dt_):
        du_lo = r.calc_lo_massavg(u, du_ho, dt_)
        umin, umax = r.compute_bounds(u)
        du, dus = limit_mult(u, us, du_ho, dus_ho, dt_)
        bad["LO u"] += check_violation(u, umin, umax, dt_, du_lo, 1e-12)["count"]
        bad["FCT u"] += check_violation(u, umin, umax, dt_, du, 1e-12)["count"]
        s, el, dofs = compute_ratio(us, u)
        smin, smax = r.bounds_from_extrema(*elem_minmax_masked(s, el, dofs))
        u_new = u + dt_ * du
        el2, dofs2 = compute_bool_indicators(u_new)
        d_us, smin, smax = fct_product(us, r.m, dus_ho, smin, smax, u_new, el2, dofs2, dt_)
        with np.errstate(invalid="ignore"):  # (inf * 0 on inactive dofs, masked out by active_dofs)
            bad["FCT us"] += check_violation(us, smin, smax, dt_, d_us, 1e-12, scale=u_new, active_dofs=dofs2)["count"]
        return du, dus

    r.limit_mult = checked
    r.run()
    return bad


def oracle_run(p, ode, pa=False, steps=6, ps=True):
    r = Remhos(Config(mesh="inline-quad", rs=1, order=p, problem=14, dt=DT, t_final=0.5, lo=5, fct=2, ps=ps, ode=ode, max_steps=steps,
                      ho_solve="pa" if pa else "exact"))
    r.refine_steps = 2 if p >= 4 else 0
    return r, r.run()


def check_run(lib, p, ode, pa, fused, steps=6):
    """rmhd_run_state with ps = 1 on inline-quad -rs 1 against the oracle: steps, masses to 1e-12, fields to check_rel"""
    from remhos_amd.case import RmhdResult, make_config

    r, out = oracle_run(p, ode, pa, steps)
    cfg = make_config("inline-quad", 1, p, 14, DT, 0.5, max_steps=steps, fused=fused, ps=1, ode_solver=ode, pa=pa)
    res = RmhdResult()
    u, us = np.zeros(r.u.size), np.zeros(r.u.size)
    assert lib.rmhd_run_state(C.byref(cfg), C.byref(res), u.ctypes.data, us.ctypes.data) == 0, lib.rmhd_last_error()
    assert res.steps == out["steps"] == steps and res.stages == {11: 1, 12: 2, 13: 3}[ode] * steps
    em, ems = abs(res.final_mass - out["mass"]) / abs(out["mass"]), abs(res.final_mass_us - out["mass_us"]) / abs(out["mass_us"])
    eu = np.abs(u.reshape(r.u.shape) - r.u).max() / np.abs(r.u).max()
    eus = np.abs(us.reshape(r.u.shape) - r.us).max() / np.abs(r.us).max()
    print(f"run p {p} ode {ode} pa {pa} fused {fused}: mass {em:.2e} mass_us {ems:.2e} u {eu:.2e} us {eus:.2e} s_max {res.s_max} {out['s_max']}")
    assert em <= 1e-12 and ems <= 1e-12
    check_rel(p, eu, f"product2d run u ode {ode}")
    check_rel(p, eus, f"product2d run us ode {ode}")
    assert res.mass_loss_us == abs(res.mass0_us - res.final_mass_us) and res.s_max > 0.0
    # the product block ran: us is not s0 u of the plain run's field
    from remhos_amd.case import Case

    s0 = Case(lib, cfg).s0
    assert np.abs(us.reshape(r.u.shape) - s0 * u.reshape(r.u.shape)).max() > 1e-6
    return res


REFUSALS = [
    (dict(lo_type=4), "-lo 5"),
    (dict(dt_control=1), "Automatic time step is not implemented for product remap."),
    (dict(fct_type=4, fused=0), "fct_type 4"),
    (dict(fct_type=1, fused=0), "fct_type 1"),
    (dict(lo_type=1, fused=0), "lo_type 1"),
    (dict(lo_type=2, fused=0), "lo_type 2"),
    (dict(ho_type=1, fused=0), "ho_type 1"),
]


def check_refusals(lib):
    from remhos_amd.case import RmhdResult, make_config

    for kw, msg in REFUSALS:
        cfg = make_config("inline-quad", 1, 2, 14, DT, 0.5, max_steps=1, ps=1, ode_solver=12, **kw)
        res = RmhdResult()
        assert lib.rmhd_run(C.byref(cfg), C.byref(res)) != 0, kw
        err = lib.rmhd_last_error().decode()
        assert msg in err and ("ps" in err or "product" in err), (kw, err)
    # periodic-square runs transport problems: products exist in remap mode only
    cfg = make_config("periodic-square", 0, 2, 5, DT, 0.1, max_steps=1, ps=1, ode_solver=12)
    res = RmhdResult()
    assert lib.rmhd_run(C.byref(cfg), C.byref(res)) != 0
    assert "Products are processed only in remap mode." in lib.rmhd_last_error().decode()


# ---- CPU: the emulation build ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emulib():
    from remhos_amd.capi import load_library
    from remhos_amd.case import bind_driver
    from tests.helpers import emu_library_path

    return bind_driver(load_library(emu_library_path()))


@pytest.mark.parametrize("p,n", [(1, 8), (2, 8), (3, 8), (6, 8), (1, 5), (2, 5)])
def test_product2d_kernels_emulated(emulib, p, n):
    c = product2d_case(p, n)
    assert len(c["el"]) % 4 == (1 if n == 5 else 0)  # (n = 5: the last workgroup has three wavefronts without an element)
    o = run_kernels(c, emulib, lambda a: np.ascontiguousarray(a).copy(), lambda a: np.asarray(a), p)
    check_kernels(c, o, p, "emu")


@pytest.mark.parametrize("p,ode,pa,fused", [(2, 12, 0, 0), (3, 13, 1, 1)])
def test_product2d_run_emulated(emulib, p, ode, pa, fused):
    """one step under the OS-thread emulation (the six-step runs of every solver are the GPU tests)"""
    check_run(emulib, p, ode, pa, fused, steps=1)


def test_product2d_refusals_emulated(emulib):
    check_refusals(emulib)
