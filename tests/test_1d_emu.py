"""dim = 1 through the C ABI (rmh_layout.dim = 1, remhos_amd/csrc/rmh_1d.hpp), the case builder and the driver: segment lattices
against the oracle -- stage by stage for every entry point, and whole runs through rmhd_run_state.

CPU: the g++ emulation build of the same kernel sources.  tests/test_gpu_1d.py runs the same functions on the device.  All
inputs come from the oracle (tests/oracle_1d.py: the 1 x 1 wrappers of det / adjugate); the oracle itself is pinned in one
dimension by the reference's own printed answers (tests/golden/reference_kat_1d.json).

Tolerances.  Lumped mass, LO rates and the limited rate: 1e-12 of the vector's max norm (the project's tolerance for the
limiter and streaming kernels); the limiter is checked on the library's own du_HO, so that the cond-limited error of the mass
solve -- held to helpers.check_rel -- does not enter.  Element extrema and bounds: equal.  Conservation per element: 1e-13 of
sum |m du| (see check_stage for the one situation in which the oracle's own arithmetic on the same inputs sets the bound).
Measured worst values over all cases of this file on the emulation (report() prints them; DESIGN.md section 3.18 has the
device's beside them): du_HO 6.1e-15 (p 1), 1.7e-14, 3.4e-14, 1.4e-14, 3.7e-14, 6.6e-14 (p 6); lumped mass 2.3e-14; LO rates
1.3e-14; limited rate against the oracle's clip_scale on the same inputs 0 (bit for bit); fused limiter and one-kernel stage
against the granular sequence 0; conservation 7.6e-14 of sum |m du| but for p = 1 on the moving 3-ring, 2.8e-13, which is the
oracle's clip_scale on the same inputs bit for bit; whole runs 1.6e-14.
"""
import json
import os

import numpy as np
import pytest

from oracle.remhos_oracle import Remhos, check_violation
from tests import oracle_1d as o1
from tests.helpers import check_rel, emu_library_path, perturbed

KAT1 = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_kat_1d.json")))

T_STAGE, DT_STAGE = 0.3, 0.002
# (name, n, periodic, graded): n = 65 puts one lane into a second wavefront, n = 3 is the smallest ring with distinct neighbours
LATTICES = [("per32", 32, True, False), ("graded7", 7, False, True), ("per65", 65, True, False), ("per3", 3, True, False)]
# p = 1 on the uniform 3-ring: six dofs, every element in every stencil -- the HO update stays inside the global bounds and the
# limiter is idle (max |du - du_HO| = 5e-15 max |du| in the oracle), which condition 3 does not allow.  That order takes the ring
# with the vertices below, where the bump sits in the two short segments and the limiter acts (0.5 / 0.6 max |du|, fixed / moving).
PER3_P1 = ("per3", 3, True, (0.0, 0.7, 0.9, 1.0))
STAGE_CASES = [(p, lo, mv) for p in range(1, 7) for lo in (3, 4, 5) for mv in (False, True) if p >= 2 or lo == 5]
MEASURED = {}  # quantity -> worst value seen this session (printed by report())


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _note(key, v):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(v))


class Backend:
    """numpy arrays for the emulation library, torch CUDA tensors for the device library"""

    def __init__(self, gpu):
        self.gpu = gpu
        from remhos_amd.capi import load_library
        from remhos_amd.case import bind_driver

        if gpu:
            import torch

            assert torch.cuda.is_available()
            self.torch = torch
            self.lib = bind_driver(load_library())
        else:
            self.lib = bind_driver(load_library(emu_library_path()))

    def arr(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return self.torch.from_numpy(a).cuda() if self.gpu else a.copy()

    def nan(self, shape):
        return self.arr(np.full(shape, np.nan))

    def host(self, a):
        return a.cpu().numpy() if self.gpu else a

    def context(self, r):
        from remhos_amd.capi import Context

        x0, vel, nbr, st, sub = o1.layout_1d(r)
        ctx = Context(self.lib, order=r.T.p, exec_mode=r.exec_mode, x0=x0, vel=vel, face_nbr=nbr, stencil27=st, subcell_vel=sub)
        assert ctx.dim == 1 and ctx.ndof == r.T.p + 1
        if self.gpu:
            ctx.set_stream(self.torch.cuda.current_stream().cuda_stream)
        if r.cfg.lo in (3, 4):
            ctx.set_lo_type(r.cfg.lo)
        return ctx


@pytest.fixture(scope="module")
def emu():
    yield Backend(False)
    report()


def report():
    """the worst values measured by the tests of a module, for DESIGN.md (shown with pytest -s)"""
    for k in sorted(MEASURED):
        print(f"measured 1d {k}: {MEASURED[k]:.3e}")


# ---- 1. the checker: the oracle reproduces the reference's three printed 1-D answers ---------------------------------------
@pytest.mark.parametrize("case", KAT1["cases"], ids=[c["name"] for c in KAT1["cases"]])
def test_oracle_reference_answers(case):
    """autotest/out_baseline.dat, 'Transport per-1D': 1000 steps of dt = 0.001 on 32 segments at order 3.  -ho 2 and -pa give the
    answer of the exact inverse (the reference disables PA in 1-D, remhos.cpp:474-480)."""
    c = KAT1["common"]
    with o1.patched():
        r = o1.make(o1.segment_lattice(c["rs"]), c["order"], case["lo"], dt=c["dt"], t_final=c["t_final"])
        rep = r.run()
    assert rep["steps"] == 1000
    assert float(f"{rep['mass']:.10g}") == case["final_mass"]
    assert float(f"{rep['max']:.10g}") == case["max_value"]


# ---- 2. + 3. one stage, every entry point ---------------------------------------------------------------------------------
def twice(bk, call, *shapes):
    """run call(*outputs) twice on outputs that start as NaN; the two results must be the same bits, and every entry written"""
    res = []
    for _ in range(2):
        outs = [bk.nan(s) for s in shapes]
        call(*outs)
        res.append([np.array(bk.host(o)) for o in outs])
    for a, b in zip(*res):
        assert np.isfinite(a).all(), "an element was left out"
        assert a.tobytes() == b.tobytes(), "two calls, different bits"
    return res[0] if len(shapes) > 1 else res[0][0]


def check_stage(bk, p, lo, mv, lattice):
    name, n, periodic, graded = lattice
    where = f"1d p{p} lo{lo} {'moving' if mv else 'fixed'} {name}"
    t, dt = T_STAGE, DT_STAGE
    with o1.patched():
        r = o1.make(o1.lattice_1d(n, periodic, graded), p, lo)
        if mv:
            o1.moving(r, lo)
        r.refine_steps = 2
        uh = perturbed(r.u)
        keep = {}
        r.stage(uh, t, dt, keep)
        m_o = keep["m"]
        # ---- conditions on the oracle's data: the test is not vacuous
        assert np.abs(keep["du"] - keep["du_ho"]).max() > 1e-6 * np.abs(keep["du"]).max(), (where, "the limiter does not act")
        if name == "per32" and p == 3:
            u_new = uh + dt * keep["du"]
            assert (np.abs(u_new - keep["umax"]) <= 1e-14).any() and (np.abs(u_new - keep["umin"]) <= 1e-14).any(), where
        ctx = bk.context(r)
        u = bk.arr(uh)
        sh, she = uh.shape, (r.lat.ne,)
        ctx.setup(t)
        # HO: du_HO, and the lumped mass and element extrema it leaves
        du_ho = twice(bk, lambda o: ctx.ho_apply(u, o), sh)
        check_rel(p, _rel(du_ho, keep["du_ho"]), where + " du_ho")
        _note(f"du_ho p{p}", _rel(du_ho, keep["du_ho"]))
        m = twice(bk, lambda o: ctx.compute_lumped_mass(t, o), sh)
        assert _rel(m, m_o) <= 1e-12, where
        _note("m", _rel(m, m_o))
        d_ho, d_m = bk.arr(du_ho), bk.arr(m)
        # LO
        if lo == 5:
            du_lo = twice(bk, lambda o: ctx.lo_massavg(u, d_ho, dt, o), sh)
            lo_o = r.calc_lo_massavg(uh, du_ho, dt)  # (on the library's du_HO)
        else:
            du_lo = twice(bk, lambda o: (ctx.lo_rdsubcell if lo == 4 else ctx.lo_rd)(u, o), sh)
            lo_o = keep["du_lo"]
        assert _rel(du_lo, lo_o) <= 1e-12, (where, _rel(du_lo, lo_o))
        _note("du_lo", _rel(du_lo, lo_o))
        d_lo = bk.arr(du_lo)
        # extrema and bounds, both bounds types
        xmn, xmx = twice(bk, lambda a, b: ctx.elem_minmax(u, a, b), she, she)
        assert np.array_equal(xmn, uh.min(axis=1)) and np.array_equal(xmx, uh.max(axis=1)), where
        d_mn, d_mx = bk.arr(xmn), bk.arr(xmx)
        bounds = {}
        for bt in (1, 0):
            ctx.set_bounds_type(bt)
            r.cfg.bounds_type = bt
            umin, umax = twice(bk, lambda a, b: ctx.bounds(d_mn, d_mx, a, b), sh, sh)
            bmin, bmax = r.bounds_from_extrema(uh.min(-1), uh.max(-1))
            assert np.array_equal(umin, bmin) and np.array_equal(umax, bmax), (where, bt)
            bounds[bt] = (umin, umax)
        umin, umax = bounds[0]
        assert np.array_equal(umin, keep["umin"]) and np.array_equal(umax, keep["umax"])
        d_min, d_max = bk.arr(umin), bk.arr(umax)
        # clip + scale on the library's own rates and lumped mass (each held to its own tolerance above: on the moving meshes the
        # fluxes m (du_HO - du_LO) are 1e3 to 1e4 times the rate they leave, and so is every relative difference of an input)
        du = twice(bk, lambda o: ctx.fct_clipscale(u, d_m, d_ho, d_lo, d_min, d_max, dt, o), sh)
        du_o = Remhos.clip_scale(uh, m, du_ho, du_lo, umin, umax, dt)
        assert _rel(du, du_o) <= 1e-12, (where, _rel(du, du_o))
        _note("du", _rel(du, du_o))
        check_rel(p, _rel(du, keep["du"]), where + " du")
        # per element: sum m du = sum m du_LO to 1e-13 of sum |m du| (over the rank's dofs, like the max norms above).  On its own
        # stage data the oracle meets this in every case (8.2e-14 at worst).  The figure is a property of the INPUTS under the
        # reference's arithmetic, though: on the moving meshes the fluxes are 1e3 times the rate they add up to, and the oracle's
        # clip_scale on the library's du_HO / du_LO / m (equal to its own to 1e-14) -- with which the kernel agrees bit for bit --
        # leaves 2.8e-13 at p = 1 on the 3-ring here (emulation) and 1.04e-13 at p = 2 on the device.  Only where that reference
        # arithmetic on the SAME inputs (du_o) misses 1e-13 for an element is the kernel held to twice the oracle's own defect there.
        defect = np.abs((m * du).sum(-1) - (m * du_lo).sum(-1)) / np.abs(m * du).sum()
        defect_o = np.abs((m * du_o).sum(-1) - (m * du_lo).sum(-1)) / np.abs(m * du_o).sum()
        _note("conservation / sum |m du|", defect.max())
        _note("conservation, the oracle's clip_scale on the same inputs", defect_o.max())
        assert mv or (defect_o <= 1e-13).all(), (where, defect_o)  # (the fixed meshes never need it)
        assert defect.shape == she and (defect <= np.where(defect_o > 1e-13, 2.0 * defect_o, 1e-13)).all(), (where, defect, defect_o)
        v = ctx.check_violation(u, d_min, d_max, dt=dt, du=bk.arr(du))
        assert v["count"] == check_violation(uh, umin, umax, dt=dt, du=du)["count"] == 0, where
        # fused limiter (after rmh_ho_apply on the same u) and the one-kernel stage, with the RK update
        ctx.ho_apply(u, d_ho)
        if lo == 5:
            duf, yf = twice(bk, lambda a, b: ctx.limit_fused(u, d_ho, dt, du=a, x_base=u, a=0.75, b=0.25, dt_rk=dt, y_out=b), sh, sh)
        else:
            duf, yf = twice(bk, lambda a, b: ctx.limit_fused_lo(u, d_ho, d_lo, dt, du=a, x_base=u, a=0.75, b=0.25, dt_rk=dt, y_out=b), sh, sh)
        dus, ys = twice(bk, lambda a, b: ctx.stage_fused(u, dt, b, x_base=u, a=0.75, b=0.25, dt_rk=dt, du=a), sh, sh)
        for tag, d, y in (("limit_fused", duf, yf), ("stage_fused", dus, ys)):
            assert _rel(d, du) <= 1e-12, (where, tag, _rel(d, du))
            assert _rel(y, 0.75 * uh + 0.25 * (uh + dt * du)) <= 1e-12, (where, tag)
            _note(tag, _rel(d, du))
        y1 = twice(bk, lambda o: ctx.stage_fused(u, dt, o, dt_rk=dt), sh)  # (no x_base, no du)
        assert _rel(y1, uh + dt * du) <= 1e-12, where
        # the stage leaves the lumped mass and the element extrema of ITS u at ITS time in the context: after an HO call on another
        # field at another time, then the stage, the fused limiter must give the limited rate of u
        ctx.setup(t + 0.1)
        ctx.ho_apply(bk.arr(2.0 * uh + 1.0), bk.nan(sh))
        ctx.setup(t)
        ctx.stage_fused(u, dt, bk.nan(sh), dt_rk=dt)
        if lo == 5:
            dua = twice(bk, lambda o: ctx.limit_fused(u, d_ho, dt, du=o), sh)
        else:
            dua = twice(bk, lambda o: ctx.limit_fused_lo(u, d_ho, d_lo, dt, du=o), sh)
        assert _rel(dua, du) <= 1e-12, (where, "limiter on the stage's lumped mass and extrema", _rel(dua, du))
        # -dtc 1: the limiter's time-step estimate, bounds type 1
        ctx.set_bounds_type(1)
        ctx.set_dt_control(True)
        est = []
        for _ in range(2):
            ctx.dt_estimate_reset()
            ctx.stage_fused(u, dt, bk.nan(sh), dt_rk=dt)
            est.append(ctx.dt_estimate_get())
        b1min, b1max = bounds[1]
        with np.errstate(divide="ignore", invalid="ignore"):
            cand = np.where(du_lo > 1e-12, (b1max - uh) / du_lo, np.where(du_lo < -1e-12, (b1min - uh) / du_lo, np.inf))
        assert est[0] == est[1] and abs(est[0] - cand.min()) <= 1e-9 * abs(cand.min()), (where, est, cand.min())
        ctx.set_dt_control(False)
        ctx.set_bounds_type(0)
        # stopwatches
        ctx.enable_timers(True)
        ctx.reset_timers()
        ctx.stage_fused(u, dt, bk.nan(sh), dt_rk=dt)
        tm = ctx.timers()
        assert len(tm) == 4 and all(np.isfinite(x) and x >= 0.0 for x in tm)
        assert ctx.last_cg_iters() == 0  # (the mass solve of a segment is direct)
        ctx.close()


@pytest.mark.parametrize("p,lo,mv", STAGE_CASES, ids=[f"p{p}-lo{lo}-{'moving' if mv else 'fixed'}" for p, lo, mv in STAGE_CASES])
def test_stage_parity(emu, p, lo, mv):
    for lattice in LATTICES:
        check_stage(emu, p, lo, mv, PER3_P1 if (p == 1 and lattice[0] == "per3") else lattice)


def check_rd_order_conditions(bk):
    """the RD entries under the order conditions and messages of the other dimensions"""
    from remhos_amd.capi import RmhError

    with o1.patched():
        r = o1.make(o1.lattice_1d(3, True, False), 1, 5)
    ctx = bk.context(r)
    u, out = bk.arr(r.u), bk.nan(r.u.shape)
    with pytest.raises(RmhError, match="orders >= 2"):
        ctx.lo_rd(u, out)
    with pytest.raises(RmhError, match="Subcell schemes require"):
        ctx.lo_rdsubcell(u, out)
    with pytest.raises(RmhError, match="lo 3"):
        ctx.set_lo_type(3)
    with pytest.raises(RmhError, match="must follow rmh_ho_apply"):
        ctx.limit_fused(u, u, 0.01, du=out)
    ctx.close()


def test_rd_order_conditions(emu):
    check_rd_order_conditions(emu)


# ---- 4. whole runs through the driver ------------------------------------------------------------------------------------
RUNS = [
    dict(order=3, lo_type=4, fused=1, dt=0.001, max_steps=20, t_final=1.0),
    dict(order=2, lo_type=3, fused=0, dt=0.001, max_steps=20, t_final=1.0),
    dict(order=3, lo_type=5, fused=1, dt=0.001, max_steps=20, t_final=1.0, bounds_type=1),
    # the CFL rule's step 0.25 h / |v| (13 steps to t = 0.1) at orders 1 to 3.  Not p = 3 with lo 5: that run is ill-conditioned in the
    # oracle itself -- a 1e-15 relative perturbation of its initial field comes out as 1.0e-11 after the 13 steps (2e-15 with lo 4,
    # 3e-14 at p = 2), and the library, which differs by 1e-14 per stage, as 1.1e-10 -- above the 2e-11 of check_rel at p = 3
    dict(order=1, lo_type=5, fused=1, dt=-1.0, max_steps=-1, t_final=0.1),
    dict(order=2, lo_type=5, fused=1, dt=-1.0, max_steps=-1, t_final=0.1),
    dict(order=2, lo_type=3, fused=0, dt=-1.0, max_steps=-1, t_final=0.1),
    dict(order=3, lo_type=4, fused=1, dt=-1.0, max_steps=-1, t_final=0.1),
]
RUN_IDS = ["p3-lo4-fused", "p2-lo3-granular", "p3-lo5-bt1", "p1-lo5-cfl", "p2-lo5-cfl", "p2-lo3-cfl-granular", "p3-lo4-cfl"]


def run_driver(bk, expect_rc=0, **kw):
    from remhos_amd.case import RmhdResult, make_config
    import ctypes as C

    kw.setdefault("rs", 3)
    kw.setdefault("problem", 0)
    cfg = make_config(mesh="periodic-segment", **kw)
    res = RmhdResult()
    ne = 4 << kw["rs"]
    u = np.full((ne, kw.get("order", 3) + 1), np.nan)
    rc = bk.lib.rmhd_run_state(C.byref(cfg), C.byref(res), u.ctypes.data, None)
    assert (rc == 0) == (expect_rc == 0), bk.lib.rmhd_last_error().decode()
    return res, u, bk.lib.rmhd_last_error().decode()


def check_run(bk, kw):
    p = kw["order"]
    with o1.patched():
        r = o1.make(o1.segment_lattice(3), p, kw["lo_type"], bounds_type=kw.get("bounds_type", 0), dt=kw["dt"], t_final=kw["t_final"],
                    max_steps=kw["max_steps"])
        cfl = r._cfl_dt()
        rep = r.run()
        errs = r.lp_errors()
    res, u, _ = run_driver(bk, **kw)
    where = f"1d run {kw}"
    assert res.steps == rep["steps"] == (20 if kw["dt"] > 0 else 13), where
    assert res.dt == (kw["dt"] if kw["dt"] > 0 else cfl), (where, res.dt, cfl)
    assert abs(res.final_mass - rep["mass"]) <= 1e-12 * abs(rep["mass"]), where
    assert abs(res.mass0 - rep["mass0"]) <= 1e-12 * abs(rep["mass0"]), where
    assert np.isfinite(u).all()
    check_rel(p, _rel(u, r.u), where)
    _note("run field", _rel(u, r.u))
    assert res.has_errors == 1
    for got, ref in zip((res.err_l1, res.err_l2, res.err_linf), errs):
        assert abs(got - ref) <= 1e-10 * abs(ref), (where, got, ref)


@pytest.mark.parametrize("kw", RUNS, ids=RUN_IDS)
def test_runs_against_oracle(emu, kw):
    check_run(emu, kw)


def test_run_verify_bounds_and_dt_control(emu):
    """-vb and -dtc 1 -bt 1 run through; -vb changes nothing"""
    base = dict(order=3, lo_type=4, fused=1, dt=0.001, max_steps=5, t_final=1.0)
    a, ua, _ = run_driver(emu, **base)
    b, ub, _ = run_driver(emu, verify_bounds=1, **base)
    assert ua.tobytes() == ub.tobytes() and a.final_mass == b.final_mass
    c, uc, _ = run_driver(emu, order=3, lo_type=5, fused=1, dt=0.002, max_steps=5, t_final=1.0, bounds_type=1, dt_control=1)
    assert c.steps >= 1 and np.isfinite(uc).all() and abs(c.final_mass - c.mass0) <= 1e-12


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
REFUSED_OPTIONS = [
    ("ps", dict(ps=1, ode_solver=13)), ("ode_solver", dict(ode_solver=11)), ("ode_solver", dict(ode_solver=12)),
    ("ode_solver", dict(ode_solver=13)), ("ho_type 1", dict(ho_type=1, fused=0)), ("lo_type", dict(lo_type=1, fused=0)),
    ("lo_type", dict(lo_type=2, fused=0)), ("fct_type", dict(fct_type=1, fused=0)), ("fct_type", dict(fct_type=4, fused=0)),
    ("mono_type", dict(mono_type=1, fused=0)), ("partitions", dict(part=(2, 1, 1))), ("self_wrap", dict(self_wrap=1)),
    ("save", dict(save=1)), ("problem", dict(problem=1)), ("problem", dict(problem=10)),
]


def check_refused_options(bk):
    for name, kw in REFUSED_OPTIONS:
        args = dict(order=3, lo_type=5, dt=0.001, max_steps=1, t_final=1.0)
        args.update(kw)
        _, _, msg = run_driver(bk, expect_rc=-1, **args)
        assert "dim = 1" in msg and name.split()[0] in msg, (name, msg)


def check_refused_entries(bk):
    from remhos_amd.capi import RmhError

    with o1.patched():
        r = o1.make(o1.lattice_1d(7, False, True), 2, 5)
    ctx = bk.context(r)
    sh = r.u.shape
    u, o = bk.arr(r.u), bk.nan(sh)
    z = lambda: bk.arr(np.zeros(sh))  # noqa: E731
    flags = np.zeros(r.u.size + r.lat.ne, dtype=np.uint8)
    fl = bk.torch.from_numpy(flags).cuda() if bk.gpu else flags
    calls = {
        "rmh_ho_neumann": lambda: ctx.ho_neumann(u, o),
        "rmh_lo_upwind": lambda: ctx.lo_upwind(u, o),
        "rmh_lo_upwind_prec": lambda: ctx.lo_upwind_prec(u, o),
        "rmh_fct_projection": lambda: ctx.fct_projection(u, z(), z(), z(), z(), z(), 0.01, o),
        "rmh_fct_fluxbased": lambda: ctx.fct_fluxbased(u, z(), z(), z(), z(), z(), 0.01, o),
        "rmh_mono_rd": lambda: ctx.mono_rd(u, z(), z(), bk.arr(np.ones(r.lat.ne)), 1, o),
        "rmh_product_ratio": lambda: ctx.product_ratio(u, u, o, fl, fl),
        "rmh_elem_minmax_masked": lambda: ctx.elem_minmax_masked(u, fl, fl, o, o),
        "rmh_fct_product": lambda: ctx.fct_product(u, z(), z(), z(), z(), z(), fl, fl, 0.01, o),
        "rmh_stage_fused_range": lambda: ctx.stage_fused_range(u, 0.01, o, 0, 3, True),
        "rmh_batch_order": lambda: ctx.batch_order(7),
        "rmh_halo_pack": lambda: ctx.halo_pack(u, fl, 1, o, o, o),
        "rmh_halo_pack_records": lambda: ctx.halo_pack_records(u, fl, 1, o),
        "rmh_exchange_setup": lambda: ctx.exchange_setup([(0, np.zeros(1, np.int32), np.zeros(1, np.int32))]),
    }
    for name, call in calls.items():
        with pytest.raises(RmhError) as ei:
            call()
        assert "dim = 1" in str(ei.value) and name in str(ei.value) and "rmh error -1" in str(ei.value), (name, str(ei.value))
    # accepted, without effect at dim = 1: the mass-solve controls
    a = bk.nan(sh)
    ctx.setup(0.0)
    ctx.ho_apply(u, a)
    ctx.set_mass_tol(0.0, 1e-2, 1)
    ctx.set_mass_completion(True, True)
    ctx.ho_apply(u, o)
    assert np.array(bk.host(a)).tobytes() == np.array(bk.host(o)).tobytes()
    ctx.close()
    # ghosts and out-of-range tables are refused at creation
    from remhos_amd.capi import Context

    x0, vel, nbr, st, _ = o1.layout_1d(r)
    with pytest.raises(RmhError, match="dim = 1"):
        Context(bk.lib, order=2, exec_mode=0, x0=x0, vel=vel, face_nbr=nbr, stencil27=st, ne_ghost=1)
    bad = st.copy()
    bad[3, 1] = 2
    with pytest.raises(RmhError, match="centre entry"):
        Context(bk.lib, order=2, exec_mode=0, x0=x0, vel=vel, face_nbr=nbr, stencil27=bad)
    bad = st.copy()
    bad[3, 2] = 7
    with pytest.raises(RmhError, match="out of range"):
        Context(bk.lib, order=2, exec_mode=0, x0=x0, vel=vel, face_nbr=nbr, stencil27=bad)


def test_refused_options(emu):
    check_refused_options(emu)


def test_refused_entries(emu):
    check_refused_entries(emu)


def check_pa_is_ignored(bk, capfd):
    base = dict(order=3, lo_type=4, fused=1, dt=0.001, max_steps=3, t_final=1.0)
    a, ua, _ = run_driver(bk, pa=0, **base)
    capfd.readouterr()
    b, ub, _ = run_driver(bk, pa=1, **base)
    assert "Disabling PA / FA for 1D." in capfd.readouterr().out
    assert ua.tobytes() == ub.tobytes() and a.final_mass == b.final_mass and a.max_value == b.max_value


def test_pa_is_ignored(emu, capfd):
    check_pa_is_ignored(emu, capfd)


def test_case_builder_1d():
    """the host case builder (no kernels): periodic-segment against the oracle's arrays"""
    from remhos_amd.case import Case, load_host_library, make_config

    lib = load_host_library()
    for p, lo in ((3, 4), (1, 5), (6, 3)):
        c = Case(lib, make_config(mesh="periodic-segment", rs=3, order=p, problem=0, dt=-1.0, t_final=1.0, lo_type=lo))
        with o1.patched():
            r = o1.make(o1.segment_lattice(3), p, lo)
            cfl = r._cfl_dt()
        x0, vel, nbr, st, sub = o1.layout_1d(r)
        assert c.dim == 1 and c.ndof == p + 1 and c.exec_mode == 0
        assert np.array_equal(c.x0, x0) and np.array_equal(c.vel, vel)
        assert np.array_equal(c.face_nbr, nbr) and np.array_equal(c.stencil27, st)
        assert np.abs(c.u0 - r.u).max() <= 1e-14  # (|d u0 / dX| <= 5.4, X to 2 ulp, exp to 1 ulp)
        assert c.dt == cfl
        if lo == 4:
            assert np.array_equal(c.subcell_vel, sub)
    with pytest.raises(RuntimeError, match="dim = 1"):
        Case(lib, make_config(mesh="periodic-segment", rs=3, order=3, problem=1, lo_type=5))
