"""MonoRDSolver (-mono 1; remhos_mono.cpp:60-356) under the host emulation: mono_rd_kernel of remhos_amd/csrc/rmh_mono.hpp (rmh_mono_rd)
against the restatement of tests/mono_oracle.py on identical inputs -- a field two steps into a run of the oracle -- with and
without the mass iteration, its conservation and determinism, the driver's -mono 1 path over ten steps and the refusals.
GPU twins: tests/test_gpu_mono.py (the check functions here take the library and a to-device conversion).

Tolerances.  Without mass_lim the kernel is a fixed sequence of sums: 1e-12 relative to max |du|, the project's tolerance for the
element-local kernels.  With mass_lim the map is iterated up to 101 times and its conditioning is the oracle's own: the oracle
runs twice, the second time with u perturbed by 1e-16 relative noise, and the tolerance is 100 x the spread of its two results
(floor 1e-12).  Measured spreads: DESIGN.md section 3.17.  An element may be left out only if an exit residual of the oracle lies
within 1e-8 (1 +- 1e-6) at some pass (the exit decision itself is then at round-off); at most 1 % of the elements."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.helpers import emu_library_path, layout_from_oracle
from tests.mono_oracle import TOL, Config, MonoRemhos

# (mesh, rs, p, problem): the orders whose mass iteration the kernel runs -- every 2-D order, 3-D orders 1 to 3
CASES_ML = [
    ("inline-quad", 1, 1, 14), ("inline-quad", 1, 2, 14), ("inline-quad", 1, 3, 14), ("inline-quad", 1, 6, 14),
    ("periodic-square", 0, 2, 5),  # (rs 0: 3 x 3 elements, the smallest periodic lattice)
    ("cube01_hex", 0, 1, 10), ("cube01_hex", 0, 2, 10), ("cube01_hex", 0, 3, 10), ("periodic-cube", 0, 2, 0),
]
# without the mass iteration every order runs: the remaining 2-D orders and 3-D orders 4 to 6 (MASS = false instantiations)
CASES_NOML = CASES_ML + [("inline-quad", 1, 4, 14), ("inline-quad", 1, 5, 14), ("cube01_hex", 0, 4, 10), ("cube01_hex", 0, 5, 10),
                         ("cube01_hex", 0, 6, 10)]
PERIODIC = ("periodic-square", "periodic-cube")
# under the emulation a pass of an element costs ~20 ms (every butterfly is a rendezvous of 64 OS threads): the second call of
# the bit-identity check is made where the first one took at most this many passes in all; the GPU twins make it everywhere
EMU_SECOND_CALL_PASSES = 300


@pytest.fixture(scope="module")
def lib():
    from remhos_amd.capi import load_library
    from remhos_amd.case import bind_driver

    return bind_driver(load_library(emu_library_path()))


def _dt(mesh):
    return {"inline-quad": 0.002, "periodic-square": 0.002, "cube01_hex": 0.02, "periodic-cube": 0.01}[mesh]


@functools.lru_cache(maxsize=None)
def reference(mesh, rs, p, prob):
    """the oracle two steps into its own -mono 1 run (3-D orders >= 4: stepped without the mass iteration, the only mode the kernel has
    there), and its results on that field: computed once, shared by the CPU and the GPU tests, never modified"""
    r = MonoRemhos(Config(mesh=mesh, rs=rs, order=p, problem=prob, dt=_dt(mesh), t_final=0.7))
    r.mass_lim = not (r.dim == 3 and p >= 4)
    scale = r.mono_scale()
    for _ in range(2):
        r.step(r.dt)
    u, t = r.u.copy(), r.t
    if r.exec_mode == 1:
        r.update_geometry(t)
    noise = 1.0 + 1e-16 * np.sin(1.0 + np.arange(u.size, dtype=np.float64).reshape(u.shape))
    out = {"r": r, "u": u, "t": t, "scale": scale}
    for ml in ((0, 1) if r.mass_lim else (0,)):
        keep = {}
        du = r.calc_mono(u, mass_lim=bool(ml), scale=scale, keep=keep)
        du2 = r.calc_mono(u * noise, mass_lim=bool(ml), scale=scale)
        out[ml] = {"du": du, "keep": keep, "spread": float(np.abs(du2 - du).max() / np.abs(du).max())}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def run_kernel(lib, ref, ml, to_dev=None, t=None, second=True):
    """rmh_mono_rd on the oracle's inputs -> du, a second du (or None), passes [ne], (iters_max, n_not_converged)"""
    from remhos_amd.capi import Context

    dev = to_dev or (lambda a: np.ascontiguousarray(a, dtype=np.float64))
    host = (lambda a: a) if to_dev is None else (lambda a: a.cpu().numpy())
    r, keep = ref["r"], ref[0]["keep"]
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=r.T.p, exec_mode=r.exec_mode, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    ctx.setup(ref["t"] if t is None else t)
    u, lo, hi, sc = dev(ref["u"]), dev(keep["xi_min"]), dev(keep["xi_max"]), dev(ref["scale"])
    du, du2 = dev(np.full_like(ref["u"], np.nan)), dev(np.full_like(ref["u"], np.nan))
    ctx.mono_rd(u, lo, hi, sc, ml, du)
    passes, last = ctx.mono_passes(), ctx.last_mono()
    if second is True or (second == "cheap" and int(np.abs(passes).sum()) <= EMU_SECOND_CALL_PASSES):
        ctx.mono_rd(u, lo, hi, sc, ml, du2)
        assert np.array_equal(ctx.mono_passes(), passes)
        out2 = host(du2)
    else:
        out2 = None
    ctx.close()
    return host(du), out2, passes, last


def check_conservation(ref, ml, du, mesh):
    """sum_i M_L,i du_i over the domain equals the oracle's; on the periodic meshes (no boundary flux) it vanishes"""
    m = ref[ml]["keep"]["m"]
    scale = float(np.abs(m * du).sum())
    got, want = float((m * du).sum()), float((m * ref[ml]["du"]).sum())
    print("sum M_L du:", got, " oracle:", want, " sum |M_L du|:", scale)
    assert abs(got - want) <= 1e-13 * scale
    if mesh in PERIODIC:
        assert abs(got) <= 1e-13 * scale and abs(want) <= 1e-13 * scale


def check_no_mass_lim(lib, mesh, rs, p, prob, to_dev=None, second=True):
    ref = reference(mesh, rs, p, prob)
    du, du2, passes, last = run_kernel(lib, ref, 0, to_dev, second=second)
    want = ref[0]["du"]
    err = float(np.abs(du - want).max() / np.abs(want).max())
    print("mass_lim = 0: max|du - oracle| / max|oracle| =", err, " oracle spread under 1e-16 noise:", ref[0]["spread"])
    assert err <= 1e-12
    assert (passes == 0).all() and last == (0, 0)
    check_conservation(ref, 0, du, mesh)
    if du2 is not None:
        assert np.array_equal(du, du2)


def check_mass_lim(lib, mesh, rs, p, prob, to_dev=None, second=True):
    ref = reference(mesh, rs, p, prob)
    want, keep, spread = ref[1]["du"], ref[1]["keep"], ref[1]["spread"]
    # the oracle alone: elements whose exit decision is at round-off may be left out, at most 1 % of them
    resid = keep["resid"]
    with np.errstate(invalid="ignore"):
        marginal = (np.abs(resid - TOL) <= 1e-6 * TOL).any(axis=1)
    assert marginal.sum() <= 0.01 * marginal.size, (int(marginal.sum()), marginal.size)
    du, du2, passes, last = run_kernel(lib, ref, 1, to_dev, second=second)
    tol = max(100.0 * spread, 1e-12)
    err = float(np.abs(du - want)[~marginal].max() / np.abs(want).max())
    print("mass_lim = 1: max|du - oracle| / max|oracle| =", err, " oracle spread:", spread, " tolerance:", tol,
          " elements left out:", int(marginal.sum()), "of", marginal.size)
    print("passes: oracle min / max", int(keep["passes"].min()), int(keep["passes"].max()), " at the cap without converging:",
          int((~keep["converged"]).sum()), " library:", last)
    assert err <= tol
    assert np.array_equal(np.abs(passes)[~marginal], keep["passes"][~marginal])
    assert np.array_equal((passes < 0)[~marginal], ~keep["converged"][~marginal])
    if not marginal.any():
        assert last == (int(keep["passes"].max()), int((~keep["converged"]).sum()))
        check_conservation(ref, 1, du, mesh)
    assert np.isfinite(du).all()
    print("what the mass iteration changes: max|du - du(mass_lim = 0)| / max|du| =", float(np.abs(du - ref[0]["du"]).max() / np.abs(want).max()))
    if du2 is not None:
        assert np.array_equal(du, du2)


def check_follows_the_moved_mesh(lib, to_dev=None):
    """the same inputs at another pseudo-time give another answer: the geometry of rmh_setup(t) is what the kernel uses"""
    ref = reference("cube01_hex", 0, 2, 10)
    a, _, _, _ = run_kernel(lib, ref, 0, to_dev, second=False)
    b, _, _, _ = run_kernel(lib, ref, 0, to_dev, t=0.5, second=False)
    assert ref["t"] < 0.1
    assert float(np.abs(a - b).max()) > 1e-6 * float(np.abs(a).max())


def check_run_10_steps(lib, rs, p):
    """rmhd_run_state -mono 1 -vb over 10 steps on inline-quad against the oracle stepping RK3 SSP: neither leaves the initial range of
    u by more than 1e-12 (what -vb checks for forced_bounds at every step, remhos.cpp:1219), same mass, same field"""
    from remhos_amd.case import RmhdResult, make_config

    mesh, prob, dt, tf, ms = "inline-quad", 14, 0.004 / (1 + rs), 0.7, 10
    r = MonoRemhos(Config(mesh=mesh, rs=rs, order=p, problem=prob, dt=dt, t_final=tf, max_steps=ms))
    lo, hi = float(r.u.min()), float(r.u.max())
    out = r.run()
    cfg = make_config(mesh, rs, p, prob, dt, tf, max_steps=ms, fused=0, mono_type=1, verify_bounds=1, lo_type=1, fct_type=3)  # (-lo / -fct are ignored)
    res = RmhdResult()
    uf = np.zeros_like(r.u)
    assert lib.rmhd_run_state(C.byref(cfg), C.byref(res), uf.ctypes.data, None) == 0, lib.rmhd_last_error()
    assert res.steps == out["steps"] == ms
    err = float(np.abs(uf - r.u).max())
    print("u range", lo, hi, " oracle", float(r.u.min()), float(r.u.max()), " library", float(uf.min()), float(uf.max()))
    print("mass", res.final_mass, out["mass"], " max |u - oracle|", err, " max |u - u0|", float(np.abs(uf - MonoRemhos(r.cfg).u).max()))
    for v in (r.u, uf):
        assert v.min() >= lo - 1e-12 and v.max() <= hi + 1e-12
    assert abs(res.final_mass - out["mass"]) <= 1e-12 * abs(out["mass"])
    assert err <= 1e-10


@pytest.mark.parametrize("mesh,rs,p,prob", CASES_NOML)
def test_mono_no_mass_lim_vs_oracle(lib, mesh, rs, p, prob):
    # (the second call of the bit-identity check: on the shapes of CASES_ML here, on every shape on the GPU)
    check_no_mass_lim(lib, mesh, rs, p, prob, second=(mesh, rs, p, prob) in CASES_ML)


@pytest.mark.parametrize("mesh,rs,p,prob", CASES_ML)
def test_mono_mass_lim_vs_oracle(lib, mesh, rs, p, prob):
    check_mass_lim(lib, mesh, rs, p, prob, second="cheap")


def test_mono_follows_the_moved_mesh(lib):
    check_follows_the_moved_mesh(lib)


def test_driver_mono_run_10_steps(lib):
    # (the smallest lattice and order: an emulated pass of the mass iteration costs ~20 ms; the GPU twin also runs -rs 1 -o 2)
    check_run_10_steps(lib, 0, 1)


def test_mono_scale_of_the_case_builder():
    """rmhd_case_mono_scale against the oracle's restatement of remhos_mono.cpp:37-57 (both unverified against MFEM itself)"""
    from remhos_amd.case import Case, load_host_library, make_config

    for mesh, rs, p, prob in (("inline-quad", 1, 3, 14), ("periodic-square", 0, 2, 5), ("cube01_hex", 0, 2, 10), ("periodic-cube", 0, 2, 0)):
        want = reference(mesh, rs, p, prob)["scale"]
        got = Case(load_host_library(), make_config(mesh, rs, p, prob, _dt(mesh), 0.7, fused=0)).mono_scale()
        assert want.min() > 0 and np.abs(got - want).max() <= 1e-13 * want.max()


def check_refusals(lib):
    from remhos_amd.case import RmhdResult, make_config

    base = dict(mesh="cube01_hex", rs=0, order=2, problem=10, dt=0.02, t_final=0.7, max_steps=1, fused=0, mono_type=1)

    def refused(call, **kw):
        res = RmhdResult()
        cfg = make_config(**{**base, **kw})
        assert call(cfg, res) != 0
        msg = lib.rmhd_last_error()
        assert msg
        return msg

    run = lambda cfg, res: lib.rmhd_run(C.byref(cfg), C.byref(res))  # noqa: E731
    part = lambda cfg, res: lib.rmhd_run_partitioned(C.byref(cfg), None, 0, C.byref(res))  # noqa: E731
    assert b"-mono 2" in refused(run, mono_type=2)
    assert b"mono_type" in refused(run, mono_type=3)
    assert b"-mono 1" in refused(run, fused=1) and b"fused" in refused(run, fused=1)
    assert b"-mono 1" in refused(run, ps=1, ode_solver=11) and b"ps" in refused(run, ps=1, ode_solver=11)
    assert b"partitioned" in refused(part, part=(2, 1, 1)) and b"-mono 1" in refused(part, part=(2, 1, 1))
    assert b"partitioned" in refused(run, part=(2, 1, 1))
    assert b"partitioned" in refused(part)
    msg = refused(run, order=4)  # 3-D p = 4: the mass iteration needs the element's M in the LDS
    assert b"-mono 1" in msg and b"order 4" in msg
    # mono_type = 0 leaves the other refusals as they are
    assert b"fct" in refused(run, mono_type=0, fct_type=3)


def test_driver_mono_refusals(lib):
    check_refusals(lib)


def test_mono_rd_contract(lib):
    """null arguments, a context with a ghost, 3-D p = 4 with mass_lim, rmh_last_mono before any call"""
    from remhos_amd.capi import Context, RmhError

    ref = reference("cube01_hex", 0, 2, 10)
    r, keep = ref["r"], ref[0]["keep"]
    x0, vel, nbr, st = layout_from_oracle(r)
    ctx = Context(lib, order=2, exec_mode=1, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    with pytest.raises(RmhError, match="no rmh_mono_rd call"):
        ctx.last_mono()
    with pytest.raises(RmhError, match="no rmh_mono_rd call"):
        ctx.mono_passes()
    u, du = np.array(ref["u"]), np.zeros_like(ref["u"])
    args = [u, np.array(keep["xi_min"]), np.array(keep["xi_max"]), np.array(ref["scale"]), 1, du]
    for k in (0, 1, 2, 3, 5):
        bad = list(args)
        bad[k] = None
        with pytest.raises(RmhError, match="null argument"):
            ctx.mono_rd(*bad)
    assert lib.rmh_mono_rd(None, u.ctypes.data, u.ctypes.data, u.ctypes.data, u.ctypes.data, 1, du.ctypes.data) != 0
    n, bad_n = C.c_int(), C.c_longlong()
    assert lib.rmh_last_mono(ctx.h, None, C.byref(bad_n)) != 0 and lib.rmh_last_mono(ctx.h, C.byref(n), None) != 0
    assert lib.rmh_mono_passes(ctx.h, None) != 0
    ctx.close()
    # a context with a ghost element (one block only)
    from remhos_amd.case import Case, make_config

    c = Case(lib, make_config("cube01_hex", 1, 1, 10, -1.0, 0.5, part=(2, 1, 1), rank=0))
    assert c.ne_ghost > 0
    ctx = Context(lib, order=1, exec_mode=c.exec_mode, x0=c.x0, vel=c.vel, face_nbr=c.face_nbr, stencil27=c.stencil27, ne_ghost=c.ne_ghost)
    ug = np.ascontiguousarray(c.u0, dtype=np.float64)
    with pytest.raises(RmhError, match="-mono 1.*ghost"):
        ctx.mono_rd(ug, ug, ug, np.ones(c.ne_owned), 1, np.zeros_like(ug))
    ctx.close()
    # 3-D order 4: refused with mass_lim, naming the option and the order; runs without
    ref4 = reference("cube01_hex", 0, 4, 10)
    r4, keep4 = ref4["r"], ref4[0]["keep"]
    x0, vel, nbr, st = layout_from_oracle(r4)
    ctx = Context(lib, order=4, exec_mode=1, x0=x0, vel=vel, face_nbr=nbr, stencil27=st)
    a4 = [np.array(ref4["u"]), np.array(keep4["xi_min"]), np.array(keep4["xi_max"]), np.array(ref4["scale"]), 1, np.zeros_like(ref4["u"])]
    with pytest.raises(RmhError, match="-mono 1.*order 4"):
        ctx.mono_rd(*a4)
    with pytest.raises(RmhError, match="no rmh_mono_rd call"):
        ctx.last_mono()
    ctx.close()
