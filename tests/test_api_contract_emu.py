"""The contract of the C-ABI entry points that their host-side plumbing has to keep (remhos_amd/csrc/rmh_api.hip), under the host
emulation and through the ABI alone (lib.rmh_*: return code and rmh_last_error):

  * which refusal wins where two conditions hold at once (the order of the null / argument / state checks of an entry point),
  * the state a failing or succeeding call leaves behind (the extrema token, the LO type, the batch order), seen through what the
    next call computes,
  * that every entry point that dispatches on (order, dimension) reaches the kernel of its dimension: called on a 2-D and on a
    3-D case, twice, bit for bit.

Numerical parity with the oracle is the business of tests/test_emu_cpu.py, test_2d.py, test_efp_emu.py and their like."""
import ctypes as C

import numpy as np
import pytest

from oracle.remhos_oracle import Config, Remhos
from tests.helpers import emu_library_path, layout_from_oracle, perturbed

OK, INVALID, STATE = 0, -1, -5  # include/rmh.h
DT = {3: 0.02, 2: 0.004}
T = 0.3


@pytest.fixture(scope="module")
def lib():
    from remhos_amd.capi import load_library

    return load_library(emu_library_path())


@pytest.fixture(scope="module")
def cases():
    """dim -> (layout arrays, sub-mesh velocity, u) of the smallest order-2 remap case: cube01_hex at rs 0 (8 hexahedra),
    inline-quad at rs 1 (64 quadrilaterals)"""
    out = {}
    for dim, (mesh, rs, prob) in {3: ("cube01_hex", 0, 10), 2: ("inline-quad", 1, 14)}.items():
        r = Remhos(Config(mesh=mesh, rs=rs, order=2, problem=prob, dt=DT[dim], t_final=0.7, lo=4))
        assert r.exec_mode == 1 and r.dim == dim
        out[dim] = (layout_from_oracle(r), np.ascontiguousarray(r.Vs.transpose(0, 2, 1)), perturbed(r.u))
    return out


def context(lib, cases, dim, order=2, subcell=True, ne_ghost=0):
    """(the mesh nodes are those of the Q2 mesh at every order; the sub-mesh velocity is the order-2 one)"""
    from remhos_amd.capi import Context

    (x0, vel, nbr, st), sub, _ = cases[dim]
    ctx = Context(lib, order=order, exec_mode=1, x0=x0, vel=vel, face_nbr=nbr, stencil27=st, ne_ghost=ne_ghost,
                  subcell_vel=sub if subcell and order == 2 else None)
    ctx.setup(T)
    return ctx


def ptr(a):
    return None if a is None else a.ctypes.data


def refused(lib, rc, code, text):
    msg = lib.rmh_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


# ---- precedence of refusals -----------------------------------------------------------------------------------------------------

def test_null_argument_before_state(lib, cases):
    u = cases[3][2]
    a, b = np.zeros_like(u), np.zeros_like(u)
    ctx = context(lib, cases, 3)  # no rmh_ho_apply yet: every rmh_lo_massavg is refused
    refused(lib, lib.rmh_lo_massavg(ctx.h, ptr(u), None, 0.02, ptr(b)), INVALID, "null argument")
    refused(lib, lib.rmh_lo_massavg(ctx.h, ptr(u), ptr(a), 0.02, ptr(b)), STATE, "rmh_lo_massavg needs the lumped mass of rmh_ho_apply")
    # the fused limiter in front of rmh_ho_apply: null argument, then the call order, then (a context with a ghost) its ghost data
    refused(lib, lib.rmh_limit_fused(ctx.h, ptr(u), None, 0.02, ptr(a), None, 0.0, 1.0, 0.0, None), INVALID, "null argument")
    refused(lib, lib.rmh_limit_fused(ctx.h, ptr(u), ptr(a), 0.02, None, None, 0.0, 1.0, 0.0, None), INVALID, "null argument")
    refused(lib, lib.rmh_limit_fused(ctx.h, ptr(u), ptr(a), 0.02, ptr(b), None, 0.0, 1.0, 0.0, None), STATE,
            "rmh_limit_fused must follow rmh_ho_apply on the same u")
    refused(lib, lib.rmh_limit_fused_lo(ctx.h, ptr(u), ptr(a), None, 0.02, ptr(b), None, 0.0, 1.0, 0.0, None), INVALID, "null du_lo")
    ctx.close()
    ctx = context(lib, cases, 3, ne_ghost=1)
    refused(lib, lib.rmh_limit_fused(ctx.h, ptr(u), ptr(a), 0.02, ptr(b), None, 0.0, 1.0, 0.0, None), STATE,
            "rmh_limit_fused must follow rmh_ho_apply on the same u")
    ctx.close()


def test_order_refusals_before_everything_else(lib, cases):
    u = cases[3][2]
    for dim in (3, 2):
        # order 1 and no sub-mesh velocity: the order is what is named
        ctx = context(lib, cases, dim, order=1)
        v = np.zeros((cases[dim][2].shape[0], 2**dim))
        w = np.zeros_like(v)
        refused(lib, lib.rmh_lo_rdsubcell(ctx.h, ptr(v), None), INVALID, "null argument")
        refused(lib, lib.rmh_lo_rdsubcell(ctx.h, ptr(v), ptr(w)), INVALID, "Subcell schemes require FE order > 2.")
        refused(lib, lib.rmh_lo_rd(ctx.h, ptr(v), ptr(w)), INVALID, "rmh_lo_rd: the RD kernel is built for orders >= 2")
        ctx.close()
        # order 2 without it
        ctx = context(lib, cases, dim, subcell=False)
        refused(lib, lib.rmh_lo_rdsubcell(ctx.h, ptr(v), ptr(w)), STATE, "rmh_lo_rdsubcell needs rmh_layout.subcell_vel")
        ctx.close()
    # -lo 2 in 3-D at order >= 4: refused in front of the ghost checks (a context with a ghost whose values were never set) ...
    ctx = context(lib, cases, 3, order=4, ne_ghost=1)
    v, w = np.zeros((u.shape[0], 125)), np.zeros((u.shape[0], 125))
    refused(lib, lib.rmh_lo_upwind_prec(ctx.h, None, ptr(w)), INVALID, "null argument")
    refused(lib, lib.rmh_lo_upwind_prec(ctx.h, ptr(v), ptr(w)), INVALID,
            "rmh_lo_upwind_prec (-lo 2): order 4 in 3-D is not supported: the element's dense matrices must fit the LDS")
    # ... which are what -lo 1 on the same context reports
    refused(lib, lib.rmh_lo_upwind(ctx.h, ptr(v), ptr(w)), STATE, "ghost values of u not set")
    ctx.close()
    ctx = context(lib, cases, 3, ne_ghost=1)
    refused(lib, lib.rmh_lo_upwind_prec(ctx.h, ptr(u), ptr(np.zeros_like(u))), STATE, "ghost values of u not set")
    ctx.close()


def test_dt_check_follows_the_null_check(lib, cases):
    u = cases[3][2]
    z = [np.zeros_like(u) for _ in range(7)]
    el, dofs = np.ones(u.shape[0], dtype=np.uint8), np.ones(u.shape, dtype=np.uint8)
    ctx = context(lib, cases, 3)
    for fn in (lib.rmh_fct_projection, lib.rmh_fct_fluxbased):
        for dt in (0.0, 0.02):
            refused(lib, fn(ctx.h, ptr(u), ptr(z[0]), ptr(z[1]), ptr(z[2]), ptr(z[3]), ptr(z[4]), dt, None), INVALID, "null argument")
        for dt in (0.0, -1.0, float("nan")):
            refused(lib, fn(ctx.h, ptr(u), ptr(z[0]), ptr(z[1]), ptr(z[2]), ptr(z[3]), ptr(z[4]), dt, ptr(z[5])), INVALID, "dt must be positive")
    refused(lib, lib.rmh_fct_product(ctx.h, ptr(u), ptr(z[0]), ptr(z[1]), ptr(z[2]), ptr(z[3]), ptr(z[4]), ptr(el), None, 0.0, ptr(z[5])),
            INVALID, "null argument")
    refused(lib, lib.rmh_fct_product(ctx.h, ptr(u), ptr(z[0]), ptr(z[1]), ptr(z[2]), ptr(z[3]), ptr(z[4]), ptr(el), ptr(dofs), 0.0, ptr(z[5])),
            INVALID, "dt must be positive")
    ctx.close()
    # FluxBasedFCT on a context with a ghost: the step is checked in front of the single-rank refusal
    ctx = context(lib, cases, 3, ne_ghost=1)
    args = (ptr(u), ptr(z[0]), ptr(z[1]), ptr(z[2]), ptr(z[3]), ptr(z[4]))
    refused(lib, lib.rmh_fct_fluxbased(ctx.h, *args, 0.0, ptr(z[5])), INVALID, "dt must be positive")
    refused(lib, lib.rmh_fct_fluxbased(ctx.h, *args, 0.02, ptr(z[5])), INVALID,
            "rmh_fct_fluxbased: contexts with ghost elements are not supported")
    ctx.close()


# ---- state left behind ----------------------------------------------------------------------------------------------------------

def test_refused_massavg_invalidates_the_token(lib, cases):
    u = cases[3][2]
    dt = DT[3]
    ctx = context(lib, cases, 3)
    y1, z2, ref, a, b = (np.zeros_like(u) for _ in range(5))
    # (what the token buys: with it the extrema of the stage's output are taken as they were -- stale after a change in place)
    t1 = ctx.stage_fused(u, dt, y1, dt_rk=dt)
    assert t1 != 0
    y1[0, :] += 0.25
    ctx.stage_fused(y1, dt, z2, dt_rk=dt, token=t1)
    ctx.stage_fused(y1, dt, ref, dt_rk=dt)
    assert not np.array_equal(ref, z2)
    # a refused rmh_lo_massavg (the stage has left no lumped mass: no ho_done) in between: the token is void
    t1 = ctx.stage_fused(u, dt, y1, dt_rk=dt)
    assert t1 != 0
    y1[0, :] += 0.25
    refused(lib, lib.rmh_lo_massavg(ctx.h, ptr(u), ptr(a), dt, ptr(b)), STATE, "rmh_lo_massavg needs the lumped mass of rmh_ho_apply")
    ctx.stage_fused(y1, dt, z2, dt_rk=dt, token=t1)
    assert np.array_equal(ref, z2)
    ctx.close()


@pytest.mark.parametrize("dim,lo", [(3, 5), (3, 4), (3, 3), (2, 5), (2, 4)])
def test_rd_calls_leave_the_lo_type(lib, cases, dim, lo):
    u = cases[dim][2]
    dt = DT[dim]
    out = []
    for rd_first in (True, False):
        ctx = context(lib, cases, dim)
        ctx.set_lo_type(lo)
        if rd_first:
            d4, d3 = np.zeros_like(u), np.zeros_like(u)
            assert lib.rmh_lo_rdsubcell(ctx.h, ptr(u), ptr(d4)) == OK, lib.rmh_last_error()
            assert lib.rmh_lo_rd(ctx.h, ptr(u), ptr(d3)) == OK, lib.rmh_last_error()
            assert np.isfinite(d4).all() and np.isfinite(d3).all() and not np.array_equal(d4, d3)
        y, du = np.full_like(u, np.nan), np.full_like(u, np.nan)
        ctx.stage_fused(u, dt, y, dt_rk=dt, du=du)
        ctx.close()
        assert np.isfinite(y).all() and np.isfinite(du).all()
        out.append((y, du))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("lo", [5, 4])
def test_batch_order_is_a_function_of_the_context(lib, cases, lo):
    u = cases[3][2]
    ctx = context(lib, cases, 3)
    ctx.set_lo_type(lo)
    before = [ctx.batch_order(n) for n in (0, 8, 4096)]
    y = np.zeros_like(u)
    ctx.stage_fused(u, DT[3], y)
    assert [ctx.batch_order(n) for n in (0, 8, 4096)] == before
    assert all(b[1] == 9 for b in before)  # (order 2: nine elements a workgroup, K2Cfg::NB in rmh_ho2.hpp, with and without the RD part)
    ctx.close()
    ctx = context(lib, cases, 2)
    refused(lib, lib.rmh_batch_order(ctx.h, 8, *[C.byref(C.c_int()) for _ in range(4)]), INVALID, "rmh_batch_order: not available for dim = 2")
    ctx.close()


# ---- every (order, dimension) dispatch, on both dimensions ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def granular(lib, cases):
    """dim -> (context behind one rmh_ho_apply, inputs of the granular entry points: computed once, read only)"""
    out = {}
    for dim in (3, 2):
        u = cases[dim][2]
        ctx = context(lib, cases, dim)
        d = {k: np.full_like(u, np.nan) for k in ("du_ho", "m", "du_lo", "umin", "umax")}
        d["xmn"], d["xmx"] = np.full(u.shape[0], np.nan), np.full(u.shape[0], np.nan)
        ctx.ho_apply(u, d["du_ho"])
        ctx.compute_lumped_mass(T, d["m"])
        ctx.lo_massavg(u, d["du_ho"], DT[dim], d["du_lo"])
        ctx.elem_minmax(u, d["xmn"], d["xmx"])
        ctx.bounds(d["xmn"], d["xmx"], d["umin"], d["umax"])
        for v in d.values():
            assert np.isfinite(v).all()
            v.flags.writeable = False
        d["u"], d["dt"] = u, DT[dim]
        out[dim] = (ctx, d)
    yield out
    for ctx, _ in out.values():
        ctx.close()


def _limiter(name):
    return lambda lib, h, d, o: getattr(lib, name)(h, ptr(d["u"]), ptr(d["m"]), ptr(d["du_ho"]), ptr(d["du_lo"]), ptr(d["umin"]),
                                                   ptr(d["umax"]), d["dt"], ptr(o[0]))


# the entry points that dispatch on (order, dimension): name -> call writing o[0] (and o[1])
ENTRIES = {
    "rmh_ho_apply": lambda lib, h, d, o: lib.rmh_ho_apply(h, ptr(d["u"]), ptr(o[0])),
    "rmh_lo_massavg": lambda lib, h, d, o: lib.rmh_lo_massavg(h, ptr(d["u"]), ptr(d["du_ho"]), d["dt"], ptr(o[0])),
    "rmh_lo_rd": lambda lib, h, d, o: lib.rmh_lo_rd(h, ptr(d["u"]), ptr(o[0])),
    "rmh_lo_rdsubcell": lambda lib, h, d, o: lib.rmh_lo_rdsubcell(h, ptr(d["u"]), ptr(o[0])),
    "rmh_elem_minmax": lambda lib, h, d, o: lib.rmh_elem_minmax(h, ptr(d["u"]), ptr(o[0]), ptr(o[1])),
    "rmh_bounds": lambda lib, h, d, o: lib.rmh_bounds(h, ptr(d["xmn"]), ptr(d["xmx"]), ptr(o[0]), ptr(o[1])),
    "rmh_fct_clipscale": _limiter("rmh_fct_clipscale"),
    "rmh_fct_projection": _limiter("rmh_fct_projection"),
    "rmh_fct_fluxbased": _limiter("rmh_fct_fluxbased"),
    "rmh_lo_upwind": lambda lib, h, d, o: lib.rmh_lo_upwind(h, ptr(d["u"]), ptr(o[0])),
    "rmh_lo_upwind_prec": lambda lib, h, d, o: lib.rmh_lo_upwind_prec(h, ptr(d["u"]), ptr(o[0])),
    "rmh_ho_neumann": lambda lib, h, d, o: lib.rmh_ho_neumann(h, ptr(d["u"]), ptr(o[0])),
    "rmh_limit_fused": lambda lib, h, d, o: lib.rmh_limit_fused(h, ptr(d["u"]), ptr(d["du_ho"]), d["dt"], ptr(o[0]), None, 0.0, 1.0, 0.0, None),
    "rmh_limit_fused_lo": lambda lib, h, d, o: lib.rmh_limit_fused_lo(h, ptr(d["u"]), ptr(d["du_ho"]), ptr(d["du_lo"]), d["dt"], ptr(o[0]), None,
                                                                     0.0, 1.0, 0.0, None),
}


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_dispatch_reaches_the_kernel_of_the_dimension(lib, granular, entry, dim):
    ctx, d = granular[dim]
    u = d["u"]
    shape = (u.shape[0],) if entry == "rmh_elem_minmax" else u.shape
    runs = []
    for _ in range(2):
        o = [np.full(shape, np.nan), np.full(shape, np.nan)]
        assert ENTRIES[entry](lib, ctx.h, d, o) == OK, lib.rmh_last_error()
        runs.append(o)
    a = runs[0]
    n_out = 2 if entry in ("rmh_elem_minmax", "rmh_bounds") else 1
    for k in range(n_out):
        assert np.isfinite(a[k]).all() and np.abs(a[k]).max() > 0.0
        assert np.array_equal(a[k], runs[1][k])
    # what the fixture's first calls gave, and the cheap identities that a kernel of the other dimension would break
    if entry in ("rmh_ho_apply", "rmh_lo_massavg", "rmh_bounds"):
        first = {"rmh_ho_apply": ("du_ho",), "rmh_lo_massavg": ("du_lo",), "rmh_bounds": ("umin", "umax")}[entry]
        assert all(np.array_equal(a[k], d[name]) for k, name in enumerate(first))
    if entry == "rmh_elem_minmax":
        assert np.array_equal(a[0], u.min(axis=1)) and np.array_equal(a[1], u.max(axis=1))
    if entry in ("rmh_fct_projection", "rmh_fct_fluxbased"):  # a limiter's result: inside the bounds it was given (-vb tolerance) ...
        un = u + d["dt"] * a[0]
        print("undershoot", float((d["umin"] - un).max()), "overshoot", float((un - d["umax"]).max()))
        assert (un >= d["umin"] - 1e-12).all() and (un <= d["umax"] + 1e-12).all()
    if entry == "rmh_fct_projection":  # ... and, element by element, the mass of the LO rate (the lumped mass: M 1, Bernstein basis)
        defect = np.abs((d["m"] * (a[0] - d["du_lo"])).sum(axis=1))
        assert (defect <= 1e-12 * np.abs(d["m"] * a[0]).sum(axis=1)).all()
    if entry in ("rmh_limit_fused", "rmh_limit_fused_lo"):  # bounds + mass average + ClipScale in one kernel
        cs = np.full_like(u, np.nan)
        assert ENTRIES["rmh_fct_clipscale"](lib, ctx.h, d, [cs]) == OK
        assert np.abs(a[0] - cs).max() <= 1e-12 * np.abs(cs).max()
