"""Checks of the unstructured 2-D quadrilateral path (mesh files, rmh_build_tables_quad, rmh_set_quad_topology) that run on either
build of the library: tests/test_unstructured_emu.py hands them the g++ emulation build (CPU), tests/test_gpu_unstructured.py the
device library.  References: the committed lattice oracle (rotated elements must give the lattice's numbers) and the CPU
restatement tests/unstructured_oracle.py (pinned by the reference's own numbers in tests/test_unstructured_oracle.py)."""
import ctypes as C
import functools
import json
import os

import numpy as np

from oracle.remhos_oracle import Config, Lattice, Remhos
from tests import unstructured_oracle as uo
from tests.helpers import check_rel, emu_library_path, layout_from_oracle, perturbed

KAT = json.load(open(os.path.join(uo.ROOT, "tests", "golden", "reference_kat_unstructured.json")))


def mesh_path(name):
    return os.path.join(uo.MESH_DIR, name + ".mesh")


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


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

    def context(self, **kw):
        from remhos_amd.capi import Context

        ctx = Context(self.lib, **kw)
        assert ctx.dim == 2
        if self.gpu:
            ctx.set_stream(self.torch.cuda.current_stream().cuda_stream)
        return ctx


def twice(bk, call, *shapes):
    """run call(*outputs) twice on outputs that start as NaN: every entry written, and the same bits both times"""
    res = []
    for _ in range(2):
        outs = [bk.nan(s) for s in shapes]
        call(*outs)
        res.append([np.array(bk.host(o)) for o in outs])
    for a, b in zip(*res):
        assert not np.isnan(a).any(), "an entry was left out"
        assert a.tobytes() == b.tobytes(), "two calls, different bits"
    return res[0] if len(shapes) > 1 else res[0][0]


# ---- 1. orientation: a lattice whose elements are turned by quarter turns must give the lattice's numbers ------------------------
def turn_perm(n, q):
    """new = old[perm] for an n x n lexicographic grid (index i + n j) seen from reference axes turned by q quarter turns:
    (xi, eta) = (1 - eta', xi') per turn, which keeps the element counter-clockwise"""
    one = np.array([(n - 1 - j) + n * i for j in range(n) for i in range(n)])
    perm = np.arange(n * n)
    for _ in range(q % 4):
        perm = perm[one]
    return perm


@functools.lru_cache(maxsize=None)
def rotated_case(p):
    """inline-quad cut into 5 x 5 elements, problem 14 at t = 0.3, element (ex, ey) turned by (ex + 2 ey) mod 4 quarter turns (see below).
    The oracle's vectors of the LATTICE are computed once per order and shared (never modified)."""
    N, t, dt = 5, 0.3, 0.004
    v = np.linspace(0.0, 1.0, N + 1)
    lat = Lattice(2, (N, N), False, [v.copy(), v.copy()], 2)
    r = Remhos(Config(mesh="inline-quad", rs=0, order=p, problem=14, dt=dt, t_final=0.7, lo=4 if p >= 2 else 5), lat)
    r.refine_steps = 2
    uh = perturbed(r.u)
    keep = {}
    r.stage(uh, t, dt, keep)
    ref = dict(m=keep["m"], du_ho=keep["du_ho"], xe_min=uh.min(-1), xe_max=uh.max(-1))
    if p >= 2:
        ref["lo4"] = keep["du_lo"]
        r.cfg.lo = 3
        ref["lo3"] = r.calc_lo_rd(uh)
        r.cfg.lo = 4
    for bt in (0, 1):
        r.cfg.bounds_type = bt
        ref["bounds", bt] = r.bounds_from_extrema(ref["xe_min"], ref["xe_max"])
    r.cfg.bounds_type = 0
    x0, vel, _, _ = layout_from_oracle(r)
    sub = np.ascontiguousarray(r.Vs.transpose(0, 2, 1)) if p >= 2 else None
    ex, ey = np.arange(N * N) % N, np.arange(N * N) // N
    # (ex + 2 ey) mod 4 quarter turns -- but the last column and the last row repeat the turn of the one before: under the plain rule
    # x-neighbours always differ by one turn and y-neighbours by two, so the four pairings g = f ^ 1 of two equally turned
    # elements (the lattice's own) would never occur and only 12 of the 16 pairings would be exercised
    turns = (np.minimum(ex, N - 2) + 2 * np.minimum(ey, N - 2)) % 4
    ev = np.stack([(ex + kx) + (N + 1) * (ey + ky) for ky in (0, 1) for kx in (0, 1)], axis=1)
    pn = np.stack([turn_perm(3, q) for q in turns])      # nodes
    pd = np.stack([turn_perm(p + 1, q) for q in turns])  # dofs
    pc = np.stack([turn_perm(2, q) for q in turns])      # corners
    rows = np.arange(N * N)[:, None]
    rot = dict(x0=np.ascontiguousarray(x0[rows, :, pn].transpose(0, 2, 1)), vel=np.ascontiguousarray(vel[rows, :, pn].transpose(0, 2, 1)),
               sub=None if sub is None else np.ascontiguousarray(sub[rows, :, pd].transpose(0, 2, 1)), ev=ev[rows, pc], u=uh[rows, pd])
    for a in (uh, *(x for x in ref.values() if isinstance(x, np.ndarray))):
        a.setflags(write=False)
    return dict(p=p, t=t, dt=dt, ne=N * N, pd=pd, rows=rows, ref=ref, rot=rot)


def check_rotated(bk, p):
    from remhos_amd.capi import build_tables_quad

    c = rotated_case(p)
    ref, rot, pd, rows, ne = c["ref"], c["rot"], c["pd"], c["rows"], c["ne"]
    nbr, topo = build_tables_quad(bk.lib, rot["ev"])
    code = topo[0]
    inner = nbr >= 0
    pairs = {(f, int(code[e, f] & 3)) for e in range(ne) for f in range(4) if inner[e, f]}
    assert len(pairs) == 16, sorted(pairs)  # every own face meets every neighbour face
    assert {int(x) for x in (code[inner] >> 2)} == {0, 1}  # both directions of the tangential parameter
    ctx = bk.context(order=p, exec_mode=1, x0=rot["x0"], vel=rot["vel"], face_nbr=nbr, subcell_vel=rot["sub"], quad_topology=topo)
    where = f"rotated 5 x 5 p{p}"
    u = bk.arr(rot["u"])
    sh = rot["u"].shape
    ctx.setup(c["t"])
    turned = lambda a: a[rows, pd]  # noqa: E731  (the lattice's vector in the turned dof order)
    du_ho = twice(bk, lambda o: ctx.ho_apply(u, o), sh)
    check_rel(p, _rel(du_ho, turned(ref["du_ho"])), where + " du_ho")
    m = twice(bk, lambda o: ctx.compute_lumped_mass(c["t"], o), sh)
    check_rel(p, _rel(m, turned(ref["m"])), where + " lumped mass")
    # rmh_lumped_mass: the context's own vector, left by rmh_ho_apply (copied out with the driver's vector kernel, z = 1 x + 0 x)
    m_ctx = bk.nan(sh)
    stream = bk.torch.cuda.current_stream().cuda_stream if bk.gpu else None
    ptr = ctx.lumped_mass_ptr()
    assert bk.lib.rmhd_axpby(1.0, ptr, 0.0, ptr, m_ctx.data_ptr() if bk.gpu else m_ctx.ctypes.data, m.size, stream) == 0
    assert np.array_equal(np.array(bk.host(m_ctx)), m), where + " rmh_lumped_mass"
    if p >= 2:
        lo3 = twice(bk, lambda o: ctx.lo_rd(u, o), sh)
        check_rel(p, _rel(lo3, turned(ref["lo3"])), where + " lo_rd")
        lo4 = twice(bk, lambda o: ctx.lo_rdsubcell(u, o), sh)
        check_rel(p, _rel(lo4, turned(ref["lo4"])), where + " lo_rdsubcell")
    xmn, xmx = twice(bk, lambda a, b: ctx.elem_minmax(u, a, b), (ne,), (ne,))
    assert np.array_equal(xmn, ref["xe_min"]) and np.array_equal(xmx, ref["xe_max"])
    d_mn, d_mx = bk.arr(xmn), bk.arr(xmx)
    for bt in (0, 1):
        ctx.set_bounds_type(bt)
        umin, umax = twice(bk, lambda a, b: ctx.bounds(d_mn, d_mx, a, b), sh, sh)
        assert np.array_equal(umin, turned(ref["bounds", bt][0])) and np.array_equal(umax, turned(ref["bounds", bt][1])), (where, bt)
    ctx.close()


# ---- 2. bounds where the vertex valence is not 4 ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def file_case(name, rs, order, problem, lo):
    from remhos_amd.case import Case, load_host_library, make_config

    return Case(load_host_library(), make_config(mesh=name, mesh_file=mesh_path(name), rs=rs, order=order, problem=problem, lo_type=lo,
                                                  fused=0, dt=-1.0 if problem >= 10 else 0.005, t_final=0.5 if problem >= 10 else 2.5))


def check_bounds_irregular(bk, name, valences):
    case = file_case(name, 1, 3, 14 if name == "star-q2" else 0, 5)
    ne = case.ne_owned
    code, ptr, els = case.quad_topology
    val = {}
    for v in case.elem_vertices.ravel():
        val[int(v)] = val.get(int(v), 0) + 1
    assert set(valences) <= set(val.values()), sorted(set(val.values()))
    # (the CSR row of a corner holds the valence - 1 other elements)
    rows = np.diff(ptr).reshape(ne, 4)
    assert all((rows[case.elem_vertices == v] == val[int(v)] - 1).all() for v in np.unique(case.elem_vertices))
    mesh = uo.QuadMesh(mesh_path(name), 1)
    r = uo.UnstructuredRemhos(Config(mesh=name, rs=1, order=3, problem=0, dt=0.005, lo=5), mesh)
    k = np.arange(ne, dtype=np.float64)
    xe_min, xe_max = np.sin(1.7 * k), np.sin(1.7 * k) + 0.5 + 0.4 * np.cos(0.9 * k)
    off = np.arange(ne) % 7 == 3  # inactive elements of the masked variant: the identities of min and max
    xe_min[off], xe_max[off] = np.inf, -np.inf
    ctx = bk.context(order=3, exec_mode=case.exec_mode, x0=case.x0, vel=case.vel, face_nbr=case.face_nbr, quad_topology=case.quad_topology)
    d_mn, d_mx = bk.arr(xe_min), bk.arr(xe_max)
    for bt in (0, 1):
        ctx.set_bounds_type(bt)
        r.cfg.bounds_type = bt
        umin, umax = twice(bk, lambda a, b: ctx.bounds(d_mn, d_mx, a, b), (ne, 16), (ne, 16))
        bmin, bmax = r.bounds_from_extrema(xe_min, xe_max)
        assert np.array_equal(umin, bmin) and np.array_equal(umax, bmax), (name, bt)
    ctx.close()


# ---- 3. the library's lumped mass on the builder's file mesh against the restatement ------------------------------------------------
def check_lumped_mass(bk, name, rs):
    """rmh_compute_lumped_mass on the curved Q2 elements of the star (remap: at t = 0 and on the moved mesh at t = 0.7) and on the
    hexagon, against the restatement's M 1 on its own nodes, by check_rel"""
    problem = 14 if name == "star-q2" else 0
    case = file_case(name, rs, 3, problem, 5)
    r = uo.make(name, rs, order=3, problem=problem, lo=5, dt=-1.0 if problem == 14 else 0.005, t_final=0.5 if problem == 14 else 2.5)
    ctx = bk.context(order=3, exec_mode=case.exec_mode, x0=case.x0, vel=case.vel, face_nbr=case.face_nbr, quad_topology=case.quad_topology)
    sh = case.u0.shape
    for t in (0.0, 0.7) if case.exec_mode == 1 else (0.0,):
        r.update_geometry(t)
        m = twice(bk, lambda o: ctx.compute_lumped_mass(t, o), sh)
        check_rel(3, _rel(m, r.m), f"{name} rs {rs} lumped mass at t = {t}")
        assert (m > 0).all()
    ctx.close()


def check_no_error_norms(lib):
    """lp error sums are refused on a file mesh, naming it: the exact field of problem 0 is wrapped over a lattice's box"""
    from remhos_amd.case import Case, make_config

    case = file_case("periodic-hexagon", 1, 3, 0, 5)
    msg = case.lp_errors(0.1, case.u0, expect_error=True)
    assert "unstructured" in msg and "error norms" in msg, msg
    lat = Case(lib, make_config(mesh="periodic-square", rs=1, order=3, problem=0, lo_type=5, dt=0.005, t_final=2.5))
    err = lat.lp_errors(0.0, lat.u0)
    assert len(err) == 3 and all(np.isfinite(err)) and err[2] > 0.0  # (a lattice has them)


# ---- 4. + 5. whole runs through the driver --------------------------------------------------------------------------------------
_RUNS = {}


def run_driver(bk, name, **kw):
    """rmhd_run_state on the mesh file; returns (result struct, final field)"""
    from remhos_amd.case import RmhdResult, make_config

    kw.setdefault("fused", 0)
    key = (bk.gpu, name, tuple(sorted(kw.items())))
    if key not in _RUNS:  # (a run is made once and shared: ctest #8 is also the 5-step run against the restatement)
        cfg = make_config(mesh=name, mesh_file=mesh_path(name), **kw)
        case = file_case(name, kw["rs"], kw["order"], kw["problem"], kw.get("lo_type", 5))
        res = RmhdResult()
        u = np.zeros((case.ne_owned, case.ndof))
        rc = bk.lib.rmhd_run_state(C.byref(cfg), C.byref(res), u.ctypes.data, None)
        assert rc == 0, bk.lib.rmhd_last_error().decode()
        u.setflags(write=False)
        _RUNS[key] = (res, u)
    return _RUNS[key]


def driver_error(bk, name, mesh_file=None, **kw):
    """the message with which rmhd_run refuses the options"""
    from remhos_amd.case import RmhdResult, make_config

    cfg = make_config(mesh=name, mesh_file=mesh_path(name) if mesh_file is None else mesh_file, **kw)
    res = RmhdResult()
    assert bk.lib.rmhd_run(C.byref(cfg), C.byref(res)) != 0
    return bk.lib.rmhd_last_error().decode()


STAR = dict(rs=1, order=3, problem=14, dt=-1.0, t_final=0.5, lo_type=5, ho_type=3, fct_type=2, max_steps=5)
HEX = dict(rs=2, order=3, problem=0, dt=0.005, t_final=2.5, ho_type=3, fct_type=2)
# a first step the LO bounds estimate of -dtc 1 refuses: in the restatement, 6 steps are 5 accepted + 1 repeated at -rs 1 and
# 1 accepted + 5 repeated at -rs 2
DTC_DT = 0.02


@functools.lru_cache(maxsize=None)
def oracle_run(name, rs, problem, dt, t_final, lo, max_steps, ho_solve, bounds_type=0, dt_control=0):
    r = uo.make(name, rs, order=3, problem=problem, dt=dt, t_final=t_final, lo=lo, fct=2, max_steps=max_steps, ho_solve=ho_solve,
                bounds_type=bounds_type, dt_control=dt_control)
    rep = r.run()
    r.u.setflags(write=False)
    return r, rep


def check_run(bk, name, pa, lo, steps, rs=None, dt=None, bounds_type=0, dt_control=0, verify_bounds=0):
    """a few steps against the restatement: steps equal, final mass to 1e-12 relative, max to 1e-10, the field by check_rel.
    With dt_control (-bt 1 -dtc 1) the repeated steps and the final step size must agree too; -max_steps counts repeated steps."""
    kw = dict(STAR if name == "star-q2" else HEX, lo_type=lo, max_steps=steps, pa=pa, bounds_type=bounds_type, dt_control=dt_control,
              verify_bounds=verify_bounds)
    if rs is not None:
        kw["rs"] = rs
    if dt is not None:
        kw["dt"] = dt
    res, u = run_driver(bk, name, **kw)
    r, rep = oracle_run(name, kw["rs"], kw["problem"], kw["dt"], kw["t_final"], lo, steps, "pa" if pa else "exact", bounds_type, dt_control)
    print(f"{name} pa {pa} lo {lo} bt {bounds_type} dtc {dt_control}: mass {res.final_mass:.16g} / {rep['mass']:.16g}, max {res.max_value:.16g} / {rep['max']:.16g}, "
          f"field {_rel(u, r.u):.3e}, steps {res.steps} + {res.repeats} repeated")
    assert res.steps == rep["steps"] and res.steps + res.repeats == steps
    if dt_control:
        assert res.repeats == r.repeats
    if name == "periodic-hexagon":
        # no error norms on a file mesh: the exact field of problem 0 is wrapped over a lattice's bounding box (rmhd_case_lp_errors)
        assert res.has_errors == 0
    assert abs(res.dt - r.dt) <= 1e-15 * r.dt
    assert abs(res.final_mass - rep["mass"]) <= 1e-12 * abs(rep["mass"])
    assert abs(res.max_value - rep["max"]) <= 1e-10
    check_rel(3, _rel(u, r.u), f"{name} pa {pa} lo {lo} field after {steps} steps")


def check_kat_hexagon(bk, k):
    line = KAT["hexagon"][k]
    res, _ = run_driver(bk, "periodic-hexagon", rs=line["rs"], order=line["order"], problem=line["problem"], dt=line["dt"],
                        t_final=line["t_final"], ho_type=line["ho"], lo_type=line["lo"], fct_type=line["fct"], pa=line["pa"])
    print(f"hexagon line {k}: steps {res.steps} mass {res.final_mass:.12g} max {res.max_value:.12g}")
    assert res.steps == 500
    assert float(f"{res.final_mass:.10g}") == line["mass"]
    assert float(f"{res.max_value:.10g}") == line["max"]


def check_kat_star(bk, pa):
    line = KAT["star_ctest8"]
    K = line["mass"]
    res, _ = run_driver(bk, "star-q2", **dict(STAR, pa=pa))
    bound = 1e-12
    if pa:
        # the -pa stopping rule (DGMassInverse: abs 1e-8) leaves its own distance from the constant: the restatement's, not the library's
        _, rep = oracle_run("star-q2", 1, 14, -1.0, 0.5, 5, 5, "pa")
        bound += abs(rep["mass"] - K) / K
    print(f"star ctest #8 pa {pa}: mass {res.final_mass:.16g}, distance {abs(res.final_mass - K) / K:.3e}, bound {bound:.3e}")
    assert res.steps == 5
    assert abs(res.final_mass - K) <= bound * K
