"""Unstructured 2-D quadrilateral meshes on the CPU: the mesh reader, refinement and topology of the host library against the
restatement (tests/unstructured_oracle.py), and the kernels, the C ABI and the driver through the g++ emulation build of the same
sources (the checks of tests/unstructured_cases.py; tests/test_gpu_unstructured.py runs them on the device).

On the emulation, the three 500-step periodic-hexagon lines are left to the device (every work-item is an OS thread there: minutes
per line); ctest #8 on star-q2 (5 steps, 80 elements) and the short runs are here."""
import numpy as np
import pytest

from tests import unstructured_cases as uc
from tests import unstructured_oracle as uo


@pytest.fixture(scope="module")
def emu():
    return uc.Backend(False)


# ---- 1. orientation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 3, 6])
def test_rotated_elements_give_the_lattice_numbers(emu, p):
    uc.check_rotated(emu, p)


# ---- 2. bounds at irregular vertices ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,valences", [("star-q2", (5,)), ("periodic-hexagon", (3, 6))])
def test_bounds_at_irregular_vertices(emu, name, valences):
    uc.check_bounds_irregular(emu, name, valences)


# ---- 3. the case builder against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["star-q2", "periodic-hexagon"])
@pytest.mark.parametrize("rs", [0, 1])
def test_builder_against_restatement(name, rs):
    problem = 14 if name == "star-q2" else 0
    case = uc.file_case(name, rs, 3, problem, 4)
    kw = dict(order=3, problem=problem, lo=4, dt=-1.0 if problem == 14 else 0.005, t_final=0.5 if problem == 14 else 2.5)
    r = uo.make(name, rs, **kw)
    mesh = r.lat
    assert case.unstructured and case.dim == 2 and case.ne_owned == mesh.ne and case.ne_ghost == 0
    assert np.array_equal(case.elem_vertices, mesh.ev)
    # nodes: the same arithmetic in another summation order -- 9 terms of size <= max |x| per refinement level, each sum within
    # 8 eps of the exact one: 16 eps max |x| between the two (max |x| = 1.31)
    tol_x = 16 * np.finfo(float).eps * np.abs(mesh.X0).max() * max(rs, 1)
    assert np.abs(case.x0.transpose(0, 2, 1) - mesh.X0).max() <= tol_x
    assert np.abs(np.array(case.bb_min[:2]) - r.bb_min).max() <= tol_x and np.abs(np.array(case.bb_max[:2]) - r.bb_max).max() <= tol_x
    assert abs(case.dt - r.dt) <= 1e-15 * r.dt
    assert np.abs(case.u0 - r.u).max() <= 1e-13
    v = r.V if r.exec_mode == 1 else r.vel(r.X0)
    assert np.abs(case.vel.transpose(0, 2, 1) - v).max() <= 1e-14
    sv = r.Vs if r.exec_mode == 1 else r.vel(r.Xs0)
    assert np.abs(case.subcell_vel.transpose(0, 2, 1) - sv).max() <= 1e-14
    if name == "star-q2":
        assert (sv[r._submesh_boundary_mask()] == 0).all() and r._submesh_boundary_mask().any()
    # topology
    assert np.array_equal(case.face_nbr, mesh.nbr)
    code, ptr, els = case.quad_topology
    assert np.array_equal(code, mesh.face_code())
    for e in range(mesh.ne):
        for k in range(4):
            row = els[ptr[4 * e + k]:ptr[4 * e + k + 1]]
            assert len(set(row)) == len(row) and set(row) == set(mesh.corners[e][k]), (e, k)
    st = -np.ones((mesh.ne, 9), dtype=np.int32)
    st[:, 4] = np.arange(mesh.ne)
    assert np.array_equal(case.stencil27, st)


@pytest.mark.parametrize("name", ["star-q2", "periodic-hexagon"])
@pytest.mark.parametrize("rs", [0, 1])
def test_lumped_mass_against_restatement(emu, name, rs):
    uc.check_lumped_mass(emu, name, rs)


def test_no_error_norms_on_a_file_mesh(emu):
    uc.check_no_error_norms(emu.lib)


def test_build_tables_quad_on_a_lattice():
    """the sibling of rmh_build_tables_2d on aligned axes: g = f ^ 1, flip = 0, and the 3 x 3 stencil as corner rows"""
    from remhos_amd.capi import build_tables_quad
    from remhos_amd.case import load_host_library

    N = 4
    ex, ey = np.arange(N * N) % N, np.arange(N * N) // N
    ev = np.stack([(ex + kx) + (N + 1) * (ey + ky) for ky in (0, 1) for kx in (0, 1)], axis=1)
    nbr, (code, ptr, els) = build_tables_quad(load_host_library(), ev)
    for e in range(N * N):
        for f in range(4):
            if nbr[e, f] >= 0:
                assert code[e, f] == f ^ 1
    assert ptr[-1] == len(els) == 4 * (N - 1) ** 2 * 3 + 4 * (N - 1) * 2 * 1  # interior vertices: 4 corners see 3 others; edge vertices: 2 see 1


# ---- 4. + 5. runs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pa", [0, 1])
def test_star_steps_against_restatement(emu, pa):
    uc.check_run(emu, "star-q2", pa, 5, 5)


@pytest.mark.parametrize("lo", [3, 4, 5])
def test_hexagon_steps_against_restatement(emu, lo):
    """(-rs 1 here, 48 elements with the vertices of valence 3 and 6: the emulation takes a minute for the 192 of -rs 2, which the
    device runs)"""
    uc.check_run(emu, "periodic-hexagon", 0, lo, 6, rs=1)


def test_hexagon_dt_control(emu):
    """-bt 1 -dtc 1 on a file mesh: the step that is too large is repeated as in the restatement.  (Not with -vb: the LO update of
    such a step leaves its bounds -- what the estimate detects -- and the reference's check aborts on it.)"""
    uc.check_run(emu, "periodic-hexagon", 0, 4, 6, rs=1, dt=uc.DTC_DT, bounds_type=1, dt_control=1)


def test_hexagon_verify_bounds(emu):
    """-vb on a file mesh: the in-loop bounds checks of the LO and the limited update pass at the reference's step"""
    uc.check_run(emu, "periodic-hexagon", 0, 4, 3, rs=1, verify_bounds=1)


@pytest.mark.parametrize("pa", [0, 1])
def test_star_ctest8(emu, pa):
    uc.check_kat_star(emu, pa)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
REFUSED = [
    (dict(fused=1), "fused = 1"), (dict(ho_type=1), "ho_type 1"), (dict(lo_type=1), "lo_type 1|2"), (dict(lo_type=2), "lo_type 1|2"),
    (dict(fct_type=1), "fct_type 1"), (dict(fct_type=4), "fct_type 4"), (dict(mono_type=1), "mono_type"), (dict(ps=1, ode_solver=12), "ps"),
    (dict(ode_solver=12), "ode_solver"), (dict(part=(2, 1, 1)), "partitions"), (dict(save=1), "save"),
]


@pytest.mark.parametrize("kw,names", REFUSED, ids=[n for _, n in REFUSED])
def test_driver_refuses_option(emu, kw, names):
    msg = uc.driver_error(emu, "star-q2", **dict(dict(uc.STAR, fused=0), **kw))
    assert names in msg and "unstructured" in msg, msg


def test_missing_file_is_an_unknown_mesh(emu):
    msg = uc.driver_error(emu, "star-q2", mesh_file="data/star-q2.mesh", **dict(uc.STAR, fused=0))
    assert "unknown lattice mesh" in msg, msg
    # a built-in name ignores the path
    from remhos_amd.case import Case, load_host_library, make_config

    c = Case(load_host_library(), make_config(mesh="inline-quad", mesh_file="data/nothing.mesh", rs=0, order=2, problem=14))
    assert not c.unstructured and c.ne_owned == 16


def _write(tmp_path, text):
    f = tmp_path / "m.mesh"
    f.write_text(text)
    return str(f)


HEAD = "MFEM mesh v1.0\n\ndimension\n2\n\nelements\n"
SQUARE = "boundary\n0\n\nvertices\n4\n2\n0 0\n1 0\n1 1\n0 1\n"


def _case_error(path):
    from remhos_amd.case import Case, load_host_library, make_config

    with pytest.raises(RuntimeError) as ei:
        Case(load_host_library(), make_config(mesh="m", mesh_file=path, rs=0, order=2, problem=14, fused=0))
    return str(ei.value)


def test_reader_refusals(tmp_path):
    from remhos_amd.case import Case, load_host_library, make_config

    ok = _write(tmp_path, HEAD + "1\n1 3 0 1 2 3\n\n" + SQUARE)
    c = Case(load_host_library(), make_config(mesh="m", mesh_file=ok, rs=1, order=2, problem=14, fused=0))
    assert c.unstructured and c.ne_owned == 4 and c.bb_max[:2] == [1.0, 1.0]  # plain vertices: the third input form
    msg = _case_error(_write(tmp_path, HEAD + "1\n1 3 0 3 2 1\n\n" + SQUARE))
    assert "clockwise" in msg and "element 0" in msg, msg
    msg = _case_error(_write(tmp_path, HEAD + "2\n1 2 0 1 2\n1 2 0 2 3\n\n" + SQUARE))
    assert "geometry type 2" in msg and "triangle" in msg, msg
    cubic = HEAD + "1\n1 3 0 1 2 3\n\nboundary\n0\n\nvertices\n4\n\nnodes\nFiniteElementSpace\nFiniteElementCollection: Cubic\nVDim: 2\nOrdering: 0\n" + "0\n" * 32
    msg = _case_error(_write(tmp_path, cubic))
    assert "'Cubic'" in msg, msg
    msg = _case_error(_write(tmp_path, "MFEM NURBS mesh v1.0\n"))
    assert "NURBS" in msg, msg
    # an element that is its own neighbour: a periodic strip one element wide
    msg = _case_error(_write(tmp_path, HEAD + "1\n1 3 0 1 1 0\n\nboundary\n0\n\nvertices\n2\n2\n0 0\n1 0\n"))
    assert "twice" in msg or "own neighbour" in msg, msg


ENTRIES = ["limit_fused", "limit_fused_lo", "stage_fused", "ho_neumann", "lo_upwind", "lo_upwind_prec", "fct_fluxbased", "mono_rd"]


def check_entry_refusals(bk):
    from remhos_amd.capi import RmhError

    case = uc.file_case("star-q2", 0, 2, 14, 5)
    ctx = bk.context(order=2, exec_mode=1, x0=case.x0, vel=case.vel, face_nbr=case.face_nbr, quad_topology=case.quad_topology)
    u = bk.arr(case.u0)
    a, b, c, d, e = (bk.arr(np.zeros_like(case.u0)) for _ in range(5))
    s = bk.arr(np.ones(case.ne_owned))
    calls = {
        "limit_fused": lambda: ctx.limit_fused(u, a, 0.01, du=b), "limit_fused_lo": lambda: ctx.limit_fused_lo(u, a, b, 0.01, du=c),
        "stage_fused": lambda: ctx.stage_fused(u, 0.01, a), "ho_neumann": lambda: ctx.ho_neumann(u, a), "lo_upwind": lambda: ctx.lo_upwind(u, a),
        "lo_upwind_prec": lambda: ctx.lo_upwind_prec(u, a), "fct_fluxbased": lambda: ctx.fct_fluxbased(u, a, b, c, d, e, 0.01, bk.arr(np.zeros_like(case.u0))),
        "mono_rd": lambda: ctx.mono_rd(u, a, b, s, 1, c),
    }
    for name in ENTRIES:
        with pytest.raises(RmhError) as ei:
            calls[name]()
        assert "unstructured" in str(ei.value) and ("rmh_" + name.split("_lo")[0] if name.startswith("limit") else "rmh_" + name) in str(ei.value), (name, str(ei.value))
    # the tables are validated like those of rmh_create
    code, ptr, els = case.quad_topology
    down = ptr.copy()
    down[1] = down[-1] + 1  # (then the next entry is smaller)
    for bad, what in (((code + 8, ptr, els), "face_code"), ((code, ptr, els + case.ne_owned), "corner_elems"), ((code, down, els), "corner_ptr")):
        with pytest.raises(RmhError, match=what):
            bk.context(order=2, exec_mode=1, x0=case.x0, vel=case.vel, face_nbr=case.face_nbr, quad_topology=bad)
    ctx.close()


def test_entry_points_refuse_an_unstructured_context(emu):
    check_entry_refusals(emu)
