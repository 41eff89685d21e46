"""TEST INFRASTRUCTURE: the oracle in one dimension (helper of tests/test_1d_emu.py and tests/test_gpu_1d.py; not collected).

oracle/remhos_oracle.py is dimension-generic except for `det` and `adjugate`, which have no 1 x 1 branch.  `patched()` installs
two wrappers in the module while a 1-D test runs and restores the originals afterwards; with them the oracle reproduces the
reference's own 1-D answers (autotest/out_baseline.dat, tests/golden/reference_kat_1d.json) to ten digits.
"""
import contextlib

import numpy as np

import oracle.remhos_oracle as ro
from oracle.remhos_oracle import Config, Lattice, Remhos, refine_coords

SEGMENT_COARSE = [0.0, 0.25, 0.5, 0.75, 1.0]  # data/periodic-segment.mesh


@contextlib.contextmanager
def patched():
    adj0, det0 = ro.adjugate, ro.det

    def adjugate(J):
        return np.ones_like(J) if J.shape[-1] == 1 else adj0(J)

    def det(J):
        return J[..., 0, 0] if J.shape[-1] == 1 else det0(J)

    ro.adjugate, ro.det = adjugate, det
    try:
        yield
    finally:
        ro.adjugate, ro.det = adj0, det0


def segment_lattice(rs):
    """data/periodic-segment.mesh refined rs times"""
    v = refine_coords(SEGMENT_COARSE, rs)
    return Lattice(1, (v.size - 1,), True, [v], 2)


def lattice_1d(n, periodic, graded):
    """n segments on [0, 1]; graded: True -- every segment 15 % longer than the one before (a jump at the seam when periodic);
    a sequence -- the n + 1 vertex coordinates themselves"""
    if n == 32 and periodic and graded is False:
        return segment_lattice(3)
    if graded is True or graded is False:
        w = 1.15 ** np.arange(n) if graded else np.ones(n)
        v = np.concatenate([[0.0], np.cumsum(w)]) / w.sum()
        v[-1] = 1.0
    else:
        v = np.asarray(graded, dtype=np.float64)
        assert v.size == n + 1 and (np.diff(v) > 0).all()
    return Lattice(1, (n,), periodic, [v], 2)


def make(lat, p, lo, bounds_type=0, **kw):
    """an oracle of problem 0 on the lattice (call inside patched())"""
    kw.setdefault("dt", 0.002)
    kw.setdefault("t_final", 1.0)
    return Remhos(Config(order=p, problem=0, lo=lo, fct=2, bounds_type=bounds_type, **kw), lat)


def moving(r, lo):
    """switch an oracle built with problem 0 to exec_mode = 1 (remap) with the displacement 0.04 sin(2 pi x): the mesh stays
    valid for pseudo-times up to 1 (|d displacement / dx| <= 0.26)"""
    disp = lambda x: 0.04 * np.sin(2.0 * np.pi * x)  # noqa: E731
    r.exec_mode = 1
    r.V = disp(r.X0)
    if lo == 4:
        r.Xs0 = np.einsum("an,enc->eac", r.T.PsiCU, r.X0)
        r.Vs = disp(r.Xs0)
    return r


def layout_1d(r):
    """the C-ABI arrays of include/rmh.h "dim = 1": x0, vel [ne][1][3], face_nbr [ne][2], stencil [ne][3], subcell_vel
    [ne][1][p + 1] (lo 4) or None"""
    lat = r.lat
    assert lat.dim == 1
    x0 = np.ascontiguousarray(r.X0.transpose(0, 2, 1))
    v = r.V if r.exec_mode == 1 else r.vel(r.X0)
    vel = np.ascontiguousarray(v.transpose(0, 2, 1))
    st = np.stack([lat.shifted((-1,)), np.arange(lat.ne), lat.shifted((1,))], axis=1).astype(np.int32)
    sub = None
    if r.cfg.lo == 4:
        sv = r.Vs if r.exec_mode == 1 else r.vel(r.Xs0)
        sub = np.ascontiguousarray(sv.transpose(0, 2, 1))
    return x0, vel, r.nbr.astype(np.int32), st, sub
