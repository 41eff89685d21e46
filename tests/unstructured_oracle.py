"""CPU restatement of Remhos on UNSTRUCTURED 2-D quadrilateral meshes read from "MFEM mesh v1.0" files (TEST INFRASTRUCTURE).

The committed lattice oracle (oracle/remhos_oracle.py) assumes that every neighbour has the element's reference axes and that the
bounds stencil is 3 x 3.  This file keeps all of it and replaces exactly what those two assumptions touch:

  * the mesh object: reader, 2 x 2 refinement with topological vertex ids, face pairing (neighbour, the neighbour's local face,
    flip) and the elements around every vertex;
  * `face_apply` and the face part of `calc_lo_rd`: the neighbour's values come from ITS face layer, walked backwards when the
    tangential parameters run against each other (the Bernstein face basis is symmetric under the reversal, so the element's own
    face points and normals stay);
  * `bounds_from_extrema` for -bt 0: the CG-node sharing of DofInfo::ComputeOverlapBounds (remhos_tools.cpp:432-495) -- an
    interior dof sees its element, an edge dof also the face neighbour, a corner dof every element at the vertex.

It is pinned by the reference's own numbers in tests/test_unstructured_oracle.py (ctest #8 on star-q2, three autotest lines on
periodic-hexagon) and is what the GPU library's file-mesh path is compared with.

H1 "Quadratic" nodes are numbered vertices first, then edges in the order of their first appearance over the elements' local edges
(0,1), (1,2), (2,3), (3,0), then element interiors; an element's 9 nodes in MFEM's local order v0 e0 v1 / e3 c e1 / v3 e2 v2 are the
lexicographic a = ax + 3 ay.  Corners are lexicographic too: k = kx + 2 ky = MFEM's (0, 1, 3, 2).
"""
from __future__ import annotations

import os

import numpy as np

from oracle.remhos_oracle import INF, Config, Remhos

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_DIR = os.path.join(ROOT, "tests", "golden", "meshes")

# face f = 2 c + side runs from corner FACE[f][0] to corner FACE[f][1] along its increasing tangential parameter
FACE = ((0, 2), (1, 3), (0, 1), (2, 3))


def _lag2(t):
    return np.array([2 * (t - 0.5) * (t - 1), -4 * t * (t - 1), 2 * t * (t - 0.5)])


def read_mesh(path):
    """-> (ev [ne, 4] vertex ids in lexicographic corner order, X [ne, 9, 2] Q2 nodes, number of vertices)"""
    L = [s.strip() for s in open(path)]
    L = [s for s in L if s and not s.startswith("#")]
    if L[0] != "MFEM mesh v1.0":
        raise ValueError(f"not an MFEM mesh v1.0 file: {L[0]!r}")
    assert L[1] == "dimension" and int(L[2]) == 2, L[1:3]
    i = L.index("elements")
    ne = int(L[i + 1])
    rows = [[int(t) for t in L[i + 2 + k].split()] for k in range(ne)]
    if any(r[1] != 3 for r in rows):
        raise ValueError("only quadrilaterals (geometry 3) are read")
    mv = np.array([r[2:6] for r in rows])
    nv = int(L[L.index("vertices") + 1])
    ev = mv[:, [0, 1, 3, 2]]
    half = np.array([0.0, 0.5, 1.0])

    def from_corners(P):  # P [ne, 4, 2] lexicographic -> bilinear map at the 9 node points
        w = np.array([[(1 - x) * (1 - y), x * (1 - y), (1 - x) * y, x * y] for y in half for x in half])
        return np.einsum("aj,ejc->eac", w, P)

    if "nodes" not in L:
        j = L.index("vertices")
        assert int(L[j + 2]) == 2
        V = np.array([[float(t) for t in L[j + 3 + k].split()] for k in range(nv)])
        return ev, from_corners(V[ev]), nv
    j = L.index("nodes")
    name = L[j + 2].split(":")[1].strip()
    ordering = int(L[j + 4].split(":")[1])
    assert int(L[j + 3].split(":")[1]) == 2
    vals = np.array([float(t) for s in L[j + 5:] for t in s.split()])
    n = vals.size // 2
    X = np.stack([vals[:n], vals[n:]], 1) if ordering == 0 else vals.reshape(n, 2)
    if name == "L2_T1_2D_P1":
        assert n == 4 * ne
        return ev, from_corners(X.reshape(ne, 4, 2)), nv
    if name not in ("Quadratic", "H1_2D_P2"):
        raise ValueError(f"nodes in the space {name!r} are not read")
    edges = {}
    for v in mv:
        for a, b in ((0, 1), (1, 2), (2, 3), (3, 0)):
            edges.setdefault((min(v[a], v[b]), max(v[a], v[b])), len(edges))
    ned = len(edges)
    assert n == nv + ned + ne
    # the numbering is an assumption about MFEM's H1 space: every edge node must be the one nearest to its edge's midpoint
    for (a, b), k in edges.items():
        mid = 0.5 * (X[a] + X[b])
        assert np.argmin(np.linalg.norm(X[nv:nv + ned] - mid, axis=1)) == k, ("edge numbering", a, b)

    def eid(a, b):
        return nv + edges[(min(a, b), max(a, b))]

    ids = np.array([[v[0], eid(v[0], v[1]), v[1], eid(v[3], v[0]), nv + ned + k, eid(v[1], v[2]), v[3], eid(v[2], v[3]), v[2]]
                    for k, v in enumerate(mv)])
    return ev, X[ids], nv


def refine(ev, X, nv):
    """2 x 2 children per element (lexicographic in the parent's axes): nodes from the parent's Q2 map, vertex ids topological"""
    mid = {}

    def midv(a, b):
        nonlocal nv
        key = (min(a, b), max(a, b))
        if key not in mid:
            mid[key] = nv
            nv += 1
        return mid[key]

    ev2, X2 = [], []
    W = {}
    for cy in (0, 1):
        for cx in (0, 1):
            W[cx, cy] = np.array([np.outer(_lag2(cy * 0.5 + ay * 0.25), _lag2(cx * 0.5 + ax * 0.25)).ravel() for ay in range(3) for ax in range(3)])
    for c, Xp in zip(ev, X):
        g = np.zeros((3, 3), dtype=int)
        g[0, 0], g[0, 2], g[2, 0], g[2, 2] = c
        g[0, 1], g[2, 1], g[1, 0], g[1, 2] = midv(c[0], c[1]), midv(c[2], c[3]), midv(c[0], c[2]), midv(c[1], c[3])
        g[1, 1] = nv
        nv += 1
        for cy in (0, 1):
            for cx in (0, 1):
                ev2.append([g[cy + (k >> 1), cx + (k & 1)] for k in range(4)])
                X2.append(W[cx, cy] @ Xp)
    return np.array(ev2), np.array(X2), nv


def topology(ev):
    """-> nbr [ne, 4] (-1: boundary), nface [ne, 4] the neighbour's local face, flip [ne, 4], corners: list over (e, k) of the sorted
    OTHER elements at that vertex"""
    ne = len(ev)
    edge, vel = {}, {}
    for e in range(ne):
        assert len(set(ev[e])) == 4, ("degenerate element", e)
        for f, (a, b) in enumerate(FACE):
            edge.setdefault(frozenset((ev[e, a], ev[e, b])), []).append((e, f))
        for k in range(4):
            vel.setdefault(ev[e, k], []).append(e)
    nbr = -np.ones((ne, 4), dtype=int)
    nface = np.zeros((ne, 4), dtype=int)
    flip = np.zeros((ne, 4), dtype=bool)
    for lst in edge.values():
        assert len(lst) <= 2, "an edge with more than two elements"
        if len(lst) == 2:
            assert lst[0][0] != lst[1][0], "an element that is its own neighbour"
            for (e, f), (g, h) in (lst, lst[::-1]):
                nbr[e, f], nface[e, f] = g, h
                flip[e, f] = ev[e, FACE[f][0]] != ev[g, FACE[h][0]]
    corners = [[sorted(g for g in vel[ev[e, k]] if g != e) for k in range(4)] for e in range(ne)]
    return nbr, nface, flip, corners


class QuadMesh:
    """stands where the oracle's Lattice stands: what Remhos.__init__ asks of it, plus the tables of topology()"""

    dim = 2
    mesh_order = 2

    def __init__(self, path, rs=0):
        ev, X, nv = read_mesh(path)
        topology(ev)  # (the refinement keys new vertices by the vertex pairs of the edges)
        for _ in range(rs):
            ev, X, nv = refine(ev, X, nv)
        J = np.stack([X[:, 5] - X[:, 3], X[:, 7] - X[:, 1]], axis=-1)
        if not (np.linalg.det(J) > 0).all():
            raise ValueError("clockwise element")
        self.ev, self.X0, self.nv = ev, X, nv
        self.ne = len(ev)
        self.n = (self.ne, 1)
        self.nbr, self.nface, self.flip, self.corners = topology(ev)
        self.periodic = bool((self.nbr >= 0).all())
        lo, hi = X.reshape(-1, 2).min(0), X.reshape(-1, 2).max(0)  # bounding box over the element nodes
        self.verts = [np.array([lo[d], hi[d]]) for d in range(2)]
        self.valence = {v: int((ev == v).sum()) for v in np.unique(ev)}

    def face_neighbors(self):
        return self.nbr

    def elem_node_ids(self):
        return np.arange(self.ne * 9).reshape(self.ne, 9)

    def lattice_nodes(self):
        return self.X0.reshape(-1, 2).copy()

    def csr(self):
        """the corner lists as the CSR of rmh_build_tables_quad: corner_ptr [4 ne + 1], corner_elems"""
        ptr, els = [0], []
        for row in self.corners:
            for lst in row:
                els += lst
                ptr.append(len(els))
        return np.array(ptr, dtype=np.int32), np.array(els, dtype=np.int32)

    def face_code(self):
        return np.where(self.nbr >= 0, self.nface + 4 * self.flip, 0).astype(np.uint8)


class UnstructuredRemhos(Remhos):
    def __init__(self, cfg: Config, mesh: QuadMesh):
        T_p = cfg.order
        D = T_p + 1
        it = np.arange(D)

        def layer(f):  # dofs of face f in the order of its tangential parameter
            lay = 0 if f % 2 == 0 else T_p
            return lay + D * it if f // 2 == 0 else it + D * lay

        self._own = [layer(f) for f in range(4)]
        # nbd[f][e, :] the neighbour's dofs that mirror the element's own face dofs; boundary faces get the element's own (masked)
        self._nbd = []
        for f in range(4):
            rows = np.array([layer(h) for h in range(4)])[mesh.nface[:, f]]
            self._nbd.append(np.where(mesh.flip[:, f, None], rows[:, ::-1], rows))
        # corner lists padded to a rectangle for the bounds
        w = max(1, max(len(lst) for row in mesh.corners for lst in row))
        self._cpad = -np.ones((mesh.ne, 4, w), dtype=int)
        for e, row in enumerate(mesh.corners):
            for k, lst in enumerate(row):
                self._cpad[e, k, :len(lst)] = lst
        super().__init__(cfg, mesh)

    def _mirrored(self, u, f):
        """u with the element's dofs on face f replaced by the neighbour's mirror dofs (0 on the domain boundary: u_nbr := 0)"""
        nb = self.nbr[:, f]
        out = u.copy()
        vals = u[np.maximum(nb, 0)[:, None], self._nbd[f]]
        out[:, self._own[f]] = np.where(nb[:, None] >= 0, vals, 0.0)
        return out

    def _submesh_boundary_mask(self):
        mesh, T = self.lat, self.T
        mask = np.zeros((mesh.ne, T.ndof), dtype=bool)
        bdr_v = set()
        for f in range(4):
            on = mesh.nbr[:, f] < 0
            mask[np.ix_(on, self._own[f])] = True
            for k in FACE[f]:
                bdr_v.update(mesh.ev[on, k])
        p = T.p
        for k, d in enumerate((0, p, (p + 1) * p, (p + 1) * p + p)):
            mask[:, d] |= np.isin(mesh.ev[:, k], list(bdr_v))
        return mask

    def face_apply(self, u):
        T = self.T
        y = np.zeros_like(u)
        for c in range(2):
            for side in (0, 1):
                F = T.PhiF[c, side]
                y += (self.sF[c, side] * ((self._mirrored(u, 2 * c + side) - u) @ F.T)) @ F
        return y

    def calc_lo_rd(self, u):
        T = self.T
        du_face = np.zeros_like(u)
        for c in range(2):
            for side in (0, 1):
                coef = self.sF[c, side] @ T.PhiF[c, side]
                du_face += coef * (self._mirrored(u, 2 * c + side) - u)
        # the element part is the lattice oracle's: run it with the face coefficients zeroed
        sF = self.sF
        self.sF = {k: np.zeros_like(v) for k, v in sF.items()}
        try:
            out = Remhos.calc_lo_rd(self, u)
        finally:
            self.sF = sF
        return out + du_face / self.m

    def bounds_from_extrema(self, xe_min, xe_max):
        if self.cfg.bounds_type == 1:
            return Remhos.bounds_from_extrema(self, xe_min, xe_max)
        T, p = self.T, self.T.p
        umin = np.repeat(xe_min[:, None], T.ndof, 1)
        umax = np.repeat(xe_max[:, None], T.ndof, 1)
        for f in range(4):
            nb = self.nbr[:, f]
            od = self._own[f]
            umin[:, od] = np.minimum(umin[:, od], np.where(nb >= 0, xe_min[np.maximum(nb, 0)], INF)[:, None])
            umax[:, od] = np.maximum(umax[:, od], np.where(nb >= 0, xe_max[np.maximum(nb, 0)], -INF)[:, None])
        cp = self._cpad
        cmin = np.where(cp >= 0, xe_min[np.maximum(cp, 0)], INF).min(-1)
        cmax = np.where(cp >= 0, xe_max[np.maximum(cp, 0)], -INF).max(-1)
        for k, d in enumerate((0, p, (p + 1) * p, (p + 1) * p + p)):
            umin[:, d] = np.minimum(umin[:, d], cmin[:, k])
            umax[:, d] = np.maximum(umax[:, d], cmax[:, k])
        return umin, umax


def make(mesh_name, rs, **kw):
    """UnstructuredRemhos on tests/golden/meshes/<mesh_name>.mesh; kw: the fields of oracle Config"""
    mesh = QuadMesh(os.path.join(MESH_DIR, mesh_name + ".mesh"), rs)
    return UnstructuredRemhos(Config(mesh=mesh_name, rs=rs, **kw), mesh)
