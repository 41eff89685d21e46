"""Numpy restatement of the reference's monolithic residual-distribution solver (-mono 1, MonolithicSolverType::ResDistMono) on the
oracle's lattices.  A HELPER of tests/test_mono_emu.py and tests/test_gpu_mono.py, not a test.

  MonoRDSolver::MonoRDSolver (scale)                                   remhos_mono.cpp:25-58
  MonoRDSolver::CalcSolution, subcell_scheme = false, no smoothness indicator   remhos_mono.cpp:60-356
      K_mat = k.SpMat(): the volume-only convection form (remhos.cpp:646-657, 1003), M_mat = m.SpMat() the consistent mass,
      M_lumped = lumpedM, all of the mesh at the operator's time (remhos.cpp:1616-1632)
  Assembly::NonlinFluxLumping                                          remhos_tools.cpp:915-973
      bdrInt of a face (remhos_tools.cpp:847-856) = PhiF^T diag(s_F) PhiF, inflow_gf = 0
  AdvectionOperator::Mult with a monolithic solver                     remhos.cpp:1687 (no LimitMult: RK3 SSP on the result)

Built on tests/upwind_oracle.py: conv_matrices (K_vol), the face speeds and traces of calc_lo_upwind, mass_matrices.

There is NO reference known answer for -mono 1 without -si: the reference's own test table runs the monolithic solver only with the
smoothness indicator, which is out of scope.  Fidelity rests on this reading of the source, line by line, and on the properties
tests/test_mono_emu.py checks (conservation, bounds over a run, determinism).  Sums over j run in numpy's order except the mass
row sum of the iteration, which runs j = s - 1 ... 0 like the reference's walk through the CSR row (remhos_mono.cpp:286-291).

scale (remhos_mono.cpp:37-57) needs MFEM's IntRules.Get(geom, OrderW + 2 p + 2 OrderGrad) and Mesh::GetElementSize; they are
restated here as order 6 dim + 4 p - 7 with order // 2 + 1 Gauss-Legendre points a direction and |det J(centre)|^(1/dim) -- not
verified against a build of the reference (MFEM is not available)."""
import numpy as np

from oracle.remhos_oracle import det, gauss_legendre_01, gll_nodes, kron_list, lagrange
from tests.upwind_oracle import Config, UpwindRemhos  # noqa: F401  (Config is re-exported for the tests)

MAX_PASSES = 101  # it = 0 ... max_iter = 100 (remhos_mono.cpp:64, 265)
TOL = 1e-8        # remhos_mono.cpp:68


class MonoRemhos(UpwindRemhos):
    mass_lim = True  # remhos.cpp:999 (false for problems 6 and 7 only)

    # ---- constructor ---------------------------------------------------------------------------------------------------------
    def mono_scale(self):
        """scale(e) = vmax_e / (2 sqrt(dim) h_e / order) on the initial mesh (remhos_mono.cpp:37-57)"""
        dim, p = self.dim, self.T.p
        nq = (6 * dim + 4 * p - 7) // 2 + 1
        xq, _ = gauss_legendre_01(nq)
        L, _ = lagrange(gll_nodes(self.lat.mesh_order), xq)
        xpts = np.einsum("qn,enc->eqc", kron_list([L] * dim), self.X0)
        v = self.vel(xpts)
        vmax = np.sqrt((v * v).sum(-1)).max(-1)
        J = np.stack([np.einsum("qn,enc->eqc", self.T.dPsiMid[c], self.X0) for c in range(dim)], axis=-1)
        h = np.abs(det(J[:, 0])) ** (1.0 / dim)  # GetElementSize(e)
        return vmax / (2.0 * (np.sqrt(dim) * h / p))

    # ---- matrices ----------------------------------------------------------------------------------------------------------
    def face_block(self, c, side):
        """bdrInt(k, BdrID, i, j) of the face (c, side) as an s x s matrix: zero rows and columns off the face"""
        P = self.T.PhiF[c, side]
        return np.matmul(P.T[None, :, :] * self.sF[c, side][:, None, :], P)

    @staticmethod
    def _balance(v, sp, sn, eps):
        """remhos_tools.cpp:958-970 / remhos_mono.cpp:329-339"""
        with np.errstate(divide="ignore", invalid="ignore"):
            pos = np.minimum(0.0, v) - np.maximum(0.0, v) * (sn / sp)[:, None]
            neg = np.maximum(0.0, v) - np.minimum(0.0, v) * (sp / sn)[:, None]
        tot = (sp + sn)[:, None]
        return np.where(tot > eps, pos, np.where(tot < -eps, neg, v))

    # ---- -mono 1 -----------------------------------------------------------------------------------------------------------------
    def calc_mono(self, u, mass_lim=None, scale=None, keep=None):
        """MonoRDSolver::CalcSolution.  Returns du; keep gets the pass counts [ne] (0 without mass_lim), converged [ne] and the
        residual norm of every pass [ne][101] (NaN where a pass was not run)."""
        T = self.T
        ne, s = u.shape
        mass_lim = self.mass_lim if mass_lim is None else mass_lim
        beta, eps = 10.0, 1e-15  # remhos_mono.cpp:68
        xe_min, xe_max = u.min(-1), u.max(-1)                      # :84-95
        xi_min, xi_max = self.bounds_from_extrema(xe_min, xe_max)  # :96-99
        K = self._cached("K_vol", self.conv_matrices)
        z = np.einsum("eij,ej->ei", K, u)  # :110
        d = z.copy()                       # :111
        up, dn = xi_max - u, u - xi_min
        alpha = np.minimum(1.0, beta * np.minimum(up, dn) / (np.maximum(up, dn) + eps))  # :128-131
        du = alpha * z     # :157
        z = z - alpha * z  # :158
        for c in range(self.dim):  # :162-166; NonlinFluxLumping, remhos_tools.cpp:915-973
            for side in (0, 1):
                b = self._cached(("bF", c, side), lambda: self.face_block(c, side))
                nb = self.nbr[:, 2 * c + side]
                xn = np.where(nb[:, None] >= 0, u[np.maximum(nb, 0)][:, T.mirror[c]], 0.0)  # (inflow_gf = 0)
                xdiff = xn - u                                                      # :938
                lump = (b * xdiff[:, :, None]).sum(-1)                              # :949
                corr = (b * (xdiff[:, None, :] - xdiff[:, :, None])).sum(-1)        # :950-951
                for y, al in ((du, alpha), (d, 1.0)):
                    ca = al * corr                                                  # :953
                    bal = self._balance(ca, np.maximum(0.0, ca).sum(-1), np.minimum(0.0, ca).sum(-1), eps)  # :954-970
                    y += lump
                    y += bal                                                        # :971
        rhoP, rhoN, xsum = np.maximum(0.0, z).sum(-1), np.minimum(0.0, z).sum(-1), u.sum(-1)  # :169-177
        sumWP = s * xe_max - xsum + eps  # :179
        sumWN = s * xe_min - xsum - eps  # :180
        wP = (xe_max[:, None] - u) / sumWP[:, None]  # :245
        wN = (xe_min[:, None] - u) / sumWN[:, None]  # :246
        du = du + (wP * rhoP[:, None] + wN * rhoN[:, None])  # :259
        ml = self.m
        m_it = np.zeros_like(u)  # :264
        passes = np.zeros(ne, dtype=np.int64)
        conv = np.ones(ne, dtype=bool)
        resid = np.full((ne, MAX_PASSES), np.nan)
        if mass_lim:
            M = self.mass_matrices()
            scale = self.mono_scale() if scale is None else scale
            gap = (beta * scale)[:, None] * np.minimum(xi_max - u, u - xi_min)  # :310-312
            diff = d - du                                                       # :292
            active = np.ones(ne, dtype=bool)
            conv[:] = False
            for it in range(MAX_PASSES):  # :265
                ud = (du + m_it) / ml     # :270
                udmin, udmax = ud.min(-1, keepdims=True), ud.max(-1, keepdims=True)  # :280-281
                acc = np.zeros_like(u)
                for j in range(s - 1, -1, -1):  # run backwards through columns (:286-291)
                    acc = acc + M[:, :, j] * (ud - ud[:, j:j + 1])
                acc = acc + np.minimum(1.0, np.maximum(0.0, np.abs(acc) / (np.abs(diff) + eps))) * diff  # eq. (27)-(29), tmp = 0 (:300)
                acc = acc * np.minimum(1.0, gap / (np.maximum(udmax - ud, ud - udmin) + eps))          # :310-313, 324
                new = self._balance(acc, np.maximum(0.0, acc).sum(-1), np.minimum(0.0, acc).sum(-1), eps)  # :325-339
                m_it = np.where(active[:, None], new, m_it)
                res = m_it + du - ml * ud                                                               # :344
                nrm = np.sqrt((res * res).sum(-1))
                resid[active, it] = nrm[active]
                passes[active] = it + 1
                done = active & (nrm <= TOL)                                                            # :347
                conv |= done
                active = active & ~done
                if not active.any():
                    break
        if keep is not None:
            keep.update(passes=passes, converged=conv, resid=resid, xi_min=xi_min, xi_max=xi_max, m=ml.copy())
        return (du + m_it) / ml  # :353

    # ---- the stage --------------------------------------------------------------------------------------------------------------
    def stage(self, u, t, dt, keep=None):
        """AdvectionOperator::Mult with a monolithic solver (remhos.cpp:1598-1687): the mesh of the stage time, then CalcSolution"""
        if self.exec_mode == 1:
            self.update_geometry(t)
        if not hasattr(self, "_scale0"):
            self._scale0 = self.mono_scale()
        return self.calc_mono(u, scale=self._scale0, keep=keep)
