"""Numpy restatement of the reference's DiscreteUpwind LO solver (-lo 1) and FluxBasedFCT (-fct 1) on the oracle's lattices.
A HELPER of tests/test_upwind_*.py and tests/test_gpu_upwind.py, not a test.

  DiscreteUpwind::CalcLOSolution / ComputeDiscreteUpwindMatrix      remhos_lo.cpp:43-100
      K = k.SpMat(): the volume-only convection form (remhos.cpp:646-657, 931-935), block diagonal, reassembled on the moved
      mesh in remap mode (remhos.cpp:1616-1617, update_D); faces: Assembly::LinearFluxLumping with alpha = 0
      (remhos_tools.cpp:876-913), the lumped upwind face fluxes of the RD solvers.
  FluxBasedFCT::CalcFCTSolution                                     remhos_fct.cpp:155-181, 295-446
      K = K_HO.SpMat(): volume form + TransposeIntegrator(DGTraceIntegrator) on interior and boundary faces, neighbour block
      kept (remhos.cpp:659-679); M = M_HO.SpMat(), the consistent mass of the mesh at the operator's time (remhos.cpp:1621-1622);
      one FCT iteration (remhos.cpp:1093).

flux_based_fct is written in the GENERAL form: the entries of K_HO between the dofs of two face-neighbour elements
(k_ij, k_ji), the fluxes dt d_ij (u_i - u_j^nbr) they give and the neighbours' coefficients (remhos_fct.cpp:316-317, 406-409, 430-436)
are all there.  cross=False drops them; tests/test_upwind_oracle.py shows that every cross d_ij is exactly 0.0 and that dropping
them changes no bit, which is what licenses the element-local HIP kernels of remhos_amd/csrc/rmh_upwind.hpp.

A flux is stored "as its owner sees it": phi[e, i, j] = f_ij for the pair's lower global index and -f_ij for the other one, so
remhos_fct.cpp:366-377 (f >= 0: pos(i) += f, neg(j) -= f; else neg(i) += f, pos(j) -= f) is "every dof adds its positive and
its negative fluxes", and :428-441 gives the same a_ij from both sides (f_ij >= 0: min(pos_i, neg_j); seen from j the flux is
<= 0: min(neg_j, pos_i)).  Sums over j run in numpy's order, the reference's in CSR order: a difference at round-off."""
import numpy as np

from oracle.remhos_oracle import Config, Remhos  # noqa: F401  (Config is re-exported for the tests)


class UpwindRemhos(Remhos):
    def update_geometry(self, t):
        super().update_geometry(t)
        self._geo = {}  # matrices of this geometry, made on first use (transport: once per run)

    def _cached(self, key, make):
        if key not in self._geo:
            self._geo[key] = make()
        return self._geo[key]

    # ---- matrices ----------------------------------------------------------------------------------------------------------
    def conv_matrices(self):
        """K_vol[e, i, j] = sum_q Phi_i(q) sum_c D_c(q) d_c Phi_j(q): ConvectionIntegrator on the mesh of update_geometry
        (remhos.cpp:646-657; D_c: remhos_lo.cpp:1168-1188); conv_apply(u) is K_vol u"""
        T = self.T
        K = np.zeros((self.lat.ne, T.ndof, T.ndof))
        for c in range(self.dim):
            K += np.matmul(T.Phi.T[None, :, :] * self.Dq[:, None, :, c], T.dPhi[c])
        return K

    def own_face_blocks(self):
        """sum over the element's faces of PhiF^T diag(s_F) PhiF: minus this is the own-side part of the upwind DG trace form in
        K_HO (remhos.cpp:663-676; face_apply(u) = cross blocks . u_nbr - own blocks . u)"""
        T = self.T
        A = np.zeros((self.lat.ne, T.ndof, T.ndof))
        for c in range(self.dim):
            for side in (0, 1):
                P = T.PhiF[c, side]
                A += np.matmul(P.T[None, :, :] * self.sF[c, side][:, None, :], P)
        return A

    def cross_face_block(self, c, side):
        """k_ij between dof i of element e and dof j of its neighbour across face (c, side): sum_q s_F(q) Phi_i(q) Phi_j^nbr(q)
        (zero rows where there is no neighbour)"""
        T = self.T
        X = np.matmul(T.PhiF[c, side].T[None, :, :] * self.sF[c, side][:, None, :], T.PhiF[c, 1 - side])
        return np.where(self.nbr[:, 2 * c + side][:, None, None] >= 0, X, 0.0)

    def cross_dij(self, c, side):
        """d_ij = max(0, -k_ij, -k_ji) of the pairs across face (c, side) (remhos_fct.cpp:314-315); k_ji is the entry of the
        neighbour's row: its cross block across the opposite face, transposed"""
        nb = np.maximum(self.nbr[:, 2 * c + side], 0)
        kij = self.cross_face_block(c, side)
        kji = self.cross_face_block(c, 1 - side)[nb].transpose(0, 2, 1)
        d = np.maximum(np.maximum(0.0, -kij), -kji)
        return np.where(self.nbr[:, 2 * c + side][:, None, None] >= 0, d, 0.0)

    @staticmethod
    def _dij(K):
        """max(0, -k_ij, -k_ji) for i != j, 0 on the diagonal (remhos_lo.cpp:93-96, remhos_fct.cpp:315)"""
        d = np.maximum(np.maximum(0.0, -K), -K.transpose(0, 2, 1))
        d[:, np.arange(K.shape[1]), np.arange(K.shape[1])] = 0.0
        return d

    # ---- -lo 1 ------------------------------------------------------------------------------------------------------------------
    def calc_lo_upwind(self, u, keep=None):
        """DiscreteUpwind::CalcLOSolution (remhos_lo.cpp:43-100): du = [ D u + lumped face fluxes ] / m with
        D_ij = k_ij + d_ij (i != j), D_ii = k_ii - sum_{j != i} d_ij"""
        T = self.T
        K = self._cached("K_vol", self.conv_matrices)
        d = self._cached("d_vol", lambda: self._dij(K))
        du = np.einsum("eij,ej->ei", K, u) + np.einsum("eij,ej->ei", d, u) - d.sum(-1) * u  # remhos_lo.cpp:52, 85-99
        face = np.zeros_like(u)
        for c in range(self.dim):  # remhos_lo.cpp:63-70; remhos_tools.cpp:876-913 with alpha = 0
            for side in (0, 1):
                nb = self.nbr[:, 2 * c + side]
                coef = self.sF[c, side] @ T.PhiF[c, side]  # row sums of bdrInt (remhos_tools.cpp:847-856): zero off the face
                unb = np.where(nb[:, None] >= 0, u[np.maximum(nb, 0)][:, T.mirror[c]], 0.0)  # (inflow_gf = 0 for these problems)
                face += coef * (unb - u)
        if keep is not None:
            keep.update(face=face)
        return (du + face) / self.m  # remhos_lo.cpp:72-73

    # ---- -fct 1 -----------------------------------------------------------------------------------------------------------------
    def flux_based_fct(self, u, m, du_ho, du_lo, umin, umax, dt, cross=True, keep=None):
        """FluxBasedFCT::CalcFCTSolution, iter_cnt = 1 (remhos_fct.cpp:155-181)."""
        T, dim = self.T, self.dim
        M = self.mass_matrices()
        d = self._cached("d_ho", lambda: self._dij(self._cached("K_vol", self.conv_matrices) - self.own_face_blocks()))
        # ComputeFluxMatrix (:295-341): f_ij = dt d_ij (u_i - u_j) + M_ij dt (duH_i - duH_j)
        phi = (dt * d) * (u[:, :, None] - u[:, None, :]) + M * (dt * (du_ho[:, :, None] - du_ho[:, None, :]))
        phi[:, np.arange(T.ndof), np.arange(T.ndof)] = 0.0
        faces = [(c, side) for c in range(dim) for side in (0, 1)] if cross else []
        xphi, xnb = [], []
        for c, side in faces:  # the pairs across the faces: no mass entry (:316-319)
            nb = np.maximum(self.nbr[:, 2 * c + side], 0)
            dx = self._cached(("d_cross", c, side), lambda: self.cross_dij(c, side))
            xphi.append((dt * dx) * (u[:, :, None] - u[nb][:, None, :]))
            xnb.append(nb)
        # AddFluxesAtDofs (:343-380)
        gp = np.maximum(phi, 0.0).sum(-1)
        gm = np.minimum(phi, 0.0).sum(-1)
        for f in xphi:
            gp = gp + np.maximum(f, 0.0).sum(-1)
            gm = gm + np.minimum(f, 0.0).sum(-1)
        # ComputeFluxCoefficients (:382-399)
        u_lo = u + dt * du_lo
        max_pos = np.maximum((umax - u_lo) * m, 0.0)
        min_neg = np.minimum((umin - u_lo) * m, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            cp = np.where(gp > max_pos, max_pos / gp, 1.0)
            cn = np.where(gm < min_neg, min_neg / gm, 1.0)
        # UpdateSolutionAndFlux (:401-446)
        a = np.where(phi >= 0.0, np.minimum(cp[:, :, None], cn[:, None, :]), np.minimum(cn[:, :, None], cp[:, None, :]))
        acc = (a * phi / m[:, :, None] / dt).sum(-1)
        for f, nb in zip(xphi, xnb):
            a = np.where(f >= 0.0, np.minimum(cp[:, :, None], cn[nb][:, None, :]), np.minimum(cn[:, :, None], cp[nb][:, None, :]))
            acc = acc + (a * f / m[:, :, None] / dt).sum(-1)
        if keep is not None:
            keep.update(cross_d=[self._geo["d_cross", c, side] for c, side in faces], cp=cp, cn=cn)
        return du_lo + acc

    # ---- the stage --------------------------------------------------------------------------------------------------------------
    def stage(self, u, t, dt, keep=None):
        """AdvectionOperator::Mult (remhos.cpp:1596-1916) with lo 1 and / or fct 1; other combinations: the base class"""
        cfg = self.cfg
        if cfg.lo != 1 and cfg.fct != 1:
            return super().stage(u, t, dt, keep)
        assert cfg.dt_control == 0
        if self.exec_mode == 1:
            self.update_geometry(t)
        du_ho = self.calc_ho(u)
        if cfg.lo == 1:
            du_lo = self.calc_lo_upwind(u)
        elif cfg.lo == 5:
            du_lo = self.calc_lo_massavg(u, du_ho, dt)
        else:
            du_lo = self.calc_lo_rd(u)
        umin, umax = self.compute_bounds(u)
        if cfg.fct == 1:
            du = self.flux_based_fct(u, self.m, du_ho, du_lo, umin, umax, dt, cross=getattr(self, "cross", True))
        elif cfg.fct == 4:
            du = self.element_fct_projection(u, self.mass_matrices(), du_ho, du_lo, umin, umax, dt)
        else:
            du = self.clip_scale(u, self.m, du_ho, du_lo, umin, umax, dt)
        if keep is not None:
            keep.update(du_ho=du_ho, du_lo=du_lo, umin=umin, umax=umax, du=du, m=self.m.copy(), rhs=self.last_rhs)
        return du
