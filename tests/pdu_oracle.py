"""Numpy restatement of the reference's preconditioned DiscreteUpwind LO solver (-lo 2) and, on the CPU only, of its Neumann HO
solver (-ho 1) on the oracle's lattices.  A HELPER of tests/test_pdu_*.py and tests/test_gpu_pdu.py, not a test.

  -lo 2 (remhos.cpp:749-771, 937-942): the DiscreteUpwind class of -lo 1 (remhos_lo.cpp:31-100), handed another matrix: not the
      volume convection form but PrecondConvectionIntegrator (remhos_tools.cpp:975-1031), per element
          K_e = M_L,e M_e^-1 C_e,    M_e the consistent element mass, M_L,e its row-sum lumping (DenseMatrix::Lump),
      both integrated with the integrator's own rule on the mesh of the operator's time (reassembled every stage in remap mode,
      remhos.cpp:1639-1642).  The rule (remhos_tools.cpp:995-1001) has order
          max(OrderGrad(el) + Order + p, 2 p + OrderW) = max((k (d - 1) + p - 1) + k + p, 2 p + k d - 1) = 2 p + k d - 1
      on tensor elements of mesh order k [MFEM, IsoparametricTransformation]: with k = 2, order 2 p + 5 in 3-D and 2 p + 3 in 2-D --
      the rule of MassIntegrator and ConvectionIntegrator, i.e. the oracle's own tables (Tables.Q = p + 3 / p + 2 points a direction).
      Everything after the matrix is -lo 1: d_ij = max(0, -K_ij, -K_ji), D = K + d - rowsum(d), LinearFluxLumping with alpha = 0,
      division by the lumped mass.
  -ho 1 (remhos_ho.cpp:136-187; remhos.cpp:914-917): NeumannHOSolver with the consistent mass form m, the volume-only convection
      form k and the lumped mass: rhs = k u + LinearFluxLumping with alpha = 1, i.e. sum_j bdrInt_ij (u_j^nbr - u_j) with
      bdrInt = PhiF^T diag(s_F) PhiF (remhos_tools.cpp:847-856), then du = 0 and du -= (M du - rhs) / m_L for at most 20 iterations,
      stopping when the GLOBAL ||M du - rhs||_2 <= 1e-4.  It exists to reproduce the reference's printed values for its first
      regression method (autotest/test.sh:17, -ho 1 -lo 2 -fct 2); it is not a product path."""
import numpy as np

from tests.upwind_oracle import Config, UpwindRemhos  # noqa: F401  (Config is re-exported for the tests)


class PduRemhos(UpwindRemhos):
    """cfg.lo == 2 selects the preconditioned matrix; self.ho_type = 1 selects the Neumann iteration (default 3: the base
    class's local inverse)."""

    ho_type = 3

    # ---- matrices ----------------------------------------------------------------------------------------------------------
    def precond_conv_matrices(self):
        """K[e] = M_L M^-1 C (remhos_tools.cpp:1025-1030) with the integrator's rule -- the tables' rule, see the module text.
        One step of iterative refinement with the residual in extended precision keeps the restatement's own error of the
        solve well below cond(M) eps."""
        M = self.mass_matrices()
        Cm = self.conv_matrices()
        X = np.linalg.solve(M, Cm)
        ld = np.longdouble
        R = (Cm.astype(ld) - np.matmul(M.astype(ld), X.astype(ld))).astype(np.float64)
        X = X + np.linalg.solve(M, R)
        return M.sum(-1)[:, :, None] * X

    def mass_cond(self):
        """max_e cond_2(M_e): what the tolerance of the kernel tests is computed from"""
        return float(np.linalg.cond(self.mass_matrices()).max())

    # ---- -lo 2 -------------------------------------------------------------------------------------------------------------
    def calc_lo_upwind_prec(self, u, keep=None):
        """DiscreteUpwind::CalcLOSolution (remhos_lo.cpp:43-100) with the preconditioned matrix"""
        K = self._cached("K_prec", self.precond_conv_matrices)
        d = self._cached("d_prec", lambda: self._dij(K))
        conv = np.einsum("eij,ej->ei", K, u)
        du = conv + np.einsum("eij,ej->ei", d, u) - d.sum(-1) * u  # remhos_lo.cpp:52, 85-99
        face = self.lumped_face_fluxes(u)
        if keep is not None:
            keep.update(face=face, conv=conv)
        return (du + face) / self.m  # remhos_lo.cpp:72-73

    def lumped_face_fluxes(self, u):
        """LinearFluxLumping with alpha = 0 (remhos_tools.cpp:876-913): what calc_lo_upwind adds"""
        keep = {}
        self.calc_lo_upwind(u, keep)
        return keep["face"]

    # ---- -ho 1 -------------------------------------------------------------------------------------------------------------
    def calc_ho_neumann(self, u):
        """NeumannHOSolver::CalcHOSolution (remhos_ho.cpp:136-187)"""
        # k u + sum_F PhiF^T diag(s_F) PhiF (u^nbr - u): LinearFluxLumping with alpha = 1 (remhos_tools.cpp:900-912)
        rhs = self.conv_apply(u) + self.face_apply(u)
        self.last_rhs = rhs
        M = self.mass_matrices()
        du = np.zeros_like(u)
        for _ in range(20):
            res = np.einsum("eij,ej->ei", M, du) - rhs
            if np.sqrt((res * res).sum()) <= 1e-4:
                break
            du = du - res / self.m
        return du

    # ---- the stage --------------------------------------------------------------------------------------------------------------
    def stage(self, u, t, dt, keep=None):
        """AdvectionOperator::Mult (remhos.cpp:1596-1916) with lo 2 and / or ho 1; other combinations: the base classes"""
        cfg = self.cfg
        if cfg.lo != 2 and self.ho_type != 1:
            return super().stage(u, t, dt, keep)
        assert cfg.dt_control == 0
        if self.exec_mode == 1:
            self.update_geometry(t)
        du_ho = self.calc_ho_neumann(u) if self.ho_type == 1 else self.calc_ho(u)
        if cfg.lo == 2:
            du_lo = self.calc_lo_upwind_prec(u)
        elif cfg.lo == 1:
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


def neumann(cfg):
    """the restatement of a `-ho 1` run"""
    r = PduRemhos(cfg)
    r.ho_type = 1
    return r
