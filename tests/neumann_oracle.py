"""The Neumann HO solver (-ho 1) of tests/pdu_oracle.py with what the kernel tests need beside du: the number of updates, the
residual norm of every check, and the amplification factor the tolerance is computed from.  A HELPER of
tests/test_neumann_emu.py, tests/test_gpu_neumann.py, not a test."""
import numpy as np

from tests.pdu_oracle import Config, PduRemhos  # noqa: F401  (Config is re-exported for the tests)

MAX_UPDATES, TOL = 20, 1e-4  # remhos_ho.cpp:165-166


class NeumannRemhos(PduRemhos):
    ho_type = 1

    def calc_ho_neumann_info(self, u):
        """calc_ho_neumann, operation by operation; returns (du, updates applied, the norms of the checks that were evaluated)"""
        rhs = self.conv_apply(u) + self.face_apply(u)
        M = self.mass_matrices()
        du = np.zeros_like(u)
        norms, updates = [], 0
        for _ in range(MAX_UPDATES):
            res = np.einsum("eij,ej->ei", M, du) - rhs
            norms.append(float(np.sqrt((res * res).sum())))
            if norms[-1] <= TOL:
                break
            du = du - res / self.m
            updates += 1
        return du, updates, np.array(norms)

    def amplification(self):
        """max_e sum_{k < 20} ||(I - M_L^-1 M_e)^k||_inf: how far the rounding error of one update can grow through the
        remaining ones"""
        M = self.mass_matrices()
        G = np.eye(M.shape[1])[None, :, :] - M / self.m[:, :, None]
        Gk = np.broadcast_to(np.eye(M.shape[1]), M.shape).copy()
        amp = np.zeros(M.shape[0])
        for _ in range(MAX_UPDATES):
            amp += np.abs(Gk).sum(-1).max(-1)
            Gk = np.matmul(Gk, G)
        return float(amp.max())


def neumann_tol(r):
    """relative to max|du|: 256 amp 2^-53 -- 256 for the few hundred products that each mass apply and the right-hand side sum
    in another order than the restatement"""
    return max(1e-12, 256.0 * r.amplification() * 2.0**-53)
