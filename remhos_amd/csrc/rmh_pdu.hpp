// DiscreteUpwind::CalcLOSolution with the PRECONDITIONED convection matrix (-lo 2, "Preconditioned Discrete Upwind";
// remhos.cpp:749-771, 937-942, remhos_lo.cpp:31-100) for gfx950, dim = 3 (p <= 3) and dim = 2 (p <= 6).
//
// The reference builds -lo 2 from the DiscreteUpwind class of -lo 1 and hands it another matrix: not the volume convection form C
// but PrecondConvectionIntegrator (remhos_tools.cpp:975-1031), per element
//   K_e = M_L,e M_e^-1 C_e,     M_e = Phi^T diag(w detJ) Phi,   M_L,e = diag(M_e 1),   C_e = K_vol of rmh_upwind.hpp,
// assembled on the mesh of the operator's time (every stage in remap mode, remhos.cpp:1639-1642).  Everything after that is -lo 1:
//   d_ij = max(0, -K_ij, -K_ji),   du_i = [ sum_j K_ij u_j + sum_{j != i} d_ij (u_j - u_i) + sum_F c_i^F (u_i^nbr - u_i) ] / m_i
// with the lumped upwind face fluxes of LinearFluxLumping (alpha = 0) and the context's lumped mass m.
//
// The two rules.  The integrator picks its own rule (remhos_tools.cpp:995-1001):
//   order = max(OrderGrad(el) + Order + p, 2 p + OrderW).
// On tensor elements of mesh order k in dimension d [MFEM, IsoparametricTransformation]: OrderGrad(el) = k (d - 1) + p - 1,
// Order = k, OrderW = k d - 1, so both arguments of the max are 2 p + k d - 1.  With the reference's k = 2 (remhos.cpp:222):
//   dim = 3: order 2 p + 5, p + 3 Gauss points a direction;    dim = 2: order 2 p + 3, p + 2 points.
// The mass row of rmh_upwind.hpp / rmh_efp.hpp uses the rule of MassIntegrator, order 2 p + OrderW = 2 p + k d - 1: the SAME rule in
// both dimensions (EfpCfg::T: Q = P + 3 / P + 2).  M_e, M_L,e and C_e are therefore formed from the one geometry phase of
// rmh_upwind.hpp; no second table is needed.  tests/pdu_oracle.py reproduces the reference's printed answers with this rule.
//
// Work decomposition: one element per workgroup (EfpCfg), s = (p+1)^dim <= 64 dofs.  Unlike -lo 1, an s x s object is unavoidable:
// M_e^-1 couples every row of C_e.
//   A  geometry phase (upw_geometry, MASS); then the owner of row i (a wavefront) forms C_i., and M_i. in one sweep (upw_sweep):
//      C_i. goes to row i of sK, the lower triangle of M_i. to the packed factor sL (row-major, s (s + 1) / 2 doubles), the row
//      sum M_L,i to sML.
//   B  Cholesky M = L L^T in place in sL, left-looking, row i in lane i of wavefront 0; the diagonal slot keeps 1 / L_kk.
//      Hand-offs between the columns are wavefront-local fences.
//   C  X = M^-1 C_e: forward and back substitution in place in sK, COLUMN j in lane j -- a column's dependent chain stays in one
//      lane, the s columns run side by side; L_km is the same address in every lane (an LDS broadcast) and row m of sK is
//      contiguous over the lanes: no bank conflicts.  Dot products run in two accumulators to shorten the chain.
//   D  one walk, ROW i in lane i: K_ij = M_L,i X_ij and K_ji = M_L,j X_ji are read from the one matrix in LDS by both owners of a
//      pair, so d_ij = d_ji bit for bit; no atomics, the same bits from run to run.  The row stride SP of sK is odd, so the lanes of
//      a row-per-lane access (stride SP doubles) and of a column-per-lane access (stride 1) both fall on distinct banks.
//
// LDS bytes per (P, DIM), from the gfx950 code object (sK = s SP doubles, sL = s (s + 1) / 2; the rest: tables, nodes, D_c, w detJ,
// face speeds, sweep buffers, u, M_L, face coefficients and neighbours):
//   dim = 3   p = 1: 6 464     2: 19 624    3: 67 120
//   dim = 2   p = 1: 1 552     2: 3 064     3: 6 240     4: 12 912     5: 23 072     6: 38 176
// p = 3 in 3-D (s = 64: sK 33 280 B, sL 16 640 B) is above the 64 KB of earlier parts; gfx950 has 160 KiB per CU and launches STATIC
// allocations up to that size (no dynamic allocation, so no function attribute to raise); two such workgroups fit a CU, as
// many as 64 KB workgroups would.  dim = 3, p >= 4 (s = 125: sK alone 125 KB) is refused at the C ABI; a global-memory variant is not
// built.
#pragma once
#include "rmh_upwind.hpp"

namespace rmh
{

template <int P, int DIM>
struct PduCfg : UpwCfg<P, DIM, true>
{
   using U = UpwCfg<P, DIM, true>;
   static constexpr int S = U::S;
   static constexpr int SP = S | 1;           // row stride of the dense matrix (odd: see above)
   static constexpr int NL = S * (S + 1) / 2; // packed lower triangle
   static constexpr bool SUPPORTED = S <= 64;
   // multiply-adds of the dense part of an element, beside UpwCfg::ELEM_FMA (here: S sweeps with the mass row, S * SWEEP_FMA):
   // Cholesky sum_k (S - k) k = (S - 1) S (S + 1) / 6 and two triangular solves with S right-hand sides, S * S (S - 1) / 2 each --
   // in floating-point operations s^3 / 3 + 2 s^3 to leading order.
   static constexpr long long CHOL_FMA = (long long)(S - 1) * S * (S + 1) / 6;
   static constexpr long long SOLVE_FMA = (long long)S * S * (S - 1);
   static constexpr long long DENSE_FMA = CHOL_FMA + SOLVE_FMA;
   static constexpr long long ELEM_FMA = S * U::SWEEP_FMA + DENSE_FMA;
};

// DiscreteUpwind::CalcLOSolution, preconditioned matrix.  m: the lumped mass M 1 of the same geometry (the context's).
template <int P, int DIM>
__global__ void __launch_bounds__((EfpCfg<P, DIM>::NT)) lo_upwind_prec_kernel(UpwArgs a, const double *u, const double *m, double *du_lo)
{
   using C = PduCfg<P, DIM>;
   using T = typename C::T;
   constexpr int D = C::D, Q = C::Q, D2 = C::D2, S = C::S, SP = C::SP, NT = C::NT, NW = C::NW, NF = C::NF, QF = C::QF, DF = C::DF;
   static_assert(S <= 64, "one row / column per lane of a wavefront");
   __shared__ double sTab[C::NTAB];
   __shared__ double sX[C::NN], sV[C::NN];
   __shared__ double sD[DIM * C::NQ], sW[C::NQ];
   __shared__ double sF[NF * QF];
   __shared__ double sBuf[NW * (C::NT1 + C::NT2)];
   __shared__ double sK[S * SP];
   __shared__ double sL[C::NL];
   __shared__ double sU[S], sML[S], sCf[NF * DF], sNb[NF * DF];
   const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
   const size_t e = blockIdx.x;
   for (int i = tid; i < S; i += NT) { sU[i] = u[e * S + i]; }
   // the mirrored face dofs of the face neighbours (0 on the domain boundary), as in lo_upwind_kernel
   for (int k = tid; k < NF * DF; k += NT)
   {
      const int f = k / DF, r = k % DF, c = f >> 1, side = f & 1;
      const int nb = a.face_nbr[e * NF + f];
      double v = 0.0;
      if (nb >= 0)
      {
         int off;
         if (DIM == 3)
         {
            const int i1 = r % D, i2 = r / D;
            const int stc = c == 0 ? 1 : (c == 1 ? D : D2), st1 = c == 0 ? D : (c == 1 ? D2 : 1), st2 = c == 0 ? D2 : (c == 1 ? 1 : D);
            off = (side ? 0 : P) * stc + i1 * st1 + i2 * st2;
         }
         else
         {
            const int layer = side ? 0 : P;
            off = c == 0 ? layer + D * r : r + D * layer;
         }
         const bool ghost = nb >= a.ne_owned;
         const double *un = ghost ? a.u_ghost + (size_t)(nb - a.ne_owned) * a.gh_ustride : u + (size_t)nb * S;
         v = un[(ghost && a.gh_compact) ? r : off];
      }
      sNb[k] = v;
   }
   upw_geometry<P, DIM, true>(a, e, sTab, sX, sV, sD, sW, sF);
   const double *tB = sTab + T::oB, *tG = sTab + T::oG;
   // lumped face coefficients c^F = B_F^T s_F (row sums of bdrInt, remhos_tools.cpp:847-856)
   for (int k = tid; k < NF * DF; k += NT)
   {
      const int f = k / DF, r = k % DF;
      const int i1 = r % D, i2 = r / D; // (dim = 2: i2 = 0)
      double acc = 0.0;
      if (DIM == 3)
      {
         for (int q2 = 0; q2 < Q; q2++)
         {
            double in = 0.0;
            for (int q1 = 0; q1 < Q; q1++) { in += sF[f * QF + q1 + Q * q2] * tB[q1 * D + i1]; }
            acc += tB[q2 * D + i2] * in;
         }
      }
      else
      {
         for (int q1 = 0; q1 < Q; q1++) { acc += sF[f * QF + q1] * tB[q1 * D + i1]; }
      }
      sCf[k] = acc;
   }
   // ---- A: C_e, the lower triangle of M_e and M_L,e -------------------------------------------------------------------------
   {
      double *t1 = sBuf + wv * (C::NT1 + C::NT2), *t2 = t1 + C::NT1;
      double kr[1], kc[1], mr[1];
      for (int r = 0; r < C::ROUNDS; r++)
      {
         const int i = r * NW + wv;
         if (i >= S) { continue; }
         upw_sweep<P, DIM, true>(i, lane, tB, tG, sD, sW, t1, t2, kr, kc, mr);
         if (lane < S)
         {
            sK[i * SP + lane] = kr[0];
            if (lane <= i) { sL[i * (i + 1) / 2 + lane] = mr[0]; } // (M_ij = M_ji bit for bit: upw_sweep)
         }
         const double ml = block_sum<1>(mr[0], nullptr); // (lanes >= S hold 0)
         if (lane == 0) { sML[i] = ml; }
      }
   }
   __syncthreads();
   // ---- B: M = L L^T, left-looking; lane i of wavefront 0 owns row i ---------------------------------------------------------
   if (wv == 0)
   {
      const bool on = lane < S;
      const double *Li = sL + (on ? lane * (lane + 1) / 2 : 0);
      for (int k = 0; k < S; k++)
      {
         const double *Lk = sL + k * (k + 1) / 2;
         double s0 = 0.0, s1 = 0.0;
         if (on && lane >= k)
         {
            s0 = Li[k];
            int mm = 0;
#pragma unroll 4
            for (; mm + 1 < k; mm += 2)
            {
               s0 = fma(-Li[mm], Lk[mm], s0);
               s1 = fma(-Li[mm + 1], Lk[mm + 1], s1);
            }
            if (mm < k) { s0 = fma(-Li[mm], Lk[mm], s0); }
            s0 += s1;
         }
         const double rinv = 1.0 / sqrt(__shfl(s0, k)); // (M_e is positive definite: w detJ > 0)
         if (on && lane == k) { sL[k * (k + 1) / 2 + k] = rinv; }
         else if (on && lane > k) { sL[lane * (lane + 1) / 2 + k] = s0 * rinv; }
         wave_lds_fence(); // (column k + 1 reads row k + 1, which lane k + 1 has just completed)
      }
   }
   __syncthreads();
   // ---- C: X = M^-1 C_e in place; thread j owns column j ---------------------------------------------------------------------
   if (tid < S)
   {
      double *col = sK + tid;
      for (int k = 0; k < S; k++) // L y = c
      {
         const double *Lk = sL + k * (k + 1) / 2;
         double s0 = col[k * SP], s1 = 0.0;
         int mm = 0;
#pragma unroll 4
         for (; mm + 1 < k; mm += 2)
         {
            s0 = fma(-Lk[mm], col[mm * SP], s0);
            s1 = fma(-Lk[mm + 1], col[(mm + 1) * SP], s1);
         }
         if (mm < k) { s0 = fma(-Lk[mm], col[mm * SP], s0); }
         col[k * SP] = (s0 + s1) * Lk[k];
      }
      for (int k = S - 1; k >= 0; k--) // L^T x = y
      {
         double s0 = col[k * SP], s1 = 0.0;
         int mm = k + 1;
#pragma unroll 4
         for (; mm + 1 < S; mm += 2)
         {
            s0 = fma(-sL[mm * (mm + 1) / 2 + k], col[mm * SP], s0);
            s1 = fma(-sL[(mm + 1) * (mm + 2) / 2 + k], col[(mm + 1) * SP], s1);
         }
         if (mm < S) { s0 = fma(-sL[mm * (mm + 1) / 2 + k], col[mm * SP], s0); }
         col[k * SP] = (s0 + s1) * sL[k * (k + 1) / 2 + k];
      }
   }
   __syncthreads();
   // ---- D: the walk; thread i owns row i --------------------------------------------------------------------------------------
   if (tid < S)
   {
      const int i = tid;
      const double ui = sU[i], mli = sML[i];
      double acc = 0.0;
      for (int j = 0; j < S; j++)
      {
         const double kij = mli * sK[i * SP + j], kji = sML[j] * sK[j * SP + i]; // K = M_L M^-1 C (remhos_tools.cpp:1025-1030)
         const double uj = sU[j];
         const double dij = j != i ? fmax(fmax(0.0, -kij), -kji) : 0.0; // remhos_lo.cpp:90-96
         acc += fma(kij, uj, dij * (uj - ui));
      }
      const int ii[3] = {i % D, DIM == 3 ? (i / D) % D : i / D, DIM == 3 ? i / D2 : 0};
      double face = 0.0;
#pragma unroll
      for (int c = 0; c < DIM; c++)
      {
         if (ii[c] != 0 && ii[c] != P) { continue; }
         const int c1 = DIM == 3 ? (c + 1) % 3 : 1 - c, c2 = DIM == 3 ? (c + 2) % 3 : c1;
         const int k = (2 * c + (ii[c] == P ? 1 : 0)) * DF + ii[c1] + (DIM == 3 ? D * ii[c2] : 0);
         face += sCf[k] * (sNb[k] - ui);
      }
      store_stream(du_lo + e * S + i, (acc + face) / m[e * S + i]);
   }
}

} // namespace rmh
