// DiscreteUpwind::CalcLOSolution (-lo 1; remhos_lo.cpp:31-100) and FluxBasedFCT::CalcFCTSolution (-fct 1, one FCT iteration;
// remhos_fct.cpp:155-181, 295-446, remhos.cpp:1093) for gfx950, dim = 3 and dim = 2.
//
// The reference writes both for an assembled CSR matrix.  On tensor lattices neither needs one:
//   * DiscreteUpwind is built from k, the volume-only convection form (remhos.cpp:646-657, 931-935): block diagonal.  Its face
//     part is Assembly::LinearFluxLumping with alpha = 0 (remhos_tools.cpp:876-913): c_i^F (u_i^nbr - u_i), c^F = B_F^T s_F.
//   * FluxBasedFCT is built from K_HO.  Its entries between the dofs of two elements are sum_q s_F(q) phi_i(q) phi_j^nbr(q) with
//     the upwind face speed s_F >= 0 and Bernstein traces >= 0, so k_ij >= 0, k_ji >= 0 and d_ij = max(0, -k_ij, -k_ji) = 0: every
//     flux between two elements is exactly zero (the mass part of the fluxes is element-local, remhos_fct.cpp:323-340) and the
//     neighbours' coefficients (:406-409) are never used.  tests/test_upwind_oracle.py proves this on the general restatement.
// So both are element-local limiters over the dense pairs (i, j) of an element, the family of rmh_efp.hpp, with
//   K^e = K_vol [ - sum_{own faces} B_F^T diag(s_F) B_F   for -fct 1 ],   K_vol_ij = sum_q Phi_i(q) sum_c D_c(q) d_c Phi_j(q),
//   D_c = alpha w (adj J v)_c (remhos_lo.cpp:1168-1188),   d_ij = max(0, -K_ij, -K_ji).
//
// Work decomposition (EfpCfg): one element per workgroup of NW wavefronts; nothing of size s x s is stored.  The geometry phase
// puts D_c, w detJ (FCT) and the upwind speeds s_F of the own faces into LDS, from x0 + t vel (remap) or the nodal velocity
// (transport) at the pseudo-time of the last rmh_setup -- the interpolation of the HO and RD kernels, evaluated point by point.
// The owner of row i (a wavefront) then forms by sum factorisation, in one sweep,
//   the ROW  K_i. = sum_c G_c^T (D_c Phi_i),   the COLUMN  K_.i = B^T (sum_c D_c d_c Phi_i)   and (FCT) the mass row M_i.,
// entry j in lane j mod 64.  dim = 3 sweeps slab by slab (one qz at a time: x- and y-contraction of the slab in LDS, the
// z-contraction accumulates in registers), which keeps the row buffers at (7 D Q + 5 D^2) doubles per wavefront -- efp_row's
// whole-row buffers beside three D_c arrays would not fit 64 KB of LDS at p = 6, so the mass row rides along in the same sweep
// with efp_row's factors (B_i B_j formed as products first: M_ij = M_ji bit for bit).
//
// The pair value d_ij is CANONICAL: an entry K_ab is the same chain of fma() calls on the same operands whether the owner of a
// forms it in its row sweep or the owner of b in its column sweep (test index a takes B, trial index b takes G, factors are
// formed as products first), and the face block is symmetric by construction.  Both owners of a pair therefore see the same
// d_ij and M_ij, the flux f_ij = dt d_ij (u_i - u_j) + M_ij dt (duH_i - duH_j) is exactly antisymmetric, and there are no
// atomics: the same bits from run to run.
//
// lo_upwind_kernel: one walk over the rows:   du_i = [ sum_j K_ij u_j + sum_{j != i} d_ij (u_j - u_i) + sum_F c_i^F (u_i^nbr - u_i) ] / m_i
// fct_fluxbased_kernel: two walks (the projection kernel's pass 0 -- row sums and z -- has no counterpart: m is an argument):
//   pass 1  the sign-split flux sums, the coefficients against m (u_max - u_lo), m (u_min - u_lo)   (remhos_fct.cpp:343-399)
//   pass 2  du_i = du_lo_i + sum_j a_ij f_ij / (m_i dt)                                             (:401-446)
#pragma once
#include "rmh_efp.hpp"
#include "rmh_stream.hpp"

namespace rmh
{

template <int P, int DIM, bool MASS>
struct UpwCfg : EfpCfg<P, DIM>
{
   using E = EfpCfg<P, DIM>;
   static constexpr int NF = 2 * DIM;                         // faces
   static constexpr int QF = DIM == 3 ? E::Q2 : E::Q;         // quadrature points of a face
   static constexpr int DF = DIM == 3 ? E::D2 : E::D;         // dofs of a face layer
   static constexpr int NA1 = 2 * DIM + (MASS ? 1 : 0);       // x-contracted arrays: row and column per component, mass
   static constexpr int NA2 = DIM == 3 ? 4 + (MASS ? 1 : 0) : 0; // xy-contracted arrays of a slab (dim = 3): row xy, z; column xy, z; mass
   static constexpr int NT1 = NA1 * E::D * E::Q, NT2 = NA2 * E::D2;
   // multiply-adds of one row sweep (row + column [+ mass]) and of an element (the figures of profiles/upwind_kernel_stats.txt)
   static constexpr long long SWEEP_FMA =
      DIM == 3 ? (long long)E::Q * ((long long)NT1 * E::Q + (long long)(6 + (MASS ? 1 : 0)) * E::Q * E::D2 + (long long)NA2 * E::S)
               : (long long)NT1 * E::Q + (long long)NA1 * E::Q * E::S;
   static constexpr long long ELEM_FMA = (MASS ? 2 : 1) * E::S * SWEEP_FMA;
};

struct UpwArgs
{
   const double *x0, *vel; // the element nodes as the context keeps them (dim = 3: hierarchical along `hier`, rmh_efp.hpp)
   const double *tab;
   double t;
   int move, hier;
   double alpha;           // -1 transport, +1 remap (remhos.cpp:648-657); also the sign of the upwind side
   const int *face_nbr;    // [ne][2 dim]
   int ne_owned;
   const double *u_ghost;  // ghost elements (dim = 3): see HoArgs, rmh_kernels.hpp
   int gh_ustride, gh_compact;
};

// adj(J) v and det J at the reference point whose 1-D mesh-basis rows are l[c], d[c] (values, derivatives along direction c)
template <int DIM>
__device__ inline void upw_point(const double *sX, const double *sV, const double (&l)[3][3], const double (&d)[3][3],
                                 double (&av)[DIM], double &detJ)
{
   if (DIM == 3)
   {
      double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, v[3] = {0, 0, 0};
#pragma unroll
      for (int az = 0; az < 3; az++)
      {
#pragma unroll
         for (int ay = 0; ay < 3; ay++)
         {
#pragma unroll
            for (int ax = 0; ax < 3; ax++)
            {
               const int n = ax + 3 * ay + 9 * az;
               const double w = l[0][ax] * l[1][ay] * l[2][az];
               const double w0 = d[0][ax] * l[1][ay] * l[2][az], w1 = l[0][ax] * d[1][ay] * l[2][az], w2 = l[0][ax] * l[1][ay] * d[2][az];
#pragma unroll
               for (int c = 0; c < 3; c++)
               {
                  const double x = sX[c * 27 + n];
                  J[c][0] += w0 * x;
                  J[c][1] += w1 * x;
                  J[c][2] += w2 * x;
                  v[c] += w * sV[c * 27 + n];
               }
            }
         }
      }
      // remhos_lo.cpp:1168-1188
      av[0] = (J[1][1] * J[2][2] - J[1][2] * J[2][1]) * v[0] + (J[2][1] * J[0][2] - J[0][1] * J[2][2]) * v[1] + (J[0][1] * J[1][2] - J[1][1] * J[0][2]) * v[2];
      av[1] = (J[2][0] * J[1][2] - J[1][0] * J[2][2]) * v[0] + (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * v[1] + (J[1][0] * J[0][2] - J[0][0] * J[1][2]) * v[2];
      av[DIM - 1] = (J[1][0] * J[2][1] - J[2][0] * J[1][1]) * v[0] + (J[2][0] * J[0][1] - J[0][0] * J[2][1]) * v[1] + (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * v[2];
      detJ = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
             J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
   }
   else
   {
      double J[2][2] = {{0, 0}, {0, 0}}, v[2] = {0, 0};
#pragma unroll
      for (int ay = 0; ay < 3; ay++)
      {
#pragma unroll
         for (int ax = 0; ax < 3; ax++)
         {
            const int n = ax + 3 * ay;
            const double w = l[0][ax] * l[1][ay], w0 = d[0][ax] * l[1][ay], w1 = l[0][ax] * d[1][ay];
#pragma unroll
            for (int c = 0; c < 2; c++)
            {
               const double x = sX[c * 9 + n];
               J[c][0] += w0 * x;
               J[c][1] += w1 * x;
               v[c] += w * sV[c * 9 + n];
            }
         }
      }
      av[0] = J[1][1] * v[0] - J[0][1] * v[1]; // remhos_lo.cpp:1113-1132
      av[1] = -J[1][0] * v[0] + J[0][0] * v[1];
      detJ = J[0][0] * J[1][1] - J[0][1] * J[1][0];
   }
}

// Geometry phase: tables, nodes, D_c = alpha w (adj J v)_c at the quadrature points (sD[c * NQ + q]), w detJ (sW, MASS only)
// and the upwind speeds of the own faces, sF[f * QF + q1 (+ Q q2)] = w_F max(0, alpha n_out . v), f = 2 c + side, face points
// along the directions (c + 1) % 3, (c + 2) % 3 (dim = 2: along 1 - c).  Called by every thread; ends with a barrier.
template <int P, int DIM, bool MASS>
__device__ inline void upw_geometry(const UpwArgs &a, size_t e, double *sTab, double *sX, double *sV, double *sD, double *sW,
                                    double *sF)
{
   using C = UpwCfg<P, DIM, MASS>;
   using T = typename C::T;
   constexpr int Q = C::Q, Q2 = C::Q2, NT = C::NT, NN = C::NN, NQ = C::NQ, QF = C::QF;
   const int tid = threadIdx.x;
   for (int i = tid; i < C::NTAB; i += NT) { sTab[i] = a.tab[i]; }
   for (int i = tid; i < NN; i += NT)
   {
      const double x = a.x0[e * NN + i], v = a.vel[e * NN + i];
      sX[i] = a.move ? x + a.t * v : x;
      sV[i] = v;
   }
   __syncthreads();
   if (DIM == 3)
   {
      for (int dir = 2; dir >= 0; dir--) // (the hierarchical node basis of the context, undone as in fct_projection_kernel)
      {
         if (!((a.hier >> dir) & 1)) { continue; }
         const int st = dir == 0 ? 1 : (dir == 1 ? 3 : 9);
         for (int i = tid; i < 81; i += NT)
         {
            const int k = ((i % 27) / st) % 3;
            if (k > 0) { sX[i] += sX[i - k * st]; sV[i] += sV[i - k * st]; }
         }
         __syncthreads();
      }
   }
   const double *tL = sTab + T::oL, *tdL = sTab + T::odL, *tW = sTab + T::oW;
   for (int q = tid; q < NQ; q += NT)
   {
      const int qi[3] = {q % Q, (q / Q) % Q, q / Q2};
      double l[3][3], d[3][3], w = 1.0;
#pragma unroll
      for (int c = 0; c < DIM; c++)
      {
#pragma unroll
         for (int k = 0; k < 3; k++) { l[c][k] = tL[qi[c] * 3 + k]; d[c][k] = tdL[qi[c] * 3 + k]; }
         w *= tW[qi[c]];
      }
      double av[DIM], detJ;
      upw_point<DIM>(sX, sV, l, d, av, detJ);
#pragma unroll
      for (int c = 0; c < DIM; c++) { sD[c * NQ + q] = a.alpha * w * av[c]; }
      if (MASS) { sW[q] = w * detJ; }
   }
   for (int k = tid; k < C::NF * QF; k += NT)
   {
      const int f = k / QF, r = k % QF, c = f >> 1, side = f & 1;
      const int q1 = r % Q, q2 = r / Q; // (dim = 2: q2 = 0)
      const int c1 = DIM == 3 ? (c + 1) % 3 : 1 - c;
      double l[3][3], d[3][3];
      // direction c: the quadratic mesh basis on {0, 1/2, 1} and its derivative at xi_c = side; the others: the rule's points
      // (every index of l / d is a compile-time constant: no scratch)
      const double ln[3] = {side ? 0.0 : 1.0, 0.0, side ? 1.0 : 0.0}, dn[3] = {side ? 1.0 : -3.0, side ? -4.0 : 4.0, side ? 3.0 : -1.0};
#pragma unroll
      for (int dd = 0; dd < DIM; dd++)
      {
         const int qd = dd == c1 ? q1 : q2;
#pragma unroll
         for (int kk = 0; kk < 3; kk++)
         {
            l[dd][kk] = dd == c ? ln[kk] : tL[qd * 3 + kk];
            d[dd][kk] = dd == c ? dn[kk] : tdL[qd * 3 + kk];
         }
      }
      double av[DIM], detJ;
      upw_point<DIM>(sX, sV, l, d, av, detJ);
      const double wF = DIM == 3 ? tW[q1] * tW[q2] : tW[q1];
      const double vn = (side ? 1.0 : -1.0) * (c == 0 ? av[0] : (c == 1 ? av[1] : av[DIM - 1])); // area-weighted outward normal . v: row c of adj(J)
      sF[k] = wF * fmax(0.0, a.alpha * vn);
   }
   __syncthreads();
}

// One sweep of the owner of row i: kr[k] = K_vol(i, j), kc[k] = K_vol(j, i) and (MASS) mr[k] = M(i, j) for j = lane + 64 k.
// t1 / t2: this wavefront's OWN LDS buffers (NT1 / NT2 doubles): the hand-offs between the contractions stay inside the
// wavefront (wave_lds_fence, rmh_stream.hpp), so the wavefronts of a workgroup walk their rows without meeting.
// Every entry K_vol(a, b) is the same chain of fma() on the same operands in the row sweep of a and the column sweep of b.
template <int P, int DIM, bool MASS>
__device__ inline void upw_sweep(int i, int lane, const double *B, const double *G, const double *sD, const double *sW, double *t1,
                                 double *t2, double (&kr)[EfpCfg<P, DIM>::JPL], double (&kc)[EfpCfg<P, DIM>::JPL],
                                 double (&mr)[EfpCfg<P, DIM>::JPL])
{
   using C = UpwCfg<P, DIM, MASS>;
   constexpr int D = C::D, Q = C::Q, D2 = C::D2, S = C::S, NQ = C::NQ, DQ = D * Q;
   const int ix = i % D, iy = DIM == 3 ? (i / D) % D : i / D, iz = DIM == 3 ? i / D2 : 0;
#pragma unroll
   for (int k = 0; k < C::JPL; k++) { kr[k] = 0.0; kc[k] = 0.0; mr[k] = 0.0; }
   for (int qz = 0; qz < (DIM == 3 ? Q : 1); qz++)
   {
      // x-contraction of the slab: t1[arr][vx + D qy]; arr = comp (row), DIM + comp (column), 2 DIM (mass)
      for (int k = lane; k < C::NT1; k += 64)
      {
         const int arr = k / DQ, r = k % DQ, vx = r % D, qy = r / D;
         const bool mass = arr == 2 * DIM, col = !mass && arr >= DIM;
         const int comp = arr % DIM;
         const double *src = (mass ? sW : sD + comp * NQ) + Q * (qy + Q * qz);
         // (test index takes B, trial index takes G along the component's own direction)
         const double *ta = B + (col ? vx : ix), *tb = ((!mass && comp == 0) ? G : B) + (col ? ix : vx);
         double acc = 0.0;
#pragma unroll
         for (int qx = 0; qx < Q; qx++) { acc = fma(src[qx], ta[qx * D] * tb[qx * D], acc); }
         t1[k] = acc;
      }
      wave_lds_fence();
      if (DIM == 3)
      {
         // y-contraction: t2[0] row (x + y components), t2[1] row (z component), t2[2], t2[3] column, t2[4] mass
         for (int k = lane; k < C::NT2; k += 64)
         {
            const int arr = k / D2, r = k % D2, vx = r % D, vy = r / D;
            const bool mass = arr == 4, col = arr == 2 || arr == 3, zc = arr == 1 || arr == 3;
            const double *ta = B + (col ? vy : iy), *tbB = B + (col ? iy : vy), *tbG = G + (col ? iy : vy);
            const double *s0 = t1 + (mass ? 6 : (col ? 3 : 0) + (zc ? 2 : 0)) * DQ + vx, *s1 = s0 + DQ;
            double acc = 0.0;
            if (mass || zc)
            {
#pragma unroll
               for (int qy = 0; qy < Q; qy++) { acc = fma(ta[qy * D] * tbB[qy * D], s0[D * qy], acc); }
            }
            else
            {
#pragma unroll
               for (int qy = 0; qy < Q; qy++)
               {
                  acc = fma(ta[qy * D] * tbB[qy * D], s0[D * qy], acc);
                  acc = fma(ta[qy * D] * tbG[qy * D], s1[D * qy], acc);
               }
            }
            t2[k] = acc;
         }
         wave_lds_fence();
#pragma unroll
         for (int k = 0; k < C::JPL; k++)
         {
            const int j = lane + 64 * k;
            if (j < S)
            {
               const int jxy = j % D2, vz = j / D2;
               const double bi = B[qz * D + iz], bv = B[qz * D + vz], bb = bi * bv;
               kr[k] = fma(bb, t2[jxy], kr[k]);
               kr[k] = fma(bi * G[qz * D + vz], t2[D2 + jxy], kr[k]);
               kc[k] = fma(bb, t2[2 * D2 + jxy], kc[k]);
               kc[k] = fma(bv * G[qz * D + iz], t2[3 * D2 + jxy], kc[k]);
               if (MASS) { mr[k] = fma(bb, t2[(MASS ? 4 : 0) * D2 + jxy], mr[k]); }
            }
         }
      }
      else
      {
         const int j = lane; // (D^2 <= 49: one entry per lane)
         if (j < S)
         {
            const int vx = j % D, vy = j / D;
#pragma unroll
            for (int qy = 0; qy < Q; qy++)
            {
               const double bi = B[qy * D + iy], bv = B[qy * D + vy], bb = bi * bv;
               kr[0] = fma(bb, t1[vx + D * qy], kr[0]);
               kr[0] = fma(bi * G[qy * D + vy], t1[DQ + vx + D * qy], kr[0]);
               kc[0] = fma(bb, t1[2 * DQ + vx + D * qy], kc[0]);
               kc[0] = fma(bv * G[qy * D + iy], t1[3 * DQ + vx + D * qy], kc[0]);
               if (MASS) { mr[0] = fma(bb, t1[(MASS ? 4 : 0) * DQ + vx + D * qy], mr[0]); }
            }
         }
         wave_lds_fence(); // (the next row's x-contraction writes t1)
      }
   }
}

// sum over the own faces that hold both i and j of (B_F^T diag(s_F) B_F)(i, j): symmetric in (i, j) bit for bit
template <int P, int DIM>
__device__ inline double upw_face_block(int i, int j, const double *B, const double *sF)
{
   using C = EfpCfg<P, DIM>;
   constexpr int D = C::D, Q = C::Q, D2 = C::D2, QF = DIM == 3 ? C::Q2 : C::Q;
   const int ii[3] = {i % D, DIM == 3 ? (i / D) % D : i / D, DIM == 3 ? i / D2 : 0};
   const int jj[3] = {j % D, DIM == 3 ? (j / D) % D : j / D, DIM == 3 ? j / D2 : 0};
   double A = 0.0;
#pragma unroll
   for (int c = 0; c < DIM; c++)
   {
      if (ii[c] != jj[c] || (ii[c] != 0 && ii[c] != P)) { continue; }
      const double *sf = sF + (2 * c + (ii[c] == P ? 1 : 0)) * QF;
      const int c1 = DIM == 3 ? (c + 1) % 3 : 1 - c, c2 = DIM == 3 ? (c + 2) % 3 : c1;
      double acc = 0.0;
      if (DIM == 3)
      {
         for (int q2 = 0; q2 < Q; q2++)
         {
            double in = 0.0;
            for (int q1 = 0; q1 < Q; q1++) { in = fma(sf[q1 + Q * q2], B[q1 * D + ii[c1]] * B[q1 * D + jj[c1]], in); }
            acc = fma(B[q2 * D + ii[c2]] * B[q2 * D + jj[c2]], in, acc);
         }
      }
      else
      {
         for (int q1 = 0; q1 < Q; q1++) { acc = fma(sf[q1], B[q1 * D + ii[c1]] * B[q1 * D + jj[c1]], acc); }
      }
      A += acc;
   }
   return A;
}

// DiscreteUpwind::CalcLOSolution.  m: the lumped mass M 1 of the same geometry (the context's).
template <int P, int DIM>
__global__ void __launch_bounds__((EfpCfg<P, DIM>::NT)) lo_upwind_kernel(UpwArgs a, const double *u, const double *m, double *du_lo)
{
   using C = UpwCfg<P, DIM, false>;
   using T = typename C::T;
   constexpr int D = C::D, Q = C::Q, D2 = C::D2, S = C::S, NT = C::NT, NW = C::NW, NF = C::NF, QF = C::QF, DF = C::DF;
   static_assert(DIM == 3 || S <= 64, "dim = 2: one row entry per lane");
   __shared__ double sTab[C::NTAB];
   __shared__ double sX[C::NN], sV[C::NN];
   __shared__ double sD[DIM * C::NQ];
   __shared__ double sF[NF * QF];
   __shared__ double sBuf[NW * (C::NT1 + C::NT2)];
   __shared__ double sU[S], sCf[NF * DF], sNb[NF * DF];
   const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
   const size_t e = blockIdx.x;
   for (int i = tid; i < S; i += NT) { sU[i] = u[e * S + i]; }
   // the mirrored face dofs of the face neighbours (0 on the domain boundary): entry r = i1 + D i2 of face f
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
         // (compact ghost records hold exactly the layer facing this rank, ordered like this face: rmh_exchange_setup)
         const double *un = ghost ? a.u_ghost + (size_t)(nb - a.ne_owned) * a.gh_ustride : u + (size_t)nb * S;
         v = un[(ghost && a.gh_compact) ? r : off];
      }
      sNb[k] = v;
   }
   upw_geometry<P, DIM, false>(a, e, sTab, sX, sV, sD, nullptr, sF);
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
   __syncthreads();
   double *t1 = sBuf + wv * (C::NT1 + C::NT2), *t2 = t1 + C::NT1;
   double kr[C::JPL], kc[C::JPL], mr[C::JPL];
   for (int r = 0; r < C::ROUNDS; r++)
   {
      const int row = r * NW + wv;
      const bool on = row < S;
      if (!on) { continue; }
      const int i = row;
      upw_sweep<P, DIM, false>(i, lane, tB, tG, sD, nullptr, t1, t2, kr, kc, mr);
      const double ui = sU[i];
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < C::JPL; k++)
      {
         const int j = lane + 64 * k;
         if (j < S)
         {
            const double dij = j != i ? fmax(fmax(0.0, -kr[k]), -kc[k]) : 0.0; // remhos_lo.cpp:90-96
            acc += fma(kr[k], sU[j], dij * (sU[j] - ui));
         }
      }
      acc = block_sum<1>(acc, nullptr);
      if (on && lane == 0)
      {
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
}

// FluxBasedFCT::CalcFCTSolution, one FCT iteration.  m: the lumped mass argument of the FCTSolver interface.
template <int P, int DIM>
__global__ void __launch_bounds__((EfpCfg<P, DIM>::NT)) fct_fluxbased_kernel(UpwArgs a, const double *u, const double *m,
                                                                             const double *du_ho, const double *du_lo,
                                                                             const double *u_min, const double *u_max, double dt,
                                                                             double *du)
{
   using C = UpwCfg<P, DIM, true>;
   using T = typename C::T;
   constexpr int S = C::S, NT = C::NT, NW = C::NW, NF = C::NF, QF = C::QF;
   static_assert(DIM == 3 || S <= 64, "dim = 2: one row entry per lane");
   __shared__ double sTab[C::NTAB];
   __shared__ double sX[C::NN], sV[C::NN];
   __shared__ double sD[DIM * C::NQ], sW[C::NQ];
   __shared__ double sF[NF * QF];
   __shared__ double sBuf[NW * (C::NT1 + C::NT2)];
   __shared__ double sU[S], sH[S], sCp[S], sCn[S];
   const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
   const size_t e = blockIdx.x;
   for (int i = tid; i < S; i += NT)
   {
      sU[i] = u[e * S + i];
      sH[i] = du_ho[e * S + i];
   }
   upw_geometry<P, DIM, true>(a, e, sTab, sX, sV, sD, sW, sF);
   const double *tB = sTab + T::oB, *tG = sTab + T::oG;
   double *t1 = sBuf + wv * (C::NT1 + C::NT2), *t2 = t1 + C::NT1;
   double kr[C::JPL], kc[C::JPL], mr[C::JPL];
   for (int pass = 1; pass <= 2; pass++)
   {
      for (int r = 0; r < C::ROUNDS; r++)
      {
         const int row = r * NW + wv;
         const bool on = row < S;
         if (!on) { continue; }
         const int i = row;
         upw_sweep<P, DIM, true>(i, lane, tB, tG, sD, sW, t1, t2, kr, kc, mr);
         const double ui = sU[i], Hi = sH[i];
         const double cpi = pass == 2 ? sCp[i] : 0.0, cni = pass == 2 ? sCn[i] : 0.0;
         double gp = 0.0, gm = 0.0;
#pragma unroll
         for (int k = 0; k < C::JPL; k++)
         {
            const int j = lane + 64 * k;
            if (j < S && j != i)
            {
               const double A = upw_face_block<P, DIM>(i, j, tB, sF);
               const double dij = fmax(fmax(0.0, A - kr[k]), A - kc[k]); // remhos_fct.cpp:314-315 with K = K_vol - A
               // (:319, 337: the flux as its owner sees it, f_ji = -f_ij bit for bit)
               const double f = fma(dt * dij, ui - sU[j], mr[k] * (dt * (Hi - sH[j])));
               if (pass == 1)
               {
                  gp += fmax(f, 0.0); // :343-380
                  gm += fmin(f, 0.0);
               }
               else
               {
                  const double aij = f >= 0.0 ? fmin(cpi, sCn[j]) : fmin(cni, sCp[j]); // :428-437
                  gp += f * aij;
               }
            }
         }
         gp = block_sum<1>(gp, nullptr);
         if (pass == 1) { gm = block_sum<1>(gm, nullptr); }
         if (on && lane == 0)
         {
            const size_t g = e * S + i;
            if (pass == 1)
            {
               // ComputeFluxCoefficients (:382-399)
               const double mi = m[g], u_lo = ui + dt * du_lo[g];
               const double max_pos = fmax((u_max[g] - u_lo) * mi, 0.0), min_neg = fmin((u_min[g] - u_lo) * mi, 0.0);
               sCp[i] = gp > max_pos ? max_pos / gp : 1.0;
               sCn[i] = gm < min_neg ? min_neg / gm : 1.0;
            }
            else { store_stream(du + g, du_lo[g] + gp / m[g] / dt); } // :440
         }
      }
      __syncthreads(); // (pass 2 reads every dof's coefficients)
   }
}

} // namespace rmh
