// MonoRDSolver::CalcSolution (-mono 1, MonolithicSolverType::ResDistMono; remhos_mono.cpp:60-356, remhos.cpp:997-1013, 1687) for
// gfx950, dim = 3 and dim = 2: the whole right-hand side of a stage as ONE bound-preserving residual-distribution update -- no
// HO / LO / FCT split and no LimitMult.  subcell_scheme = false, no smoothness indicator, inflow_gf = 0.
//
// Per element (the reference's loop over k, :123-355), with K_vol the volume-only convection form (k.SpMat(), remhos.cpp:646-657,
// block diagonal), b^F = B_F^T diag(s_F) B_F the upwind face matrix of face F (bdrInt, remhos_tools.cpp:847-856), M the consistent
// and m_L the lumped mass of the mesh at the operator's time:
//   z = K_vol u,  d = z                                                                                            (:110-111)
//   alpha_j = min(1, beta min(xi_max - u, u - xi_min) / (max(xi_max - u, u - xi_min) + eps)),  beta = 10, eps = 1e-15   (:128-131)
//   du = alpha z,  z -= alpha z                                                                                   (:157-158)
//   every face F: Assembly::NonlinFluxLumping (remhos_tools.cpp:915-973) with alpha into du and with alpha = 1 into d (:162-166):
//       xDiff_i = u_i^nbr - u_i,   y_i += sum_j b_ij xDiff_i,   corr_i = alpha_i sum_j b_ij (xDiff_j - xDiff_i),
//       corr balanced against SumCorrP / SumCorrN of the face (:958-972),   y_i += corr_i
//   rhoP = sum max(0, z), rhoN = sum min(0, z),  du_i += (xe_max - u_i) / sumWeightsP rhoP + (xe_min - u_i) / sumWeightsN rhoN   (:169-180, 242-260)
//   mass_lim: at most 101 passes of  uDot = (du + m_it) / m_L,  m_it_i = sum_j M_ij (uDot_i - uDot_j),  the blend (27)-(29) against
//       d - du, alpha from scale(k), the balancing of MassP / MassN, exit at ||m_it + du - m_L uDot||_2 <= 1e-8         (:264-348)
//   du = (du + m_it) / m_L                                                                                        (:350-354)
//
// Work decomposition (EfpCfg / UpwCfg): one element per workgroup of NW wavefronts.
//   A  geometry phase (upw_geometry); the owner of row i (a wavefront) forms K_i. and -- where M is kept -- M_i. in one sweep
//      (upw_sweep), reduces z_i = K_i. u with the wavefront's butterfly and puts M_i. into row i of sM.  The column the sweep also
//      returns is not used.
//   B  faces: a wavefront owns one (face, face dof i) pair at a time, face dof j in lane j (at most 49 of them): the entries b_ij
//      are formed from the face speeds, the two sums over j are butterflies.  One thread per face then adds up SumCorrP / SumCorrN in
//      the order of the face dofs, for alpha and for alpha = 1.
//   C  per dof (thread i, i + NT, ...): alpha, the volume split, the balanced face terms of the up to DIM faces of the dof, the
//      element redistribution.  Element extrema of u, sum u, rhoP, rhoN: block reductions in a fixed order.
//   D  mass iteration: wavefront 0, dof i in lane i (s <= 64), uDot in LDS (read as a broadcast), row i of sM in lane i (row stride
//      SP odd: no bank conflicts), summed j = s - 1 ... 0 like the reference's walk through the CSR row.  Every reduction is a
//      butterfly whose result is the same bits in every lane, so the exit test is wave-uniform and no barrier is inside the loop.
// No atomics anywhere: two calls give the same bits.
//
// M must stay resident over the passes: sM holds s SP doubles where s <= 64 (every 2-D order, 3-D orders 1 to 3).  3-D orders >= 4
// run without mass_lim only (the C ABI refuses them with mass_lim); those instantiations form no mass rows at all (MASS = false).
#pragma once
#include "rmh_upwind.hpp"

namespace rmh
{

constexpr int MONO_MAX_PASSES = 101; // it = 0 ... max_iter = 100 (remhos_mono.cpp:64, 265)

template <int P, int DIM>
struct MonoCfg : UpwCfg<P, DIM, (EfpCfg<P, DIM>::S <= 64)>
{
   using U = UpwCfg<P, DIM, (EfpCfg<P, DIM>::S <= 64)>;
   static constexpr int S = U::S;
   static constexpr bool HASM = S <= 64;      // the mass iteration is built (one dof per lane of a wavefront)
   static constexpr int SP = S | 1;           // row stride of sM
   static constexpr int NM = HASM ? S * SP : 1;
   static constexpr int NFD = U::NF * U::DF;  // (face, face dof) pairs
   // multiply-adds of an element without the passes, and of one pass
   static constexpr long long ELEM_FMA = S * U::SWEEP_FMA + (long long)NFD * U::DF * U::QF;
   static constexpr long long PASS_FMA = (long long)S * S;
};

// entry (r, j) of the face matrix b^F between the face dofs r and j of one face, sf: the face's speeds (upw_geometry's sF)
template <int P, int DIM>
__device__ inline double mono_face_entry(int r, int j, const double *B, const double *sf)
{
   using C = EfpCfg<P, DIM>;
   constexpr int D = C::D, Q = C::Q;
   double acc = 0.0;
   if (DIM == 3)
   {
      const int i1 = r % D, i2 = r / D, j1 = j % D, j2 = j / D;
      for (int q2 = 0; q2 < Q; q2++)
      {
         double in = 0.0;
         for (int q1 = 0; q1 < Q; q1++) { in = fma(sf[q1 + Q * q2], B[q1 * D + i1] * B[q1 * D + j1], in); }
         acc = fma(B[q2 * D + i2] * B[q2 * D + j2], in, acc);
      }
   }
   else
   {
      for (int q1 = 0; q1 < Q; q1++) { acc = fma(sf[q1], B[q1 * D + r] * B[q1 * D + j], acc); }
   }
   return acc;
}

// element dof of face dof r = i1 + D i2 of face f = 2 c + side (the layout of lo_upwind_kernel's sNb / sCf)
template <int P, int DIM>
__device__ inline int mono_face_dof(int f, int r)
{
   constexpr int D = P + 1, D2 = D * D;
   const int c = f >> 1, layer = (f & 1) ? P : 0;
   if (DIM == 3)
   {
      const int i1 = r % D, i2 = r / D;
      const int stc = c == 0 ? 1 : (c == 1 ? D : D2), st1 = c == 0 ? D : (c == 1 ? D2 : 1), st2 = c == 0 ? D2 : (c == 1 ? 1 : D);
      return layer * stc + i1 * st1 + i2 * st2;
   }
   return c == 0 ? layer + D * r : r + D * layer;
}

// remhos_tools.cpp:958-970: the correction of a face dof balanced against the sums of the face
__device__ inline double mono_balance(double v, double sumP, double sumN, double eps)
{
   if (sumP + sumN > eps) { return fmin(0.0, v) - fmax(0.0, v) * sumN / sumP; }
   if (sumP + sumN < -eps) { return fmax(0.0, v) - fmin(0.0, v) * sumP / sumN; }
   return v;
}

// m: the lumped mass of the same geometry (the context's).  scale: [ne] (remhos_mono.cpp:37-57).  rec: [ne], the passes of the
// element's mass iteration, negative when it left the loop at the cap; 0 without mass_lim.
template <int P, int DIM>
__global__ void __launch_bounds__((EfpCfg<P, DIM>::NT)) mono_rd_kernel(UpwArgs a, const double *u, const double *m, const double *xi_min,
                                                                       const double *xi_max, const double *scale, int mass_lim,
                                                                       double *du, int *rec)
{
   using C = MonoCfg<P, DIM>;
   using T = typename C::T;
   constexpr int D = C::D, D2 = C::D2, S = C::S, SP = C::SP, NT = C::NT, NW = C::NW, NF = C::NF, QF = C::QF, DF = C::DF, NFD = C::NFD;
   constexpr bool HASM = C::HASM;
   static_assert(DIM == 3 || S <= 64, "dim = 2: one row entry per lane");
   static_assert(DF <= 64, "one face dof per lane");
   __shared__ double sTab[C::NTAB];
   __shared__ double sX[C::NN], sV[C::NN];
   __shared__ double sD[DIM * C::NQ], sW[HASM ? C::NQ : 1];
   __shared__ double sF[NF * QF];
   __shared__ double sBuf[NW * (C::NT1 + C::NT2)];
   __shared__ double sM[C::NM];
   __shared__ double sU[S], sZ[S], sDu[S], sDd[S], sAl[S], sUd[HASM ? S : 1];
   __shared__ double sNb[NFD], sLump[NFD], sCorr[NFD], sBal[NF * 4];
   __shared__ double s_red[4];
   const double beta = 10.0, eps = 1.e-15, tol = 1.e-8; // remhos_mono.cpp:68
   const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
   const size_t e = blockIdx.x;
   for (int i = tid; i < S; i += NT) { sU[i] = u[e * S + i]; }
   // the mirrored face dofs of the face neighbours (0 on the domain boundary: inflow_gf = 0), as in lo_upwind_kernel
   for (int k = tid; k < NFD; k += NT)
   {
      const int f = k / DF, r = k % DF;
      const int nb = a.face_nbr[e * NF + f];
      double v = 0.0;
      if (nb >= 0)
      {
         const int off = mono_face_dof<P, DIM>(f ^ 1, r); // (the opposite layer of the neighbour)
         const bool ghost = nb >= a.ne_owned;
         const double *un = ghost ? a.u_ghost + (size_t)(nb - a.ne_owned) * a.gh_ustride : u + (size_t)nb * S;
         v = un[(ghost && a.gh_compact) ? r : off];
      }
      sNb[k] = v;
   }
   upw_geometry<P, DIM, HASM>(a, e, sTab, sX, sV, sD, HASM ? sW : nullptr, sF);
   const double *tB = sTab + T::oB, *tG = sTab + T::oG;
   // ---- A: z = K_vol u, M ----------------------------------------------------------------------------------------------------
   {
      double *t1 = sBuf + wv * (C::NT1 + C::NT2), *t2 = t1 + C::NT1;
      double kr[C::JPL], kc[C::JPL], mr[C::JPL];
      for (int r = 0; r < C::ROUNDS; r++)
      {
         const int i = r * NW + wv;
         if (i >= S) { continue; }
         upw_sweep<P, DIM, HASM>(i, lane, tB, tG, sD, HASM ? sW : nullptr, t1, t2, kr, kc, mr);
         double acc = 0.0;
#pragma unroll
         for (int k = 0; k < C::JPL; k++)
         {
            const int j = lane + 64 * k;
            if (j < S)
            {
               acc = fma(kr[k], sU[j], acc);
               if (HASM) { sM[HASM ? i * SP + j : 0] = mr[k]; }
            }
         }
         acc = block_sum<1>(acc, nullptr);
         if (lane == 0) { sZ[i] = acc; }
      }
   }
   // ---- B: the two sums of NonlinFluxLumping over the face dofs j (remhos_tools.cpp:944-952) --------------------------------------
   for (int w = wv; w < NFD; w += NW)
   {
      const int f = w / DF, r = w % DF;
      double lump = 0.0, corr = 0.0;
      if (lane < DF)
      {
         const double b = mono_face_entry<P, DIM>(r, lane, tB, sF + f * QF);
         const double xdi = sNb[w] - sU[mono_face_dof<P, DIM>(f, r)];
         const double xdj = sNb[f * DF + lane] - sU[mono_face_dof<P, DIM>(f, lane)];
         lump = b * xdi;
         corr = b * (xdj - xdi);
      }
      lump = block_sum<1>(lump, nullptr);
      corr = block_sum<1>(corr, nullptr);
      if (lane == 0) { sLump[w] = lump; sCorr[w] = corr; }
   }
   __syncthreads();
   // ---- C: alpha, the volume split (:125-159) and the element sums (:169-180) ----------------------------------------------------
   double umin = INFINITY, umax = -INFINITY, xsum = 0.0, rhoP = 0.0, rhoN = 0.0;
   for (int i = tid; i < S; i += NT)
   {
      const size_t g = e * S + i;
      const double ui = sU[i], up = xi_max[g] - ui, dn = ui - xi_min[g];
      const double al = fmin(1.0, beta * fmin(up, dn) / (fmax(up, dn) + eps));
      const double z = sZ[i], az = al * z, zr = z - az;
      sAl[i] = al;
      sDu[i] = az;
      sDd[i] = z;
      umin = fmin(umin, ui);
      umax = fmax(umax, ui);
      xsum += ui;
      rhoP += fmax(0.0, zr);
      rhoN += fmin(0.0, zr);
   }
   umin = block_min<NW>(umin, s_red);
   umax = block_max<NW>(umax, s_red);
   xsum = block_sum<NW>(xsum, s_red);
   rhoP = block_sum<NW>(rhoP, s_red);
   rhoN = block_sum<NW>(rhoN, s_red);
   __syncthreads(); // (NW = 1: the reductions above hold no barrier; sAl is read by other threads below)
   // SumCorrP / SumCorrN of every face, for alpha (into du) and for alpha = 1 (into d), in the order of the face dofs (:953-955)
   if (tid < NF)
   {
      double pa = 0.0, na = 0.0, p1 = 0.0, n1 = 0.0;
      for (int r = 0; r < DF; r++)
      {
         const double c1 = sCorr[tid * DF + r], ca = sAl[mono_face_dof<P, DIM>(tid, r)] * c1;
         pa += fmax(0.0, ca);
         na += fmin(0.0, ca);
         p1 += fmax(0.0, c1);
         n1 += fmin(0.0, c1);
      }
      sBal[tid * 4 + 0] = pa;
      sBal[tid * 4 + 1] = na;
      sBal[tid * 4 + 2] = p1;
      sBal[tid * 4 + 3] = n1;
   }
   __syncthreads();
   const double sumWP = S * umax - xsum + eps, sumWN = S * umin - xsum - eps; // :179-180
   const bool iterate = HASM && mass_lim;
   for (int i = tid; i < S; i += NT)
   {
      const double ui = sU[i], al = sAl[i];
      double dui = sDu[i], di = sDd[i];
      const int ii[3] = {i % D, DIM == 3 ? (i / D) % D : i / D, DIM == 3 ? i / D2 : 0};
#pragma unroll
      for (int c = 0; c < DIM; c++)
      {
         if (ii[c] != 0 && ii[c] != P) { continue; }
         const int c1 = DIM == 3 ? (c + 1) % 3 : 1 - c, c2 = DIM == 3 ? (c + 2) % 3 : c1;
         const int f = 2 * c + (ii[c] == P ? 1 : 0), k = f * DF + ii[c1] + (DIM == 3 ? D * ii[c2] : 0);
         const double lump = sLump[k], c1v = sCorr[k];
         dui += lump;
         dui += mono_balance(al * c1v, sBal[f * 4 + 0], sBal[f * 4 + 1], eps);
         di += lump;
         di += mono_balance(c1v, sBal[f * 4 + 2], sBal[f * 4 + 3], eps);
      }
      dui += (umax - ui) / sumWP * rhoP + (umin - ui) / sumWN * rhoN; // :245-259
      if (iterate) { sDu[i] = dui; sDd[i] = di; }
      else { store_stream(du + e * S + i, dui / m[e * S + i]); } // :353 with m_it = 0
   }
   if (!iterate)
   {
      if (tid == 0) { rec[e] = 0; }
      return;
   }
   __syncthreads();
   // ---- D: the mass iteration (:264-348), wavefront 0, dof i in lane i ------------------------------------------------------------
   if (HASM && wv == 0)
   {
      const bool on = lane < S;
      const int i = on ? lane : 0;
      const size_t g = e * S + i;
      const double ui = sU[i], dui = sDu[i], di = sDd[i], ml = m[g];
      const double gap = beta * scale[e] * fmin(xi_max[g] - ui, ui - xi_min[g]); // :310-312
      const double diff = di - dui;
      const double *Mi = sM + (HASM ? i * SP : 0);
      double mit = 0.0;
      int passes = 0;
      bool conv = false;
      for (int it = 0; it < MONO_MAX_PASSES; it++)
      {
         const double ud = (dui + mit) / ml;
         if (on) { sUd[HASM ? i : 0] = ud; }
         wave_lds_fence();
         const double udmin = block_min<1>(on ? ud : INFINITY, nullptr), udmax = block_max<1>(on ? ud : -INFINITY, nullptr);
         double acc = 0.0;
         for (int j = S - 1; j >= 0; j--) { acc += Mi[j] * (ud - sUd[HASM ? j : 0]); } // run backwards through columns (:286-291)
         acc += fmin(1.0, fmax(0.0, fabs(acc) / (fabs(diff) + eps))) * diff;          // eq. (27) - (29), tmp = 0 (:300)
         acc *= fmin(1.0, gap / (fmax(udmax - ud, ud - udmin) + eps));                 // :310-313, 324
         const double massP = block_sum<1>(on ? fmax(0.0, acc) : 0.0, nullptr), massN = block_sum<1>(on ? fmin(0.0, acc) : 0.0, nullptr);
         mit = mono_balance(acc, massP, massN, eps);                                   // :329-339
         const double res = on ? mit + dui - ml * ud : 0.0;
         const double nrm = sqrt(block_sum<1>(res * res, nullptr));                    // (the same bits in every lane)
         wave_lds_fence(); // (the next pass writes sUd)
         passes = it + 1;
         if (nrm <= tol) { conv = true; break; }
      }
      if (on) { store_stream(du + g, (dui + mit) / ml); }
      if (lane == 0) { rec[e] = conv ? passes : -passes; }
   }
}

} // namespace rmh
