// ElementFCTProjection::CalcFCTSolution (-fct 4; remhos_fct.cpp:613-731, remhos_fct.hpp:157-174) for gfx950, dim = 3 and dim = 2.
//
// Zalesak-type limiting of the antidiffusive fluxes between every pair of dofs of an element,
//   F_ij = M_ij (duH_i - duH_j) + (beta_j z_i - beta_i z_j),   z = M duH - ML duL,  ML = row sums of M,  beta = ML / sum ML,
// with the element's CONSISTENT mass matrix M = Phi^T diag(w detJ) Phi at the pseudo-time of the last rmh_setup (the reference
// assembles it with MassIntegrator on the moved mesh and ignores the lumped mass it is handed).
//
// Work decomposition: one element per workgroup of NW wavefronts.  M (s x s, s = (p+1)^dim: 941 KB at p = 6) is never stored:
// a wavefront forms ONE ROW of it at a time by sum factorisation from w detJ in LDS,
//   M_i. = B^T (x) B^T (x) B^T ((w detJ) . Phi_i):  Q^2 D + Q D^2 + D^3 outputs of Q multiply-adds each (dim = 3),
// keeps the row in registers (lane l holds the entries j = l, l + 64, ...) and reduces over the row with the wavefront's butterfly.
// The element is walked three times, NW rows per round:
//   pass 0  ML_i = sum_j M_ij, z_i = sum_j M_ij duH_j - ML_i duL_i
//   pass 1  the sign-split flux sums gp_i, gm_i and the ratios against ML (du_max - duL), ML (du_min - duL)   (:677-708)
//   pass 2  du_i = duL_i + sum_j a_ij F_ij / ML_i                                                            (:710-729)
// The owner of row i evaluates F for every j != i as the reference's F(max(i, j), min(i, j)) -- the factors B_i B_j of the row
// are formed as products first, so M_ij and M_ji are the same bits and both owners of a pair see the same flux with the same
// sign.  No atomics: the summation order of every dof is fixed and the result is the same bits from run to run.
#pragma once
#include "rmh_kernels.hpp"

namespace rmh
{

template <int P, int DIM>
struct EfpCfg
{
   using T = TabLayoutQ<P, (DIM == 3 ? P + 3 : P + 2)>; // (the rule of the HO kernels: rmh_tables.hpp)
   static constexpr int D = T::D, Q = T::Q, D2 = D * D, Q2 = Q * Q;
   static constexpr int S = DIM == 3 ? D2 * D : D2;  // dofs of an element
   static constexpr int NQ = DIM == 3 ? Q2 * Q : Q2; // quadrature points
   static constexpr int NW = S <= 16 ? 1 : (S <= 64 ? 2 : 4); // rows in flight = wavefronts
   static constexpr int NT = 64 * NW;
   static constexpr int JPL = (S + 63) / 64;         // row entries per lane
   static constexpr int ROUNDS = (S + NW - 1) / NW;
   static constexpr int N1 = DIM == 3 ? Q2 * D : Q * D; // x-contracted row, per wavefront
   static constexpr int N2 = DIM == 3 ? Q * D2 : 1;     // xy-contracted row (dim = 3)
   static constexpr int NG = DIM == 3 ? 6 * Q * 9 : 1;  // x-contracted nodes of the geometry phase (overlaid on the row buffers)
   static constexpr int NROWBUF = NW * (N1 + N2) > NG ? NW * (N1 + N2) : NG;
   static constexpr int NN = DIM == 3 ? 81 : 18;        // node values of an element
   static constexpr int NTAB = T::oBg;                  // B, G, L, dL, w
   // multiply-adds of one row and of the three passes over an element (the figure of profiles/efp_kernel_stats.txt)
   static constexpr long long ROW_FMA = DIM == 3 ? (long long)Q * (Q2 * D + Q * D2 + D2 * D) : (long long)Q * (Q * D + D2);
   static constexpr long long ELEM_FMA = 3 * S * ROW_FMA;
};

// F(a, b) of remhos_fct.cpp:672-673 for a > b, with a fixed rounding sequence (both owners of a pair must get the same bits)
__device__ inline double efp_flux(double Mab, double Ha, double Hb, double ba, double bb, double za, double zb)
{
   return fma(Mab, Ha - Hb, fma(bb, za, -(ba * zb)));
}

// Row i of the element mass matrix into m[k] = M(i, lane + 64 k); t1 / t2: this wavefront's LDS buffers.  Called by every
// thread of the workgroup (two barriers).
template <int P, int DIM>
__device__ inline void efp_row(int i, int lane, const double *B, const double *sW, double *t1, double *t2,
                               double (&m)[EfpCfg<P, DIM>::JPL])
{
   using C = EfpCfg<P, DIM>;
   constexpr int D = C::D, Q = C::Q, D2 = C::D2, Q2 = C::Q2, S = C::S;
   if (DIM == 3)
   {
      const int ix = i % D, iy = (i / D) % D, iz = i / D2;
      for (int k = lane; k < Q2 * D; k += 64)
      {
         const int jx = k % D, qyz = k / D;
         double acc = 0.0;
#pragma unroll
         for (int qx = 0; qx < Q; qx++) { acc += sW[qx + Q * qyz] * (B[qx * D + ix] * B[qx * D + jx]); }
         t1[k] = acc;
      }
      __syncthreads();
      for (int k = lane; k < Q * D2; k += 64)
      {
         const int jx = k % D, jy = (k / D) % D, qz = k / D2;
         double acc = 0.0;
#pragma unroll
         for (int qy = 0; qy < Q; qy++) { acc += (B[qy * D + iy] * B[qy * D + jy]) * t1[(qy + Q * qz) * D + jx]; }
         t2[k] = acc;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < C::JPL; k++)
      {
         const int j = lane + 64 * k;
         double acc = 0.0;
         if (j < S)
         {
            const int jxy = j % D2, jz = j / D2;
#pragma unroll
            for (int qz = 0; qz < Q; qz++) { acc += (B[qz * D + iz] * B[qz * D + jz]) * t2[jxy + D2 * qz]; }
         }
         m[k] = acc;
      }
   }
   else
   {
      const int ix = i % D, iy = i / D;
      for (int k = lane; k < Q * D; k += 64)
      {
         const int jx = k % D, qy = k / D;
         double acc = 0.0;
#pragma unroll
         for (int qx = 0; qx < Q; qx++) { acc += sW[qx + Q * qy] * (B[qx * D + ix] * B[qx * D + jx]); }
         t1[k] = acc;
      }
      __syncthreads();
      {
         const int j = lane; // (D^2 <= 49: one entry per lane)
         double acc = 0.0;
         if (j < S)
         {
            const int jx = j % D, jy = j / D;
#pragma unroll
            for (int qy = 0; qy < Q; qy++) { acc += (B[qy * D + iy] * B[qy * D + jy]) * t1[qy * D + jx]; }
         }
         m[0] = acc;
      }
      __syncthreads(); // (the next row's x-contraction writes t1)
   }
}

// x0 / vel: the element nodes as the context keeps them on the device -- dim = 3: [ne][3][27], hierarchical along the directions
// of the bit mask `hier` (RMH_HIER, rmh_ho2.hpp; put back into nodal form in LDS like lumped_mass_kernel does); dim = 2:
// [ne][2][9], nodal.
template <int P, int DIM>
__global__ void __launch_bounds__((EfpCfg<P, DIM>::NT)) fct_projection_kernel(const double *x0, const double *vel,
                                                                              const double *gtab, double t, int move, int hier,
                                                                              const double *u, const double *du_ho,
                                                                              const double *du_lo, const double *u_min,
                                                                              const double *u_max, double dt, double *du)
{
   using C = EfpCfg<P, DIM>;
   using T = typename C::T;
   constexpr int Q = C::Q, Q2 = C::Q2, S = C::S, NT = C::NT, NW = C::NW, NN = C::NN;
   static_assert(DIM == 3 || S <= 64, "dim = 2: one row entry per lane");
   __shared__ double sTab[C::NTAB];
   __shared__ double sX[NN];
   __shared__ double sW[C::NQ];
   __shared__ double sBuf[C::NROWBUF];
   __shared__ double sH[S], sL[S], sML[S], sBeta[S], sZ[S], sRp[S], sRm[S];
   __shared__ double s_red[4];
   const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
   const size_t e = blockIdx.x;
   const double *tB = sTab + T::oB, *tL = sTab + T::oL, *tdL = sTab + T::odL, *tW = sTab + T::oW;
   for (int i = tid; i < C::NTAB; i += NT) { sTab[i] = gtab[i]; }
   for (int i = tid; i < NN; i += NT)
   {
      const double x = x0[e * NN + i];
      sX[i] = move ? x + t * vel[e * NN + i] : x;
   }
   for (int i = tid; i < S; i += NT)
   {
      sH[i] = du_ho[e * S + i];
      sL[i] = du_lo[e * S + i];
   }
   __syncthreads();
   // ---- w detJ at the quadrature points -----------------------------------------------------------------------------------
   if (DIM == 3)
   {
      for (int dir = 2; dir >= 0; dir--) // (the host took the differences along x, then y, then z: undone in the reverse order)
      {
         if (!((hier >> dir) & 1)) { continue; }
         const int st = dir == 0 ? 1 : (dir == 1 ? 3 : 9);
         for (int i = tid; i < 81; i += NT)
         {
            const int a = ((i % 27) / st) % 3;
            if (a > 0) { sX[i] += sX[i - a * st]; } // (entries with a = 0 are only read in this pass)
         }
         __syncthreads();
      }
      // x-contraction of the nodes: sG[((comp*2 + kind)*Q + qx)*9 + ay + 3*az], kind 0: L.X, 1: dL.X
      double *sG = sBuf;
      for (int k = tid; k < 6 * Q * 9; k += NT)
      {
         const int arr = k / (Q * 9), r = k % (Q * 9);
         const int qx = r / 9, n2 = r % 9;
         const int comp = arr / 2, kind = arr % 2;
         const double *src = sX + comp * 27 + 3 * n2;
         const double *w = (kind ? tdL : tL) + qx * 3;
         sG[k] = w[0] * src[0] + w[1] * src[1] + w[2] * src[2];
      }
      __syncthreads();
      for (int col = tid; col < Q2; col += NT) // column (qx, qy): Jacobian at its Q points
      {
         const int qx = col % Q, qy = col / Q;
         double A[3][3][3]; // [comp][d/dxi, d/deta, value for d/dzeta][az]
#pragma unroll
         for (int comp = 0; comp < 3; comp++)
         {
#pragma unroll
            for (int az = 0; az < 3; az++)
            {
               double a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
               for (int ay = 0; ay < 3; ay++)
               {
                  const double Ly = tL[qy * 3 + ay], dLy = tdL[qy * 3 + ay];
                  const double xl = sG[((comp * 2 + 0) * Q + qx) * 9 + ay + 3 * az];
                  const double xd = sG[((comp * 2 + 1) * Q + qx) * 9 + ay + 3 * az];
                  a0 += Ly * xd;
                  a1 += dLy * xl;
                  a2 += Ly * xl;
               }
               A[comp][0][az] = a0; A[comp][1][az] = a1; A[comp][2][az] = a2;
            }
         }
         const double wxy = tW[qx] * tW[qy];
         for (int qz = 0; qz < Q; qz++)
         {
            double J[3][3];
#pragma unroll
            for (int comp = 0; comp < 3; comp++)
            {
               double j0 = 0, j1 = 0, j2 = 0;
#pragma unroll
               for (int az = 0; az < 3; az++)
               {
                  const double Lz = tL[qz * 3 + az], dLz = tdL[qz * 3 + az];
                  j0 += Lz * A[comp][0][az];
                  j1 += Lz * A[comp][1][az];
                  j2 += dLz * A[comp][2][az];
               }
               J[comp][0] = j0; J[comp][1] = j1; J[comp][2] = j2;
            }
            const double A11 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
            const double A21 = J[2][0] * J[1][2] - J[1][0] * J[2][2];
            const double A31 = J[1][0] * J[2][1] - J[2][0] * J[1][1];
            sW[col + Q2 * qz] = wxy * tW[qz] * (J[0][0] * A11 + J[0][1] * A21 + J[0][2] * A31);
         }
      }
   }
   else
   {
      for (int q = tid; q < Q2; q += NT)
      {
         const int qx = q % Q, qy = q / Q;
         double J[2][2] = {{0, 0}, {0, 0}};
#pragma unroll
         for (int ay = 0; ay < 3; ay++)
         {
#pragma unroll
            for (int ax = 0; ax < 3; ax++)
            {
               const double lx = tL[qx * 3 + ax], ly = tL[qy * 3 + ay], dx = tdL[qx * 3 + ax], dy = tdL[qy * 3 + ay];
#pragma unroll
               for (int c = 0; c < 2; c++)
               {
                  const double xn = sX[c * 9 + ax + 3 * ay];
                  J[c][0] += dx * ly * xn;
                  J[c][1] += lx * dy * xn;
               }
            }
         }
         sW[q] = tW[qx] * tW[qy] * (J[0][0] * J[1][1] - J[0][1] * J[1][0]);
      }
   }
   __syncthreads(); // (also: the geometry phase is done with sBuf)
   double *t1 = sBuf + wv * (C::N1 + C::N2), *t2 = t1 + C::N1;
   double m[C::JPL];
   // ---- pass 0: row sums and z = M duH - ML duL (:650-662) -------------------------------------------------------------------
   for (int r = 0; r < C::ROUNDS; r++)
   {
      const int row = r * NW + wv;
      const bool on = row < S;
      const int i = on ? row : S - 1; // (a wavefront without a row in the last round keeps the barriers company)
      efp_row<P, DIM>(i, lane, tB, sW, t1, t2, m);
      double a = 0.0, b = 0.0;
#pragma unroll
      for (int k = 0; k < C::JPL; k++)
      {
         const int j = lane + 64 * k;
         if (j < S) { a += m[k]; b += m[k] * sH[j]; }
      }
      a = block_sum<1>(a, nullptr);
      b = block_sum<1>(b, nullptr);
      if (on && lane == 0) { sML[i] = a; sZ[i] = b - a * sL[i]; }
   }
   __syncthreads();
   {
      double a = 0.0;
      for (int i = tid; i < S; i += NT) { a += sML[i]; }
      const double inv = 1.0 / block_sum<NW>(a, s_red); // (beta /= beta.Sum(): mfem::Vector divides by multiplying with 1 / c)
      for (int i = tid; i < S; i += NT) { sBeta[i] = sML[i] * inv; }
   }
   __syncthreads();
   // ---- pass 1: sums of the positive / negative fluxes of every dof, ratios (:677-708) ------------------------------------------
   for (int r = 0; r < C::ROUNDS; r++)
   {
      const int row = r * NW + wv;
      const bool on = row < S;
      const int i = on ? row : S - 1;
      efp_row<P, DIM>(i, lane, tB, sW, t1, t2, m);
      const double Hi = sH[i], bi = sBeta[i], zi = sZ[i];
      double gp = 0.0, gm = 0.0;
#pragma unroll
      for (int k = 0; k < C::JPL; k++)
      {
         const int j = lane + 64 * k;
         if (j < S && j != i)
         {
            if (j < i) // the pair's flux is F(i, j): the reference's `i` side
            {
               const double f = efp_flux(m[k], Hi, sH[j], bi, sBeta[j], zi, sZ[j]);
               if (f >= 0.0) { gp += f; } else { gm += f; }
            }
            else // F(j, i): the `j` side
            {
               const double f = efp_flux(m[k], sH[j], Hi, sBeta[j], bi, sZ[j], zi);
               if (f >= 0.0) { gm -= f; } else { gp -= f; }
            }
         }
      }
      gp = block_sum<1>(gp, nullptr);
      gm = block_sum<1>(gm, nullptr);
      if (on && lane == 0)
      {
         const size_t g = e * S + i;
         const double ui = u[g], ML = sML[i], dl = sL[i];
         const double du_max = (u_max[g] - ui) / dt, du_min = (u_min[g] - ui) / dt;
         const double rp = fmax(ML * (du_max - dl), 0.0), rm = fmin(ML * (du_min - dl), 0.0);
         sRp[i] = (rp < gp) ? rp / gp : 1.0;
         sRm[i] = (rm > gm) ? rm / gm : 1.0;
      }
   }
   __syncthreads();
   // ---- pass 2: the limited fluxes (:710-729) -------------------------------------------------------------------------------------
   for (int r = 0; r < C::ROUNDS; r++)
   {
      const int row = r * NW + wv;
      const bool on = row < S;
      const int i = on ? row : S - 1;
      efp_row<P, DIM>(i, lane, tB, sW, t1, t2, m);
      const double Hi = sH[i], bi = sBeta[i], zi = sZ[i], rpi = sRp[i], rmi = sRm[i];
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < C::JPL; k++)
      {
         const int j = lane + 64 * k;
         if (j < S && j != i)
         {
            if (j < i)
            {
               const double f = efp_flux(m[k], Hi, sH[j], bi, sBeta[j], zi, sZ[j]);
               const double aij = (f >= 0.0) ? fmin(rpi, sRm[j]) : fmin(rmi, sRp[j]);
               acc += f * aij;
            }
            else
            {
               const double f = efp_flux(m[k], sH[j], Hi, sBeta[j], bi, sZ[j], zi);
               const double aji = (f >= 0.0) ? fmin(sRp[j], rmi) : fmin(sRm[j], rpi);
               acc -= f * aji;
            }
         }
      }
      acc = block_sum<1>(acc, nullptr);
      if (on && lane == 0) { store_stream(du + e * S + i, sL[i] + acc / sML[i]); }
   }
}

} // namespace rmh
