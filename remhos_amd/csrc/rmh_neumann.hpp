// NeumannHOSolver::CalcHOSolution (-ho 1; remhos_ho.cpp:131-187, remhos.cpp:914-917) for gfx950, dim = 3 and dim = 2, orders 1 - 6.
//
//   rhs = K_vol u + sum_F PhiF^T diag(s_F) PhiF (u^nbr - u)      (LinearFluxLumping with alpha = 1, remhos_tools.cpp:900-912:
//                                                                  the right-hand side of -ho 3)
//   du = 0;   for iter = 1 .. 20:   res = M du - rhs;   if the GLOBAL ||res||_2 <= 1e-4: return du;   du -= res / m_L
// with M the consistent element mass and m_L its row sums.  After the 20th update the reference returns without another check.
// It is a crude solver by design: on small lattices it usually runs out its 20 iterations 10 - 90 % away from M^-1 rhs, so what
// has to be reproduced is the reference's STOPPING ITERATION, not a converged answer.
//
// The iteration is element-local; only the stopping test couples the elements.  So the element kernel runs all 20 updates and
// records the squared residual norm of its element at every check, one workgroup adds them up and finds the first check K that
// passes, and -- only if there is one -- the element kernel runs again and stops after K - 1 updates:
//   neumann_rhs_kernel    one element per workgroup: rhs by sum factorisation, to a scratch vector of the context; w detJ at the
//                         quadrature points goes to a second one (the geometry phase is needed once)
//   neumann_iter_kernel   one element per workgroup: n = *n_updates updates entirely in LDS (first pass: 20); before update k
//                         it writes part[k][e] = sum_i res_i^2; then du
//   neumann_norms_kernel  one workgroup: norms[k] = sqrt(sum_e part[k][e]), K = the first k with norms[k] <= 1e-4, or none
//   neumann_iter_kernel   again with *n_updates = K - 1; leaves at once when there is no K (the first pass's du is the answer:
//                         the common case); K = 1 writes exact zeros
// Four launches on one stream, no host synchronisation, no atomics: safe under graph capture.  Every sum has a fixed order
// (one chain of fma() per output, the wavefront butterfly and a serial sum over the wavefronts for the norms), so the result is
// the same bits from run to run, and an element's partial sums do not depend on the global decision.
//
// M du is never a matrix: M du = B^T (w detJ) B du by sum factorisation (dim = 3: six contractions of at most Q^2 D outputs,
// one barrier each), so every order fits in both dimensions.  LDS per workgroup of the iteration kernel: B, w detJ, two
// contraction buffers and three vectors of s doubles; the rhs kernel also holds the geometry tables, D_c and the face speeds.
// The figures per instantiation are in profiles/neumann_kernel_stats.txt.
#pragma once
#include "rmh_upwind.hpp"

namespace rmh
{

constexpr int NEUMANN_MAX_UPDATES = 20;  // remhos_ho.cpp:166
constexpr double NEUMANN_TOL = 1e-4;     // remhos_ho.cpp:165
constexpr int NEUMANN_NORMS_NT = 256;
// control words of a call (device ints): [0] the first pass's update count (20, constant), [1] the second pass's (K - 1; -1:
// nothing to do), [2] updates applied, [3] checks evaluated
constexpr int NEUMANN_NCTL = 4;

template <int P, int DIM>
struct NmCfg : UpwCfg<P, DIM, true>
{
   using U = UpwCfg<P, DIM, true>;
   static constexpr int D = U::D, Q = U::Q, D2 = U::D2, Q2 = U::Q2, S = U::S, NQ = U::NQ, NF = U::NF, QF = U::QF, DF = U::DF;
   static constexpr int cmax(int a, int b) { return a > b ? a : b; }
   // the two contraction buffers: whatever the volume term, the face term and the mass apply put there (see the kernels)
   static constexpr int NB1 = DIM == 3 ? 3 * Q2 * D : cmax(2 * Q * D, NF * Q);
   static constexpr int NB2 = DIM == 3 ? cmax(cmax(2 * Q * D2, NQ), NF * QF) : cmax(NQ, NF * DF);
   // multiply-adds of one mass apply and of the rhs of an element
   static constexpr long long MASS_FMA = DIM == 3 ? 2LL * (Q * D2 * D + Q2 * D * D + NQ * D) : 2LL * (Q * D * D + NQ * D);
};

// out[o along DIR] = sum_k c(o, k) in[k along DIR] over an N0 x N1 x N2 array (index k0 + N0 (k1 + N1 k2)); FWD: c = M[o D + k]
// (dofs -> points), otherwise M[k D + o] (points -> dofs).  One output per thread and turn, one chain of fma(); the caller puts
// the barrier.  scale: multiplied onto the outputs (the weights at the points).
template <int N0, int N1, int N2, int DIR, int NOUT, bool FWD, int D, int NT>
__device__ inline void nm_contract(const double *in, double *out, const double *M, const double *scale = nullptr)
{
   constexpr int NIN = DIR == 0 ? N0 : (DIR == 1 ? N1 : N2);
   constexpr int O0 = DIR == 0 ? NOUT : N0, O1 = DIR == 1 ? NOUT : N1, O2 = DIR == 2 ? NOUT : N2;
   constexpr int ST = DIR == 0 ? 1 : (DIR == 1 ? N0 : N0 * N1);
   for (int k = threadIdx.x; k < O0 * O1 * O2; k += NT)
   {
      const int k0 = k % O0, k1 = (k / O0) % O1, k2 = k / (O0 * O1);
      const int o = DIR == 0 ? k0 : (DIR == 1 ? k1 : k2);
      const int base = (DIR == 0 ? 0 : k0) + N0 * ((DIR == 1 ? 0 : k1) + N1 * (DIR == 2 ? 0 : k2));
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < NIN; j++) { acc = fma(FWD ? M[o * D + j] : M[j * D + o], in[base + j * ST], acc); }
      out[k] = scale ? acc * scale[k] : acc;
   }
}

// y = M x = B^T (w detJ) B x of the element; x: S doubles in LDS.  Returns the buffer (b1 or b2) that holds y.  Called by every
// thread; ends with a barrier.
template <int P, int DIM>
__device__ inline const double *nm_mass_apply(const double *x, const double *B, const double *sW, double *b1, double *b2)
{
   using C = NmCfg<P, DIM>;
   constexpr int D = C::D, Q = C::Q, NT = C::NT;
   if (DIM == 3)
   {
      nm_contract<D, D, D, 0, Q, true, D, NT>(x, b2, B);
      __syncthreads();
      nm_contract<Q, D, D, 1, Q, true, D, NT>(b2, b1, B);
      __syncthreads();
      nm_contract<Q, Q, D, 2, Q, true, D, NT>(b1, b2, B, sW);
      __syncthreads();
      nm_contract<Q, Q, Q, 0, D, false, D, NT>(b2, b1, B);
      __syncthreads();
      nm_contract<D, Q, Q, 1, D, false, D, NT>(b1, b2, B);
      __syncthreads();
      nm_contract<D, D, Q, 2, D, false, D, NT>(b2, b1, B);
      __syncthreads();
      return b1;
   }
   nm_contract<D, D, 1, 0, Q, true, D, NT>(x, b1, B);
   __syncthreads();
   nm_contract<Q, D, 1, 1, Q, true, D, NT>(b1, b2, B, sW);
   __syncthreads();
   nm_contract<Q, Q, 1, 0, D, false, D, NT>(b2, b1, B);
   __syncthreads();
   nm_contract<D, Q, 1, 1, D, false, D, NT>(b1, b2, B);
   __syncthreads();
   return b2;
}

// rhs = K_vol u + sum_F PhiF^T diag(s_F) PhiF (u^nbr - u)
template <int P, int DIM>
__global__ void __launch_bounds__((EfpCfg<P, DIM>::NT)) neumann_rhs_kernel(UpwArgs a, const double *u, double *rhs, double *wdet)
{
   using C = NmCfg<P, DIM>;
   using T = typename C::T;
   constexpr int D = C::D, Q = C::Q, D2 = C::D2, Q2 = C::Q2, S = C::S, NQ = C::NQ, NT = C::NT, NF = C::NF, QF = C::QF, DF = C::DF;
   __shared__ double sTab[C::NTAB];
   __shared__ double sX[C::NN], sV[C::NN];
   __shared__ double sD[DIM * NQ], sW[NQ];
   __shared__ double sF[NF * QF];
   __shared__ double sB1[C::NB1], sB2[C::NB2];
   __shared__ double sU[S], sR[S], sNb[NF * DF];
   const int tid = threadIdx.x;
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
   // ---- K_vol u = Phi^T sum_c D_c (d_c Phi u) -----------------------------------------------------------------------------------
   if (DIM == 3)
   {
      double *AB = sB2, *AG = sB2 + Q * D2;                        // x-contracted: values, x-derivative
      nm_contract<D, D, D, 0, Q, true, D, NT>(sU, AB, tB);
      nm_contract<D, D, D, 0, Q, true, D, NT>(sU, AG, tG);
      __syncthreads();
      double *BB = sB1, *BG = sB1 + Q2 * D, *GB = sB1 + 2 * Q2 * D; // xy-contracted: values, y-derivative, x-derivative
      nm_contract<Q, D, D, 1, Q, true, D, NT>(AB, BB, tB);
      nm_contract<Q, D, D, 1, Q, true, D, NT>(AB, BG, tG);
      nm_contract<Q, D, D, 1, Q, true, D, NT>(AG, GB, tB);
      __syncthreads();
      for (int q = tid; q < NQ; q += NT)
      {
         const int qxy = q % Q2, qz = q / Q2;
         double gx = 0.0, gy = 0.0, gz = 0.0;
#pragma unroll
         for (int iz = 0; iz < D; iz++)
         {
            const double b = tB[qz * D + iz];
            gx = fma(b, GB[qxy + Q2 * iz], gx);
            gy = fma(b, BG[qxy + Q2 * iz], gy);
            gz = fma(tG[qz * D + iz], BB[qxy + Q2 * iz], gz);
         }
         sB2[q] = fma(sD[q], gx, fma(sD[NQ + q], gy, sD[2 * NQ + q] * gz)); // (AB, AG were read in the last phase)
      }
      __syncthreads();
      nm_contract<Q, Q, Q, 0, D, false, D, NT>(sB2, sB1, tB);
      __syncthreads();
      nm_contract<D, Q, Q, 1, D, false, D, NT>(sB1, sB2, tB);
      __syncthreads();
      nm_contract<D, D, Q, 2, D, false, D, NT>(sB2, sR, tB);
   }
   else
   {
      double *AB = sB1, *AG = sB1 + Q * D;
      nm_contract<D, D, 1, 0, Q, true, D, NT>(sU, AB, tB);
      nm_contract<D, D, 1, 0, Q, true, D, NT>(sU, AG, tG);
      __syncthreads();
      for (int q = tid; q < NQ; q += NT)
      {
         const int qx = q % Q, qy = q / Q;
         double gx = 0.0, gy = 0.0;
#pragma unroll
         for (int iy = 0; iy < D; iy++)
         {
            gx = fma(tB[qy * D + iy], AG[qx + Q * iy], gx);
            gy = fma(tG[qy * D + iy], AB[qx + Q * iy], gy);
         }
         sB2[q] = fma(sD[q], gx, sD[NQ + q] * gy);
      }
      __syncthreads();
      nm_contract<Q, Q, 1, 0, D, false, D, NT>(sB2, sB1, tB);
      __syncthreads();
      nm_contract<D, Q, 1, 1, D, false, D, NT>(sB1, sR, tB);
   }
   __syncthreads();
   // ---- the faces: traces of u^nbr - u at the face points, times s_F, back onto the face dofs; entry r = i1 + D i2 of face f,
   //      i1 / i2 along the directions (c + 1) % 3, (c + 2) % 3 (dim = 2: i1 along 1 - c) like sF -------------------------------
   for (int k = tid; k < NF * DF; k += NT)
   {
      const int f = k / DF, r = k % DF, c = f >> 1, side = f & 1;
      int own;
      if (DIM == 3)
      {
         const int i1 = r % D, i2 = r / D;
         const int stc = c == 0 ? 1 : (c == 1 ? D : D2), st1 = c == 0 ? D : (c == 1 ? D2 : 1), st2 = c == 0 ? D2 : (c == 1 ? 1 : D);
         own = (side ? P : 0) * stc + i1 * st1 + i2 * st2;
      }
      else
      {
         const int layer = side ? P : 0;
         own = c == 0 ? layer + D * r : r + D * layer;
      }
      sB2[k] = sNb[k] - sU[own];
   }
   __syncthreads();
   if (DIM == 3)
   {
      nm_contract<D, D, NF, 0, Q, true, D, NT>(sB2, sB1, tB);
      __syncthreads();
      nm_contract<Q, D, NF, 1, Q, true, D, NT>(sB1, sB2, tB, sF);
      __syncthreads();
      nm_contract<Q, Q, NF, 0, D, false, D, NT>(sB2, sB1, tB);
      __syncthreads();
      nm_contract<D, Q, NF, 1, D, false, D, NT>(sB1, sB2, tB);
   }
   else
   {
      nm_contract<D, NF, 1, 0, Q, true, D, NT>(sB2, sB1, tB, sF);
      __syncthreads();
      nm_contract<Q, NF, 1, 0, D, false, D, NT>(sB1, sB2, tB);
   }
   __syncthreads();
   for (int i = tid; i < S; i += NT)
   {
      const int ii[3] = {i % D, DIM == 3 ? (i / D) % D : i / D, DIM == 3 ? i / D2 : 0};
      double r = sR[i];
#pragma unroll
      for (int c = 0; c < DIM; c++)
      {
         if (ii[c] != 0 && ii[c] != P) { continue; }
         const int c1 = DIM == 3 ? (c + 1) % 3 : 1 - c, c2 = DIM == 3 ? (c + 2) % 3 : c1;
         r += sB2[(2 * c + (ii[c] == P ? 1 : 0)) * DF + ii[c1] + (DIM == 3 ? D * ii[c2] : 0)];
      }
      rhs[e * S + i] = r; // (read again by the iteration kernel: no streaming store)
   }
   for (int q = tid; q < NQ; q += NT) { wdet[e * NQ + q] = sW[q]; } // (the iteration kernel's mass weights)
}

// n = *n_updates updates of du = 0; du -= (M du - rhs) / m_L on every element; n < 0: nothing to do.  part != null: the squared
// residual norm of the element at the check before update k goes to part[k * ne + e], k < n.  wdet: w detJ at the element's
// quadrature points as neumann_rhs_kernel left them -- no geometry phase here, which keeps this kernel at a fraction of the
// registers and LDS of the kernels that have one.
template <int P, int DIM>
__global__ void __launch_bounds__((EfpCfg<P, DIM>::NT)) neumann_iter_kernel(const double *tab, const double *wdet, const double *rhs,
                                                                           const double *m, const int *n_updates, double *part,
                                                                           double *du)
{
   using C = NmCfg<P, DIM>;
   using T = typename C::T;
   constexpr int D = C::D, Q = C::Q, S = C::S, NQ = C::NQ, NT = C::NT, NW = C::NW;
   __shared__ double sB[Q * D];
   __shared__ double sW[NQ];
   __shared__ double sB1[C::NB1], sB2[C::NB2];
   __shared__ double sR[S], sDu[S], sML[S];
   __shared__ double s_red[4];
   const int n = *n_updates; // (the same word for every workgroup: uniform)
   if (n < 0) { return; }
   const int tid = threadIdx.x;
   const size_t e = blockIdx.x, ne = gridDim.x;
   if (n == 0)
   {
      for (int i = tid; i < S; i += NT) { store_stream(du + e * S + i, 0.0); }
      return;
   }
   for (int i = tid; i < Q * D; i += NT) { sB[i] = tab[T::oB + i]; }
   for (int q = tid; q < NQ; q += NT) { sW[q] = wdet[e * NQ + q]; }
   for (int i = tid; i < S; i += NT)
   {
      sR[i] = rhs[e * S + i];
      sML[i] = m[e * S + i];
   }
   __syncthreads();
   const double *tB = sB;
   for (int it = 0; it < n; it++)
   {
      // (the first residual is -rhs: M 0 needs no sweep)
      const double *y = it == 0 ? nullptr : nm_mass_apply<P, DIM>(sDu, tB, sW, sB1, sB2);
      double acc = 0.0;
      for (int i = tid; i < S; i += NT)
      {
         const double res = it == 0 ? -sR[i] : y[i] - sR[i];
         acc = fma(res, res, acc);
         sDu[i] = (it == 0 ? 0.0 : sDu[i]) - res / sML[i];
      }
      if (part)
      {
         acc = block_sum<NW>(acc, s_red);
         if (tid == 0) { part[(size_t)it * ne + e] = acc; }
      }
      __syncthreads(); // (the next sweep reads every dof's du)
   }
   for (int i = tid; i < S; i += NT) { store_stream(du + e * S + i, sDu[i]); }
}

// norms[k] = sqrt(sum_e part[k][e]) up to the first check that passes; the control words of the second pass and of
// rmh_last_neumann.  One workgroup.
__global__ void __launch_bounds__(NEUMANN_NORMS_NT) neumann_norms_kernel(const double *part, int ne, double *norms, int *ctl)
{
   __shared__ double s_red[NEUMANN_NORMS_NT / 64];
   int K = 0; // the first check (counted from 1) with ||res|| <= tol; 0: none
   int k = 0;
   for (; k < NEUMANN_MAX_UPDATES && K == 0; k++)
   {
      double acc = 0.0;
      for (int e = threadIdx.x; e < ne; e += NEUMANN_NORMS_NT) { acc += part[(size_t)k * ne + e]; }
      const double nrm = sqrt(block_sum<NEUMANN_NORMS_NT / 64>(acc, s_red)); // (the same value in every thread)
      if (threadIdx.x == 0) { norms[k] = nrm; }
      if (nrm <= NEUMANN_TOL) { K = k + 1; }
   }
   if (threadIdx.x == 0)
   {
      ctl[1] = K ? K - 1 : -1;
      ctl[2] = K ? K - 1 : NEUMANN_MAX_UPDATES;
      ctl[3] = k;
   }
}

} // namespace rmh
