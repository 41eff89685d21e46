// dim = 1: the RK stage on segment lattices (Q2 mesh nodes, Bernstein DG space of order p, Q = p + 1 Gauss-Legendre points --
// the rule of order 2p + 1 that MFEM's integrators pick in one dimension), behind the same C ABI as the other dimensions
// (rmh_layout.dim = 1).  What the reference's regression suite runs on data/periodic-segment.mesh (autotest/test.sh).
//
// Shape: ONE LANE per element.  An element has p + 1 <= 7 dofs and as many quadrature points, so neither the
// workgroup-per-element shape of 3-D nor the wavefront-per-element shape of 2-D fits; every loop over dofs and quadrature
// points is unrolled at compile time (template parameter P) and the element's vectors live in registers -- no LDS, no
// barrier, no cross-lane operation, no atomic in any sum: the summation order is the program order, the same bits from run
// to run.  (The time-step estimate of -dtc 1 is folded with the order-independent atomic minimum the other dimensions use.)
//
// Mass solve.  With Q = p + 1 the quadrature points ARE the Gauss-Legendre nodes of the nodal basis the local mass solve
// works in (DGMassInverse, remhos_ho.cpp:79): in that basis the element mass matrix is the diagonal w_q det J_q, exactly.
// M^-1 = Ci diag(1 / (w det J)) Ci^T with Ci the inverse of the Bernstein collocation matrix B[q][i] -- the exact (dense)
// inverse of the (p + 1) x (p + 1) Bernstein mass matrix, the semantics of -ho 3; no iteration, nothing for
// rmh_set_mass_tol / rmh_set_mass_completion to control.
//
// Neighbours.  The Bernstein basis is interpolatory at both ends: the trace of the neighbour across a face is its dof p or
// dof 0, read straight from u.  The bounds stencil (e - 1, e, e + 1) holds the face neighbours, so a whole stage -- HO, LO,
// the extrema of three elements recomputed from u, bounds, clip + scale, RK update -- depends on u of three elements only and
// is ONE kernel (seg_stage_kernel) with no synchronisation between elements.  The granular entry points launch the same
// device functions one by one.  Lanes past the last element leave before their first load.
//
// Parity path of the reference's 1-D regression cases (10^2 ... 10^4 dofs): written for parity, not timed or tuned.
#pragma once
#include "rmh_kernels.hpp"
#include "rmh_tables.hpp"

namespace rmh
{

template <int P>
struct TabLayout1 : TabLayoutQ<P, P + 1>
{
};

struct SegArgs
{
   const double *x0;     // [ne][3] mesh nodes of the segment (0, 1/2, 1)
   const double *vel;    // [ne][3] remap: displacement; transport: nodal velocity
   const int *face_nbr;  // [ne][2] (left, right) or -1
   const int *st3;       // [ne][3] bounds stencil (e - 1, e, e + 1), -1: none
   const double *tab;    // TabLayout1<P>
   const double *subvel; // [ne][p + 1] sub-mesh node velocity (lo 4) or null
   double t;
   int move;
   double alpha, upw;
   int ne;
};

// what a stage adds to SegArgs (seg_stage_kernel, seg_limit_kernel)
struct SegStageArgs
{
   const double *u, *du_ho, *du_lo; // du_ho / du_lo: seg_limit_kernel only (du_lo null: mass-based average)
   const double *xe_min, *xe_max;   // seg_limit_kernel: element extrema of u; seg_stage_kernel recomputes them
   double *m, *xe_min_out, *xe_max_out; // seg_stage_kernel: lumped mass and extrema of u, left for the context
   int lo_type, bounds_type;
   double dt;
   double *dt_est;
   double *du;
   const double *x_base;
   double a, b, dt_rk;
   double *y_out;
};

template <int P>
struct SegGeo
{
   double wdet[P + 1], dq[P + 1]; // w det J and alpha w v at the quadrature points
   double s0, s1;                 // upwind speeds max(0, +-v . n_out) of the left / right end
};

template <int P>
__device__ inline void seg_geometry(const SegArgs &a, size_t e, double t, SegGeo<P> &g)
{
   using T = TabLayout1<P>;
   const double *L = a.tab + T::oL, *dL = a.tab + T::odL, *W = a.tab + T::oW;
   double X[3], V[3];
#pragma unroll
   for (int k = 0; k < 3; k++)
   {
      const double x = a.x0[e * 3 + k], v = a.vel[e * 3 + k];
      V[k] = v;
      X[k] = a.move ? x + t * v : x;
   }
#pragma unroll
   for (int q = 0; q < T::Q; q++)
   {
      double J = 0.0, vq = 0.0;
#pragma unroll
      for (int k = 0; k < 3; k++)
      {
         J += dL[q * 3 + k] * X[k];
         vq += L[q * 3 + k] * V[k];
      }
      g.wdet[q] = W[q] * J;
      g.dq[q] = a.alpha * W[q] * vq; // adj(J) = 1 for a 1 x 1 Jacobian
   }
   g.s0 = fmax(0.0, a.upw * -V[0]); // outward normal -1 at xi = 0, +1 at xi = 1; the end nodes are mesh nodes
   g.s1 = fmax(0.0, a.upw * V[2]);
}

// lumped mass M 1 = B^T (w det J)
template <int P>
__device__ inline void seg_lumped_mass(const double *tab, const SegGeo<P> &g, double m[P + 1])
{
   using T = TabLayout1<P>;
   const double *B = tab + T::oB;
#pragma unroll
   for (int i = 0; i < T::D; i++)
   {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < T::Q; q++) { s += B[q * T::D + i] * g.wdet[q]; }
      m[i] = s;
   }
}

// the element's u and the traces of its face neighbours (0 on the domain boundary)
template <int P>
__device__ inline void seg_load_u(const SegArgs &a, const double *u, size_t e, double ue[P + 1], double &un0, double &un1)
{
   constexpr int D = P + 1;
#pragma unroll
   for (int i = 0; i < D; i++) { ue[i] = u[e * D + i]; }
   const int n0 = a.face_nbr[e * 2], n1 = a.face_nbr[e * 2 + 1];
   un0 = n0 >= 0 ? u[(size_t)n0 * D + P] : 0.0;
   un1 = n1 >= 0 ? u[(size_t)n1 * D] : 0.0;
}

// D . grad u at the quadrature points (the volume part of K u before the test functions)
template <int P>
__device__ inline void seg_conv_q(const double *tab, const SegGeo<P> &g, const double ue[P + 1], double gq[P + 1])
{
   using T = TabLayout1<P>;
   const double *G = tab + T::oG;
#pragma unroll
   for (int q = 0; q < T::Q; q++)
   {
      double ux = 0.0;
#pragma unroll
      for (int i = 0; i < T::D; i++) { ux += G[q * T::D + i] * ue[i]; }
      gq[q] = g.dq[q] * ux;
   }
}

// LocalInverseHOSolver::CalcHOSolution (remhos_ho.cpp:84-129): du = M^-1 (K_vol + K_face) u, see "Mass solve" above
template <int P>
__device__ inline void seg_ho(const double *tab, const SegGeo<P> &g, const double ue[P + 1], double un0, double un1, double du[P + 1])
{
   using T = TabLayout1<P>;
   constexpr int D = T::D;
   const double *Ci = tab + T::oCi;
   double xg[D];
   seg_conv_q<P>(tab, g, ue, xg);
   const double f0 = g.s0 * (un0 - ue[0]), f1 = g.s1 * (un1 - ue[P]);
#pragma unroll
   for (int q = 0; q < D; q++) { xg[q] = (xg[q] + Ci[q] * f0 + Ci[P * D + q] * f1) / g.wdet[q]; }
#pragma unroll
   for (int i = 0; i < D; i++)
   {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < D; q++) { s += Ci[i * D + q] * xg[q]; }
      du[i] = s;
   }
}

// (PA)ResidualDistribution(Subcell)::CalcLOSolution (remhos_lo.cpp:111-245, 965-1034, 1620-1802); subvel != null: lo 4
template <int P>
__device__ inline void seg_lo_rd(const double *tab, const SegGeo<P> &g, const double ue[P + 1], double un0, double un1,
                                 const double m[P + 1], const double *subvel, double alpha, double du[P + 1])
{
   using T = TabLayout1<P>;
   constexpr int D = T::D;
   constexpr double eps = 1e-15, gamma = 1.0;
   const double *B = tab + T::oB;
   double gq[D], z[D];
   seg_conv_q<P>(tab, g, ue, gq);
   double xmax = ue[0], xmin = ue[0], xsum = 0.0, rhoP = 0.0, rhoN = 0.0;
#pragma unroll
   for (int i = 0; i < D; i++)
   {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < D; q++) { s += B[q * D + i] * gq[q]; }
      z[i] = s;
      rhoP += fmax(0.0, s);
      rhoN += fmin(0.0, s);
      xmax = fmax(xmax, ue[i]);
      xmin = fmin(xmin, ue[i]);
      xsum += ue[i];
   }
   const double sumWP = D * xmax - xsum + eps, sumWN = D * xmin - xsum - eps;
   double wP[D], wN[D];
#pragma unroll
   for (int i = 0; i < D; i++)
   {
      wP[i] = (xmax - ue[i]) / sumWP;
      wN[i] = (xmin - ue[i]) / sumWN;
   }
   if (subvel)
   {
      // subcell fluctuations with the 1-point rule on the closed-uniform sub-mesh (remhos_lo.cpp:1051-1192): subcell k has
      // the corners k, k + 1 and the weights -+ alpha v_mid (adj(J_sub) = 1: the sub-mesh positions do not enter)
      double nwP[D], nwN[D], sumFP = 0.0, sumFN = 0.0;
#pragma unroll
      for (int i = 0; i < D; i++) { nwP[i] = 0.0; nwN[i] = 0.0; }
#pragma unroll
      for (int k = 0; k < P; k++)
      {
         const double vm = alpha * ((subvel[k] + subvel[k + 1]) * 0.5);
         const double fluct = -vm * ue[k] + vm * ue[k + 1];
         const double smax = fmax(ue[k], ue[k + 1]), smin = fmin(ue[k], ue[k + 1]), ssum = ue[k] + ue[k + 1];
         const double fP = fmax(0.0, fluct), fN = fmin(0.0, fluct);
         const double swP = 2 * smax - ssum + eps, swN = 2 * smin - ssum - eps;
         sumFP += fP;
         sumFN += fN;
#pragma unroll
         for (int j = 0; j < 2; j++)
         {
            nwP[k + j] += fP * ((smax - ue[k + j]) / swP);
            nwN[k + j] += fN * ((smin - ue[k + j]) / swN);
         }
      }
      const double auxP = gamma / (rhoP + eps), auxN = gamma / (rhoN - eps);
      const double keepP = 1.0 - fmin(auxP * sumFP, 1.0), addP = fmin(auxP, 1.0 / (sumFP + eps));
      const double keepN = 1.0 - fmin(auxN * sumFN, 1.0), addN = fmax(auxN, 1.0 / (sumFN - eps));
#pragma unroll
      for (int i = 0; i < D; i++)
      {
         wP[i] = wP[i] * keepP + addP * nwP[i];
         wN[i] = wN[i] * keepN + addN * nwN[i];
      }
   }
#pragma unroll
   for (int i = 0; i < D; i++)
   {
      // lumped upwind face fluxes: only the end dofs see a face (remhos_lo.cpp:854-868)
      double fl = 0.0;
      if (i == 0) { fl += g.s0 * (un0 - ue[0]); }
      if (i == P) { fl += g.s1 * (un1 - ue[P]); }
      du[i] = (fl + wP[i] * rhoP + wN[i] * rhoN) / m[i];
   }
}

// MassBasedAvg::CalcLOSolution (remhos_lo.cpp:247-324) with the lumped mass: ubar = int (u + dt du_HO) / int 1
template <int P>
__device__ inline void seg_lo_massavg(const double ue[P + 1], const double du_ho[P + 1], const double m[P + 1], double dt,
                                      double du_lo[P + 1])
{
   double mass = 0.0, vol = 0.0;
#pragma unroll
   for (int i = 0; i <= P; i++)
   {
      mass += m[i] * (ue[i] + dt * du_ho[i]);
      vol += m[i];
   }
   const double ubar = mass / vol;
#pragma unroll
   for (int i = 0; i <= P; i++) { du_lo[i] = (ubar - ue[i]) / dt; }
}

template <int P>
__device__ inline void seg_minmax(const double *ue, double &lo, double &hi)
{
   lo = ue[0];
   hi = ue[0];
#pragma unroll
   for (int i = 1; i <= P; i++)
   {
      lo = fmin(lo, ue[i]);
      hi = fmax(hi, ue[i]);
   }
}

// DofInfo::ComputeBounds from the extrema of the stencil (index 0: e - 1, 1: e, 2: e + 1; absent: +inf / -inf):
// bt 0 overlap bounds (remhos_tools.cpp:432-495: the end dofs share their CG node with the neighbour), bt 1 the element and
// its face neighbours (:381-430)
template <int P>
__device__ inline void seg_bounds(int bt, const double lo[3], const double hi[3], double umin[P + 1], double umax[P + 1])
{
#pragma unroll
   for (int i = 0; i <= P; i++)
   {
      double l = lo[1], h = hi[1];
      if (bt == 1 || i == 0) { l = fmin(l, lo[0]); h = fmax(h, hi[0]); }
      if (bt == 1 || i == P) { l = fmin(l, lo[2]); h = fmax(h, hi[2]); }
      umin[i] = l;
      umax[i] = h;
   }
}

// ClipScaleSolver::CalcFCTSolution (remhos_fct.cpp:449-541)
template <int P>
__device__ inline void seg_clipscale(const double ue[P + 1], const double m[P + 1], const double du_ho[P + 1], const double du_lo[P + 1],
                                     const double umin[P + 1], const double umax[P + 1], double dt, double du[P + 1])
{
   constexpr double eps = 1.0e-15;
   double f[P + 1], sumNeg = 0.0, sumPos = 0.0;
#pragma unroll
   for (int i = 0; i <= P; i++)
   {
      const double u_new_lo = ue[i] + dt * du_lo[i];
      const double f_clip_min = m[i] / dt * (umin[i] - u_new_lo);
      const double f_clip_max = m[i] / dt * (umax[i] - u_new_lo);
      double fc = m[i] * (du_ho[i] - du_lo[i]);
      fc = fmin(f_clip_max, fmax(f_clip_min, fc));
      f[i] = fc;
      sumNeg += fmin(fc, 0.0);
      sumPos += fmax(fc, 0.0);
   }
   const double new_mass = sumNeg + sumPos;
   // (one ratio per element, not one division per dof: new_mass > eps makes sumPos > 0, new_mass < -eps makes sumNeg < 0)
   const double rP = new_mass > eps ? sumNeg / sumPos : 0.0, rN = new_mass < -eps ? sumPos / sumNeg : 0.0;
#pragma unroll
   for (int i = 0; i <= P; i++)
   {
      double fc = f[i];
      if (new_mass > eps) { fc = fmin(0.0, fc) - fmax(0.0, fc) * rP; }
      if (new_mass < -eps) { fc = fmax(0.0, fc) - fmin(0.0, fc) * rN; }
      du[i] = du_lo[i] + fc / m[i];
   }
}

// bounds, clip + scale, the time-step estimate and the RK update y = a x_base + b (u + dt_rk du) of one element: the tail
// shared by the fused limiter and the one-kernel stage
template <int P>
__device__ inline void seg_limit_tail(const SegStageArgs &s, size_t e, const double ue[P + 1], const double m[P + 1],
                                      const double du_ho[P + 1], const double du_lo[P + 1], const double lo[3], const double hi[3])
{
   constexpr int D = P + 1;
   double umin[D], umax[D], du[D];
   seg_bounds<P>(s.bounds_type, lo, hi, umin, umax);
   if (s.dt_est)
   {
      double dtc = INFINITY;
#pragma unroll
      for (int i = 0; i < D; i++) { dtc = fmin(dtc, dt_candidate(ue[i], du_lo[i], umin[i], umax[i])); }
      atomic_min_nonneg(s.dt_est, dtc);
   }
   seg_clipscale<P>(ue, m, du_ho, du_lo, umin, umax, s.dt, du);
#pragma unroll
   for (int i = 0; i < D; i++)
   {
      if (s.du) { s.du[e * D + i] = du[i]; }
      if (s.y_out)
      {
         const double y = ue[i] + s.dt_rk * du[i];
         s.y_out[e * D + i] = (s.x_base ? s.a * s.x_base[e * D + i] : 0.0) + s.b * y;
      }
   }
}

#define RMH_SEG_ELEMENT(ne)                                        \
   const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; \
   if (e >= (size_t)(ne)) { return; }

// MODE 0: HO solution, lumped mass, element extrema; MODE 2: the RD solvers (a.subvel: lo 4), lumped mass, element
// extrema; MODE 4: the lumped mass at time a.t alone (rmh_compute_lumped_mass)
template <int P, int MODE>
__global__ void __launch_bounds__(64) seg_ho_kernel(SegArgs a, const double *u, double *du, double *m, double *xe_min, double *xe_max)
{
   RMH_SEG_ELEMENT(a.ne);
   constexpr int D = P + 1;
   SegGeo<P> g;
   seg_geometry<P>(a, e, a.t, g);
   double me[D];
   seg_lumped_mass<P>(a.tab, g, me);
#pragma unroll
   for (int i = 0; i < D; i++) { m[e * D + i] = me[i]; }
   if (MODE == 4) { return; }
   double ue[D], un0, un1, r[D];
   seg_load_u<P>(a, u, e, ue, un0, un1);
   if (MODE == 0) { seg_ho<P>(a.tab, g, ue, un0, un1, r); }
   else { seg_lo_rd<P>(a.tab, g, ue, un0, un1, me, a.subvel ? a.subvel + e * D : nullptr, a.alpha, r); }
#pragma unroll
   for (int i = 0; i < D; i++) { du[e * D + i] = r[i]; }
   double lo, hi;
   seg_minmax<P>(ue, lo, hi);
   xe_min[e] = lo;
   xe_max[e] = hi;
}

template <int P>
__global__ void __launch_bounds__(64) seg_massavg_kernel(const double *u, const double *du_ho, const double *m, double dt, double *du_lo,
                                                         int ne)
{
   RMH_SEG_ELEMENT(ne);
   constexpr int D = P + 1;
   double ue[D], dh[D], me[D], dl[D];
#pragma unroll
   for (int i = 0; i < D; i++)
   {
      ue[i] = u[e * D + i];
      dh[i] = du_ho[e * D + i];
      me[i] = m[e * D + i];
   }
   seg_lo_massavg<P>(ue, dh, me, dt, dl);
#pragma unroll
   for (int i = 0; i < D; i++) { du_lo[e * D + i] = dl[i]; }
}

template <int P>
__global__ void __launch_bounds__(64) seg_minmax_kernel(const double *u, double *xe_min, double *xe_max, int ne)
{
   RMH_SEG_ELEMENT(ne);
   double lo, hi;
   seg_minmax<P>(u + e * (P + 1), lo, hi);
   xe_min[e] = lo;
   xe_max[e] = hi;
}

// extrema of the stencil of element e from arrays of element extrema
__device__ inline void seg_stencil_extrema(const int *st3, size_t e, const double *xe_min, const double *xe_max, double lo[3], double hi[3])
{
#pragma unroll
   for (int k = 0; k < 3; k++)
   {
      const int nb = st3[e * 3 + k];
      lo[k] = nb >= 0 ? xe_min[nb] : INFINITY;
      hi[k] = nb >= 0 ? xe_max[nb] : -INFINITY;
   }
}

template <int P>
__global__ void __launch_bounds__(64) seg_bounds_kernel(int bt, const int *st3, const double *xe_min, const double *xe_max, double *u_min,
                                                        double *u_max, int ne)
{
   RMH_SEG_ELEMENT(ne);
   constexpr int D = P + 1;
   double lo[3], hi[3], umin[D], umax[D];
   seg_stencil_extrema(st3, e, xe_min, xe_max, lo, hi);
   seg_bounds<P>(bt, lo, hi, umin, umax);
#pragma unroll
   for (int i = 0; i < D; i++)
   {
      u_min[e * D + i] = umin[i];
      u_max[e * D + i] = umax[i];
   }
}

template <int P>
__global__ void __launch_bounds__(64) seg_clipscale_kernel(const double *u, const double *m, const double *du_ho, const double *du_lo,
                                                           const double *u_min, const double *u_max, double dt, double *du, int ne)
{
   RMH_SEG_ELEMENT(ne);
   constexpr int D = P + 1;
   double ue[D], me[D], dh[D], dl[D], lo[D], hi[D], r[D];
#pragma unroll
   for (int i = 0; i < D; i++)
   {
      ue[i] = u[e * D + i];
      me[i] = m[e * D + i];
      dh[i] = du_ho[e * D + i];
      dl[i] = du_lo[e * D + i];
      lo[i] = u_min[e * D + i];
      hi[i] = u_max[e * D + i];
   }
   seg_clipscale<P>(ue, me, dh, dl, lo, hi, dt, r);
#pragma unroll
   for (int i = 0; i < D; i++) { du[e * D + i] = r[i]; }
}

// Fused LimitMult (rmh_limit_fused, rmh_limit_fused_lo): LO rate (mass-based average unless s.du_lo is given), bounds from
// the context's element extrema, clip + scale, RK update -- with the lumped mass s.m left by the HO kernel
template <int P>
__global__ void __launch_bounds__(64) seg_limit_kernel(SegArgs a, SegStageArgs s)
{
   RMH_SEG_ELEMENT(a.ne);
   constexpr int D = P + 1;
   double ue[D], me[D], dh[D], dl[D], lo[3], hi[3];
#pragma unroll
   for (int i = 0; i < D; i++)
   {
      ue[i] = s.u[e * D + i];
      me[i] = s.m[e * D + i];
      dh[i] = s.du_ho[e * D + i];
      dl[i] = s.du_lo ? s.du_lo[e * D + i] : 0.0;
   }
   if (!s.du_lo) { seg_lo_massavg<P>(ue, dh, me, s.dt, dl); }
   seg_stencil_extrema(a.st3, e, s.xe_min, s.xe_max, lo, hi);
   seg_limit_tail<P>(s, e, ue, me, dh, dl, lo, hi);
}

// The whole RK stage of one element (rmh_stage_fused): AdvectionOperator::Mult = MultUnlimited + LimitMult
// (remhos.cpp:1596-1916) and the RK vector update.  Also leaves the lumped mass and the element extrema of u.
template <int P>
__global__ void __launch_bounds__(64) seg_stage_kernel(SegArgs a, SegStageArgs s)
{
   RMH_SEG_ELEMENT(a.ne);
   constexpr int D = P + 1;
   SegGeo<P> g;
   seg_geometry<P>(a, e, a.t, g);
   double me[D], ue[D], un0, un1, dh[D], dl[D], lo[3], hi[3];
   seg_lumped_mass<P>(a.tab, g, me);
   seg_load_u<P>(a, s.u, e, ue, un0, un1);
   seg_ho<P>(a.tab, g, ue, un0, un1, dh);
   if (s.lo_type == 5) { seg_lo_massavg<P>(ue, dh, me, s.dt, dl); }
   else { seg_lo_rd<P>(a.tab, g, ue, un0, un1, me, s.lo_type == 4 ? a.subvel + e * D : nullptr, a.alpha, dl); }
   seg_minmax<P>(ue, lo[1], hi[1]);
#pragma unroll
   for (int k = 0; k < 3; k += 2)
   {
      const int nb = a.st3[e * 3 + k];
      lo[k] = INFINITY;
      hi[k] = -INFINITY;
      if (nb >= 0) { seg_minmax<P>(s.u + (size_t)nb * D, lo[k], hi[k]); }
   }
#pragma unroll
   for (int i = 0; i < D; i++) { s.m[e * D + i] = me[i]; }
   s.xe_min_out[e] = lo[1];
   s.xe_max_out[e] = hi[1];
   seg_limit_tail<P>(s, e, ue, me, dh, dl, lo, hi);
}

} // namespace rmh
