// Product-field remap (-ps) on quadrilateral elements (rmh_layout.dim = 2): the per-element pieces of
// AdvectionOperator::LimitMult's second block (remhos.cpp:1848-1915), restating what product_ratio_kernel,
// elem_minmax_masked_kernel and fct_product_kernel of rmh_kernels.hpp compute for hexahedra -- same operations, same
// guards, same divisions.
//
// Shape.  A quadrilateral element has (p + 1)^2 = 4 ... 49 dofs: a wavefront per element, one dof per lane, four elements
// per 256-thread workgroup, grid = ceil(ne / 4).  (The 3-D kernels give an element a workgroup of KCfg<P>::NT threads.)
// Nothing synchronises more than a wavefront: the element's count, sums and extrema go through the DPP trees of
// rmh_ho2.hpp (wave_sum / wave_minmax: a fixed order, the same for every element wherever it sits) and come back to all
// lanes as a scalar (wave_bcast); no LDS, no barrier, no atomics.  A wavefront past the last element leaves before its
// first load; the lanes past the element's last dof stay in the wavefront through every reduction and contribute its
// identity (their loads re-read the last dof, their stores are masked).
#pragma once
#include "rmh_kernels.hpp"
#include "rmh_ho2.hpp"

namespace rmh
{

template <int P>
struct P2Cfg
{
   static constexpr int D2 = (P + 1) * (P + 1);
   static constexpr int NT = 256, NW = NT / 64; // elements per workgroup
   static_assert(D2 <= 64, "one dof per lane");
   static int grid(int ne) { return (ne + NW - 1) / NW; }
};

// the reduction of a value over the wavefront, in all its lanes
__device__ inline double wave_all_sum(double v) { return wave_bcast<63>(wave_sum(v)); }
__device__ inline double wave_all_min(double v) { return wave_bcast<63>(wave_minmax<true>(v)); }
__device__ inline double wave_all_max(double v) { return wave_bcast<63>(wave_minmax<false>(v)); }

// ComputeBoolIndicators (remhos_sync.cpp:23-47) and, with us != null, ComputeRatio (:50-96): s = us / u on the active
// dofs, the mean of the active ratios elsewhere in an active element, 0 in empty elements.
template <int P>
__global__ void __launch_bounds__(P2Cfg<P>::NT) product_ratio2d_kernel(const double *us, const double *u, double *s,
                                                                       unsigned char *active_el, unsigned char *active_dofs, int ne)
{
   using C = P2Cfg<P>;
   const int lane = threadIdx.x & 63;
   const int e = blockIdx.x * C::NW + (threadIdx.x >> 6);
   if (e >= ne) { return; } // (the whole wavefront)
   const bool on = lane < C::D2;
   const size_t g = (size_t)e * C::D2 + min(lane, C::D2 - 1);
   const double ui = u[g];
   const bool act = on && ui > RMH_EMPTY_ZONE_TOL;
   if (on) { active_dofs[g] = act ? 1 : 0; }
   double r = 0.0;
   if (us && act) { r = us[g] / ui; }
   const double cnt = wave_all_sum(act ? 1.0 : 0.0);
   if (lane == 0) { active_el[e] = cnt > 0.0 ? 1 : 0; }
   if (!us) { return; }
   const double sum = wave_all_sum(r);
   const double s_avg = cnt > 0.0 ? sum / cnt : 0.0;
   if (on) { s[g] = act ? r : s_avg; }
}

// DofInfo::ComputeElementsMinMax with the active-element / active-dof masks (remhos_tools.cpp:497-523): inactive
// elements and dofs do not contribute; an inactive element gets (+inf, -inf), the identities of the bounds stencil.
template <int P>
__global__ void __launch_bounds__(P2Cfg<P>::NT) elem_minmax_masked2d_kernel(const double *u, const unsigned char *active_el,
                                                                            const unsigned char *active_dofs, double *xe_min,
                                                                            double *xe_max, int ne)
{
   using C = P2Cfg<P>;
   const int lane = threadIdx.x & 63;
   const int e = blockIdx.x * C::NW + (threadIdx.x >> 6);
   if (e >= ne) { return; }
   const size_t g = (size_t)e * C::D2 + min(lane, C::D2 - 1);
   const bool take = lane < C::D2 && active_el[e] != 0 && active_dofs[g] != 0;
   const double v = u[g];
   const double lmin = wave_all_min(take ? v : INFINITY);
   const double lmax = wave_all_max(take ? v : -INFINITY);
   if (lane == 0) { xe_min[e] = lmin; xe_max[e] = lmax; }
}

// ClipScaleSolver::CalcFCTProduct (remhos_fct.cpp:543-566) in one pass over the element:
//   FCTSolver::CalcCompatibleLOProduct (remhos_fct.cpp:26-115): s_avg = mass_us / mass_u, pulled onto [smin, smax] of the
//     active dofs when it misses them by round-off only, local bounds widened to s_avg where they exclude it (s_min / s_max
//     are updated in place like the reference's), d_us_LO = (u_new s_avg - us) / dt;
//   FCTSolver::ScaleProductBounds (:117-153): us_min/max = s_min/max * u_new on active dofs, 0 elsewhere;
//   ClipScaleSolver::CalcFCTSolution (:449-541) on (us, m, d_us_HO, d_us_LO, us_min, us_max);
//   ZeroOutEmptyDofs (remhos_sync.cpp:98-116): empty elements get d_us = 0.
template <int P>
__global__ void __launch_bounds__(P2Cfg<P>::NT) fct_product2d_kernel(const double *us, const double *m, const double *d_us_ho,
                                                                     double *s_min, double *s_max, const double *u_new,
                                                                     const unsigned char *active_el,
                                                                     const unsigned char *active_dofs, double dt, double *d_us,
                                                                     int ne)
{
   using C = P2Cfg<P>;
   constexpr double eps12 = 1e-12, eps = 1.0e-15;
   const int lane = threadIdx.x & 63;
   const int e = blockIdx.x * C::NW + (threadIdx.x >> 6);
   if (e >= ne) { return; }
   const bool on = lane < C::D2;
   const size_t g = (size_t)e * C::D2 + min(lane, C::D2 - 1);
   const bool el_on = active_el[e] != 0;
   const double usv = us[g], dho = d_us_ho[g], un = u_new[g];
   const double mm = on ? m[g] : 1.0;
   double lo = 0.0, hi = 0.0; // (written below by the dof's own lane: the lanes past the last dof do not read them)
   if (on) { lo = s_min[g]; hi = s_max[g]; }
   const bool act = on && active_dofs[g] != 0;
   const double mass_us = wave_all_sum(on ? (usv + dt * dho) * mm : 0.0);
   const double mass_u = wave_all_sum(on ? un * mm : 0.0);
   const double smin = wave_all_min(act ? lo : INFINITY);
   const double smax = wave_all_max(act ? hi : -INFINITY);
   double s_avg = el_on ? mass_us / mass_u : 0.0;
   // (the reference repeats these two tests for every active dof; they do not depend on the dof)
   if (el_on && s_avg < smin && mass_us + eps12 > smin * mass_u) { s_avg = smin; }
   if (el_on && s_avg > smax && mass_us - eps12 < smax * mass_u) { s_avg = smax; }
   double us_lo = 0.0, us_hi = 0.0, dl = 0.0;
   if (el_on)
   {
      if (act)
      {
         if (s_avg + eps12 < lo) { lo = s_avg; s_min[g] = s_avg; }
         if (s_avg - eps12 > hi) { hi = s_avg; s_max[g] = s_avg; }
         us_lo = lo * un;
         us_hi = hi * un;
      }
      dl = (un * s_avg - usv) / dt;
   }
   const double us_new_lo = usv + dt * dl;
   const double f_clip_min = mm / dt * (us_lo - us_new_lo);
   const double f_clip_max = mm / dt * (us_hi - us_new_lo);
   double fc = mm * (dho - dl);
   fc = fmin(f_clip_max, fmax(f_clip_min, fc));
   const double sumNeg = wave_all_sum(on ? fmin(fc, 0.0) : 0.0);
   const double sumPos = wave_all_sum(on ? fmax(fc, 0.0) : 0.0);
   const double new_mass = sumNeg + sumPos;
   if (new_mass > eps) { fc = fmin(0.0, fc) - fmax(0.0, fc) * sumNeg / sumPos; }
   if (new_mass < -eps) { fc = fmax(0.0, fc) - fmin(0.0, fc) * sumPos / sumNeg; }
   if (on) { d_us[g] = el_on ? dl + fc / mm : 0.0; }
}

} // namespace rmh
