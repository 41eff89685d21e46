// The host driver (include/rmh_driver.h), in this order: the classes of include/remhos_amd/solvers.hpp (Vector, the HO / LO / FCT /
// monolithic solvers, AdvectionOperator, the ODE solvers), which forward to the C ABI; then, in the anonymous namespace, the option
// refusals (validate_config, check_case), the set-up pieces both time loops share (layout, exchange plan, RCCL id rendezvous, step
// clock, result tail), one block through the solver classes (BlockRun: rmhd_run, rmhd_run_state, rmhd_run_rank) and the blocks of
// a partition through the one-kernel stage (rmhd_run_partitioned).
#include "../../include/remhos_amd/solvers.hpp"
#include "../../include/rmh_driver.h"
#include "rmh_host.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <ctime>
#include <memory>
#include <sys/stat.h>
#include <unistd.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace remhos
{

extern thread_local std::string g_driver_error;
CaseConfig to_config(const rmhd_config &c);

void rmh_abort(const char *msg, const char *file, int line)
{
   std::fprintf(stderr, "\nremhos_amd abort: %s\n ... in %s:%d\n ... last rmh error: %s\n", msg, file, line,
                rmh_last_error());
   std::abort();
}

#define RMH_CALL(expr) RMH_VERIFY((expr) == 0, #expr)
#define HIP_CALL(expr) RMH_VERIFY((expr) == hipSuccess, #expr)

// ---- Vector ------------------------------------------------------------------------------
Vector::Vector(int n) { SetSize(n); }
Vector::Vector(const Vector &o)
{
   SetSize(o.size);
   if (size) { HIP_CALL(hipMemcpyAsync(data, o.data, sizeof(double) * size, hipMemcpyDeviceToDevice, nullptr)); }
}
Vector &Vector::operator=(const Vector &o)
{
   if (this == &o) { return *this; }
   if (size != o.size) { SetSize(o.size); }
   if (size) { HIP_CALL(hipMemcpyAsync(data, o.data, sizeof(double) * size, hipMemcpyDeviceToDevice, nullptr)); }
   return *this;
}
Vector::~Vector()
{
   if (own && data) { (void)hipFree(data); }
}
void Vector::SetSize(int n)
{
   if (own && data) { (void)hipFree(data); }
   data = nullptr;
   size = n;
   own = true;
   if (n > 0) { HIP_CALL(hipMalloc((void **)&data, sizeof(double) * n)); }
}
void Vector::CopyFromHost(const double *h)
{
   HIP_CALL(hipMemcpy(data, h, sizeof(double) * size, hipMemcpyHostToDevice));
}
void Vector::CopyToHost(double *h) const
{
   HIP_CALL(hipMemcpy(h, data, sizeof(double) * size, hipMemcpyDeviceToHost));
}

__global__ void fill_kernel(double *z, double v, int n)
{
   for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) { z[i] = v; }
}
__global__ void axpby_kernel(double a, const double *x, double b, const double *y, double *z, int n)
{
   for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
   {
      z[i] = a * x[i] + b * y[i];
   }
}
static int grid_for(int n) { return std::max(1, std::min(2048, (n + 255) / 256)); }

Vector &Vector::operator=(double value)
{
   if (size) { hipLaunchKernelGGL(fill_kernel, dim3(grid_for(size)), dim3(256), 0, nullptr, data, value, size); }
   return *this;
}
void add(const Vector &x, double a, const Vector &y, Vector &z)
{
   const int n = x.Size();
   hipLaunchKernelGGL(axpby_kernel, dim3(grid_for(n)), dim3(256), 0, nullptr, 1.0, x.Read(), a, y.Read(), z.Write(),
                      n);
}
void add(double a, const Vector &x, double b, const Vector &y, Vector &z)
{
   const int n = x.Size();
   hipLaunchKernelGGL(axpby_kernel, dim3(grid_for(n)), dim3(256), 0, nullptr, a, x.Read(), b, y.Read(), z.Write(), n);
}

void TimingData::Update(rmh_ctx *ctx)
{
   double t[4];
   RMH_CALL(rmh_timers(ctx, t));
   sw_rhs = t[0];
   sw_L2inv = t[1];
   sw_LO = t[2];
   sw_FCT = t[3];
}

// ---- solvers: forward to the C ABI ------------------------------------------------------------
void SpaceLayout::ExchangeFaceNbrData(const double *u) const
{
   if (!exchange) { return; }
   RMH_CALL(rmh_exchange_begin(ctx, u));
   RMH_CALL(rmh_exchange_end(ctx));
}
void SpaceLayout::ExchangeElementExtrema(const double *el_min, const double *el_max) const
{
   if (!exchange) { return; }
   RMH_CALL(rmh_exchange_minmax_begin(ctx, el_min, el_max));
   RMH_CALL(rmh_exchange_minmax_end(ctx));
}

LocalInverseHOSolver::LocalInverseHOSolver(ParFiniteElementSpace &space, bool partial_assembly) : HOSolver(space)
{
   // remhos_ho.cpp:77-81 (M_inv->SetAbsTol(1e-8), M_inv->SetRelTol(0.0)) / :104-115 (exact element inverse)
   if (partial_assembly)
   {
      RMH_CALL(rmh_set_mass_tol(pfes.Ctx(), 0.0, 1e-8, 100));
      RMH_CALL(rmh_set_mass_completion(pfes.Ctx(), 1, 1));
   }
   else
   {
      RMH_CALL(rmh_set_mass_tol(pfes.Ctx(), 1e-14, 0.0, 100));
      RMH_CALL(rmh_set_mass_completion(pfes.Ctx(), 0, 0));
   }
}

void LocalInverseHOSolver::CalcHOSolution(const Vector &u, Vector &du) const
{
   RMH_VERIFY(timer, "Timer not set."); // remhos_ho.cpp:86
   pfes.ExchangeFaceNbrData(u.Read());  // remhos_ho.cpp:122 (inside K.Mult for the PA branch)
   RMH_CALL(rmh_ho_apply(pfes.Ctx(), u.Read(), du.Write()));
}

void CGHOSolver::CalcHOSolution(const Vector &u, Vector &du) const
{
   RMH_VERIFY(timer, "Timer not set.");
   double rel, abs;
   int maxit;
   RMH_CALL(rmh_get_mass_tol(pfes.Ctx(), &rel, &abs, &maxit));
   RMH_CALL(rmh_set_mass_tol(pfes.Ctx(), 1e-12, 0.0, 500)); // remhos_ho.cpp:60-63
   pfes.ExchangeFaceNbrData(u.Read());
   RMH_CALL(rmh_ho_apply(pfes.Ctx(), u.Read(), du.Write()));
   RMH_CALL(rmh_set_mass_tol(pfes.Ctx(), rel, abs, maxit));
}

void MassBasedAvg::CalcLOSolution(const Vector &u, Vector &du) const
{
   // remhos_lo.cpp:247-324
   if (du_HO)
   {
      RMH_CALL(rmh_lo_massavg(pfes.Ctx(), u.Read(), du_HO->Read(), dt, du.Write()));
      du_HO = nullptr;
   }
   else
   {
      Vector du_HO_tmp(u.Size());
      ho_solver.CalcHOSolution(u, du_HO_tmp);
      RMH_CALL(rmh_lo_massavg(pfes.Ctx(), u.Read(), du_HO_tmp.Read(), dt, du.Write()));
   }
}

void PAResidualDistribution::CalcLOSolution(const Vector &u, Vector &du) const
{
   RMH_CALL(rmh_lo_rd(pfes.Ctx(), u.Read(), du.Write()));
}

void PAResidualDistributionSubcell::CalcLOSolution(const Vector &u, Vector &du) const
{
   RMH_CALL(rmh_lo_rdsubcell(pfes.Ctx(), u.Read(), du.Write()));
}

void ClipScaleSolver::CalcFCTSolution(const ParGridFunction &u, const Vector &m, const Vector &du_ho,
                                      const Vector &du_lo, const Vector &u_min, const Vector &u_max,
                                      Vector &du) const
{
   RMH_CALL(rmh_fct_clipscale(pfes.Ctx(), u.Read(), m.Read(), du_ho.Read(), du_lo.Read(), u_min.Read(), u_max.Read(),
                              dt, du.Write()));
}

void ClipScaleSolver::CalcFCTProduct(const ParGridFunction &us, const Vector &m, const Vector &d_us_HO, const Vector &d_us_LO,
                                     Vector &s_min, Vector &s_max, const Vector &u_new, const Array<bool> &active_el,
                                     const Array<bool> &active_dofs, Vector &d_us)
{
   (void)d_us_LO; // (only solvers with NeedsLOProductInput() read it, remhos.cpp:1865-1869)
   static_assert(sizeof(bool) == 1, "Array<bool> is handed to the kernels as a byte array");
   RMH_CALL(rmh_fct_product(pfes.Ctx(), us.Read(), m.Read(), d_us_HO.Read(), s_min.ReadWrite(), s_max.ReadWrite(), u_new.Read(),
                            (const unsigned char *)active_el.Read(), (const unsigned char *)active_dofs.Read(), dt, d_us.Write()));
   if (verify_bounds)
   {
      // Check the bounds of the final solution (remhos_fct.cpp:568-610): us + dt d_us against the scaled bounds
      // (s_min u_new, s_max u_new) of ScaleProductBounds on the active dofs, eps = 1e-12.  (The kernel keeps the scaled
      // bounds in registers; s_min / s_max come back updated like the reference's, so the product below IS us_min / us_max.)
      rmh_violation v;
      RMH_CALL(rmh_check_violation(pfes.Ctx(), us.Read(), dt, d_us.Read(), s_min.Read(), s_max.Read(), u_new.Read(), 1e-12,
                                   (const unsigned char *)active_dofs.Read(), &v));
      if (v.count > 0)
      {
         const int nd = pfes.GetNDofs();
         std::printf("Final us %lld %lld %.17g %.17g %.17g\n---\n", v.first % nd, v.first / nd, v.first_min, v.first_value, v.first_max);
         RMH_VERIFY(false, "Bounds violation FCT us.");
      }
   }
}

void ElementFCTProjection::CalcFCTSolution(const ParGridFunction &u, const Vector &m, const Vector &du_ho,
                                           const Vector &du_lo, const Vector &u_min, const Vector &u_max,
                                           Vector &du) const
{
   RMH_CALL(rmh_fct_projection(pfes.Ctx(), u.Read(), m.Read(), du_ho.Read(), du_lo.Read(), u_min.Read(), u_max.Read(),
                               dt, du.Write()));
}

void ElementFCTProjection::CalcFCTProduct(const ParGridFunction &, const Vector &, const Vector &, const Vector &, Vector &,
                                          Vector &, const Vector &, const Array<bool> &, const Array<bool> &, Vector &)
{
   RMH_VERIFY(false, "Product remap (-ps) is not implemented for ElementFCTProjection (-fct 4)");
}

void NeumannHOSolver::CalcHOSolution(const Vector &u, Vector &du) const
{
   // remhos_ho.cpp:136-187 (the assembly-level check of :138-139 is the driver's: ho_type 1 with pa is refused)
   RMH_CALL(rmh_ho_neumann(pfes.Ctx(), u.Read(), du.Write()));
}

void DiscreteUpwind::CalcLOSolution(const Vector &u, Vector &du) const
{
   // remhos_lo.cpp:43-100 (D is rebuilt on the mesh of the operator's time by the kernel: update_D)
   if (preconditioned) { RMH_CALL(rmh_lo_upwind_prec(pfes.Ctx(), u.Read(), du.Write())); } // remhos.cpp:937-942
   else { RMH_CALL(rmh_lo_upwind(pfes.Ctx(), u.Read(), du.Write())); }
}

void FluxBasedFCT::CalcFCTSolution(const ParGridFunction &u, const Vector &m, const Vector &du_ho, const Vector &du_lo,
                                   const Vector &u_min, const Vector &u_max, Vector &du) const
{
   RMH_VERIFY(smth_indicator == NULL, "TODO: update SI bounds."); // remhos_fct.cpp:160
   RMH_VERIFY(iter_cnt == 1, "FluxBasedFCT: one FCT iteration (remhos.cpp:1093)");
   RMH_CALL(rmh_fct_fluxbased(pfes.Ctx(), u.Read(), m.Read(), du_ho.Read(), du_lo.Read(), u_min.Read(), u_max.Read(), dt,
                              du.Write()));
}

void FluxBasedFCT::CalcFCTProduct(const ParGridFunction &, const Vector &, const Vector &, const Vector &, Vector &, Vector &,
                                  const Vector &, const Array<bool> &, const Array<bool> &, Vector &)
{
   RMH_VERIFY(false, "Product remap (-ps) is not implemented for FluxBasedFCT (-fct 1)");
}

MonoRDSolver::MonoRDSolver(ParFiniteElementSpace &space, DofInfo &dofs_, SmoothnessIndicator *si, const double *scale_host,
                           bool subcell, bool timedep, bool masslim)
   : MonolithicSolver(space), dofs(dofs_), smth_indicator(si), scale(space.GetNE()), subcell_scheme(subcell), time_dep(timedep),
     mass_lim(masslim)
{
   RMH_VERIFY(!subcell, "MonoRDSolver: the subcell scheme (-mono 2) is not built");
   RMH_VERIFY(si == NULL, "MonoRDSolver: the smoothness indicator (-si) is not built");
   RMH_VERIFY(scale_host, "MonoRDSolver: scale not given");
   scale.CopyFromHost(scale_host);
}

void MonoRDSolver::CalcSolution(const Vector &u, Vector &du) const
{
   // remhos_mono.cpp:84-99 (the element extrema again inside the kernel), :108-355
   dofs.ComputeElementsMinMax(u, dofs.xe_min, dofs.xe_max);
   dofs.ComputeBounds(dofs.xe_min, dofs.xe_max, dofs.xi_min, dofs.xi_max);
   RMH_CALL(rmh_mono_rd(pfes.Ctx(), u.Read(), dofs.xi_min.Read(), dofs.xi_max.Read(), scale.Read(), mass_lim ? 1 : 0, du.Write()));
}


// remhos.cpp:1557-1594
static void report_violation(const rmh_violation &v, const std::string &info)
{
   if (v.count == 0) { return; }
   std::printf("%s bounds violation: %lld %.17g %.17g %.17g\n%.17g %.17g\n(%lld dofs out of bounds; largest overshoot %.3e, undershoot %.3e)\n",
               info.c_str(), v.first, v.first_min, v.first_value, v.first_max, v.first_max - v.first_value,
               v.first_value - v.first_min, v.count, v.over, v.under);
   std::fflush(stdout);
   RMH_VERIFY(false, "Aborted due to bounds violation.");
}
void check_violation(ParFiniteElementSpace &pfes, const Vector &u_new, const Vector &u_min, const Vector &u_max, std::string info,
                     double tol, const Array<bool> *active_dofs)
{
   rmh_violation v;
   RMH_CALL(rmh_check_violation(pfes.Ctx(), u_new.Read(), 0.0, nullptr, u_min.Read(), u_max.Read(), nullptr, tol,
                                active_dofs ? (const unsigned char *)active_dofs->Read() : nullptr, &v));
   report_violation(v, info);
}
void check_violation(ParFiniteElementSpace &pfes, const Vector &u, double dt, const Vector &du_new, const Vector &u_min,
                     const Vector &u_max, std::string info, double tol, const Array<bool> *active_dofs)
{
   rmh_violation v;
   RMH_CALL(rmh_check_violation(pfes.Ctx(), u.Read(), dt, du_new.Read(), u_min.Read(), u_max.Read(), nullptr, tol,
                                active_dofs ? (const unsigned char *)active_dofs->Read() : nullptr, &v));
   report_violation(v, info);
}

// remhos_sync.cpp:23-96
void ComputeBoolIndicators(ParFiniteElementSpace &pfes, const Vector &u, Array<bool> &ind_elem, Array<bool> &ind_dofs)
{
   RMH_CALL(rmh_product_ratio(pfes.Ctx(), nullptr, u.Read(), nullptr, (unsigned char *)ind_elem.Write(),
                              (unsigned char *)ind_dofs.Write()));
}
void ComputeRatio(ParFiniteElementSpace &pfes, const Vector &us, const Vector &u, Vector &s, Array<bool> &bool_el,
                  Array<bool> &bool_dof)
{
   RMH_CALL(rmh_product_ratio(pfes.Ctx(), us.Read(), u.Read(), s.Write(), (unsigned char *)bool_el.Write(),
                              (unsigned char *)bool_dof.Write()));
}

DofInfo::DofInfo(ParFiniteElementSpace &space)
   : pfes(space), xe_min(space.GetNE()), xe_max(space.GetNE()), xi_min(space.GetVSize()), xi_max(space.GetVSize())
{
}
void DofInfo::ComputeElementsMinMax(const Vector &u, Vector &u_min, Vector &u_max, Array<bool> *active_el,
                                    Array<bool> *active_dof) const
{
   if (active_el && active_dof)
   {
      RMH_CALL(rmh_elem_minmax_masked(pfes.Ctx(), u.Read(), (const unsigned char *)active_el->Read(),
                                      (const unsigned char *)active_dof->Read(), u_min.Write(), u_max.Write()));
      return;
   }
   RMH_CALL(rmh_elem_minmax(pfes.Ctx(), u.Read(), u_min.Write(), u_max.Write()));
}
void DofInfo::ComputeBounds(const Vector &el_min, const Vector &el_max, Vector &dof_min, Vector &dof_max) const
{
   pfes.ExchangeElementExtrema(el_min.Read(), el_max.Read()); // remhos_tools.cpp:461-466
   RMH_CALL(rmh_bounds(pfes.Ctx(), el_min.Read(), el_max.Read(), dof_min.Write(), dof_max.Write()));
}

// ---- AdvectionOperator (remhos.cpp:1596-1739, 1798-1916) -----------------------------------------
AdvectionOperator::AdvectionOperator(ParFiniteElementSpace &space, DofInfo &dofs_, HOSolver *hos, LOSolver *los,
                                     FCTSolver *fct, bool fused_limiter, bool product_sync)
   : LimitedTimeDependentOperator((product_sync ? 2 : 1) * space.GetVSize()), pfes(space), dofs(dofs_), ho_solver(hos),
     lo_solver(los), fct_solver(fct),
     lumpedM(rmh_lumped_mass(space.Ctx()) ? const_cast<double *>(rmh_lumped_mass(space.Ctx())) : nullptr, space.GetVSize()),
     du_HO(space.GetVSize()), du_LO(fused_limiter ? 0 : space.GetVSize()), d_us_HO(product_sync ? space.GetVSize() : 0),
     s_ratio(product_sync ? space.GetVSize() : 0), u_new(product_sync ? space.GetVSize() : 0), fused(fused_limiter),
     product(product_sync)
{
   if (ho_solver) { ho_solver->timer = &timer; }
   if (lo_solver) { lo_solver->timer = &timer; }
   if (fct_solver) { fct_solver->timer = &timer; }
   if (product)
   {
      // flag arrays of product remap (mfem::Array<bool> on the device)
      static_assert(sizeof(bool) == 1, "Array<bool> is handed to the kernels as a byte array");
      const int ne = space.GetNE(), n = space.GetVSize();
      bool *p = nullptr;
      HIP_CALL(hipMalloc((void **)&p, (size_t)2 * (ne + n)));
      s_bool_el.MakeRef(p, ne);
      s_bool_dofs.MakeRef(p + ne, n);
      s_bool_el_new.MakeRef(p + ne + n, ne);
      s_bool_dofs_new.MakeRef(p + 2 * ne + n, n);
   }
}

AdvectionOperator::~AdvectionOperator()
{
   if (product) { (void)hipFree(s_bool_el.Write()); }
}

void AdvectionOperator::MultUnlimited(const Vector &X, Vector &Y) const
{
   // remap: move the mesh to the stage time and re-set-up M_HO, K_HO, lumpedM
   // (remhos.cpp:1598-1637) -- matrix-free here: the kernels evaluate x0 + t*v themselves
   RMH_CALL(rmh_setup(pfes.Ctx(), GetTime()));
   const int n = pfes.GetVSize();
   if (mono_solver) // remhos.cpp:1687
   {
      const Vector u(const_cast<double *>(X.Read()), n);
      Vector d_u(Y.Write(), n);
      mono_solver->CalcSolution(u, d_u);
      return;
   }
   RMH_VERIFY(ho_solver && lo_solver && fct_solver, "FCT requires HO and LO solvers."); // remhos.cpp:1690
   if (product)
   {
      // Remap the product field (remhos.cpp:1709-1738).  Its HO rate is formed FIRST: the context keeps the element
      // extrema of the last vector rmh_ho_apply saw, and the fused limiter of u relies on them.
      const Vector us(const_cast<double *>(X.Read()) + n, n);
      Vector d_us(Y.Write() + n, n);
      ho_solver->CalcHOSolution(us, d_us);
   }
   const Vector u(const_cast<double *>(X.Read()), n);
   Vector d_u(Y.Write(), n);
   ho_solver->CalcHOSolution(u, d_u);
   // Limiting is deferred to LimitMult()
}

void AdvectionOperator::LimitMult(const Vector &X, Vector &Y) const
{
   if (mono_solver) { return; } // (the monolithic solver's result is final: the reference's Mult has no limiting step either)
   const int n = pfes.GetVSize();
   const Vector u(const_cast<double *>(X.Read()), n);
   Vector d_u(Y.Write(), n);
   if (fused)
   {
      if (verify_bounds) { du_HO = d_u; } // (the fused kernel overwrites the HO rate; the check re-forms the LO rate from it)
      // d_u holds du_HO on entry; the fused kernel reads du_HO and writes d_u element by element
      RMH_CALL(rmh_limit_fused(pfes.Ctx(), u.Read(), d_u.Read(), dt, d_u.Write(), nullptr, 0.0, 1.0, 0.0, nullptr));
      if (verify_bounds)
      {
         // remhos.cpp:1824-1837 for the fused limiter: it keeps du_LO and the dof bounds in registers, so the granular
         // kernels form them once more for the check
         if (du_LO.Size() != n) { du_LO.SetSize(n); }
         auto mba = dynamic_cast<MassBasedAvg *>(lo_solver);
         if (mba) { mba->SetHOSolution(du_HO); }
         lo_solver->CalcLOSolution(u, du_LO);
         dofs.ComputeElementsMinMax(u, dofs.xe_min, dofs.xe_max);
         dofs.ComputeBounds(dofs.xe_min, dofs.xe_max, dofs.xi_min, dofs.xi_max);
         check_violation(pfes, u, dt, du_LO, dofs.xi_min, dofs.xi_max, "LimitMult LO u", 1e-12, nullptr);
         check_violation(pfes, u, dt, d_u, dofs.xi_min, dofs.xi_max, "LimitMult FCT solution u", 1e-12, nullptr);
      }
   }
   else
   {
      // the reference's sequence, remhos.cpp:1812-1831 (the x_gf face-neighbour exchange at
      // :1812-1813 is dead weight for ClipScale and is skipped)
      du_HO = d_u; // Vector du_HO(d_u)
      auto mba = dynamic_cast<MassBasedAvg *>(lo_solver);
      if (mba) { mba->SetHOSolution(du_HO); }
      lo_solver->CalcLOSolution(u, du_LO);
      dofs.ComputeElementsMinMax(u, dofs.xe_min, dofs.xe_max);
      dofs.ComputeBounds(dofs.xe_min, dofs.xe_max, dofs.xi_min, dofs.xi_max);
      if (verify_bounds) { check_violation(pfes, u, dt, du_LO, dofs.xi_min, dofs.xi_max, "LimitMult LO u", 1e-12, nullptr); } // :1824-1828
      fct_solver->CalcFCTSolution(u, lumpedM, du_HO, du_LO, dofs.xi_min, dofs.xi_max, d_u);
      if (verify_bounds) { check_violation(pfes, u, dt, d_u, dofs.xi_min, dofs.xi_max, "LimitMult FCT solution u", 1e-12, nullptr); } // :1833-1837
      UpdateTimeStepEstimate(u, du_LO, dofs.xi_min, dofs.xi_max); // remhos.cpp:1839-1842 (no-op with a fixed dt)
   }
   if (!product) { return; }
   // Remap the product field (remhos.cpp:1848-1915)
   const Vector us(const_cast<double *>(X.Read()) + n, n);
   Vector d_us(Y.Write() + n, n);
   d_us_HO = d_us; // Vector d_us_HO(d_us)
   Vector d_us_LO;
   RMH_VERIFY(!fct_solver->NeedsLOProductInput(), "no FCT solver on this path needs the LO product rate"); // :1866-1870
   // Compute the ratio s = us_old / u_old, and old active dofs.
   ComputeRatio(pfes, us, u, s_ratio, s_bool_el, s_bool_dofs);
   // Bounds for s, based on the old values (and old active dofs).
   dofs.ComputeElementsMinMax(s_ratio, dofs.xe_min, dofs.xe_max, &s_bool_el, &s_bool_dofs);
   dofs.ComputeBounds(dofs.xe_min, dofs.xe_max, dofs.xi_min, dofs.xi_max); // (+inf, -inf) of inactive elements = "&s_bool_el"
   // Evolve u and get the new active dofs.
   add(u, dt, d_u, u_new);
   ComputeBoolIndicators(pfes, u_new, s_bool_el_new, s_bool_dofs_new);
   fct_solver->CalcFCTProduct(us, lumpedM, d_us_HO, d_us_LO, dofs.xi_min, dofs.xi_max, u_new, s_bool_el_new, s_bool_dofs_new,
                              d_us);
}

void AdvectionOperator::UpdateTimeStepEstimate(const Vector &x, const Vector &dx, const Vector &x_min,
                                               const Vector &x_max) const
{
   RMH_CALL(rmh_dt_estimate_update(pfes.Ctx(), x.Read(), dx.Read(), x_min.Read(), x_max.Read()));
}
void AdvectionOperator::ResetTimeStepRatio() const { RMH_CALL(rmh_dt_estimate_reset(pfes.Ctx())); }
real_t AdvectionOperator::GetTimeStepRatio() const
{
   double est = 0.0;
   RMH_CALL(rmh_dt_estimate_get(pfes.Ctx(), &est));
   return (dt != 0.) ? est / dt : 0.; // remhos.cpp:1997
}

// ---- IDP solvers (remhos_solvers.cpp) ---------------------------------------------------------------------------------
void ForwardEulerIDPSolver::Init(LimitedTimeDependentOperator &f_)
{
   IDPODESolver::Init(f_);
   dx.SetSize(f_.Height());
}
void ForwardEulerIDPSolver::Step(Vector &x, real_t &t, real_t &dt)
{
   // one limited leg over the whole step (the reference's -s 11, remhos_solvers.cpp:30-40)
   f->SetTime(t);
   f->SetDt(dt);
   f->MultUnlimited(x, dx);
   f->LimitMult(x, dx);
   add(x, dt, dx, x);
   t += dt;
}

// An explicit Runge-Kutta method  X_i = x_n + dt sum_j A_ij k_j  (last row: the weights b, abscissa 1) run as a chain of
// LIMITED forward Euler legs (the reference's RKIDPSolver, remhos_solvers.hpp:94-126; masks absent, remhos.cpp:502-507).
// The chain stands at a state that is itself a row of the tableau, "here"; leg i has to carry it to row i over the
// pseudo-time span = abscissa_i - at.  As an Euler rate that is
//      U_i = sum_j (A_ij - here_j) / span * k_j ,
// but the earlier k_j are gone: what the chain kept of stage j is its limited rate L_j = limit(U_j).  Reading U_j = L_j
// backwards gives every earlier k_j as a combination of L_0 .. L_j ("worth"), and U_i becomes
//      U_i = w_i k_i + sum_{k<i} w_k L_k .
// A leg whose successor's abscissa does not lie ahead of its own is limited and remembered, but the chain stays put.
std::vector<RKIDPSolver::EulerLeg> RKIDPSolver::PlanLegs(int stages, const real_t *a_packed, const real_t *b_row, const real_t *c_abs)
{
   auto row = [&](int i) { return (i < stages - 1) ? a_packed + i * (i + 1) / 2 : b_row; };
   auto abscissa = [&](int i) { return (i < stages - 1) ? c_abs[i] : real_t(1); };
   std::vector<std::vector<real_t>> worth(stages, std::vector<real_t>(stages, 0.)); // k_j = sum_k worth[j][k] L_k
   std::vector<real_t> here(stages, 0.);
   real_t at = 0.;
   std::vector<EulerLeg> legs(stages);
   for (int i = 0; i < stages; i++)
   {
      EulerLeg &leg = legs[i];
      leg.from = at;
      leg.span = abscissa(i) - at;
      RMH_VERIFY(leg.span > 0. && row(i)[i] != 0., "tableau cannot be run as forward Euler legs");
      leg.w.assign(i + 1, 0.);
      for (int j = 0; j < i; j++)
      {
         const real_t g = (row(i)[j] - here[j]) / leg.span;
         if (g == 0.) { continue; }
         for (int k = 0; k <= j; k++) { leg.w[k] += g * worth[j][k]; }
      }
      leg.w[i] = row(i)[i] / leg.span;
      for (int k = 0; k < i; k++) { worth[i][k] = -leg.w[k] / leg.w[i]; }
      worth[i][i] = 1. / leg.w[i];
      leg.lands = (i == stages - 1) || abscissa(i + 1) > abscissa(i);
      if (leg.lands)
      {
         at = abscissa(i);
         for (int j = 0; j < stages; j++) { here[j] = (j <= i) ? row(i)[j] : 0.; }
      }
   }
   return legs;
}

RKIDPSolver::RKIDPSolver(int stages, const real_t a_packed[], const real_t b_row[], const real_t c_abs[])
   : legs(PlanLegs(stages, a_packed, b_row, c_abs)), limited(stages)
{
}
void RKIDPSolver::Init(LimitedTimeDependentOperator &f_)
{
   IDPODESolver::Init(f_);
   for (Vector &v : limited) { v.SetSize(f->Height()); }
}
void RKIDPSolver::Step(Vector &x, real_t &t, real_t &dt)
{
   f->SetTime(t);
   for (size_t i = 0; i < legs.size(); i++)
   {
      const EulerLeg &leg = legs[i];
      Vector &rate = limited[i];
      f->SetDt(leg.span * dt);
      f->MultUnlimited(x, rate); // k_i at the state (and mesh position) the chain stands at
      if (i > 0 || leg.w[0] != 1.)
      {
         add(leg.w[i], rate, (i > 0) ? leg.w[0] : 0., limited[0], rate);
         for (size_t k = 1; k < i; k++) { add(rate, leg.w[k], limited[k], rate); }
      }
      f->LimitMult(x, rate); // rate: U_i in, L_i out
      if (leg.lands)
      {
         add(x, leg.span * dt, rate, x);
         f->SetTime(t + (leg.from + leg.span) * dt);
      }
   }
   t += dt;
}

// midpoint rule and the three-stage third-order method that the reference runs as -s 12 / -s 13 (remhos_solvers.cpp:252-260):
// lower-triangular rows packed one after the other, weights, abscissae
const real_t RK2IDPSolver::a[] = {1. / 2.};
const real_t RK2IDPSolver::b[] = {0., 1.};
const real_t RK2IDPSolver::c[] = {1. / 2.};
const real_t RK3IDPSolver::a[] = {1. / 3., /**/ 0., 2. / 3.};
const real_t RK3IDPSolver::b[] = {1. / 4., 0., 3. / 4.};
const real_t RK3IDPSolver::c[] = {1. / 3., 2. / 3.};

// ---- RK3 SSP [MFEM RK3SSPSolver::Step] -------------------------------------------------------------
void RK3SSPSolver::Init(LimitedTimeDependentOperator &op)
{
   f = &op;
   y.SetSize(op.Height());
   k.SetSize(op.Height());
}
// The schedule of the method, read by RK3SSPSolver::Step and by both one-kernel stage loops below: stage i takes its input x_i
// (x_0 = x) at the time t + c dt and leaves  a x + b (x_i + dt f(t + c dt, x_i))  -- x_1, x_2 and the new x.
struct RK3SSPStage { double c, a, b; };
constexpr RK3SSPStage RK3SSP[3] = {{0., 0., 1.}, {1., 3. / 4, 1. / 4}, {1. / 2, 1. / 3, 2. / 3}};

void RK3SSPSolver::Step(Vector &x, real_t &t, real_t &dt)
{
   for (int i = 0; i < 3; i++)
   {
      const RK3SSPStage &st = RK3SSP[i];
      const Vector &xi = (i == 0) ? x : y;
      f->SetTime(t + st.c * dt);
      f->Mult(xi, k);
      add(xi, dt, k, y);
      if (i > 0) { add(st.a, x, st.b, y, (i == 2) ? x : y); } // (stage 0: a = 0, b = 1)
   }
   t += dt;
}

} // namespace remhos

using namespace remhos;

namespace
{
int refuse(const std::string &why) { g_driver_error = why; return -1; }

// ---- option refusals ---------------------------------------------------------------------------------------------------
// Every option set the entry points refuse is refused in one of two places: validate_config (what rmhd_config alone decides, before
// a case is built) and check_case (what needs the built CaseData: dimension, order, exec_mode).  A new rule goes into the one that
// can decide it, at the place its precedence asks for: the FIRST rule that fails is the one reported, and
// tests/golden/driver_refusals.json pins which.
bool is_segment_mesh(const rmhd_config &cfg) { return std::strncmp(cfg.mesh, "periodic-segment", sizeof(cfg.mesh)) == 0; }

// An unstructured quadrilateral mesh from a file (rmhd_config.mesh_file; data/star-q2.mesh, data/periodic-hexagon.mesh): the name is
// none of the built-in lattices and the file can be opened.  (Neither: the case builder answers "unknown lattice mesh".)
bool is_file_mesh(const rmhd_config &cfg)
{
   if (is_builtin_mesh(std::string(cfg.mesh, strnlen(cfg.mesh, sizeof(cfg.mesh)))) || !cfg.mesh_file[0]) { return false; }
   if (strnlen(cfg.mesh_file, sizeof(cfg.mesh_file)) == sizeof(cfg.mesh_file)) { return false; }
   FILE *f = std::fopen(cfg.mesh_file, "r");
   if (f) { std::fclose(f); }
   return f != nullptr;
}

struct Validated
{
   std::string refusal; // empty: `cfg` is the effective config
   rmhd_config cfg;     // the caller's, with pa cleared on a segment mesh and -ho / -lo / -fct / -pa at their defaults beside -mono
};

// What the entry points accept of rmhd_config, before a device context exists.  partitioned_entry: rmhd_run_partitioned; id_file:
// the caller names an RCCL id file (one process per block).  The groups, in the order they are asked: dim = 1, a mesh file,
// -mono, -ho / -lo / -fct, the entry point's own rule.
Validated validate_config(const rmhd_config &in, bool partitioned_entry, bool id_file)
{
   Validated v{std::string(), in};
   rmhd_config &cfg = v.cfg;
   std::string &no = v.refusal;
   const char *why = nullptr;
   const int ode = cfg.ode_solver;
   // "is this run partitioned" has two spellings, and they stay: the second also refuses rank != 0 on one block, which the first
   // leaves to the case builder ("bad rank")
   const bool many_blocks = partitioned_entry || cfg.px * cfg.py * cfg.pz > 1;
   const bool many_blocks_or_rank = partitioned_entry || cfg.px > 1 || cfg.py > 1 || cfg.pz > 1 || cfg.rank != 0;

   // dim = 1 (-m data/periodic-segment.mesh): what a segment run takes -- -ho 2|3, -lo 3|4|5, -fct 2, -s 3, one block
   if (is_segment_mesh(cfg))
   {
      const int lo = cfg.lo_type, fct = cfg.fct_type;
      if (cfg.ps) { why = "ps (-ps): product remap"; }
      else if (ode != 0 && ode != 3) { why = "ode_solver (-s 11|12|13): the IDP solvers"; }
      else if (cfg.ho_type == 1) { why = "ho_type 1 (-ho 1): the Neumann HO solver"; }
      else if (lo == 1 || lo == 2) { why = "lo_type 1|2 (-lo 1|2): the DiscreteUpwind LO solvers"; }
      else if (fct == 1 || fct == 4) { why = "fct_type 1|4 (-fct 1|4): the flux-based and element-projection FCT solvers"; }
      else if (cfg.mono_type) { why = "mono_type (-mono): the monolithic RD solver"; }
      else if (many_blocks_or_rank) { why = "partitions (px, py, pz, rank): box-partitioned runs"; }
      else if (cfg.self_wrap) { why = "self_wrap: the self-wrapped halo"; }
      else if (cfg.save) { why = "save (-save): the MFEM mesh / field writer"; }
      if (why) { no = std::string(why) + " is not available for dim = 1 (periodic-segment: -ho 2|3, -lo 3|4|5, -fct 2, -s 3, one block)"; return v; }
      if (cfg.pa)
      {
         // remhos.cpp:474-480; the element mass solve of a segment is exact either way (rmh_1d.hpp)
         std::printf("Disabling PA / FA for 1D.\n");
         std::fflush(stdout);
         cfg.pa = 0;
      }
   }
   // a mesh file takes -ho 2|3 [-pa], -lo 3|4|5, -fct 2, -bt, -dtc, -vb, -s 3 on one block through the granular solver sequence
   if (is_file_mesh(cfg))
   {
      const int lo = cfg.lo_type, fct = cfg.fct_type;
      if (many_blocks_or_rank) { why = "partitions (px, py, pz, rank): box-partitioned runs are"; }
      else if (cfg.mono_type) { why = "mono_type (-mono): the monolithic RD solver is"; }
      else if (cfg.fused) { why = "fused = 1: the fused limiter and the one-kernel stage (they read the neighbour tables with the lattice rule) are"; }
      else if (cfg.ho_type == 1) { why = "ho_type 1 (-ho 1): the Neumann HO solver is"; }
      else if (lo == 1 || lo == 2) { why = "lo_type 1|2 (-lo 1|2): the DiscreteUpwind LO solvers are"; }
      else if (fct == 1) { why = "fct_type 1 (-fct 1): the flux-based FCT solver is"; }
      else if (fct == 4) { why = "fct_type 4 (-fct 4): the element FCT projection is"; }
      else if (cfg.ps) { why = "ps (-ps): product remap is"; }
      else if (ode != 0 && ode != 3) { why = "ode_solver (-s 11|12|13): the IDP solvers are"; }
      else if (cfg.self_wrap) { why = "self_wrap: the self-wrapped halo is"; }
      else if (cfg.save) { why = "save (-save): the MFEM mesh / field writer is"; }
      if (why) { no = std::string(why) + " not available on an unstructured mesh file (-ho 2|3 [-pa], -lo 3|4|5, -fct 2, -bt 0|1, -dtc 0|1, -vb, -s 3, one block, fused = 0)"; return v; }
   }
   if (const int mono = cfg.mono_type)
   {
      if (mono == 2) { no = "mono_type 2 (-mono 2): the subcell variant of the monolithic RD solver (ResDistMonoSubcell) is not built"; }
      else if (mono != 1) { no = "mono_type must be 0 (off) or 1 (-mono 1, MonoRDSolver): got " + std::to_string(mono); }
      else if (many_blocks) { no = "mono_type 1 (-mono 1): partitioned runs are not built for the monolithic RD solver (one block, rmhd_run with fused = 0)"; }
      else if (cfg.self_wrap) { no = "mono_type 1 (-mono 1): a self-wrapped block (self_wrap) has ghost elements, which rmh_mono_rd does not take"; }
      else if (cfg.fused) { no = "mono_type 1 (-mono 1): the fused limiter and the one-kernel stage are the HO / LO / FCT split the monolithic solver replaces (fused must be 0)"; }
      else if (cfg.ps) { no = "mono_type 1 (-mono 1) with -ps: product remap (ps) is not built for the monolithic RD solver"; }
      else if (ode != 0 && ode != 3) { no = "mono_type 1 (-mono 1): runs through RK3 SSP (-s 3); the IDP solvers limit a rate the monolithic solver does not have"; }
      else if (cfg.dt_control) { no = "mono_type 1 (-mono 1) with -dtc: the time step estimate is formed from the LO solution, which the monolithic solver does not have"; }
      if (!no.empty()) { return v; }
      // -ho, -lo and -fct are ignored beside -mono, as in the reference (remhos.cpp:1687): they take their defaults here
      cfg.ho_type = 0; cfg.lo_type = 5; cfg.fct_type = 0; cfg.pa = 0;
   }
   // -ho: 0 means 3; no other value may fall through to the local inverse
   if (cfg.ho_type < 0 || cfg.ho_type > 3) { no = "ho_type must be 1 (Neumann iteration), 2 (CG) or 3 (local inverse; 0 means 3): got " + std::to_string(cfg.ho_type); return v; }
   if (cfg.ho_type == 1)
   {
      // NeumannHOSolver (-ho 1) runs through the granular solver sequence on one block: its stopping test is a global norm
      if (many_blocks) { no = "ho_type 1 (-ho 1): partitioned runs are not built for the Neumann HO solver (one block, rmhd_run with fused = 0)"; }
      else if (cfg.self_wrap) { no = "ho_type 1 (-ho 1): a self-wrapped block (self_wrap) has ghost elements, which rmh_ho_neumann does not take"; }
      else if (cfg.fused) { no = "ho_type 1 (-ho 1): the one-kernel stage has the local inverse built in (fused must be 0)"; }
      else if (cfg.pa) { no = "ho_type 1 (-ho 1) with -pa: PA for DG is not supported for Neummann Solver"; } // remhos_ho.cpp:138-139
      else if (cfg.ps) { no = "ho_type 1 (-ho 1) with -ps: product remap (ps) is not built for the Neumann HO solver"; }
      if (!no.empty()) { return v; }
   }
   const int fct = cfg.fct_type;
   if (fct != 0 && fct != 1 && fct != 2 && fct != 4) { no = "fct_type must be 1 (flux-based FCT), 2 (clip + scale; 0 means 2) or 4 (element FCT projection)"; return v; }
   if (fct == 1 || cfg.lo_type == 1 || cfg.lo_type == 2)
   {
      // DiscreteUpwind (-lo 1, preconditioned: -lo 2) and FluxBasedFCT (-fct 1) run through the granular solver sequence on one block
      const std::string who = fct == 1 ? "fct_type 1" : (cfg.lo_type == 2 ? "lo_type 2" : "lo_type 1");
      if (many_blocks) { no = who + ": partitioned runs are not built for the DiscreteUpwind / FluxBasedFCT solvers (one block, rmhd_run with fused = 0)"; }
      else if (cfg.fused) { no = who + ": the fused limiter and the one-kernel stage have their LO solver and clip + scale built in (fused must be 0)"; }
      else if (cfg.ps) { no = who + ": product remap (ps) is not implemented for the DiscreteUpwind / FluxBasedFCT solvers"; }
      else if (fct == 1 && cfg.pa) { no = "Flux-based FCT and PA are incompatible."; } // remhos.cpp:1088
      else if (fct == 1 && cfg.self_wrap) { no = "fct_type 1: a self-wrapped block has ghost elements, which rmh_fct_fluxbased does not take"; }
      if (!no.empty()) { return v; }
   }
   if (fct == 4)
   {
      if (partitioned_entry) { no = "rmhd_run_partitioned runs the one-kernel stage, which has clip + scale built in: fct_type 4 runs through rmhd_run / rmhd_run_rank with fused = 0"; }
      else if (cfg.fused) { no = "fct_type 4: the fused limiter and the one-kernel stage have clip + scale built in (fused must be 0)"; }
      else if (cfg.ps) { no = "fct_type 4: product remap (ps) is not implemented for the element FCT projection"; }
      if (!no.empty()) { return v; }
   }
   // the entry point's own rule
   const CaseConfig cc = to_config(cfg);
   if (partitioned_entry && !cfg.fused) { no = "rmhd_run_partitioned runs the one-kernel stage (fused = 1)"; }
   else if (!partitioned_entry && cc.px * cc.py * cc.pz != 1 && !id_file) { no = "rmhd_run drives one block; box-partitioned runs go through rmhd_run_partitioned, or through rmhd_run_rank with one process per block"; }
   return v;
}

// The refusals that need the built case: its dimension, order and exec_mode
std::string check_case(const rmhd_config &cfg, const CaseConfig &cc, const CaseData &cd, bool partitioned_entry)
{
   if (partitioned_entry) { return cd.dim != 3 ? "the partitioned stage loop is for the 3-D cases" : ""; }
   if (cc.lo_type == 2 && cd.dim == 3 && cd.order >= 4) { return "lo_type 2 (-lo 2): order " + std::to_string(cd.order) + " in 3-D is not supported: the element's dense matrices must fit the LDS (orders 1 to 3 in 3-D, 1 to 6 in 2-D)"; }
   if (cfg.mono_type && cd.dim == 3 && cd.order >= 4) { return "mono_type 1 (-mono 1): order " + std::to_string(cd.order) + " in 3-D is not supported: the element's mass matrix must stay in the LDS over the passes of the mass iteration (orders 1 to 3 in 3-D, 1 to 6 in 2-D)"; }
   if (cfg.ps)
   {
      // what product remap (-ps) asks of the other options, in 3-D and in 2-D alike
      if (cd.exec_mode != 1) { return "Products are processed only in remap mode."; }                  // remhos.cpp:1713
      if (cfg.dt_control) { return "Automatic time step is not implemented for product remap."; }      // remhos.cpp:1714
      if (cc.lo_type != 5) { return "product remap is built for -lo 5 (what the fused limiter kernel takes)"; }
   }
   return "";
}

// ---- set-up pieces of both time loops ------------------------------------------------------------------------------------
struct CtxDelete { void operator()(rmh_ctx *c) const { rmh_destroy(c); } };
typedef std::unique_ptr<rmh_ctx, CtxDelete> CtxPtr;

rmh_layout make_layout(const CaseData &cd, int device)
{
   rmh_layout L;
   L.dim = cd.dim; L.order = cd.order; L.mesh_order = 2; L.exec_mode = cd.exec_mode; // (dim 2: build_case_2d, one rank)
   L.ne_owned = cd.ne_owned; L.ne_ghost = cd.ne_ghost; // (> 0: a self-wrapped block -- rmhd_config.self_wrap -- or a block of a partition)
   L.x0 = cd.x0.data(); L.vel = cd.vel.data(); L.face_nbr = cd.face_nbr.data(); L.stencil27 = cd.stencil27.data();
   L.subcell_vel = cd.subcell_vel.empty() ? nullptr : cd.subcell_vel.data();
   L.device = device;
   return L;
}

// The exchange plan of a block from the case builder's halo lists; compact records unless a block is one element thin
struct ExchangePlan
{
   std::vector<int> prank, scount, rfirst, rcount;
   std::vector<const int *> selems;
   bool thin = false;
   ExchangePlan(const CaseData &cd, const CaseConfig &cc)
   {
      for (const Peer &pr : cd.peers)
      {
         prank.push_back(pr.rank);
         scount.push_back((int)pr.send_elems.size());
         selems.push_back(pr.send_elems.data());
         rfirst.push_back(pr.recv_slots.empty() ? 0 : pr.recv_slots.front());
         rcount.push_back((int)pr.recv_slots.size());
      }
      const int P3[3] = {cc.px, cc.py, cc.pz};
      for (int dd = 0; dd < 3; dd++) { thin = thin || (P3[dd] > 1 && cd.n[dd] / P3[dd] < 2); }
   }
   bool only_peer_is(int rank) const { return prank.size() == 1 && prank[0] == rank; }
   int setup(rmh_ctx *ctx) const
   {
      const rmh_exchange_desc d = {(int)prank.size(), prank.data(), scount.data(), selems.data(), rfirst.data(), rcount.data()};
      return rmh_exchange_setup(ctx, &d, thin ? 0 : 1);
   }
};

// ncclUniqueId rendezvous through a file.  Record = magic, launch tag, id.  The launch tag is what tells this launch's
// file from a stale one (a path reused by a later run, or left by a crashed one): RMH_COMM_NONCE if the launcher exports
// it (bench.py does), else the parent process id (ranks started by one shell loop / one torchrun agent share it; ranks started
// through per-rank wrappers have different parents and NEED the nonce).  Rank 0 removes a stale file first, writes <path>.tmp
// and renames it; the others poll until they read a record with their tag that is fresh: not older than five minutes with a
// nonce, not older than the reader's own start (less 30 s) without.  Rank 0 deletes the file once ncclCommInitRank -- a
// collective -- has returned.
struct IdRecord { char magic[8]; long long tag; char id[128]; };

long long launch_tag()
{
   if (const char *v = std::getenv("RMH_COMM_NONCE")) { return std::atoll(v); }
   return (long long)getppid();
}
// (without a nonce of the launcher the parent pid can repeat across launches of one shell: a reader then also refuses a
// record that is older than its own start by more than half a minute -- a file left by an earlier, crashed launch)
const std::time_t g_library_loaded = std::time(nullptr);

bool read_or_write_id(const char *path, bool writer, char id[128])
{
   IdRecord rec;
   if (writer)
   {
      std::memcpy(rec.magic, "RMHNCCL1", 8);
      rec.tag = launch_tag();
      std::memcpy(rec.id, id, 128);
      const std::string tmp = std::string(path) + ".tmp";
      FILE *f = std::fopen(tmp.c_str(), "wb");
      if (!f) { return false; }
      const bool ok = std::fwrite(&rec, sizeof(rec), 1, f) == 1;
      std::fclose(f);
      return ok && std::rename(tmp.c_str(), path) == 0;
   }
   for (int tries = 0; tries < 12000; tries++)
   {
      struct stat sb;
      FILE *f = std::fopen(path, "rb");
      if (f)
      {
         const bool ok = std::fread(&rec, sizeof(rec), 1, f) == 1 && fstat(fileno(f), &sb) == 0;
         std::fclose(f);
         const bool fresh = std::getenv("RMH_COMM_NONCE") ? std::time(nullptr) - sb.st_mtime < 300 : sb.st_mtime + 30 >= g_library_loaded;
         if (ok && std::memcmp(rec.magic, "RMHNCCL1", 8) == 0 && rec.tag == launch_tag() && fresh)
         {
            std::memcpy(id, rec.id, 128);
            return true;
         }
      }
      std::this_thread::sleep_for(std::chrono::milliseconds(10));
   }
   return false;
}

// The RCCL communicator of `nranks` processes for ctx: rank 0 removes a stale file, makes the id and writes it, every rank reads it
// and joins; rank 0 removes the file once every rank has read it (ncclCommInitRank is collective).  nullptr on success; else what
// failed: ID_FILE_FAILED, or the name of the rmh_* call whose reason rmh_last_error() has.
const char *const ID_FILE_FAILED = "cannot exchange the RCCL unique id through the file";
const char *rccl_rendezvous(rmh_ctx *ctx, const char *comm_id_file, int nranks, int rank)
{
   char id[128];
   if (rank == 0)
   {
      std::remove(comm_id_file); // (a stale record: see read_or_write_id)
      if (rmh_comm_unique_id(id) != 0) { return "rmh_comm_unique_id"; }
   }
   if (!read_or_write_id(comm_id_file, rank == 0, id)) { return ID_FILE_FAILED; }
   if (rmh_comm_init(ctx, id, nranks, rank) != 0) { return "rmh_comm_init"; }
   if (rank == 0) { std::remove(comm_id_file); }
   return nullptr;
}

// MPI_Allreduce of the reports and of the -dtc estimate (remhos.cpp:1074-1081, 1412-1421, 1993) over the ranks of a communicator:
// rmh_allreduce (op 0 sum, 1 min, 2 max).  ctx = null: one process, nothing to reduce.  A failure aborts (strict) or is remembered.
struct Reduce
{
   rmh_ctx *ctx;
   bool strict;
   bool failed = false;
   double operator()(double v, int op)
   {
      if (ctx && rmh_allreduce(ctx, &v, 1, op) != 0) { RMH_VERIFY(!strict, "rmh_allreduce(ctx, &v, 1, op)"); failed = true; }
      return v;
   }
};

// The step bookkeeping of remhos.cpp:1142-1197, 1296 for both time loops
struct StepClock
{
   double t = 0.0, dt = 0.0, t_final = 0.0;
   int max_steps = -1, repeats = 0;
   int ti = 0, ti_total = 0; // accepted steps / all steps incl. repeated ones (remhos.cpp:1142)

   double next_dt() const { return std::min(dt, t_final - t); }
   void count_step() { ti++; ti_total++; }
   // -dtc (remhos.cpp:1178-1197): false = the step of dt_real is taken back and repeated with 0.85 dt -- the caller restores its
   // state and looks at crashed() -- else dt may grow
   bool accept(double dt_ratio, double dt_real)
   {
      if (dt_ratio < 1.) { ti--; t -= dt_real; dt = 0.85 * dt; repeats++; return false; }
      if (dt_ratio > 1.25) { dt *= 1.02; }
      return true;
   }
   bool crashed() const { return !(dt >= 1e-12); } // "The time step crashed!"
   // -ms counts repeated steps too (remhos.cpp:1296)
   bool done() const { return t >= t_final - 1.e-8 * dt || ti_total == max_steps; }
};

// What both entry points report alike: masses, dt, step counts, the stopwatches T = (rhs, inv, lo, fct) with their figures of merit
// over `fom_stages` stages, wall clock, CG iterations, repeats
void fill_result_tail(rmhd_result *res, double mass0, double mass, double umax, const StepClock &clock, int stages_per_step,
                      long long global_dofs, int fom_stages, const double T[4], double wall, int cg_iters)
{
   res->final_mass = mass; res->max_value = umax; res->mass0 = mass0; res->mass_loss = std::fabs(mass0 - mass);
   res->dt = clock.dt; res->t_end = clock.t; res->steps = clock.ti;
   res->stages = stages_per_step * clock.ti_total; // the FOMs count repeated steps too (remhos.cpp:1340-1348)
   res->global_dofs = global_dofs;
   res->t_rhs = T[0]; res->t_inv = T[1]; res->t_lo = T[2]; res->t_fct = T[3];
   res->t_total = T[0] + T[2] + T[3]; // remhos.cpp:1933 (omits INV)
   const double dofs_steps = 1e-6 * (double)global_dofs * fom_stages;
   res->fom_rhs = T[0] > 0 ? dofs_steps / T[0] : 0;
   res->fom_inv = T[1] > 0 ? dofs_steps / T[1] : 0;
   res->fom_lo = T[2] > 0 ? dofs_steps / T[2] : 0;
   res->fom_fct = T[3] > 0 ? dofs_steps / T[3] : 0;
   res->fom = res->t_total > 0 ? dofs_steps / res->t_total : 0;
   res->wall = wall; res->fom_wall = dofs_steps / wall;
   res->cg_iters_max = cg_iters; res->repeats = clock.repeats;
}

// ---- one block through the solver classes: rmhd_run, rmhd_run_state, rmhd_run_rank -------------------------------------------
// A block with neighbours (ne_ghost > 0) has the other blocks of the partition, one process each, over RCCL (comm_id_file) -- or,
// self-wrapped, this rank itself.  The solver classes then run the exchanges the reference's would (SpaceLayout::
// ExchangeFaceNbrData / ExchangeElementExtrema) through the library's plan; a self-wrapped block without an id file uses a one-rank
// RCCL communicator, or device copies (RMH_EXCHANGE=local; always under the host emulation).  Returns the refusal, or ""
std::string connect_neighbours(rmh_ctx *ctx, const CaseConfig &cc, const CaseData &cd, const char *comm_id_file, bool &reduce_over_ranks)
{
   const std::string head = "neighbour exchange: ";
   const ExchangePlan plan(cd, cc);
   const char *tr = std::getenv("RMH_EXCHANGE");
   char id[128];
   bool ok = plan.setup(ctx) == 0;
   if (ok && comm_id_file)
   {
      const char *failed = rccl_rendezvous(ctx, comm_id_file, cc.px * cc.py * cc.pz, cc.rank);
      if (failed == ID_FILE_FAILED) { return head + ID_FILE_FAILED; }
      reduce_over_ranks = ok = !failed;
   }
   else if (ok && plan.only_peer_is(cc.rank) && !(tr && std::string(tr) == "local") && rmh_comm_unique_id(id) == 0) { ok = rmh_comm_init(ctx, id, 1, 0) == 0; }
   else if (ok && plan.only_peer_is(cc.rank)) { ok = rmh_comm_connect_local(ctx, 0, ctx, 0) == 0; }
   else if (ok) { return head + "a block with neighbour ranks needs the RCCL id file"; }
   return ok ? "" : head + rmh_last_error();
}

// The context of the block: rmh_create, the tables of a mesh file, the neighbour exchange, -bt, -dtc.  Returns the refusal, or ""
// (a context that a refusal leaves in `ctx` is the caller's to destroy: CtxPtr does)
std::string open_context(const rmhd_config &cfg, const CaseConfig &cc, const CaseData &cd, const char *comm_id_file, int device,
                         CtxPtr &ctx, bool &reduce_over_ranks)
{
   const rmh_layout L = make_layout(cd, device);
   rmh_ctx *c = nullptr;
   if (rmh_create(&L, &c) != 0) { return rmh_last_error(); }
   ctx.reset(c);
   if (cd.unstructured && rmh_set_quad_topology(c, cd.face_code.data(), cd.corner_ptr.data(), cd.corner_elems.data()) != 0) { return rmh_last_error(); }
   rmh_enable_timers(c, 1);
   if (cd.ne_ghost > 0)
   {
      const std::string why = connect_neighbours(c, cc, cd, comm_id_file, reduce_over_ranks);
      if (!why.empty()) { return why; }
      if (cfg.fused && !cfg.ps && (cfg.ode_solver == 0 || cfg.ode_solver == 3)) { return "a block with neighbours and the one-kernel stage runs through rmhd_run_partitioned"; }
   }
   if (rmh_set_bounds_type(c, cfg.bounds_type) != 0 || (cfg.dt_control && rmh_set_dt_control(c, 1) != 0)) { return rmh_last_error(); }
   return "";
}

struct Solvers
{
   std::unique_ptr<HOSolver> ho; std::unique_ptr<LOSolver> lo; std::unique_ptr<FCTSolver> fct; std::unique_ptr<ODESolver> ode;
   int ode_type = 3, stages_per_step = 3;
   bool fused = false; // one kernel per RK stage (rmh_stage_fused with the LO solver and the mass tolerance of the options)
};

// solver factory of remhos.cpp:912-925, 927-995, 486-500 for the options on the path
Solvers make_solvers(const rmhd_config &cfg, const CaseConfig &cc, const CaseData &cd, ParFiniteElementSpace &pfes)
{
   Solvers s;
   if (cfg.ho_type == 1) { s.ho.reset(new NeumannHOSolver(pfes)); } // remhos.cpp:914-917
   else if (cfg.ho_type == 2) { s.ho.reset(new CGHOSolver(pfes)); }
   else { s.ho.reset(new LocalInverseHOSolver(pfes, cfg.pa != 0)); }
   if (cc.lo_type == 5) { s.lo.reset(new MassBasedAvg(pfes, *s.ho, nullptr)); }
   else if (cc.lo_type == 1) { s.lo.reset(new DiscreteUpwind(pfes, cd.exec_mode == 1)); } // remhos.cpp:931-936
   else if (cc.lo_type == 2) { s.lo.reset(new DiscreteUpwind(pfes, cd.exec_mode == 1, true)); } // remhos.cpp:937-942
   else if (cc.lo_type == 3) { s.lo.reset(new PAResidualDistribution(pfes)); }
   else { s.lo.reset(new PAResidualDistributionSubcell(pfes)); }
   // remhos.cpp:983-995
   if (cfg.fct_type == 4) { s.fct.reset(new ElementFCTProjection(pfes, cd.dt)); }
   else if (cfg.fct_type == 1) { s.fct.reset(new FluxBasedFCT(pfes, nullptr, cd.dt, 1)); } // remhos.cpp:1086-1096
   else { s.fct.reset(new ClipScaleSolver(pfes, nullptr, cd.dt)); }
   // -ps / -s 11|12|13 (remhos.cpp:484-507, 875-904): block vector [u | us], IDP solvers.  They limit a COMBINATION of
   // the stage's HO rate and the earlier limited updates, so the stage cannot be the one-kernel rmh_stage_fused:
   // HO kernel + fused limiter kernel (fused = 1) or the reference's call sequence (fused = 0).
   s.ode_type = cfg.ode_solver ? cfg.ode_solver : 3;
   RMH_VERIFY(s.ode_type == 3 || s.ode_type == 11 || s.ode_type == 12 || s.ode_type == 13, "-s must be 3, 11, 12 or 13");
   s.fused = cfg.fused != 0 && !cfg.ps && s.ode_type == 3;
   if (s.fused)
   {
      RMH_CALL(rmh_set_lo_type(pfes.Ctx(), cc.lo_type));
      if (cfg.ho_type == 2) { RMH_CALL(rmh_set_mass_tol(pfes.Ctx(), 1e-12, 0.0, 500)); }
   }
   switch (s.ode_type) // remhos.cpp:486-500
   {
      case 11: s.ode.reset(new ForwardEulerIDPSolver()); break;
      case 12: s.ode.reset(new RK2IDPSolver()); break;
      case 13: s.ode.reset(new RK3IDPSolver()); break;
      default: s.ode.reset(new RK3SSPSolver()); break;
   }
   s.stages_per_step = s.ode_type == 11 ? 1 : (s.ode_type == 12 ? 2 : 3);
   return s;
}

// Setup of the monolithic solver (if any): remhos.cpp:997-1006; mass_lim: :999
std::unique_ptr<MonolithicSolver> make_mono_solver(const rmhd_config &cfg, const CaseConfig &cc, const CaseData &cd,
                                                   ParFiniteElementSpace &pfes, DofInfo &dofs)
{
   if (cfg.mono_type != 1) { return nullptr; }
   const std::vector<double> scale = mono_scale(cd, cc.problem);
   const bool mass_lim = cc.problem != 6 && cc.problem != 7;
   return std::unique_ptr<MonolithicSolver>(new MonoRDSolver(pfes, dofs, nullptr, scale.data(), false, cd.exec_mode == 1, mass_lim));
}

// -vb: global extrema of u (GetMinMax, remhos.cpp:1124) and of s = us / u on its active dofs (ComputeMinMaxS,
// remhos_sync.cpp:116-140) -- element extrema on the device, the ne values reduced on the host (a debug mode) -- and the
// monotonicity check of every step against them
struct VbMonitor
{
   ParFiniteElementSpace &pfes; DofInfo &dofs; Reduce &reduce;
   const int ne, vsize;
   const bool ps, unit_range;
   Vector vb_s;
   bool *vb_flags = nullptr;
   std::vector<double> h_emin, h_emax;
   double u_min_glob = 0., u_max_glob = 0., s_min_glob = 0., s_max_glob = 0.;

   VbMonitor(ParFiniteElementSpace &pfes_, DofInfo &dofs_, Reduce &reduce_, bool ps_, int problem)
      : pfes(pfes_), dofs(dofs_), reduce(reduce_), ne(pfes_.GetNE()), vsize(pfes_.GetVSize()), ps(ps_),
        unit_range(problem % 10 == 6 || problem % 10 == 7), vb_s(ps_ ? pfes_.GetVSize() : 0), h_emin(ne), h_emax(ne)
   {
      if (ps) { HIP_CALL(hipMalloc((void **)&vb_flags, (size_t)ne + vsize)); }
   }
   ~VbMonitor() { if (vb_flags) { (void)hipFree(vb_flags); } }
   VbMonitor(const VbMonitor &) = delete; // (and with it the assignment: the reference members)

   void global_minmax(const Vector &v, Array<bool> *el, Array<bool> *df, double &lo, double &hi)
   {
      dofs.ComputeElementsMinMax(v, dofs.xe_min, dofs.xe_max, el, df);
      dofs.xe_min.CopyToHost(h_emin.data());
      dofs.xe_max.CopyToHost(h_emax.data());
      lo = INFINITY; hi = -INFINITY;
      for (int e = 0; e < ne; e++) { lo = std::fmin(lo, h_emin[e]); hi = std::fmax(hi, h_emax[e]); }
      lo = reduce(lo, 1);
      hi = reduce(hi, 2);
   }
   // the extrema of u and, with -ps, of s for S = [u | us]
   void minmax_of(Vector &S, double &ulo, double &uhi, double &slo, double &shi)
   {
      const Vector u(S.ReadWrite(), vsize);
      global_minmax(u, nullptr, nullptr, ulo, uhi);
      if (!ps) { return; }
      const Vector us(S.ReadWrite() + vsize, vsize);
      Array<bool> el(vb_flags, ne), df(vb_flags + ne, vsize);
      ComputeRatio(pfes, us, u, vb_s, el, df);
      global_minmax(vb_s, &el, &df, slo, shi);
   }
   void start(Vector &S) { minmax_of(S, u_min_glob, u_max_glob, s_min_glob, s_max_glob); }
   // Monotonicity check for debug purposes mainly (remhos.cpp:1218-1262; forced_bounds holds for every LO solver here)
   void check(Vector &S)
   {
      const double eps = 1e-10;
      double u_min_new, u_max_new, s_min_new = s_min_glob, s_max_new = s_max_glob;
      minmax_of(S, u_min_new, u_max_new, s_min_new, s_max_new);
      const double ulo = unit_range ? 0.0 : u_min_glob, uhi = unit_range ? 1.0 : u_max_glob;
      const double slo = unit_range ? 0.0 : s_min_glob, shi = unit_range ? 1.0 : s_max_glob;
      char msg[96];
      std::snprintf(msg, sizeof(msg), "Undershoot of %.6e", ulo - u_min_new); RMH_VERIFY(u_min_new > ulo - eps, msg);
      std::snprintf(msg, sizeof(msg), "Overshoot of %.6e", u_max_new - uhi); RMH_VERIFY(u_max_new < uhi + eps, msg);
      std::snprintf(msg, sizeof(msg), "Undershoot in s of %.6e", slo - s_min_new); RMH_VERIFY(s_min_new > slo - eps, msg);
      std::snprintf(msg, sizeof(msg), "Overshoot in s of %.6e", s_max_new - shi); RMH_VERIFY(s_max_new < shi + eps, msg);
      if (!unit_range) { u_min_glob = u_min_new; u_max_glob = u_max_new; } // (s_min / s_max stay the initial ones, like the reference's)
   }
};

// One SSP-RK3 step u -> y1 -> y2 -> u of the one-kernel stage (rmh_stage_fused): the stage times and combinations of
// RK3SSPSolver::Step; input and output vectors of a stage differ (y_out may alias x_base).  tok_u names the element extrema of u
// left by the stage that wrote it (rmh_stage_fused_chain).
// With vb_du (-vb) the kernel also hands out the limited rate, no tokens are used, and the granular kernels form the dof bounds of
// the stage input for the check of remhos.cpp:1833-1837 (the LO rate never leaves the kernel: its check, :1824-1828, is the granular
// sequence's -- rmhd_config.fused = 0).
void fused_step(ParFiniteElementSpace &pfes, DofInfo &dofs, Vector &u, Vector &y1, Vector &y2, double &t, double dt_real,
                unsigned long long &tok_u, Vector *vb_du)
{
   rmh_ctx *ctx = pfes.Ctx();
   const int ne = pfes.GetNE();
   Vector *const x[4] = {&u, &y1, &y2, &u};
   unsigned long long tok = tok_u;
   for (int i = 0; i < 3; i++)
   {
      const RK3SSPStage &st = RK3SSP[i];
      const Vector &in = *x[i];
      const double *xb = (i == 0) ? nullptr : u.Read();
      RMH_CALL(rmh_setup(ctx, t + st.c * dt_real));
      if (!vb_du)
      {
         RMH_CALL(rmh_stage_fused_chain(ctx, in.Read(), dt_real, xb, st.a, st.b, dt_real, x[i + 1]->Write(), nullptr, 0, ne, 1, tok,
                                        (i == 2) ? &tok_u : &tok));
         continue;
      }
      RMH_CALL(rmh_stage_fused_chain(ctx, in.Read(), dt_real, xb, st.a, st.b, dt_real, x[i + 1]->Write(), vb_du->Write(), 0, ne, 1, 0, nullptr));
      dofs.ComputeElementsMinMax(in, dofs.xe_min, dofs.xe_max);
      dofs.ComputeBounds(dofs.xe_min, dofs.xe_max, dofs.xi_min, dofs.xi_max);
      check_violation(pfes, in, dt_real, *vb_du, dofs.xi_min, dofs.xi_max, "LimitMult FCT solution u", 1e-12, nullptr);
   }
   if (vb_du) { tok_u = 0; }
   t += dt_real;
}

// Everything of one block's run that lives on the device.  rmhd_run_rank declares it AFTER the holder of the context, so every
// Vector, DofInfo, solver and the AdvectionOperator here is destroyed BEFORE rmh_destroy; the members are declared in the order
// the run creates them.
struct BlockRun
{
   const rmhd_config &cfg; const CaseConfig &cc; const CaseData &cd;
   rmh_ctx *const ctx;
   Reduce reduce;
   const int vsize;
   const bool ps, vb, dtc;
   ParFiniteElementSpace pfes; DofInfo dofs; Solvers solvers; AdvectionOperator adv; std::unique_ptr<MonolithicSolver> mono_solver;
   Vector S, u; // Primary scalar field is u; for product remap we also evolve us (remhos.cpp:875-904): S = [u | us]
   std::vector<double> h_u, h_m, h_us;
   Vector masses;
   double mass0 = 0.0; long double mass0_us_acc = 0.0L;
   StepClock clock;
   std::chrono::steady_clock::time_point w0, w1;

   BlockRun(const rmhd_config &cfg_, const CaseConfig &cc_, const CaseData &cd_, rmh_ctx *ctx_, bool reduce_over_ranks);
   void run();
   void report(rmhd_result *res, double *u_final, double *us_final);
};

BlockRun::BlockRun(const rmhd_config &cfg_, const CaseConfig &cc_, const CaseData &cd_, rmh_ctx *ctx_, bool reduce_over_ranks)
   : cfg(cfg_), cc(cc_), cd(cd_), ctx(ctx_), reduce{reduce_over_ranks ? ctx_ : nullptr, true}, vsize(cd_.ne_owned * cd_.ndof),
     ps(cfg_.ps != 0), vb(cfg_.verify_bounds != 0), dtc(cfg_.dt_control != 0),
     pfes(ctx_, cd_.ne_owned, cd_.ndof, (long long)cd_.ne_global * cd_.ndof, cd_.ne_ghost > 0), dofs(pfes),
     solvers(make_solvers(cfg_, cc_, cd_, pfes)),
     adv(pfes, dofs, solvers.ho.get(), solvers.lo.get(), solvers.fct.get(),
         (ps || solvers.ode_type > 10) && cfg_.fused != 0 && cc_.lo_type == 5, ps),
     mono_solver(make_mono_solver(cfg_, cc_, cd_, pfes, dofs)), S((ps ? 2 : 1) * vsize), u(S.ReadWrite(), vsize), h_u(vsize),
     h_m(vsize), h_us(ps ? vsize : 0), masses(vsize)
{
   adv.mono_solver = mono_solver.get();
   adv.verify_bounds = solvers.fct->verify_bounds = vb; // remhos.cpp:1115-1116
   u.CopyFromHost(cd.u0.data());
   if (ps)
   {
      // s = s0 where the element is active (BoolFunctionCoefficient on ComputeBoolIndicators(u), remhos.cpp:890-894),
      // us = u * s node by node ("we don't target conservation at initialization", :899-900)
      for (int e = 0; e < cd.ne_owned; e++)
      {
         bool active = false;
         for (int i = 0; i < cd.ndof; i++) { active = active || cd.u0[(size_t)e * cd.ndof + i] > 1e-12; } // EMPTY_ZONE_TOL
         for (int i = 0; i < cd.ndof; i++)
         {
            const size_t k = (size_t)e * cd.ndof + i;
            h_us[k] = cd.u0[k] * (active ? cd.s0[k] : 0.0);
         }
      }
      Vector us(S.ReadWrite() + vsize, vsize);
      us.CopyFromHost(h_us.data());
   }
   // initial mass (remhos.cpp:1073-1076)
   RMH_CALL(rmh_compute_lumped_mass(ctx, 0.0, masses.Write()));
   masses.CopyToHost(h_m.data());
   // (sums of ~1e7 terms: accumulated in extended precision so that the printed mass carries no summation error of its
   // own -- the conservation claims are at the 1e-12 level)
   long double mass0_acc = 0.0L;
   for (int i = 0; i < vsize; i++) { mass0_acc += (long double)h_m[i] * cd.u0[i]; }
   mass0 = reduce((double)mass0_acc, 0);
   for (int i = 0; i < (ps ? vsize : 0); i++) { mass0_us_acc += (long double)h_m[i] * h_us[i]; } // remhos.cpp:1077-1081
   // Print the starting mesh and initial condition (remhos.cpp:1015-1030)
   if (cfg.save)
   {
      const std::string e = save_mfem(cd, 0.0, cd.u0.data(), "meshHO_init.mesh", "sltn_init.gf");
      RMH_VERIFY(e.empty(), e.c_str());
   }
   clock.dt = cd.dt; clock.max_steps = cc.max_steps;
   clock.t_final = cd.exec_mode == 1 ? 1.0 : cc.t_final; // For remap, the pseudo-time always evolves from 0 to 1 (remhos.cpp:1128-1134)
   adv.SetTime(clock.t);
   solvers.ode->Init(adv);
}

void BlockRun::run()
{
   const bool fused = solvers.fused;
   HIP_CALL(hipDeviceSynchronize());
   w0 = std::chrono::steady_clock::now();
   Vector y1(fused ? vsize : 0), y2(fused ? vsize : 0);
   unsigned long long tok_u = 0;
   Vector Sold(dtc ? vsize : 0);
   Vector vb_du(vb && fused ? vsize : 0);
   std::unique_ptr<VbMonitor> monitor;
   if (vb) { monitor.reset(new VbMonitor(pfes, dofs, reduce, ps, cc.problem)); monitor->start(S); }
   bool done = false;
   while (!done)
   {
      if (vb) { monitor->check(S); }
      double dt_real = clock.next_dt();
      // This also resets the time step estimate when automatic dt is on (remhos.cpp:1150-1152)
      adv.SetDt(dt_real);
      if (dtc) { adv.ResetTimeStepRatio(); Sold = u; }
      if (fused) { fused_step(pfes, dofs, u, y1, y2, clock.t, dt_real, tok_u, vb ? &vb_du : nullptr); }
      else { solvers.ode->Step(S, clock.t, dt_real); }
      clock.count_step();
      // remhos.cpp:1178-1197; the estimate is the minimum over the ranks of a partition (MPI_Allreduce(MIN),
      // remhos.cpp:1993): every rank takes the same accept / repeat decision, hence issues the same exchanges
      if (dtc && !clock.accept(reduce(adv.GetTimeStepRatio(), 1), dt_real))
      {
         // Repeat with the proper time step.
         u = Sold;
         tok_u = 0; // (u is no longer the output of the last stage)
         RMH_VERIFY(!clock.crashed(), "The time step crashed!");
         continue;
      }
      done = clock.done();
   }
   HIP_CALL(hipDeviceSynchronize());
   w1 = std::chrono::steady_clock::now();
}

void BlockRun::report(rmhd_result *res, double *u_final, double *us_final)
{
   const double t = clock.t;
   // final mass: remap uses the lumped mass at the final position (remhos.cpp:1382-1413)
   if (cd.exec_mode == 1) { RMH_CALL(rmh_compute_lumped_mass(ctx, t, masses.Write())); masses.CopyToHost(h_m.data()); }
   u.CopyToHost(h_u.data());
   // Print the final mesh and solution (remhos.cpp:1365-1380)
   if (cfg.save)
   {
      const std::string e = save_mfem(cd, t, h_u.data(), "meshHO_final.mesh", "sltn_final.gf");
      RMH_VERIFY(e.empty(), e.c_str());
   }
   long double mass_acc = 0.0L;
   double umax = -INFINITY;
   for (int i = 0; i < vsize; i++) { mass_acc += (long double)h_m[i] * h_u[i]; umax = std::fmax(umax, h_u[i]); }
   const double mass = reduce((double)mass_acc, 0);
   umax = reduce(umax, 2);
   if (u_final) { std::copy(h_u.begin(), h_u.end(), u_final); }
   // Compute errors, if the exact solution is known (remhos.cpp:1438-1470)
   double es[3];
   if (lp_error_sums(cd, cc.problem, t, h_u.data(), es).empty())
   {
      res->has_errors = 1;
      res->err_l1 = reduce(es[0], 0); res->err_l2 = std::sqrt(reduce(es[1], 0)); res->err_linf = reduce(es[2], 2);
   }
   if (ps)
   {
      // remhos.cpp:1404, 1416-1434: mass of us with the same lumped masses; max of the ratio s = us / u
      Vector us(S.ReadWrite() + vsize, vsize), s_fin(vsize);
      us.CopyToHost(h_us.data());
      if (us_final) { std::copy(h_us.begin(), h_us.end(), us_final); }
      long double acc = 0.0L;
      for (int i = 0; i < vsize; i++) { acc += (long double)h_m[i] * h_us[i]; }
      bool *flags = nullptr;
      HIP_CALL(hipMalloc((void **)&flags, (size_t)cd.ne_owned + vsize));
      Array<bool> el(flags, cd.ne_owned), dfl(flags + cd.ne_owned, vsize);
      ComputeRatio(pfes, us, u, s_fin, el, dfl);
      std::vector<double> h_s(vsize);
      s_fin.CopyToHost(h_s.data());
      (void)hipFree(flags);
      double smax = -INFINITY;
      for (int i = 0; i < vsize; i++) { smax = std::fmax(smax, h_s[i]); }
      res->final_mass_us = reduce((double)acc, 0);
      res->mass0_us = reduce((double)mass0_us_acc, 0);
      res->mass_loss_us = std::fabs(res->mass0_us - res->final_mass_us);
      res->s_max = reduce(smax, 2);
   }
   adv.Timer().Update(ctx); const TimingData &T = adv.Timer();
   const double sw[4] = {T.sw_rhs, T.sw_L2inv, T.sw_LO, T.sw_FCT};
   int it = 0; rmh_last_cg_iters(ctx, &it);
   const int stages = solvers.stages_per_step * clock.ti_total;
   fill_result_tail(res, mass0, mass, umax, clock, solvers.stages_per_step, pfes.GlobalVSize(), stages,
                    sw, std::chrono::duration<double>(w1 - w0).count(), it);
}
} // namespace

extern "C" int rmhd_run(const rmhd_config *cfg, rmhd_result *res) { return rmhd_run_rank(cfg, nullptr, 0, res, nullptr, nullptr); }

extern "C" int rmhd_run_state(const rmhd_config *cfg, rmhd_result *res, double *u_final, double *us_final) { return rmhd_run_rank(cfg, nullptr, 0, res, u_final, us_final); }

extern "C" int rmhd_run_rank(const rmhd_config *cfg_in, const char *comm_id_file, int device, rmhd_result *res, double *u_final,
                             double *us_final)
{
   if (!cfg_in || !res) { return refuse("null argument"); }
   std::memset(res, 0, sizeof(*res));
   if (!(comm_id_file && comm_id_file[0])) { comm_id_file = nullptr; }
   const Validated v = validate_config(*cfg_in, false, comm_id_file != nullptr);
   if (!v.refusal.empty()) { return refuse(v.refusal); }
   const rmhd_config &cfg = v.cfg;
   const CaseConfig cc = to_config(cfg);
   CaseData cd;
   std::string err = build_case(cc, cd);
   if (err.empty()) { err = check_case(cfg, cc, cd, false); }
   if (!err.empty()) { return refuse(err); }
   // Destruction runs bottom-up: `run` (every Vector, DofInfo, solver and the AdvectionOperator) goes before `ctx` (rmh_destroy),
   // also on the refusals that find the context already open.
   CtxPtr ctx;
   bool reduce_over_ranks = false;
   err = open_context(cfg, cc, cd, comm_id_file, device, ctx, reduce_over_ranks);
   if (!err.empty()) { return refuse(err); }
   BlockRun run(cfg, cc, cd, ctx.get(), reduce_over_ranks);
   run.run();
   run.report(res, u_final, us_final);
   return 0;
}

extern "C" int rmhd_axpby(double a, const double *x, double b, const double *y, double *z, long long n, void *stream)
{
   if (n < 0 || n > 0x7fffffffLL || (n > 0 && (!x || !y || !z))) { g_driver_error = "rmhd_axpby: bad argument"; return -1; }
   if (n == 0) { return 0; }
   hipLaunchKernelGGL(remhos::axpby_kernel, dim3(remhos::grid_for((int)n)), dim3(256), 0, (hipStream_t)stream, a, x, b, y, z, (int)n);
   if (hipGetLastError() != hipSuccess) { g_driver_error = "rmhd_axpby: launch failed"; return -1; }
   return 0;
}

extern "C" int rmhd_id_file_exchange(const char *path, int writer, char id[128])
{
   if (!path || !path[0] || !id) { g_driver_error = "rmhd_id_file_exchange: null argument"; return -1; }
   if (!read_or_write_id(path, writer != 0, id)) { g_driver_error = std::string("rmhd_id_file_exchange: ") + (writer ? "cannot write " : "no fresh record of this launch at ") + path; return -1; }
   return 0;
}

// ---- box-partitioned runs: the time loop of remhos() (remhos.cpp:1146-1330) over the blocks of a ParMesh-like
// partition, one fused kernel per RK stage and block, one neighbour exchange per stage (rmh_exchange_begin / _end) ----
namespace
{
// A failing rmh_* / HIP call of the functions below: the call and its reason into the error, -1 to the caller
#define RMHD_TRY(expr) do { if ((expr) != 0) { return refuse(std::string(#expr) + ": " + rmh_last_error()); } } while (0)
#define RMHD_HIP(expr) do { if ((expr) != hipSuccess) { return refuse(#expr); } } while (0)

struct Block
{
   CaseData cd;
   rmh_ctx *ctx = nullptr;
   double *x = nullptr, *y1 = nullptr, *y2 = nullptr, *xold = nullptr, *m = nullptr;
   int vsize = 0;
   unsigned long long tok = 0; // token of the extrema of the vector the next stage reads (rmh_stage_fused_chain)
   hipStream_t stream = nullptr; // the context's stream: a non-blocking one, so that the exchange stream overlaps it

   Block() {}
   Block(const Block &) = delete; Block &operator=(const Block &) = delete;
   // the buffers, then the context, then the stream the context ran on
   ~Block()
   {
      (void)hipFree(x); (void)hipFree(y1); (void)hipFree(y2); (void)hipFree(xold); (void)hipFree(m);
      if (ctx) { rmh_destroy(ctx); }
      if (stream) { (void)hipStreamDestroy(stream); }
   }
};

// Set-up of one block this process owns: case, context on a stream of its own, the options of the one-kernel stage, buffers,
// exchange plan
int setup_block(Block &b, const rmhd_config *cfg, const CaseConfig &cc, int device, bool rccl)
{
   std::string err = build_case(cc, b.cd);
   if (err.empty()) { err = check_case(*cfg, cc, b.cd, true); }
   if (!err.empty()) { return refuse(err); }
   const rmh_layout L = make_layout(b.cd, device);
   RMHD_TRY(rmh_create(&L, &b.ctx));
   // RMH_COMM_CUS = k: the stage kernels leave k compute units to the exchange stream (rmh_stream_create_reserving; only
   // where RCCL kernels run beside them -- same-process blocks exchange by device copies)
   const char *ecu = std::getenv("RMH_COMM_CUS");
   const int kcu = (rccl && ecu) ? std::atoi(ecu) : 0;
   void *sv = nullptr;
   RMHD_TRY(rmh_stream_create_reserving(device, kcu > 0 ? kcu : 0, &sv));
   b.stream = (hipStream_t)sv;
   RMHD_TRY(rmh_set_stream(b.ctx, b.stream));
   RMHD_TRY(rmh_set_lo_type(b.ctx, cc.lo_type));
   RMHD_TRY(rmh_set_bounds_type(b.ctx, cfg->bounds_type));
   if (cfg->dt_control) { RMHD_TRY(rmh_set_dt_control(b.ctx, 1)); }
   if (cfg->ho_type == 2) { RMHD_TRY(rmh_set_mass_tol(b.ctx, 1e-12, 0.0, 500)); }
   else if (cfg->pa)
   {
      // LocalInverseHOSolver on a partially assembled M (remhos_ho.cpp:77-81): DGMassInverse's rule, completed
      RMHD_TRY(rmh_set_mass_tol(b.ctx, 0.0, 1e-8, 100));
      RMHD_TRY(rmh_set_mass_completion(b.ctx, 1, 1));
   }
   b.vsize = b.cd.ne_owned * b.cd.ndof;
   const size_t bytes = sizeof(double) * (size_t)b.vsize;
   RMHD_HIP(hipMalloc((void **)&b.x, bytes));
   RMHD_HIP(hipMalloc((void **)&b.y1, bytes));
   RMHD_HIP(hipMalloc((void **)&b.y2, bytes));
   RMHD_HIP(hipMalloc((void **)&b.m, bytes));
   if (cfg->dt_control) { RMHD_HIP(hipMalloc((void **)&b.xold, bytes)); }
   RMHD_HIP(hipMemcpy(b.x, b.cd.u0.data(), bytes, hipMemcpyHostToDevice));
   if (ExchangePlan(b.cd, cc).setup(b.ctx) != 0) { return refuse(std::string("rmh_exchange_setup: ") + rmh_last_error()); }
   return 0;
}

// The transport between the blocks: RCCL between processes (one block each), device copies between the blocks of this one
int connect_blocks(std::vector<Block> &blocks, const char *comm_id_file, int nranks, int rank)
{
   if (comm_id_file)
   {
      const char *failed = rccl_rendezvous(blocks[0].ctx, comm_id_file, nranks, rank);
      if (failed == ID_FILE_FAILED) { return refuse(failed); }
      return failed ? refuse(std::string(failed) + ": " + rmh_last_error()) : 0;
   }
   for (int r = 0; r < nranks; r++)
   {
      for (size_t j = 0; j < blocks[r].cd.peers.size(); j++)
      {
         const int q = blocks[r].cd.peers[j].rank;
         if (q < r) { continue; } // (each pair once; a block may be its own neighbour's neighbour only through q != r)
         int jq = -1;
         for (size_t i = 0; i < blocks[q].cd.peers.size(); i++) { if (blocks[q].cd.peers[i].rank == r) { jq = (int)i; } }
         if (jq < 0) { return refuse("halo lists of two blocks do not mirror each other"); }
         RMHD_TRY(rmh_comm_connect_local(blocks[r].ctx, (int)j, blocks[q].ctx, jq));
      }
   }
   return 0;
}

// Mass and maximum of x over all blocks and ranks at time t; with `errors`, also the sums of the error norms where the exact
// solution is known (remhos.cpp:1438-1470; MPI-reduced like ComputeLpError): errors[3] = has any, then sum |e| w, sum e^2 w, max |e|
bool mass_and_max(std::vector<Block> &blocks, Reduce &reduce, int problem, double t, double &mass, double &umax, double *errors)
{
   mass = 0.0; umax = -INFINITY;
   for (Block &b : blocks)
   {
      if (rmh_compute_lumped_mass(b.ctx, b.cd.exec_mode == 1 ? t : 0.0, b.m) != 0) { return false; }
      if (hipStreamSynchronize(b.stream) != hipSuccess) { return false; } // (a non-blocking stream: the copies below do not wait for it)
      std::vector<double> hm(b.vsize), hu(b.vsize);
      if (hipMemcpy(hm.data(), b.m, sizeof(double) * b.vsize, hipMemcpyDeviceToHost) != hipSuccess) { return false; }
      if (hipMemcpy(hu.data(), b.x, sizeof(double) * b.vsize, hipMemcpyDeviceToHost) != hipSuccess) { return false; }
      long double acc = 0.0L; // (extended precision: see BlockRun)
      for (int i = 0; i < b.vsize; i++) { acc += (long double)hm[i] * hu[i]; umax = std::fmax(umax, hu[i]); }
      mass += (double)acc;
      double es[3];
      if (errors && lp_error_sums(b.cd, problem, t, hu.data(), es).empty())
      {
         errors[3] = 1.0; errors[0] += es[0]; errors[1] += es[1]; errors[2] = std::fmax(errors[2], es[2]);
      }
   }
   mass = reduce(mass, 0);  // MPI_Allreduce SUM, remhos.cpp:1412
   umax = reduce(umax, 2);  // MPI_Allreduce MAX, remhos.cpp:1415
   return true;
}

// One RK stage of all blocks: post every exchange, run the elements that reach no ghost while the messages are
// in flight, complete the exchanges, run the halo-dependent shells
bool stage_of_all_blocks(std::vector<Block> &blocks, int which, double t, double dt_real)
{
   const RK3SSPStage &st = RK3SSP[which];
   const double ts = t + st.c * dt_real;
   auto in = [&](Block &b) { return which == 0 ? b.x : (which == 1 ? b.y1 : b.y2); };
   auto out = [&](Block &b) { return which == 0 ? b.y1 : (which == 1 ? b.y2 : b.x); };
   for (Block &b : blocks) { if (rmh_exchange_begin(b.ctx, in(b)) != 0) { return false; } }
   for (Block &b : blocks)
   {
      if (rmh_setup(b.ctx, ts) != 0) { return false; }
      if (rmh_stage_fused_chain(b.ctx, in(b), dt_real, which == 0 ? nullptr : b.x, st.a, st.b, dt_real, out(b), nullptr,
                                b.cd.ne_halo, b.cd.ne_owned, 0, b.tok, nullptr) != 0) { return false; }
   }
   for (Block &b : blocks) { if (rmh_exchange_end(b.ctx) != 0) { return false; } }
   for (Block &b : blocks)
   {
      if (rmh_stage_fused_chain(b.ctx, in(b), dt_real, which == 0 ? nullptr : b.x, st.a, st.b, dt_real, out(b), nullptr, 0,
                                b.cd.ne_halo, 1, b.tok, &b.tok) != 0) { return false; }
   }
   return true;
}

// TimingData buckets: HIP events around the launches of every `every`-th step (default 4; RMH_DRIVER_TIMERS = k, 0 =
// never), scaled to all steps in the report.  Events around EVERY launch cost the 48^3-element blocks of an 8-rank strong run
// 8 % (measured with all eight blocks on one GPU: 14.8 k -> 16.1 k MDOFs*stage/s without them); the wall clock is exact.
struct TimerSampling
{
   int every = 4, timed_steps = 0, counted_steps = 0;
   int timed_from = 0; // steps taken before the stopwatches (re)started (rmhd_config.warmup_steps)
   std::chrono::steady_clock::time_point w0;
};

// The time loop: RK3SSPSolver::Step per step, -dtc with the estimate reduced over blocks and ranks
int partitioned_loop(std::vector<Block> &blocks, const rmhd_config *cfg, Reduce &reduce, StepClock &clock, TimerSampling &ts)
{
   bool done = false;
   while (!done)
   {
      if (cfg->warmup_steps > 0 && clock.ti_total == cfg->warmup_steps)
      {
         // the timed region starts here: everything before is finished on every rank (the reduction is the barrier)
         RMHD_HIP(hipDeviceSynchronize());
         (void)reduce(0.0, 0);
         for (Block &b : blocks) { RMHD_TRY(rmh_reset_timers(b.ctx)); }
         ts.timed_from = clock.ti_total;
         ts.timed_steps = ts.counted_steps = 0;
         ts.w0 = std::chrono::steady_clock::now();
      }
      const bool sample = ts.every > 0 && ts.counted_steps % ts.every == 0;
      for (Block &b : blocks) { RMHD_TRY(rmh_enable_timers(b.ctx, sample ? 1 : 0)); }
      ts.timed_steps += sample ? 1 : 0;
      ts.counted_steps++;
      const double dt_real = clock.next_dt();
      if (cfg->dt_control)
      {
         for (Block &b : blocks)
         {
            RMHD_TRY(rmh_dt_estimate_reset(b.ctx));
            RMHD_HIP(hipMemcpyAsync(b.xold, b.x, sizeof(double) * b.vsize, hipMemcpyDeviceToDevice, b.stream));
         }
         RMHD_HIP(hipDeviceSynchronize());
      }
      for (int which = 0; which < 3; which++)
      {
         if (!stage_of_all_blocks(blocks, which, clock.t, dt_real)) { return refuse(std::string("stage: ") + rmh_last_error()); }
      }
      clock.t += dt_real;
      clock.count_step();
      if (cfg->dt_control)
      {
         double est = INFINITY;
         for (Block &b : blocks) { double e = 0; RMHD_TRY(rmh_dt_estimate_get(b.ctx, &e)); est = std::fmin(est, e); }
         est = reduce(est, 1); // MPI_Allreduce MIN, remhos.cpp:1993
         if (!clock.accept(dt_real != 0. ? est / dt_real : 0., dt_real))
         {
            for (Block &b : blocks)
            {
               RMHD_HIP(hipMemcpyAsync(b.x, b.xold, sizeof(double) * b.vsize, hipMemcpyDeviceToDevice, b.stream));
               b.tok = 0; // (x is no longer the output of the last stage)
            }
            RMHD_HIP(hipDeviceSynchronize());
            if (clock.crashed()) { return refuse("The time step crashed!"); }
            continue;
         }
      }
      done = clock.done();
   }
   return 0;
}
} // namespace

extern "C" int rmhd_run_partitioned(const rmhd_config *cfg_in, const char *comm_id_file, int device, rmhd_result *res)
{
   if (!cfg_in || !res) { return refuse("null argument"); }
   if (!(comm_id_file && comm_id_file[0])) { comm_id_file = nullptr; }
   const bool rccl = comm_id_file != nullptr;
   const Validated v = validate_config(*cfg_in, true, rccl);
   if (!v.refusal.empty()) { return refuse(v.refusal); }
   const rmhd_config *cfg = &v.cfg;
   const CaseConfig cc0 = to_config(*cfg);
   const int nranks = cc0.px * cc0.py * cc0.pz;
   // every block this process owns; a block frees its buffers, its context and its stream when `blocks` goes, on every return
   std::vector<Block> blocks(rccl ? 1 : nranks);
   for (size_t k = 0; k < blocks.size(); k++)
   {
      CaseConfig cc = cc0;
      cc.rank = rccl ? cc0.rank : (int)k;
      if (setup_block(blocks[k], cfg, cc, device, rccl) != 0) { return -1; }
   }
   if (connect_blocks(blocks, comm_id_file, nranks, cc0.rank) != 0) { return -1; }
   Reduce reduce{rccl ? blocks[0].ctx : nullptr, false}; // over the blocks of this process, then over the ranks of the communicator
   double mass0 = 0, umax0 = 0;
   if (!mass_and_max(blocks, reduce, cc0.problem, 0.0, mass0, umax0, nullptr)) { return refuse("initial mass"); }
   StepClock clock;
   clock.dt = blocks[0].cd.dt; clock.max_steps = cc0.max_steps;
   clock.t_final = blocks[0].cd.exec_mode == 1 ? 1.0 : cc0.t_final;
   TimerSampling ts;
   const char *tenv = std::getenv("RMH_DRIVER_TIMERS");
   ts.every = tenv ? std::max(0, std::atoi(tenv)) : 4;
   for (Block &b : blocks) { RMHD_TRY(rmh_enable_timers(b.ctx, 0)); }
   RMHD_HIP(hipDeviceSynchronize());
   ts.w0 = std::chrono::steady_clock::now();
   if (partitioned_loop(blocks, cfg, reduce, clock, ts) != 0) { return -1; }
   RMHD_HIP(hipDeviceSynchronize());
   (void)reduce(0.0, 0); // (every rank has finished its last stage)
   const auto w1 = std::chrono::steady_clock::now();
   double mass = 0, umax = 0, errors[4] = {0, 0, 0, 0};
   if (!mass_and_max(blocks, reduce, cc0.problem, clock.t, mass, umax, errors)) { return refuse("final mass"); }
   if (errors[3] != 0.) { errors[0] = reduce(errors[0], 0); errors[1] = reduce(errors[1], 0); errors[2] = reduce(errors[2], 2); }
   double tk = 0.0;
   int itmax = 0;
   for (Block &b : blocks)
   {
      double tm[4];
      RMHD_TRY(rmh_timers(b.ctx, tm));
      tk = std::fmax(tk, tm[0]);
      int it = 0;
      rmh_last_cg_iters(b.ctx, &it);
      itmax = std::max(itmax, it);
   }
   if (ts.timed_steps > 0) { tk *= (double)ts.counted_steps / ts.timed_steps; } // (sampled steps -> all steps of the timed region)
   tk = reduce(tk, 2); // MPI_Reduce MAX of the stopwatches, remhos.cpp:1934
   const double wall = reduce(std::chrono::duration<double>(w1 - ts.w0).count(), 2);
   if (reduce.failed) { return refuse(std::string("rmh_allreduce: ") + rmh_last_error()); }
   std::memset(res, 0, sizeof(*res));
   res->timer_every = ts.every; res->timer_steps = ts.timed_steps;
   if (errors[3] != 0.) { res->has_errors = 1; res->err_l1 = errors[0]; res->err_l2 = std::sqrt(errors[1]); res->err_linf = errors[2]; }
   res->timed_stages = 3 * (clock.ti_total - ts.timed_from);
   res->n_peers = (int)blocks[0].cd.peers.size();
   res->transport = rccl ? 1 : (nranks > 1 ? 2 : 0);
   if (rccl) { (void)rmh_comm_count(blocks[0].ctx, &res->comm_ranks); }
   long long sd = 0, gd = 0;
   if (res->n_peers > 0) { (void)rmh_exchange_buffers(blocks[0].ctx, nullptr, &sd, nullptr, &gd); }
   res->send_bytes_per_stage = 8 * sd; res->recv_bytes_per_stage = 8 * gd;
   const double T[4] = {tk, 0., 0., 0.}; // the whole stage is one kernel: everything is in the RHS bucket
   fill_result_tail(res, mass0, mass, umax, clock, 3, blocks[0].cd.ne_global * blocks[0].cd.ndof, res->timed_stages, T, wall, itmax);
   return 0;
}

#undef RMHD_TRY
#undef RMHD_HIP

