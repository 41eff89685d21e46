// DofInfo::ComputeBounds on unstructured quadrilateral meshes (rmh_layout.dim = 2 with rmh_set_quad_topology): the dof bounds
// from given element extrema where the neighbours of an element are not a 3 x 3 lattice stencil -- a vertex may belong to 3, 5
// or 6 elements, and a neighbour's reference axes may be turned against the element's.
//   bounds_type 0: ComputeOverlapBounds (remhos_tools.cpp:432-495) reduces the element extrema over the CG nodes of the H1
//     bounds space and hands every dof the value of its node.  Without that space: an interior dof belongs to its element only,
//     a dof on an edge also to the face neighbour across the edge, a corner dof to every element that contains the vertex (the
//     CSR row of the corner: the OTHER elements at the vertex).
//   bounds_type 1: ComputeMatrixSparsityBounds (remhos_tools.cpp:381-430): the element and its four face neighbours, for
//     every dof.
// Only min and max are taken: the result is the same bits whatever the order, and the (+inf, -inf) of the inactive elements of
// the masked variant (rmh_elem_minmax_masked) are the identities of both, so they pass through.
//
// Shape (as rmh_product2d.hpp): a wavefront per element, one dof per lane, four elements per 256-thread workgroup; no LDS, no
// barrier, no atomics, no cross-lane operation -- lanes past the element's last dof simply leave.
#pragma once
#include "rmh_product2d.hpp"

namespace rmh
{

template <int P>
__global__ void __launch_bounds__(P2Cfg<P>::NT) bounds_quad_kernel(int bounds_type, const int *face_nbr, const int *corner_ptr,
                                                                   const int *corner_elems, const double *xe_min,
                                                                   const double *xe_max, double *u_min, double *u_max, int ne)
{
   using C = P2Cfg<P>;
   constexpr int D = P + 1;
   const int lane = threadIdx.x & 63;
   const int e = blockIdx.x * C::NW + (threadIdx.x >> 6);
   if (e >= ne || lane >= C::D2) { return; }
   const int ix = lane % D, iy = lane / D;
   double lo = xe_min[e], hi = xe_max[e];
#pragma unroll
   for (int f = 0; f < 4; f++)
   {
      // face f = 2 c + side holds the dofs of layer side * P in direction c
      const int ic = f < 2 ? ix : iy;
      if (bounds_type == 1 || ic == (f & 1) * P)
      {
         const int nb = face_nbr[(size_t)e * 4 + f];
         if (nb >= 0)
         {
            lo = fmin(lo, xe_min[nb]);
            hi = fmax(hi, xe_max[nb]);
         }
      }
   }
   const bool cx = ix == 0 || ix == P, cy = iy == 0 || iy == P;
   if (bounds_type == 0 && cx && cy)
   {
      const size_t k = (size_t)e * 4 + (ix == P ? 1 : 0) + (iy == P ? 2 : 0); // corner k = kx + 2 ky
      for (int j = corner_ptr[k]; j < corner_ptr[k + 1]; j++)
      {
         const int g = corner_elems[j];
         lo = fmin(lo, xe_min[g]);
         hi = fmax(hi, xe_max[g]);
      }
   }
   u_min[(size_t)e * C::D2 + lane] = lo;
   u_max[(size_t)e * C::D2 + lane] = hi;
}

} // namespace rmh
