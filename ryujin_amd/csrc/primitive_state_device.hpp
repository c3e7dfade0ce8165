// to_primitive_state() of the Descriptions on the device, from U itself (no precomputed values): shared by the
// Postprocessor sweep (kernels_postprocessor.hpp) and the Quantities sweep (kernels_quantities.hpp).

#pragma once

#include <hip/hip_runtime.h>

#include "euler_aeos_device.hpp"
#include "euler_device.hpp"
#include "scalar_conservation_device.hpp"
#include "shallow_water_device.hpp"

namespace ryujin_hip
{
  template <int DIM>
  RYUJIN_DEV void primitive_state(const EulerParams &P, const Euler<DIM> *, const double (&U)[DIM + 2],
                                  double (&V)[DIM + 2])
  {
    /* euler/hyperbolic_system.h:1277-1293: (rho, v, p) */
    const double rho_inverse = 1. / U[0];
    V[0] = U[0];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      V[1 + d] = U[1 + d] * rho_inverse;
    V[1 + DIM] = (P.gamma - 1.) * Euler<DIM>::internal_energy(U);
  }

  template <int DIM>
  RYUJIN_DEV void primitive_state(const EulerAeosParams &, const EulerAeos<DIM> *, const double (&U)[DIM + 2],
                                  double (&V)[DIM + 2])
  {
    /* euler_aeos/hyperbolic_system.h:1498-1514: (rho, v, e), e the specific internal energy */
    const double rho_inverse = 1. / U[0];
    V[0] = U[0];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      V[1 + d] = U[1 + d] * rho_inverse;
    V[1 + DIM] = EulerAeos<DIM>::internal_energy(U) * rho_inverse;
  }

  template <int DIM>
  RYUJIN_DEV void primitive_state(const ShallowWaterParams &P, const ShallowWater<DIM> *, const double (&U)[DIM + 1],
                                  double (&V)[DIM + 1])
  {
    /* shallow_water/hyperbolic_system.h:1302-1314: (h, v) with the sharp inverse water depth */
    const double h_inverse = ShallowWater<DIM>::inverse_water_depth_sharp(P, U);
    V[0] = U[0];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      V[1 + d] = U[1 + d] * h_inverse;
  }

  template <int DIM>
  RYUJIN_DEV void primitive_state(const ScalarParams &, const ScalarConservation<DIM> *, const double (&U)[1],
                                  double (&V)[1])
  {
    V[0] = U[0]; /* scalar_conservation/hyperbolic_system.h:485 */
  }
} // namespace ryujin_hip
