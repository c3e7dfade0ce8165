// HIP kernels for the shallow-water states that bring their own bathymetry (initial_states_bathymetry_device.hpp):
//   k_initial_values_bathymetry_points      one thread per point, out[n * K] (evaluate)
//   k_initial_values_bathymetry_nodes       one thread per node of the state vector, the pad lane of an odd state
//                                           zeroed as state_upload leaves it (interpolate)
//   k_initial_values_bathymetry_dirichlet   one thread per boundary_map entry, at the stage time t + c tau_rk formed
//                                           from the tau on the device
//   k_initial_precomputed_points            the bed, initial_precomputations(affine_transform(point)), one thread per
//                                           point (evaluate_initial_precomputed)
//   k_initial_precomputed_nodes             the same into the context's bathymetry, one thread per node, ghost rows
//                                           included (interpolate_initial_precomputed)
// The two bed kernels serve EVERY shallow-water state, the function state included: a state without a bed writes
// exact zeros. Kernels of their own, selected by the host by state id, so that the kernels of the states before them
// keep their registers. Launch shape and the stage-time arithmetic are those of kernels_initial_values_library.hpp.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "initial_states_bathymetry_device.hpp"
#include "kernels_initial_values_library.hpp"

namespace ryujin_hip
{
  template <int DIM>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_values_bathymetry_points(
      const InitialValuesParams P, const uint32_t n, const double *__restrict__ points, const double t,
      double *__restrict__ out)
  {
    constexpr int K = DIM + 1;
    const uint32_t i = blockIdx.x * (uint32_t)kInitialValuesBlock + threadIdx.x;
    if (i >= n)
      return;
    double x[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      x[d] = points[(size_t)i * DIM + d];
    double U[K];
    initial_state_sw_bathymetry<DIM>(P, x, t, U);
#pragma unroll
    for (int q = 0; q < K; ++q)
      out[(size_t)i * K + q] = U[q];
  }

  template <int DIM>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_values_bathymetry_nodes(
      const InitialValuesParams P, const uint32_t n_relevant, const double *__restrict__ positions, const double t,
      const int stride, double *__restrict__ state)
  {
    constexpr int K = DIM + 1;
    const uint32_t i = blockIdx.x * (uint32_t)kInitialValuesBlock + threadIdx.x;
    if (i >= n_relevant)
      return;
    double x[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      x[d] = positions[(size_t)i * DIM + d];
    double U[K];
    initial_state_sw_bathymetry<DIM>(P, x, t, U);
#pragma unroll
    for (int q = 0; q < K; ++q)
      state[(size_t)i * stride + q] = U[q];
    for (int q = K; q < stride; ++q)
      state[(size_t)i * stride + q] = 0.;
  }

  /* b_id: entries whose boundary id does not read Dirichlet data are skipped (their slot is never read) */
  template <int DIM>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_values_bathymetry_dirichlet(
      const InitialValuesParams P, const uint32_t n_bdry, const double *__restrict__ b_positions,
      const uint8_t *__restrict__ b_id, const double t, const double c,
      const DeviceScalars *__restrict__ scalars, double *__restrict__ dirichlet)
  {
    constexpr int K = DIM + 1;
    const uint32_t e = blockIdx.x * (uint32_t)kInitialValuesBlock + threadIdx.x;
    if (e >= n_bdry)
      return;
    if (!iv_library_reads_dirichlet(b_id[e]))
      return;
    const double time = iv_library_stage_time(t, c, scalars);
    double x[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      x[d] = b_positions[(size_t)e * DIM + d];
    double U[K];
    initial_state_sw_bathymetry<DIM>(P, x, time, U);
#pragma unroll
    for (int q = 0; q < K; ++q)
      dirichlet[(size_t)e * K + q] = U[q];
  }

  template <int DIM>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_precomputed_points(
      const InitialValuesParams P, const uint32_t n, const double *__restrict__ points, double *__restrict__ out)
  {
    const uint32_t i = blockIdx.x * (uint32_t)kInitialValuesBlock + threadIdx.x;
    if (i >= n)
      return;
    double x[DIM];
    iv_transform_point<DIM>(P, points + (size_t)i * DIM, x);
    out[i] = initial_precomputations_sw<DIM>(P, x);
  }

  template <int DIM>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_precomputed_nodes(
      const InitialValuesParams P, const uint32_t n_relevant, const double *__restrict__ positions,
      double *__restrict__ bathymetry)
  {
    const uint32_t i = blockIdx.x * (uint32_t)kInitialValuesBlock + threadIdx.x;
    if (i >= n_relevant)
      return;
    double x[DIM];
    iv_transform_point<DIM>(P, positions + (size_t)i * DIM, x);
    bathymetry[i] = initial_precomputations_sw<DIM>(P, x);
  }
} // namespace ryujin_hip
