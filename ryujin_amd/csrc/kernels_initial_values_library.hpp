// HIP kernels for the Riemann-data, shock-front, ramp-up and Noh states (initial_states_library_device.hpp): the three
// consumers of kernels_initial_values.hpp once more, for initial_state_library<E>().
//   k_initial_values_library_points                 one thread per point (evaluate, interpolate)
//   k_initial_values_library_dirichlet              one thread per boundary_map entry, at the stage time t + c tau_rk
//                                                   formed from the tau on the device
//   k_initial_values_library_eos_function_points,
//   k_initial_values_library_eos_function_dirichlet the same two on an EulerAEOS context with the "function" equation
//                                                   of state: the sie program through the interpreter, a [slot][lane]
//                                                   column of LDS for its operand stack, no thread leaves before the
//                                                   interpreter has run
// Kernels of their own, selected by the host by state id, so that the kernels of the ten states before them keep their
// registers. Launch shape, argument lists and the stage-time arithmetic are those of kernels_initial_values.hpp.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "initial_states_library_device.hpp"
#include "kernels_initial_values.hpp"

namespace ryujin_hip
{
  /* the stage time of the Dirichlet kernels: two rounded operations, the bits of the host's t + c * tau; an invalid
   * tau_max ends the step in RYUJIN_ERR_TAU whatever this stage sees: evaluate at t */
  RYUJIN_DEV double iv_library_stage_time(const double t, const double c, const DeviceScalars *__restrict__ scalars)
  {
    double time = t;
    if (c != 0.) {
      double tau = scalars->tau_rk;
      if (!(tau > 0.) || isinf(tau))
        tau = 0.;
      const double increment = c * tau;
      time = t + increment;
    }
    return time;
  }

  RYUJIN_DEV bool iv_library_reads_dirichlet(const int id)
  {
    return id == RYUJIN_BC_DIRICHLET || id == RYUJIN_BC_DYNAMIC || id == RYUJIN_BC_DIRICHLET_MOMENTUM;
  }

  template <typename E>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_values_library_points(
      const InitialValuesParams P, const uint32_t n, const double *__restrict__ positions, const double t,
      const int stride, double *__restrict__ out)
  {
    constexpr int DIM = E::DIMENSION, K = E::K;
    const uint32_t i = blockIdx.x * (uint32_t)kInitialValuesBlock + threadIdx.x;
    if (i >= n)
      return;
    double x[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      x[d] = positions[(size_t)i * DIM + d];
    double U[K];
    initial_state_library<E>(P, x, t, U);
#pragma unroll
    for (int q = 0; q < K; ++q)
      out[(size_t)i * stride + q] = U[q];
    for (int q = K; q < stride; ++q) /* the pad lane of an odd state, as state_upload leaves it */
      out[(size_t)i * stride + q] = 0.;
  }

  /* b_id: entries whose boundary id does not read Dirichlet data are skipped (their slot is never read) */
  template <typename E>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_values_library_dirichlet(
      const InitialValuesParams P, const uint32_t n_bdry, const double *__restrict__ b_positions,
      const uint8_t *__restrict__ b_id, const double t, const double c,
      const DeviceScalars *__restrict__ scalars, double *__restrict__ dirichlet)
  {
    constexpr int DIM = E::DIMENSION, K = E::K;
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
    initial_state_library<E>(P, x, time, U);
#pragma unroll
    for (int q = 0; q < K; ++q)
      dirichlet[(size_t)e * K + q] = U[q];
  }

  template <int DIM>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_values_library_eos_function_points(
      const InitialValuesParams P, const EosProgram *__restrict__ program, const uint32_t n,
      const double *__restrict__ positions, const double t, const int stride, double *__restrict__ out)
  {
    constexpr int K = DIM + 2;
    __shared__ double lds[eos_function_lds_doubles(kInitialValuesBlock)];
    const uint32_t i = blockIdx.x * (uint32_t)kInitialValuesBlock + threadIdx.x;
    const bool active = i < n;
    double x[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      x[d] = active ? positions[(size_t)i * DIM + d] : 0.;
    double U[K];
    initial_state_library_eos_function<DIM, kInitialValuesBlock>(P, program, x, t, active, lds + threadIdx.x, U);
    if (!active)
      return;
#pragma unroll
    for (int q = 0; q < K; ++q)
      out[(size_t)i * stride + q] = U[q];
    for (int q = K; q < stride; ++q) /* the pad lane of an odd state, as state_upload leaves it */
      out[(size_t)i * stride + q] = 0.;
  }

  template <int DIM>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_values_library_eos_function_dirichlet(
      const InitialValuesParams P, const EosProgram *__restrict__ program, const uint32_t n_bdry,
      const double *__restrict__ b_positions, const uint8_t *__restrict__ b_id, const double t, const double c,
      const DeviceScalars *__restrict__ scalars, double *__restrict__ dirichlet)
  {
    constexpr int K = DIM + 2;
    __shared__ double lds[eos_function_lds_doubles(kInitialValuesBlock)];
    const uint32_t e = blockIdx.x * (uint32_t)kInitialValuesBlock + threadIdx.x;
    bool active = e < n_bdry;
    if (active)
      active = iv_library_reads_dirichlet(b_id[e]);
    const double time = iv_library_stage_time(t, c, scalars);
    double x[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      x[d] = active ? b_positions[(size_t)e * DIM + d] : 0.;
    double U[K];
    initial_state_library_eos_function<DIM, kInitialValuesBlock>(P, program, x, time, active, lds + threadIdx.x, U);
    if (!active)
      return;
#pragma unroll
    for (int q = 0; q < K; ++q)
      dirichlet[(size_t)e * K + q] = U[q];
  }
} // namespace ryujin_hip
