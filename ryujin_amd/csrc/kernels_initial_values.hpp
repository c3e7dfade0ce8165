// HIP kernels for InitialValues on the device (gfx950): initial_state(position, t) of an analytic state at
// arbitrary points, at the mesh nodes, and at the boundary_map entries at a Runge-Kutta stage time.
//
// Reference: source/initial_values.template.h:222-262 (interpolate_hyperbolic_vector) and
// source/hyperbolic_module.template.h:137-139 (Dirichlet data of prepare_state_vector) called with the stage times
// of source/time_integrator.template.h:279-510.
//   k_initial_values_points     one thread per point: positions AoS [n][DIM] -> states AoS [n][stride]. With
//                               stride = K it serves ryujin_hip_initial_values_evaluate, with stride = KP and the
//                               context's node positions it writes a state vector in place
//                               (ryujin_hip_initial_values_interpolate; ghost rows are evaluated like owned rows, the
//                               same function of the same position on every rank: nothing to exchange).
//   k_initial_values_dirichlet  one thread per boundary_map entry in the library's grouped order (positions permuted
//                               once at configure time): writes the buffer k_apply_bc* reads. The stage time
//                               t + c tau_rk is formed HERE, from the tau the first stage left on the device, so
//                               that the host never waits for it; two rounded operations (the library is built with
//                               -ffp-contract=off), i.e. the bits of the host's t + c * tau.
//   k_initial_values_function_points, k_initial_values_function_dirichlet
//                               the same two for the expression-defined "function" state
//                               (initial_state_function, expression.hpp): kernels of their own, so that the two above
//                               keep their registers and take no LDS. The programs are read by scalar loads, the
//                               operand stack is a [slot][lane] column of LDS; no thread leaves before the
//                               interpreter has run, so that its loop and its branches stay wave-uniform.
// Both are latency-bound launches of a few thousand threads at most on the boundary (2 in 1-D); 64 threads per block
// spread the boundary of a 2-D mesh over as many compute units as it has waves (profiles/initial_values_timing.md).

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "initial_states_device.hpp"
#include "kernels_euler.hpp"

namespace ryujin_hip
{
  constexpr int kInitialValuesBlock = 64;

  template <typename E>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_values_points(
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
    initial_state<E>(P, x, t, U);
#pragma unroll
    for (int q = 0; q < K; ++q)
      out[(size_t)i * stride + q] = U[q];
    for (int q = K; q < stride; ++q) /* the pad lane of an odd state, as state_upload leaves it */
      out[(size_t)i * stride + q] = 0.;
  }

  /* b_id: entries whose boundary id does not read Dirichlet data are skipped (their slot is never read) */
  template <typename E>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_values_dirichlet(
      const InitialValuesParams P, const uint32_t n_bdry, const double *__restrict__ b_positions,
      const uint8_t *__restrict__ b_id, const double t, const double c,
      const DeviceScalars *__restrict__ scalars, double *__restrict__ dirichlet)
  {
    constexpr int DIM = E::DIMENSION, K = E::K;
    const uint32_t e = blockIdx.x * (uint32_t)kInitialValuesBlock + threadIdx.x;
    if (e >= n_bdry)
      return;
    const int id = b_id[e];
    if (id != RYUJIN_BC_DIRICHLET && id != RYUJIN_BC_DYNAMIC && id != RYUJIN_BC_DIRICHLET_MOMENTUM)
      return;
    double time = t;
    if (c != 0.) {
      /* an invalid tau_max ends the step in RYUJIN_ERR_TAU whatever this stage sees: evaluate at t */
      double tau = scalars->tau_rk;
      if (!(tau > 0.) || isinf(tau))
        tau = 0.;
      const double increment = c * tau;
      time = t + increment;
    }
    double x[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      x[d] = b_positions[(size_t)e * DIM + d];
    double U[K];
    initial_state<E>(P, x, time, U);
#pragma unroll
    for (int q = 0; q < K; ++q)
      dirichlet[(size_t)e * K + q] = U[q];
  }

  template <typename E>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_values_function_points(
      const InitialValuesParams P, const IvFunctionProgram *__restrict__ program, const uint32_t n,
      const double *__restrict__ positions, const double t, const int stride, double *__restrict__ out)
  {
    constexpr int DIM = E::DIMENSION, K = E::K;
    __shared__ double lds[iv_function_lds_doubles(kInitialValuesBlock)];
    const uint32_t i = blockIdx.x * (uint32_t)kInitialValuesBlock + threadIdx.x;
    const bool active = i < n;
    double x[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      x[d] = active ? positions[(size_t)i * DIM + d] : 0.;
    double U[K];
    initial_state_function<E, kInitialValuesBlock>(P, program, x, t, lds + threadIdx.x, U);
    if (!active)
      return;
#pragma unroll
    for (int q = 0; q < K; ++q)
      out[(size_t)i * stride + q] = U[q];
    for (int q = K; q < stride; ++q) /* the pad lane of an odd state, as state_upload leaves it */
      out[(size_t)i * stride + q] = 0.;
  }

  template <typename E>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_values_function_dirichlet(
      const InitialValuesParams P, const IvFunctionProgram *__restrict__ program, const uint32_t n_bdry,
      const double *__restrict__ b_positions, const uint8_t *__restrict__ b_id, const double t, const double c,
      const DeviceScalars *__restrict__ scalars, double *__restrict__ dirichlet)
  {
    constexpr int DIM = E::DIMENSION, K = E::K;
    __shared__ double lds[iv_function_lds_doubles(kInitialValuesBlock)];
    const uint32_t e = blockIdx.x * (uint32_t)kInitialValuesBlock + threadIdx.x;
    bool active = e < n_bdry;
    if (active) {
      const int id = b_id[e];
      active = id == RYUJIN_BC_DIRICHLET || id == RYUJIN_BC_DYNAMIC || id == RYUJIN_BC_DIRICHLET_MOMENTUM;
    }
    double time = t;
    if (c != 0.) {
      /* as k_initial_values_dirichlet */
      double tau = scalars->tau_rk;
      if (!(tau > 0.) || isinf(tau))
        tau = 0.;
      const double increment = c * tau;
      time = t + increment;
    }
    double x[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      x[d] = active ? b_positions[(size_t)e * DIM + d] : 0.;
    double U[K];
    initial_state_function<E, kInitialValuesBlock>(P, program, x, time, lds + threadIdx.x, U);
    if (!active)
      return;
#pragma unroll
    for (int q = 0; q < K; ++q)
      dirichlet[(size_t)e * K + q] = U[q];
  }

  /* k_initial_values_points and k_initial_values_dirichlet for the analytic EulerAEOS states on a context with the
   * "function" equation of state (initial_state_eos_function): the sie program through the interpreter, kernels of
   * their own for the reasons above */
  template <int DIM>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_values_eos_function_points(
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
    initial_state_eos_function<DIM, kInitialValuesBlock>(P, program, x, t, active, lds + threadIdx.x, U);
    if (!active)
      return;
#pragma unroll
    for (int q = 0; q < K; ++q)
      out[(size_t)i * stride + q] = U[q];
    for (int q = K; q < stride; ++q) /* the pad lane of an odd state, as state_upload leaves it */
      out[(size_t)i * stride + q] = 0.;
  }

  template <int DIM>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_values_eos_function_dirichlet(
      const InitialValuesParams P, const EosProgram *__restrict__ program, const uint32_t n_bdry,
      const double *__restrict__ b_positions, const uint8_t *__restrict__ b_id, const double t, const double c,
      const DeviceScalars *__restrict__ scalars, double *__restrict__ dirichlet)
  {
    constexpr int K = DIM + 2;
    __shared__ double lds[eos_function_lds_doubles(kInitialValuesBlock)];
    const uint32_t e = blockIdx.x * (uint32_t)kInitialValuesBlock + threadIdx.x;
    bool active = e < n_bdry;
    if (active) {
      const int id = b_id[e];
      active = id == RYUJIN_BC_DIRICHLET || id == RYUJIN_BC_DYNAMIC || id == RYUJIN_BC_DIRICHLET_MOMENTUM;
    }
    double time = t;
    if (c != 0.) {
      /* as k_initial_values_dirichlet */
      double tau = scalars->tau_rk;
      if (!(tau > 0.) || isinf(tau))
        tau = 0.;
      const double increment = c * tau;
      time = t + increment;
    }
    double x[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      x[d] = active ? b_positions[(size_t)e * DIM + d] : 0.;
    double U[K];
    initial_state_eos_function<DIM, kInitialValuesBlock>(P, program, x, time, active, lds + threadIdx.x, U);
    if (!active)
      return;
#pragma unroll
    for (int q = 0; q < K; ++q)
      dirichlet[(size_t)e * K + q] = U[q];
  }
} // namespace ryujin_hip
