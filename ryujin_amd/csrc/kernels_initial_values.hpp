// HIP kernels for InitialValues on the device (gfx950): initial_state(position, t) of the configured state at
// arbitrary points, at the mesh nodes, and at the boundary_map entries at a Runge-Kutta stage time; and the bed that
// a shallow-water state brings.
//
// Reference: source/initial_values.template.h:222-262 (interpolate_hyperbolic_vector) and
// source/hyperbolic_module.template.h:137-139 (Dirichlet data of prepare_state_vector) called with the stage times
// of source/time_integrator.template.h:279-510.
//
// Two kernel shapes, each a template over the SOURCE of the state:
//   k_initial_state_points<Source>     one thread per point: positions AoS [n][DIM] -> states AoS [n][stride], the
//                                      lanes K..stride zeroed. With stride = K it serves
//                                      ryujin_hip_initial_values_evaluate, with stride = KP and the context's node
//                                      positions it writes a state vector in place
//                                      (ryujin_hip_initial_values_interpolate; ghost rows are evaluated like owned
//                                      rows, the same function of the same position on every rank: nothing to
//                                      exchange).
//   k_initial_state_dirichlet<Source>  one thread per boundary_map entry in the library's grouped order (positions
//                                      permuted once at configure time): writes the buffer k_apply_bc* reads. The
//                                      stage time t + c tau_rk is formed HERE, from the tau the first stage left on
//                                      the device, so that the host never waits for it; two rounded operations (the
//                                      library is built with -ffp-contract=off), i.e. the bits of the host's
//                                      t + c * tau.
// The sources, selected by the host (ryujin_hip_ctx::with_initial_state_source); every instantiation is a kernel of
// its own, so that a cheap state keeps its registers and takes no LDS whatever the others need:
//   IvAnalyticSource<E>                 initial_state<E>, the states of initial_states_device.hpp
//   IvLibrarySource<E>                  initial_state_library<E>: Riemann data, shock front, ramp up, Noh, ...
//                                       (initial_states_library_device.hpp)
//   IvBathymetrySource<DIM>             initial_state_sw_bathymetry<DIM>: the shallow-water states that bring their
//                                       own bathymetry (initial_states_bathymetry_device.hpp)
//   IvFunctionSource<E>                 initial_state_function<E>: the expression-defined "function" state
//                                       (expression.hpp)
//   IvEosFunctionSource<DIM>,
//   IvLibraryEosFunctionSource<DIM>     the analytic and the library states of EulerAEOS on a context with the
//                                       "function" equation of state: the sie program through the interpreter
// The last three are INTERPRETED: the programs are read by scalar loads, the operand stack is a [slot][lane] column
// of LDS, and no thread leaves before the interpreter has run, so that its loop and its branches stay wave-uniform.
//   k_initial_precomputed<DIM>          the bed, initial_precomputations(affine_transform(point)), one thread per
//                                       point: into a caller's buffer (evaluate_initial_precomputed) or, at the node
//                                       positions, into the context's bathymetry, ghost rows included
//                                       (interpolate_initial_precomputed). It serves EVERY shallow-water state, the
//                                       function state included: a state without a bed writes exact zeros.
// All are latency-bound launches of a few thousand threads at most on the boundary (2 in 1-D); 64 threads per block
// spread the boundary of a 2-D mesh over as many compute units as it has waves (profiles/initial_values_timing.md).

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "initial_states_bathymetry_device.hpp"
#include "initial_states_device.hpp"
#include "initial_states_library_device.hpp"
#include "kernels_euler.hpp"

namespace ryujin_hip
{
  constexpr int kInitialValuesBlock = 64;

  /* the kernel argument of a source that interprets no program: empty, where the others take their pointer */
  struct IvNoProgram {
  };

  /* A source names its Description, the kernel argument that is its program, the doubles of LDS a block needs for it
   * (0: none, the source is not interpreted), and state(): the existing evaluator behind one signature. `program`,
   * `active` and `column` (&lds[lane]) reach the interpreted evaluators only. */
  template <typename E>
  struct IvAnalyticSource {
    using Description = E;
    using Program = IvNoProgram;
    static constexpr int lds_doubles = 0;
    RYUJIN_DEV static void state(const InitialValuesParams &P, Program, const double (&x)[E::DIMENSION],
                                 const double t, bool, double *, double (&U)[E::K])
    {
      initial_state<E>(P, x, t, U);
    }
  };

  template <typename E>
  struct IvLibrarySource {
    using Description = E;
    using Program = IvNoProgram;
    static constexpr int lds_doubles = 0;
    RYUJIN_DEV static void state(const InitialValuesParams &P, Program, const double (&x)[E::DIMENSION],
                                 const double t, bool, double *, double (&U)[E::K])
    {
      initial_state_library<E>(P, x, t, U);
    }
  };

  template <int DIM>
  struct IvBathymetrySource {
    using Description = ShallowWater<DIM>;
    using Program = IvNoProgram;
    static constexpr int lds_doubles = 0;
    RYUJIN_DEV static void state(const InitialValuesParams &P, Program, const double (&x)[DIM], const double t,
                                 bool, double *, double (&U)[DIM + 1])
    {
      initial_state_sw_bathymetry<DIM>(P, x, t, U);
    }
  };

  template <typename E>
  struct IvFunctionSource {
    using Description = E;
    using Program = const IvFunctionProgram *__restrict__;
    static constexpr int lds_doubles = iv_function_lds_doubles(kInitialValuesBlock);
    RYUJIN_DEV static void state(const InitialValuesParams &P, Program program,
                                 const double (&x)[E::DIMENSION], const double t, bool, double *column,
                                 double (&U)[E::K])
    {
      initial_state_function<E, kInitialValuesBlock>(P, program, x, t, column, U);
    }
  };

  template <int DIM>
  struct IvEosFunctionSource {
    using Description = EulerAeos<DIM>;
    using Program = const EosProgram *__restrict__;
    static constexpr int lds_doubles = eos_function_lds_doubles(kInitialValuesBlock);
    RYUJIN_DEV static void state(const InitialValuesParams &P, Program program,
                                 const double (&x)[DIM], const double t, const bool active, double *column,
                                 double (&U)[DIM + 2])
    {
      initial_state_eos_function<DIM, kInitialValuesBlock>(P, program, x, t, active, column, U);
    }
  };

  template <int DIM>
  struct IvLibraryEosFunctionSource {
    using Description = EulerAeos<DIM>;
    using Program = const EosProgram *__restrict__;
    static constexpr int lds_doubles = eos_function_lds_doubles(kInitialValuesBlock);
    RYUJIN_DEV static void state(const InitialValuesParams &P, Program program,
                                 const double (&x)[DIM], const double t, const bool active, double *column,
                                 double (&U)[DIM + 2])
    {
      initial_state_library_eos_function<DIM, kInitialValuesBlock>(P, program, x, t, active, column, U);
    }
  };

  /* An interpreted source keeps every lane of the wave until its interpreter has run (the loop is wave-uniform); a
   * source without LDS lets a lane without a point leave at once. */
  template <typename Source>
  constexpr bool iv_keeps_idle_lanes = Source::lds_doubles > 0;

  /* The state of one lane, U, at `position`. Idle lanes arrive from an interpreted source only: they evaluate x = 0
   * and the caller stores nothing. */
  template <typename Source>
  RYUJIN_DEV void iv_source_state(const InitialValuesParams &P, const typename Source::Program program,
                                  const bool active, const double *__restrict__ position, const double t,
                                  double (&U)[Source::Description::K])
  {
    constexpr int DIM = Source::Description::DIMENSION;
    double x[DIM];
    if constexpr (iv_keeps_idle_lanes<Source>) {
      __shared__ double lds[Source::lds_doubles];
#pragma unroll
      for (int d = 0; d < DIM; ++d)
        x[d] = active ? position[d] : 0.;
      Source::state(P, program, x, t, active, lds + threadIdx.x, U);
    } else {
#pragma unroll
      for (int d = 0; d < DIM; ++d)
        x[d] = position[d];
      Source::state(P, program, x, t, true, nullptr, U);
    }
  }

  /* entries whose boundary id does not read Dirichlet data are skipped (their slot is never read) */
  RYUJIN_DEV bool iv_reads_dirichlet(const int id)
  {
    return id == RYUJIN_BC_DIRICHLET || id == RYUJIN_BC_DYNAMIC || id == RYUJIN_BC_DIRICHLET_MOMENTUM;
  }

  /* the stage time of the Dirichlet kernel: two rounded operations, the bits of the host's t + c * tau */
  RYUJIN_DEV double iv_stage_time(const double t, const double c, const DeviceScalars *__restrict__ scalars)
  {
    double time = t;
    if (c != 0.) {
      /* an invalid tau_max ends the step in RYUJIN_ERR_TAU whatever this stage sees: evaluate at t */
      double tau = scalars->tau_rk;
      if (!(tau > 0.) || isinf(tau))
        tau = 0.;
      const double increment = c * tau;
      time = t + increment;
    }
    return time;
  }

  template <typename Source>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_state_points(
      const InitialValuesParams P, const typename Source::Program program, const uint32_t n,
      const double *__restrict__ positions, const double t, const int stride, double *__restrict__ out)
  {
    constexpr int DIM = Source::Description::DIMENSION, K = Source::Description::K;
    const uint32_t i = blockIdx.x * (uint32_t)kInitialValuesBlock + threadIdx.x;
    const bool active = i < n;
    if constexpr (!iv_keeps_idle_lanes<Source>)
      if (!active)
        return;
    double U[K];
    iv_source_state<Source>(P, program, active, positions + (size_t)i * DIM, t, U);
    if (!active)
      return;
#pragma unroll
    for (int q = 0; q < K; ++q)
      out[(size_t)i * stride + q] = U[q];
    for (int q = K; q < stride; ++q) /* the pad lane of an odd state, as state_upload leaves it */
      out[(size_t)i * stride + q] = 0.;
  }

  template <typename Source>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_state_dirichlet(
      const InitialValuesParams P, const typename Source::Program program, const uint32_t n_bdry,
      const double *__restrict__ b_positions, const uint8_t *__restrict__ b_id, const double t, const double c,
      const DeviceScalars *__restrict__ scalars, double *__restrict__ dirichlet)
  {
    constexpr int DIM = Source::Description::DIMENSION, K = Source::Description::K;
    const uint32_t e = blockIdx.x * (uint32_t)kInitialValuesBlock + threadIdx.x;
    const bool active = e < n_bdry && iv_reads_dirichlet(b_id[e]);
    if constexpr (!iv_keeps_idle_lanes<Source>)
      if (!active)
        return;
    const double time = iv_stage_time(t, c, scalars);
    double U[K];
    iv_source_state<Source>(P, program, active, b_positions + (size_t)e * DIM, time, U);
    if (!active)
      return;
#pragma unroll
    for (int q = 0; q < K; ++q)
      dirichlet[(size_t)e * K + q] = U[q];
  }

  template <int DIM>
  __global__ __launch_bounds__(kInitialValuesBlock) void k_initial_precomputed(
      const InitialValuesParams P, const uint32_t n, const double *__restrict__ points, double *__restrict__ out)
  {
    const uint32_t i = blockIdx.x * (uint32_t)kInitialValuesBlock + threadIdx.x;
    if (i >= n)
      return;
    double x[DIM];
    iv_transform_point<DIM>(P, points + (size_t)i * DIM, x);
    out[i] = initial_precomputations_sw<DIM>(P, x);
  }
} // namespace ryujin_hip
