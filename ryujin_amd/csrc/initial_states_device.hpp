// Analytic initial / Dirichlet states on the device: InitialValues::initial_state(position, t).
//
// Reference: source/initial_values.template.h:66-148 (affine transform: translate by `position`, roll `direction`
// onto the x-axis -- z first, then y --, rotate the momentum back) composed with the InitialState classes
//   source/euler/initial_state_{uniform,radial_contrast,isentropic_vortex,leblanc,rarefaction}.h
//   source/shallow_water/initial_state_{circular_dam_break,paraboloid,ritter_dam_break,smooth_vortex,sloping_friction}.h
// in the operation order of their Python restatement ryujin_amd/initial_states.py (the specification: same
// statements, same `<=` against `<` at the jumps), so that the two differ by the library functions alone.
//
// ONE function, initial_state<E>(), serves every consumer (evaluate, interpolate, the Dirichlet kernel): the same
// (x, t) gives the same bits wherever it is evaluated. The library is built with -ffp-contract=off.
//
// The expression-defined state "function" (source/*/initial_state_function.h) has a device function of its own,
// initial_state_function<E>(), which again serves every consumer: it needs the programs and a column of LDS for the
// operand stack, which the ten analytic states above it do without.
//
// Whatever does not depend on (x, t) -- the normalised direction and its rotation cosines, the Riemann-fan
// constants of the rarefaction, sqrt(g h_L) of the Ritter solution, the uniform depth of the incline -- is formed
// once on the host by ryujin_hip_initial_values_configure (InitialValuesParams::c).

#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "euler_aeos_device.hpp"
#include "euler_device.hpp"
#include "expression.hpp"
#include "scalar_conservation_device.hpp"
#include "shallow_water_device.hpp"

namespace ryujin_hip
{
  /* RYUJIN_IV_* of ryujin_hip.h */
  enum InitialStateId {
    kIvUniform = 0,
    kIvRadialContrast = 1,
    kIvIsentropicVortex = 2,
    kIvLeblanc = 3,
    kIvRarefaction = 4,
    kIvCircularDamBreak = 5,
    kIvParaboloid = 6,
    kIvRitterDamBreak = 7,
    kIvSmoothVortex = 8,
    kIvSlopingFriction = 9,
    /* no RYUJIN_IV_* value: configured by ryujin_hip_initial_values_configure_function, evaluated by
     * initial_state_function() below through kernels of its own */
    kIvFunction = 10
  };

  struct InitialValuesParams {
    int state;
    int roll_z, roll_y;      /* the rolls of affine_transform that are not the identity (norm > 1e-14) */
    double p[16];            /* the state's parameters, ryujin_hip_initial_values::params */
    double c[16];            /* constants derived from them on the host (see the states below) */
    double position[3];
    double nz_x, nz_z;       /* roll about y that takes the z-component away (dim = 3) */
    double ny_x, ny_y;       /* roll about z that takes the y-component away (dim >= 2) */
    /* EulerAEOS: the configured equation of state, for from_initial_state (euler_aeos/hyperbolic_system.h:1470-1512) */
    int eos;
    double eos_gamma, eos_b, eos_q, eos_pinf, eos_a;
    double jwl_A, jwl_B, jwl_R1, jwl_R2, jwl_omega, jwl_rho_0;
  };

  /* affine_transform (initial_values.template.h:70-109) */
  template <int DIM>
  RYUJIN_DEV void iv_transform_point(const InitialValuesParams &P, const double *__restrict__ x, double (&y)[DIM])
  {
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      y[d] = x[d] - P.position[d];
    if constexpr (DIM == 3) {
      if (P.roll_z) {
        const double a = P.nz_x * y[0] + P.nz_z * y[2];
        const double b = -P.nz_z * y[0] + P.nz_x * y[2];
        y[0] = a;
        y[2] = b;
      }
    }
    if constexpr (DIM >= 2) {
      if (P.roll_y) {
        const double a = P.ny_x * y[0] + P.ny_y * y[1];
        const double b = -P.ny_y * y[0] + P.ny_x * y[1];
        y[0] = a;
        y[1] = b;
      }
    }
  }

  /* affine_transform_vector (initial_values.template.h:115-149) */
  template <int DIM>
  RYUJIN_DEV void iv_transform_vector(const InitialValuesParams &P, double (&m)[DIM])
  {
    if constexpr (DIM >= 2) {
      if (P.roll_y) {
        const double a = P.ny_x * m[0] - P.ny_y * m[1];
        const double b = P.ny_y * m[0] + P.ny_x * m[1];
        m[0] = a;
        m[1] = b;
      }
    }
    if constexpr (DIM == 3) {
      if (P.roll_z) {
        const double a = P.nz_x * m[0] - P.nz_z * m[2];
        const double b = P.nz_z * m[0] + P.nz_x * m[2];
        m[0] = a;
        m[2] = b;
      }
    }
  }

  /* EquationOfState::specific_internal_energy(rho, p), as initial_states.aeos_specific_internal_energy */
  RYUJIN_DEV double iv_specific_internal_energy(const InitialValuesParams &P, const double rho, const double p)
  {
    const double g = P.eos_gamma;
    switch (P.eos) {
    case RYUJIN_EOS_POLYTROPIC_GAS:
      return p / (rho * (g - 1.));
    case RYUJIN_EOS_NOBLE_ABEL_STIFFENED_GAS:
      return P.eos_q + (p + g * P.eos_pinf) * (1. - P.eos_b * rho) / (rho * (g - 1.));
    case RYUJIN_EOS_VAN_DER_WAALS:
      return (p + P.eos_a * rho * rho) * (1. - P.eos_b * rho) / (rho * (g - 1.)) - P.eos_a * rho;
    default: {
      const double ratio = rho / P.jwl_rho_0;
      const double first = P.jwl_A * (1. - P.jwl_omega / P.jwl_R1 * ratio) * exp(-P.jwl_R1 / ratio);
      const double second = P.jwl_B * (1. - P.jwl_omega / P.jwl_R2 * ratio) * exp(-P.jwl_R2 / ratio);
      return (p - first - second) / (rho * P.jwl_omega);
    }
    }
  }

  /* The Euler / EulerAEOS states in their own frame: primitive (rho, v, p) with v along the first axis (`v1`) or in
   * the plane (`v1`, `v2`), and the gamma the ideal-gas energy is formed with. */
  struct IvPrimitive {
    double rho, v1, v2, p, gamma;
    int profile_1d; /* the kinetic energy as the 1-D restatements write it: 0.5 rho u u, left to right */
  };

  template <int DIM>
  RYUJIN_DEV IvPrimitive iv_euler_primitive(const InitialValuesParams &P, const double (&x)[DIM], const double t)
  {
    IvPrimitive s{0., 0., 0., 0., P.c[0], 0};
    switch (P.state) {
    case kIvUniform: /* initial_state_uniform.h:36-50 */
      s.rho = P.p[0];
      s.v1 = P.p[1];
      s.p = P.p[2];
      break;
    case kIvRadialContrast: { /* initial_state_radial_contrast.h:29-62 */
      double r2 = x[0] * x[0];
#pragma unroll
      for (int d = 1; d < DIM; ++d)
        r2 += x[d] * x[d];
      const bool inside = sqrt(r2) <= P.p[6];
      s.rho = inside ? P.p[0] : P.p[3];
      s.v1 = inside ? P.p[1] : P.p[4];
      s.p = inside ? P.p[2] : P.p[5];
      break;
    }
    case kIvIsentropicVortex: { /* initial_state_isentropic_vortex.h:54-92 (dim = 2) */
      const double gamma = P.c[0], mach = P.p[0];
      const double xb = x[0] - mach * t;
      const double yb = x[DIM >= 2 ? 1 : 0];
      const double r2 = xb * xb + yb * yb;
      const double factor = P.c[1] /* beta / (2 pi) */ * exp(0.5 - 0.5 * r2);
      const double T = 1. - P.c[2] /* (gamma - 1) / (2 gamma) */ * factor * factor;
      s.v1 = mach - factor * yb;
      s.v2 = factor * xb;
      s.rho = dev_pow(T, P.c[3] /* 1 / (gamma - 1) */);
      s.p = dev_pow(s.rho, gamma);
      break;
    }
    case kIvLeblanc: { /* initial_state_leblanc.h:63-120, gamma = 5/3 */
      constexpr double rarefaction_speed = 0.49578489518897934;
      constexpr double contact_velocity = 0.62183867139173454;
      constexpr double right_shock_speed = 0.82911836253346982;
      constexpr double pre_contact_density = 5.4079335349316249e-02;
      constexpr double post_contact_density = 3.9999980604299963e-03;
      constexpr double contact_pressure = 0.51557792765096996e-03;
      s.profile_1d = 1;
      s.gamma = 5. / 3.;
      const double xx = x[0];
      if (xx <= -1. / 3. * t) {
        s.rho = 1.;
        s.v1 = 0.;
        s.p = 2. / 3. * 1.e-1;
      } else if (xx < rarefaction_speed * t) { /* (never at t = 0: x / t stays inside this branch) */
        const double chi = xx / t;
        const double b = 0.75 - 0.75 * chi;
        const double b3 = b * b * b;
        s.rho = b3;
        s.v1 = 0.75 * (1. / 3. + chi);
        s.p = (1. / 15.) * (b3 * b * b);
      } else if (xx < contact_velocity * t) {
        s.rho = pre_contact_density;
        s.v1 = contact_velocity;
        s.p = contact_pressure;
      } else if (xx < right_shock_speed * t) {
        s.rho = post_contact_density;
        s.v1 = contact_velocity;
        s.p = contact_pressure;
      } else {
        s.rho = 1.e-3;
        s.v1 = 0.;
        s.p = 2. / 3. * 1.e-10;
      }
      break;
    }
    default: { /* kIvRarefaction: initial_state_rarefaction.h:40-160 */
      /* c: 0 gamma, 1 rho_l, 2 u_l, 3 p_l, 4 c_l, 5 rho_r, 6 u_r, 7 p_r, 8 c_r, 9 k1, 10 k2, 11 k3,
       * 12 density_exponent, 13 pressure_exponent, 14 t_0 = 0.2 / (u_r - u_l) */
      s.profile_1d = 1;
      const double xx = x[0];
      const double tt = P.c[14] + t;
      if (xx <= tt * (P.c[2] - P.c[4])) {
        s.rho = P.c[1];
        s.v1 = P.c[2];
        s.p = P.c[3];
      } else if (xx <= tt * (P.c[6] - P.c[8])) {
        const double chi = xx / tt;
        const double base = P.c[9] + P.c[10] * (P.c[2] - chi);
        s.rho = P.c[1] * dev_pow(base, P.c[12]);
        s.v1 = P.c[9] * (P.c[11] + chi);
        s.p = P.c[3] * dev_pow(base, P.c[13]);
      } else {
        s.rho = P.c[5];
        s.v1 = P.c[6];
        s.p = P.c[7];
      }
      break;
    }
    }
    return s;
  }

  /* initial_state(position, t) of the configured state for the Description E, conserved, U[E::K].
   * E = Euler<DIM>: from_primitive_state with the ideal gas (euler/hyperbolic_system.h:1255-1272);
   * E = EulerAeos<DIM>: from_initial_state through the configured equation of state;
   * E = ShallowWater<DIM>: (h, q). */
  template <typename E>
  RYUJIN_DEV void initial_state(const InitialValuesParams &P, const double *__restrict__ x_in, const double t,
                                double (&U)[E::K])
  {
    constexpr int DIM = E::DIMENSION;
    double x[DIM];
    iv_transform_point<DIM>(P, x_in, x);
    double m[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      m[d] = 0.;

    if constexpr (std::is_same<typename E::Params, ShallowWaterParams>::value) {
      double h = 0.;
      switch (P.state) {
      case kIvCircularDamBreak: { /* initial_state_circular_dam_break.h:48-54: |x|^2 against `radius`, sic */
        double r2 = x[0] * x[0];
#pragma unroll
        for (int d = 1; d < DIM; ++d)
          r2 += x[d] * x[d];
        h = r2 <= P.p[1] ? P.p[2] : P.p[0];
        break;
      }
      case kIvParaboloid: { /* initial_state_paraboloid.h:66-101 (dim = 1) */
        /* p: 0 a, 1 h0, 2 length, 3 B; c: 0 g, 1 k, 2 h0 / (a a), 3 s, 4 a a B B / (8 g g h0), 5 1/4 k k - s s,
         * 6 s k, 7 -(B B / (4 g)), 8 -(B / g) */
        const double k = P.c[1], s = P.c[3], B = P.p[3];
        const double xc = x[0] - 0.5 * P.p[2];
        const double z = P.c[2] * (xc * xc);
        double term1 = P.c[4] * exp(-k * t);
        term1 *= P.c[5] * cos(2. * s * t) - P.c[6] * sin(2. * s * t);
        const double term2 = P.c[7] * exp(-k * t);
        double term3 = P.c[8] * exp(-1. / 2. * k * t);
        term3 = term3 * (s * cos(s * t) + 1. / 2. * k * sin(s * t)) * (x[0] - 1. / 2. * P.p[2]);
        double htilde = P.p[1] - z;
        htilde = htilde + (term1 + term2 + term3);
        h = fmax(htilde, 0.);
        const double v = B * exp(-1. / 2. * k * t) * sin(s * t);
        m[0] = h * v;
        break;
      }
      case kIvRitterDamBreak: { /* initial_state_ritter_dam_break.h:58-80 */
        /* p: 0 time_initial, 1 left_depth; c: 0 g, 1 aL = sqrt(g left_depth), 2 4 / (9 g) */
        const double aL = P.c[1];
        const double ts = t + P.p[0];
        const double xA = -ts * aL;
        const double xB = 2. * ts * aL;
        if (x[0] <= xA) {
          h = P.p[1];
        } else if (x[0] <= xB) {
          const double tmp = aL - x[0] / (2. * ts);
          h = P.c[2] * tmp * tmp;
          const double v = 2. / 3. * (x[0] / ts + aL);
          m[0] = h * v;
        }
        break;
      }
      case kIvSmoothVortex: { /* initial_state_smooth_vortex.h:55-85, without bathymetry (dim = 2) */
        /* p: 0 reference depth, 1 mach, 2 beta; c: 0 g, 1 beta / (2 pi), 2 1 / (2 g) */
        const double mach = P.p[1];
        const double xb = x[0] - mach * t;
        const double yb = x[DIM >= 2 ? 1 : 0];
        const double r2 = xb * xb + yb * yb;
        const double factor = P.c[1] * exp(0.5 - 0.5 * r2);
        h = P.p[0] - P.c[2] * factor * factor;
        const double u = mach - factor * yb;
        const double v = factor * xb;
        m[0] = h * u;
        if constexpr (DIM >= 2)
          m[1] = h * v;
        break;
      }
      default: /* kIvSlopingFriction: initial_state_sloping_friction.h:50-85; c: 0 the uniform depth */
        h = P.c[0];
        m[0] = P.p[1];
        break;
      }
      iv_transform_vector<DIM>(P, m);
      U[0] = h;
#pragma unroll
      for (int d = 0; d < DIM; ++d)
        U[1 + d] = m[d];
    } else {
      const IvPrimitive s = iv_euler_primitive<DIM>(P, x, t);
      m[0] = s.rho * s.v1;
      if constexpr (DIM >= 2)
        m[1] = s.rho * s.v2;
      double kinetic;
      if (s.profile_1d)
        kinetic = 0.5 * s.rho * s.v1 * s.v1;
      else
        kinetic = 0.5 * s.rho * (s.v1 * s.v1 + s.v2 * s.v2);
      double E_total;
      if constexpr (std::is_same<typename E::Params, EulerAeosParams>::value)
        E_total = s.rho * iv_specific_internal_energy(P, s.rho, s.p) +
                  0.5 * s.rho * (s.v1 * s.v1 + s.v2 * s.v2);
      else
        E_total = s.p / (s.gamma - 1.) + kinetic;
      iv_transform_vector<DIM>(P, m);
      U[0] = s.rho;
#pragma unroll
      for (int d = 0; d < DIM; ++d)
        U[1 + d] = m[d];
      U[1 + DIM] = E_total;
    }
  }

  /* initial_state<EulerAeos<DIM>>() on a context whose equation of state is the "function" one: from_initial_state
   * takes specific_internal_energy(rho, p) from the sie program of the interpreter (eos_function_value), everything
   * else is the statements above on the same operands. Every lane of the wave calls it, a lane without a point with
   * active = false: its interpreter runs on (1, 1) and the caller stores nothing. */
  template <int DIM, int BLOCK>
  RYUJIN_DEV void initial_state_eos_function(const InitialValuesParams &P, const EosProgram *__restrict__ F,
                                             const double (&x_in)[DIM], const double t, const bool active,
                                             double *column, double (&U)[DIM + 2])
  {
    double x[DIM];
    iv_transform_point<DIM>(P, x_in, x);
    const IvPrimitive s = iv_euler_primitive<DIM>(P, x, t);
    const double sie = eos_function_value<BLOCK>(F, kEosSpecificInternalEnergy, active ? s.rho : 1.,
                                                 active ? s.p : 1., column);
    double m[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      m[d] = 0.;
    m[0] = s.rho * s.v1;
    if constexpr (DIM >= 2)
      m[1] = s.rho * s.v2;
    const double E_total = s.rho * sie + 0.5 * s.rho * (s.v1 * s.v1 + s.v2 * s.v2);
    iv_transform_vector<DIM>(P, m);
    U[0] = s.rho;
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      U[1 + d] = m[d];
    U[1 + DIM] = E_total;
  }

  /* ---- configuration = function: one expression in (x, t) per primitive component -------------------------- */

  constexpr int kIvMaxExpressions = 5; /* Euler, dim = 3: density, three velocities, pressure */

  /* The programs of the components back to back, each closed by kExResult with its component as `slot`. The same
   * for every lane: read through a const __restrict__ kernel argument at wave-uniform indices, i.e. by scalar loads,
   * and every branch on an opcode is wave-uniform. */
  struct IvFunctionProgram {
    int n;
    int pad;
    ExprInstruction code[kIvMaxExpressions * (RYUJIN_EXPR_MAX_INSTRUCTIONS + 1)];
  };

  /* doubles of LDS per block of `block` threads: [slot][lane], operands first, then the components' values; a lane
   * reads and writes its own column only (no barrier), consecutive lanes consecutive doubles (no bank conflict) */
  constexpr int iv_function_lds_doubles(const int block)
  {
    return (RYUJIN_EXPR_MAX_STACK + kIvMaxExpressions) * block;
  }

  template <int BLOCK>
  struct IvLdsStack {
    double *column; /* &lds[lane] */
    RYUJIN_DEV double load(const int slot) const { return column[slot * BLOCK]; }
    RYUJIN_DEV void store(const int slot, const double value) { column[slot * BLOCK] = value; }
  };

  struct IvDevicePow {
    RYUJIN_DEV double operator()(const double a, const double b) const { return dev_pow(a, b); }
  };

  /* initial_state(position, t) of the function state, conserved, U[E::K]: affine_transform of the point, the K
   * programs at the transformed point and t, from_primitive_state of the Description as Function::compute calls it
   * (euler/hyperbolic_system.h:1255-1272: p / (gamma - 1) + 1/2 rho |v|^2; euler_aeos/hyperbolic_system.h:1473-1493:
   * the LAST primitive component is the specific internal energy e, E = rho e + 1/2 rho |v|^2, no equation of state
   * enters; shallow_water/hyperbolic_system.h:1286-1297: (h, h v); scalar conservation: the value itself), the
   * momentum rotated back. Every lane of the wave calls it (a lane without a point passes any finite x): the
   * interpreter's loop is not under a divergent branch. */
  template <typename E, int BLOCK>
  RYUJIN_DEV void initial_state_function(const InitialValuesParams &P, const IvFunctionProgram *__restrict__ F,
                                         const double (&x_in)[E::DIMENSION], const double t, double *column,
                                         double (&U)[E::K])
  {
    constexpr int DIM = E::DIMENSION, K = E::K;
    static_assert(K <= kIvMaxExpressions, "one expression per primitive component");
    double x[DIM];
    iv_transform_point<DIM>(P, x_in, x);
    IvLdsStack<BLOCK> stack{column};
    expr_evaluate(F->code, F->n, x[0], x[DIM >= 2 ? 1 : 0], x[DIM >= 3 ? 2 : 0], t, stack, IvDevicePow{});
    double prim[K];
#pragma unroll
    for (int q = 0; q < K; ++q)
      prim[q] = stack.load(RYUJIN_EXPR_MAX_STACK + q);

    if constexpr (std::is_same<typename E::Params, ScalarParams>::value) {
      U[0] = prim[0];
    } else {
      double m[DIM];
#pragma unroll
      for (int d = 0; d < DIM; ++d)
        m[d] = prim[0] * prim[1 + d];
      iv_transform_vector<DIM>(P, m);
      U[0] = prim[0];
#pragma unroll
      for (int d = 0; d < DIM; ++d)
        U[1 + d] = m[d];
      if constexpr (!std::is_same<typename E::Params, ShallowWaterParams>::value) {
        double v2 = prim[1] * prim[1];
#pragma unroll
        for (int d = 1; d < DIM; ++d)
          v2 += prim[1 + d] * prim[1 + d];
        const double kinetic = 0.5 * prim[0] * v2;
        if constexpr (std::is_same<typename E::Params, EulerAeosParams>::value)
          U[1 + DIM] = prim[0] * prim[1 + DIM] + kinetic;
        else
          U[1 + DIM] = prim[1 + DIM] / (P.c[0] - 1.) + kinetic;
      }
    }
  }
} // namespace ryujin_hip
