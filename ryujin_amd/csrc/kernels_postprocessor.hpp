// HIP kernels for Postprocessor::compute() (schlieren and vorticity fields), gfx950.
//
// Reference: source/postprocessor.template.h, steps 1 - 3.
//   k_postprocess_sweep      step 1 (:120-207) and the local part of step 2 (:213-237): one lane per row over the
//                            SELL-64 slices like every other sweep; ALL requested quantities in one walk of the row
//                            (one read of c_ij, one gather of U_j per entry), raw values SoA [n_quantities][n_owned],
//                            max |.| / min |.| per quantity folded per wave and published with one atomic on the bit
//                            pattern of the non-negative double (order preserving, as tau_max_bits): exact, and
//                            independent of the launch shape
//   k_postprocess_normalise  step 3 (:243-261), behind the reduction of the bounds over the ranks
// Step 4 (:267-270, AffineConstraints::distribute) has no counterpart: ryujin_hip_offline carries no affine
// constraints; rows of length 1 (constrained DoFs) get 0 as in step 1.
//
// Which components are evaluated is RUN-TIME data (PostprocessDesc in the kernel arguments, wave-uniform): the
// kernels are instantiated per Description and dimension only.

#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "euler_aeos_device.hpp"
#include "euler_device.hpp"
#include "kernels_euler.hpp"
#include "primitive_state_device.hpp"
#include "scalar_conservation_device.hpp"
#include "shallow_water_device.hpp"

namespace ryujin_hip
{
  constexpr int kPostprocessMaxQuantities = 8; /* RYUJIN_PP_MAX_QUANTITIES */
  constexpr int kPostprocessSchlieren = 0, kPostprocessVorticity = 1; /* RYUJIN_PP_SCHLIEREN / _VORTICITY */

  struct PostprocessDesc {
    int n;             /* number of quantities, <= kPostprocessMaxQuantities */
    int any_primitive; /* some quantity reads to_primitive_state(U_j) */
    int load_mask;     /* bit g: some quantity reads the g-th pair of doubles of the (padded) state U_j */
    int kind[kPostprocessMaxQuantities];
    int select[kPostprocessMaxQuantities]; /* is_primitive * K + component: index into (U_j, to_primitive_state(U_j)) */
  };

  /* bounds, device: [0, MAXQ) bit patterns of q_max, [MAXQ, 2 MAXQ) of q_min */
  __global__ void k_postprocess_reset_bounds(unsigned long long *__restrict__ bounds)
  {
    const int q = threadIdx.x;
    if (q < kPostprocessMaxQuantities) {
      bounds[q] = 0ull; /* q_max starts from 0. (:222) */
      bounds[kPostprocessMaxQuantities + q] = (unsigned long long)__double_as_longlong(DBL_MAX);
    }
  }

  /* the pairs of doubles of U_j that some quantity reads (PostprocessDesc::load_mask, wave-uniform): schlieren of rho
   * alone gathers 16 bytes per entry instead of the whole state. The components left out are never selected. */
  template <int K>
  RYUJIN_DEV void load_state_pairs(const double *__restrict__ U, const uint32_t i, const int mask, double (&v)[K])
  {
    constexpr int KP = StatePad<K>::KP;
    const double2 *b = reinterpret_cast<const double2 *>(U + (size_t)i * KP);
#pragma unroll
    for (int g = 0; g < KP / 2; ++g) {
      double2 t{0., 0.};
      if ((mask >> g) & 1)
        t = b[g];
      v[2 * g] = t.x;
      if (2 * g + 1 < K)
        v[2 * g + 1] = t.y;
    }
  }

  /* V[index] for a wave-uniform run-time index: a chain of selects on a scalar condition, so that V stays in
   * registers (a dynamically indexed array would live in scratch) */
  template <int N>
  RYUJIN_DEV double select_component(const double (&V)[N], const int index)
  {
    double x = V[0];
#pragma unroll
    for (int s = 1; s < N; ++s)
      x = (index == s) ? V[s] : x;
    return x;
  }

  RYUJIN_DEV double wave_max(double x)
  {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      x = fmax(x, __shfl_xor(x, off, 64));
    return x;
  }

  template <typename E, bool USE_TILES>
  __global__ void __launch_bounds__(kBlock)
  k_postprocess_sweep(const typename E::Params P, const DeviceMesh M, const PostprocessDesc D,
                      const int fold_bounds, const double *__restrict__ U, double *__restrict__ raw,
                      unsigned long long *__restrict__ bounds)
  {
    constexpr int K = E::K;
    constexpr int DIM = E::DIMENSION;
    constexpr int MAXQ = kPostprocessMaxQuantities;
    const RowCtx r = row_context(M);
    if (!r.valid)
      return;
    const bool owned = r.row < M.n_owned;
    const bool row_active = r.len > 1; /* (r.len is 0 beyond n_owned) */
    const uint32_t i = owned ? r.row : M.n_owned - 1;

    double acc[MAXQ][DIM];
#pragma unroll
    for (int q = 0; q < MAXQ; ++q)
#pragma unroll
      for (int d = 0; d < DIM; ++d)
        acc[q][d] = 0.;

    /* software pipeline (see k_low_order): the operands of column c + 1 and the index of column c + 2 are on
     * their way while column c is worked on; arrived() pins the wait for column c in front of those loads. There
     * is no store inside the loop. Padding entries point at an owned row: the gathers need no predicate. */
    const double *__restrict__ cij = M.cij;
    uint32_t j_n = tile_column<USE_TILES>(M, r.base, r.row, r.lane);
    uint32_t j_nn = r.width > 1 ? tile_column<USE_TILES>(M, (uint64_t)r.base + 1, r.row, r.lane) : i;
    double c_n[DIM], U_n[K];
    load_entry<DIM>(cij, r.base, r.lane, c_n);
    load_state_pairs<K>(U, j_n, D.load_mask, U_n);

    for (uint32_t c = 0; c < r.width; ++c) {
      const uint64_t colbase = (uint64_t)r.base + c;
      const bool active = row_active && c < r.len;
      double c_ij[DIM], V[2 * K];
#pragma unroll
      for (int d = 0; d < DIM; ++d)
        c_ij[d] = c_n[d];
#pragma unroll
      for (int q = 0; q < K; ++q)
        V[q] = U_n[q];
      arrived(c_ij);
#pragma unroll
      for (int q = 0; q < K; ++q)
        arrived(V[q]);
      if (c + 1 < r.width) {
        j_n = j_nn;
        load_entry<DIM>(cij, colbase + 1, r.lane, c_n);
        load_state_pairs<K>(U, j_n, D.load_mask, U_n);
        j_nn = (c + 2 < r.width) ? tile_column<USE_TILES>(M, colbase + 2, r.row, r.lane) : i;
      }

      if (!active)
        continue;

      {
        double U_j[K], prim_j[K];
#pragma unroll
        for (int q = 0; q < K; ++q)
          U_j[q] = prim_j[q] = V[q];
        if (D.any_primitive) /* wave-uniform */
          primitive_state(P, static_cast<const E *>(nullptr), U_j, prim_j);
#pragma unroll
        for (int q = 0; q < K; ++q)
          V[K + q] = prim_j[q];
      }

#pragma unroll
      for (int q = 0; q < MAXQ; ++q) {
        if (q >= D.n) /* wave-uniform */
          break;
        const int s = D.select[q];
        if (D.kind[q] == kPostprocessSchlieren) {
          const double x = select_component(V, s);
#pragma unroll
          for (int d = 0; d < DIM; ++d)
            acc[q][d] += c_ij[d] * x;
        } else if constexpr (DIM == 2) {
          /* -= cross_product_2d(c_ij) * q_j, cross_product_2d(c) = (c_y, -c_x)  (:187) */
          const double x = select_component(V, s), y = select_component(V, s + 1);
          acc[q][0] += c_ij[0] * y - c_ij[1] * x;
        } else if constexpr (DIM == 3) {
          const double x = select_component(V, s), y = select_component(V, s + 1),
                       z = select_component(V, s + 2);
          acc[q][0] += c_ij[1] * z - c_ij[2] * y;
          acc[q][1] += c_ij[2] * x - c_ij[0] * z;
          acc[q][2] += c_ij[0] * y - c_ij[1] * x;
        }
      }
    }

    const double m_i_inverse = 1. / M.mi[i];
    const uint32_t lane = r.lane;
#pragma unroll
    for (int q = 0; q < MAXQ; ++q) {
      if (q >= D.n)
        break;
      double value;
      if (DIM == 2 && D.kind[q] == kPostprocessVorticity) {
        value = acc[q][0] * m_i_inverse; /* signed (:203) */
      } else {
        double n2 = acc[q][0] * acc[q][0];
#pragma unroll
        for (int d = 1; d < DIM; ++d)
          n2 += acc[q][d] * acc[q][d];
        value = sqrt(n2) * m_i_inverse;
      }
      if (!row_active)
        value = 0.;
      if (owned)
        raw[(size_t)q * M.n_owned + r.row] = value;
      if (fold_bounds) { /* wave-uniform */
        const double a = fabs(value);
        const double hi = wave_max(owned ? a : 0.);
        const double lo = wave_min(owned ? a : DBL_MAX);
        if (lane == 0) {
          /* a wave peeks at the running bound and skips the atomic unless it can move it (publish_tau_min) */
          const unsigned long long hi_bits = (unsigned long long)__double_as_longlong(hi);
          const unsigned long long lo_bits = (unsigned long long)__double_as_longlong(lo);
          if (hi_bits > __hip_atomic_load(&bounds[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(&bounds[q], hi_bits);
          if (lo_bits < __hip_atomic_load(&bounds[MAXQ + q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMin(&bounds[MAXQ + q], lo_bits);
        }
      }
    }
  }

  /* step 3 (:243-261): r = max(0, |v| - q_min - floor) / max(q_max - q_min, eps), copysign(1 - exp(-beta r), v) */
  __global__ void __launch_bounds__(kBlock)
  k_postprocess_normalise(const uint32_t n_owned, const int n_quantities, const double beta,
                          const unsigned long long *__restrict__ bounds, const double *__restrict__ raw,
                          double *__restrict__ out)
  {
    constexpr double eps = DBL_EPSILON;
    constexpr double floor = 1.0e-10;
    const size_t n = (size_t)n_owned * n_quantities;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
      const int q = (int)(e / n_owned);
      const double q_max = __longlong_as_double((long long)bounds[q]);
      const double q_min = __longlong_as_double((long long)bounds[kPostprocessMaxQuantities + q]);
      const double v = raw[e];
      const double ratio = fmax(0., fabs(v) - q_min - floor) / fmax(q_max - q_min, eps);
      const double magnitude = 1. - exp(-beta * ratio);
      out[e] = copysign(magnitude, v);
    }
  }
} // namespace ryujin_hip
