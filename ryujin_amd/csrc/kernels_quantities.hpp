// HIP kernels for Quantities::accumulate() (point maps, space and time averages), gfx950.
//
// Reference: source/quantities.template.h.
//   k_quantities_sweep   internal_accumulate() (:369-407) and the trapezoid update of accumulate() (:536-545) in ONE
//                        pass over the points of a manifold: one lane per point, U_i gathered through the index list
//                        (or addressed directly when the list is one contiguous run), (V, V o V) of
//                        V = to_primitive_state(U_i) stored, the time sums updated in the reference's order
//                          sum += 0.5 tau old;  sum += 0.5 tau new
//                        against ONE array of previous values that is overwritten behind the sum (val_old / val_new
//                        of the reference without the swap), and the 1 + 2k weighted sums  sum w, sum w V, sum w V o V
//                        folded per lane, per wave (shuffles), per block (LDS, the waves in order): one partial row
//                        per block
//   k_quantities_final   one wave: the block partials lane-strided, then the same shuffle tree; on one rank it
//                        divides by the mass sum (:420-421) and writes the row (t, mean V, mean V o V) of the time
//                        series at the row number the host hands over
//   k_quantities_row     the division and the row behind the sum over the ranks
// No floating-point atomics anywhere: launch shape and summation order are fixed by (n_points, kQuantitiesMaxBlocks)
// alone, so a series is reproducible bit for bit for a given partition.
//
// Longest chain of additions a term passes through (tests/helpers_quantities.py computes its tolerance from these
// constants): ceil(n_points / (blocks * kBlock)) per lane + 6 shuffle levels + kWavesPerBlock
// + ceil(blocks / 64) per lane of the final wave + 6 shuffle levels (+ the ranks).

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_euler.hpp"
#include "primitive_state_device.hpp"

namespace ryujin_hip
{
  constexpr int kQuantitiesMaxBlocks = 1024; /* 4 blocks = 16 waves per CU on 256 CUs */

  struct QuantitiesSweep {
    uint32_t n_points;
    uint32_t first;        /* contiguous run: point p is row first + p */
    const uint32_t *index; /* gather path: point p is row index[p] */
    const double *weight;  /* [n_points] */
    int store;             /* write (V, V o V) to values */
    int add;               /* values holds the previous call's: update sum (time averaging, not the first call) */
    int reduce;            /* fold the weighted sums into partial */
    double half_tau;       /* 0.5 * (t_new - t_old) */
    double *values;        /* [n_points][2 K] */
    double *sum;           /* [n_points][2 K] */
    double *partial;       /* [gridDim.x][1 + 2 K] */
  };

  template <typename E, bool GATHER>
  __global__ void __launch_bounds__(kBlock)
  k_quantities_sweep(const typename E::Params P, const QuantitiesSweep S, const double *__restrict__ U)
  {
    constexpr int K = E::K;
    constexpr int NQ = 1 + 2 * K;
    __shared__ double lds[kWavesPerBlock][NQ];

    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      acc[q] = 0.;

    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < S.n_points; p += stride) {
      const uint32_t i = GATHER ? S.index[p] : S.first + p;
      double U_i[K], V[K], x[2 * K];
      load_state<K>(U, i, U_i);
      primitive_state(P, static_cast<const E *>(nullptr), U_i, V);
#pragma unroll
      for (int q = 0; q < K; ++q) {
        x[q] = V[q];
        x[K + q] = V[q] * V[q]; /* schur_product (:400) */
      }

      if (S.store) { /* wave-uniform */
        double2 *v = reinterpret_cast<double2 *>(S.values + (size_t)p * (2 * K));
        if (S.add) {
          double2 *s = reinterpret_cast<double2 *>(S.sum + (size_t)p * (2 * K));
#pragma unroll
          for (int g = 0; g < K; ++g) {
            const double2 old = v[g];
            double2 a = s[g];
            a.x += S.half_tau * old.x;
            a.x += S.half_tau * x[2 * g];
            a.y += S.half_tau * old.y;
            a.y += S.half_tau * x[2 * g + 1];
            s[g] = a;
          }
        }
#pragma unroll
        for (int g = 0; g < K; ++g)
          v[g] = double2{x[2 * g], x[2 * g + 1]};
      }

      if (S.reduce) {
        const double w = S.weight[p];
        acc[0] += w;
#pragma unroll
        for (int q = 0; q < 2 * K; ++q)
          acc[1 + q] += w * x[q];
      }
    }

    if (!S.reduce)
      return;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      double v = acc[q];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, 64);
      if ((threadIdx.x & 63) == 0)
        lds[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < NQ) {
      double v = 0.;
#pragma unroll
      for (int w = 0; w < kWavesPerBlock; ++w)
        v += lds[w][threadIdx.x];
      S.partial[(size_t)blockIdx.x * NQ + threadIdx.x] = v;
    }
  }

  /* launched with ONE wave. sums [NQ] always; row [NQ] = (t, sums[1..] / sums[0]) unless null (more than one rank:
   * k_quantities_row behind the sum over the ranks). n_blocks = 0 (no point on this rank) gives zeros. */
  template <int NQ>
  __global__ void __launch_bounds__(64)
  k_quantities_final(const uint32_t n_blocks, const double *__restrict__ partial, const double t,
                     double *__restrict__ sums, double *__restrict__ row)
  {
    double s[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      double v = 0.;
      for (uint32_t b = threadIdx.x; b < n_blocks; b += 64)
        v += partial[(size_t)b * NQ + q];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, 64);
      s[q] = v;
    }
    if (threadIdx.x != 0)
      return;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      sums[q] = s[q];
    if (row) {
      row[0] = t;
#pragma unroll
      for (int q = 1; q < NQ; ++q)
        row[q] = s[q] / s[0];
    }
  }

  template <int NQ>
  __global__ void k_quantities_row(const double *__restrict__ sums, const double t, double *__restrict__ row)
  {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
      const double mass = sums[0];
      row[0] = t;
#pragma unroll
      for (int q = 1; q < NQ; ++q)
        row[q] = sums[q] / mass;
    }
  }
} // namespace ryujin_hip
