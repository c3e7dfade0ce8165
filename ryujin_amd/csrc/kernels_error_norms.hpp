// HIP kernels for TimeLoop::compute_error() (analytic-solution error norms), gfx950.
//
// Reference: source/time_loop.template.h:692-833. U is the state vector, A the analytic one (both AoS with the padded
// stride of a state vector, ghost rows filled), e = U - A per node and selected component.
//   k_error_norms_nodal   linfty_norm() of e and of A over the owned rows (:740, :774): max |.| per lane, per wave
//                         (shuffles), published with one atomic on the bit pattern of the non-negative double (order
//                         preserving, as the postprocessor's bounds): exact and independent of the launch shape
//   k_error_norms_cells   VectorTools::integrate_difference(.., L1_norm | L2_norm) against the zero function (:743-792)
//                         over the cells of this rank: one lane per cell. The vertex indices [v][cell] and JxW
//                         [q][cell] (or the cell measure [cell], JxW_q = weights[q] * measure) are coalesced streams
//                         read ONCE per cell; the shape table N[q][v] sits in LDS (wave-uniform index: a broadcast).
//                         The component loop is the outer loop: a lane holds the 2 * dofs_per_cell nodal values of one
//                         component, forms e_q = sum_v N_qv e_v and A_q likewise, and adds
//                           |e_q| JxW_q,  e_q^2 JxW_q,  |A_q| JxW_q,  A_q^2 JxW_q
//                         to four sums per component. Index loads stand in front of the gathers, there is no store in
//                         the loop. The sums are folded per lane, per wave (shuffles), per block (LDS, the waves in
//                         order): one partial row per block, as k_quantities_sweep.
//                         <DPC, NQ> = (2, 3), (4, 9), (8, 27): Q1 with QGauss(3) in 1-D, 2-D, 3-D, everything in
//                         registers. <0, 0>: any table (dofs_per_cell in [2, 27], n_q in [1, 64]; Q2, dG, another
//                         quadrature): run-time loops that re-read indices and nodal values per quadrature point (from
//                         the cache) instead of keeping arrays a run-time index would push into scratch.
//   k_error_norms_final   one wave: the block partials lane-strided, then the same shuffle tree; on one rank it also
//                         takes the roots and ratios and writes the consolidated sums (:794-805)
//   k_error_norms_result  roots, ratios and consolidated sums behind the reduction over the ranks
// No floating-point atomics anywhere: launch shape and summation order are fixed by (n_cells, kErrorNormsMaxBlocks)
// alone, so the results are reproducible bit for bit for a given partition.
//
// Longest chain of additions a term passes through (tests/helpers_error_norms.py computes its tolerance from these
// constants): n_q within the cell + ceil(n_cells / (blocks * kBlock)) per lane + 6 shuffle levels + kWavesPerBlock
// + ceil(blocks / 64) per lane of the final wave + 6 shuffle levels (+ the ranks).

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels_euler.hpp"
#include "kernels_postprocessor.hpp"

namespace ryujin_hip
{
  constexpr int kErrorNormsMaxBlocks = 1024;   /* 4 blocks = 16 waves per CU on 256 CUs */
  constexpr int kErrorNormsMaxComponents = 5;  /* problem_dimension of Euler in 3-D */
  constexpr int kErrorNormsMaxDofs = 27;       /* Q2 in 3-D */
  constexpr int kErrorNormsMaxPoints = 64;
  constexpr int kErrorNormsSums = 4 * kErrorNormsMaxComponents; /* per component: L1 e, L2^2 e, L1 A, L2^2 A */
  /* result row: (Linf, L1, L2) consolidated, then per component (Linf, L1, L2 of e; Linf, L1, L2 of A) */
  constexpr int kErrorNormsResult = 3 + 6 * kErrorNormsMaxComponents;

  struct ErrorNormsDesc {
    int n;                                   /* number of selected components */
    int component[kErrorNormsMaxComponents]; /* their indices in the state */
    int stride;                              /* doubles per node of U and A (the padded state) */
    int normalize;
  };

  struct ErrorNormsCells {
    uint32_t n_cells;
    int dofs_per_cell, n_q;
    int jxw_per_cell;          /* jxw is [n_cells], JxW_q = weights[q] * jxw[cell]; else jxw is [n_q][n_cells] */
    const uint32_t *cell_dofs; /* [dofs_per_cell][n_cells] */
    const double *jxw;
    const double *shape;       /* [n_q][dofs_per_cell] */
    const double *weights;     /* [n_q] (zeros without jxw_per_cell) */
    double *partial;           /* [gridDim.x][kErrorNormsSums] */
  };

  __global__ void __launch_bounds__(kBlock)
  k_error_norms_nodal(const uint32_t n_owned, const ErrorNormsDesc D, const double *__restrict__ U,
                      const double *__restrict__ A, unsigned long long *__restrict__ max_bits)
  {
    constexpr int MAXC = kErrorNormsMaxComponents;
    double hi_e[MAXC], hi_a[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      hi_e[c] = hi_a[c] = 0.;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_owned; i += stride) {
      const size_t base = (size_t)i * D.stride;
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        if (c >= D.n) /* wave-uniform */
          break;
        const double a = A[base + D.component[c]];
        const double u = U[base + D.component[c]];
        hi_e[c] = fmax(hi_e[c], fabs(u - a));
        hi_a[c] = fmax(hi_a[c], fabs(a));
      }
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c >= D.n)
        break;
      const double e = wave_max(hi_e[c]);
      const double a = wave_max(hi_a[c]);
      if ((threadIdx.x & 63) == 0) {
        const unsigned long long e_bits = (unsigned long long)__double_as_longlong(e);
        const unsigned long long a_bits = (unsigned long long)__double_as_longlong(a);
        if (e_bits > __hip_atomic_load(&max_bits[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
          atomicMax(&max_bits[c], e_bits);
        if (a_bits > __hip_atomic_load(&max_bits[MAXC + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
          atomicMax(&max_bits[MAXC + c], a_bits);
      }
    }
  }

  template <int DPC, int NQ>
  __global__ void __launch_bounds__(kBlock)
  k_error_norms_cells(const ErrorNormsDesc D, const ErrorNormsCells C, const double *__restrict__ U,
                      const double *__restrict__ A)
  {
    constexpr int MAXC = kErrorNormsMaxComponents;
    constexpr int NS = kErrorNormsSums;
    constexpr bool FIXED = DPC > 0;
    __shared__ double s_shape[kErrorNormsMaxPoints * kErrorNormsMaxDofs];
    __shared__ double s_weights[kErrorNormsMaxPoints];
    __shared__ double lds[kWavesPerBlock][NS];

    const int dpc = FIXED ? DPC : C.dofs_per_cell;
    const int n_q = FIXED ? NQ : C.n_q;
    for (int e = threadIdx.x; e < n_q * dpc; e += blockDim.x)
      s_shape[e] = C.shape[e];
    for (int q = threadIdx.x; q < n_q; q += blockDim.x)
      s_weights[q] = C.weights[q];
    __syncthreads();

    double acc[MAXC][4];
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
#pragma unroll
      for (int s = 0; s < 4; ++s)
        acc[c][s] = 0.;

    const size_t n_cells = C.n_cells;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x; cell < C.n_cells; cell += stride) {
      if constexpr (FIXED) {
        uint32_t idx[DPC];
#pragma unroll
        for (int v = 0; v < DPC; ++v)
          idx[v] = C.cell_dofs[(size_t)v * n_cells + cell];
        double w[NQ];
        if (C.jxw_per_cell) { /* wave-uniform */
          const double measure = C.jxw[cell];
#pragma unroll
          for (int q = 0; q < NQ; ++q)
            w[q] = s_weights[q] * measure;
        } else {
#pragma unroll
          for (int q = 0; q < NQ; ++q)
            w[q] = C.jxw[(size_t)q * n_cells + cell];
        }
        /* The component loop is a real loop (one copy of the NQ * DPC products in the code, not five); what a
         * run-time c would index -- the component list in the kernel arguments, the accumulators -- is reached
         * through chains of selects on a scalar condition, so that both stay in registers. */
#pragma unroll 1
        for (int c = 0; c < D.n; ++c) {
          int comp = D.component[0];
#pragma unroll
          for (int k = 1; k < MAXC; ++k)
            comp = (c == k) ? D.component[k] : comp;
          /* an offset the compiler cannot see through (always 0): without it the NQ * DPC table reads are hoisted
           * out of the component and cell loops into registers -- 432 of them in 3-D, i.e. scratch */
          int table = 0;
          asm volatile("" : "+s"(table));
          double e[DPC], a[DPC];
#pragma unroll
          for (int v = 0; v < DPC; ++v) {
            const size_t at = (size_t)idx[v] * D.stride + comp;
            a[v] = A[at];
            e[v] = U[at] - a[v];
          }
          double t[4] = {0., 0., 0., 0.}; /* the sums of this cell */
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            double e_q = 0., a_q = 0.;
#pragma unroll
            for (int v = 0; v < DPC; ++v) {
              const double N = s_shape[table + q * DPC + v];
              e_q += N * e[v];
              a_q += N * a[v];
            }
            t[0] += fabs(e_q) * w[q];
            t[1] += e_q * e_q * w[q];
            t[2] += fabs(a_q) * w[q];
            t[3] += a_q * a_q * w[q];
          }
#pragma unroll
          for (int k = 0; k < MAXC; ++k)
#pragma unroll
            for (int s = 0; s < 4; ++s)
              acc[k][s] += (c == k) ? t[s] : 0.; /* (x + 0 = x: the other components keep their bits) */
        }
      } else {
        const double measure = C.jxw_per_cell ? C.jxw[cell] : 0.;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
          if (c >= D.n)
            break;
          const int comp = D.component[c];
          double t[4] = {0., 0., 0., 0.}; /* the sums of this cell */
          for (int q = 0; q < n_q; ++q) {
            const double w = C.jxw_per_cell ? s_weights[q] * measure : C.jxw[(size_t)q * n_cells + cell];
            double e_q = 0., a_q = 0.;
            for (int v = 0; v < dpc; ++v) {
              const uint32_t i = C.cell_dofs[(size_t)v * n_cells + cell];
              const size_t at = (size_t)i * D.stride + comp;
              const double N = s_shape[q * dpc + v];
              const double a = A[at];
              e_q += N * (U[at] - a);
              a_q += N * a;
            }
            t[0] += fabs(e_q) * w;
            t[1] += e_q * e_q * w;
            t[2] += fabs(a_q) * w;
            t[3] += a_q * a_q * w;
          }
#pragma unroll
          for (int s = 0; s < 4; ++s)
            acc[c][s] += t[s];
        }
      }
    }

#pragma unroll
    for (int c = 0; c < MAXC; ++c)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        double v = acc[c][s];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
          v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0)
          lds[threadIdx.x >> 6][4 * c + s] = v;
      }
    __syncthreads();
    if (threadIdx.x < NS) {
      double v = 0.;
#pragma unroll
      for (int w = 0; w < kWavesPerBlock; ++w)
        v += lds[w][threadIdx.x];
      C.partial[(size_t)blockIdx.x * NS + threadIdx.x] = v;
    }
  }

  /* (:774-805) per component the three norms of e and of A, and the consolidated sums over the components in order.
   * A zero analytic norm gives the reference's IEEE result: x / 0 = inf, 0 / 0 = NaN. */
  RYUJIN_DEV void error_norms_result(const ErrorNormsDesc &D, const double *__restrict__ sums,
                                     const unsigned long long *__restrict__ max_bits, double *__restrict__ result)
  {
    constexpr int MAXC = kErrorNormsMaxComponents;
    double linf = 0., l1 = 0., l2 = 0.;
    for (int c = 0; c < D.n; ++c) {
      const double linf_e = __longlong_as_double((long long)max_bits[c]);
      const double linf_a = __longlong_as_double((long long)max_bits[MAXC + c]);
      const double l1_e = sums[4 * c + 0], l2_e = sqrt(sums[4 * c + 1]);
      const double l1_a = sums[4 * c + 2], l2_a = sqrt(sums[4 * c + 3]);
      double *d = result + 3 + 6 * c;
      d[0] = linf_e;
      d[1] = l1_e;
      d[2] = l2_e;
      d[3] = linf_a;
      d[4] = l1_a;
      d[5] = l2_a;
      if (D.normalize) {
        linf += linf_e / linf_a;
        l1 += l1_e / l1_a;
        l2 += l2_e / l2_a;
      } else {
        linf += linf_e;
        l1 += l1_e;
        l2 += l2_e;
      }
    }
    result[0] = linf;
    result[1] = l1;
    result[2] = l2;
  }

  /* launched with ONE wave. sums [kErrorNormsSums] always; result unless null (more than one rank:
   * k_error_norms_result behind the reduction over the ranks). n_blocks = 0 (no cell on this rank) gives zeros. */
  __global__ void __launch_bounds__(64)
  k_error_norms_final(const ErrorNormsDesc D, const uint32_t n_blocks, const double *__restrict__ partial,
                      double *sums, const unsigned long long *__restrict__ max_bits, double *__restrict__ result)
  {
    constexpr int NS = kErrorNormsSums;
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      double v = 0.;
      for (uint32_t b = threadIdx.x; b < n_blocks; b += 64)
        v += partial[(size_t)b * NS + q];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, 64);
      if (threadIdx.x == 0)
        sums[q] = v;
    }
    /* (the component index is run-time data: the result is formed from the sums in memory, written by this lane) */
    if (threadIdx.x == 0 && result)
      error_norms_result(D, sums, max_bits, result);
  }

  __global__ void k_error_norms_result(const ErrorNormsDesc D, const double *__restrict__ sums,
                                       const unsigned long long *__restrict__ max_bits, double *__restrict__ result)
  {
    if (threadIdx.x == 0 && blockIdx.x == 0)
      error_norms_result(D, sums, max_bits, result);
  }
} // namespace ryujin_hip
