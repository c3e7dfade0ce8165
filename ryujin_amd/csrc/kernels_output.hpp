// HIP kernels for VTUOutput on the device (gfx950): the level-set cell selection and the per-output extraction.
//
// Reference: source/vtu_output.template.h:80-205 (schedule_output) and source/selected_components_extractor.h.
// Configure time (everything that depends on the mesh and the manifolds only):
//   k_output_levelsets     the manifold programs at the nodes, f [n_manifolds][n_nodes]: the shape of
//                          k_initial_state_points<IvFunctionSource> -- the programs read by scalar loads, the operand
//                          stack a [slot][lane] column of LDS, no thread leaves before the interpreter has run
//   k_output_cell_flags    one lane per cell: output_cell_selected() (output_selection.hpp) on the vertex values
//   k_output_count         set flags per block of kBlock items: wave ballots, one LDS add per wave
//   k_output_scan          ONE block turns the block counts into exclusive offsets, kBlock counts per round with a
//                          running carry; a launch of its own between the count and the compaction, so that no block
//                          ever waits for another one (no look-back, no cooperative launch)
//   k_output_compact       item i with a set flag goes to offsets[block] + (set flags before it in its block): the
//                          list keeps ascending index, so the result is reproducible and equal to numpy.flatnonzero
//   k_output_mark_nodes    the vertices of the selected cells (plain stores of the same byte)
//   k_output_connectivity  the selected cells' vertices in the new node numbering
// Per output:
//   k_output_extract       one lane per output node: U read once, to_primitive_state evaluated once, every requested
//                          quantity written SoA [n_quantities][n_nodes] as Float64 or Float32 (one IEEE conversion)
// No floating-point atomics anywhere; the integer flags and lists are written by exactly one lane each.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "initial_states_device.hpp"
#include "kernels_euler.hpp"
#include "kernels_postprocessor.hpp"
#include "output_selection.hpp"
#include "primitive_state_device.hpp"

namespace ryujin_hip
{
  constexpr int kOutputMaxManifolds = 8;   /* RYUJIN_OUT_MAX_MANIFOLDS */
  constexpr int kOutputMaxQuantities = 32; /* RYUJIN_OUT_MAX_QUANTITIES */
  constexpr int kOutputMaxVertices = 8;    /* 2^dim, dim <= 3 */
  constexpr int kOutputLevelsetBlock = 64;
  static_assert(kOutputBlock == kBlock, "output_selection.hpp plans for the block of the kernels");

  /* The programs of the manifolds back to back, each closed by kExResult with its manifold as `slot`
   * (the layout of IvFunctionProgram). */
  struct OutputManifoldProgram {
    int n;
    int n_manifolds;
    ExprInstruction code[kOutputMaxManifolds * (RYUJIN_EXPR_MAX_INSTRUCTIONS + 1)];
  };

  constexpr int output_levelset_lds_doubles(const int block)
  {
    return (RYUJIN_EXPR_MAX_STACK + kOutputMaxManifolds) * block;
  }

  template <int DIM>
  __global__ __launch_bounds__(kOutputLevelsetBlock) void k_output_levelsets(
      const OutputManifoldProgram *__restrict__ program, const uint32_t n_nodes, const double *__restrict__ positions,
      double *__restrict__ f)
  {
    __shared__ double lds[output_levelset_lds_doubles(kOutputLevelsetBlock)];
    const uint32_t i = blockIdx.x * (uint32_t)kOutputLevelsetBlock + threadIdx.x;
    const bool active = i < n_nodes;
    double x[3] = {0., 0., 0.};
#pragma unroll
    for (int d = 0; d < DIM; ++d)
      x[d] = active ? positions[(size_t)i * DIM + d] : 0.;
    IvLdsStack<kOutputLevelsetBlock> stack{lds + threadIdx.x};
    /* FunctionParser<dim>(expression) has no time: the parser knows no `t`, the interpreter's fourth variable is unused */
    expr_evaluate(program->code, program->n, x[0], x[1], x[2], 0., stack, IvDevicePow{});
    if (!active)
      return;
    const int n_manifolds = program->n_manifolds;
    for (int m = 0; m < n_manifolds; ++m)
      f[(size_t)m * n_nodes + i] = stack.load(RYUJIN_EXPR_MAX_STACK + m);
  }

  /* cell_dofs [dofs_per_cell][n_cells] (transposed: lane = cell reads it coalesced) */
  __global__ __launch_bounds__(kBlock) void k_output_cell_flags(const uint32_t n_cells, const int dofs_per_cell,
                                                                const uint32_t *__restrict__ cell_dofs,
                                                                const int n_manifolds, const uint32_t n_nodes,
                                                                const double *__restrict__ f,
                                                                uint8_t *__restrict__ flags)
  {
    const uint32_t c = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (c >= n_cells)
      return;
    uint32_t dof[kOutputMaxVertices];
#pragma unroll
    for (int v = 0; v < kOutputMaxVertices; ++v)
      dof[v] = v < dofs_per_cell ? cell_dofs[(size_t)v * n_cells + c] : 0u;
    const bool selected = output_cell_selected(n_manifolds, dofs_per_cell, [&](const int m, const int v) {
      uint32_t j = dof[0];
#pragma unroll
      for (int s = 1; s < kOutputMaxVertices; ++s)
        j = (v == s) ? dof[s] : j;
      return f[(size_t)m * n_nodes + j];
    });
    flags[c] = selected ? 1 : 0;
  }

  RYUJIN_DEV uint32_t output_lane() { return threadIdx.x & 63u; }

  __global__ __launch_bounds__(kBlock) void k_output_count(const uint32_t n, const uint8_t *__restrict__ flags,
                                                           uint32_t *__restrict__ counts)
  {
    __shared__ uint32_t wave_count[kBlock / 64];
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    const bool set = i < n && flags[i] != 0;
    const unsigned long long ballot = __ballot(set);
    if (output_lane() == 0)
      wave_count[threadIdx.x / 64] = (uint32_t)__popcll(ballot);
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t total = 0;
#pragma unroll
      for (int w = 0; w < kBlock / 64; ++w)
        total += wave_count[w];
      counts[blockIdx.x] = total;
    }
  }

  /* launched with ONE block: offsets[b] = counts[0] + ... + counts[b - 1], b in [0, n_blocks]; rounds of kBlock
   * counts, the carry of the rounds before in a register of every thread */
  __global__ __launch_bounds__(kBlock) void k_output_scan(const uint32_t n_blocks, const uint32_t *__restrict__ counts,
                                                          uint32_t *__restrict__ offsets)
  {
    __shared__ uint32_t wave_total[kBlock / 64];
    const uint32_t lane = output_lane(), wave = threadIdx.x / 64;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += kBlock) {
      const uint32_t b = base + threadIdx.x;
      const uint32_t mine = b < n_blocks ? counts[b] : 0u;
      /* inclusive scan over the wave */
      uint32_t inclusive = mine;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t other = __shfl_up(inclusive, off, 64);
        if (lane >= (uint32_t)off)
          inclusive += other;
      }
      if (lane == 63)
        wave_total[wave] = inclusive;
      __syncthreads();
      uint32_t before = 0, round_total = 0;
#pragma unroll
      for (uint32_t w = 0; w < kBlock / 64; ++w) {
        before += w < wave ? wave_total[w] : 0u;
        round_total += wave_total[w];
      }
      if (b < n_blocks)
        offsets[b] = carry + before + inclusive - mine;
      carry += round_total;
      __syncthreads(); /* wave_total is rewritten in the next round */
    }
    if (threadIdx.x == 0)
      offsets[n_blocks] = carry;
  }

  /* list [offsets[n_blocks]]; map (may be NULL) [n]: the position of item i in the list, or kOutputNotSelected */
  __global__ __launch_bounds__(kBlock) void k_output_compact(const uint32_t n, const uint8_t *__restrict__ flags,
                                                             const uint32_t *__restrict__ offsets,
                                                             uint32_t *__restrict__ list, uint32_t *__restrict__ map)
  {
    __shared__ uint32_t wave_count[kBlock / 64];
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    const uint32_t lane = output_lane(), wave = threadIdx.x / 64;
    const bool set = i < n && flags[i] != 0;
    const unsigned long long ballot = __ballot(set);
    if (lane == 0)
      wave_count[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (uint32_t w = 0; w < kBlock / 64; ++w)
      before += w < wave ? wave_count[w] : 0u;
    const uint32_t rank = before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    const uint32_t position = offsets[blockIdx.x] + rank;
    if (set)
      list[position] = i;
    if (map && i < n)
      map[i] = set ? position : kOutputNotSelected;
  }

  __global__ __launch_bounds__(kBlock) void k_output_mark_nodes(const uint32_t n_selected, const uint32_t n_cells,
                                                                const int dofs_per_cell,
                                                                const uint32_t *__restrict__ cell_ids,
                                                                const uint32_t *__restrict__ cell_dofs,
                                                                uint8_t *__restrict__ node_flags)
  {
    const uint32_t s = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (s >= n_selected)
      return;
    const uint32_t c = cell_ids[s];
    for (int v = 0; v < dofs_per_cell; ++v)
      node_flags[cell_dofs[(size_t)v * n_cells + c]] = 1;
  }

  /* connectivity [n_selected][dofs_per_cell] in the caller's vertex order */
  __global__ __launch_bounds__(kBlock) void k_output_connectivity(const uint32_t n_selected, const uint32_t n_cells,
                                                                  const int dofs_per_cell,
                                                                  const uint32_t *__restrict__ cell_ids,
                                                                  const uint32_t *__restrict__ cell_dofs,
                                                                  const uint32_t *__restrict__ node_map,
                                                                  uint32_t *__restrict__ connectivity)
  {
    const uint32_t s = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (s >= n_selected)
      return;
    const uint32_t c = cell_ids[s];
    for (int v = 0; v < dofs_per_cell; ++v)
      connectivity[(size_t)s * dofs_per_cell + v] = node_map[cell_dofs[(size_t)v * n_cells + c]];
  }

  /* What one output writes: run-time data in device memory, the same for every lane (read through a const __restrict__
   * pointer at wave-uniform indices, i.e. by scalar loads; every branch on it is wave-uniform). */
  struct OutputDesc {
    int n;             /* quantities */
    int any_state;     /* some quantity reads U or to_primitive_state(U) */
    int any_primitive; /* ... the latter */
    int n_precomputed, n_initial_precomputed; /* components per node of the two AoS arrays */
    int kind[kOutputMaxQuantities];           /* OutputKind */
    int index[kOutputMaxQuantities];          /* conserved, primitive: the component; precomputed, initial: the column */
    const double *column[kOutputMaxQuantities]; /* alpha, postprocessed: one double per node */
  };

  /* node_ids == NULL: the nodes [0, n_nodes) themselves (the full output) */
  template <typename E, typename T>
  __global__ __launch_bounds__(kBlock) void k_output_extract(const typename E::Params P,
                                                             const OutputDesc *__restrict__ desc,
                                                             const uint32_t n_nodes,
                                                             const uint32_t *__restrict__ node_ids,
                                                             const double *__restrict__ U,
                                                             const double *__restrict__ precomputed,
                                                             const double *__restrict__ initial_precomputed,
                                                             T *__restrict__ out)
  {
    constexpr int K = E::K;
    constexpr int KP = StatePad<K>::KP;
    const OutputDesc &D = *desc;
    const uint32_t p = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (p >= n_nodes)
      return;
    const uint32_t i = node_ids ? node_ids[p] : p;

    double V[2 * K];
#pragma unroll
    for (int q = 0; q < 2 * K; ++q)
      V[q] = 0.;
    if (D.any_state) { /* wave-uniform */
      double U_i[K], prim_i[K];
      const double2 *b = reinterpret_cast<const double2 *>(U + (size_t)i * KP);
#pragma unroll
      for (int g = 0; g < KP / 2; ++g) {
        const double2 t = b[g];
        U_i[2 * g] = t.x;
        if (2 * g + 1 < K)
          U_i[2 * g + 1] = t.y;
      }
#pragma unroll
      for (int q = 0; q < K; ++q)
        prim_i[q] = U_i[q];
      if (D.any_primitive) /* wave-uniform */
        primitive_state(P, static_cast<const E *>(nullptr), U_i, prim_i);
#pragma unroll
      for (int q = 0; q < K; ++q) {
        V[q] = U_i[q];
        V[K + q] = prim_i[q];
      }
    }

    for (int q = 0; q < D.n; ++q) {
      const int kind = D.kind[q], index = D.index[q];
      double value;
      if (kind == kOutConserved)
        value = select_component(V, index);
      else if (kind == kOutPrimitive)
        value = select_component(V, K + index);
      else if (kind == kOutPrecomputed)
        value = precomputed[(size_t)i * D.n_precomputed + index];
      else if (kind == kOutInitialPrecomputed)
        value = initial_precomputed[(size_t)i * D.n_initial_precomputed + index];
      else
        value = D.column[q][i];
      out[(size_t)q * n_nodes + p] = (T)value;
    }
  }
} // namespace ryujin_hip
