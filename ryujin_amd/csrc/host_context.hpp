// The host tables of a context: everything ryujin_hip_ctx::create() derives from the offline data, the parameters and
// the device layout (host_layout.hpp) without a device -- the argument checks, the component counts, the boundary map
// grouped by DoF, the coupling pairs, the export slices, the launch knobs of the mesh and the exchange tables.
// create() (ryujin_hip.hip) calls these in sequence and uploads what they return. No HIP: plain C++17, checked on the
// CPU by tests/cpp/context_tables.cc.

#pragma once

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_layout.hpp"
#include "ryujin_hip.h"

namespace ryujin_hip
{
  /* the error of the library: a status of ryujin_hip.h and its message (guarded(), ryujin_hip.hip) */
  struct HipError : std::runtime_error {
    int status;
    HipError(int status, const std::string &what)
        : std::runtime_error(what)
        , status(status)
    {
    }
  };

  /* Components per node: K of the state (KP: padded to whole pairs, the device stride), NB limiter bounds, NPREC
   * precomputed values, RS doubles of the Riemann record (0: scalar conservation keeps none). The one place that
   * knows them on the host; ryujin_hip.hip ties every field to the Descriptions of the device headers. */
  struct SystemShape {
    int K, KP, NB, NPREC, RS;
    int RS_stored; /* the doubles of the record that memory holds (the stride of the per-state buffer): RS, or 4 of
                    * Euler's 8 in 1-D and 2-D (Euler<DIM>::kRecordStored, euler_device.hpp) */
  };

#ifndef RYUJIN_COMPACT_RECORD
#define RYUJIN_COMPACT_RECORD 1 /* as euler_device.hpp; ryujin_hip.hip ties the two together (shape_matches) */
#endif

  constexpr SystemShape system_shape(const int equation, const int dim)
  {
    SystemShape s{dim + 2, 0, 3, 2, ((dim == 3 ? 9 : 6) + dim + 1) / 2 * 2, 0}; /* Euler: the record holds the state in 3-D */
    const bool stores_whole_record = RYUJIN_COMPACT_RECORD == 0 || dim == 3;
    if (equation == RYUJIN_EQ_EULER_AEOS)
      s = SystemShape{dim + 2, 0, 4, 4, (6 + dim + 1) / 2 * 2, 0};
    else if (equation == RYUJIN_EQ_SHALLOW_WATER)
      s = SystemShape{dim + 1, 0, 5, 2, (2 + dim + 1) / 2 * 2, 0};
    else if (equation == RYUJIN_EQ_SCALAR_CONSERVATION)
      s = SystemShape{1, 0, 2, 2 * dim, 0, 0};
    s.KP = (s.K + 1) / 2 * 2;
    s.RS_stored = (equation == RYUJIN_EQ_EULER && !stores_whole_record) ? 4 : s.RS;
    return s;
  }

  /* What create() refuses without a device and without the layout, in the order in which it always has (the first
   * fault found is the one reported). The refusals that need the layout are made by the builders below. */
  inline void check_create_arguments(const ryujin_hip_offline &o, const ryujin_hip_params &p, const bool have_comm)
  {
    if (p.equation != RYUJIN_EQ_EULER && p.equation != RYUJIN_EQ_SHALLOW_WATER &&
        p.equation != RYUJIN_EQ_EULER_AEOS && p.equation != RYUJIN_EQ_SCALAR_CONSERVATION)
      throw HipError(RYUJIN_ERR_UNSUPPORTED, "unknown equation");
    if (p.equation == RYUJIN_EQ_SCALAR_CONSERVATION) {
      if (p.sc_flux < RYUJIN_FLUX_BURGERS || p.sc_flux > RYUJIN_FLUX_FUNCTION)
        throw HipError(RYUJIN_ERR_UNSUPPORTED, "unknown flux");
      if (p.sc_flux == RYUJIN_FLUX_KPP && p.dim == 3)
        throw HipError(RYUJIN_ERR_UNSUPPORTED, "KPP is only defined in (1 or) 2 space dimensions");
      if (p.sc_random_entropies != 0) /* std::random_device in riemann_solver.template.h:93-107 */
        throw HipError(RYUJIN_ERR_UNSUPPORTED,
                       "scalar conservation: random entropies are not reproducible in the reference");
      for (uint32_t b = 0; b < o.n_bdry; ++b)
        if (o.b_id[b] == RYUJIN_BC_SLIP || o.b_id[b] == RYUJIN_BC_NO_SLIP || o.b_id[b] == RYUJIN_BC_DYNAMIC)
          throw HipError(RYUJIN_ERR_UNSUPPORTED, "slip, no-slip and dynamic boundary conditions are "
                                                 "unavailable for scalar conservation equations");
    }
    if (p.equation == RYUJIN_EQ_EULER_AEOS) {
      if (p.eos < RYUJIN_EOS_POLYTROPIC_GAS || p.eos > RYUJIN_EOS_FUNCTION)
        throw HipError(RYUJIN_ERR_UNSUPPORTED, "unknown equation of state");
      for (uint32_t b = 0; b < o.n_bdry; ++b)
        if (o.b_id[b] == RYUJIN_BC_DYNAMIC) /* __builtin_trap() in euler_aeos/hyperbolic_system.h:1337 */
          throw HipError(RYUJIN_ERR_UNSUPPORTED,
                         "euler aeos: dynamic boundary conditions are not implemented in the reference");
    }
    if (p.equation == RYUJIN_EQ_SHALLOW_WATER && p.dim == 3)
      throw HipError(RYUJIN_ERR_UNSUPPORTED, "the shallow water equations are defined for dim 1 and 2");
    if (p.dim < 1 || p.dim > 3)
      throw HipError(RYUJIN_ERR_ARG, "dim must be 1, 2 or 3");
    if (p.limiter_iterations < 0 || p.limiter_iterations > 2)
      throw HipError(RYUJIN_ERR_ARG, "The number of limiter iterations must be between [0,2]");
    if (p.debug_stencil_classes > 1)
      throw HipError(RYUJIN_ERR_ARG, "debug_stencil_classes must be < 0 (off), 0 or 1 (classes without the table of norms)");
    if (p.debug_pij_storage > 2)
      throw HipError(RYUJIN_ERR_ARG, "debug_pij_storage must be < 0, 0, 1 or 2 (per-tile P_ij in 3-D was retired)");
    if (p.equation == RYUJIN_EQ_SCALAR_CONSERVATION && p.sc_flux == RYUJIN_FLUX_FUNCTION &&
        (!(p.sc_derivative_approximation_delta > 0.) || !std::isfinite(p.sc_derivative_approximation_delta)))
      throw HipError(RYUJIN_ERR_ARG, "flux: derivative approximation delta must be positive and finite");
    if (o.discontinuous_ansatz != 0) {
      /* Scalar conservation: refused. The branch is written (k_low_order_sc<DIM, HAS_STAGES, true>,
       * k_bounds_combine_minmax<2, 0b10>, k_pij_lij<E, true>), but the reference's own scalar Riemann solver cannot
       * run on a dG stencil: the entries between DoFs of face-neighbour cells that do not lie on the shared face have
       * c_ij = 0 exactly, n_ij = c_ij / |c_ij| is 0/0, and |f_i.n - f_j.n| / max(|u_i - u_j|, 2 delta) -- taken
       * through std::max, which returns its first argument when the comparison with a NaN fails
       * (scalar_conservation/riemann_solver.template.h:63,95-96) -- stays NaN: d_ij = 0 * NaN
       * (tests/test_dg_q1.py::test_scalar_conservation_on_a_dg_stencil_is_nan_in_the_reference_formulas). */
      if (p.equation == RYUJIN_EQ_SCALAR_CONSERVATION)
        throw HipError(RYUJIN_ERR_UNSUPPORTED,
                       "discontinuous ansatz with scalar conservation equations: the reference's Riemann solver is 0/0 "
                       "on the structural zeros of a dG stencil");
      if (!o.incidence || !o.mass_matrix_inverse)
        throw HipError(RYUJIN_ERR_ARG, "discontinuous ansatz without incidence / inverse mass matrix");
    }
    if (o.n_nbr > 0 && !have_comm)
      throw HipError(RYUJIN_ERR_COMM, "offline data has neighbour ranks but no communicator was given");
  }

  /* bit c of lower_mask[row] <=> column c of the row lies below the diagonal (cols < row); [rows_padded], all zero
   * where a row may be wider than the 32 bits */
  inline std::vector<uint32_t> lower_mask(const SellLayout &L)
  {
    std::vector<uint32_t> mask(L.rows_padded, 0u);
    if (L.max_row_len <= 32)
      parallel_chunks(L.n_owned, [&](const uint64_t i0, const uint64_t i1) {
        for (uint32_t i = (uint32_t)i0; i < (uint32_t)i1; ++i)
          for (uint32_t c = 1; c < L.row_len[i]; ++c)
            if (L.cols[L.pos(i, c)] < i)
              mask[i] |= 1u << c;
      });
    return mask;
  }

  /* The boundary map grouped by DoF; the entries of a DoF (a group) keep the order of the offline data. */
  struct BoundaryTables {
    uint32_t n_bdry = 0, n_groups = 0;
    std::vector<uint32_t> perm; /* [n_bdry] grouped entry -> entry of the offline data */
    std::vector<uint32_t> b_i;  /* [n_bdry] ... and the offline arrays in that order */
    std::vector<uint8_t> b_id;
    std::vector<double> b_normal;    /* [n_bdry][dim] */
    std::vector<uint32_t> grp_start; /* [n_groups + 1] first entry of every group, then n_bdry */
    std::vector<uint32_t> rows;      /* [n_groups] the DoF of every group, ascending */
    /* which rows of a slice are boundary DoFs, and the group of the first one (BcFold); [n_slices] each */
    std::vector<unsigned long long> bc_mask;
    std::vector<uint32_t> bc_first;
    bool needs_dirichlet = false; /* an id whose boundary condition reads the Dirichlet state */

    /* dst[e] = src[perm[e]], entries of `stride` doubles */
    void permute(const double *src, const int stride, double *dst) const
    {
      for (uint32_t e = 0; e < n_bdry; ++e)
        std::memcpy(dst + (size_t)e * stride, src + (size_t)perm[e] * stride, sizeof(double) * stride);
    }
  };

  inline BoundaryTables build_boundary_tables(const ryujin_hip_offline &o, const SellLayout &L, const int dim)
  {
    BoundaryTables B;
    B.n_bdry = o.n_bdry;
    B.perm.resize(o.n_bdry);
    std::iota(B.perm.begin(), B.perm.end(), 0u);
    std::stable_sort(B.perm.begin(), B.perm.end(), [&](uint32_t a, uint32_t b) { return o.b_i[a] < o.b_i[b]; });
    B.b_i.resize(o.n_bdry);
    B.b_id.resize(o.n_bdry);
    B.b_normal.resize((size_t)o.n_bdry * dim);
    B.permute(o.b_normal, dim, B.b_normal.data());
    for (uint32_t e = 0; e < o.n_bdry; ++e) {
      B.b_i[e] = o.b_i[B.perm[e]];
      if (B.b_i[e] >= o.n_owned)
        throw HipError(RYUJIN_ERR_ARG, "boundary_map entry refers to a non-owned DoF");
      B.b_id[e] = o.b_id[B.perm[e]];
      /* ids whose boundary condition reads the Dirichlet state (hyperbolic_system.h:1099-1159) */
      if (B.b_id[e] == RYUJIN_BC_DIRICHLET || B.b_id[e] == RYUJIN_BC_DYNAMIC ||
          B.b_id[e] == RYUJIN_BC_DIRICHLET_MOMENTUM)
        B.needs_dirichlet = true;
      if (e == 0 || B.b_i[e] != B.b_i[e - 1]) {
        B.grp_start.push_back(e);
        B.rows.push_back(B.b_i[e]);
      }
    }
    B.n_groups = (uint32_t)B.rows.size();
    B.grp_start.push_back(o.n_bdry);
    B.bc_mask.assign(L.n_slices, 0ull);
    B.bc_first.assign(L.n_slices, 0u);
    for (uint32_t g = B.n_groups; g-- > 0;) {
      B.bc_mask[B.rows[g] / kWave] |= 1ull << (B.rows[g] % kWave);
      B.bc_first[B.rows[g] / kWave] = g; /* descending loop: the smallest group of the slice wins */
    }
    return B;
  }

  /* coupling boundary pairs: the position of (p_i, p_col) in the device layout and the value of c_ji, [n_pairs][dim];
   * `cij`: SellLayout::scatter(o, o.cij, dim) */
  struct PairTables {
    std::vector<uint32_t> pos;
    std::vector<double> cji;
  };

  inline PairTables build_pair_tables(const ryujin_hip_offline &o, const SellLayout &L, const std::vector<double> &cij,
                                      const int dim)
  {
    PairTables P{std::vector<uint32_t>(o.n_pairs), std::vector<double>((size_t)o.n_pairs * dim)};
    for (uint32_t q = 0; q < o.n_pairs; ++q) {
      const uint64_t pos = L.pos(o.p_i[q], o.p_col[q]);
      if (L.cols[pos] != o.p_j[q])
        throw HipError(RYUJIN_ERR_ARG, "coupling_boundary_pairs do not match the sparsity pattern");
      P.pos[q] = (uint32_t)pos;
      for (int d = 0; d < dim; ++d)
        P.cji[(size_t)q * dim + d] = cij[L.comp_pos(L.idx_t[pos], (uint32_t)dim, (uint32_t)d)];
    }
    return P;
  }

  /* rows [0, n_export) are the ones other ranks hold as ghosts (offline_data.template.h:213-249): the slices they fill */
  inline uint32_t n_export_slices(const ryujin_hip_offline &o, const SellLayout &L)
  {
    return std::min<uint32_t>(L.n_slices, (o.n_export + kWave - 1) / kWave);
  }

  /* The overlap of the exchanges with the interior rows rests on: only export rows couple to ghost columns (true for
   * a symmetric stencil: if i sees the ghost j, the owner of j sees i). Checked, not assumed. */
  inline bool interior_rows_read_ghosts(const SellLayout &L, const uint32_t n_export_slices)
  {
    const uint32_t first = n_export_slices * kWave;
    if (L.n_owned <= first)
      return false;
    std::atomic<bool> found{false};
    parallel_chunks(L.n_owned - first, [&](const uint64_t i0, const uint64_t i1) {
      for (uint32_t i = first + (uint32_t)i0; i < first + (uint32_t)i1 && !found.load(std::memory_order_relaxed); ++i)
        for (uint32_t c = 0; c < L.row_len[i]; ++c)
          if (L.cols[L.pos(i, c)] >= L.n_owned) {
            found.store(true, std::memory_order_relaxed);
            break;
          }
    });
    return found.load();
  }

  /* What the launches take from the mesh (DeviceMesh). */
  struct MeshKnobs {
    uint32_t band_stride, xcd_chunk, tail_queue_columns, bounds_stride;
  };

  /* xcd_chunk_3d: the library's choice in 3-D (RYUJIN_XCD_CHUNK_3D); waves_per_block: kWavesPerBlock */
  inline MeshKnobs mesh_knobs(const ryujin_hip_params &p, const SellLayout &L, const int dim, const uint32_t xcd_chunk_3d,
                              const uint32_t waves_per_block)
  {
    MeshKnobs k{1u, 0u, 0u, 0u};
    /* stacked blocks (row_context(), kernels_euler.hpp): debug_band_stride < 0 off, > 0 that many slices, 0 from the
     * mesh, in 2-D: C2 (G = 47) -1.1 % per update, every sweep a little; in 3-D stacking lattice planes (G = 365 on the C4
     * share) LOSES 1.7 % and stacking lattice rows (G = 2) is noise -- the re-fetches of neighbour data across XCDs that
     * the counters show are not what limits the sweeps (profiles/r05p_ab_band_2d.log, r05p_ab_band_3d.log) */
    if (p.debug_band_stride > 0)
      k.band_stride = (uint32_t)p.debug_band_stride;
    else if (p.debug_band_stride == 0 && dim == 2) {
      const uint32_t G = (L.lattice_stride(dim) + kWave / 2) / kWave;
      if (G >= 2 && (uint64_t)G * waves_per_block * 4 <= L.n_slices)
        k.band_stride = G;
    }
    /* XCD-local block ranges (row_context()): debug_xcd_chunk < 0 off, > 0 that many blocks per XCD and chunk */
    if (p.debug_xcd_chunk > 0)
      k.xcd_chunk = (uint32_t)p.debug_xcd_chunk;
    else if (p.debug_xcd_chunk == 0 && dim == 3)
      k.xcd_chunk = xcd_chunk_3d;
    /* the queue of undecided pairs of k_pij_lij: (widest row - 1) columns, at most 63 */
    k.tail_queue_columns = std::max<uint32_t>(1u, std::min<uint32_t>(63u, L.max_row_len - 1u));
    /* SoA stride of the limiter bounds: covers the ghost range (dG reads bounds_j) */
    k.bounds_stride = (std::max<uint32_t>(L.rows_padded, L.n_relevant) + 63u) / 64u * 64u;
    return k;
  }

  /* The exchange pattern in the device layout; everything empty on a single rank. */
  struct ExchangeTables {
    int n_nbr = 0;
    std::vector<int> nbr_rank;                              /* [n_nbr] */
    std::vector<uint32_t> send_off, recv_off, row_send_off; /* [n_nbr + 1], as in the offline data */
    std::vector<uint32_t> row_send_pos; /* [row_send_off[n_nbr]] position of (row_send_row, row_send_col) */
    std::vector<uint64_t> row_recv_off; /* [n_nbr + 1] offsets into the ghost CSR region */
    size_t send_buffer_doubles = 0;     /* the widest vector exchange (KP or NPREC per row), or the matrix exchange */
  };

  inline ExchangeTables build_exchange_tables(const ryujin_hip_offline &o, const SellLayout &L, const int KP,
                                              const int NPREC)
  {
    ExchangeTables X;
    if (o.n_nbr <= 0)
      return X;
    const int n = X.n_nbr = o.n_nbr;
    X.nbr_rank.assign(o.nbr_rank, o.nbr_rank + n);
    X.send_off.assign(o.send_off, o.send_off + n + 1);
    X.recv_off.assign(o.recv_off, o.recv_off + n + 1);
    X.row_send_off.assign(o.row_send_off, o.row_send_off + n + 1);
    X.row_send_pos.resize(X.row_send_off[n]);
    for (uint32_t e = 0; e < X.row_send_off[n]; ++e)
      X.row_send_pos[e] = (uint32_t)L.pos(o.row_send_row[e], o.row_send_col[e]);
    X.row_recv_off.resize((size_t)n + 1);
    for (int q = 0; q <= n; ++q)
      X.row_recv_off[q] = L.ghost_ptr[X.recv_off[q] - L.n_owned];
    X.send_buffer_doubles = std::max<size_t>((size_t)X.send_off[n] * std::max(KP, NPREC), X.row_send_off[n]);
    return X;
  }
} // namespace ryujin_hip
