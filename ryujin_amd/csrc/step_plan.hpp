// Which kernels one update runs (ryujin_hip_ctx::step): decided once per update, here, from plain numbers. Host only --
// no HIP, no context -- so that the decision can be read and checked on a CPU (tests/cpp/step_plan_cases.cc walks the
// whole input lattice). step() launches what the plan names and decides nothing itself; the context keeps the plan of
// the latest update (last_plan) for the debug fetch, the statistics and the timers.
#ifndef RYUJIN_HIP_STEP_PLAN_HPP
#define RYUJIN_HIP_STEP_PLAN_HPP

#include <algorithm>
#include <cstdint>

namespace ryujin_hip
{
  enum class PlanEquation { euler, euler_aeos, scalar, shallow_water };

  constexpr uint32_t kPlanWavesPerBlock = 4; /* kWavesPerBlock of the kernels (ryujin_hip.hip asserts it) */

  /* columns of a Q1 stencil: the widest row the kernels with the row in registers / LDS take */
  constexpr int q1_stencil_width(const int dim) { return dim == 1 ? 3 : (dim == 2 ? 9 : 27); }

  struct StepPlanInput {
    PlanEquation equation = PlanEquation::euler;
    int dim = 1;
    bool fusable_precompute = false; /* E::kFusablePrecompute */
    int stages = 0, limiter_iterations = 2;
    bool dg = false;
    uint32_t max_row_len = 0, n_slices = 0;
    uint32_t n_export_slices = 0; /* a sweep on several ranks is two launches: [0, n_export_slices) and the rest */
    int debug_pij_storage = 0;
    int debug_next_tile_mask = 0; /* < 0: step 6 hands no tile mask to step 7; > 0: it does, and stores every zero */
    bool checked = false; /* debug_expensive_bounds_check */
    double limited_fraction = 1.;
    double per_slice_max_limited = 1.; /* RYUJIN_PER_SLICE_MAX_LIMITED (kernels_euler.hpp) */
    uint32_t resident_waves_step5 = 0, resident_waves_step6 = 0, bc_fold_max_slices = 0;
    bool pending_precompute = false;
    int riemann_newton_max_iterations = 0, rarefaction_power = 0; /* Euler */
    bool friction = false;                                        /* shallow water: manning != 0 */
  };

  struct StepPlan {
    int dim = 1;
    uint32_t resident_waves_step5 = 0, resident_waves_step6 = 0; /* for the two per-launch decisions below */
    /* step 2; `split`: event 8 is recorded behind the first kernel (sweep_ms[0]) */
    enum class Step2 {
      alpha_then_dij,  /* k_alpha_aeos + k_dij_aeos; Euler's general Riemann path: k_alpha + k_dij_records */
      dij_alpha_sc,    /* scalar conservation */
      records,         /* k_dij_alpha_records */
      dij_alpha        /* rows of more than 32 entries */
    } step2 = Step2::dij_alpha;
    bool step2_split = false;
    bool fast_riemann = false; /* Euler: no Newton iterations, integral rarefaction exponent */
    /* step 3: k_dij_diag_unrolled<3 | 9 | 27>, 0: k_dij_diag */
    int diag_width = 0;
    /* step 4: k_low_order_sw_single_walk<has_stages, friction> or k_low_order*<has_stages, stores_p, dg> */
    bool step4_single_walk = false, step4_has_stages = false, step4_friction = false, step4_stores_p = true;
    bool dg = false;
    enum class Step5 { none, stage0_per_tile, stage0_per_slice, stage0_groups, recompute, pij_lij } step5 = Step5::none;
    uint32_t step5_groups = 1; /* stage0_groups: waves per slice, 1..4 */
    bool wide = false;         /* rows of more than 64 entries (k_pij_lij, k_high_order) */
    bool has_V = false;        /* step 5 leaves V_i = U_i^low + sum_j lambda P_ij: step 6 may take it */
    int pij_stored = 1;        /* as ryujin_hip_limiter_statistics reports it: 1 everywhere, 2 per slice, 3 per tile */
    bool tiles_predicted_from_history = false;
    enum class Step6 { none, per_slice, cached, high_order } step6 = Step6::none;
    bool step6_flags = false; /* step 6 leaves SliceFlags::unlimited for every slice: the last sweep may use it */
    enum class Step7 { none, last_cached, high_order } step7 = Step7::none;
    /* step 6 leaves SliceFlags::next_tiles -- the (slice, column) tiles in which some pair is limited -- and step 7 reads
     * l'_ij, l'_ji and the descriptors of those tiles only (kernels_limiter.hpp). The single-launch cached step 6 with
     * one wave per slice in EVERY launch of the sweep, up to two dimensions, in front of the cached step 7, unchecked */
    bool next_tile_mask = false;
    /* ... and step 6 does not store the zeros of the tiles outside the mask (outside the export slices) */
    bool next_tiles_elided = false;
    bool fuse_precompute = false;
    bool checked = false;
    /* refusals: what step() throws as RYUJIN_ERR_UNSUPPORTED / as an internal error (nullptr: none) */
    const char *unsupported = nullptr, *violated = nullptr;

    bool per_slice() const { return pij_stored == 2; }
    bool per_tile() const { return pij_stored == 3; }

    /* The two decisions that depend on the size of the individual launch (the export and the interior part of a split
     * sweep differ). k_pij_lij_recompute on small meshes: up to four waves per slice, each taking a share of the
     * columns (see the kernel), as long as all of them are resident at once (256 CUs x 4 SIMDs x 2 waves of this
     * kernel) */
    uint32_t recompute_groups(const uint32_t grid_x) const
    {
      return std::min(4u, std::max(1u, resident_waves_step5 / std::max(1u, grid_x * kPlanWavesPerBlock)));
    }
    /* step 6 on small meshes, up to two dimensions: the four waves of a block share one slice (see the kernel) while
     * all of them fit. (Not with P_ij stored per tile: the export part of a large mesh may be this small, and the split
     * variant does not form the tiles step 5 left out.) */
    bool step6_shares_slices(const uint32_t n_launch_slices) const
    {
      return step6 == Step6::cached && dim <= 2 && !per_tile() &&
             n_launch_slices * kPlanWavesPerBlock <= resident_waves_step6;
    }
  };

  /* the launches of a sweep (ryujin_hip_ctx::sweep): the export part and the interior part, or the whole mesh */
  inline bool some_launch_shares_slices(const StepPlan &p, const uint32_t n_slices, const uint32_t n_export_slices)
  {
    const uint32_t n_export = std::min(n_export_slices, n_slices);
    return (n_export != 0 && p.step6_shares_slices(n_export)) ||
           (n_slices > n_export && p.step6_shares_slices(n_slices - n_export));
  }

  /* what the tile mask relies on (nullptr: nothing violated): every launch of step 6 is the single-launch cached kernel
   * with one wave per slice, which writes the mask; step 7 is the cached kernel, which reads it; the checked kernels
   * read the whole second-pass matrix */
  inline const char *next_tile_mask_violated(const StepPlan &p, const uint32_t n_slices, const uint32_t n_export_slices)
  {
    if (!p.next_tile_mask)
      return p.next_tiles_elided ? "step plan: zeros are elided under the tile mask only" : nullptr;
    if (p.step6 != StepPlan::Step6::cached || p.dim > 2)
      return "step plan: the tile mask needs the single-launch cached step 6, dim <= 2";
    if (some_launch_shares_slices(p, n_slices, n_export_slices))
      return "step plan: the tile mask needs one wave per slice in every launch of step 6";
    if (p.step7 != StepPlan::Step7::last_cached)
      return "step plan: the tile mask needs the cached step 7";
    if (p.checked)
      return "step plan: the checked kernels read all of l_ij";
    return nullptr;
  }

  inline StepPlan plan_step(const StepPlanInput &in)
  {
    const bool is_euler = in.equation == PlanEquation::euler, is_aeos = in.equation == PlanEquation::euler_aeos;
    const bool is_scalar = in.equation == PlanEquation::scalar, is_sw = in.equation == PlanEquation::shallow_water;
    const int n_iterations = in.limiter_iterations;
    const uint32_t q1_width = (uint32_t)q1_stencil_width(in.dim);
    StepPlan p;
    p.dim = in.dim;
    p.resident_waves_step5 = in.resident_waves_step5;
    p.resident_waves_step6 = in.resident_waves_step6;
    p.checked = in.checked;
    p.dg = in.dg;
    p.wide = in.max_row_len > 64;

    /* Step 2 */
    p.fast_riemann = is_euler && in.riemann_newton_max_iterations == 0 && in.rarefaction_power > 0;
    if (is_aeos) {
      if (in.max_row_len > 32)
        p.unsupported = "euler aeos: stencils of more than 32 entries";
      p.step2 = StepPlan::Step2::alpha_then_dij;
    } else if (is_scalar)
      p.step2 = StepPlan::Step2::dij_alpha_sc;
    else if ((p.fast_riemann || is_sw) && in.max_row_len <= 32)
      p.step2 = StepPlan::Step2::records;
    else if (is_euler && in.max_row_len <= 32)
      /* (Euler's general Riemann path -- Newton iterations or a non-integral exponent -- holds twice the registers
       * and keeps the two-kernel form: the indicator sweep and the Riemann sweep) */
      p.step2 = StepPlan::Step2::alpha_then_dij;
    else
      p.step2 = StepPlan::Step2::dij_alpha;
    p.step2_split = p.step2 == StepPlan::Step2::alpha_then_dij || p.step2 == StepPlan::Step2::dij_alpha_sc;

    /* Step 3 */
    p.diag_width = in.max_row_len <= 3 ? 3 : (in.max_row_len <= 9 ? 9 : (in.max_row_len <= 27 ? 27 : 0));

    /* Euler, stages == 0, limiter on: P_ij (part 1) is recomputed in step 5 instead of stored in step 4.
     * A/B on MI355X: -7 % per update in 2-D (k=4, 9 columns). In 3-D (k=5, 27 columns) step 4 drops from 2.01
     * to 1.34 ms on 4.2 M gridpoints but step 5 grows from 2.16 to 2.77-2.94 ms (27 flux evaluations per row at
     * 240 registers): -0.7 % ... +1.5 % per update, inside the run-to-run spread -- so only for dim <= 2.
     * Rows of at most 64 entries: k_pij_lij_recompute keeps the undecided pairs of a row in ONE 64-bit mask indexed by
     * the column (wider rows take k_pij_lij<WIDE>, which walks the columns in blocks of 63). */
    const bool recompute_p =
        is_euler && in.dim <= 2 && in.stages == 0 && n_iterations != 0 && !in.dg && in.max_row_len <= 64;
    /* Euler and EulerAEOS, stages == 0, Q1 stencil widths: step 4 does not touch P_ij; step 5 forms it once from
     * d_ij, m_ij and the per-node vectors, limits it and stores it for steps 6 and 7 (kernels_limiter_stage0.hpp)
     * -- any dimension */
    const bool stage0_pij =
        (is_euler || is_aeos) && in.stages == 0 && n_iterations != 0 && !in.dg && in.max_row_len <= q1_width;

    /* Step 4. Shallow water, rows of at most 3 / 9 columns (1-D, 2-D Q1): one walk over the stencil, the shift-free
     * part of the limiter's U_ij_bar parked in LDS (kernels_shallow_water.hpp); wider rows: the two walks of the
     * reference. Otherwise the kernel of the Description with stage vectors, the first part of P_ij stored (Euler,
     * EulerAEOS) -- unless step 5 forms it (recompute_p, stage0_pij) --, dG */
    p.step4_single_walk = is_sw && !in.dg && in.max_row_len <= (uint32_t)(in.dim == 1 ? 3 : 9);
    p.step4_has_stages = in.stages != 0;
    p.step4_friction = is_sw && in.friction;
    p.step4_stores_p = !(recompute_p || stage0_pij);

    /* step 5 on small meshes: up to four waves per slice, each taking a share of the columns (decided for the whole
     * mesh, not per launch: the export and the interior part of a split sweep must agree on whether V_i exists) */
    const uint32_t step5_groups = std::min<uint32_t>(
        4u, in.resident_waves_step5 /
                std::max<uint32_t>(1u, (in.n_slices + kPlanWavesPerBlock - 1) / kPlanWavesPerBlock * kPlanWavesPerBlock));
    /* WHERE STEP 5 STORES P_ij, only where steps 6 and 7 will read it (kernels_limiter_stage0.hpp): where the update has
     * two limiter passes and one wave per slice, and not in the checked build (its kernels read all of P_ij). Same bits
     * in every case. debug_pij_storage (create() refuses other values): 0 the default; 1 per slice, nothing predicted;
     * 2 per tile with nothing predicted (tests: every tile the neighbour's l_ji limits goes through step 6's repair), per
     * slice as 1 in 3-D; < 0 everywhere, as rounds 1 - 4.
     *   PER TILE, up to two dimensions: step 5 stores a (slice, column) tile iff one of its own l_ij comes out limited
     *   or step 6 read the tile in one of the last updates (SliceFlags::needed_tiles); step 6 -- one launch, the plain
     *   kernel -- forms the few tiles that are limited through the neighbour's l_ji alone and were not predicted
     *   (kernels_limiter_stage0.hpp, next_cached_slice). On the Mach-3 step a third to 45 % of the tiles are stored
     *   where 71 - 93 % of the slices would be, and the update is faster than with either alternative at every stage of
     *   the flow (profiles/r05t_ab_tile_*). (In 3-D per tile was measured as a loss and retired: DESIGN_HISTORY.md.)
     *   PER SLICE (3-D; debug_pij_storage = 1 in any dimension): WHILE that pays. Its bookkeeping (the prediction and
     *   the trigger in step 5, step 6 as three launches) costs a few per cent of the three sweeps, the savings are
     *   proportional to the share of unlimited slices. Above RYUJIN_PER_SLICE_MAX_LIMITED (the measured break-even,
     *   profiles/r04*_ab_limited_fraction*) the plain kernels run: P_ij stored EVERYWHERE, step 6 in one launch. The
     *   fraction is the one step 6 counted between the two latest host synchronisations (1 until the first: the first
     *   update of a context runs the plain kernels). */
    const int storage = in.debug_pij_storage;
    const bool selective = stage0_pij && n_iterations == 2 && step5_groups < 2 && storage >= 0 && !in.checked;
    const bool tile_store = in.dim <= 2 && selective && storage != 1;
    const bool per_slice =
        selective && !tile_store && (storage != 0 || in.limited_fraction <= in.per_slice_max_limited);
    p.pij_stored = per_slice ? 2 : (tile_store ? 3 : 1);
    p.tiles_predicted_from_history = tile_store && storage == 0;

    /* Step 5. V_i exists where the update has two limiter passes (d_V is allocated exactly then) and the kernel
     * writes it: k_pij_lij always, k_lij_stage0 with one wave per slice, k_pij_lij_recompute never */
    const bool two_passes = n_iterations == 2;
    if (n_iterations == 0)
      p.step5 = StepPlan::Step5::none;
    else if (stage0_pij) {
      p.step5 = tile_store ? StepPlan::Step5::stage0_per_tile
                           : (per_slice ? StepPlan::Step5::stage0_per_slice : StepPlan::Step5::stage0_groups);
      p.step5_groups = (tile_store || per_slice) ? 1u : std::max(1u, step5_groups);
      p.has_V = two_passes && p.step5_groups == 1;
    } else if (recompute_p)
      p.step5 = StepPlan::Step5::recompute;
    else {
      p.step5 = StepPlan::Step5::pij_lij;
      p.has_V = two_passes;
    }

    /* Steps 6 (the first of two limiter passes) and 7 (the last pass). Per slice, step 6 is three launches over all
     * slices: the light one finishes the slices without a stored P_ij in which nothing was limited (V_i), the repair
     * launch completes the P_ij of the slices that turned out limited without (all of) it, the heavy one runs the
     * limited slices (kernels_limiter.hpp). With P_ij stored per tile the plain cached kernel forms the tiles step 5
     * left out (forms_missing_tiles). */
    const bool cached = in.max_row_len <= q1_width;
    if (two_passes) {
      p.step6 = per_slice ? StepPlan::Step6::per_slice : (cached ? StepPlan::Step6::cached : StepPlan::Step6::high_order);
      p.step6_flags = per_slice || (cached && p.has_V);
    }
    if (n_iterations != 0)
      p.step7 = cached ? StepPlan::Step7::last_cached : StepPlan::Step7::high_order;

    /* The tile mask from step 6 to step 7. Whether the waves of a block share a slice is decided per launch
     * (step6_shares_slices), and the sharing variant writes no mask: none of the sweep's launches may take it. */
    p.next_tile_mask = in.debug_next_tile_mask >= 0 && p.step6 == StepPlan::Step6::cached && in.dim <= 2 &&
                       !some_launch_shares_slices(p, in.n_slices, in.n_export_slices) &&
                       p.step7 == StepPlan::Step7::last_cached && !in.checked;
    p.next_tiles_elided = p.next_tile_mask && in.debug_next_tile_mask == 0;

    /* the last sweep leaves the precomputed values and Riemann records of the new vector, where the next pre-pass
     * would be a sweep of its own (large meshes: below bc_fold_max_slices the boundary conditions ride on that sweep) */
    p.fuse_precompute = in.fusable_precompute && in.pending_precompute && n_iterations != 0 &&
                        in.n_slices > in.bc_fold_max_slices && cached;

    /* what the kernels rely on (step 6 reads V_i and, per tile, forms missing tiles with one wave per slice; the
     * checked kernels read all of P_ij) */
    if (p.per_tile() && !(p.has_V && p.step5 == StepPlan::Step5::stage0_per_tile && p.step5_groups == 1 && in.dim <= 2))
      p.violated = "step plan: P_ij per tile needs V_i, one wave per slice and dim <= 2";
    else if (p.per_slice() && !(p.has_V && p.step5 == StepPlan::Step5::stage0_per_slice))
      p.violated = "step plan: P_ij per slice needs V_i";
    else if (p.wide && p.step5 != StepPlan::Step5::none && p.step5 != StepPlan::Step5::pij_lij)
      p.violated = "step plan: rows of more than 64 entries need k_pij_lij<WIDE> in step 5";
    else if (p.checked && p.pij_stored != 1)
      p.violated = "step plan: the checked kernels read all of P_ij";
    else if (const char *v = next_tile_mask_violated(p, in.n_slices, in.n_export_slices))
      p.violated = v;
    return p;
  }
} // namespace ryujin_hip

#endif
