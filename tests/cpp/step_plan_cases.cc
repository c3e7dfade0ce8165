// CPU check of the step plan (ryujin_amd/csrc/step_plan.hpp): which kernels an update runs.
//   step_plan_cases lattice     the invariants the kernels rely on, over the whole input lattice: JSON with the number of
//                               plans, the violations and how often each variant occurred
//   step_plan_cases path equation dim max_row_len n_slices limited_fraction [resident_waves5 resident_waves6 fold]
//                               the kernel path of one configuration (defaults of create()) as JSON: one name per launch
//                               of a one-launch sweep, as rocprofv3 prints it
//   step_plan_cases plan equation dim max_row_len n_slices limited_fraction stages [n_launch_slices ...] [key=1 ...]
//                               every field of the plan of one configuration (defaults of create(), a step() outside
//                               the device-resident driver: no pending pre-pass) under the names of
//                               HyperbolicModule.last_plan(), and per given launch size what the sweeps of steps 5
//                               and 6 make of it: gridDim.y of step 5, whether step 6 shares slices. Options:
//                               newton=N (riemann_newton_max_iterations), checked=1 (debug_expensive_bounds_check),
//                               friction=1 (a Manning coefficient), no_split=1 (debug_no_small_mesh_split),
//                               dg=1 (the discontinuous ansatz)
// (test infrastructure; built by tests/test_step_plan.py)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "step_plan.hpp"

using namespace ryujin_hip;
using Step5 = StepPlan::Step5;
using Step6 = StepPlan::Step6;

namespace
{
  const char *b(const bool v) { return v ? "true" : "false"; }

  std::string equation_name(const PlanEquation e, const int dim)
  {
    const char *n = e == PlanEquation::euler ? "Euler"
                                             : (e == PlanEquation::euler_aeos
                                                    ? "EulerAeos"
                                                    : (e == PlanEquation::scalar ? "ScalarConservation" : "ShallowWater"));
    return std::string(n) + "<" + std::to_string(dim) + ">";
  }

  /* the kernels of steps 2 - 7 on a mesh of one part (every sweep one launch of n_slices slices) */
  std::vector<std::string> kernel_path(const StepPlanInput &in, const StepPlan &p)
  {
    const std::string E = equation_name(in.equation, in.dim), D = std::to_string(in.dim);
    const std::string W = std::to_string(q1_stencil_width(in.dim));
    const bool is_euler = in.equation == PlanEquation::euler, is_aeos = in.equation == PlanEquation::euler_aeos;
    std::vector<std::string> k;
    switch (p.step2) {
    case StepPlan::Step2::alpha_then_dij:
      if (is_aeos) {
        k.push_back("k_alpha_aeos<" + D + ">");
        k.push_back("k_dij_aeos<" + D + ">");
      } else {
        k.push_back("k_alpha<" + E + " >");
        k.push_back("k_dij_records<" + E + ", " + b(!p.fast_riemann) + ">");
      }
      break;
    case StepPlan::Step2::dij_alpha_sc: k.push_back("k_dij_alpha_sc<" + D + ">"); break;
    case StepPlan::Step2::records: k.push_back("k_dij_alpha_records<" + E + ", false>"); break;
    case StepPlan::Step2::dij_alpha: k.push_back("k_dij_alpha<" + E + " >"); break;
    }
    k.push_back(p.diag_width ? "k_dij_diag_unrolled<" + std::to_string(p.diag_width) + ">" : "k_dij_diag");
    if (p.step4_single_walk)
      k.push_back("k_low_order_sw_single_walk<" + D + ", " + b(p.step4_has_stages) + ", " + (in.dim == 1 ? "3" : "9") +
                  ", " + b(p.step4_friction) + ">");
    else if (is_euler || is_aeos)
      k.push_back(std::string(is_euler ? "k_low_order<" : "k_low_order_aeos<") + D + ", " + b(p.step4_has_stages) +
                  ", " + b(p.step4_stores_p) + ", " + b(p.dg) + ">");
    else
      k.push_back(std::string(in.equation == PlanEquation::scalar ? "k_low_order_sc<" : "k_low_order_sw<") + D + ", " +
                  b(p.step4_has_stages) + ", " + b(p.dg) + ">");
    const uint32_t grid_x = (in.n_slices + kPlanWavesPerBlock - 1) / kPlanWavesPerBlock;
    switch (p.step5) {
    case Step5::none: break;
    case Step5::stage0_per_tile: k.push_back("k_lij_stage0<" + E + ", 1, false, true>"); break;
    case Step5::stage0_per_slice: k.push_back("k_lij_stage0<" + E + ", 1, true, false>"); break;
    case Step5::stage0_groups:
      k.push_back("k_lij_stage0<" + E + ", " + std::to_string(p.step5_groups) + ", false, false>");
      break;
    case Step5::recompute:
      k.push_back("k_pij_lij_recompute<" + D + ", " + std::to_string(p.recompute_groups(grid_x)) + ">");
      break;
    case Step5::pij_lij: k.push_back("k_pij_lij<" + E + ", " + b(p.dg) + ", " + b(p.wide) + ">"); break;
    }
    const std::string CP = in.dim == 3 ? "2" : W; /* RYUJIN_HO_CP_3D; in 2-D RYUJIN_HO_CP_2D is the full width */
    switch (p.step6) {
    case Step6::none: break;
    case Step6::per_slice:
      k.push_back("k_high_order_next_cached<" + E + ", " + W + ", " + CP + ", false, 1>");
      k.push_back("k_pij_repair<" + E + " >");
      k.push_back("k_high_order_next_cached<" + E + ", " + W + ", " + CP + ", false, 2>");
      break;
    case Step6::cached:
      if (p.step6_shares_slices(in.n_slices))
        k.push_back("k_high_order_next_cached<" + E + ", " + W + ", " + W + ", true, 0>");
      else
        k.push_back("k_high_order_next_cached<" + E + ", " + W + ", " + CP + ", false, 0>");
      break;
    case Step6::high_order: k.push_back("k_high_order<" + E + ", false, " + b(p.wide) + ">"); break;
    }
    if (p.step7 == StepPlan::Step7::last_cached)
      k.push_back("k_high_order_last_cached<" + E + ", " + W + ", 3>");
    else if (p.step7 == StepPlan::Step7::high_order)
      k.push_back("k_high_order<" + E + ", true, false>");
    return k;
  }

  /* the inputs of a context created with the defaults of create() and of ryujin_hip_default_params (gamma = 7/5:
   * rarefaction exponent 7) */
  StepPlanInput default_input(char **argv)
  {
    StepPlanInput in;
    const std::string eq = argv[2];
    in.equation = eq == "euler" ? PlanEquation::euler
                                : (eq == "euler_aeos" ? PlanEquation::euler_aeos
                                                      : (eq == "scalar" ? PlanEquation::scalar : PlanEquation::shallow_water));
    in.dim = std::atoi(argv[3]);
    in.max_row_len = (uint32_t)std::atoi(argv[4]);
    in.n_slices = (uint32_t)std::atoll(argv[5]);
    in.limited_fraction = std::atof(argv[6]);
    in.resident_waves_step5 = 2048u;
    in.resident_waves_step6 = 4096u;
    in.bc_fold_max_slices = 4096u;
    in.per_slice_max_limited = 0.8;
    in.fusable_precompute = in.equation == PlanEquation::euler || in.equation == PlanEquation::shallow_water;
    in.rarefaction_power = 7;
    return in;
  }

  int run_path(int argc, char **argv)
  {
    if (argc < 7)
      return 2;
    StepPlanInput in = default_input(argv);
    if (argc > 7)
      in.resident_waves_step5 = (uint32_t)std::atoi(argv[7]);
    if (argc > 8)
      in.resident_waves_step6 = (uint32_t)std::atoi(argv[8]);
    if (argc > 9)
      in.bc_fold_max_slices = (uint32_t)std::atoi(argv[9]);
    in.pending_precompute = true; /* a stage of the device-resident SSPRK33 driver */
    const StepPlan p = plan_step(in);
    if (p.unsupported || p.violated) {
      std::fprintf(stderr, "%s\n", p.unsupported ? p.unsupported : p.violated);
      return 1;
    }
    std::printf("{\"pij_stored\": %d, \"has_V\": %s, \"fuse_precompute\": %s, \"kernels\": [", p.pij_stored, b(p.has_V),
                b(p.fuse_precompute));
    const auto k = kernel_path(in, p);
    for (size_t i = 0; i < k.size(); ++i)
      std::printf("%s\"%s\"", i ? ", " : "", k[i].c_str());
    std::printf("]}\n");
    return 0;
  }

  int run_plan(int argc, char **argv)
  {
    if (argc < 8)
      return 2;
    StepPlanInput in = default_input(argv);
    in.stages = std::atoi(argv[7]);
    std::vector<const char *> sizes;
    for (int q = 8; q < argc; ++q) {
      const char *eq = std::strchr(argv[q], '=');
      if (eq == nullptr) {
        sizes.push_back(argv[q]);
        continue;
      }
      const std::string key(argv[q], eq - argv[q]);
      const int value = std::atoi(eq + 1);
      if (key == "newton")
        in.riemann_newton_max_iterations = value;
      else if (key == "checked")
        in.checked = value != 0;
      else if (key == "friction")
        in.friction = value != 0;
      else if (key == "dg")
        in.dg = value != 0;
      else if (key == "no_split") {
        if (value != 0)
          in.resident_waves_step5 = in.resident_waves_step6 = 0; /* as create() */
      } else
        return 2;
    }
    const StepPlan p = plan_step(in);
    if (p.unsupported || p.violated) {
      std::fprintf(stderr, "%s\n", p.unsupported ? p.unsupported : p.violated);
      return 1;
    }
    const char *step2[] = {"alpha_then_dij", "dij_alpha_sc", "records", "dij_alpha"};
    const char *step5[] = {"none", "stage0_per_tile", "stage0_per_slice", "stage0_groups", "recompute", "pij_lij"};
    const char *step6[] = {"none", "per_slice", "cached", "high_order"};
    const char *step7[] = {"none", "last_cached", "high_order"};
    std::printf("{\"step2\": \"%s\", \"step2_split\": %s, \"fast_riemann\": %s, \"diag_width\": %d, "
                "\"step4_single_walk\": %s, \"step4_has_stages\": %s, \"step4_friction\": %s, \"step4_stores_p\": %s, "
                "\"dg\": %s, \"step5\": \"%s\", \"step5_groups\": %u, \"wide\": %s, \"has_V\": %s, \"pij_stored\": %d, "
                "\"tiles_predicted_from_history\": %s, \"step6\": \"%s\", \"step6_flags\": %s, \"step7\": \"%s\", "
                "\"fuse_precompute\": %s, \"checked\": %s, \"launches\": [",
                step2[(int)p.step2], b(p.step2_split), b(p.fast_riemann), p.diag_width, b(p.step4_single_walk),
                b(p.step4_has_stages), b(p.step4_friction), b(p.step4_stores_p), b(p.dg), step5[(int)p.step5],
                p.step5_groups, b(p.wide), b(p.has_V), p.pij_stored, b(p.tiles_predicted_from_history),
                step6[(int)p.step6], b(p.step6_flags), step7[(int)p.step7], b(p.fuse_precompute), b(p.checked));
    for (size_t q = 0; q < sizes.size(); ++q) {
      const uint32_t n_launch = (uint32_t)std::atoll(sizes[q]);
      const uint32_t grid_x = (n_launch + kPlanWavesPerBlock - 1) / kPlanWavesPerBlock;
      /* gridDim.y of the step-5 launch (step5_limiter in ryujin_hip.hip): the waves that share a slice */
      const uint32_t grid_y = p.step5 == Step5::stage0_groups
                                  ? p.step5_groups
                                  : (p.step5 == Step5::recompute ? p.recompute_groups(grid_x) : 1u);
      std::printf("%s{\"n_slices\": %u, \"step5_grid_y\": %u, \"recompute_groups\": %u, \"step6_shares_slices\": %s}",
                  q > 0 ? ", " : "", n_launch, grid_y, p.recompute_groups(grid_x), b(p.step6_shares_slices(n_launch)));
    }
    std::printf("]}\n");
    return 0;
  }

  int run_lattice()
  {
    const struct {
      PlanEquation e;
      int dim;
    } pairs[11] = {{PlanEquation::euler, 1},      {PlanEquation::euler, 2},         {PlanEquation::euler, 3},
                   {PlanEquation::euler_aeos, 1}, {PlanEquation::euler_aeos, 2},    {PlanEquation::euler_aeos, 3},
                   {PlanEquation::scalar, 1},     {PlanEquation::scalar, 2},        {PlanEquation::scalar, 3},
                   {PlanEquation::shallow_water, 1}, {PlanEquation::shallow_water, 2}};
    const uint32_t widths[] = {3, 9, 27, 33, 65};
    /* resident_waves_step5 = 2048: 4 waves per slice up to 512 slices, 3 up to 680, 2 up to 1024, then 1;
     * bc_fold_max_slices = 600 */
    const uint32_t slices[] = {5, 100, 512, 513, 600, 601, 680, 684, 1024, 1025, 5000};
    const int storages[] = {-1, 0, 1, 2};
    const double fractions[] = {0.1, 0.8, 0.81, 1.0};
    unsigned long long n = 0, bad = 0, refused = 0;
    std::map<std::string, unsigned long long> seen;
    std::string first_bad;
    auto fail = [&](const char *what) {
      if (!bad++)
        first_bad = what;
    };
    for (const auto &pr : pairs)
      for (int stages = 0; stages <= 2; ++stages)
        for (int iterations = 0; iterations <= 2; ++iterations)
          for (int dg = 0; dg <= 1; ++dg)
            for (const uint32_t width : widths)
              for (const uint32_t n_slices : slices)
                for (const int storage : storages)
                  for (int checked = 0; checked <= 1; ++checked)
                    for (const double fraction : fractions)
                      for (int pending = 0; pending <= 1; ++pending)
                        for (int newton = 0; newton <= 1; ++newton) { /* Euler's Riemann path, shallow water's friction */
                          StepPlanInput in;
                          in.equation = pr.e;
                          in.dim = pr.dim;
                          in.fusable_precompute = pr.e == PlanEquation::euler || pr.e == PlanEquation::shallow_water;
                          in.stages = stages;
                          in.limiter_iterations = iterations;
                          in.dg = dg != 0;
                          in.max_row_len = width;
                          in.n_slices = n_slices;
                          in.debug_pij_storage = storage;
                          in.checked = checked != 0;
                          in.limited_fraction = fraction;
                          in.per_slice_max_limited = 0.8;
                          in.resident_waves_step5 = 2048;
                          in.resident_waves_step6 = 4096;
                          in.bc_fold_max_slices = 600;
                          in.pending_precompute = pending != 0;
                          in.riemann_newton_max_iterations = newton;
                          in.rarefaction_power = 7;
                          in.friction = newton != 0;
                          const StepPlan p = plan_step(in);
                          ++n;
                          const bool is_aeos = pr.e == PlanEquation::euler_aeos;
                          if ((p.unsupported != nullptr) != (is_aeos && width > 32))
                            fail("EulerAEOS with rows of more than 32 entries is refused, and nothing else");
                          if (p.unsupported) {
                            ++refused;
                            continue;
                          }
                          if (p.violated)
                            fail(p.violated);
                          const bool stage0 = p.step5 == Step5::stage0_per_tile || p.step5 == Step5::stage0_per_slice ||
                                              p.step5 == Step5::stage0_groups;
                          const uint32_t ny = p.step5 == Step5::stage0_groups ? p.step5_groups : 1u;
                          if (p.pij_stored < 1 || p.pij_stored > 3 || ny < 1 || ny > 4)
                            fail("range");
                          if (p.per_tile() && !(p.has_V && ny == 1 && in.dim <= 2 && p.step5 == Step5::stage0_per_tile))
                            fail("per tile implies V_i, one wave per slice, dim <= 2 and the stage-0 kernel");
                          if (p.per_slice() && !(p.has_V && p.step5 == Step5::stage0_per_slice))
                            fail("per slice implies V_i and the stage-0 kernel");
                          if ((p.step5 == Step5::stage0_per_tile) != p.per_tile() ||
                              (p.step5 == Step5::stage0_per_slice) != p.per_slice())
                            fail("the step-5 kernel and the storage mode agree");
                          if (in.checked && p.pij_stored != 1)
                            fail("the checked build stores P_ij everywhere");
                          if (p.wide && !(p.step5 == Step5::none || p.step5 == Step5::pij_lij))
                            fail("rows of more than 64 entries take k_pij_lij<WIDE>, the one step-5 kernel with blocks");
                          if (p.tiles_predicted_from_history && !p.per_tile())
                            fail("tiles are predicted only where they are stored per tile");
                          if (p.step4_stores_p != !(p.step5 == Step5::recompute || stage0))
                            fail("step 4 stores its part of P_ij exactly when step 5 neither recomputes nor forms it");
                          if (!p.step4_stores_p && (p.step4_has_stages || p.dg))
                            fail("k_low_order<.., stores_p = false> exists without stages and dG only");
                          if (p.has_V && !(iterations == 2 && (p.step5 == Step5::pij_lij || (stage0 && ny == 1))))
                            fail("V_i exists only where two passes run and the step-5 kernel writes it");
                          if ((p.step6 != Step6::none) != (iterations == 2) ||
                              (p.step7 != StepPlan::Step7::none) != (iterations != 0) ||
                              (p.step5 != Step5::none) != (iterations != 0))
                            fail("sweeps and limiter passes");
                          if ((p.step6 == Step6::per_slice) != p.per_slice())
                            fail("step 6 runs as three launches exactly with P_ij per slice");
                          if (p.step6_flags && !(p.has_V && p.step6 != Step6::high_order && p.step6 != Step6::none))
                            fail("step 6 leaves the unlimited flags only from V_i");
                          for (const uint32_t part : {1u, 7u, 1024u, 1025u, n_slices})
                            if (p.step6_shares_slices(part) && (p.per_tile() || p.per_slice() || in.dim > 2 || width > 9))
                              fail("the slice-sharing step 6 never goes with per-tile (or per-slice) storage, 3-D or wide rows");
                          for (const uint32_t gx : {1u, 128u, 171u, 256u, 257u, 4000u})
                            if (p.recompute_groups(gx) < 1 || p.recompute_groups(gx) > 4)
                              fail("recompute groups");
                          if (p.fuse_precompute && !(in.fusable_precompute && pending && iterations != 0 &&
                                                     n_slices > 600 && p.step7 == StepPlan::Step7::last_cached))
                            fail("fused pre-pass");
                          ++seen["pij_stored_" + std::to_string(p.pij_stored)];
                          ++seen["step5_" + std::to_string((int)p.step5)];
                          if (p.step5 == Step5::stage0_groups)
                            ++seen["stage0_groups_" + std::to_string(p.step5_groups)];
                          ++seen["step6_" + std::to_string((int)p.step6)];
                          if (p.step6_shares_slices(n_slices))
                            ++seen["step6_shares_slices"];
                          if (p.fuse_precompute)
                            ++seen["fuse_precompute"];
                          if (p.has_V)
                            ++seen["has_V"];
                        }
    std::printf("{\"plans\": %llu, \"refused\": %llu, \"violations\": %llu, \"first\": \"%s\"", n, refused, bad,
                first_bad.c_str());
    for (const auto &s : seen)
      std::printf(", \"%s\": %llu", s.first.c_str(), s.second);
    std::printf("}\n");
    return bad == 0 ? 0 : 1;
  }
} // namespace

int main(int argc, char **argv)
{
  if (argc >= 2 && !std::strcmp(argv[1], "lattice"))
    return run_lattice();
  if (argc >= 2 && !std::strcmp(argv[1], "path"))
    return run_path(argc, argv);
  if (argc >= 2 && !std::strcmp(argv[1], "plan"))
    return run_plan(argc, argv);
  return 2;
}
