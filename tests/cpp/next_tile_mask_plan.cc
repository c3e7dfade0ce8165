// CPU check of the tile mask in the step plan (ryujin_amd/csrc/step_plan.hpp, StepPlan::next_tile_mask): step 6 hands
// its mask of limited tiles to step 7 exactly where every launch of step 6 is the single-launch cached kernel with one
// wave per slice, step 7 is the cached kernel and the run is not checked; with the switch at its default step 6 then
// does not store the zeros of the other tiles (next_tiles_elided).
//   next_tile_mask_plan plan equation dim max_row_len n_slices n_export_slices limited_fraction stages [key=value ...]
//                          the boolean of one configuration (defaults of create()) as JSON, with the inputs it has to
//                          follow from. Options: checked=1, no_split=1, dg=1, mask=-1 | 1 (debug_next_tile_mask),
//                          storage=N (debug_pij_storage), iterations=N
//   next_tile_mask_plan lattice
//                          the boolean against its definition, written out here once more, over the input lattice of
//                          step_plan_cases.cc extended by the switch and by split sweeps; no plan is violated
//   next_tile_mask_plan forced
//                          the boolean forced on in plans that must not carry it: every one is refused
// (test infrastructure; built by tests/test_step_plan_next_tile_mask.py)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "step_plan.hpp"

using namespace ryujin_hip;
using Step6 = StepPlan::Step6;
using Step7 = StepPlan::Step7;

namespace
{
  const char *b(const bool v) { return v ? "true" : "false"; }

  /* the definition: the launches of a sweep are the export part and the rest, or the whole mesh */
  bool expected(const StepPlanInput &in, const StepPlan &p)
  {
    if (in.debug_next_tile_mask < 0 || p.step6 != Step6::cached || p.step7 != Step7::last_cached || in.checked ||
        in.dim > 2)
      return false;
    const uint32_t n_export = in.n_export_slices < in.n_slices ? in.n_export_slices : in.n_slices;
    const uint32_t parts[2] = {n_export, in.n_slices - n_export};
    for (const uint32_t part : parts)
      if (part != 0 && p.step6_shares_slices(part))
        return false;
    return true;
  }

  StepPlanInput default_input()
  {
    StepPlanInput in;
    in.resident_waves_step5 = 2048u;
    in.resident_waves_step6 = 4096u;
    in.bc_fold_max_slices = 4096u;
    in.per_slice_max_limited = 0.8;
    in.rarefaction_power = 7;
    return in;
  }

  int run_plan(int argc, char **argv)
  {
    if (argc < 9)
      return 2;
    StepPlanInput in = default_input();
    const std::string eq = argv[2];
    in.equation = eq == "euler" ? PlanEquation::euler
                                : (eq == "euler_aeos" ? PlanEquation::euler_aeos
                                                      : (eq == "scalar" ? PlanEquation::scalar : PlanEquation::shallow_water));
    in.fusable_precompute = in.equation == PlanEquation::euler || in.equation == PlanEquation::shallow_water;
    in.dim = std::atoi(argv[3]);
    in.max_row_len = (uint32_t)std::atoi(argv[4]);
    in.n_slices = (uint32_t)std::atoll(argv[5]);
    in.n_export_slices = (uint32_t)std::atoll(argv[6]);
    in.limited_fraction = std::atof(argv[7]);
    in.stages = std::atoi(argv[8]);
    for (int q = 9; q < argc; ++q) {
      const char *e = std::strchr(argv[q], '=');
      if (e == nullptr)
        return 2;
      const std::string key(argv[q], e - argv[q]);
      const int value = std::atoi(e + 1);
      if (key == "checked")
        in.checked = value != 0;
      else if (key == "dg")
        in.dg = value != 0;
      else if (key == "mask")
        in.debug_next_tile_mask = value;
      else if (key == "storage")
        in.debug_pij_storage = value;
      else if (key == "iterations")
        in.limiter_iterations = value;
      else if (key == "no_split") {
        if (value != 0)
          in.resident_waves_step5 = in.resident_waves_step6 = 0; /* as create() */
      } else if (key == "newton" || key == "friction") {
        /* (options of step_plan_cases.cc the boolean does not depend on) */
      } else
        return 2;
    }
    const StepPlan p = plan_step(in);
    if (p.unsupported || p.violated) {
      std::fprintf(stderr, "%s\n", p.unsupported ? p.unsupported : p.violated);
      return 1;
    }
    const uint32_t n_export = in.n_export_slices < in.n_slices ? in.n_export_slices : in.n_slices;
    std::printf("{\"next_tile_mask\": %s, \"next_tiles_elided\": %s, \"step6_cached\": %s, \"step7_last_cached\": %s, "
                "\"checked\": %s, \"export_shares_slices\": %s, \"interior_shares_slices\": %s}\n",
                b(p.next_tile_mask), b(p.next_tiles_elided), b(p.step6 == Step6::cached),
                b(p.step7 == Step7::last_cached), b(p.checked),
                b(n_export != 0 && p.step6_shares_slices(n_export)),
                b(in.n_slices > n_export && p.step6_shares_slices(in.n_slices - n_export)));
    return 0;
  }

  int run_lattice()
  {
    const struct {
      PlanEquation e;
      int dim;
    } pairs[11] = {{PlanEquation::euler, 1},         {PlanEquation::euler, 2},      {PlanEquation::euler, 3},
                   {PlanEquation::euler_aeos, 1},    {PlanEquation::euler_aeos, 2}, {PlanEquation::euler_aeos, 3},
                   {PlanEquation::scalar, 1},        {PlanEquation::scalar, 2},     {PlanEquation::scalar, 3},
                   {PlanEquation::shallow_water, 1}, {PlanEquation::shallow_water, 2}};
    const uint32_t widths[] = {3, 9, 27, 33, 65};
    const uint32_t slices[] = {5, 100, 1024, 1025, 1030, 2100, 5000};
    const uint32_t exports[] = {0, 6, 1024, 1025};
    const int storages[] = {-1, 0, 1, 2};
    unsigned long long n = 0, bad = 0, elided = 0, on = 0, on_split_sweep = 0, off_by_switch = 0, off_by_sharing = 0;
    std::string first_bad;
    auto fail = [&](const char *what) {
      if (!bad++)
        first_bad = what;
    };
    for (const auto &pr : pairs)
      for (int stages = 0; stages <= 1; ++stages)
        for (int iterations = 0; iterations <= 2; ++iterations)
          for (int dg = 0; dg <= 1; ++dg)
            for (const uint32_t width : widths)
              for (const uint32_t n_slices : slices)
                for (const uint32_t n_export : exports)
                  for (const int storage : storages)
                    for (int checked = 0; checked <= 1; ++checked)
                      for (int no_split = 0; no_split <= 1; ++no_split)
                        for (int mask = -1; mask <= 1; ++mask) {
                          StepPlanInput in = default_input();
                          in.equation = pr.e;
                          in.dim = pr.dim;
                          in.stages = stages;
                          in.limiter_iterations = iterations;
                          in.dg = dg != 0;
                          in.max_row_len = width;
                          in.n_slices = n_slices;
                          in.n_export_slices = n_export;
                          in.debug_pij_storage = storage;
                          in.checked = checked != 0;
                          in.limited_fraction = 0.5;
                          in.bc_fold_max_slices = 600;
                          in.debug_next_tile_mask = mask;
                          if (no_split)
                            in.resident_waves_step5 = in.resident_waves_step6 = 0;
                          const StepPlan p = plan_step(in);
                          if (p.unsupported)
                            continue;
                          ++n;
                          if (p.violated)
                            fail(p.violated);
                          if (p.next_tile_mask != expected(in, p))
                            fail("the boolean is its definition");
                          if (p.next_tiles_elided != (p.next_tile_mask && mask == 0))
                            fail("zeros are elided exactly under the mask with the switch at its default");
                          if (p.next_tiles_elided)
                            ++elided;
                          if (p.next_tile_mask) {
                            ++on;
                            if (n_export != 0 && n_export < n_slices)
                              ++on_split_sweep;
                            if (p.per_slice() || p.step6 != Step6::cached || p.step7 != Step7::last_cached ||
                                p.checked || in.dim > 2 || width > 9 || iterations != 2)
                              fail("the mask goes with the cached kernels of two passes up to two dimensions only");
                          } else if (mask < 0) {
                            StepPlanInput again = in;
                            again.debug_next_tile_mask = 0;
                            if (plan_step(again).next_tile_mask)
                              ++off_by_switch;
                          } else if (p.step6 == Step6::cached && p.step7 == Step7::last_cached && !p.checked &&
                                     in.dim <= 2)
                            ++off_by_sharing;
                        }
    std::printf("{\"plans\": %llu, \"violations\": %llu, \"first\": \"%s\", \"on\": %llu, \"elided\": %llu, "
                "\"on_split_sweep\": %llu, "
                "\"off_by_switch\": %llu, \"off_by_sharing\": %llu}\n",
                n, bad, first_bad.c_str(), on, elided, on_split_sweep, off_by_switch, off_by_sharing);
    return bad == 0 ? 0 : 1;
  }

  /* plans that must not carry the mask, with the boolean forced on */
  int run_forced()
  {
    struct Forced {
      const char *name;
      PlanEquation e;
      int dim;
      uint32_t width, n_slices, n_export;
      int storage;
      bool checked;
    };
    const Forced cases[] = {
        {"split", PlanEquation::shallow_water, 2, 9, 100, 0, 0, false},             /* four waves per slice */
        {"split_export_part", PlanEquation::shallow_water, 2, 9, 1138, 6, 0, false}, /* ... in the export launch only */
        {"per_slice", PlanEquation::euler, 2, 9, 5000, 0, 1, false},                /* light, repair, heavy */
        {"per_slice_3d", PlanEquation::euler, 3, 27, 5000, 0, 0, false},
        {"generic_step7", PlanEquation::euler, 2, 25, 5000, 0, 0, false}, /* k_high_order<E, true> */
        {"checked", PlanEquation::euler, 2, 9, 5000, 0, 0, true},
    };
    int bad = 0;
    std::printf("{");
    for (size_t q = 0; q < sizeof(cases) / sizeof(cases[0]); ++q) {
      const Forced &c = cases[q];
      StepPlanInput in = default_input();
      in.equation = c.e;
      in.dim = c.dim;
      in.max_row_len = c.width;
      in.n_slices = c.n_slices;
      in.n_export_slices = c.n_export;
      in.debug_pij_storage = c.storage;
      in.checked = c.checked;
      in.limited_fraction = 0.5;
      StepPlan p = plan_step(in);
      const bool was_off = !p.next_tile_mask && p.violated == nullptr && p.unsupported == nullptr;
      p.next_tile_mask = true;
      const char *v = next_tile_mask_violated(p, in.n_slices, in.n_export_slices);
      if (!was_off || v == nullptr)
        ++bad;
      std::printf("%s\"%s\": {\"off_in_the_plan\": %s, \"refused\": \"%s\"}", q ? ", " : "", c.name, b(was_off),
                  v ? v : "");
    }
    /* ... and the plan that does carry it passes */
    StepPlanInput in = default_input();
    in.equation = PlanEquation::euler;
    in.dim = 2;
    in.max_row_len = 9;
    in.n_slices = 5000;
    const StepPlan p = plan_step(in);
    if (!p.next_tile_mask || p.violated != nullptr)
      ++bad;
    /* (plan_step() derives the cached steps 6 and 7 from the same row width: the generic step 7 behind the cached
     * step 6 exists only as an edited plan) */
    StepPlan generic7 = p;
    generic7.step7 = Step7::high_order;
    const char *v7 = next_tile_mask_violated(generic7, in.n_slices, in.n_export_slices);
    StepPlan checked = p;
    checked.checked = true;
    const char *vc = next_tile_mask_violated(checked, in.n_slices, in.n_export_slices);
    StepPlan elided_alone = p; /* zeros elided without the mask that says where */
    elided_alone.next_tile_mask = false;
    const char *ve = next_tile_mask_violated(elided_alone, in.n_slices, in.n_export_slices);
    if (v7 == nullptr || vc == nullptr || ve == nullptr || !p.next_tiles_elided)
      ++bad;
    std::printf(", \"accepted\": %s, \"accepted_with_generic_step7\": \"%s\", \"accepted_but_checked\": \"%s\"}\n",
                b(p.next_tile_mask && p.violated == nullptr), v7 ? v7 : "", vc ? vc : "");
    return bad == 0 ? 0 : 1;
  }
} // namespace

int main(int argc, char **argv)
{
  if (argc >= 2 && !std::strcmp(argv[1], "plan"))
    return run_plan(argc, argv);
  if (argc >= 2 && !std::strcmp(argv[1], "lattice"))
    return run_lattice();
  if (argc >= 2 && !std::strcmp(argv[1], "forced"))
    return run_forced();
  return 2;
}
