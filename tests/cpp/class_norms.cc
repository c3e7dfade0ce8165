// CPU check of the table of norms next to the stencil classes (ryujin_amd/csrc/host_layout.hpp,
// SellLayout::class_norms): for every class entry the two doubles are |c_ij| = sqrt(c_0 c_0 + c_1 c_1 [+ c_2 c_2]) and
// 1 / |c_ij|, bit for bit -- recomputed here from the EXPLICIT c_ij array in the device layout (lane 0 of a slice of
// the class: what step 2 would have computed for that column without the table), every intermediate rounded to a
// double on its own -- and the table is empty exactly where class_table is. Prints the counts.
// usage: class_norms box dim nx ny nz | class_norms mach3 cells_per_unit n_ranks rank
// (test infrastructure; built by tests/test_class_norms.py)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "host_layout.hpp"
#include "ryujin_synth.h"

using namespace ryujin_hip;

static uint64_t bits(const double x)
{
  uint64_t b;
  std::memcpy(&b, &x, sizeof b);
  return b;
}

int main(int argc, char **argv)
{
  if (argc < 5)
    return 2;
  ryujin_synth_spec spec{};
  const std::string kind = argv[1];
  for (int f = 0; f < 6; ++f)
    spec.bc[f] = RYUJIN_BC_SLIP;
  spec.cut_kind = RYUJIN_CUT_NONE;
  spec.n_ranks = 1;
  if (kind == "mach3") { /* offline.mach3_step_2d(cells_per_unit, n_ranks=, rank=) */
    const uint32_t cpu = (uint32_t)std::atoi(argv[2]);
    spec.dim = 2;
    spec.n_cells[0] = 3 * cpu;
    spec.n_cells[1] = cpu;
    spec.n_cells[2] = 1;
    spec.upper[0] = 3.;
    spec.upper[1] = spec.upper[2] = 1.;
    spec.bc[0] = RYUJIN_BC_DIRICHLET;
    spec.bc[1] = RYUJIN_BC_DO_NOTHING;
    spec.cut_kind = RYUJIN_CUT_BOX;
    spec.cut_lo[0] = 0.6;
    spec.cut_lo[1] = -1.;
    spec.cut_hi[0] = 4.;
    spec.cut_hi[1] = 0.2;
    spec.cut_bc = RYUJIN_BC_SLIP;
    spec.n_ranks = std::atoi(argv[3]);
    spec.rank = std::atoi(argv[4]);
  } else {
    if (argc < 6)
      return 2;
    spec.dim = std::atoi(argv[2]);
    for (int d = 0; d < 3; ++d) {
      spec.n_cells[d] = d < spec.dim ? (uint32_t)std::atoi(argv[3 + d]) : 1u;
      spec.lower[d] = 0.;
      spec.upper[d] = 1.;
    }
    for (int f = 2 * spec.dim; f < 6; ++f)
      spec.bc[f] = RYUJIN_BC_DO_NOTHING;
  }
  ryujin_synth *synth = ryujin_synth_build(&spec);
  if (!synth) {
    std::fprintf(stderr, "%s\n", ryujin_synth_last_error());
    return 3;
  }
  const ryujin_hip_offline &o = *ryujin_synth_offline(synth);
  const int dim = spec.dim;
  SellLayout L;
  L.build(o);
  L.build_stencil_classes(o, dim);
  const std::vector<double> cij = L.scatter(o, o.cij, (uint32_t)dim);
  const uint32_t W = stencil_class_entry_words(dim);
  const size_t n_entries = L.class_table.size() / W;
  uint64_t bad = 0, checked = 0, not_finite = 0;

  bad += L.class_norms.empty() != L.class_table.empty();
  bad += L.class_norms.size() != n_entries * 2;

  /* every entry through a slice of its class */
  std::vector<char> seen(n_entries, 0);
  for (uint32_t s = 0; s < L.n_slices && !L.slice_class.empty() && bad == 0; ++s) {
    const uint32_t cls = L.slice_class[s];
    if (cls == kStencilClassNone || seen[cls])
      continue;
    const uint32_t width = L.slice_off[s + 1] - L.slice_off[s];
    for (uint32_t c = 0; c < width; ++c) {
      const uint64_t p = ((uint64_t)L.slice_off[s] + c) * kWave;
      volatile double norm2 = 0.;
      for (int d = 0; d < dim; ++d) {
        const double x = cij[L.comp_pos(p, (uint32_t)dim, (uint32_t)d)];
        volatile double square = x * x;
        norm2 = d == 0 ? square : norm2 + square;
      }
      volatile double norm = std::sqrt(norm2);
      volatile double inverse = 1. / norm;
      const double *e = L.class_norms.data() + ((size_t)cls + c) * 2;
      bad += bits(e[0]) != bits(norm);
      bad += bits(e[1]) != bits(inverse);
      /* (column 0 is the row itself: c_ii = 0 in the interior, 1 / 0 = inf on both sides, read by no kernel) */
      not_finite += c > 0 && (!std::isfinite(e[0]) || !std::isfinite(e[1]) || !(e[0] > 0.));
      seen[cls + c] = 1;
      ++checked;
    }
  }
  for (size_t e = 0; e < n_entries; ++e)
    bad += !seen[e];
  std::printf("{\"n_entries\": %llu, \"n_norms\": %llu, \"n_checked\": %llu, \"not_finite\": %llu, \"violations\": %llu}\n",
              (unsigned long long)n_entries, (unsigned long long)(L.class_norms.size() / 2), (unsigned long long)checked,
              (unsigned long long)not_finite, (unsigned long long)bad);
  ryujin_synth_free(synth);
  return bad == 0 ? 0 : 1;
}
