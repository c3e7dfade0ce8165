// CPU check of the stencil classes (ryujin_amd/csrc/host_layout.hpp, SellLayout::build_stencil_classes): every slice
// that is marked uniform must reproduce the explicit arrays from its class entry, lane by lane --
//   the bits of c_ij and of m_ij in the device layout, and row + delta == cols
// -- must have no padding, and must be as wide as its class; no two classes hold the same key; and a slice that is not
// marked is not uniform (as long as the cap on the number of classes was not reached). Prints the counts.
// usage: stencil_classes box dim nx ny nz | stencil_classes mach3 cells_per_unit n_ranks rank
// (test infrastructure; built by tests/test_stencil_classes.py)
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
  /* what the sweeps read where there is no class: the arrays in the device layout */
  const std::vector<double> cij = L.scatter(o, o.cij, (uint32_t)dim), mij = L.scatter(o, o.mij, 1);
  const uint32_t W = stencil_class_entry_words(dim);
  const uint32_t word_m = dim <= 2 ? 2u : 3u, word_delta = word_m + 1u;
  const uint32_t n_classes = L.n_stencil_classes();
  uint64_t bad = 0, uniform = 0, uniform_tiles = 0, padded = 0;

  bad += L.slice_class.empty() != (L.n_uniform_slices == 0);
  bad += L.slice_class.empty() != L.class_table.empty() || L.slice_class.empty() != L.class_first.empty();
  bad += !L.slice_class.empty() && L.slice_class.size() != L.n_slices;
  bad += n_classes > kStencilClassesMax;
  bad += !L.class_first.empty() && (uint64_t)L.class_first.back() * W != L.class_table.size();

  for (uint32_t s = 0; s < L.n_slices; ++s) {
    const uint32_t width = L.slice_off[s + 1] - L.slice_off[s];
    const uint32_t cls = L.slice_class.empty() ? kStencilClassNone : L.slice_class[s];
    const bool full = (uint64_t)(s + 1) * kWave <= L.n_owned;
    if (cls != kStencilClassNone) {
      ++uniform;
      uniform_tiles += width;
      /* the class: an entry of class_first, as wide as the slice */
      uint32_t k = 0;
      while (k < n_classes && L.class_first[k] != cls)
        ++k;
      if (k == n_classes || L.class_first[k + 1] - cls != width || !full || width == 0) {
        ++bad;
        continue;
      }
      for (uint32_t l = 0; l < kWave; ++l)
        padded += L.row_len[(size_t)s * kWave + l] != width;
      for (uint32_t c = 0; c < width; ++c) {
        const uint64_t *e = L.class_table.data() + ((size_t)cls + c) * W;
        for (uint32_t l = 0; l < kWave; ++l) {
          const uint64_t p = ((uint64_t)L.slice_off[s] + c) * kWave + l;
          const uint32_t row = s * kWave + l;
          for (int d = 0; d < dim; ++d)
            bad += bits(cij[L.comp_pos(p, (uint32_t)dim, (uint32_t)d)]) != e[d];
          for (uint32_t d = (uint32_t)dim; d < word_m; ++d)
            bad += e[d] != 0;
          bad += bits(mij[p]) != e[word_m];
          bad += (e[word_delta] >> 32) != 0;
          bad += (uint32_t)((int32_t)row + (int32_t)(uint32_t)e[word_delta]) != L.cols[p];
        }
      }
    } else if (n_classes < kStencilClassesMax && full && width > 0) {
      /* not marked: some lane differs from lane 0 somewhere, or a row is shorter than the slice */
      bool same = true;
      for (uint32_t l = 0; l < kWave && same; ++l)
        same = L.row_len[(size_t)s * kWave + l] == width;
      for (uint32_t c = 0; c < width && same; ++c) {
        const uint64_t p0 = ((uint64_t)L.slice_off[s] + c) * kWave;
        for (uint32_t l = 1; l < kWave && same; ++l) {
          same = L.cols[p0 + l] - l == L.cols[p0] && bits(mij[p0 + l]) == bits(mij[p0]);
          for (int d = 0; d < dim && same; ++d)
            same = bits(cij[L.comp_pos(p0 + l, (uint32_t)dim, (uint32_t)d)]) == bits(cij[L.comp_pos(p0, (uint32_t)dim, (uint32_t)d)]);
        }
      }
      bad += same;
    }
  }
  bad += padded;
  bad += uniform != L.n_uniform_slices || uniform_tiles != L.n_uniform_tiles;
  /* two slices share a class only if their keys are bit-equal: every slice equals its class entry (above), and no two
   * classes are the same key */
  for (uint32_t a = 0; a < n_classes; ++a)
    for (uint32_t b = a + 1; b < n_classes; ++b) {
      const uint32_t wa = L.class_first[a + 1] - L.class_first[a], wb = L.class_first[b + 1] - L.class_first[b];
      bad += wa == wb && std::memcmp(L.class_table.data() + (size_t)L.class_first[a] * W,
                                     L.class_table.data() + (size_t)L.class_first[b] * W, (size_t)wa * W * 8) == 0;
    }
  std::printf("{\"n_slices\": %u, \"n_full_slices\": %u, \"n_tiles\": %llu, \"n_uniform_slices\": %llu, \"n_uniform_tiles\": %llu, "
              "\"n_classes\": %u, \"padded_rows\": %llu, \"violations\": %llu}\n",
              L.n_slices, L.n_owned / kWave, (unsigned long long)L.slice_off[L.n_slices], (unsigned long long)uniform,
              (unsigned long long)uniform_tiles, n_classes, (unsigned long long)padded, (unsigned long long)bad);
  ryujin_synth_free(synth);
  return bad == 0 ? 0 : 1;
}
