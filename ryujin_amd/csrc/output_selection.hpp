// VTUOutput: which quantity a name stands for, which cells a level set selects, and where a selected item goes.
//
// Reference: source/vtu_output.template.h (schedule_output, :80-205) and source/selected_components_extractor.h.
//   output_names()              View::component_names, primitive_component_names, precomputed_names and
//                               initial_precomputed_names of source/<eq>/hyperbolic_system.h, per Description and
//                               dimension
//   output_postprocess_names()  Postprocessor::component_names() (source/postprocessor.template.h:74-97): the prefix
//                               "schlieren_" / "vorticity_" in front of the conserved or primitive component name
//   output_resolve()            name -> (kind, index) in the search order of SelectedComponentsExtractor::extract
//                               (:77-88): conserved, primitive, precomputed, initial precomputed, "alpha"; the
//                               postprocessed names, which the reference always appends (:119-123), come last
//   output_cell_selected()      the cell filter of the level-set output (:167-188), host and device
//   output_compaction_*()       the order-preserving compaction plan of the kernels (kernels_output.hpp): per-block
//                               counts -> exclusive offsets; an item goes to offsets[block] + (selected items before it
//                               in its block). output_compact() is the plan executed on the host, for the CPU tests.
// Host standard library only -- no HIP, no context; checked on the CPU by tests/cpp/output_selection_cases.cc.
#ifndef RYUJIN_HIP_OUTPUT_SELECTION_HPP
#define RYUJIN_HIP_OUTPUT_SELECTION_HPP

#include <cfloat>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define RYUJIN_OUTPUT_HD __host__ __device__ __forceinline__
#else
#define RYUJIN_OUTPUT_HD inline
#endif

namespace ryujin_hip
{
  /* RYUJIN_EQ_* of ryujin_hip.h, repeated so that this header stands alone */
  constexpr int kOutEqEuler = 0, kOutEqShallowWater = 1, kOutEqEulerAeos = 2, kOutEqScalarConservation = 3;
  /* RYUJIN_PP_SCHLIEREN / RYUJIN_PP_VORTICITY */
  constexpr int kOutPpSchlieren = 0, kOutPpVorticity = 1;

  enum OutputKind : int {
    kOutConserved = 0,
    kOutPrimitive = 1,
    kOutPrecomputed = 2,
    kOutInitialPrecomputed = 3,
    kOutAlpha = 4,
    kOutPostprocessed = 5
  };

  constexpr int kOutputBlock = 256; /* items per block of the compaction (kBlock of the kernels) */

  struct OutputNames {
    std::vector<std::string> conserved, primitive, precomputed, initial_precomputed;
  };

  /* `base` in 1-D, base_1 .. base_dim otherwise */
  inline void output_vector_names(std::vector<std::string> &names, const std::string &base, const int dim)
  {
    if (dim == 1)
      names.push_back(base);
    else
      for (int d = 0; d < dim; ++d)
        names.push_back(base + "_" + std::to_string(d + 1));
  }

  /* false: no such Description or dimension */
  inline bool output_names(const int equation, const int dim, OutputNames &names)
  {
    names = OutputNames{};
    if (dim < 1 || dim > 3)
      return false;
    switch (equation) {
    case kOutEqEuler:      /* euler/hyperbolic_system.h:240-297 */
    case kOutEqEulerAeos: /* euler_aeos/hyperbolic_system.h:335-396 */
      names.conserved.push_back("rho");
      output_vector_names(names.conserved, "m", dim);
      names.conserved.push_back("E");
      names.primitive.push_back("rho");
      output_vector_names(names.primitive, "v", dim);
      if (equation == kOutEqEuler) {
        names.primitive.push_back("p");
        names.precomputed = {"s", "eta_h"};
      } else {
        names.primitive.push_back("e");
        names.precomputed = {"p", "surrogate_gamma", "surrogate_specific_entropy", "surrogate_harten_entropy"};
      }
      return true;
    case kOutEqShallowWater: /* shallow_water/hyperbolic_system.h:207-264 */
      names.conserved.push_back("h");
      output_vector_names(names.conserved, "m", dim);
      names.primitive.push_back("h");
      output_vector_names(names.primitive, "v", dim);
      names.precomputed = {"eta_m", "h_star"};
      names.initial_precomputed = {"bathymetry"};
      return true;
    case kOutEqScalarConservation: /* scalar_conservation/hyperbolic_system.h:187-236 */
      names.conserved = {"u"};
      names.primitive = {"u"};
      output_vector_names(names.precomputed, "f", dim);
      output_vector_names(names.precomputed, "df", dim);
      return true;
    default:
      return false;
    }
  }

  /* ryujin_hip_postprocess_quantity */
  struct OutputPostprocessQuantity {
    int kind, is_primitive, component;
  };

  /* Postprocessor::component_names() for the configured quantities, in their order; a quantity outside the state
   * gets the empty name, which no request matches */
  inline std::vector<std::string> output_postprocess_names(const OutputNames &names, const OutputPostprocessQuantity *q,
                                                           const int n)
  {
    std::vector<std::string> out;
    for (int i = 0; i < n; ++i) {
      const std::vector<std::string> &from = q[i].is_primitive ? names.primitive : names.conserved;
      const bool known = (q[i].kind == kOutPpSchlieren || q[i].kind == kOutPpVorticity) && q[i].component >= 0 &&
                         q[i].component < (int)from.size();
      out.push_back(known ? std::string(q[i].kind == kOutPpSchlieren ? "schlieren_" : "vorticity_") +
                                from[q[i].component]
                          : std::string());
    }
    return out;
  }

  struct OutputResolved {
    int kind;  /* OutputKind */
    int index; /* component within its array; 0 for alpha */
  };

  /* SelectedComponentsExtractor::check (:25-45), with its message */
  inline std::string output_invalid_name_message(const std::string &name)
  {
    return "Invalid component name: \"" + name +
           "\" is not a valid conserved/primitive/precomputed/initial component name.";
  }

  /* true and `out`, or false and `error` */
  inline bool output_resolve(const OutputNames &names, const std::vector<std::string> &postprocess_names,
                             const std::string &name, OutputResolved &out, std::string &error)
  {
    const auto search = [&](const std::vector<std::string> &list, const int kind) {
      for (size_t i = 0; i < list.size(); ++i)
        if (!list[i].empty() && list[i] == name) {
          out = OutputResolved{kind, (int)i};
          return true;
        }
      return false;
    };
    if (search(names.conserved, kOutConserved) || search(names.primitive, kOutPrimitive) ||
        search(names.precomputed, kOutPrecomputed) || search(names.initial_precomputed, kOutInitialPrecomputed))
      return true;
    if (name == "alpha") {
      out = OutputResolved{kOutAlpha, 0};
      return true;
    }
    if (search(postprocess_names, kOutPostprocessed))
      return true;
    error = output_invalid_name_message(name);
    return false;
  }

  /* The cell filter (:171-187): selected if for SOME manifold one vertex has f >= -100 eps and one has f <= +100 eps,
   * eps = DBL_EPSILON. value(m, v) is the level set m at vertex v of the cell. A NaN is neither: it selects nothing. */
  template <typename Value>
  RYUJIN_OUTPUT_HD bool output_cell_selected(const int n_manifolds, const int n_vertices, Value &&value)
  {
    constexpr double eps = DBL_EPSILON;
    for (int m = 0; m < n_manifolds; ++m) {
      unsigned int above = 0, below = 0;
      for (int v = 0; v < n_vertices; ++v) {
        const double f = value(m, v);
        if (f >= 0. - 100. * eps)
          above++;
        if (f <= 0. + 100. * eps)
          below++;
        if (above > 0 && below > 0)
          return true;
      }
    }
    return false;
  }

  /* ---- the compaction plan ---------------------------------------------------------------------------------- */

  inline size_t output_compaction_blocks(const size_t n, const size_t block = kOutputBlock)
  {
    return (n + block - 1) / block;
  }

  /* counts[b] = number of set flags among the items [b * block, (b + 1) * block) */
  inline void output_compaction_counts(const uint8_t *flags, const size_t n, uint32_t *counts,
                                       const size_t block = kOutputBlock)
  {
    const size_t n_blocks = output_compaction_blocks(n, block);
    for (size_t b = 0; b < n_blocks; ++b) {
      uint32_t c = 0;
      for (size_t i = b * block; i < n && i < (b + 1) * block; ++i)
        c += flags[i] ? 1u : 0u;
      counts[b] = c;
    }
  }

  /* offsets[b] = counts[0] + ... + counts[b - 1] for b in [0, n_blocks]: offsets[n_blocks] is the total */
  inline uint32_t output_compaction_offsets(const uint32_t *counts, const size_t n_blocks, uint32_t *offsets)
  {
    uint32_t running = 0;
    for (size_t b = 0; b < n_blocks; ++b) {
      offsets[b] = running;
      running += counts[b];
    }
    offsets[n_blocks] = running;
    return running;
  }

  /* The plan executed: list = the indices of the set flags in ascending order; map (may be NULL) [n] = position of
   * item i in the list, or kOutputNotSelected. Returns the length of the list. */
  constexpr uint32_t kOutputNotSelected = 0xffffffffu;

  inline uint32_t output_compact(const uint8_t *flags, const size_t n, std::vector<uint32_t> &list, uint32_t *map,
                                 const size_t block = kOutputBlock)
  {
    const size_t n_blocks = output_compaction_blocks(n, block);
    std::vector<uint32_t> counts(n_blocks), offsets(n_blocks + 1);
    output_compaction_counts(flags, n, counts.data(), block);
    const uint32_t total = output_compaction_offsets(counts.data(), n_blocks, offsets.data());
    list.assign(total, 0u);
    for (size_t b = 0; b < n_blocks; ++b) {
      uint32_t rank = 0;
      for (size_t i = b * block; i < n && i < (b + 1) * block; ++i) {
        if (flags[i]) {
          list[offsets[b] + rank] = (uint32_t)i;
          if (map)
            map[i] = offsets[b] + rank;
          ++rank;
        } else if (map)
          map[i] = kOutputNotSelected;
      }
    }
    return total;
  }
} // namespace ryujin_hip

#endif
