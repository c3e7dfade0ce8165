// Stand-alone checker of ryujin_amd/csrc/output_selection.hpp (tests/test_output_selection_cpu.py): prints what the
// header computes as JSON, the expectations are formed in Python. No HIP, no context.
//   output_selection_cases names <equation> <dim>                 the four name tables
//   output_selection_cases resolve <equation> <dim> <pp> <name>   pp = comma separated kind:is_primitive:component
//   output_selection_cases cell <n_manifolds> <n_vertices> <hex bits of the vertex values, manifold major>
//   output_selection_cases compact <block> <flags as a string of 0 and 1, or @file>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "output_selection.hpp"

using namespace ryujin_hip;

namespace
{
  void print_list(const char *key, const std::vector<std::string> &names, const bool last = false)
  {
    std::printf("\"%s\": [", key);
    for (size_t i = 0; i < names.size(); ++i)
      std::printf("%s\"%s\"", i ? ", " : "", names[i].c_str());
    std::printf("]%s", last ? "" : ", ");
  }

  std::vector<OutputPostprocessQuantity> parse_pp(const std::string &text)
  {
    std::vector<OutputPostprocessQuantity> out;
    if (text == "-")
      return out;
    std::stringstream all(text);
    std::string item;
    while (std::getline(all, item, ',')) {
      OutputPostprocessQuantity q{};
      if (std::sscanf(item.c_str(), "%d:%d:%d", &q.kind, &q.is_primitive, &q.component) != 3) {
        std::fprintf(stderr, "bad postprocess quantity '%s'\n", item.c_str());
        std::exit(2);
      }
      out.push_back(q);
    }
    return out;
  }
} // namespace

int main(int argc, char **argv)
{
  if (argc < 2)
    return 2;
  const std::string mode = argv[1];
  if (mode == "names" && argc == 4) {
    OutputNames names;
    if (!output_names(std::atoi(argv[2]), std::atoi(argv[3]), names)) {
      std::printf("null\n");
      return 0;
    }
    std::printf("{");
    print_list("conserved", names.conserved);
    print_list("primitive", names.primitive);
    print_list("precomputed", names.precomputed);
    print_list("initial_precomputed", names.initial_precomputed, true);
    std::printf("}\n");
    return 0;
  }
  if (mode == "resolve" && argc == 6) {
    OutputNames names;
    if (!output_names(std::atoi(argv[2]), std::atoi(argv[3]), names))
      return 2;
    const std::vector<OutputPostprocessQuantity> pp = parse_pp(argv[4]);
    const std::vector<std::string> pp_names = output_postprocess_names(names, pp.data(), (int)pp.size());
    OutputResolved r{-1, -1};
    std::string error;
    const bool ok = output_resolve(names, pp_names, argv[5], r, error);
    std::string escaped;
    for (const char c : error) {
      if (c == '"' || c == '\\')
        escaped += '\\';
      escaped += c;
    }
    std::printf("{\"ok\": %s, \"kind\": %d, \"index\": %d, \"error\": \"%s\", ", ok ? "true" : "false", r.kind, r.index,
                escaped.c_str());
    print_list("postprocess_names", pp_names, true);
    std::printf("}\n");
    return 0;
  }
  if (mode == "cell" && argc >= 4) {
    const int n_manifolds = std::atoi(argv[2]), n_vertices = std::atoi(argv[3]);
    if (argc != 4 + n_manifolds * n_vertices)
      return 2;
    std::vector<double> f((size_t)n_manifolds * n_vertices);
    for (size_t e = 0; e < f.size(); ++e) {
      const uint64_t bits = std::strtoull(argv[4 + e], nullptr, 16);
      std::memcpy(&f[e], &bits, sizeof(double));
    }
    const bool selected = output_cell_selected(n_manifolds, n_vertices,
                                               [&](const int m, const int v) { return f[(size_t)m * n_vertices + v]; });
    std::printf("{\"selected\": %s}\n", selected ? "true" : "false");
    return 0;
  }
  if (mode == "compact" && argc == 4) {
    const size_t block = (size_t)std::atoll(argv[2]);
    std::string text = argv[3];
    if (!text.empty() && text[0] == '@') {
      std::ifstream in(text.substr(1));
      std::stringstream buffer;
      buffer << in.rdbuf();
      text = buffer.str();
    }
    std::vector<uint8_t> flags;
    for (const char c : text)
      if (c == '0' || c == '1')
        flags.push_back(c == '1');
    const size_t n = flags.size(), n_blocks = output_compaction_blocks(n, block);
    std::vector<uint32_t> counts(n_blocks), offsets(n_blocks + 1), list, map(n);
    output_compaction_counts(flags.data(), n, counts.data(), block);
    const uint32_t total = output_compaction_offsets(counts.data(), n_blocks, offsets.data());
    const uint32_t length = output_compact(flags.data(), n, list, map.data(), block);
    const auto print = [](const char *key, const std::vector<uint32_t> &v, const bool last) {
      std::printf("\"%s\": [", key);
      for (size_t i = 0; i < v.size(); ++i)
        std::printf("%s%u", i ? ", " : "", v[i]);
      std::printf("]%s", last ? "" : ", ");
    };
    std::printf("{\"n\": %zu, \"n_blocks\": %zu, \"total\": %u, \"length\": %u, ", n, n_blocks, total, length);
    print("counts", counts, false);
    print("offsets", offsets, false);
    print("list", list, false);
    print("map", map, true);
    std::printf("}\n");
    return 0;
  }
  std::fprintf(stderr, "usage: see the head of tests/cpp/output_selection_cases.cc\n");
  return 2;
}
