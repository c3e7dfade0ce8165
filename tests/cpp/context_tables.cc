// CPU check of the host tables of a context (ryujin_amd/csrc/host_context.hpp): runs what ryujin_hip_ctx::create()
// runs on the host -- check_create_arguments, system_shape, SellLayout::build, lower_mask, build_boundary_tables,
// build_pair_tables, n_export_slices, interior_rows_read_ghosts, mesh_knobs, build_exchange_tables -- on an OfflineData
// dump or on the forward-facing step mesh, and prints every table as JSON; the expected values are formed by
// tests/test_context_tables.py. A refusal (HipError) is printed as its status, its message and the stage that threw.
// usage: context_tables shape
//        context_tables (file PATH | mach3 cells_per_unit n_ranks rank) [key=value ...]
//   params:   equation dim sc_flux sc_random_entropies eos limiter_iterations debug_pij_storage sc_delta
//             debug_band_stride debug_xcd_chunk
//   offline:  n_export b_id0 b_i0 p_col0 (entry 0 of the array) dg (discontinuous_ansatz, no matrices)
//   others:   have_comm (default 1)  permute=PATH (doubles [n_bdry][K] then [n_bdry][dim], permuted and printed)
//             arrays=0 (print the scalars only)
// (test infrastructure; built by tests/test_context_tables.py)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "host_context.hpp"
#include "ryujin_offline_io.h"
#include "ryujin_synth.h"

using namespace ryujin_hip;

namespace
{
  template <typename T>
  void print_array(const char *name, const std::vector<T> &v, const char *end = ", ")
  {
    std::printf("\"%s\": [", name);
    for (size_t q = 0; q < v.size(); ++q)
      std::printf("%s%llu", q ? "," : "", (unsigned long long)v[q]);
    std::printf("]%s", end);
  }

  /* doubles as their bit patterns: compared bit for bit */
  void print_bits(const char *name, const std::vector<double> &v)
  {
    std::vector<uint64_t> b(v.size());
    if (!v.empty())
      std::memcpy(b.data(), v.data(), v.size() * sizeof(double));
    print_array(name, b);
  }

  constexpr uint32_t kXcdChunk3d = 8, kWavesPerBlock = 4; /* the values ryujin_hip.hip passes to mesh_knobs() */
} // namespace

int main(int argc, char **argv)
{
  if (argc >= 2 && std::string(argv[1]) == "shape") {
    std::printf("[");
    const int eq[4] = {RYUJIN_EQ_EULER, RYUJIN_EQ_SHALLOW_WATER, RYUJIN_EQ_EULER_AEOS, RYUJIN_EQ_SCALAR_CONSERVATION};
    for (int e = 0; e < 4; ++e)
      for (int dim = 1; dim <= (eq[e] == RYUJIN_EQ_SHALLOW_WATER ? 2 : 3); ++dim) {
        const SystemShape s = system_shape(eq[e], dim);
        std::printf("%s[%d, %d, %d, %d, %d, %d, %d]", e + dim > 1 ? ", " : "", eq[e], dim, s.K, s.KP, s.NB, s.NPREC, s.RS);
      }
    std::printf("]\n");
    return 0;
  }
  if (argc < 3)
    return 2;

  /* the offline data */
  ryujin_synth *synth = nullptr;
  ryujin_offline_file *file = nullptr;
  ryujin_hip_offline o{};
  int dim = 0, next = 3;
  if (std::string(argv[1]) == "file") {
    file = ryujin_offline_read(argv[2]);
    if (!file) {
      std::fprintf(stderr, "%s\n", ryujin_offline_io_last_error());
      return 3;
    }
    o = *ryujin_offline_file_view(file);
    dim = ryujin_offline_file_dim(file);
  } else { /* offline.mach3_step_2d(cells_per_unit, n_ranks=, rank=) */
    if (argc < 5)
      return 2;
    ryujin_synth_spec spec{};
    const uint32_t cpu = (uint32_t)std::atoi(argv[2]);
    spec.dim = dim = 2;
    spec.n_cells[0] = 3 * cpu;
    spec.n_cells[1] = cpu;
    spec.n_cells[2] = 1;
    spec.upper[0] = 3.;
    spec.upper[1] = spec.upper[2] = 1.;
    for (int f = 0; f < 6; ++f)
      spec.bc[f] = f < 4 ? RYUJIN_BC_SLIP : RYUJIN_BC_DO_NOTHING;
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
    synth = ryujin_synth_build(&spec);
    if (!synth) {
      std::fprintf(stderr, "%s\n", ryujin_synth_last_error());
      return 3;
    }
    o = *ryujin_synth_offline(synth);
    next = 5;
  }

  /* the edits */
  ryujin_hip_params p{};
  p.equation = RYUJIN_EQ_EULER;
  p.dim = dim;
  p.limiter_iterations = 2;
  p.sc_derivative_approximation_delta = 1.e-10;
  bool have_comm = true, arrays = true;
  std::string permute_path;
  std::vector<uint8_t> b_id(o.b_id, o.b_id + o.n_bdry);
  std::vector<uint32_t> b_i(o.b_i, o.b_i + o.n_bdry), p_col(o.p_col, o.p_col + o.n_pairs);
  o.b_id = b_id.data();
  o.b_i = b_i.data();
  o.p_col = p_col.data();
  const std::map<std::string, int *> int_fields = {
      {"equation", &p.equation},
      {"dim", &p.dim},
      {"sc_flux", &p.sc_flux},
      {"sc_random_entropies", &p.sc_random_entropies},
      {"eos", &p.eos},
      {"limiter_iterations", &p.limiter_iterations},
      {"debug_pij_storage", &p.debug_pij_storage},
      {"debug_band_stride", &p.debug_band_stride},
      {"debug_xcd_chunk", &p.debug_xcd_chunk},
      {"dg", &o.discontinuous_ansatz},
  };
  for (int a = next; a < argc; ++a) {
    const std::string arg = argv[a];
    const size_t eq = arg.find('=');
    if (eq == std::string::npos)
      return 2;
    const std::string key = arg.substr(0, eq), value = arg.substr(eq + 1);
    if (int_fields.count(key))
      *int_fields.at(key) = std::atoi(value.c_str());
    else if (key == "sc_delta")
      p.sc_derivative_approximation_delta = std::strtod(value.c_str(), nullptr); /* "nan" and "inf" included */
    else if (key == "n_export")
      o.n_export = (uint32_t)std::strtoul(value.c_str(), nullptr, 10);
    else if (key == "b_id0" && !b_id.empty())
      b_id[0] = (uint8_t)std::atoi(value.c_str());
    else if (key == "b_i0" && !b_i.empty())
      b_i[0] = (uint32_t)std::strtoul(value.c_str(), nullptr, 10);
    else if (key == "p_col0" && !p_col.empty())
      p_col[0] = (uint32_t)std::strtoul(value.c_str(), nullptr, 10);
    else if (key == "have_comm")
      have_comm = std::atoi(value.c_str()) != 0;
    else if (key == "arrays")
      arrays = std::atoi(value.c_str()) != 0;
    else if (key == "permute")
      permute_path = value;
    else
      return 2;
  }

  /* the host half of create(), in its order */
  const char *stage = "check_create_arguments";
  try {
    check_create_arguments(o, p, have_comm);
    dim = p.dim;
    const SystemShape shape = system_shape(p.equation, dim);
    stage = "layout";
    SellLayout L;
    L.build(o);
    const std::vector<uint32_t> mask = lower_mask(L);
    stage = "build_pair_tables";
    const PairTables pairs = build_pair_tables(o, L, L.scatter(o, o.cij, (uint32_t)dim), dim);
    stage = "build_boundary_tables";
    const BoundaryTables B = build_boundary_tables(o, L, dim);
    stage = "mesh_knobs";
    const MeshKnobs knobs = mesh_knobs(p, L, dim, kXcdChunk3d, kWavesPerBlock);
    const uint32_t n_export = n_export_slices(o, L);
    const bool reads_ghosts = interior_rows_read_ghosts(L, n_export);
    stage = "build_exchange_tables";
    const ExchangeTables X = build_exchange_tables(o, L, shape.KP, shape.NPREC);

    std::printf("{\"status\": 0, \"dim\": %d, \"n_owned\": %u, \"n_relevant\": %u, \"n_slices\": %u, \"rows_padded\": %u, "
                "\"max_row_len\": %u, \"nnz_sell\": %llu, ",
                dim, L.n_owned, L.n_relevant, L.n_slices, L.rows_padded, L.max_row_len, (unsigned long long)L.nnz_sell);
    std::printf("\"band_stride\": %u, \"xcd_chunk\": %u, \"tail_queue_columns\": %u, \"bounds_stride\": %u, ",
                knobs.band_stride, knobs.xcd_chunk, knobs.tail_queue_columns, knobs.bounds_stride);
    std::printf("\"n_export_slices\": %u, \"interior_rows_read_ghosts\": %d, ", n_export, (int)reads_ghosts);
    std::printf("\"n_bdry\": %u, \"n_groups\": %u, \"needs_dirichlet\": %d, ", B.n_bdry, B.n_groups, (int)B.needs_dirichlet);
    if (arrays) {
      print_array("lower_mask", mask);
      print_array("perm", B.perm);
      print_array("b_i", B.b_i);
      print_array("b_id", B.b_id);
      print_bits("b_normal", B.b_normal);
      print_array("grp_start", B.grp_start);
      print_array("rows", B.rows);
      print_array("bc_mask", B.bc_mask);
      print_array("bc_first", B.bc_first);
      print_array("pair_pos", pairs.pos);
      print_bits("pair_cji", pairs.cji);
      print_array("nbr_rank", X.nbr_rank);
      print_array("send_off", X.send_off);
      print_array("recv_off", X.recv_off);
      print_array("row_send_off", X.row_send_off);
      print_array("row_send_pos", X.row_send_pos);
      print_array("row_recv_off", X.row_recv_off);
    }
    if (!permute_path.empty()) {
      const size_t n_K = (size_t)B.n_bdry * shape.K, n_dim = (size_t)B.n_bdry * dim;
      std::vector<double> in(n_K + n_dim), by_K(n_K), by_dim(n_dim);
      std::FILE *f = std::fopen(permute_path.c_str(), "rb");
      if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size())
        return 3;
      std::fclose(f);
      B.permute(in.data(), shape.K, by_K.data());
      B.permute(in.data() + n_K, dim, by_dim.data());
      print_bits("permuted_K", by_K);
      print_bits("permuted_dim", by_dim);
    }
    std::printf("\"n_nbr\": %d, \"send_buffer_doubles\": %llu}\n", X.n_nbr, (unsigned long long)X.send_buffer_doubles);
  } catch (const HipError &e) {
    std::printf("{\"status\": %d, \"message\": \"%s\", \"stage\": \"%s\"}\n", e.status, e.what(), stage);
  }
  if (synth)
    ryujin_synth_free(synth);
  if (file)
    ryujin_offline_file_free(file);
  return 0;
}
