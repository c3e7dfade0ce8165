// libryujin_hip.so -- C ABI (include/ryujin_hip.h) over the HIP kernels.
//
// One context per (rank, GPU). Everything the module owns lives in HBM for the lifetime of
// the context (hyperbolic_module.h:319-333: alpha, bounds, r, d_ij, l_ij, l_ij_next, p_ij);
// state vectors are device resident behind handles. All sweeps of one step() are enqueued on
// one HIP stream without host synchronisation; the only host<->device round trip per step is
// the 24-byte scalar read-back (tau, restart flag) at the end.
// Multi-GPU: ghost exchange as RCCL point-to-point (ncclSend/ncclRecv grouped per neighbour)
// over xGMI, tau_max / restart flag as 1-element all-reduces, all stream ordered.

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <limits>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "ryujin_hip.h"

#ifndef RYUJIN_XCD_CHUNK_3D
#define RYUJIN_XCD_CHUNK_3D 8 /* XCD-local block ranges (ryujin_hip_params::debug_xcd_chunk == 0), blocks per XCD and chunk. Counted and timed
                                 (profiles/r06a_xcd_probe_sedov3d.md, r06g_xcd_probe_*.md): the L2-miss read traffic of the sweeps falls
                                 in every configuration -- C3 step 5 15.7 -> 10.1 GB, step 2 13.3 -> 9.6 GB per launch; C2 -20 ... -25 % in
                                 every sweep -- and the TIME follows only on C3 (200^3, planes of 4.5 MB: step 5 -5 %, the update
                                 -2.1 %); C4 +-1 %, C2 and C5 +-0.2 %. The sweeps are not bound by the bytes their gathers re-fetch
                                 across XCDs (HBM itself delivers 5.8 - 6.7 TB/s for their read/write mixes,
                                 profiles/r06h_hbm_mix.md): on in 3-D, where it is a gain or a wash, off below */
#endif

#include "host_layout.hpp"
#include "host_context.hpp"
#include "step_plan.hpp"
#include "rank_reduce.hpp"
#include "kernels_euler.hpp"
#include "kernels_limiter.hpp"
#include "kernels_limiter_stage0.hpp"
#include "kernels_euler_aeos.hpp"
#include "kernels_shallow_water.hpp"
#include "scalar_conservation_device.hpp"
#include "kernels_postprocessor.hpp"
#include "kernels_quantities.hpp"
#include "kernels_initial_values.hpp"
#include "kernels_error_norms.hpp"
#include "kernels_output.hpp"

using namespace ryujin_hip;

namespace
{
  thread_local std::string g_error;

#define HIP_CHECK(expr)                                                                        \
  do {                                                                                         \
    const hipError_t err_ = (expr);                                                            \
    if (err_ != hipSuccess)                                                                    \
      throw HipError(RYUJIN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(err_));     \
  } while (0)

#define NCCL_CHECK(expr)                                                                       \
  do {                                                                                         \
    const ncclResult_t res_ = (expr);                                                          \
    if (res_ != ncclSuccess)                                                                   \
      throw HipError(RYUJIN_ERR_COMM, std::string(#expr) + ": " + ncclGetErrorString(res_));   \
  } while (0)

  template <typename T>
  struct DeviceBuffer {
    T *ptr = nullptr;
    void *base = nullptr;
    size_t n = 0;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    ~DeviceBuffer() { release(); }
    void release()
    {
      if (base)
        (void)hipFree(base);
      ptr = nullptr;
      base = nullptr;
      n = 0;
    }
    void alloc(size_t count, bool zero = true)
    {
      release();
      n = count;
      if (count == 0)
        count = 1;
      /* (the allocator hands out 2 MiB aligned blocks; shifting the streams of a context against each other by
       * 4.25 KiB or 260 KiB per stream changed no kernel time: profiles/r03i_placement_*.log) */
      HIP_CHECK(hipMalloc(&base, count * sizeof(T)));
      ptr = static_cast<T *>(base);
      if (zero) {
        /* hipMemset on device memory is asynchronous and ordered on the NULL stream, which does not
         * synchronise with the non-blocking streams of the context: a kernel launched right after the
         * allocation could otherwise be overwritten by the late memset (seen as a flaky zero result of
         * the first ryujin_hip_state_integrals call) */
        HIP_CHECK(hipMemset(ptr, 0, count * sizeof(T)));
        HIP_CHECK(hipDeviceSynchronize());
      }
    }
    void upload(const std::vector<T> &host)
    {
      alloc(host.size(), false);
      if (!host.empty())
        HIP_CHECK(hipMemcpy(ptr, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    }
    void upload(const T *host, size_t count)
    {
      alloc(count, false);
      if (count)
        HIP_CHECK(hipMemcpy(ptr, host, count * sizeof(T), hipMemcpyHostToDevice));
    }
  };

  EulerParams make_euler_params(const ryujin_hip_params &p)
  {
    EulerParams q{};
    q.gamma = p.gamma;
    q.gamma_inverse = 1. / p.gamma;
    q.gamma_plus_one_inverse = 1. / (p.gamma + 1.);
    q.gamma_minus_one_inverse = 1. / (p.gamma - 1.);
    q.reference_density = p.reference_density;
    q.vacuum_small = p.vacuum_state_relaxation_small;
    q.vacuum_large = p.vacuum_state_relaxation_large;
    q.evc_factor = p.indicator_evc_factor;
    q.lim_newton_tolerance = p.limiter_newton_tolerance;
    q.lim_relaxation_factor = p.limiter_relaxation_factor;
    q.lim_newton_max_iterations = p.limiter_newton_max_iterations;
    q.riemann_newton_max_iterations = p.riemann_newton_max_iterations;
    q.riemann_newton_tolerance = p.riemann_newton_tolerance;
    {
      /* gamma = 7/5 in binary gives 2 gamma / (gamma - 1) = 7 (1 + 3e-16): integral to round-off counts
       * (x^7 against x^(7 + 2e-15) differs by 2e-15 |ln x|, far inside the 1e-12 contract on d_ij) */
      const double e = 2. * p.gamma / (p.gamma - 1.);
      q.rarefaction_power =
          (std::fabs(e - std::rint(e)) <= 8. * std::numeric_limits<double>::epsilon() * e && e >= 1. && e <= 16.)
              ? (int)std::rint(e)
              : 0;
    }
  
    return q;
  }

  EulerAeosParams make_aeos_params(const ryujin_hip_params &p)
  {
    EulerAeosParams aeosparams{};
    aeosparams.eos = p.eos;
    aeosparams.strict = p.compute_strict_bounds != 0;
    aeosparams.gamma = p.gamma;
    aeosparams.eos_b = p.eos_covolume_b;
    aeosparams.eos_q = p.eos_q;
    aeosparams.eos_pinf = p.eos_pinf;
    aeosparams.vdw_a = p.eos_vdw_a;
    aeosparams.jwl_A = p.jwl_A;
    aeosparams.jwl_B = p.jwl_B;
    aeosparams.jwl_R1 = p.jwl_R1;
    aeosparams.jwl_R2 = p.jwl_R2;
    aeosparams.jwl_omega = p.jwl_omega;
    aeosparams.jwl_rho_0 = p.jwl_rho_0;
    aeosparams.jwl_q_0 = p.jwl_q_0;
    /* interpolation parameters of the surrogate (equation_of_state_noble_abel_stiffened_gas.h:52-56,
     * equation_of_state_van_der_waals.h:46-52; zero for the other equations of state) */
    aeosparams.b = aeosparams.pinf = aeosparams.q = 0.;
    if (p.eos == RYUJIN_EOS_NOBLE_ABEL_STIFFENED_GAS) {
      aeosparams.b = p.eos_covolume_b;
      aeosparams.pinf = p.eos_pinf;
      aeosparams.q = p.eos_q;
    } else if (p.eos == RYUJIN_EOS_VAN_DER_WAALS) {
      aeosparams.b = p.eos_covolume_b;
      if (p.eos_covolume_b > 0.)
        aeosparams.pinf = p.eos_vdw_a / (p.eos_covolume_b * p.eos_covolume_b);
    }
    aeosparams.reference_density = p.reference_density;
    aeosparams.vacuum_small = p.vacuum_state_relaxation_small;
    aeosparams.vacuum_large = p.vacuum_state_relaxation_large;
    aeosparams.evc_factor = p.indicator_evc_factor;
    aeosparams.lim_newton_tolerance = p.limiter_newton_tolerance;
    aeosparams.lim_relaxation_factor = p.limiter_relaxation_factor;
    aeosparams.lim_newton_max_iterations = p.limiter_newton_max_iterations;
    return aeosparams;
  }

  ShallowWaterParams make_sw_params(const ryujin_hip_params &p)
  {
    ShallowWaterParams q{};
    q.gravity = p.gravity;
    q.manning = p.manning_friction_coefficient;
    q.reference_water_depth = p.reference_water_depth;
    q.dry_state_relaxation_factor = p.dry_state_relaxation_factor;
    q.dry_small = p.dry_state_relaxation_small;
    q.dry_large = p.dry_state_relaxation_large;
    q.evc_factor = p.indicator_evc_factor;
    q.lim_newton_tolerance = p.limiter_newton_tolerance;
    q.lim_relaxation_factor = p.limiter_relaxation_factor;
    q.limit_on_kinetic_energy = p.limiter_limit_on_kinetic_energy;
    q.limit_on_square_velocity = p.limiter_limit_on_square_velocity;
    return q;
  }

  /* Events that order two streams of ONE device: no timing, and no system-scope fence when they complete (the
   * kernels on either side carry their own device-scope release/acquire; a system-scope fence per event writes
   * back and invalidates the L2s under the interior launch that runs next to it). */
  constexpr unsigned kDeviceEventFlags = hipEventDisableTiming | hipEventDisableSystemFence;

  /* (a runtime that does not know the flag -- the process may run on the ROCm runtime its host application
   * bundles -- gets the plain synchronisation event; so does a context created with
   * ryujin_hip_params::system_scope_events != 0) */
  void create_device_event(hipEvent_t *e, const bool system_scope = false)
  {
    if (system_scope || hipEventCreateWithFlags(e, kDeviceEventFlags) != hipSuccess) {
      (void)hipGetLastError();
      HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
  }

  /* waves of k_pij_lij_recompute an MI355X holds at once (256 CUs x 4 SIMDs x 2): below that step 5 splits the
   * columns of a slice over several waves */
  constexpr uint32_t kResidentWavesStep5 = 2048;
  /* the same for the first of the two high-order sweeps (4 waves per SIMD) */
  constexpr uint32_t kResidentWavesStep6 = 4096;
  /* boundary conditions ride on the pre-pass kernel up to this many slices (262 k gridpoints), see BcFold */
  constexpr uint32_t kBcFoldMaxSlices = 4096;

  int grid_for(size_t n, int block = kBlock) { return (int)std::max<size_t>(1, (n + block - 1) / block); }

  /* step 5 on small meshes: launch(std::integral_constant<int, NY>), NY = min(groups, 4) waves per slice, at least 1 */
  template <typename F>
  void with_groups(const uint32_t groups, F &&launch)
  {
    if (groups >= 4)
      launch(std::integral_constant<int, 4>{});
    else if (groups == 3)
      launch(std::integral_constant<int, 3>{});
    else if (groups == 2)
      launch(std::integral_constant<int, 2>{});
    else
      launch(std::integral_constant<int, 1>{});
  }

  /* a run-time bool as a template argument: launch(std::true_type{}) or launch(std::false_type{}) */
  template <typename F>
  void with_bool(const bool value, F &&launch)
  {
    if (value)
      launch(std::true_type{});
    else
      launch(std::false_type{});
  }

  template <typename E> constexpr bool is_euler_v = std::is_same<typename E::Params, EulerParams>::value;
  template <typename E> constexpr bool is_aeos_v = std::is_same<typename E::Params, EulerAeosParams>::value;
  template <typename E> constexpr bool is_scalar_v = std::is_same<typename E::Params, ScalarParams>::value;
  template <typename E> constexpr bool is_sw_v = std::is_same<typename E::Params, ShallowWaterParams>::value;

  static_assert(kPlanWavesPerBlock == (uint32_t)kWavesPerBlock, "step_plan.hpp counts the waves of a block");
} // namespace

/* In-process transport (test facility): several contexts of ONE process, each driven by its own host
 * thread, exchange ghost data on a single GPU (RCCL refuses two ranks on one device). It shares the pack
 * kernels, send/receive offsets, ghost-row layout, streams and events with the RCCL path and -- like RCCL --
 * is purely STREAM ORDERED: no hipStreamSynchronize, no device-side idle point. An ncclSend/ncclRecv pair
 * becomes "neighbour records an event behind its pack kernel; my comm_stream waits for that event and pulls
 * the segment with a device-to-device copy"; because the pull runs on the RECEIVER's stream, a second event
 * in the opposite direction keeps the sender from re-packing its send buffer before every neighbour has
 * pulled (with RCCL the send kernel itself sits on the sender's stream). The host threads only rendezvous
 * on generation counters so that an event is always recorded before a wait on it is enqueued (the one
 * ordering HIP requires; it also makes the cross-stream dependency graph acyclic). A missing
 * hipStreamWaitEvent in the shared choreography is therefore a real data race here, as it would be with
 * RCCL. All-reduces: every rank writes its value into a device slot (double buffered by parity), records
 * an event, waits for the events of all other ranks and reduces the slots with a one-thread kernel. The host
 * half -- the rendezvous and the host-valued vector reductions (reduce_over_ranks) -- is HostRendezvous. */
struct LocalGroup : HostRendezvous {
  static constexpr int kRing = 2;
  /* exchange number g: packed[r] / pulled[r] = number of exchanges whose event rank r has recorded */
  std::vector<unsigned long> packed, pulled, reduced;
  std::vector<hipEvent_t> ev_packed, ev_pulled, ev_reduced; /* [rank * kRing + g % kRing] */
  std::vector<std::vector<const double *>> mail;           /* [src][dst] -> segment in src's send buffer */
  unsigned long long *slots = nullptr;                      /* device: [2][n_ranks][2] 8-byte slots */
  int refs = 0;
  int device = 0;
  /* Measurement facility: ONE rank of an n-rank slab partition run alone, every neighbour replaced by the rank
   * itself (the segment packed for the opposite neighbour is pulled into the ghost range: a periodic channel).
   * Same launches, pack kernels, copies, events and reductions as a middle rank of a real run, on an unshared
   * GPU -- what the choreography costs per rank, without the network (scripts/overhead_loopback.py). */
  bool loopback = false;

  LocalGroup(int n, int dev)
      : HostRendezvous(n)
      , packed(n, 0)
      , pulled(n, 0)
      , reduced(n, 0)
      , ev_packed((size_t)n * kRing, nullptr)
      , ev_pulled((size_t)n * kRing, nullptr)
      , ev_reduced((size_t)n * kRing, nullptr)
      , mail(n, std::vector<const double *>(n, nullptr))
      , device(dev)
  {
    HIP_CHECK(hipSetDevice(dev));
    for (auto *set : {&ev_packed, &ev_pulled, &ev_reduced})
      for (auto &e : *set)
        create_device_event(&e); /* one GPU by construction */
    HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&slots), sizeof(unsigned long long) * 4 * n));
    HIP_CHECK(hipMemset(slots, 0, sizeof(unsigned long long) * 4 * n));
    HIP_CHECK(hipDeviceSynchronize());
  }

  ~LocalGroup()
  {
    /* contexts of the group may still have waits on these events enqueued */
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    for (auto *set : {&ev_packed, &ev_pulled, &ev_reduced})
      for (auto &e : *set)
        if (e)
          (void)hipEventDestroy(e);
    if (slots)
      (void)hipFree(slots);
  }
};

struct ryujin_hip_comm {
  ncclComm_t comm = nullptr;
  int rank = 0, n_ranks = 1, device = 0;
  LocalGroup *local = nullptr;
};

struct ryujin_hip_ctx {
  ryujin_hip_params params{};
  int dim = 0, K = 0, KP = 0, NB = 3, NPREC = 2, RS = 0, RS_stored = 0; /* system_shape() */
  int device = 0;
  ryujin_hip_comm *comm = nullptr;
  hipStream_t stream = nullptr;      /* compute */
  hipStream_t comm_stream = nullptr; /* ghost exchange, overlapped with the interior rows */
  hipEvent_t ev_comm = nullptr;
  hipStream_t launch_stream = nullptr; /* the stream the sweep lambdas launch on (stream or comm_stream) */
  FusedSadd pending_sadd{0., 0., nullptr}; /* set by time_step for the SSPRK stages, consumed by step */
  bool pending_precompute = false; /* set by time_step: the next call on the new vector is prepare_state_vector */
  hipEvent_t ev_prev = nullptr; /* compute stream -> comm_stream: everything enqueued so far */
  hipEvent_t ev_exp = nullptr;  /* comm_stream -> compute stream: the latest export part (not its exchange) */
  bool comm_pending = false;    /* comm_stream holds work the compute stream has not joined */
  bool exp_pending = false;     /* ... of which an export part later kernels on the compute stream depend on */
  bool exchange_after_exp = false; /* an exchange was enqueued behind the latest export part (ev_exp misses it) */
  StepBegin pending_begin{}; /* set by step(), carried by its first sweep (step_begin) */
  uint32_t bc_fold_max_slices = kBcFoldMaxSlices;
  uint32_t resident_waves_step5 = kResidentWavesStep5, resident_waves_step6 = kResidentWavesStep6;
  bool interior_reads_ghosts = false; /* asymmetric stencil: every sweep joins the exchanges (no overlap) */
  uint32_t n_export_slices = 0;

  SellLayout L;
  DeviceMesh mesh{};
  EulerParams eparams{};
  ShallowWaterParams swparams{};
  EulerAeosParams aeosparams{};
  ScalarParams scparams{};
  /* RYUJIN_FLUX_FUNCTION (ryujin_hip_flux_configure_function): the programs of the flux components, and what the
   * latest update ran (ryujin_hip_flux_info; host values) */
  DeviceBuffer<FluxProgram> d_flux_function;
  int flux_n_instructions = 0;
  int last_flux_kind = -1, last_flux_n_instructions = 0, last_step2_interpreted = 0;
  bool flux_interpreted_pairs() const { return scparams.flux == RYUJIN_FLUX_FUNCTION && scparams.use_averaged_entropy; }
  /* RYUJIN_EOS_FUNCTION (ryujin_hip_eos_configure_function): the four programs of the equation of state, and what
   * the latest prepare_state_vector ran (ryujin_hip_eos_info; host values) */
  DeviceBuffer<EosProgram> d_eos_function;
  int eos_n_instructions[kEosPrograms] = {0, 0, 0, 0};
  int last_eos_kind = -1, last_eos_n_instructions[kEosPrograms] = {0, 0, 0, 0}, last_precompute_interpreted = 0;
  void set_eos_function(const EosProgram &program, double b, double pinf, double q);
  DeviceBuffer<double> d_Z; /* initial_precomputed (bathymetry), shallow water only */

  template <typename E>
  const typename E::Params &eq_params() const
  {
    if constexpr (std::is_same<typename E::Params, EulerParams>::value)
      return eparams;
    else if constexpr (std::is_same<typename E::Params, EulerAeosParams>::value)
      return aeosparams;
    else if constexpr (std::is_same<typename E::Params, ScalarParams>::value)
      return scparams;
    else
      return swparams;
  }

  /* mesh arrays */
  DeviceBuffer<uint32_t> d_slice_off, d_cols, d_idx_t, d_lower_mask;
  DeviceBuffer<TileDesc> d_tiles; /* the tile map (host_layout.hpp); empty with debug_tile_map < 0 */
  DeviceBuffer<uint64_t> d_chain_loads; /* ... and the lanes of its chained tiles that fetch their node themselves */
  /* the stencil classes (host_layout.hpp); empty where no slice is uniform, in 3-D and with debug_stencil_classes < 0 */
  DeviceBuffer<uint32_t> d_slice_class;
  DeviceBuffer<uint64_t> d_class_table;
  DeviceBuffer<double> d_class_norms; /* SellLayout::class_norms; empty with debug_stencil_classes = 1 */
  DeviceBuffer<uint16_t> d_row_len;
  DeviceBuffer<double> d_cij, d_mij, d_mi, d_mi_inv;
  bool dg = false; /* discontinuous ansatz */
  DeviceBuffer<double> d_incidence, d_minv, d_bounds_combined;

  /* boundary data: the boundary map grouped by DoF (host_context.hpp) and its device copies */
  BoundaryTables bdry;
  DeviceBuffer<uint32_t> d_grp_start, d_b_i, d_bc_first;
  DeviceBuffer<unsigned long long> d_bc_mask; /* BcFold: boundary rows of every slice */
  DeviceBuffer<double> d_b_normal, d_dirichlet;
  DeviceBuffer<uint8_t> d_b_id;
  bool have_dirichlet = false;
  /* ryujin_hip_state_download_prepared: the distinct boundary_map rows (bdry.rows), packed on the device, scattered on
   * the host */
  DeviceBuffer<uint32_t> d_bc_rows;
  DeviceBuffer<double> d_bc_pack;
  double *h_bc_pack = nullptr; /* pinned */
  /* ryujin_hip_host_register: caller-owned arrays pinned in place */
  std::vector<const void *> registered_host;

  /* coupling boundary pairs (d_p_pos.n of them) */
  DeviceBuffer<uint32_t> d_p_i, d_p_j, d_p_pos;
  DeviceBuffer<double> d_p_cji;

  /* module-owned vectors and matrices */
  DeviceBuffer<double> d_alpha, d_bounds, d_r, d_dij, d_lij, d_lij_next, d_pij;
  DeviceBuffer<double> d_gamma; /* EulerAEOS: surrogate gamma_i of cycle 0, one double per node, for the stencil minimum of cycle 1 */
  DeviceBuffer<DeviceScalars> d_scalars;
  DeviceBuffer<double> d_integrals; /* ryujin_hip_state_integrals: block partials + result */
  DeviceScalars *h_scalars = nullptr; /* pinned */
  /* Postprocessor (ryujin_hip_postprocess_*, kernels_postprocessor.hpp): allocated by the first compute */
  PostprocessDesc pp_desc{};
  double pp_beta = 10.;
  bool pp_recompute_bounds = true, pp_configured = false, pp_have_bounds = false, pp_computed = false;
  DeviceBuffer<double> d_pp_raw, d_pp_normalised;  /* SoA [n_quantities][n_owned] */
  DeviceBuffer<unsigned long long> d_pp_bounds;    /* [2][kPostprocessMaxQuantities]: q_max, q_min (bit patterns) */
  template <typename E>
  void postprocess_compute(int h);
  /* Quantities (ryujin_hip_quantities_*, kernels_quantities.hpp) */
  struct Manifold {
    uint32_t n_points = 0, first = 0;
    bool contiguous = false; /* index[p] = first + p: addressed without the index stream */
    int options = 0;
    DeviceBuffer<uint32_t> d_index;
    DeviceBuffer<double> d_weight;
    DeviceBuffer<double> d_values;  /* [n_points][2 K]: (V, V o V) of the latest evaluation (val_new) */
    DeviceBuffer<double> d_sum;     /* [n_points][2 K]: val_sum, time-averaged manifolds only */
    DeviceBuffer<double> d_partial; /* [n_blocks + 1][1 + 2 K]: block partials, then the sums */
    uint32_t n_blocks = 0;
    double t_old = 0., t_new = 0., t_sum = 0.;
    bool have_values = false; /* an accumulate since the last clear */
    /* space_averaged_time_series: rows (t, mean V, mean V o V) in device chunks of kSeriesChunkRows rows; the host
     * knows the row number, so appending a row is an enqueue (and, every kSeriesChunkRows calls, an allocation) */
    std::vector<std::unique_ptr<DeviceBuffer<double>>> series;
    size_t n_rows = 0;
  };
  static constexpr size_t kSeriesChunkRows = 1024;
  std::vector<std::unique_ptr<Manifold>> manifolds;
  Manifold &manifold(int id)
  {
    if (id < 0 || id >= (int)manifolds.size())
      throw HipError(RYUJIN_ERR_ARG, "quantities: unknown manifold " + std::to_string(id));
    return *manifolds[id];
  }
  template <typename E>
  void quantities_evaluate(Manifold &m, int h, bool accumulate, double t);
  /* Error norms (ryujin_hip_error_norms_*, kernels_error_norms.hpp): the cells of this rank, transposed */
  struct ErrorNorms {
    uint32_t n_cells = 0, n_blocks = 0;
    int dofs_per_cell = 0, n_q = 0, jxw_per_cell = 0;
    DeviceBuffer<uint32_t> d_cell_dofs; /* [dofs_per_cell][n_cells] */
    DeviceBuffer<double> d_jxw;         /* [n_q][n_cells], or [n_cells] with jxw_per_cell */
    DeviceBuffer<double> d_shape, d_weights;
    DeviceBuffer<double> d_work; /* [n_blocks][kErrorNormsSums] partials, the sums, the maxima (bits), the result */
  };
  std::unique_ptr<ErrorNorms> error_norms;
  void error_norms_compute(int h_state, int h_analytic, const ErrorNormsDesc &D, double *host_result);
  /* VTUOutput (ryujin_hip_output_*, kernels_output.hpp): the requested quantities and everything the level sets select
   * on this rank's cells -- computed once, in configure */
  struct Output {
    OutputDesc desc{}; /* kinds and indices; the columns are filled in per output */
    bool needs_precomputed = false, needs_postprocessed = false;
    int n_postprocess = 0, pp_kind[kPostprocessMaxQuantities] = {}, pp_select[kPostprocessMaxQuantities] = {};
    int n_manifolds = 0, dofs_per_cell = 0;
    uint32_t n_cells = 0, n_selected_cells = 0, n_selected_nodes = 0;
    DeviceBuffer<double> d_levelsets;                          /* [n_manifolds][n_relevant] */
    DeviceBuffer<uint32_t> d_cell_ids, d_node_ids, d_connectivity; /* the selection */
    DeviceBuffer<double> d_columns;                            /* [columns][n_relevant]: alpha and postprocessed, ghosts exchanged */
    DeviceBuffer<OutputDesc> d_desc;
    DeviceBuffer<unsigned char> d_out; /* the values of one output, grown on demand */
  };
  std::unique_ptr<Output> output;
  template <typename E>
  void output_extract(Output &o, int h, bool levelsets, bool float64, void *host_out);
  /* time-dependent Dirichlet data inside a device-resident RK step (ryujin_hip_time_step_fn): the tau of the
   * first stage is copied to the host as soon as it exists (behind step 3 of the first stage), the later stages'
   * boundary data is evaluated at t + c_s tau while the rest of the first stage runs */
  static constexpr int kMaxRkStages = 5;
  unsigned long long *h_tau_early = nullptr; /* pinned */
  hipEvent_t ev_tau = nullptr;
  bool want_tau_early = false;
  double *h_dirichlet_stage[kMaxRkStages] = {}; /* pinned staging, one per RK stage */
  /* InitialValues (ryujin_hip_initial_values_*, kernels_initial_values.hpp): the configured analytic state, the
   * node positions and the boundary_map positions in the grouped order of d_b_i (bdry.permute applied once) */
  bool iv_configured = false;
  InitialValuesParams iv{};
  DeviceBuffer<double> d_iv_positions, d_iv_b_positions;
  DeviceBuffer<IvFunctionProgram> d_iv_function; /* iv.state == kIvFunction: the programs of the components */
  DeviceBuffer<double> d_iv_points, d_iv_values; /* scratch of evaluate(), grown on demand */
  /* Dirichlet data of a prepare_state_vector() evaluated on the device at t + c tau_rk (c = 0: at t) */
  struct IvStage {
    bool on;
    double t, c;
  };
  void require_initial_values() const
  {
    if (!iv_configured)
      throw HipError(RYUJIN_ERR_ARG, "initial values: not configured (ryujin_hip_initial_values_configure)");
  }
  /* f(source, program): the source of the configured state on this context (kernels_initial_values.hpp) and the
   * program its evaluator interprets, IvNoProgram where it interprets none */
  template <typename E, typename F>
  void with_initial_state_source(F &&f);
  template <typename E>
  void initial_values_points(const double *d_points, size_t n, double t, int stride, double *d_out);
  /* the bathymetry of the configured state (k_initial_precomputed), shallow water only */
  void require_initial_precomputed() const
  {
    require_initial_values();
    if (params.equation != RYUJIN_EQ_SHALLOW_WATER)
      throw HipError(RYUJIN_ERR_UNSUPPORTED, "initial values: this Description has no initial_precomputed values");
  }
  void initial_precomputed_points(const double *d_points, size_t n, double *d_out);

  struct State {
    DeviceBuffer<double> U, prec;
    DeviceBuffer<double> rrec; /* Euler, EulerAEOS, shallow water: per-node Riemann records (E::riemann_record) */
    bool used = false;
    /* prec and rrec of the owned rows belong to the U stored here, before boundary conditions (left behind by the
     * last sweep of the step that wrote U: FusedPrecompute); cleared by whatever else writes U */
    bool precomputed = false;
    /* some prepare_state_vector has run on this storage since it was handed out (ryujin_hip_output_extract) */
    bool prepared = false;
  };
  std::vector<std::unique_ptr<State>> states;

  /* exchange pattern (host_context.hpp) */
  ExchangeTables exch;
  DeviceBuffer<uint32_t> d_send_idx, d_row_send_pos;
  DeviceBuffer<double> d_send_buf;

  /* V_i = U_i^low + sum_j lambda P_ij, where step 5 leaves it (StepPlan::has_V): step 6 may take it */
  DeviceBuffer<double> d_V;
  /* what the latest update ran (step_plan.hpp). Where it stored P_ij per slice or per tile, ryujin_hip_debug_fetch
   * forms the rest from the operands in last_s0 */
  StepPlan last_plan{};
  Stage0Src last_s0{};
  /* what steps 5 and 6 of the latest update launched (ryujin_hip_debug_plan): written by the sweep lambdas next to the
   * launch itself, one record per part of the sweep (one on one rank; the export and the interior part on several).
   * Host values only. */
  struct LaunchRecord {
    uint32_t n_slices = 0, grid_y = 0;
    bool shares_slices = false;
  };
  struct LaunchLog {
    static constexpr int kParts = 2;
    int n_step5 = 0, n_step6 = 0;
    LaunchRecord step5[kParts], step6[kParts];
  } last_launches{};
  void record_step5(const DeviceMesh &mm, const uint32_t grid_y)
  {
    if (last_launches.n_step5 < LaunchLog::kParts)
      last_launches.step5[last_launches.n_step5] = LaunchRecord{mm.slice_end - mm.slice_begin, grid_y, false};
    ++last_launches.n_step5;
  }
  void record_step6(const DeviceMesh &mm, const uint32_t grid_y, const bool shares_slices)
  {
    if (last_launches.n_step6 < LaunchLog::kParts)
      last_launches.step6[last_launches.n_step6] = LaunchRecord{mm.slice_end - mm.slice_begin, grid_y, shares_slices};
    ++last_launches.n_step6;
  }
  /* SliceFlags (kernels_limiter.hpp), [n_slices] each; `unlimited` starts at 0 = "limited": the first update of a
   * context stores P_ij everywhere */
  DeviceBuffer<uint8_t> d_slice_unlimited, d_slice_first_stored, d_slice_todo;
  DeviceBuffer<uint32_t> d_slice_needed; /* SliceFlags::needed_tiles; starts as all ones: the first update stores every tile */
  DeviceBuffer<uint32_t> d_slice_next_tiles; /* SliceFlags::next_tiles: step 6 writes every word before step 7 reads it */
  /* fractions of the (sampled) slices in which the first high-order sweep found a limited pair / whose P_ij step 5
   * stored, from the device counters at the latest host synchronisation (DeviceScalars::n_sampled_*); 1 until the
   * first measurement. Diagnostics only: nothing is decided from them. */
  double limited_fraction = 1., stored_fraction = 1.;
  unsigned int seen_sampled_slices = 0, seen_sampled_limited = 0, seen_sampled_stored = 0;
  unsigned int seen_sampled_tiles = 0, seen_sampled_tiles_stored = 0;
  unsigned int seen_sampled_tiles_needed = 0, seen_sampled_tiles_formed = 0;
  double tiles_needed_fraction = 1., tiles_formed_fraction = 0.; /* of the tiles: read by step 6; formed there */
  void update_limited_fraction()
  {
    const unsigned int d_tiles = h_scalars->n_sampled_tiles - seen_sampled_tiles;
    const unsigned int d_tiles_stored = h_scalars->n_sampled_tiles_stored - seen_sampled_tiles_stored;
    seen_sampled_tiles = h_scalars->n_sampled_tiles;
    seen_sampled_tiles_stored = h_scalars->n_sampled_tiles_stored;
    const unsigned int d_slices = h_scalars->n_sampled_slices - seen_sampled_slices;
    const unsigned int d_limited = h_scalars->n_sampled_limited - seen_sampled_limited;
    const unsigned int d_stored = h_scalars->n_sampled_stored - seen_sampled_stored;
    seen_sampled_slices = h_scalars->n_sampled_slices;
    seen_sampled_limited = h_scalars->n_sampled_limited;
    seen_sampled_stored = h_scalars->n_sampled_stored;
    if (d_slices != 0) {
      limited_fraction = (double)d_limited / (double)d_slices;
      stored_fraction = last_plan.per_slice() ? (double)d_stored / (double)d_slices : 1.;
    }
    const unsigned int d_needed = h_scalars->n_sampled_tiles_needed - seen_sampled_tiles_needed;
    const unsigned int d_formed = h_scalars->n_sampled_tiles_formed - seen_sampled_tiles_formed;
    seen_sampled_tiles_needed = h_scalars->n_sampled_tiles_needed;
    seen_sampled_tiles_formed = h_scalars->n_sampled_tiles_formed;
    if (last_plan.per_tile() && d_tiles != 0) { /* (of the tiles, by step 5; step 6 adds the few it has to form itself) */
      stored_fraction = (double)d_tiles_stored / (double)d_tiles;
      tiles_needed_fraction = (double)d_needed / (double)d_tiles;
      tiles_formed_fraction = (double)d_formed / (double)d_tiles;
    }
  }
  void ensure_pij()
  {
    if (d_pij.n == 0)
      d_pij.alloc(L.nnz_total * (size_t)K);
  }
  template <typename E>
  void store_pij_for_debug();

  unsigned n_restarts = 0, n_warnings = 0;
  unsigned long long n_exchanges = 0, n_allreduces = 0; /* ryujin_hip_exchange_info */

  /* profiling */
  bool timers_enabled = false;
  /* device-resident RK driver: per-step host synchronisation is deferred to the end of the RK step */
  bool deferred = false;
  int rk_stage = 0; /* selects the event set while deferred */
  double sweep_ms_accum[8] = {};
  unsigned sweep_updates_accum = 0;
  hipEvent_t ev_rk[5][9] = {};
  hipEvent_t ev[9] = {};
  hipEvent_t ev_user[2] = {};
  double sweep_ms[8] = {};

  ~ryujin_hip_ctx()
  {
    if (stream)
      (void)hipStreamSynchronize(stream);
    if (comm_stream) {
      (void)hipStreamSynchronize(comm_stream);
      (void)hipStreamDestroy(comm_stream);
    }
    if (ev_prev)
      (void)hipEventDestroy(ev_prev);
    if (ev_exp)
      (void)hipEventDestroy(ev_exp);
    if (ev_comm)
      (void)hipEventDestroy(ev_comm);
    for (auto &e : ev)
      if (e)
        (void)hipEventDestroy(e);
    for (auto &set : ev_rk)
      for (auto &e : set)
        if (e)
          (void)hipEventDestroy(e);
    for (auto &e : ev_user)
      if (e)
        (void)hipEventDestroy(e);
    if (h_scalars)
      (void)hipHostFree(h_scalars);
    if (h_bc_pack)
      (void)hipHostFree(h_bc_pack);
    for (const void *ptr : registered_host)
      (void)hipHostUnregister(const_cast<void *>(ptr));
    if (h_tau_early)
      (void)hipHostFree(h_tau_early);
    if (ev_tau)
      (void)hipEventDestroy(ev_tau);
    for (auto *b : h_dirichlet_stage)
      if (b)
        (void)hipHostFree(b);
    if (stream)
      (void)hipStreamDestroy(stream);
  }

  State &state(int h)
  {
    if (h < 0 || h >= (int)states.size() || !states[h] || !states[h]->used)
      throw HipError(RYUJIN_ERR_ARG, "invalid state handle " + std::to_string(h));
    return *states[h];
  }

  void create(const ryujin_hip_offline &o, const ryujin_hip_params &p, ryujin_hip_comm *c, int dev);
  void exchange_vector(double *v, int stride, bool after_split_sweep);
  void exchange_matrix(double *m, bool after_split_sweep);
  unsigned long local_exchanges = 0, local_reduces = 0; /* in-process transport: generation counters */
  void local_before_pack();
  void local_exchange(double *base, const std::vector<size_t> &send_offset,
                      const std::vector<size_t> &recv_offset, const std::vector<size_t> &recv_count);
  void allreduce_scalar(void *dev_ptr, int op, int count = 1);
  /* more than one rank whose values differ: not the loopback group, which stands for all of its ranks itself */
  bool several_ranks() const { return comm && comm->n_ranks > 1 && !(comm->local && comm->local->loopback); }
  bool reduce_over_ranks(double *dev, std::initializer_list<RankReduceSegment> segments, bool counted = true);
  void wait_comm();
  void join_export();
  void finish();
  void begin_exchange(bool after_split_sweep);
  void end_exchange();
  template <typename F>
  void sweep(F &&launch);
  template <typename E>
  void prepare_state_vector(int h, const double *dirichlet, IvStage iv_stage = IvStage{false, 0., 0.});
  template <typename E>
  int step(int h_old, int stages, const int *h_stage, const double *w, int h_new, double tau_in,
           double tau_max_in, double *tau_out);
  /* ... and its stages: each launches what the plan names */
  template <int DIM>
  struct StepArgs {
    State &old, &nw;
    StageArgs<DIM> S{};
    double weight = 1.;
    SliceFlags slice_flags{}, tile_flags{};
    FusedSadd fused_sadd{0., 0., nullptr}; /* applied by the last sweep */
    FusedPrecompute fused_prec{nullptr, nullptr};
  };
  template <typename E>
  StepPlanInput plan_input(int stages) const;
  template <typename E>
  void step2_dij_alpha(const StepPlan &plan, const State &old);
  template <typename E>
  void step3_diagonal_tau(const StepPlan &plan, const State &old);
  void ensure_limiter_buffers(const StepPlan &plan);
  template <typename E>
  void step4_low_order(const StepPlan &plan, const StepArgs<E::DIMENSION> &a);
  template <typename E>
  void step5_limiter(const StepPlan &plan, const StepArgs<E::DIMENSION> &a);
  template <typename E>
  void step6_high_order_next(const StepPlan &plan, const StepArgs<E::DIMENSION> &a);
  template <typename E>
  void step7_high_order_last(const StepPlan &plan, const StepArgs<E::DIMENSION> &a);
  int finish_step(double *tau_out);
  template <typename E>
  int time_step(int scheme, int h_state, int n_tmp, const int *h_tmp, const double *dirichlet,
                double tau_max, int cfl_recovery, double cfl_min, double cfl_max, double *tau_out,
                double t = 0., ryujin_hip_dirichlet_fn dirichlet_fn = nullptr, void *dirichlet_user = nullptr,
                bool dirichlet_on_device = false);
  void mark(int k)
  {
    if (timers_enabled)
      HIP_CHECK(hipEventRecord(deferred ? ev_rk[rk_stage][k] : ev[k], stream));
  }
};

/* Check, derive, create, upload: the host tables come from host_context.hpp, one call each; nothing touches the device
 * before every argument has passed. */
void ryujin_hip_ctx::create(const ryujin_hip_offline &o, const ryujin_hip_params &p,
                            ryujin_hip_comm *c, int dev)
{
  check_create_arguments(o, p, c != nullptr);
  params = p;
  comm = c;
  device = dev;
  dim = p.dim;
  const SystemShape shape = system_shape(p.equation, dim);
  K = shape.K;
  KP = shape.KP;
  NB = shape.NB;
  NPREC = shape.NPREC;
  RS = shape.RS;
  RS_stored = shape.RS_stored;
  dg = o.discontinuous_ansatz != 0;

  /* ---- streams and events -------------------------------------------------- */
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  HIP_CHECK(hipStreamCreateWithFlags(&comm_stream, hipStreamNonBlocking));
  launch_stream = stream;
  create_device_event(&ev_prev, p.system_scope_events != 0);
  create_device_event(&ev_exp, p.system_scope_events != 0);
  create_device_event(&ev_comm, p.system_scope_events != 0);
  for (auto &e : ev)
    HIP_CHECK(hipEventCreate(&e));
  for (auto &set : ev_rk)
    for (auto &e : set)
      HIP_CHECK(hipEventCreate(&e));
  for (auto &e : ev_user)
    HIP_CHECK(hipEventCreate(&e));
  HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&h_scalars), sizeof(DeviceScalars)));

  /* ---- parameter blocks ---------------------------------------------------- */
  eparams = make_euler_params(p);
  aeosparams = make_aeos_params(p);

  scparams.flux = p.sc_flux;
  scparams.use_greedy_wavespeed = p.sc_use_greedy_wavespeed != 0;
  scparams.use_averaged_entropy = p.sc_use_averaged_entropy != 0;
  for (int d = 0; d < 3; ++d)
    for (int n = 0; n < 4; ++n)
      scparams.poly[d][n] = p.sc_flux_polynomial[d][n];
  /* flux.h:33-34; the "function" flux reads its own parameter (flux_function.h:40-44) */
  scparams.delta = p.sc_flux == RYUJIN_FLUX_POLYNOMIAL || p.sc_flux == RYUJIN_FLUX_FUNCTION
                       ? p.sc_derivative_approximation_delta
                       : 1.e4 * std::numeric_limits<double>::epsilon();
  if (p.equation == RYUJIN_EQ_SCALAR_CONSERVATION && p.sc_flux == RYUJIN_FLUX_FUNCTION) {
    /* the default expression of flux_function.h:32, in every direction (as "burgers"), until
     * ryujin_hip_flux_configure_function replaces it */
    static const char *const defaults[3] = {"0.5*u*u", "0.5*u*u; 0.5*u*u", "0.5*u*u; 0.5*u*u; 0.5*u*u"};
    auto program = std::make_unique<FluxProgram>();
    std::string error;
    if (const int status = flux_compile(defaults[dim - 1], dim, *program, error))
      throw HipError(status, error);
    d_flux_function.upload(program.get(), 1);
    flux_n_instructions = program->n_instructions;
  }
  scparams.evc_factor = p.indicator_evc_factor;
  scparams.lim_relaxation_factor = p.limiter_relaxation_factor;

  if (p.equation == RYUJIN_EQ_EULER_AEOS && p.eos == RYUJIN_EOS_FUNCTION) {
    /* the defaults of equation_of_state_function.h:32-53 (the polytropic gas with 1.4, interpolation parameters 0),
     * until ryujin_hip_eos_configure_function replaces them */
    auto program = std::make_unique<EosProgram>();
    std::string error;
    if (const int status = eos_compile(nullptr, 0., 0., 0., *program, error))
      throw HipError(status, error);
    set_eos_function(*program, 0., 0., 0.);
  }

  swparams = make_sw_params(p);
  if (p.equation == RYUJIN_EQ_SHALLOW_WATER) {
    if (o.initial_precomputed)
      d_Z.upload(o.initial_precomputed, o.n_relevant);
    else
      d_Z.alloc(o.n_relevant); /* flat bed */
  }

  /* ---- stencil ------------------------------------------------------------- */
  L.build(o);
  d_slice_off.upload(L.slice_off);
  d_row_len.upload(L.row_len);
  d_cols.upload(L.cols);
  d_idx_t.upload(L.idx_t);
  if (p.debug_tile_map >= 0) { /* (3-D sweeps keep streaming the explicit indices, tile_map_pays(); they use the chain codes) */
    L.build_tiles();
    d_tiles.upload(L.tiles);
    d_chain_loads.upload(L.chain_loads);
  }
  if (p.debug_stencil_classes >= 0 && stencil_classes_pay(dim)) {
    L.build_stencil_classes(o, dim);
    if (L.n_uniform_slices != 0) {
      d_slice_class.upload(L.slice_class);
      d_class_table.upload(L.class_table);
      if (p.debug_stencil_classes != 1) /* 1: the classes without the table of norms (A/B) */
        d_class_norms.upload(L.class_norms);
    }
  }
  d_lower_mask.upload(lower_mask(L));
  {
    const auto cij = L.scatter(o, o.cij, (uint32_t)dim);
    d_cij.upload(cij);
    d_mij.upload(L.scatter(o, o.mij, 1));
    if (dg) {
      d_incidence.upload(L.scatter(o, o.incidence, 1));
      d_minv.upload(L.scatter(o, o.mass_matrix_inverse, 1));
    }
    const PairTables pairs = build_pair_tables(o, L, cij, dim);
    d_p_i.upload(o.p_i, o.n_pairs);
    d_p_j.upload(o.p_j, o.n_pairs);
    d_p_pos.upload(pairs.pos);
    d_p_cji.upload(pairs.cji);
  }
  d_mi.upload(o.mi, o.n_relevant);
  d_mi_inv.upload(o.mi_inv, o.n_relevant);

  /* ---- boundary map, grouped by DoF ---------------------------------------- */
  bdry = build_boundary_tables(o, L, dim);
  d_bc_mask.upload(bdry.bc_mask);
  d_bc_first.upload(bdry.bc_first);
  d_grp_start.upload(bdry.grp_start);
  d_b_i.upload(bdry.b_i);
  d_b_normal.upload(bdry.b_normal);
  d_b_id.upload(bdry.b_id);
  d_dirichlet.alloc((size_t)bdry.n_bdry * K);

  /* ---- the mesh as the kernels see it -------------------------------------- */
  const MeshKnobs knobs = mesh_knobs(p, L, dim, RYUJIN_XCD_CHUNK_3D, kWavesPerBlock);
  mesh.n_owned = L.n_owned;
  mesh.n_relevant = L.n_relevant;
  mesh.n_slices = L.n_slices;
  mesh.bounds_stride = knobs.bounds_stride;
  mesh.slice_begin = 0;
  mesh.slice_end = L.n_slices;
  mesh.slice_off = d_slice_off.ptr;
  mesh.row_len = d_row_len.ptr;
  mesh.cols = d_cols.ptr;
  mesh.idx_t = d_idx_t.ptr;
  mesh.tiles = d_tiles.n != 0 ? d_tiles.ptr : nullptr;
  mesh.chain_loads = d_chain_loads.n != 0 ? d_chain_loads.ptr : nullptr;
  mesh.slice_class = d_slice_class.n != 0 ? d_slice_class.ptr : nullptr;
  mesh.class_table = d_class_table.n != 0 ? reinterpret_cast<const StencilClassEntry *>(d_class_table.ptr) : nullptr;
  mesh.class_norms = d_class_norms.n != 0 ? d_class_norms.ptr : nullptr;
  mesh.tail_queue_columns = knobs.tail_queue_columns;
  mesh.band_stride = knobs.band_stride;
  mesh.xcd_chunk = knobs.xcd_chunk;
  mesh.cij = d_cij.ptr;
  mesh.mij = d_mij.ptr;
  mesh.incidence = dg ? d_incidence.ptr : nullptr;
  mesh.mass_matrix_inverse = dg ? d_minv.ptr : nullptr;
  mesh.mi = d_mi.ptr;
  mesh.mi_inv = d_mi_inv.ptr;
  mesh.measure_of_omega_inverse = 1. / o.measure_of_omega;

  /* ---- the choreography of the ghost exchange ------------------------------ */
  n_export_slices = ryujin_hip::n_export_slices(o, L);
  /* test hooks (ryujin_hip_params::debug_*; tests/test_gpu_parity.py runs the partitioned cases through both
   * branches of each): force the fallback choreography / move the mesh size below which boundary conditions
   * ride on the pre-pass / small meshes run the kernels of the large ones */
  interior_reads_ghosts = interior_rows_read_ghosts(L, n_export_slices) || p.debug_join_exchanges != 0;
  if (p.debug_bc_fold_max_slices != 0)
    bc_fold_max_slices = p.debug_bc_fold_max_slices < 0 ? 0u : (uint32_t)p.debug_bc_fold_max_slices;
  if (p.debug_no_small_mesh_split != 0)
    resident_waves_step5 = resident_waves_step6 = 0;

  /* ---- module-owned storage (prepare(): hyperbolic_module.template.h:52-86) ---- */
  d_alpha.alloc(L.n_relevant);
  if (params.equation == RYUJIN_EQ_EULER_AEOS)
    d_gamma.alloc(L.n_relevant);
  d_bounds.alloc((size_t)NB * mesh.bounds_stride);
  if (dg)
    d_bounds_combined.alloc((size_t)NB * mesh.bounds_stride);
  d_r.alloc((size_t)L.n_relevant * KP);
  d_dij.alloc(L.nnz_total);
  d_lij.alloc(L.nnz_total);
  d_lij_next.alloc(L.nnz_total);
  /* (p_ij is allocated by the first step: ensure_pij) */
  d_scalars.alloc(1);

  /* ---- exchange pattern ---- */
  exch = build_exchange_tables(o, L, KP, NPREC);
  if (exch.n_nbr > 0) {
    d_send_idx.upload(o.send_idx, exch.send_off[exch.n_nbr]);
    d_row_send_pos.upload(exch.row_send_pos);
    d_send_buf.alloc(exch.send_buffer_doubles);
  }
  HIP_CHECK(hipStreamSynchronize(stream));
}

/* ---- stream choreography of the ghost exchange ------------------------------------------------
 * Two streams. Every sweep runs as two launches: the few export slices (the rows other ranks hold as
 * ghosts = the only rows that couple to ghost columns) on comm_stream, the interior slices on the compute
 * stream. Exchanges (pack + RCCL send/recv, or the in-process copies) follow the export launch that
 * produced their data in stream order on comm_stream -- the reference's SynchronizationDispatch idea
 * (source/openmp.h:141-183), taken one step further: no SWEEP on the compute stream ever waits for an
 * exchange (the scalar all-reduces do, see allreduce_scalar). Dependencies:
 *   export part N      needs interior parts <= N-1 (ev_prev: compute -> comm), export parts and
 *                      exchanges <= N-1 (stream order on comm_stream)
 *   interior part N    needs export parts <= N-1 (ev_exp: comm -> compute, recorded BEFORE exchange N-1),
 *                      interior parts <= N-1 (stream order); never ghost data
 *   exchange N         needs export part N only (stream order)
 * so an exchange has the whole interior launch of the NEXT sweep as well to hide behind, and a short sweep
 * (the pre-pass, 30 us in 2-D) no longer exposes the latency of the exchange in front of it. Kernels outside
 * sweep() that touch export rows (boundary conditions, boundary d_ij) call join_export(); whoever reads the
 * ghost range on the compute stream or on the host, and the scalar all-reduces (one communicator: RCCL orders
 * them behind the exchanges anyway), call wait_comm().
 * (Round 2 started with a third stream for the export part and a join of every exchange in front of the next
 * sweep: +11 % per update on a middle rank in 2-D without any network in the loop, profiles/r02k_*.) */
void ryujin_hip_ctx::wait_comm()
{
  if (comm_pending) {
    HIP_CHECK(hipEventRecord(ev_comm, comm_stream)); /* the tail of comm_stream as of now */
    HIP_CHECK(hipStreamWaitEvent(stream, ev_comm, 0));
    comm_pending = false;
    exp_pending = false;
    exchange_after_exp = false;
  }
}

void ryujin_hip_ctx::join_export()
{
  if (interior_reads_ghosts) {
    wait_comm();
    return;
  }
  if (exp_pending) {
    HIP_CHECK(hipStreamWaitEvent(stream, ev_exp, 0));
    exp_pending = false;
  }
}

/* dynamic LDS of k_pij_lij: the queue of undecided pairs, (widest row - 1) columns of 64 two-byte entries per wave */
static inline size_t tail_queue_bytes(const DeviceMesh &mm)
{
  return (size_t)kWavesPerBlock * mm.tail_queue_columns * 64u * sizeof(uint16_t);
}

void ryujin_hip_ctx::finish()
{
  wait_comm();
  HIP_CHECK(hipStreamSynchronize(stream));
}

/* exchange of data the compute stream produced outside a sweep (the state vector behind the boundary
 * conditions); after a sweep the export part already sits on comm_stream */
void ryujin_hip_ctx::begin_exchange(bool after_split_sweep)
{
  if (after_split_sweep)
    return;
  HIP_CHECK(hipEventRecord(ev_prev, stream)); /* everything enqueued so far */
  HIP_CHECK(hipStreamWaitEvent(comm_stream, ev_prev, 0));
}

void ryujin_hip_ctx::end_exchange()
{
  ++n_exchanges;
  comm_pending = true;
  exchange_after_exp = true;
}

template <typename F>
void ryujin_hip_ctx::sweep(F &&launch)
{
  auto run = [&](uint32_t s0, uint32_t s1, hipStream_t on) {
    if (s1 <= s0)
      return;
    DeviceMesh mm = mesh;
    mm.begin = pending_begin;
    mm.slice_begin = s0;
    mm.slice_end = s1;
    /* one wave per slice, 4 slices per block (waves beyond slice_end return at once) */
    const dim3 grid((s1 - s0 + kWavesPerBlock - 1) / kWavesPerBlock);
    launch_stream = on;
    launch(mm, grid);
    launch_stream = stream;
  };
  struct Consume { /* the start of a step rides on one sweep only */
    StepBegin &b;
    ~Consume() { b = StepBegin{}; }
  } consume{pending_begin};
  if (exch.n_nbr == 0) {
    run(0, L.n_slices, stream);
    return;
  }
  join_export();
  HIP_CHECK(hipEventRecord(ev_prev, stream));
  HIP_CHECK(hipStreamWaitEvent(comm_stream, ev_prev, 0));
  run(0, n_export_slices, comm_stream);
  HIP_CHECK(hipEventRecord(ev_exp, comm_stream));
  exp_pending = true;
  comm_pending = true;
  exchange_after_exp = false; /* stream order: ev_exp covers every exchange enqueued so far */
  run(n_export_slices, L.n_slices, stream);
}

/* in-process transport, part 1 (before the pack kernel): the send buffer may only be overwritten once
 * every neighbour has pulled the segments of the previous exchange */
void ryujin_hip_ctx::local_before_pack()
{
  LocalGroup &g = *comm->local;
  const unsigned long x = local_exchanges;
  if (x == 0)
    return;
  for (int q = 0; q < exch.n_nbr; ++q) {
    const int peer = g.loopback ? comm->rank : exch.nbr_rank[q];
    g.await(g.pulled, peer, x);
    HIP_CHECK(hipStreamWaitEvent(comm_stream,
                                 g.ev_pulled[(size_t)peer * LocalGroup::kRing + (x - 1) % LocalGroup::kRing], 0));
  }
}

/* part 2 (behind the pack kernel): publish the per-neighbour segments of the send buffer behind an event,
 * pull the neighbours' segments behind theirs. Stream ordered throughout, see LocalGroup. */
void ryujin_hip_ctx::local_exchange(double *base, const std::vector<size_t> &send_offset,
                                    const std::vector<size_t> &recv_offset,
                                    const std::vector<size_t> &recv_count)
{
  LocalGroup &g = *comm->local;
  const unsigned long x = local_exchanges;
  const size_t slot = x % LocalGroup::kRing;
  const int me = comm->rank;
  for (int q = 0; q < exch.n_nbr; ++q)
    g.mail[me][exch.nbr_rank[q]] = d_send_buf.ptr + send_offset[q];
  HIP_CHECK(hipEventRecord(g.ev_packed[(size_t)me * LocalGroup::kRing + slot], comm_stream));
  g.publish(g.packed, me, x + 1);
  for (int q = 0; q < exch.n_nbr; ++q) {
    const int peer = g.loopback ? me : exch.nbr_rank[q];
    g.await(g.packed, peer, x + 1);
    HIP_CHECK(hipStreamWaitEvent(comm_stream, g.ev_packed[(size_t)peer * LocalGroup::kRing + slot], 0));
    /* loopback: what the neighbour on the other side would have received from me */
    const double *src = g.loopback ? g.mail[me][exch.nbr_rank[exch.n_nbr - 1 - q]] : g.mail[exch.nbr_rank[q]][me];
    if (recv_count[q])
      HIP_CHECK(hipMemcpyAsync(base + recv_offset[q], src, recv_count[q] * sizeof(double),
                               hipMemcpyDeviceToDevice, comm_stream));
  }
  HIP_CHECK(hipEventRecord(g.ev_pulled[(size_t)me * LocalGroup::kRing + slot], comm_stream));
  g.publish(g.pulled, me, x + 1);
  ++local_exchanges;
}

/* 1-element all-reduce on a device scalar; op: 0 = min (double), 1 = max (int) */
void ryujin_hip_ctx::allreduce_scalar(void *dev_ptr, int op, int count)
{
  if (!comm || comm->n_ranks <= 1)
    return;
  /* The scalar is written by export parts as well, and ONE communicator serves both streams: RCCL orders the
   * operations of a communicator in issue order whatever stream they are enqueued on, so an all-reduce on the
   * compute stream implicitly waits for the point-to-point exchanges issued before it. The join is therefore
   * made explicit -- for BOTH transports, so that the in-process transport the partitioned parity tests (and
   * scripts/overhead_loopback.py) run has exactly the dependency graph of the RCCL leg. This is the one place
   * where the compute stream waits for an exchange: the exchange of alpha in front of the tau_max reduction
   * of the first stage, enqueued behind the export part of step 2 and long finished when step 3 retires (two
   * interior launches later), and whatever is in flight at the end of a step / of a Runge-Kutta step. */
  wait_comm();
  ++n_allreduces;
  if (!comm->local) {
    if (op == 0)
      NCCL_CHECK(ncclAllReduce(dev_ptr, dev_ptr, 1, ncclDouble, ncclMin, comm->comm, stream));
    else
      NCCL_CHECK(ncclAllReduce(dev_ptr, dev_ptr, count, ncclInt, ncclMax, comm->comm, stream));
    return;
  }
  /* in-process transport: slot write -> event -> wait for everybody's event -> slot reduce, all on the
   * compute stream (see LocalGroup) */
  LocalGroup &g = *comm->local;
  const unsigned long a = local_reduces;
  const size_t par = a & 1;
  const int me = comm->rank;
  unsigned long long *slots = g.slots + par * (size_t)g.n_ranks * 2;
  hipLaunchKernelGGL(k_slot_write, dim3(1), dim3(1), 0, stream, dev_ptr, op, count, slots + (size_t)me * 2);
  HIP_CHECK(hipEventRecord(g.ev_reduced[(size_t)me * LocalGroup::kRing + par], stream));
  g.publish(g.reduced, me, a + 1);
  for (int q = 0; q < g.n_ranks && !g.loopback; ++q) {
    if (q == me)
      continue;
    g.await(g.reduced, q, a + 1);
    HIP_CHECK(hipStreamWaitEvent(stream, g.ev_reduced[(size_t)q * LocalGroup::kRing + par], 0));
  }
  if (g.loopback) /* reduce over my own slot only */
    hipLaunchKernelGGL(k_slot_reduce, dim3(1), dim3(1), 0, stream, slots + (size_t)me * 2, 1, op, count, dev_ptr);
  else
    hipLaunchKernelGGL(k_slot_reduce, dim3(1), dim3(1), 0, stream, slots, g.n_ranks, op, count, dev_ptr);
  ++local_reduces;
}

/* A few device doubles reduced over the ranks, segment by segment, the same bits on every rank; false (and nothing
 * enqueued) where there is nothing to reduce over. RCCL: one stream-ordered all-reduce per segment, counted as one.
 * In-process transport: through the host (HostRendezvous::reduce), the stream drained before and behind. No join
 * with the comm stream: the callers make it where they need one. */
bool ryujin_hip_ctx::reduce_over_ranks(double *dev, std::initializer_list<RankReduceSegment> segments, bool counted)
{
  if (!several_ranks())
    return false;
  if (!comm->local) {
    if (counted)
      ++n_allreduces;
    for (const RankReduceSegment &s : segments) {
      const ncclRedOp_t op = s.op == RankReduceOp::Sum ? ncclSum : (s.op == RankReduceOp::Max ? ncclMax : ncclMin);
      NCCL_CHECK(ncclAllReduce(dev, dev, s.count, ncclDouble, op, comm->comm, stream));
      dev += s.count;
    }
    return true;
  }
  int n = 0;
  for (const RankReduceSegment &s : segments)
    n += s.count;
  double host[kRankReduceMaxValues];
  if (n > kRankReduceMaxValues)
    throw HipError(RYUJIN_ERR_ARG, "reduce_over_ranks: row too long");
  HIP_CHECK(hipMemcpyAsync(host, dev, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  comm->local->reduce(comm->rank, host, n, segments);
  HIP_CHECK(hipMemcpyAsync(dev, host, sizeof(double) * n, hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipStreamSynchronize(stream)); /* host[] goes out of scope */
  return true;
}

void ryujin_hip_ctx::exchange_vector(double *v, int stride, bool after_split_sweep)
{
  if (exch.n_nbr == 0)
    return;
  begin_exchange(after_split_sweep);
  if (comm->local)
    local_before_pack();
  const uint32_t n_send = exch.send_off[exch.n_nbr];
  hipLaunchKernelGGL(k_pack_vector, dim3(grid_for((size_t)n_send * stride)), dim3(kBlock), 0, comm_stream,
                     n_send, d_send_idx.ptr, stride, v, d_send_buf.ptr);
  if (comm->local) {
    std::vector<size_t> off(exch.n_nbr), dst(exch.n_nbr), rcnt(exch.n_nbr);
    for (int q = 0; q < exch.n_nbr; ++q) {
      off[q] = (size_t)exch.send_off[q] * stride;
      dst[q] = (size_t)exch.recv_off[q] * stride;
      rcnt[q] = (size_t)(exch.recv_off[q + 1] - exch.recv_off[q]) * stride;
    }
    local_exchange(v, off, dst, rcnt);
    end_exchange();
    return;
  }
  NCCL_CHECK(ncclGroupStart());
  for (int q = 0; q < exch.n_nbr; ++q) {
    NCCL_CHECK(ncclSend(d_send_buf.ptr + (size_t)exch.send_off[q] * stride,
                        (size_t)(exch.send_off[q + 1] - exch.send_off[q]) * stride, ncclDouble, exch.nbr_rank[q],
                        comm->comm, comm_stream));
    NCCL_CHECK(ncclRecv(v + (size_t)exch.recv_off[q] * stride,
                        (size_t)(exch.recv_off[q + 1] - exch.recv_off[q]) * stride, ncclDouble, exch.nbr_rank[q],
                        comm->comm, comm_stream));
  }
  NCCL_CHECK(ncclGroupEnd());
  end_exchange();
}

void ryujin_hip_ctx::exchange_matrix(double *m, bool after_split_sweep)
{
  if (exch.n_nbr == 0)
    return;
  begin_exchange(after_split_sweep);
  if (comm->local)
    local_before_pack();
  const uint32_t n_send = exch.row_send_off[exch.n_nbr];
  hipLaunchKernelGGL(k_pack_matrix, dim3(grid_for(n_send)), dim3(kBlock), 0, comm_stream, n_send,
                     d_row_send_pos.ptr, m, d_send_buf.ptr);
  if (comm->local) {
    std::vector<size_t> off(exch.n_nbr), dst(exch.n_nbr), rcnt(exch.n_nbr);
    for (int q = 0; q < exch.n_nbr; ++q) {
      off[q] = exch.row_send_off[q];
      dst[q] = L.nnz_sell + exch.row_recv_off[q];
      rcnt[q] = exch.row_recv_off[q + 1] - exch.row_recv_off[q];
    }
    local_exchange(m, off, dst, rcnt);
    end_exchange();
    return;
  }
  NCCL_CHECK(ncclGroupStart());
  for (int q = 0; q < exch.n_nbr; ++q) {
    NCCL_CHECK(ncclSend(d_send_buf.ptr + exch.row_send_off[q], exch.row_send_off[q + 1] - exch.row_send_off[q],
                        ncclDouble, exch.nbr_rank[q], comm->comm, comm_stream));
    NCCL_CHECK(ncclRecv(m + L.nnz_sell + exch.row_recv_off[q], exch.row_recv_off[q + 1] - exch.row_recv_off[q],
                        ncclDouble, exch.nbr_rank[q], comm->comm, comm_stream));
  }
  NCCL_CHECK(ncclGroupEnd());
  end_exchange();
}

/* the caller has waited for the streams: nothing enqueued may still read the earlier programs */
void ryujin_hip_ctx::set_eos_function(const EosProgram &program, const double b, const double pinf, const double q)
{
  d_eos_function.upload(&program, 1);
  for (int w = 0; w < kEosPrograms; ++w)
    eos_n_instructions[w] = program.n_instructions(w);
  aeosparams.eos = RYUJIN_EOS_FUNCTION;
  aeosparams.b = b;
  aeosparams.pinf = pinf;
  aeosparams.q = q;
  iv.eos = RYUJIN_EOS_FUNCTION; /* an analytic state configured earlier goes through the sie program from now on */
  for (auto &s : states)
    if (s)
      s->precomputed = false;
}

template <typename E>
void ryujin_hip_ctx::store_pij_for_debug()
{
  finish();
  DeviceMesh mm = mesh;
  mm.begin = StepBegin{};
  mm.slice_begin = 0;
  mm.slice_end = L.n_slices;
  const dim3 grid((L.n_slices + kWavesPerBlock - 1) / kWavesPerBlock), block(kBlock);
  hipLaunchKernelGGL(k_pij_stage0_store<E>, grid, block, 0, stream, mm, last_s0, d_pij.ptr,
                     last_plan.per_slice() ? (const uint8_t *)d_slice_first_stored.ptr : (const uint8_t *)nullptr);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(stream));
}

/* initial_precomputations(affine_transform(point)) of the configured state, one thread per point, on the compute
 * stream: into a caller's buffer, or at the node positions into the context's bathymetry */
void ryujin_hip_ctx::initial_precomputed_points(const double *d_points, size_t n, double *d_out)
{
  if (n == 0)
    return;
  const dim3 grid(grid_for(n, kInitialValuesBlock)), block(kInitialValuesBlock);
  if (dim == 1)
    hipLaunchKernelGGL(k_initial_precomputed<1>, grid, block, 0, stream, iv, (uint32_t)n, d_points, d_out);
  else
    hipLaunchKernelGGL(k_initial_precomputed<2>, grid, block, 0, stream, iv, (uint32_t)n, d_points, d_out);
  HIP_CHECK(hipGetLastError());
}

/* Which evaluator the configured state gets on a context of Description E: the one place that decides it, for the
 * points and for the Dirichlet kernel alike. */
template <typename E, typename F>
void ryujin_hip_ctx::with_initial_state_source(F &&f)
{
  constexpr int DIM = E::DIMENSION;
  if (iv_is_bathymetry_state(iv.state)) {
    /* the states of initial_states_bathymetry_device.hpp */
    if constexpr (std::is_same<typename E::Params, ShallowWaterParams>::value)
      f(IvBathymetrySource<DIM>{}, IvNoProgram{});
    else
      throw HipError(RYUJIN_ERR_ARG, "initial values: the Description of this context has no such state");
  } else if (iv.state == kIvFunction) {
    f(IvFunctionSource<E>{}, d_iv_function.ptr);
  } else if constexpr (is_scalar_v<E>) {
    throw HipError(RYUJIN_ERR_UNSUPPORTED, "initial values: scalar conservation has the function state only");
  } else {
    /* the states of initial_states_library_device.hpp, or the analytic ones */
    const bool library = iv_is_library_state(iv.state);
    if constexpr (std::is_same<typename E::Params, EulerAeosParams>::value) {
      if (aeosparams.eos == RYUJIN_EOS_FUNCTION) {
        /* through the sie program of the function equation of state */
        if (library)
          f(IvLibraryEosFunctionSource<DIM>{}, d_eos_function.ptr);
        else
          f(IvEosFunctionSource<DIM>{}, d_eos_function.ptr);
        return;
      }
    }
    if (library)
      f(IvLibrarySource<E>{}, IvNoProgram{});
    else
      f(IvAnalyticSource<E>{}, IvNoProgram{});
  }
}

/* one thread per point (k_initial_state_points) on the compute stream */
template <typename E>
void ryujin_hip_ctx::initial_values_points(const double *d_points, size_t n, double t, int stride, double *d_out)
{
  if (n == 0)
    return;
  with_initial_state_source<E>([&](auto source, auto program) {
    hipLaunchKernelGGL(k_initial_state_points<decltype(source)>, dim3(grid_for(n, kInitialValuesBlock)),
                       dim3(kInitialValuesBlock), 0, stream, iv, program, (uint32_t)n, d_points, t, stride, d_out);
  });
  HIP_CHECK(hipGetLastError());
}

template <typename E>
void ryujin_hip_ctx::prepare_state_vector(int h, const double *dirichlet, IvStage iv_stage)
{
  const auto &eparams = eq_params<E>(); /* shadows the member: the equation's parameter block */
  State &s = state(h);
  s.prepared = true;
  const dim3 block(kBlock);
  if (iv_stage.on && bdry.n_bdry && bdry.needs_dirichlet) {
    /* initial_state(position, t + c tau) of every boundary_map entry, evaluated where the data is read: behind
     * every kernel of the previous stage that read the buffer (compute stream order; the export part of the previous
     * pre-pass may have applied boundary conditions on comm_stream) and behind the step-4 kernel of the first stage,
     * which left tau_rk. Nothing on the host waits for tau. */
    with_initial_state_source<E>([&](auto source, auto program) {
      join_export();
      hipLaunchKernelGGL(k_initial_state_dirichlet<decltype(source)>, dim3(grid_for(bdry.n_bdry, kInitialValuesBlock)),
                         dim3(kInitialValuesBlock), 0, stream, iv, program, bdry.n_bdry, d_iv_b_positions.ptr,
                         d_b_id.ptr, iv_stage.t, iv_stage.c, d_scalars.ptr, d_dirichlet.ptr);
    });
    HIP_CHECK(hipGetLastError());
    have_dirichlet = true;
  } else if (dirichlet && bdry.n_bdry) {
    /* permute into the grouped order, then upload */
    if (deferred) {
      /* inside a device-resident RK step: a pinned staging buffer per stage, no host synchronisation (a buffer
       * is rewritten in the next RK step at the earliest, i.e. behind the end-of-step synchronisation). The
       * copy is ordered on the compute stream behind every kernel of the previous stage that read the data. */
      double *&buf = h_dirichlet_stage[rk_stage];
      if (!buf)
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&buf), (size_t)bdry.n_bdry * K * sizeof(double)));
      bdry.permute(dirichlet, K, buf);
      join_export(); /* the export part of the previous pre-pass may have applied boundary conditions */
      HIP_CHECK(hipMemcpyAsync(d_dirichlet.ptr, buf, (size_t)bdry.n_bdry * K * sizeof(double), hipMemcpyHostToDevice,
                               stream));
    } else {
      std::vector<double> tmp((size_t)bdry.n_bdry * K);
      bdry.permute(dirichlet, K, tmp.data());
      HIP_CHECK(hipMemcpyAsync(d_dirichlet.ptr, tmp.data(), tmp.size() * sizeof(double),
                               hipMemcpyHostToDevice, stream));
      HIP_CHECK(hipStreamSynchronize(stream)); /* tmp goes out of scope */
    }
    have_dirichlet = true;
  }
  if (bdry.needs_dirichlet && !have_dirichlet)
    throw HipError(RYUJIN_ERR_ARG, "prepare_state_vector: the boundary map holds dirichlet / dynamic / "
                                   "dirichlet_momentum ids but no Dirichlet data was ever passed");
  /* Boundary conditions (:102-146). Small meshes: applied by the first pre-pass sweep itself (apply_bc_row; a
   * launch less per update). Boundary rows may be export rows -- read by the pack kernel of an exchange of this
   * vector that is still in flight (two calls in a row): the export part runs behind it in stream order on
   * comm_stream, the interior part never writes them. Large meshes: a launch of its own in front of the sweep
   * (the streaming pre-pass kernel keeps its occupancy); it writes export rows from the compute stream and
   * therefore joins whatever comm_stream still holds for them. */
  const BcFold bc{bdry.n_groups ? d_bc_mask.ptr : nullptr, d_bc_first.ptr, d_grp_start.ptr, d_b_normal.ptr,
                  d_b_id.ptr,   d_dirichlet.ptr};
  const bool fold_bc = L.n_slices <= bc_fold_max_slices;
  /* the step that wrote this vector left its precomputed values and Riemann records behind (FusedPrecompute):
   * no pre-pass sweep, the boundary rows are redone behind the boundary conditions */
  bool have_records = false;
  if constexpr (E::kFusablePrecompute)
    have_records = s.precomputed && !fold_bc;
  s.precomputed = false;
  if (!fold_bc && bdry.n_groups) {
    if (exchange_after_exp)
      wait_comm();
    else
      join_export();
    if constexpr (E::kFusablePrecompute) {
      if (have_records)
        hipLaunchKernelGGL(k_apply_bc_records<E>, dim3(grid_for(bdry.n_groups)), block, 0, stream, eparams, bdry.n_groups,
                           d_b_i.ptr, d_row_len.ptr, bc, s.U.ptr, s.prec.ptr, s.rrec.ptr);
    }
    if (!have_records)
      hipLaunchKernelGGL(k_apply_bc<E>, dim3(grid_for(bdry.n_groups)), block, 0, stream, eparams, bdry.n_groups, d_b_i.ptr,
                         bc, s.U.ptr);
  }
  /* U.update_ghost_values(), :148, is enqueued BEHIND the export part of the first pre-pass sweep, which
   * reads owned states only: the interior part of step 2 then waits for that export part alone, and the
   * exchange of U hides behind the interior parts of the pre-pass and of step 2 */
  if constexpr (std::is_same<typename E::Params, EulerAeosParams>::value) {
    /* n_precomputation_cycles = 2 (euler_aeos/hyperbolic_system.h:433), ghost update after each */
    const bool eos_function = eparams.eos == RYUJIN_EOS_FUNCTION;
    last_eos_kind = eparams.eos;
    last_precompute_interpreted = eos_function;
    for (int w = 0; w < kEosPrograms; ++w)
      last_eos_n_instructions[w] = eos_function ? eos_n_instructions[w] : 0;
    sweep([&](const DeviceMesh &mm, dim3 grid) {
      if (eos_function) {
        /* the interpreter: a kernel of its own, one wave per block and slice */
        const dim3 slices(mm.slice_end - mm.slice_begin), wave(kEosFunctionBlock);
        with_bool(fold_bc, [&](auto fold) {
          hipLaunchKernelGGL((k_precompute_aeos0_function<E::DIMENSION, decltype(fold)::value>), slices, wave, 0,
                             launch_stream, eparams, mm, bc, d_eos_function.ptr, s.U.ptr, s.prec.ptr, s.rrec.ptr,
                             d_gamma.ptr);
        });
      } else
        with_bool(fold_bc, [&](auto fold) {
          hipLaunchKernelGGL((k_precompute_aeos0<E::DIMENSION, decltype(fold)::value>), grid, block, 0, launch_stream,
                             eparams, mm, bc, s.U.ptr, s.prec.ptr, s.rrec.ptr, d_gamma.ptr);
        });
    });
    exchange_vector(s.U.ptr, KP, true);
    exchange_vector(s.prec.ptr, 4, true);
    if (L.n_relevant > L.n_owned) {
      /* Riemann records of the ghost rows from the exchanged (U_j, p_j): on comm_stream behind the two exchanges */
      hipLaunchKernelGGL(k_ghost_records_aeos<E::DIMENSION>, dim3(grid_for(L.n_relevant - L.n_owned)), block, 0,
                         exch.n_nbr ? comm_stream : stream, eparams, L.n_owned, L.n_relevant, s.U.ptr, s.prec.ptr,
                         s.rrec.ptr, d_gamma.ptr);
      if (exch.n_nbr) {
        comm_pending = true;
        exchange_after_exp = true;
      }
    }
    sweep([&](const DeviceMesh &mm, dim3 grid) {
      hipLaunchKernelGGL(k_precompute_aeos1<E::DIMENSION>, grid, block, 0, launch_stream, eparams, mm, s.U.ptr,
                         d_gamma.ptr, s.prec.ptr, s.prec.ptr);
    });
    exchange_vector(s.prec.ptr, 4, true);
  } else if constexpr (std::is_same<typename E::Params, ScalarParams>::value) {
    sweep([&](const DeviceMesh &mm, dim3 grid) {
      if (eparams.flux == RYUJIN_FLUX_FUNCTION) {
        /* the interpreter: a kernel of its own, one wave per block and slice */
        const dim3 slices(mm.slice_end - mm.slice_begin), wave(kFluxFunctionBlock);
        with_bool(fold_bc, [&](auto fold) {
          hipLaunchKernelGGL((k_precompute_sc_function<E::DIMENSION, decltype(fold)::value>), slices, wave, 0,
                             launch_stream, eparams, mm, bc, d_flux_function.ptr, s.U.ptr, s.prec.ptr);
        });
      } else
        with_bool(fold_bc, [&](auto fold) {
          hipLaunchKernelGGL((k_precompute_sc<E::DIMENSION, decltype(fold)::value>), grid, block, 0, launch_stream,
                             eparams, mm, bc, s.U.ptr, s.prec.ptr);
        });
    });
    exchange_vector(s.U.ptr, KP, true);
    exchange_vector(s.prec.ptr, E::NPREC, true);
  } else {
    static_assert(std::is_same<typename E::Params, EulerParams>::value ||
                      std::is_same<typename E::Params, ShallowWaterParams>::value,
                  "Descriptions with node records");
    /* The pre-pass reads owned U only. Precomputed values and records of the ghost rows are computed locally
     * from the exchanged ghost states (functions of U_j alone: nothing to exchange, :157-160 moves the same
     * numbers), behind the exchange of U on comm_stream. */
    if (have_records) {
      /* the owned rows are complete. Their producers: the last sweep of the step (its export part sits on
       * comm_stream, in front of this exchange in stream order) and, for boundary rows, the kernel above on the
       * compute stream -- with boundary DoFs the exchange is ordered behind the compute stream as well */
      exchange_vector(s.U.ptr, KP, bdry.n_groups == 0);
    } else {
      sweep([&](const DeviceMesh &mm, dim3 grid) {
        with_bool(fold_bc, [&](auto fold) {
          hipLaunchKernelGGL((k_precompute_records<E, decltype(fold)::value>), grid, block, 0, launch_stream, eparams,
                             mm, bc, s.U.ptr, s.prec.ptr, s.rrec.ptr);
        });
      });
      exchange_vector(s.U.ptr, KP, true);
    }
    if (L.n_relevant > L.n_owned) {
      hipLaunchKernelGGL(k_ghost_precompute_records<E>, dim3(grid_for(L.n_relevant - L.n_owned)), block, 0,
                         exch.n_nbr ? comm_stream : stream, eparams, L.n_owned, L.n_relevant, s.U.ptr, s.prec.ptr,
                         s.rrec.ptr);
      if (exch.n_nbr) { /* work on comm_stream behind the latest export part, as an exchange (not counted as one) */
        comm_pending = true;
        exchange_after_exp = true;
      }
    }
  }
  HIP_CHECK(hipGetLastError());
}

/* what step_plan.hpp decides from (plan_step): everything of the context that selects a kernel */
template <typename E>
StepPlanInput ryujin_hip_ctx::plan_input(const int stages) const
{
  StepPlanInput in;
  in.equation = is_euler_v<E> ? PlanEquation::euler
                              : (is_aeos_v<E> ? PlanEquation::euler_aeos
                                              : (is_scalar_v<E> ? PlanEquation::scalar : PlanEquation::shallow_water));
  in.dim = E::DIMENSION;
  in.fusable_precompute = E::kFusablePrecompute;
  in.stages = stages;
  in.limiter_iterations = params.limiter_iterations;
  in.dg = dg;
  in.max_row_len = L.max_row_len;
  in.n_slices = L.n_slices;
  in.n_export_slices = exch.n_nbr != 0 ? n_export_slices : 0u; /* the launches of sweep() */
  in.debug_pij_storage = params.debug_pij_storage;
  in.debug_next_tile_mask = params.debug_next_tile_mask;
  in.checked = params.debug_expensive_bounds_check != 0;
  in.limited_fraction = limited_fraction;
  in.per_slice_max_limited = (double)RYUJIN_PER_SLICE_MAX_LIMITED;
  in.resident_waves_step5 = resident_waves_step5;
  in.resident_waves_step6 = resident_waves_step6;
  in.bc_fold_max_slices = bc_fold_max_slices;
  in.pending_precompute = pending_precompute;
  in.riemann_newton_max_iterations = eparams.riemann_newton_max_iterations;
  in.rarefaction_power = eparams.rarefaction_power;
  in.friction = swparams.manning != 0.;
  return in;
}

/* Step 2: d_ij (upper triangle), alpha_i; ghost alpha (:341-424) */
template <typename E>
void ryujin_hip_ctx::step2_dij_alpha(const StepPlan &plan, const State &old)
{
  constexpr int DIM = E::DIMENSION;
  const auto &eparams = eq_params<E>(); /* shadows the member: the equation's parameter block */
  const dim3 block(kBlock);
  if constexpr (is_aeos_v<E>) {
    sweep([&](const DeviceMesh &mm, dim3 grid) {
      hipLaunchKernelGGL(k_alpha_aeos<DIM>, grid, block, 0, launch_stream, eparams, mm, old.U.ptr, old.prec.ptr,
                         d_alpha.ptr);
    });
    mark(8);
    exchange_vector(d_alpha.ptr, 1, true);
    sweep([&](const DeviceMesh &mm, dim3 grid) {
      hipLaunchKernelGGL(k_dij_aeos<DIM>, grid, block, 0, launch_stream, eparams, mm, d_lower_mask.ptr,
                         old.rrec.ptr, d_dij.ptr);
    });
  } else if constexpr (is_scalar_v<E>) {
    /* the function flux enters step 2 through f((u_i + u_j) / 2) of the averaged entropy alone */
    const bool interpreted = flux_interpreted_pairs();
    last_flux_kind = eparams.flux;
    last_flux_n_instructions = eparams.flux == RYUJIN_FLUX_FUNCTION ? flux_n_instructions : 0;
    last_step2_interpreted = interpreted ? 1 : 0;
    sweep([&](const DeviceMesh &mm, dim3 grid) {
      if (interpreted)
        hipLaunchKernelGGL(k_dij_alpha_sc_function<DIM>, grid, block, 0, launch_stream, eparams, mm,
                           d_flux_function.ptr, old.U.ptr, old.prec.ptr, d_dij.ptr, d_alpha.ptr);
      else
        hipLaunchKernelGGL(k_dij_alpha_sc<DIM>, grid, block, 0, launch_stream, eparams, mm, old.U.ptr,
                           old.prec.ptr, d_dij.ptr, d_alpha.ptr);
    });
    mark(8);
    exchange_vector(d_alpha.ptr, 1, true);
  } else if (plan.step2 == StepPlan::Step2::records) {
    sweep([&](const DeviceMesh &mm, dim3 grid) {
      hipLaunchKernelGGL((k_dij_alpha_records<E, false>), grid, block, 0, launch_stream, eparams, mm,
                         old.U.ptr, old.prec.ptr, old.rrec.ptr, d_dij.ptr, d_alpha.ptr);
    });
    exchange_vector(d_alpha.ptr, 1, true);
  } else if (plan.step2 == StepPlan::Step2::alpha_then_dij) {
    sweep([&](const DeviceMesh &mm, dim3 grid) {
      hipLaunchKernelGGL(k_alpha<E>, grid, block, 0, launch_stream, eparams, mm, old.U.ptr, old.prec.ptr,
                         d_alpha.ptr);
    });
    mark(8); /* end of the indicator kernel: sweep_ms[0] = k_alpha alone */
    exchange_vector(d_alpha.ptr, 1, true); /* overlaps with the Riemann sweep as well */
    sweep([&](const DeviceMesh &mm, dim3 grid) {
      if constexpr (is_euler_v<E>)
        with_bool(!plan.fast_riemann, [&](auto newton) {
          hipLaunchKernelGGL((k_dij_records<E, decltype(newton)::value>), grid, block, 0, launch_stream, eparams, mm,
                             d_lower_mask.ptr, old.rrec.ptr, old.U.ptr, d_dij.ptr);
        });
    });
  } else {
    sweep([&](const DeviceMesh &mm, dim3 grid) {
      hipLaunchKernelGGL(k_dij_alpha<E>, grid, block, 0, launch_stream, eparams, mm, old.U.ptr,
                         old.prec.ptr, d_dij.ptr, d_alpha.ptr);
    });
    exchange_vector(d_alpha.ptr, 1, true);
  }
}

/* Step 3: boundary d_ij, symmetrise, diagonal, tau_max (:432-578) */
template <typename E>
void ryujin_hip_ctx::step3_diagonal_tau(const StepPlan &plan, const State &old)
{
  constexpr int DIM = E::DIMENSION;
  const auto &eparams = eq_params<E>();
  const dim3 block(kBlock);
  if (const uint32_t n_pairs = (uint32_t)d_p_pos.n) {
    join_export(); /* boundary pairs may sit in export rows, whose d_ij the export part wrote on comm_stream
                    * (and may point to ghost columns: the U exchange precedes that export part in stream order) */
    if constexpr (is_aeos_v<E>)
      hipLaunchKernelGGL(k_dij_boundary_aeos<DIM>, dim3(grid_for(n_pairs)), block, 0, stream, eparams,
                         n_pairs, d_p_i.ptr, d_p_j.ptr, d_p_pos.ptr, d_p_cji.ptr, old.rrec.ptr, d_dij.ptr);
    else if constexpr (is_scalar_v<E>) {
      if (flux_interpreted_pairs())
        hipLaunchKernelGGL(k_dij_boundary_sc_function<DIM>, dim3(grid_for(n_pairs, kFluxFunctionBlock)),
                           dim3(kFluxFunctionBlock), 0, stream, eparams, d_flux_function.ptr, n_pairs, d_p_i.ptr,
                           d_p_j.ptr, d_p_pos.ptr, d_p_cji.ptr, old.U.ptr, old.prec.ptr, d_dij.ptr);
      else
        hipLaunchKernelGGL(k_dij_boundary_sc<DIM>, dim3(grid_for(n_pairs)), block, 0, stream, eparams,
                           n_pairs, d_p_i.ptr, d_p_j.ptr, d_p_pos.ptr, d_p_cji.ptr, old.U.ptr,
                           old.prec.ptr, d_dij.ptr);
    }
    else
      hipLaunchKernelGGL(k_dij_boundary<E>, dim3(grid_for(n_pairs)), block, 0, stream, eparams,
                         n_pairs, d_p_i.ptr, d_p_j.ptr, d_p_pos.ptr, d_p_cji.ptr, old.U.ptr, d_dij.ptr);
  }
  sweep([&](const DeviceMesh &mm, dim3 grid) {
    auto unrolled = [&](auto width) {
      hipLaunchKernelGGL(k_dij_diag_unrolled<decltype(width)::value>, grid, block, 0, launch_stream, mm,
                         d_lower_mask.ptr, params.cfl, d_dij.ptr, d_scalars.ptr);
    };
    if (plan.diag_width == 3)
      unrolled(std::integral_constant<int, 3>{});
    else if (plan.diag_width == 9)
      unrolled(std::integral_constant<int, 9>{});
    else if (plan.diag_width == 27)
      unrolled(std::integral_constant<int, 27>{});
    else
      hipLaunchKernelGGL(k_dij_diag, grid, block, 0, launch_stream, mm, params.cfl, d_dij.ptr,
                         d_scalars.ptr);
  });
  /* Utilities::MPI::min(tau_max), :571. Inside a device-resident RK step only the first stage needs the
   * global minimum (it defines tau); later stages use their local tau_max for the validity check only,
   * whose flag is reduced once at the end of the RK step together with the restart flag. */
  if (!(deferred && rk_stage > 0))
    allreduce_scalar(&d_scalars.ptr->tau_max_bits, 0);
  if (want_tau_early && deferred && rk_stage == 0) {
    /* tau_max = min(tau_max argument, CFL bound over all ranks) is final here: hand it to the host while
     * steps 4-7 of this stage run (time-dependent Dirichlet data of the later stages) */
    join_export();
    HIP_CHECK(hipMemcpyAsync(h_tau_early, &d_scalars.ptr->tau_max_bits, sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipEventRecord(ev_tau, stream));
  }
  /* tau itself is resolved inside the step-4 kernel (finalize_tau) */
}

/* the buffers the planned kernels of steps 4 - 7 need beyond those create() made; allocated by the first update that
 * takes the path */
void ryujin_hip_ctx::ensure_limiter_buffers(const StepPlan &plan)
{
  if (params.limiter_iterations == 2 && d_V.n == 0) {
    d_V.alloc((size_t)L.n_relevant * KP);
    d_slice_unlimited.alloc(L.n_slices);
  }
  ensure_pij();
  if (plan.per_slice() && d_slice_first_stored.n == 0) {
    d_slice_first_stored.alloc(L.n_slices);
    d_slice_todo.alloc(L.n_slices);
  }
  if (plan.tiles_predicted_from_history && d_slice_needed.n == 0) { /* all ones: the first update stores every tile */
    d_slice_needed.alloc(L.n_slices);
    HIP_CHECK(hipMemsetAsync(d_slice_needed.ptr, 0xff, (size_t)L.n_slices * sizeof(uint32_t), launch_stream));
  }
  if (plan.next_tile_mask && d_slice_next_tiles.n == 0)
    d_slice_next_tiles.alloc(L.n_slices);
}

/* Step 4: low-order update, bounds, r_i, p_ij; ghost r (:597-884) */
template <typename E>
void ryujin_hip_ctx::step4_low_order(const StepPlan &plan, const StepArgs<E::DIMENSION> &a)
{
  constexpr int DIM = E::DIMENSION;
  const auto &eparams = eq_params<E>();
  const dim3 block(kBlock);
  const State &old = a.old, &nw = a.nw;
  sweep([&](const DeviceMesh &mm, dim3 grid) {
    /* every step-4 kernel takes the same arguments; shallow water adds the bathymetry */
    auto launch = [&](auto kernel, auto... bathymetry) {
      hipLaunchKernelGGL(kernel, grid, block, 0, launch_stream, eparams, mm, d_scalars.ptr, a.weight, a.S, old.U.ptr,
                         old.prec.ptr, bathymetry..., d_alpha.ptr, d_dij.ptr, nw.U.ptr, d_r.ptr, d_bounds.ptr,
                         d_pij.ptr);
    };
    if constexpr (is_sw_v<E>) {
      if (plan.step4_single_walk) {
        constexpr int kSwWidth = DIM == 1 ? 3 : 9;
        return with_bool(plan.step4_has_stages, [&](auto has_stages) {
          with_bool(plan.step4_friction, [&](auto friction) {
            launch(k_low_order_sw_single_walk<DIM, decltype(has_stages)::value, kSwWidth, decltype(friction)::value>,
                   d_Z.ptr);
          });
        });
      }
    }
    /* <has_stages, stores_p, dg>; not storing P_ij goes with no stage vectors and a continuous ansatz (plan_step) */
    auto launch4 = [&](auto has_stages, auto stores_p, auto dg_) {
      constexpr bool HS = decltype(has_stages)::value, SP = decltype(stores_p)::value, DG = decltype(dg_)::value;
      if constexpr (is_euler_v<E>)
        launch(k_low_order<DIM, HS, SP, DG>);
      else if constexpr (is_aeos_v<E>)
        launch(k_low_order_aeos<DIM, HS, SP, DG>);
      else if constexpr (is_scalar_v<E>)
        launch(k_low_order_sc<DIM, HS, DG>);
      else
        launch(k_low_order_sw<DIM, HS, DG>, d_Z.ptr);
    };
    if (!plan.step4_stores_p)
      launch4(std::false_type{}, std::false_type{}, std::false_type{});
    else
      with_bool(plan.step4_has_stages, [&](auto has_stages) {
        with_bool(plan.dg, [&](auto dg_) { launch4(has_stages, std::true_type{}, dg_); });
      });
  });
  /* EXPENSIVE_BOUNDS_CHECK as a run-time option (Euler): is_admissible() of the low-order update (:851-855) */
  if (plan.checked)
    sweep([&](const DeviceMesh &mm, dim3 grid) {
      hipLaunchKernelGGL(k_check_admissible<E>, grid, block, 0, launch_stream, eparams, mm, d_scalars.ptr,
                         (const double *)nw.U.ptr);
    });
  exchange_vector(d_r.ptr, KP, true);
  if (plan.dg && plan.step5 != StepPlan::Step5::none) {
    /* the bounds are extended over the stencil in step 5: their ghost range has to be current
     * (hyperbolic_module.template.h:601-613); SoA, one scalar vector per bound */
    for (int b = 0; b < NB; ++b)
      exchange_vector(d_bounds.ptr + (size_t)b * mesh.bounds_stride, 1, true);
  }
}

/* Step 5: second part of p_ij, first l_ij; ghost rows of l_ij (:892-1041) */
template <typename E>
void ryujin_hip_ctx::step5_limiter(const StepPlan &plan, const StepArgs<E::DIMENSION> &a)
{
  using Step5 = StepPlan::Step5;
  constexpr int DIM = E::DIMENSION;
  const auto &eparams = eq_params<E>();
  const dim3 block(kBlock);
  const State &old = a.old, &nw = a.nw;
  if (plan.step5 == Step5::none)
    return;
  if (plan.dg) {
    /* bounds over the stencil (:938-948) with the Description's Limiter::combine_bounds; steps 5-7 read the
     * extended bounds */
    sweep([&](const DeviceMesh &mm, dim3 grid) {
      if constexpr (is_euler_v<E>)
        hipLaunchKernelGGL(k_bounds_combine_euler, grid, block, 0, launch_stream, mm, d_bounds.ptr,
                           d_bounds_combined.ptr);
      else if constexpr (is_sw_v<E>)
        hipLaunchKernelGGL(k_bounds_combine_sw, grid, block, 0, launch_stream, mm, d_bounds.ptr,
                           d_bounds_combined.ptr);
      else if constexpr (is_aeos_v<E>)
        hipLaunchKernelGGL((k_bounds_combine_minmax<4, 0x2u>), grid, block, 0, launch_stream, mm, d_bounds.ptr,
                           d_bounds_combined.ptr);
      else
        hipLaunchKernelGGL((k_bounds_combine_minmax<2, 0x2u>), grid, block, 0, launch_stream, mm, d_bounds.ptr,
                           d_bounds_combined.ptr);
    });
    std::swap(d_bounds.ptr, d_bounds_combined.ptr);
  }
  sweep([&](const DeviceMesh &mm, dim3 grid) {
    if constexpr (is_euler_v<E> || is_aeos_v<E>) {
      /* <waves per slice, P_ij per slice, P_ij per tile>; several waves per slice leave no V_i */
      auto stage0 = [&](auto ny, auto per_slice, auto per_tile, const SliceFlags &flags, const int storage) {
        constexpr int NY = decltype(ny)::value;
        hipLaunchKernelGGL((k_lij_stage0<E, NY, decltype(per_slice)::value, decltype(per_tile)::value>),
                           dim3(grid.x, NY), block, 0, launch_stream, eparams, mm, d_scalars.ptr, old.U.ptr,
                           d_alpha.ptr, d_dij.ptr, nw.U.ptr, d_r.ptr, d_bounds.ptr, d_pij.ptr, d_lij.ptr,
                           NY == 1 ? d_V.ptr : nullptr, flags, storage);
        record_step5(mm, NY);
      };
      constexpr std::integral_constant<int, 1> one{};
      if (plan.step5 == Step5::stage0_per_tile) {
        if constexpr (DIM <= 2)
          stage0(one, std::false_type{}, std::true_type{}, a.tile_flags, 0);
        return;
      }
      if (plan.step5 == Step5::stage0_per_slice)
        return stage0(one, std::true_type{}, std::false_type{}, a.slice_flags, params.debug_pij_storage);
      if (plan.step5 == Step5::stage0_groups)
        return with_groups(plan.step5_groups,
                           [&](auto ny) { stage0(ny, std::false_type{}, std::false_type{}, a.tile_flags, 0); });
    }
    if constexpr (is_euler_v<E>) {
      if (plan.step5 == Step5::recompute) {
        with_groups(plan.recompute_groups(grid.x), [&](auto ny) {
          constexpr int NY = decltype(ny)::value;
          hipLaunchKernelGGL((k_pij_lij_recompute<DIM, NY>), dim3(grid.x, NY), block, 0, launch_stream, eparams,
                             mm, d_scalars.ptr, a.weight, old.U.ptr, d_alpha.ptr, d_dij.ptr, nw.U.ptr, d_r.ptr,
                             d_bounds.ptr, d_pij.ptr, d_lij.ptr);
          record_step5(mm, NY);
        });
        return;
      }
    }
    with_bool(plan.dg, [&](auto dg_) {
      with_bool(plan.wide, [&](auto wide) {
        hipLaunchKernelGGL((k_pij_lij<E, decltype(dg_)::value, decltype(wide)::value>), grid, block,
                           tail_queue_bytes(mm), launch_stream, eparams, mm, d_scalars.ptr, nw.U.ptr, d_r.ptr,
                           d_bounds.ptr, d_pij.ptr, d_lij.ptr, d_V.ptr);
      });
    });
    record_step5(mm, 1);
  });
  if (plan.checked) /* the first limiter pass in the checked control flow (limiter.template.h:110-134,244-322) */
    sweep([&](const DeviceMesh &mm, dim3 grid) {
      hipLaunchKernelGGL(k_check_limiter<E>, grid, block, 0, launch_stream, eparams, mm, d_scalars.ptr,
                         (const double *)nw.U.ptr, (const double *)d_bounds.ptr, (const double *)d_pij.ptr,
                         (const double *)nullptr);
    });
  exchange_matrix(d_lij.ptr, true);
}

/* Step 6, the first of two limiter passes: symmetrise l_ij, high-order update, next l_ij (:1053-1182) */
template <typename E>
void ryujin_hip_ctx::step6_high_order_next(const StepPlan &plan, const StepArgs<E::DIMENSION> &a)
{
  using Step6 = StepPlan::Step6;
  constexpr int DIM = E::DIMENSION;
  constexpr int kWidth = q1_stencil_width(DIM);
  /* 3-D: cache all l_ij and the P_ij of the first RYUJIN_HO_CP_3D columns */
  constexpr int kCachedP =
      DIM == 3 ? RYUJIN_HO_CP_3D : (DIM == 2 ? (RYUJIN_HO_CP_2D < kWidth ? RYUJIN_HO_CP_2D : kWidth) : kWidth);
  const auto &eparams = eq_params<E>();
  const dim3 block(kBlock);
  const State &nw = a.nw;
  double *const V = plan.has_V ? d_V.ptr : nullptr;
  uint8_t *const unlimited = plan.has_V ? d_slice_unlimited.ptr : nullptr;
  sweep([&](const DeviceMesh &mm, dim3 grid) {
    if constexpr (is_euler_v<E> || is_aeos_v<E>) {
      if (plan.step6 == Step6::per_slice) { /* light, repair, heavy (plan_step) */
        auto launch_mode = [&](auto mode) {
          hipLaunchKernelGGL((k_high_order_next_cached<E, kWidth, kCachedP, false, decltype(mode)::value>), grid,
                             block, 0, launch_stream, eparams, mm, nw.U.ptr, d_bounds.ptr, d_pij.ptr, d_lij.ptr,
                             d_lij_next.ptr, d_V.ptr, last_s0, a.slice_flags);
        };
        launch_mode(std::integral_constant<int, kHoLight>{});
        hipLaunchKernelGGL(k_pij_repair<E>, grid, block, 0, launch_stream, mm, last_s0, d_pij.ptr, a.slice_flags);
        launch_mode(std::integral_constant<int, kHoHeavy>{});
        record_step6(mm, 1, false);
        return;
      }
    }
    if constexpr (DIM <= 2) {
      const uint32_t n_launch = mm.slice_end - mm.slice_begin;
      if (plan.step6_shares_slices(n_launch)) {
        hipLaunchKernelGGL((k_high_order_next_cached<E, kWidth, kWidth, true>), dim3(n_launch), block, 0,
                           launch_stream, eparams, mm, nw.U.ptr, d_bounds.ptr, d_pij.ptr, d_lij.ptr, d_lij_next.ptr,
                           V, last_s0, SliceFlags{unlimited, nullptr, nullptr});
        record_step6(mm, 1, true);
        return;
      }
    }
    if (plan.step6 == Step6::cached) {
      SliceFlags flags6 = a.tile_flags;
      flags6.unlimited = unlimited;
      flags6.next_tiles = plan.next_tile_mask ? d_slice_next_tiles.ptr : nullptr;
      /* (what the ghost exchange sends -- entries of the export slices -- is always stored) */
      flags6.next_tiles_elide =
          plan.next_tiles_elided && (exch.n_nbr == 0 || mm.slice_begin >= n_export_slices) ? 1u : 0u;
      hipLaunchKernelGGL((k_high_order_next_cached<E, kWidth, kCachedP>), grid, block, 0, launch_stream, eparams, mm,
                         nw.U.ptr, d_bounds.ptr, d_pij.ptr, d_lij.ptr, d_lij_next.ptr, V, last_s0, flags6);
    } else
      with_bool(plan.wide, [&](auto wide) {
        hipLaunchKernelGGL((k_high_order<E, false, decltype(wide)::value>), grid, block, 0, launch_stream, eparams,
                           mm, nw.U.ptr, d_bounds.ptr, d_pij.ptr, d_lij.ptr, d_lij_next.ptr,
                           FusedSadd{0., 0., nullptr});
      });
    record_step6(mm, 1, false);
  });
  if (plan.checked) /* the update after the first pass (:1121-1126) and the second pass's success (:1155-1161) */
    sweep([&](const DeviceMesh &mm, dim3 grid) {
      hipLaunchKernelGGL(k_check_admissible<E>, grid, block, 0, launch_stream, eparams, mm, d_scalars.ptr,
                         (const double *)nw.U.ptr);
      hipLaunchKernelGGL(k_check_limiter<E>, grid, block, 0, launch_stream, eparams, mm, d_scalars.ptr,
                         (const double *)nw.U.ptr, (const double *)d_bounds.ptr, (const double *)d_pij.ptr,
                         (const double *)d_lij.ptr);
    });
  exchange_matrix(d_lij_next.ptr, true);
}

/* Step 7, the last limiter pass: symmetrise l_ij, high-order update; carries a pending sadd and the next pre-pass */
template <typename E>
void ryujin_hip_ctx::step7_high_order_last(const StepPlan &plan, const StepArgs<E::DIMENSION> &a)
{
  constexpr int DIM = E::DIMENSION;
  constexpr int kWidth = q1_stencil_width(DIM);
  constexpr int kLastChunk = DIM == 3 ? RYUJIN_LAST_CHUNK_3D : (DIM == 2 ? RYUJIN_LAST_CHUNK_2D : kWidth);
  const auto &eparams = eq_params<E>();
  const dim3 block(kBlock);
  const State &nw = a.nw;
  sweep([&](const DeviceMesh &mm, dim3 grid) {
    if (plan.step7 == StepPlan::Step7::last_cached)
      hipLaunchKernelGGL((k_high_order_last_cached<E, kWidth, kLastChunk>), grid, block, 0, launch_stream, eparams,
                         mm, nw.U.ptr, d_pij.ptr, d_lij.ptr, a.fused_sadd, a.fused_prec,
                         plan.step6_flags ? d_slice_unlimited.ptr : nullptr,
                         plan.next_tile_mask ? (const uint32_t *)d_slice_next_tiles.ptr : (const uint32_t *)nullptr);
    else
      hipLaunchKernelGGL((k_high_order<E, true>), grid, block, 0, launch_stream, eparams, mm, nw.U.ptr,
                         d_bounds.ptr, d_pij.ptr, d_lij.ptr, d_lij_next.ptr, a.fused_sadd);
  });
  if (plan.checked) /* the final update (:1121-1126) */
    sweep([&](const DeviceMesh &mm, dim3 grid) {
      hipLaunchKernelGGL(k_check_admissible<E>, grid, block, 0, launch_stream, eparams, mm, d_scalars.ptr,
                         (const double *)nw.U.ptr);
    });
}

/* the end of an update outside a device-resident RK step: scalars read back, timers, status */
int ryujin_hip_ctx::finish_step(double *tau_out)
{
  HIP_CHECK(hipMemcpyAsync(h_scalars, d_scalars.ptr, sizeof(DeviceScalars), hipMemcpyDeviceToHost,
                           stream));
  HIP_CHECK(hipStreamSynchronize(stream));
  update_limited_fraction();

  if (timers_enabled) {
    for (int k = 0; k < 7; ++k) {
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
      sweep_ms[k + 1] = ms;
    }
    sweep_ms[0] = 0.;
    if (last_plan.step2_split) {
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[8]));
      sweep_ms[0] = ms;
    }
    for (int k = 0; k < 8; ++k)
      sweep_ms_accum[k] += sweep_ms[k];
    ++sweep_updates_accum;
  }

  if (h_scalars->tau_invalid)
    return RYUJIN_ERR_TAU;
  *tau_out = h_scalars->tau;

  if (h_scalars->restart_needed) {
    if (params.id_violation_strategy == RYUJIN_IDV_WARN) {
      n_warnings++;
      return RYUJIN_WARN;
    }
    n_restarts++;
    return RYUJIN_RESTART;
  }
  return RYUJIN_OK;
}

template <typename E>
int ryujin_hip_ctx::step(int h_old, int stages, const int *h_stage, const double *w, int h_new,
                         double tau_in, double tau_max_in, double *tau_out)
{
  constexpr int DIM = E::DIMENSION;
  State &old = state(h_old);
  State &nw = state(h_new);
  if (h_old == h_new)
    throw HipError(RYUJIN_ERR_ARG, "old and new state vector must differ");
  nw.precomputed = false; /* rewritten below */

  /* which kernels this update runs: decided here, once (step_plan.hpp) */
  const StepPlan plan = plan_step(plan_input<E>(stages));
  if (plan.unsupported)
    throw HipError(RYUJIN_ERR_UNSUPPORTED, plan.unsupported);
  if (plan.violated)
    throw HipError(RYUJIN_ERR_ARG, std::string("internal: ") + plan.violated);
  last_plan = plan;
  last_launches = LaunchLog{};
  pending_precompute = false;

  /* scalars: tau_max := tau_max_in, flags := 0 -- carried by the first sweep of step 2 (step_begin) */
  const bool use_device_tau = deferred && rk_stage > 0;
  struct ClearBegin { /* a step that throws before its first sweep must not leave it armed */
    StepBegin &b;
    ~ClearBegin() { b = StepBegin{}; }
  } clear_begin{pending_begin};
  pending_begin = StepBegin{d_scalars.ptr,
                            tau_max_in,
                            tau_in,
                            (!deferred || rk_stage == 0) ? 1 : 0,
                            (deferred && rk_stage > 0) ? rk_stage - 1 : -1,
                            use_device_tau ? 1 : 0,
                            deferred ? rk_stage : 0};
  mark(0);
  step2_dij_alpha<E>(plan, old);
  mark(1);
  step3_diagonal_tau<E>(plan, old);
  mark(2);

  StepArgs<DIM> a{old, nw};
  {
    double acc = -1.;
    for (int s = 0; s < stages; ++s)
      acc += w[s];
    a.weight = -acc;
  }
  a.S.stages = stages;
  for (int s = 0; s < stages; ++s) {
    a.S.U[s] = state(h_stage[s]).U.ptr;
    a.S.prec[s] = state(h_stage[s]).prec.ptr;
    a.S.w[s] = w[s];
  }
  ensure_limiter_buffers(plan);
  a.slice_flags = SliceFlags{d_slice_unlimited.ptr, d_slice_first_stored.ptr, d_slice_todo.ptr};
  a.tile_flags = SliceFlags{nullptr, nullptr, nullptr, plan.tiles_predicted_from_history ? d_slice_needed.ptr : nullptr};
  last_s0 = Stage0Src{d_scalars.ptr, old.U.ptr, d_alpha.ptr, d_dij.ptr, d_r.ptr, plan.per_tile() ? 1 : 0};
  step4_low_order<E>(plan, a);
  mark(3);
  step5_limiter<E>(plan, a);
  mark(4);

  /* a pending sadd of the device-resident RK driver is applied by the last sweep, and so are the precomputed values
   * and Riemann records of the new vector where the plan says so (fuse_precompute) */
  a.fused_sadd = pending_sadd;
  pending_sadd = FusedSadd{0., 0., nullptr};
  if (plan.fuse_precompute)
    a.fused_prec = FusedPrecompute{nw.prec.ptr, nw.rrec.ptr};
  const int n_iterations = params.limiter_iterations;
  if (a.fused_sadd.src && n_iterations == 0)
    throw HipError(RYUJIN_ERR_ARG, "internal: fused sadd without a limiter pass");
  if (n_iterations == 2) {
    step6_high_order_next<E>(plan, a);
    mark(5);
    std::swap(d_lij.ptr, d_lij_next.ptr);
  }
  if (n_iterations != 0) {
    step7_high_order_last<E>(plan, a);
    mark(4 + n_iterations);
  }
  for (int k = 5 + n_iterations; k <= 7; ++k)
    mark(k);
  nw.precomputed = plan.fuse_precompute;

  join_export(); /* (the exchange of U_new stays in flight: whoever reads its ghost range joins it) */
  if (!deferred)
    allreduce_scalar(&d_scalars.ptr->restart_needed, 1); /* MPI::logical_or(restart_needed), :1194 */
  /* (deferred: the restart flag is folded into its accumulator by the next stage's step_begin(), or by
   * time_step() behind the last stage) */

  HIP_CHECK(hipGetLastError());
  if (deferred) {
    *tau_out = std::numeric_limits<double>::quiet_NaN(); /* known at the end of the RK step */
    return RYUJIN_OK;
  }
  return finish_step(tau_out);
}

/* Device-resident Runge-Kutta driver: ryujin::TimeIntegrator::step for the
 * schemes that consist solely of prepare_state_vector + step<s> + sadd
 * (source/time_integrator.template.h:207-403), including the bang-bang CFL recovery (:250-274).
 * All stages are enqueued back to back: the tau of the first stage stays on the device, the restart /
 * tau-validity flags of all stages are accumulated there, and the host synchronises ONCE per RK step.
 * A Restart is therefore detected at the end of the RK step instead of inside it; the reference repeats
 * the whole RK step from the untouched state vector anyway, so the outcome is the same. */
template <typename E>
int ryujin_hip_ctx::time_step(int scheme, int h_state, int n_tmp, const int *h_tmp, const double *dirichlet,
                              double tau_max, int cfl_recovery, double cfl_min, double cfl_max,
                              double *tau_out, double t, ryujin_hip_dirichlet_fn dirichlet_fn,
                              void *dirichlet_user, bool dirichlet_on_device)
{
  const int U = h_state;
  int n_stages = 0;
  double tau_factor = 1.;
  switch (scheme) {
  case RYUJIN_SCHEME_ERK_11: n_stages = 1; break;
  case RYUJIN_SCHEME_SSPRK_22: n_stages = 2; break;
  case RYUJIN_SCHEME_ERK_22: n_stages = 2; tau_factor = 2.; break;
  case RYUJIN_SCHEME_SSPRK_33: n_stages = 3; break;
  case RYUJIN_SCHEME_ERK_33: n_stages = 3; tau_factor = 3.; break;
  case RYUJIN_SCHEME_ERK_43: n_stages = 4; tau_factor = 4.; break;
  case RYUJIN_SCHEME_ERK_54: n_stages = 5; tau_factor = 5.; break;
  default: throw HipError(RYUJIN_ERR_ARG, "unknown time stepping scheme");
  }
  const bool erk = scheme != RYUJIN_SCHEME_SSPRK_22 && scheme != RYUJIN_SCHEME_SSPRK_33;
  /* temp_ vectors: SSPRK22 2, SSPRK33 2, ERK s stages: s (time_integrator.template.h:163-205) */
  const int n_needed = erk ? n_stages : 2;
  if (n_tmp < n_needed)
    throw HipError(RYUJIN_ERR_ARG, "time_step: not enough temporary state vectors for this scheme");
  const int *T = h_tmp;
  const double first_tau_max = erk ? tau_max / n_stages : tau_max;

  /* explicit Runge-Kutta stages 2.. as (number of stage vectors, their handles, weights):
   * step_erk_22/33/43/54 (time_integrator.template.h:341-500) */
  struct ErkStage {
    int n;
    int h[4];
    double w[4];
  };
  ErkStage erk_stage[5] = {};
  if (scheme == RYUJIN_SCHEME_ERK_22) {
    erk_stage[1] = {1, {U}, {-1.}};
  } else if (scheme == RYUJIN_SCHEME_ERK_33) {
    erk_stage[1] = {1, {U}, {-1.}};
    erk_stage[2] = {2, {U, T[0]}, {0.75, -2.}};
  } else if (scheme == RYUJIN_SCHEME_ERK_43) {
    erk_stage[1] = {1, {U}, {-1.}};
    erk_stage[2] = {1, {T[0]}, {-1.}};
    erk_stage[3] = {2, {T[0], T[1]}, {5. / 3., -10. / 3.}};
  } else if (scheme == RYUJIN_SCHEME_ERK_54) {
    constexpr double c = 0.2;
    constexpr double a_21 = +0.2;
    constexpr double a_31 = +0.26075582269554909, a_32 = +0.13924417730445096;
    constexpr double a_41 = -0.25856517872570289, a_42 = +0.91136274166280729, a_43 = -0.05279756293710430;
    constexpr double a_51 = +0.21623276431503774, a_52 = +0.51534223099602405, a_53 = -0.81662794199265554,
                     a_54 = +0.88505294668159373;
    constexpr double a_61 = -0.10511678454691901, a_62 = +0.87880047152100838, a_63 = -0.58903404061484477,
                     a_64 = +0.46213380485434047;
    erk_stage[1] = {1, {U}, {(a_31 - a_21) / c}};
    erk_stage[2] = {2, {U, T[0]}, {(a_41 - a_31) / c, (a_42 - a_32) / c}};
    erk_stage[3] = {3, {U, T[0], T[1]}, {(a_51 - a_41) / c, (a_52 - a_42) / c, (a_53 - a_43) / c}};
    erk_stage[4] = {4, {U, T[0], T[1], T[2]},
                    {(a_61 - a_51) / c, (a_62 - a_52) / c, (a_63 - a_53) / c, (a_64 - a_54) / c}};
  }

  auto single_step = [&]() -> int {
    double dummy = 0.;
    deferred = true;
    struct Guard {
      bool &flag, &armed;
      ~Guard() { flag = armed = false; }
    } guard{deferred, pending_precompute};
    int result = -1; /* handle that holds the new solution */
    const double no_limit = std::numeric_limits<double>::max();
    const int none[1] = {0};
    const double no_w[1] = {0.};

    /* Dirichlet data of stage st: time independent (the array, uploaded once), or initial_state(position,
     * t + c_s tau) per stage (time_integrator.template.h:279-510: SSPRK22 t, t+tau; SSPRK33 t, t+tau, t+tau/2;
     * ERK stage s at t + s tau) through the caller's function. tau is known on the host as soon as step 3 of
     * the first stage has run; the first stage's remaining sweeps are already enqueued behind it. */
    const bool time_dependent = dirichlet_fn != nullptr && bdry.n_bdry > 0 && bdry.needs_dirichlet;
    std::vector<double> stage_data;
    double tau_first = 0.;
    auto stage_coefficient = [&](int st) -> double {
      if (st == 0)
        return 0.;
      return erk ? (double)st : (scheme == RYUJIN_SCHEME_SSPRK_33 && st == 2 ? 0.5 : 1.);
    };
    auto dirichlet_at = [&](int st) -> const double * {
      if (!time_dependent)
        return st == 0 ? dirichlet : nullptr;
      const double c = stage_coefficient(st);
      stage_data.assign((size_t)bdry.n_bdry * K, 0.);
      dirichlet_fn(dirichlet_user, t + c * tau_first, stage_data.data());
      return stage_data.data();
    };
    /* ... or through the configured analytic state on the device (ryujin_hip_time_step_iv): the kernel forms the
     * stage time from the tau the first stage left in DeviceScalars::tau_rk; the host waits for nothing */
    auto device_dirichlet_at = [&](int st) { return IvStage{dirichlet_on_device, t, stage_coefficient(st)}; };
    struct EarlyTau {
      bool &flag;
      ~EarlyTau() { flag = false; }
    } early_tau{want_tau_early};
    if (time_dependent && n_stages > 1) {
      if (!h_tau_early) {
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&h_tau_early), sizeof(unsigned long long)));
        HIP_CHECK(hipEventCreateWithFlags(&ev_tau, hipEventDisableTiming));
      }
      want_tau_early = true;
    }

    rk_stage = 0;
    prepare_state_vector<E>(U, dirichlet_at(0), device_dirichlet_at(0));
    pending_precompute = true; /* every stage's result goes straight into the next prepare_state_vector() */
    step<E>(U, 0, none, no_w, T[0], 0., first_tau_max, &dummy);
    result = T[0];
    if (want_tau_early) {
      HIP_CHECK(hipEventSynchronize(ev_tau));
      tau_first = __builtin_bit_cast(double, *h_tau_early);
      if (!(tau_first > 0.) || std::isinf(tau_first))
        tau_first = 0.; /* invalid tau_max: the step ends in RYUJIN_ERR_TAU whatever the later stages see */
    }
    if (erk) {
      for (int st = 1; st < n_stages; ++st) {
        rk_stage = st;
        prepare_state_vector<E>(T[st - 1], dirichlet_at(st), device_dirichlet_at(st));
        pending_precompute = true;
        step<E>(T[st - 1], erk_stage[st].n, erk_stage[st].h, erk_stage[st].w, T[st], 1. /*device tau*/,
                no_limit, &dummy);
        result = T[st];
      }
    } else {
      /* sadd(dst, s, b, U) right after step(.., dst): folded into the last sweep of that step when there
       * is one (limiter iterations >= 1), saving one pass over the state vectors per stage */
      /* (not with the checked build's extra kernels: they look at the update before the sadd, as the reference does) */
      const bool fuse = params.limiter_iterations >= 1 && !params.debug_expensive_bounds_check;
      auto stage_with_sadd = [&](int h_old, int h_new, double sa, double sb) {
        struct Disarm { /* a step that throws before its last sweep must not leave the sadd armed */
          FusedSadd &p;
          ~Disarm() { p = FusedSadd{0., 0., nullptr}; }
        } disarm{pending_sadd};
        if (fuse)
          pending_sadd = FusedSadd{sa, sb, state(U).U.ptr};
        pending_precompute = fuse; /* (an sadd of its own rewrites the vector) */
        step<E>(h_old, 0, none, no_w, h_new, 1., no_limit, &dummy);
        if (!fuse)
          ryujin_hip_sadd(this, h_new, sa, sb, U);
      };
      rk_stage = 1;
      prepare_state_vector<E>(T[0], dirichlet_at(1), device_dirichlet_at(1));
      if (scheme == RYUJIN_SCHEME_SSPRK_22)
        stage_with_sadd(T[0], T[1], 1. / 2., 1. / 2.);
      else
        stage_with_sadd(T[0], T[1], 1. / 4., 3. / 4.);
      result = T[1];
      if (n_stages >= 3) {
        rk_stage = 2;
        prepare_state_vector<E>(T[1], dirichlet_at(2), device_dirichlet_at(2));
        stage_with_sadd(T[1], T[0], 2. / 3., 1. / 3.);
        result = T[0];
      }
    }
    /* the only host synchronisation of the RK step */
    join_export();
    hipLaunchKernelGGL(k_accumulate_flags, dim3(1), dim3(1), 0, stream, rk_stage, d_scalars.ptr);
    /* MPI::logical_or over the ranks of the flags accumulated over all stages (restart_accum and
     * tau_invalid_accum are adjacent ints): one collective per RK step instead of one per stage */
    static_assert(offsetof(DeviceScalars, tau_invalid_accum) ==
                      offsetof(DeviceScalars, restart_accum) + sizeof(int),
                  "flag accumulators must be adjacent");
    allreduce_scalar(&d_scalars.ptr->restart_accum, 1, 2);
    HIP_CHECK(hipMemcpyAsync(h_scalars, d_scalars.ptr, sizeof(DeviceScalars), hipMemcpyDeviceToHost,
                             stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    update_limited_fraction();
    if (timers_enabled) {
      for (int st = 0; st < n_stages; ++st) {
        for (int k = 0; k < 7; ++k) {
          float ms = 0.f;
          HIP_CHECK(hipEventElapsedTime(&ms, ev_rk[st][k], ev_rk[st][k + 1]));
          sweep_ms_accum[k + 1] += ms;
        }
        if (last_plan.step2_split) {
          float ms = 0.f;
          HIP_CHECK(hipEventElapsedTime(&ms, ev_rk[st][0], ev_rk[st][8]));
          sweep_ms_accum[0] += ms;
        }
        ++sweep_updates_accum;
      }
    }
    return result;
  };

  if (cfl_recovery == RYUJIN_CFL_RECOVERY_BANG_BANG) {
    params.id_violation_strategy = RYUJIN_IDV_RAISE_EXCEPTION;
    params.cfl = cfl_max;
  }
  int result = single_step();
  /* Both accumulators hold kStageCode - (first stage that raised the flag), max-reduced over the ranks.
   * Under raise_exception the reference throws Restart at the end of the offending stage and never
   * evaluates tau_max of a later one (hyperbolic_module.template.h:1194-1207), whereas here all stages are
   * already enqueued and run on the inadmissible state: an invalid tau_max only counts ("We crashed",
   * :573-576) if it was found in a stage not later than the first Restart. */
  const int first_outcome = ryujin_hip_debug_rk_outcome(h_scalars->restart_accum, h_scalars->tau_invalid_accum,
                                                         params.id_violation_strategy);
  if (first_outcome == RYUJIN_ERR_TAU)
    return RYUJIN_ERR_TAU;
  int status = RYUJIN_OK;
  if (h_scalars->restart_accum) {
    if (params.id_violation_strategy == RYUJIN_IDV_RAISE_EXCEPTION) {
      n_restarts++;
      if (cfl_recovery != RYUJIN_CFL_RECOVERY_BANG_BANG)
        return RYUJIN_RESTART; /* the caller owns the recovery: state vector untouched */
      params.id_violation_strategy = RYUJIN_IDV_WARN;
      params.cfl = cfl_min;
      result = single_step();
      if (h_scalars->tau_invalid_accum)
        return RYUJIN_ERR_TAU;
      if (h_scalars->restart_accum) {
        n_warnings++;
        status = RYUJIN_WARN;
      }
    } else {
      n_warnings++;
      status = RYUJIN_WARN;
    }
  }
  /* state_vector.swap(temp_[..]): the caller's handle keeps naming the solution */
  std::swap(states[U], states[result]);
  *tau_out = tau_factor * h_scalars->tau_rk;
  return status;
}

/* Postprocessor::compute() (source/postprocessor.template.h:108-271) on the device: ghost exchange of the state
 * vector (the sweep gathers ghost U_j), one sweep for all quantities, the bounds reduced over the ranks, the
 * normalisation. One rank / RCCL: nothing here waits for the device. */
template <typename E>
void ryujin_hip_ctx::postprocess_compute(int h)
{
  State &s = state(h);
  const uint32_t n_owned = L.n_owned;
  const int n = pp_desc.n;
  constexpr int MAXQ = kPostprocessMaxQuantities;
  if (d_pp_raw.n != (size_t)n * n_owned) {
    d_pp_raw.alloc((size_t)n * n_owned);
    d_pp_normalised.alloc((size_t)n * n_owned);
  }
  if (d_pp_bounds.n == 0)
    d_pp_bounds.alloc(2 * MAXQ);
  wait_comm();
  exchange_vector(s.U.ptr, KP, false);
  wait_comm();

  const bool fold_bounds = pp_recompute_bounds || !pp_have_bounds;
  if (fold_bounds)
    hipLaunchKernelGGL(k_postprocess_reset_bounds, dim3(1), dim3(64), 0, stream, d_pp_bounds.ptr);
  DeviceMesh mm = mesh;
  mm.begin = StepBegin{};
  mm.slice_begin = 0;
  mm.slice_end = L.n_slices;
  const dim3 grid((L.n_slices + kWavesPerBlock - 1) / kWavesPerBlock);
  hipLaunchKernelGGL((k_postprocess_sweep<E, tile_map_pays<E::DIMENSION>()>), grid, dim3(kBlock), 0, stream,
                     eq_params<E>(), mm, pp_desc, fold_bounds ? 1 : 0, s.U.ptr, d_pp_raw.ptr, d_pp_bounds.ptr);
  HIP_CHECK(hipGetLastError());

  if (fold_bounds) {
    /* q_max, then q_min (the bit patterns are those of non-negative doubles: reduced as doubles) */
    static_assert(2 * MAXQ <= kRankReduceMaxValues, "HostRendezvous::scratch holds a row per rank");
    reduce_over_ranks(reinterpret_cast<double *>(d_pp_bounds.ptr),
                      {{MAXQ, RankReduceOp::Max}, {MAXQ, RankReduceOp::Min}});
  }
  pp_have_bounds = true;

  const size_t total = (size_t)n * n_owned;
  hipLaunchKernelGGL(k_postprocess_normalise, dim3(std::min<size_t>(grid_for(total), 4096)), dim3(kBlock), 0, stream,
                     n_owned, n, pp_beta, d_pp_bounds.ptr, d_pp_raw.ptr, d_pp_normalised.ptr);
  HIP_CHECK(hipGetLastError());
  pp_computed = true;
}

/* internal_accumulate() of one manifold on state h. accumulate: the trapezoid update, the weighted sums over all
 * ranks and one row of the time series as well (Quantities::accumulate, :516-549); otherwise only the values
 * (write_out of an "instantaneous" manifold that is not averaged, :615-617). */
template <typename E>
void ryujin_hip_ctx::quantities_evaluate(Manifold &m, int h, bool accumulate, double t)
{
  constexpr int NQ = 1 + 2 * E::K;
  static_assert(NQ <= kRankReduceMaxValues, "HostRendezvous::scratch holds a row per rank");
  State &s = state(h);
  const bool time_averaged = (m.options & RYUJIN_Q_TIME_AVERAGED) != 0;

  QuantitiesSweep S{};
  S.n_points = m.n_points;
  S.first = m.first;
  S.index = m.d_index.ptr;
  S.weight = m.d_weight.ptr;
  S.store = m.d_values.n != 0;
  S.values = m.d_values.ptr;
  S.sum = m.d_sum.ptr;
  S.partial = m.d_partial.ptr;
  S.reduce = accumulate;

  if (accumulate) {
    std::swap(m.t_old, m.t_new); /* (:519; the values are not swapped: one array, updated behind the sum) */
    if (m.t_old == 0. && m.t_new == 0.) {
      /* We have not accumulated any statistics yet (:529-532) */
      m.t_old = t - 1.;
      m.t_new = t;
    } else {
      m.t_new = t;
      const double tau = m.t_new - m.t_old;
      S.add = time_averaged;
      S.half_tau = 0.5 * tau;
      m.t_sum += tau;
    }
  }

  if (m.n_points > 0) { /* (no zero-sized grid) */
    if (m.contiguous)
      hipLaunchKernelGGL((k_quantities_sweep<E, false>), dim3(m.n_blocks), dim3(kBlock), 0, stream, eq_params<E>(), S,
                         s.U.ptr);
    else
      hipLaunchKernelGGL((k_quantities_sweep<E, true>), dim3(m.n_blocks), dim3(kBlock), 0, stream, eq_params<E>(), S,
                         s.U.ptr);
    HIP_CHECK(hipGetLastError());
  }
  m.have_values = true;
  if (!accumulate)
    return;

  /* one row of the time series (:549) */
  const size_t chunk = m.n_rows / kSeriesChunkRows;
  if (chunk >= m.series.size()) {
    m.series.emplace_back(new DeviceBuffer<double>());
    m.series.back()->alloc(kSeriesChunkRows * NQ, false);
  }
  double *row = m.series[chunk]->ptr + (m.n_rows % kSeriesChunkRows) * NQ;
  double *sums = m.d_partial.ptr + (size_t)m.n_blocks * NQ;
  hipLaunchKernelGGL(k_quantities_final<NQ>, dim3(1), dim3(64), 0, stream, m.n_points > 0 ? m.n_blocks : 0u,
                     m.d_partial.ptr, t, sums, several_ranks() ? nullptr : row);
  HIP_CHECK(hipGetLastError());
  if (reduce_over_ranks(sums, {{NQ, RankReduceOp::Sum}})) {
    hipLaunchKernelGGL(k_quantities_row<NQ>, dim3(1), dim3(64), 0, stream, sums, t, row);
    HIP_CHECK(hipGetLastError());
  }
  ++m.n_rows;
}

/* TimeLoop::compute_error() (source/time_loop.template.h:692-833) behind prepare_state_vector and the analytic
 * vector: ghost exchange of the state vector (the cells of this rank reach into the ghost range), the nodal maxima,
 * the cell integrals, both reduced over the ranks, then roots, ratios and the consolidated sums on the device. The
 * result row is the one copy to the host. */
void ryujin_hip_ctx::error_norms_compute(int h_state, int h_analytic, const ErrorNormsDesc &D, double *host_result)
{
  constexpr int NS = kErrorNormsSums, MAXC = kErrorNormsMaxComponents;
  static_assert(NS + 2 * MAXC <= kRankReduceMaxValues, "HostRendezvous::scratch holds a row per rank");
  static_assert(sizeof(unsigned long long) == sizeof(double), "sums and max_bits are reduced as one row of doubles");
  ErrorNorms &en = *error_norms;
  State &s = state(h_state);
  State &a = state(h_analytic);
  wait_comm();
  exchange_vector(s.U.ptr, KP, false);
  wait_comm();

  double *partial = en.d_work.ptr;
  double *sums = partial + (size_t)en.n_blocks * NS;
  unsigned long long *max_bits = reinterpret_cast<unsigned long long *>(sums + NS);
  double *result = sums + NS + 2 * MAXC;
  HIP_CHECK(hipMemsetAsync(max_bits, 0, sizeof(unsigned long long) * 2 * MAXC, stream)); /* max |.| starts from 0 */
  if (L.n_owned > 0) {
    const uint32_t blocks = (uint32_t)std::min<size_t>(kErrorNormsMaxBlocks, ((size_t)L.n_owned + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_error_norms_nodal, dim3(blocks), dim3(kBlock), 0, stream, L.n_owned, D, s.U.ptr, a.U.ptr,
                       max_bits);
    HIP_CHECK(hipGetLastError());
  }
  if (en.n_cells > 0) { /* (no zero-sized grid) */
    ErrorNormsCells C{};
    C.n_cells = en.n_cells;
    C.dofs_per_cell = en.dofs_per_cell;
    C.n_q = en.n_q;
    C.jxw_per_cell = en.jxw_per_cell;
    C.cell_dofs = en.d_cell_dofs.ptr;
    C.jxw = en.d_jxw.ptr;
    C.shape = en.d_shape.ptr;
    C.weights = en.d_weights.ptr;
    C.partial = partial;
    const dim3 grid(en.n_blocks), block(kBlock);
    if (en.dofs_per_cell == 2 && en.n_q == 3)
      hipLaunchKernelGGL((k_error_norms_cells<2, 3>), grid, block, 0, stream, D, C, s.U.ptr, a.U.ptr);
    else if (en.dofs_per_cell == 4 && en.n_q == 9)
      hipLaunchKernelGGL((k_error_norms_cells<4, 9>), grid, block, 0, stream, D, C, s.U.ptr, a.U.ptr);
    else if (en.dofs_per_cell == 8 && en.n_q == 27)
      hipLaunchKernelGGL((k_error_norms_cells<8, 27>), grid, block, 0, stream, D, C, s.U.ptr, a.U.ptr);
    else
      hipLaunchKernelGGL((k_error_norms_cells<0, 0>), grid, block, 0, stream, D, C, s.U.ptr, a.U.ptr);
    HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_error_norms_final, dim3(1), dim3(64), 0, stream, D, en.n_blocks, partial, sums, max_bits,
                     several_ranks() ? nullptr : result);
  HIP_CHECK(hipGetLastError());
  /* the sums, then the maxima behind them (bit patterns of non-negative doubles: reduced as doubles) */
  if (reduce_over_ranks(sums, {{NS, RankReduceOp::Sum}, {2 * MAXC, RankReduceOp::Max}})) {
    hipLaunchKernelGGL(k_error_norms_result, dim3(1), dim3(64), 0, stream, D, sums, max_bits, result);
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipMemcpyAsync(host_result, result, sizeof(double) * kErrorNormsResult, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
}

/* ============================================================================ C ABI */

namespace
{
  template <typename F>
  int guarded(F &&f)
  {
    try {
      return f();
    } catch (const HipError &e) {
      g_error = e.what();
      return e.status;
    } catch (const RankGroupAborted &e) {
      g_error = e.what();
      return RYUJIN_ERR_COMM;
    } catch (const std::invalid_argument &e) {
      g_error = e.what();
      return RYUJIN_ERR_ARG;
    } catch (const std::exception &e) {
      g_error = e.what();
      return RYUJIN_ERR_HIP;
    }
  }

  /* entry points that touch the device: make the context's device current first (a host thread may drive
   * contexts on several devices) */
  template <typename F>
  int guarded_ctx(ryujin_hip_ctx *ctx, F &&f)
  {
    const int status = guarded([&]() {
      if (!ctx)
        throw HipError(RYUJIN_ERR_ARG, "null context");
      HIP_CHECK(hipSetDevice(ctx->device));
      return f();
    });
    /* in-process transport: a rank that failed must not leave the rank threads of its group waiting for it */
    if (status < 0 && status != RYUJIN_ERR_TAU && ctx && ctx->comm && ctx->comm->local)
      ctx->comm->local->abort();
    return status;
  }

  /* the arguments of a Runge-Kutta step (ryujin_hip_time_step_n, _fn, _iv): RYUJIN_OK, or RYUJIN_ERR_TAU by the
   * tau_max rule of step(); every other error throws */
  int check_time_step_args(ryujin_hip_ctx *ctx, int h_state, int n_tmp, const int *h_tmp, double tau_max,
                           const double *tau_out)
  {
    if (!h_tmp || !tau_out || n_tmp < 1 || n_tmp > 8)
      throw HipError(RYUJIN_ERR_ARG, "time_step: bad argument");
    if (std::isnan(tau_max) || !(tau_max > 0.))
      return RYUJIN_ERR_TAU; /* as in step() */
    ctx->state(h_state);
    for (int q = 0; q < n_tmp; ++q) {
      ctx->state(h_tmp[q]);
      if (h_tmp[q] == h_state)
        throw HipError(RYUJIN_ERR_ARG, "time_step: temporary vectors must differ from the state vector");
      for (int r = 0; r < q; ++r)
        if (h_tmp[r] == h_tmp[q])
          throw HipError(RYUJIN_ERR_ARG, "time_step: temporary vectors must be distinct");
    }
    return RYUJIN_OK;
  }

  template <typename E>
  struct EqTag {
    using type = E;
  };

  template <typename F>
  auto dispatch_equation(int equation, int dim, F &&f)
  {
    if (equation == RYUJIN_EQ_SHALLOW_WATER) {
      if (dim == 1)
        return f(EqTag<ShallowWater<1>>{});
      return f(EqTag<ShallowWater<2>>{});
    }
    if (equation == RYUJIN_EQ_SCALAR_CONSERVATION) {
      switch (dim) {
      case 1: return f(EqTag<ScalarConservation<1>>{});
      case 2: return f(EqTag<ScalarConservation<2>>{});
      default: return f(EqTag<ScalarConservation<3>>{});
      }
    }
    if (equation == RYUJIN_EQ_EULER_AEOS) {
      switch (dim) {
      case 1: return f(EqTag<EulerAeos<1>>{});
      case 2: return f(EqTag<EulerAeos<2>>{});
      default: return f(EqTag<EulerAeos<3>>{});
      }
    }
    switch (dim) {
    case 1: return f(EqTag<Euler<1>>{});
    case 2: return f(EqTag<Euler<2>>{});
    default: return f(EqTag<Euler<3>>{});
    }
  }

  /* system_shape() (host_context.hpp) against the Descriptions of the device headers */
  template <typename E>
  constexpr bool shape_matches(const int equation)
  {
    const SystemShape s = system_shape(equation, E::DIMENSION);
    bool ok = s.K == E::K && s.KP == StatePad<E::K>::KP && s.NB == E::NB;
    if constexpr (is_scalar_v<E>)
      ok = ok && s.NPREC == E::NPREC && s.RS == 0 && s.RS_stored == 0;
    else
      ok = ok && s.RS == E::RS;
    if constexpr (is_euler_v<E> || is_sw_v<E>) /* the generic kernels: load_record(), store_record() */
      ok = ok && s.RS_stored == E::kRecordStored;
    else if constexpr (is_aeos_v<E>)
      ok = ok && s.RS_stored == E::RS;
    if constexpr (is_aeos_v<E>)
      ok = ok && s.NPREC == E::NPREC;
    return ok;
  }
  static_assert(shape_matches<Euler<1>>(RYUJIN_EQ_EULER) && shape_matches<Euler<2>>(RYUJIN_EQ_EULER) &&
                    shape_matches<Euler<3>>(RYUJIN_EQ_EULER),
                "system_shape(): Euler");
  static_assert(shape_matches<EulerAeos<1>>(RYUJIN_EQ_EULER_AEOS) && shape_matches<EulerAeos<2>>(RYUJIN_EQ_EULER_AEOS) &&
                    shape_matches<EulerAeos<3>>(RYUJIN_EQ_EULER_AEOS),
                "system_shape(): EulerAEOS");
  static_assert(shape_matches<ShallowWater<1>>(RYUJIN_EQ_SHALLOW_WATER) &&
                    shape_matches<ShallowWater<2>>(RYUJIN_EQ_SHALLOW_WATER),
                "system_shape(): shallow water");
  static_assert(shape_matches<ScalarConservation<1>>(RYUJIN_EQ_SCALAR_CONSERVATION) &&
                    shape_matches<ScalarConservation<2>>(RYUJIN_EQ_SCALAR_CONSERVATION) &&
                    shape_matches<ScalarConservation<3>>(RYUJIN_EQ_SCALAR_CONSERVATION),
                "system_shape(): scalar conservation");

  /* n rows from row `first` on between an AoS host array of stride K and the device array of stride KP */
  template <bool kUpload>
  void transfer_rows(const ryujin_hip_ctx &ctx, double *dev, std::conditional_t<kUpload, const double, double> *host,
                     const size_t first, const size_t n)
  {
    const size_t K = ctx.K, KP = ctx.KP;
    dev += first * KP;
    host += first * K;
    std::vector<double> tmp(K == KP ? 0 : n * KP, 0.);
    if constexpr (kUpload) {
      for (size_t i = 0; i < n && K != KP; ++i)
        std::memcpy(&tmp[i * KP], &host[i * K], sizeof(double) * K);
      HIP_CHECK(hipMemcpy(dev, K == KP ? host : tmp.data(), n * KP * sizeof(double), hipMemcpyHostToDevice));
    } else {
      HIP_CHECK(hipMemcpy(K == KP ? host : tmp.data(), dev, n * KP * sizeof(double), hipMemcpyDeviceToHost));
      for (size_t i = 0; i < n && K != KP; ++i)
        std::memcpy(&host[i * K], &tmp[i * KP], sizeof(double) * K);
    }
  }
} // namespace

extern "C" {

const char *ryujin_hip_last_error(void)
{
  return g_error.c_str();
}

const char *ryujin_hip_version(void)
{
  return "ryujin_hip 0.4 (gfx950; Euler, Euler AEOS, shallow water, scalar conservation; SELL-64)";
}

void ryujin_hip_default_params(ryujin_hip_params *p, int equation, int dim)
{
  std::memset(p, 0, sizeof(*p));
  p->equation = equation;
  p->dim = dim;
  p->gamma = 7. / 5.;
  p->reference_density = 1.;
  p->vacuum_state_relaxation_small = 1.e2;
  p->vacuum_state_relaxation_large = 1.e4;
  p->gravity = 9.81;
  p->manning_friction_coefficient = 0.;
  p->reference_water_depth = 1.;
  p->dry_state_relaxation_factor = 2.e-1;
  p->dry_state_relaxation_small = 1.e2;
  p->dry_state_relaxation_large = 1.e4;
  p->cfl = 0.2;
  p->id_violation_strategy = RYUJIN_IDV_WARN;
  p->indicator_evc_factor = 1.;
  p->limiter_iterations = 2;
  p->limiter_newton_tolerance = 1.e-10;
  p->limiter_newton_max_iterations = 2;
  p->limiter_relaxation_factor = 1.;
  p->limiter_limit_on_kinetic_energy = 0;
  p->limiter_limit_on_square_velocity = 1;
  p->riemann_newton_max_iterations = 0;
  p->riemann_newton_tolerance = 1.e-10;
  p->eos = RYUJIN_EOS_POLYTROPIC_GAS;
  p->compute_strict_bounds = 1;
  p->eos_covolume_b = 0.;
  p->eos_q = 0.;
  p->eos_pinf = 0.;
  p->eos_vdw_a = 0.;
  p->eos_gas_constant_R = 287.052874;
  p->jwl_A = 6.3207e13;
  p->jwl_B = -4.472e9;
  p->jwl_R1 = 11.3;
  p->jwl_R2 = 1.13;
  p->jwl_omega = 0.8938;
  p->jwl_rho_0 = 1895.;
  p->jwl_q_0 = 0.;
  p->jwl_cv = 2487. / 1895.;
  p->sc_flux = RYUJIN_FLUX_BURGERS;
  p->sc_flux_polynomial[0][2] = 0.5; /* "0.5*u*u", the default expression of flux_function.h:32 */
  p->sc_derivative_approximation_delta = 1.e-10;
  p->sc_use_greedy_wavespeed = 0;
  p->sc_use_averaged_entropy = 0;
  p->sc_random_entropies = 0;
  p->system_scope_events = 0;
  p->debug_join_exchanges = 0;
  p->debug_bc_fold_max_slices = 0;
  p->debug_no_small_mesh_split = 0;
  p->debug_pij_storage = 0;
  p->debug_expensive_bounds_check = 0;
  p->debug_tile_map = 0;
  p->debug_band_stride = 0;
  p->debug_xcd_chunk = 0;
  p->debug_stencil_classes = 0;
  p->debug_next_tile_mask = 0;
  /* the profiling scripts wrap bench.py, which takes the defaults: let them select a mapping without a flag */
  if (const char *e = std::getenv("RYUJIN_XCD_CHUNK"))
    p->debug_xcd_chunk = std::atoi(e);
  if (const char *e = std::getenv("RYUJIN_BAND_STRIDE"))
    p->debug_band_stride = std::atoi(e);
}

int ryujin_hip_comm_unique_id(char id[RYUJIN_HIP_UNIQUE_ID_BYTES])
{
  return guarded([&]() {
    static_assert(sizeof(ncclUniqueId) <= RYUJIN_HIP_UNIQUE_ID_BYTES, "unique id size");
    ncclUniqueId uid;
    NCCL_CHECK(ncclGetUniqueId(&uid));
    std::memset(id, 0, RYUJIN_HIP_UNIQUE_ID_BYTES);
    std::memcpy(id, &uid, sizeof(uid));
    return RYUJIN_OK;
  });
}

int ryujin_hip_comm_init(ryujin_hip_comm **comm, const char id[RYUJIN_HIP_UNIQUE_ID_BYTES], int rank,
                         int n_ranks, int device)
{
  return guarded([&]() {
    auto c = std::make_unique<ryujin_hip_comm>();
    c->rank = rank;
    c->n_ranks = n_ranks;
    c->device = device;
    HIP_CHECK(hipSetDevice(device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    NCCL_CHECK(ncclCommInitRank(&c->comm, n_ranks, uid, rank));
    *comm = c.release();
    return RYUJIN_OK;
  });
}

int ryujin_hip_comm_init_local(ryujin_hip_comm **comms, int n_ranks, int device)
{
  return guarded([&]() {
    if (n_ranks < 1)
      throw HipError(RYUJIN_ERR_ARG, "n_ranks must be positive");
    auto *group = new LocalGroup(n_ranks, device);
    group->refs = n_ranks;
    for (int r = 0; r < n_ranks; ++r) {
      auto *c = new ryujin_hip_comm;
      c->rank = r;
      c->n_ranks = n_ranks;
      c->device = device;
      c->local = group;
      comms[r] = c;
    }
    return RYUJIN_OK;
  });
}

int ryujin_hip_comm_init_loopback(ryujin_hip_comm **comm, int rank, int n_ranks, int device)
{
  return guarded([&]() {
    if (!comm || n_ranks < 2 || rank < 0 || rank >= n_ranks)
      throw HipError(RYUJIN_ERR_ARG, "loopback communicator: 0 <= rank < n_ranks, n_ranks >= 2");
    auto *group = new LocalGroup(n_ranks, device);
    group->refs = 1;
    group->loopback = true;
    auto *c = new ryujin_hip_comm;
    c->rank = rank;
    c->n_ranks = n_ranks;
    c->device = device;
    c->local = group;
    *comm = c;
    return RYUJIN_OK;
  });
}

void ryujin_hip_comm_destroy(ryujin_hip_comm *comm)
{
  if (!comm)
    return;
  if (comm->local) {
    bool last;
    {
      std::lock_guard<std::mutex> lock(comm->local->mtx);
      last = --comm->local->refs == 0;
    }
    if (last)
      delete comm->local;
  }
  if (comm->comm)
    (void)ncclCommDestroy(comm->comm);
  delete comm;
}

int ryujin_hip_comm_info(const ryujin_hip_comm *comm, int *rank, int *n_ranks, int *rccl_rank, int *rccl_count,
                         int *rccl_device)
{
  return guarded([&]() {
    if (!comm)
      throw HipError(RYUJIN_ERR_ARG, "null communicator");
    int r = -1, n = -1, d = -1;
    if (comm->comm) {
      NCCL_CHECK(ncclCommUserRank(comm->comm, &r));
      NCCL_CHECK(ncclCommCount(comm->comm, &n));
      NCCL_CHECK(ncclCommCuDevice(comm->comm, &d));
    }
    if (rank)
      *rank = comm->rank;
    if (n_ranks)
      *n_ranks = comm->n_ranks;
    if (rccl_rank)
      *rccl_rank = r;
    if (rccl_count)
      *rccl_count = n;
    if (rccl_device)
      *rccl_device = d;
    return RYUJIN_OK;
  });
}

int ryujin_hip_exchange_info(ryujin_hip_ctx *ctx, int *n_nbr, int *nbr_rank, int max_nbr,
                             unsigned long long *n_exchanges, unsigned long long *n_allreduces)
{
  return guarded([&]() {
    if (!ctx)
      throw HipError(RYUJIN_ERR_ARG, "null context");
    if (n_nbr)
      *n_nbr = ctx->exch.n_nbr;
    if (nbr_rank)
      for (int q = 0; q < ctx->exch.n_nbr && q < max_nbr; ++q)
        nbr_rank[q] = ctx->exch.nbr_rank[q];
    if (n_exchanges)
      *n_exchanges = ctx->n_exchanges;
    if (n_allreduces)
      *n_allreduces = ctx->n_allreduces;
    return RYUJIN_OK;
  });
}

int ryujin_hip_create(ryujin_hip_ctx **ctx, const ryujin_hip_offline *offline,
                      const ryujin_hip_params *params, ryujin_hip_comm *comm, int device)
{
  return guarded([&]() {
    if (!ctx || !offline || !params)
      throw HipError(RYUJIN_ERR_ARG, "null argument");
    auto c = std::make_unique<ryujin_hip_ctx>();
    c->create(*offline, *params, comm, device);
    *ctx = c.release();
    return RYUJIN_OK;
  });
}

void ryujin_hip_destroy(ryujin_hip_ctx *ctx)
{
  delete ctx;
}

int ryujin_hip_state_alloc(ryujin_hip_ctx *ctx, int *handle)
{
  return guarded_ctx(ctx, [&]() {
    int h = -1;
    for (size_t q = 0; q < ctx->states.size(); ++q)
      if (!ctx->states[q]->used) {
        h = (int)q;
        break;
      }
    if (h < 0) {
      ctx->states.push_back(std::make_unique<ryujin_hip_ctx::State>());
      h = (int)ctx->states.size() - 1;
      ctx->states[h]->U.alloc((size_t)ctx->L.n_relevant * ctx->KP);
      ctx->states[h]->prec.alloc((size_t)ctx->L.n_relevant * ctx->NPREC);
      if (ctx->RS_stored != 0) /* E::kRecordStored; scalar conservation keeps no node records */
        ctx->states[h]->rrec.alloc((size_t)ctx->L.n_relevant * ctx->RS_stored);
    }
    ctx->states[h]->used = true;
    ctx->states[h]->precomputed = false;
    ctx->states[h]->prepared = false;
    *handle = h;
    return RYUJIN_OK;
  });
}

int ryujin_hip_state_free(ryujin_hip_ctx *ctx, int handle)
{
  return guarded_ctx(ctx, [&]() {
    ctx->state(handle).used = false;
    return RYUJIN_OK;
  });
}

int ryujin_hip_state_upload(ryujin_hip_ctx *ctx, int handle, const double *U_aos)
{
  return guarded_ctx(ctx, [&]() {
    auto &s = ctx->state(handle);
    ctx->finish();
    s.precomputed = false;
    transfer_rows<true>(*ctx, s.U.ptr, U_aos, 0, ctx->L.n_relevant);
    return RYUJIN_OK;
  });
}

int ryujin_hip_state_download(ryujin_hip_ctx *ctx, int handle, double *U_aos)
{
  return guarded_ctx(ctx, [&]() {
    auto &s = ctx->state(handle);
    ctx->finish();
    transfer_rows<false>(*ctx, s.U.ptr, U_aos, 0, ctx->L.n_relevant);
    return RYUJIN_OK;
  });
}

int ryujin_hip_state_download_precomputed(ryujin_hip_ctx *ctx, int handle, double *prec_aos)
{
  return guarded_ctx(ctx, [&]() {
    auto &s = ctx->state(handle);
    ctx->finish();
    HIP_CHECK(hipMemcpy(prec_aos, s.prec.ptr, (size_t)ctx->L.n_relevant * ctx->NPREC * sizeof(double),
                        hipMemcpyDeviceToHost));
    return RYUJIN_OK;
  });
}

int ryujin_hip_host_register(ryujin_hip_ctx *ctx, const void *ptr, size_t bytes)
{
  return guarded_ctx(ctx, [&]() {
    if (!ptr || bytes == 0)
      throw HipError(RYUJIN_ERR_ARG, "host_register: null or empty range");
    /* a range that is registered already is registered AGAIN: the caller's allocator may have released the
     * memory and handed the same address out anew in the meantime, and the old pinning does not cover the new pages */
    const auto known = std::find(ctx->registered_host.begin(), ctx->registered_host.end(), ptr);
    if (known != ctx->registered_host.end()) {
      ctx->finish();
      if (hipHostUnregister(const_cast<void *>(ptr)) != hipSuccess)
        (void)hipGetLastError();
      ctx->registered_host.erase(known);
    }
    if (hipHostRegister(const_cast<void *>(ptr), bytes, hipHostRegisterDefault) != hipSuccess) {
      (void)hipGetLastError(); /* not fatal: transfers of pageable memory are staged by the runtime */
      return RYUJIN_WARN;
    }
    ctx->registered_host.push_back(ptr);
    return RYUJIN_OK;
  });
}

int ryujin_hip_host_unregister(ryujin_hip_ctx *ctx, const void *ptr)
{
  return guarded_ctx(ctx, [&]() {
    const auto it = std::find(ctx->registered_host.begin(), ctx->registered_host.end(), ptr);
    if (it == ctx->registered_host.end())
      return RYUJIN_WARN;
    ctx->finish();
    HIP_CHECK(hipHostUnregister(const_cast<void *>(ptr)));
    ctx->registered_host.erase(it);
    return RYUJIN_OK;
  });
}

int ryujin_hip_state_download_owned(ryujin_hip_ctx *ctx, int handle, double *U_aos)
{
  return guarded_ctx(ctx, [&]() {
    auto &s = ctx->state(handle);
    ctx->finish();
    transfer_rows<false>(*ctx, s.U.ptr, U_aos, 0, ctx->L.n_owned);
    return RYUJIN_OK;
  });
}

int ryujin_hip_state_download_prepared(ryujin_hip_ctx *ctx, int handle, double *U_aos)
{
  return guarded_ctx(ctx, [&]() {
    auto &s = ctx->state(handle);
    const int K = ctx->K, KP = ctx->KP;
    const uint32_t n_rows = (uint32_t)ctx->bdry.rows.size();
    /* boundary rows inside export slices get their boundary conditions from the export part of the pre-pass, on
     * comm_stream (fold_bc): the pack kernel below reads them, so the compute stream joins comm_stream FIRST */
    ctx->wait_comm();
    if (n_rows != 0) {
      if (ctx->d_bc_rows.n == 0) {
        ctx->d_bc_rows.upload(ctx->bdry.rows);
        ctx->d_bc_pack.alloc((size_t)n_rows * KP);
        HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&ctx->h_bc_pack), (size_t)n_rows * KP * sizeof(double)));
      }
      hipLaunchKernelGGL(k_pack_vector, dim3(grid_for((size_t)n_rows * KP)), dim3(kBlock), 0, ctx->stream, n_rows,
                         ctx->d_bc_rows.ptr, KP, s.U.ptr, ctx->d_bc_pack.ptr);
      HIP_CHECK(hipGetLastError());
    }
    ctx->finish();
    if (n_rows != 0) {
      HIP_CHECK(hipMemcpy(ctx->h_bc_pack, ctx->d_bc_pack.ptr, (size_t)n_rows * KP * sizeof(double),
                          hipMemcpyDeviceToHost));
      for (uint32_t q = 0; q < n_rows; ++q)
        std::memcpy(&U_aos[(size_t)ctx->bdry.rows[q] * K], &ctx->h_bc_pack[(size_t)q * KP], sizeof(double) * K);
    }
    /* the ghost range [n_owned, n_relevant) */
    if (ctx->L.n_relevant != ctx->L.n_owned)
      transfer_rows<false>(*ctx, s.U.ptr, U_aos, ctx->L.n_owned, ctx->L.n_relevant - ctx->L.n_owned);
    return RYUJIN_OK;
  });
}

int ryujin_hip_prepare_state_vector(ryujin_hip_ctx *ctx, int handle, double /*t*/,
                                    const double *dirichlet_aos)
{
  return guarded_ctx(ctx, [&]() {
    dispatch_equation(ctx->params.equation, ctx->dim, [&](auto tag) {
      ctx->template prepare_state_vector<typename decltype(tag)::type>(handle, dirichlet_aos);
      return 0;
    });
    return RYUJIN_OK;
  });
}

int ryujin_hip_step(ryujin_hip_ctx *ctx, int h_old, int stages, const int *h_stage,
                    const double *stage_weights, int h_new, double tau_in, double tau_max_in,
                    double *tau_out)
{
  return guarded_ctx(ctx, [&]() {
    if (stages < 0 || stages > 4 || !tau_out)
      throw HipError(RYUJIN_ERR_ARG, "stages must be in [0,4]");
    /* tau_max = min(tau_max argument, CFL bound) must be positive and finite (:571-576). The device
     * minimum works on the bit patterns of positive doubles, so a NaN or non-positive argument -- which
     * makes the reference throw whatever the CFL bound is -- is caught here. */
    if (std::isnan(tau_max_in) || !(tau_max_in > 0.))
      return RYUJIN_ERR_TAU;
    return dispatch_equation(ctx->params.equation, ctx->dim, [&](auto tag) {
      return ctx->template step<typename decltype(tag)::type>(h_old, stages, h_stage, stage_weights,
                                                              h_new, tau_in, tau_max_in, tau_out);
    });
  });
}

int ryujin_hip_time_step_n(ryujin_hip_ctx *ctx, int scheme, int h_state, int n_tmp, const int *h_tmp,
                           const double *dirichlet_aos, double tau_max, int cfl_recovery,
                           double cfl_min, double cfl_max, double *tau_out)
{
  return guarded_ctx(ctx, [&]() {
    if (const int status = check_time_step_args(ctx, h_state, n_tmp, h_tmp, tau_max, tau_out))
      return status;
    return dispatch_equation(ctx->params.equation, ctx->dim, [&](auto tag) {
      return ctx->template time_step<typename decltype(tag)::type>(scheme, h_state, n_tmp, h_tmp,
                                                                   dirichlet_aos, tau_max, cfl_recovery,
                                                                   cfl_min, cfl_max, tau_out);
    });
  });
}

int ryujin_hip_time_step_fn(ryujin_hip_ctx *ctx, int scheme, int h_state, int n_tmp, const int *h_tmp, double t,
                            ryujin_hip_dirichlet_fn dirichlet_fn, void *user, double tau_max, int cfl_recovery,
                            double cfl_min, double cfl_max, double *tau_out)
{
  return guarded_ctx(ctx, [&]() {
    if (const int status = check_time_step_args(ctx, h_state, n_tmp, h_tmp, tau_max, tau_out))
      return status;
    return dispatch_equation(ctx->params.equation, ctx->dim, [&](auto tag) {
      return ctx->template time_step<typename decltype(tag)::type>(scheme, h_state, n_tmp, h_tmp, nullptr, tau_max,
                                                                   cfl_recovery, cfl_min, cfl_max, tau_out, t,
                                                                   dirichlet_fn, user);
    });
  });
}

int ryujin_hip_device_count(int *n_devices)
{
  return guarded([&]() {
    if (!n_devices)
      throw HipError(RYUJIN_ERR_ARG, "null argument");
    HIP_CHECK(hipGetDeviceCount(n_devices));
    return RYUJIN_OK;
  });
}

int ryujin_hip_time_step(ryujin_hip_ctx *ctx, int scheme, int h_state, const int h_tmp[3],
                         const double *dirichlet_aos, double tau_max, int cfl_recovery, double cfl_min,
                         double cfl_max, double *tau_out)
{
  return ryujin_hip_time_step_n(ctx, scheme, h_state, 3, h_tmp, dirichlet_aos, tau_max, cfl_recovery,
                                cfl_min, cfl_max, tau_out);
}

int ryujin_hip_get_timers_accum(ryujin_hip_ctx *ctx, double ms[8], unsigned *n_updates, int reset)
{
  return guarded([&]() {
    if (!ctx || !ms || !n_updates)
      throw HipError(RYUJIN_ERR_ARG, "null argument");
    for (int k = 0; k < 8; ++k)
      ms[k] = ctx->sweep_ms_accum[k];
    *n_updates = ctx->sweep_updates_accum;
    if (reset) {
      for (auto &v : ctx->sweep_ms_accum)
        v = 0.;
      ctx->sweep_updates_accum = 0;
    }
    return RYUJIN_OK;
  });
}

int ryujin_hip_sadd(ryujin_hip_ctx *ctx, int h_dst, double s, double b, int h_src)
{
  return guarded_ctx(ctx, [&]() {
    auto &dst = ctx->state(h_dst);
    auto &src = ctx->state(h_src);
    const size_t n = (size_t)ctx->L.n_relevant * ctx->KP;
    dst.precomputed = false;
    ctx->wait_comm();
    const int grid = (int)std::min<size_t>(2048, (n / 2 + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_sadd, dim3(std::max(1, grid)), dim3(kBlock), 0, ctx->stream, n, s, b,
                       dst.U.ptr, src.U.ptr);
    HIP_CHECK(hipGetLastError());
    return RYUJIN_OK;
  });
}

int ryujin_hip_set_cfl(ryujin_hip_ctx *ctx, double cfl)
{
  ctx->params.cfl = cfl;
  return RYUJIN_OK;
}

int ryujin_hip_get_cfl(ryujin_hip_ctx *ctx, double *cfl)
{
  *cfl = ctx->params.cfl;
  return RYUJIN_OK;
}

int ryujin_hip_set_id_violation_strategy(ryujin_hip_ctx *ctx, int strategy)
{
  ctx->params.id_violation_strategy = strategy;
  return RYUJIN_OK;
}

int ryujin_hip_get_alpha(ryujin_hip_ctx *ctx, double *alpha)
{
  return guarded_ctx(ctx, [&]() {
    ctx->finish();
    HIP_CHECK(hipMemcpy(alpha, ctx->d_alpha.ptr, (size_t)ctx->L.n_relevant * sizeof(double),
                        hipMemcpyDeviceToHost));
    return RYUJIN_OK;
  });
}

int ryujin_hip_state_integrals(ryujin_hip_ctx *ctx, int handle, double *out)
{
  return guarded_ctx(ctx, [&]() {
    if (!out)
      throw HipError(RYUJIN_ERR_ARG, "null argument");
    auto &st = ctx->state(handle);
    ctx->wait_comm();
    constexpr uint32_t n_blocks = 512;
    const int K = ctx->K;
    if (ctx->d_integrals.n < (size_t)(n_blocks + 1) * 8)
      ctx->d_integrals.alloc((size_t)(n_blocks + 1) * 8);
    double *partial = ctx->d_integrals.ptr, *result = ctx->d_integrals.ptr + (size_t)n_blocks * 8;
    auto launch = [&](auto tag) {
      constexpr int KK = decltype(tag)::value;
      hipLaunchKernelGGL(k_integrals_partial<KK>, dim3(n_blocks), dim3(kBlock), 0, ctx->stream,
                         ctx->L.n_owned, ctx->d_mi.ptr, st.U.ptr, partial);
      hipLaunchKernelGGL(k_integrals_final<KK>, dim3(1), dim3(64), 0, ctx->stream, n_blocks, partial,
                         result);
    };
    switch (K) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    default: launch(std::integral_constant<int, 5>{}); break;
    }
    HIP_CHECK(hipGetLastError());
    ctx->reduce_over_ranks(result, {{K, RankReduceOp::Sum}}, false);
    HIP_CHECK(hipMemcpyAsync(out, result, sizeof(double) * K, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RYUJIN_OK;
  });
}

int ryujin_hip_get_counters(ryujin_hip_ctx *ctx, unsigned *n_restarts, unsigned *n_warnings)
{
  *n_restarts = ctx->n_restarts;
  *n_warnings = ctx->n_warnings;
  return RYUJIN_OK;
}

int ryujin_hip_limiter_statistics(ryujin_hip_ctx *ctx, double *limited_slice_fraction, int *pij_stored,
                                  double *stored_slice_fraction)
{
  return guarded([&]() {
    if (!ctx)
      throw HipError(RYUJIN_ERR_ARG, "null context");
    if (limited_slice_fraction)
      *limited_slice_fraction = ctx->limited_fraction;
    if (pij_stored)
      *pij_stored = ctx->last_plan.pij_stored;
    if (stored_slice_fraction)
      *stored_slice_fraction = ctx->stored_fraction;
    return RYUJIN_OK;
  });
}

int ryujin_hip_tile_statistics(ryujin_hip_ctx *ctx, double *stored_fraction, double *read_fraction,
                               double *formed_by_step6_fraction)
{
  return guarded([&]() {
    if (!ctx)
      throw HipError(RYUJIN_ERR_ARG, "null context");
    const bool tiles = ctx->last_plan.per_tile();
    if (stored_fraction)
      *stored_fraction = tiles ? ctx->stored_fraction : 1.;
    if (read_fraction)
      *read_fraction = tiles ? ctx->tiles_needed_fraction : 1.;
    if (formed_by_step6_fraction)
      *formed_by_step6_fraction = tiles ? ctx->tiles_formed_fraction : 0.;
    return RYUJIN_OK;
  });
}

int ryujin_hip_layout_info(ryujin_hip_ctx *ctx, unsigned long long *n_tiles, unsigned long long *n_regular_tiles)
{
  return guarded([&]() {
    if (!ctx)
      throw HipError(RYUJIN_ERR_ARG, "null context");
    if (n_tiles)
      *n_tiles = ctx->L.slice_off[ctx->L.n_slices];
    if (n_regular_tiles)
      *n_regular_tiles = (ctx->d_tiles.n != 0 && tile_map_pays(ctx->dim)) ? ctx->L.n_regular_tiles : 0ull;
    return RYUJIN_OK;
  });
}

int ryujin_hip_chain_info(ryujin_hip_ctx *ctx, unsigned long long *n_chained_tiles,
                          unsigned long long *n_chained_entries)
{
  return guarded([&]() {
    if (!ctx)
      throw HipError(RYUJIN_ERR_ARG, "null context");
    /* (what the sweeps of this dimension use: every chained tile with its mask in 3-D, below that the tiles in which
     * only the lane at the end of the wave loads -- 63 entries each; chain_masks_pay(), kernels_euler.hpp) */
    const bool masks = ctx->dim == 3;
    if (n_chained_tiles)
      *n_chained_tiles = ctx->d_tiles.n == 0 ? 0ull : (masks ? ctx->L.n_chained_tiles : ctx->L.n_end_lane_tiles);
    if (n_chained_entries)
      *n_chained_entries = ctx->d_tiles.n == 0 ? 0ull : (masks ? ctx->L.n_chained_entries : 63ull * ctx->L.n_end_lane_tiles);
    return RYUJIN_OK;
  });
}

int ryujin_hip_stencil_class_info(ryujin_hip_ctx *ctx, unsigned long long *n_uniform_slices,
                                  unsigned long long *n_classes, double *uniform_entry_fraction)
{
  return guarded([&]() {
    if (!ctx)
      throw HipError(RYUJIN_ERR_ARG, "null context");
    const bool table = ctx->d_slice_class.n != 0;
    const uint64_t n_tiles = ctx->L.slice_off[ctx->L.n_slices];
    if (n_uniform_slices)
      *n_uniform_slices = table ? ctx->L.n_uniform_slices : 0ull;
    if (n_classes)
      *n_classes = table ? ctx->L.n_stencil_classes() : 0ull;
    if (uniform_entry_fraction)
      *uniform_entry_fraction = table && n_tiles != 0 ? (double)ctx->L.n_uniform_tiles / (double)n_tiles : 0.;
    return RYUJIN_OK;
  });
}

int ryujin_hip_next_tile_mask_info(ryujin_hip_ctx *ctx, int *active, unsigned long long *n_tiles,
                                   unsigned long long *n_named)
{
  return guarded_ctx(ctx, [&]() {
    const auto &L = ctx->L;
    const bool on = ctx->last_plan.next_tile_mask && ctx->d_slice_next_tiles.n == L.n_slices;
    std::vector<uint32_t> words(on ? L.n_slices : 0u);
    if (on) {
      ctx->finish();
      HIP_CHECK(hipMemcpy(words.data(), ctx->d_slice_next_tiles.ptr, words.size() * sizeof(uint32_t),
                          hipMemcpyDeviceToHost));
    }
    unsigned long long tiles = 0, named = 0;
    for (uint32_t s = 0; s < L.n_slices; ++s) {
      const uint32_t width = L.slice_off[s + 1] - L.slice_off[s];
      const uint32_t off_diagonal = width > 1 ? width - 1 : 0u;
      tiles += off_diagonal;
      named += on ? (unsigned long long)__builtin_popcount(words[s] & ~1u) : off_diagonal;
    }
    if (active)
      *active = on ? 1 : 0;
    if (n_tiles)
      *n_tiles = tiles;
    if (n_named)
      *n_named = named;
    return RYUJIN_OK;
  });
}

int ryujin_hip_debug_plan(ryujin_hip_ctx *ctx, int *out, int n)
{
  return guarded([&]() {
    if (!ctx || (n > 0 && !out) || n < 0)
      throw HipError(RYUJIN_ERR_ARG, "null context or output");
    const StepPlan &p = ctx->last_plan;
    const auto &log = ctx->last_launches;
    int v[RYUJIN_DEBUG_PLAN_LENGTH] = {(int)p.step2,
                                       p.step2_split,
                                       p.fast_riemann,
                                       p.diag_width,
                                       p.step4_single_walk,
                                       p.step4_has_stages,
                                       p.step4_friction,
                                       p.step4_stores_p,
                                       p.dg,
                                       (int)p.step5,
                                       (int)p.step5_groups,
                                       p.wide,
                                       p.has_V,
                                       p.pij_stored,
                                       p.tiles_predicted_from_history,
                                       (int)p.step6,
                                       p.step6_flags,
                                       (int)p.step7,
                                       p.fuse_precompute,
                                       p.checked,
                                       log.n_step5,
                                       log.n_step6};
    static_assert(22 + 5 * ryujin_hip_ctx::LaunchLog::kParts == RYUJIN_DEBUG_PLAN_LENGTH, "layout of the record");
    for (int q = 0; q < ryujin_hip_ctx::LaunchLog::kParts; ++q) {
      v[22 + 2 * q] = (int)log.step5[q].n_slices;
      v[23 + 2 * q] = (int)log.step5[q].grid_y;
      v[26 + 3 * q] = (int)log.step6[q].n_slices;
      v[27 + 3 * q] = (int)log.step6[q].grid_y;
      v[28 + 3 * q] = log.step6[q].shares_slices;
    }
    for (int q = 0; q < std::min(n, (int)RYUJIN_DEBUG_PLAN_LENGTH); ++q)
      out[q] = v[q];
    return (int)RYUJIN_DEBUG_PLAN_LENGTH;
  });
}

int ryujin_hip_debug_fetch(ryujin_hip_ctx *ctx, int what, double *out, size_t n_doubles)
{
  return guarded_ctx(ctx, [&]() {
    const auto &L = ctx->L;
    ctx->finish();
    /* the second-pass matrix of an update whose step 6 elided the zeros of the unlimited tiles: written now */
    auto materialise_zeros = [&](double *dev) {
      if (!ctx->last_plan.next_tiles_elided || ctx->last_plan.step6 == StepPlan::Step6::none)
        return;
      DeviceMesh mm = ctx->mesh;
      mm.slice_begin = 0;
      mm.slice_end = L.n_slices;
      hipLaunchKernelGGL(k_fill_unnamed_tiles, dim3((L.n_slices + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0,
                         ctx->stream, mm, (const uint32_t *)ctx->d_slice_next_tiles.ptr, dev);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
    };
    auto fetch_matrix = [&](const double *dev, uint32_t n_comp) {
      if (n_doubles < L.nnz_owned_logical * n_comp)
        throw HipError(RYUJIN_ERR_ARG, "output buffer too small");
      std::vector<double> tmp(L.nnz_total * n_comp);
      HIP_CHECK(hipMemcpy(tmp.data(), dev, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
      L.gather_logical(tmp, n_comp, out);
    };
    switch (what) {
    case 0: fetch_matrix(ctx->d_dij.ptr, 1); break;
    case 1:
      materialise_zeros(ctx->d_lij.ptr);
      fetch_matrix(ctx->d_lij.ptr, 1);
      break;
    case 2:
      ctx->ensure_pij();
      if (ctx->last_plan.pij_stored != 1)
        dispatch_equation(ctx->params.equation, ctx->dim, [&](auto tag) {
          using E = typename decltype(tag)::type;
          if constexpr (std::is_same<typename E::Params, EulerParams>::value ||
                        std::is_same<typename E::Params, EulerAeosParams>::value)
            ctx->template store_pij_for_debug<E>();
          return 0;
        });
      fetch_matrix(ctx->d_pij.ptr, (uint32_t)ctx->K);
      break;
    case 5: fetch_matrix(ctx->d_lij_next.ptr, 1); break;
    case 6:
    case 7:
    case 8: { /* plain CSR over ALL locally relevant rows: owned rows, then the ghost rows as received */
      if (what == 7)
        materialise_zeros(ctx->d_lij.ptr);
      const double *dev = what == 6 ? ctx->d_dij.ptr : (what == 7 ? ctx->d_lij.ptr : ctx->d_lij_next.ptr);
      const uint64_t n_ghost_entries = L.nnz_total - L.nnz_sell;
      if (n_doubles < L.nnz_owned_logical + n_ghost_entries)
        throw HipError(RYUJIN_ERR_ARG, "output buffer too small");
      std::vector<double> tmp(L.nnz_total);
      HIP_CHECK(hipMemcpy(tmp.data(), dev, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
      L.gather_logical(tmp, 1, out);
      std::copy(tmp.begin() + L.nnz_sell, tmp.end(), out + L.nnz_owned_logical);
      break;
    }
    case 9: {
      if (n_doubles < (size_t)L.n_relevant * ctx->K)
        throw HipError(RYUJIN_ERR_ARG, "output buffer too small");
      std::vector<double> tmp((size_t)L.n_relevant * ctx->KP);
      HIP_CHECK(hipMemcpy(tmp.data(), ctx->d_r.ptr, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < L.n_relevant; ++i)
        for (int q = 0; q < ctx->K; ++q)
          out[(size_t)i * ctx->K + q] = tmp[(size_t)i * ctx->KP + q];
      break;
    }
    case 3: {
      if (n_doubles < (size_t)L.n_owned * ctx->NB)
        throw HipError(RYUJIN_ERR_ARG, "output buffer too small");
      std::vector<double> tmp((size_t)ctx->NB * ctx->mesh.bounds_stride);
      HIP_CHECK(hipMemcpy(tmp.data(), ctx->d_bounds.ptr, tmp.size() * sizeof(double),
                          hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < L.n_owned; ++i)
        for (int b = 0; b < ctx->NB; ++b)
          out[(size_t)i * ctx->NB + b] = tmp[(size_t)b * ctx->mesh.bounds_stride + i];
      break;
    }
    case 4: {
      if (n_doubles < (size_t)L.n_owned * ctx->K)
        throw HipError(RYUJIN_ERR_ARG, "output buffer too small");
      std::vector<double> tmp((size_t)L.n_relevant * ctx->KP);
      HIP_CHECK(hipMemcpy(tmp.data(), ctx->d_r.ptr, tmp.size() * sizeof(double),
                          hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < L.n_owned; ++i)
        for (int q = 0; q < ctx->K; ++q)
          out[(size_t)i * ctx->K + q] = tmp[(size_t)i * ctx->KP + q];
      break;
    }
    default: throw HipError(RYUJIN_ERR_ARG, "unknown debug_fetch selector");
    }
    return RYUJIN_OK;
  });
}

int ryujin_hip_debug_fill(ryujin_hip_ctx *ctx, int what, double value)
{
  return guarded_ctx(ctx, [&]() {
    if (what != 5)
      throw HipError(RYUJIN_ERR_ARG, "unknown debug_fill selector");
    ctx->finish();
    const auto &L = ctx->L;
    std::vector<double> tmp(L.nnz_total);
    HIP_CHECK(hipMemcpy(tmp.data(), ctx->d_lij_next.ptr, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (uint32_t s = 0; s < L.n_slices; ++s) /* (column 0, the diagonal, is written by no sweep) */
      std::fill(tmp.begin() + ((size_t)L.slice_off[s] + 1) * 64, tmp.begin() + (size_t)L.slice_off[s + 1] * 64, value);
    HIP_CHECK(hipMemcpy(ctx->d_lij_next.ptr, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice));
    return RYUJIN_OK;
  });
}

int ryujin_hip_debug_addresses(ryujin_hip_ctx *ctx, uint64_t out[8])
{
  return guarded([&]() {
    if (!ctx || !out)
      throw HipError(RYUJIN_ERR_ARG, "null argument");
    ctx->ensure_pij();
    const void *p[8] = {ctx->d_cols.ptr, ctx->d_cij.ptr, ctx->d_mij.ptr, ctx->d_dij.ptr,
                        ctx->d_lij.ptr,  ctx->d_lij_next.ptr, ctx->d_pij.ptr, ctx->d_idx_t.ptr};
    for (int q = 0; q < 8; ++q)
      out[q] = (uint64_t)(uintptr_t)p[q];
    return RYUJIN_OK;
  });
}

int ryujin_hip_debug_layout(const ryujin_hip_offline *offline, uint64_t *ptr, uint32_t *col,
                            uint64_t *transposed, const double *data, uint32_t n_comp, double *out)
{
  return guarded([&]() {
    SellLayout L;
    L.build(*offline);
    const RefView ref(*offline);
    std::vector<uint64_t> lptr((size_t)L.n_relevant + 1, 0);
    for (uint32_t i = 0; i < L.n_relevant; ++i)
      lptr[i + 1] = lptr[i] + ref.row_length(i);
    /* device position -> logical index */
    std::vector<uint64_t> logical_of(L.nnz_total, ~uint64_t(0));
    for (uint32_t i = 0; i < L.n_relevant; ++i)
      for (uint32_t c = 0; c < ref.row_length(i); ++c)
        logical_of[L.pos(i, c)] = lptr[i] + c;
    std::vector<double> dev;
    if (data && out)
      dev = L.scatter(*offline, data, n_comp);
    for (uint32_t i = 0; i < L.n_relevant; ++i)
      for (uint32_t c = 0; c < ref.row_length(i); ++c) {
        const uint64_t p = L.pos(i, c), e = lptr[i] + c;
        if (col)
          col[e] = L.cols[p];
        if (transposed)
          transposed[e] = logical_of[L.idx_t[p]];
        if (data && out)
          for (uint32_t d = 0; d < n_comp; ++d)
            out[e * n_comp + d] = dev[L.comp_pos(p, n_comp, d)];
      }
    if (ptr)
      std::copy(lptr.begin(), lptr.end(), ptr);
    return RYUJIN_OK;
  });
}

int ryujin_hip_debug_pow(int device, const double *x, const double *y, double *out, size_t n)
{
  return guarded([&]() {
    HIP_CHECK(hipSetDevice(device));
    DeviceBuffer<double> dx, dy, dout;
    dx.upload(x, n);
    dy.upload(y, n);
    dout.alloc(n);
    hipLaunchKernelGGL(k_debug_pow, dim3(grid_for(n)), dim3(kBlock), 0, nullptr, n, dx.ptr, dy.ptr,
                       dout.ptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(out, dout.ptr, n * sizeof(double), hipMemcpyDeviceToHost));
    return RYUJIN_OK;
  });
}

/* device functions evaluated on n independent items (parity tests against the reference's unit-test
 * baselines: tests/euler/riemann_solver.cc, tests/euler/limiter.cc, tests/shallow_water/riemann_solver.cc) */
namespace
{
  __global__ void __launch_bounds__(kBlock)
  k_debug_function(const EulerParams PE, const ShallowWaterParams PS, const EulerAeosParams PA, const int which,
                   const size_t n, const double *__restrict__ in, double *__restrict__ out)
  {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n)
      return;
    if (which == RYUJIN_DEBUG_AEOS_RIEMANN) {
      /* through the PRODUCTION evaluation path: per-node records, dij_from_records with n = (1) */
      using A = EulerAeos<1>;
      const double *v = in + q * 10;
      const A::RiemannData rd_i = A::make_riemann_data(PA, v[0], v[1], v[2], v[3], v[4]),
                           rd_j = A::make_riemann_data(PA, v[5], v[6], v[7], v[8], v[9]);
      const double r_i[A::RS] = {rd_i.rho, rd_i.p, rd_i.gamma, rd_i.a, rd_i.alpha, rd_i.alpha_hat, rd_i.u, 0.},
                   r_j[A::RS] = {rd_j.rho, rd_j.p, rd_j.gamma, rd_j.a, rd_j.alpha, rd_j.alpha_hat, rd_j.u, 0.};
      const double n[1] = {1.};
      out[q] = A::dij_from_records(PA, r_i, r_j, n);
      return;
    }
    if (which == RYUJIN_DEBUG_AEOS_DIJ_2D || which == RYUJIN_DEBUG_AEOS_DIJ_RECORDS_2D) {
      using A = EulerAeos<2>;
      const double *v = in + q * 10;
      const double U_i[4] = {v[0], v[1], v[2], v[3]}, U_j[4] = {v[4], v[5], v[6], v[7]}, c[2] = {v[8], v[9]};
      const double p_i = A::precompute_cycle0(PA, U_i).p, p_j = A::precompute_cycle0(PA, U_j).p;
      if (which == RYUJIN_DEBUG_AEOS_DIJ_2D) {
        out[q] = A::dij_from_states(PA, U_i, p_i, U_j, p_j, c);
      } else {
        double r_i[A::RS], r_j[A::RS];
        A::riemann_record(PA, U_i, p_i, r_i);
        A::riemann_record(PA, U_j, p_j, r_j);
        out[q] = A::dij_from_records(PA, r_i, r_j, c);
      }
      return;
    }
    if (which == RYUJIN_DEBUG_AEOS_LIMIT_1D) {
      /* the composition the sweeps use: limit_fast(), and limit() for the undecided pairs */
      const double *v = in + q * 10;
      const double bnd[4] = {v[0], v[1], v[2], v[3]}, U[3] = {v[4], v[5], v[6]}, Pij[3] = {v[7], v[8], v[9]};
      bool success, undecided;
      double l = EulerAeos<1>::limit_fast(PA, bnd, U, Pij, success, undecided);
      if (undecided)
        l = EulerAeos<1>::limit(PA, bnd, U, Pij, success);
      out[q * 3 + 0] = l;
      out[q * 3 + 1] = success ? 1. : 0.;
      out[q * 3 + 2] = undecided ? 1. : 0.;
      return;
    }
    if (which == RYUJIN_DEBUG_EULER_RIEMANN) {
      const double *v = in + q * 8;
      const Euler<1>::RiemannData rd_i{v[0], v[1], v[2], v[3]}, rd_j{v[4], v[5], v[6], v[7]};
      out[q] = Euler<1>::riemann_compute(PE, rd_i, rd_j);
    } else if (which == RYUJIN_DEBUG_EULER_LIMIT_1D) {
      /* the composition the sweeps use: limit_fast(), and limit() for the undecided pairs */
      const double *v = in + q * 9;
      const double bnd[3] = {v[0], v[1], v[2]}, U[3] = {v[3], v[4], v[5]}, Pij[3] = {v[6], v[7], v[8]};
      bool success, undecided;
      double l = Euler<1>::limit_fast(PE, bnd, U, Pij, success, undecided);
      if (undecided)
        l = Euler<1>::limit(PE, bnd, U, Pij, success);
      out[q * 3 + 0] = l;
      out[q * 3 + 1] = success ? 1. : 0.;
      out[q * 3 + 2] = undecided ? 1. : 0.;
    } else if (which == RYUJIN_DEBUG_EULER_LIMIT_2D) {
      EulerParams P2 = PE; /* (the parameter block carries no dimension) */
      const double *v = in + q * 11;
      const double bnd[3] = {v[0], v[1], v[2]}, U[4] = {v[3], v[4], v[5], v[6]}, Pij[4] = {v[7], v[8], v[9], v[10]};
      bool success, undecided, s2;
      double l = Euler<2>::limit_fast(P2, bnd, U, Pij, success, undecided);
      if (undecided)
        l = Euler<2>::limit(P2, bnd, U, Pij, success);
      double t_r;
      const double psi_r = Euler<2>::first_psi_r(P2, bnd, U, Pij, s2, t_r);
      out[q * 5 + 0] = l;
      out[q * 5 + 1] = success ? 1. : 0.;
      out[q * 5 + 2] = undecided ? 1. : 0.;
      out[q * 5 + 3] = t_r;
      out[q * 5 + 4] = psi_r;
    } else if (which == RYUJIN_DEBUG_EULER_LIMIT_CHECKED_1D) {
      const double *v = in + q * 9;
      const double bnd[3] = {v[0], v[1], v[2]}, U[3] = {v[3], v[4], v[5]}, Pij[3] = {v[6], v[7], v[8]};
      bool success;
      out[q * 3 + 0] = Euler<1>::limit_checked(PE, bnd, U, Pij, success);
      out[q * 3 + 1] = success ? 1. : 0.;
      out[q * 3 + 2] = 0.;
    } else if (which == RYUJIN_DEBUG_SW_RIEMANN) {
      const double *v = in + q * 6;
      const ShallowWater<1>::RiemannData rd_i{v[0], v[1], v[2]}, rd_j{v[3], v[4], v[5]};
      out[q * 2 + 0] = ShallowWater<1>::compute_h_star(PS, rd_i, rd_j);
      out[q * 2 + 1] = ShallowWater<1>::lambda_max(PS, rd_i, rd_j);
    } else if (which == RYUJIN_DEBUG_EULER_DIJ_2D) {
      const double *v = in + q * 10;
      const double U_i[4] = {v[0], v[1], v[2], v[3]}, U_j[4] = {v[4], v[5], v[6], v[7]}, c[2] = {v[8], v[9]};
      out[q] = Euler<2>::dij_from_states(PE, U_i, U_j, c);
    } else if (which == RYUJIN_DEBUG_EULER_DIJ_3D) {
      const double *v = in + q * 13;
      const double U_i[5] = {v[0], v[1], v[2], v[3], v[4]}, U_j[5] = {v[5], v[6], v[7], v[8], v[9]},
                   c[3] = {v[10], v[11], v[12]};
      out[q] = Euler<3>::dij_from_states(PE, U_i, U_j, c);
    } else if (which == RYUJIN_DEBUG_EULER_DIJ_RECORDS_2D) {
      const double *v = in + q * 10;
      const double U_i[4] = {v[0], v[1], v[2], v[3]}, U_j[4] = {v[4], v[5], v[6], v[7]}, c[2] = {v[8], v[9]};
      double r_i[Euler<2>::RS], r_j[Euler<2>::RS];
      Euler<2>::riemann_record(PE, U_i, r_i);
      Euler<2>::riemann_record(PE, U_j, r_j);
      out[q] = PE.riemann_newton_max_iterations == 0 && PE.rarefaction_power > 0
                   ? Euler<2>::dij_from_records<false>(PE, r_i, r_j, c)
                   : Euler<2>::dij_from_records<true>(PE, r_i, r_j, c);
    } else if (which == RYUJIN_DEBUG_EULER_DIJ_RECORDS_3D) {
      const double *v = in + q * 13;
      const double U_i[5] = {v[0], v[1], v[2], v[3], v[4]}, U_j[5] = {v[5], v[6], v[7], v[8], v[9]},
                   c[3] = {v[10], v[11], v[12]};
      double r_i[Euler<3>::RS], r_j[Euler<3>::RS];
      Euler<3>::riemann_record(PE, U_i, r_i);
      Euler<3>::riemann_record(PE, U_j, r_j);
      out[q] = PE.riemann_newton_max_iterations == 0 && PE.rarefaction_power > 0
                   ? Euler<3>::dij_from_records<false>(PE, r_i, r_j, c)
                   : Euler<3>::dij_from_records<true>(PE, r_i, r_j, c);
    } else if (which == RYUJIN_DEBUG_EULER_RIEMANN_RECORDS) {
      /* the PRODUCTION evaluation path (per-node records, dij_from_records) on the reference's Riemann data */
      const double *v = in + q * 8;
      double r_i[Euler<1>::RS], r_j[Euler<1>::RS];
      const double u_i[1] = {v[1]}, u_j[1] = {v[5]}, n[1] = {1.};
      Euler<1>::riemann_record_from_primitive(PE, v[0], v[2], v[3], u_i, r_i);
      Euler<1>::riemann_record_from_primitive(PE, v[4], v[6], v[7], u_j, r_j);
      out[q] = PE.riemann_newton_max_iterations == 0 && PE.rarefaction_power > 0
                   ? Euler<1>::dij_from_records<false>(PE, r_i, r_j, n)
                   : Euler<1>::dij_from_records<true>(PE, r_i, r_j, n);
    } else if (which == RYUJIN_DEBUG_SW_RIEMANN_RECORDS) {
      const double *v = in + q * 6;
      const double r_i[ShallowWater<1>::RS] = {v[0], v[2], v[1], 0.}, r_j[ShallowWater<1>::RS] = {v[3], v[5], v[4], 0.};
      const double n[1] = {1.};
      out[q] = ShallowWater<1>::dij_from_records<false>(PS, r_i, r_j, n);
    } else if (which == RYUJIN_DEBUG_SW_DIJ_2D || which == RYUJIN_DEBUG_SW_DIJ_RECORDS_2D) {
      const double *v = in + q * 8;
      const double U_i[3] = {v[0], v[1], v[2]}, U_j[3] = {v[3], v[4], v[5]}, c[2] = {v[6], v[7]};
      if (which == RYUJIN_DEBUG_SW_DIJ_2D) {
        out[q] = ShallowWater<2>::dij_from_states(PS, U_i, U_j, c);
      } else {
        double r_i[ShallowWater<2>::RS], r_j[ShallowWater<2>::RS];
        ShallowWater<2>::riemann_record(PS, U_i, r_i);
        ShallowWater<2>::riemann_record(PS, U_j, r_j);
        out[q] = ShallowWater<2>::dij_from_records<false>(PS, r_i, r_j, c);
      }
    }
  }
} // namespace

/* The limiter of one Description on n independent items bounds[NB], U[K], P[K], as the sweeps compose it:
 * limit_fast(), and limit() for the undecided pairs -- or limit_checked() alone (debug_expensive_bounds_check).
 * out: l, success, undecided; WITH_TRACE (Euler, EulerAEOS): also t_r behind the density clip and psi_r there. */
extern "C++" {
namespace
{
  template <typename E, bool WITH_TRACE>
  __global__ void __launch_bounds__(kBlock)
  k_debug_limit(const typename E::Params P, const bool checked, const size_t n, const double *__restrict__ in,
                double *__restrict__ out)
  {
    constexpr int K = E::K, NB = E::NB, n_in = NB + 2 * K, n_out = WITH_TRACE ? 5 : 3;
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n)
      return;
    const double *v = in + q * n_in;
    double bnd[NB], U[K], Pij[K];
#pragma unroll
    for (int b = 0; b < NB; ++b)
      bnd[b] = v[b];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      U[k] = v[NB + k];
      Pij[k] = v[NB + K + k];
    }
    bool success, undecided = false;
    double l;
    if (checked) {
      l = E::limit_checked(P, bnd, U, Pij, success);
    } else {
      l = E::limit_fast(P, bnd, U, Pij, success, undecided);
      if (undecided)
        l = E::limit(P, bnd, U, Pij, success);
    }
    out[q * n_out + 0] = l;
    out[q * n_out + 1] = success ? 1. : 0.;
    out[q * n_out + 2] = undecided ? 1. : 0.;
    if constexpr (WITH_TRACE) {
      bool s2;
      double t_r, psi_r;
      if constexpr (std::is_same<typename E::Params, EulerParams>::value) {
        psi_r = E::first_psi_r(P, bnd, U, Pij, s2, t_r);
      } else {
        t_r = E::density_clip(P, bnd, U, Pij, s2);
        double U_r[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
          U_r[k] = U[k] + t_r * Pij[k];
        psi_r = E::psi_of(P, U_r, bnd[2], bnd[3], 1. + P.vacuum_small * DBL_EPSILON).psi;
      }
      out[q * n_out + 3] = t_r;
      out[q * n_out + 4] = psi_r;
    }
  }

  template <typename E, bool WITH_TRACE>
  void debug_limit(const typename E::Params &P, const bool checked, const double *in, double *out, const size_t n)
  {
    constexpr size_t n_in = E::NB + 2 * E::K, n_out = WITH_TRACE ? 5 : 3;
    DeviceBuffer<double> din, dout;
    din.upload(in, n * n_in);
    dout.alloc(n * n_out);
    hipLaunchKernelGGL((k_debug_limit<E, WITH_TRACE>), dim3(grid_for(n)), dim3(kBlock), 0, nullptr, P, checked, n,
                       din.ptr, dout.ptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(out, dout.ptr, n * n_out * sizeof(double), hipMemcpyDeviceToHost));
  }
} // namespace
} /* extern "C++": templates */

int ryujin_hip_debug_function(int device, const ryujin_hip_params *params, int which, const double *in,
                              double *out, size_t n)
{
  return guarded([&]() {
    if (!params || !in || !out)
      throw HipError(RYUJIN_ERR_ARG, "null argument");
    /* the limiters pair by pair: a kernel of their own (k_debug_limit) */
    if (which >= RYUJIN_DEBUG_EULER_LIMIT_3D && which <= RYUJIN_DEBUG_SCALAR_LIMIT) {
      HIP_CHECK(hipSetDevice(device));
      const bool checked = params->debug_expensive_bounds_check != 0;
      switch (which) {
      case RYUJIN_DEBUG_EULER_LIMIT_3D:
        debug_limit<Euler<3>, true>(make_euler_params(*params), checked, in, out, n);
        break;
      case RYUJIN_DEBUG_AEOS_LIMIT_2D:
        debug_limit<EulerAeos<2>, true>(make_aeos_params(*params), checked, in, out, n);
        break;
      case RYUJIN_DEBUG_AEOS_LIMIT_3D:
        debug_limit<EulerAeos<3>, true>(make_aeos_params(*params), checked, in, out, n);
        break;
      case RYUJIN_DEBUG_SW_LIMIT_1D:
        debug_limit<ShallowWater<1>, false>(make_sw_params(*params), checked, in, out, n);
        break;
      case RYUJIN_DEBUG_SW_LIMIT_2D:
        debug_limit<ShallowWater<2>, false>(make_sw_params(*params), checked, in, out, n);
        break;
      default: /* the scalar limiter reads no parameter (scalar_conservation/limiter.template.h) */
        debug_limit<ScalarConservation<1>, false>(ScalarParams{}, checked, in, out, n);
        break;
      }
      return RYUJIN_OK;
    }
    size_t n_in, n_out;
    switch (which) {
    case RYUJIN_DEBUG_EULER_RIEMANN:
    case RYUJIN_DEBUG_EULER_RIEMANN_RECORDS: n_in = 8; n_out = 1; break;
    case RYUJIN_DEBUG_SW_RIEMANN_RECORDS: n_in = 6; n_out = 1; break;
    case RYUJIN_DEBUG_AEOS_RIEMANN:
    case RYUJIN_DEBUG_AEOS_DIJ_2D:
    case RYUJIN_DEBUG_AEOS_DIJ_RECORDS_2D: n_in = 10; n_out = 1; break;
    case RYUJIN_DEBUG_AEOS_LIMIT_1D: n_in = 10; n_out = 3; break;
    case RYUJIN_DEBUG_EULER_LIMIT_1D:
    case RYUJIN_DEBUG_EULER_LIMIT_CHECKED_1D: n_in = 9; n_out = 3; break;
    case RYUJIN_DEBUG_EULER_LIMIT_2D: n_in = 11; n_out = 5; break;
    case RYUJIN_DEBUG_SW_RIEMANN: n_in = 6; n_out = 2; break;
    case RYUJIN_DEBUG_EULER_DIJ_2D:
    case RYUJIN_DEBUG_EULER_DIJ_RECORDS_2D: n_in = 10; n_out = 1; break;
    case RYUJIN_DEBUG_EULER_DIJ_3D:
    case RYUJIN_DEBUG_EULER_DIJ_RECORDS_3D: n_in = 13; n_out = 1; break;
    case RYUJIN_DEBUG_SW_DIJ_2D:
    case RYUJIN_DEBUG_SW_DIJ_RECORDS_2D: n_in = 8; n_out = 1; break;
    default: throw HipError(RYUJIN_ERR_ARG, "unknown debug function");
    }
    /* these two form p from the closed-form equation of state inside the kernel; the programs of the function one
     * belong to a context */
    if ((which == RYUJIN_DEBUG_AEOS_DIJ_2D || which == RYUJIN_DEBUG_AEOS_DIJ_RECORDS_2D) &&
        params->eos == RYUJIN_EOS_FUNCTION)
      throw HipError(RYUJIN_ERR_UNSUPPORTED, "debug function: not offered with the function equation of state");
    HIP_CHECK(hipSetDevice(device));
    DeviceBuffer<double> din, dout;
    din.upload(in, n * n_in);
    dout.alloc(n * n_out);
    hipLaunchKernelGGL(k_debug_function, dim3(grid_for(n)), dim3(kBlock), 0, nullptr,
                       make_euler_params(*params), make_sw_params(*params), make_aeos_params(*params), which, n,
                       din.ptr, dout.ptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy(out, dout.ptr, n * n_out * sizeof(double), hipMemcpyDeviceToHost));
    return RYUJIN_OK;
  });
}

/* The decision at the end of a device-resident RK step from the two accumulated flags
 * (0 = never raised, otherwise kStageCode - index of the first stage that raised it; see time_step) */
int ryujin_hip_debug_rk_outcome(int restart_accum, int tau_invalid_accum, int id_violation_strategy)
{
  const int t = tau_invalid_accum, r = restart_accum;
  const bool restart_wins = id_violation_strategy == RYUJIN_IDV_RAISE_EXCEPTION && r > t;
  if (t > 0 && !restart_wins)
    return RYUJIN_ERR_TAU;
  if (r > 0)
    return id_violation_strategy == RYUJIN_IDV_RAISE_EXCEPTION ? RYUJIN_RESTART : RYUJIN_WARN;
  return RYUJIN_OK;
}

int ryujin_hip_set_timers(ryujin_hip_ctx *ctx, int enable)
{
  ctx->timers_enabled = enable != 0;
  return RYUJIN_OK;
}

int ryujin_hip_get_timers(ryujin_hip_ctx *ctx, double ms[8])
{
  for (int k = 0; k < 8; ++k)
    ms[k] = ctx->sweep_ms[k];
  return RYUJIN_OK;
}

int ryujin_hip_synchronize(ryujin_hip_ctx *ctx)
{
  return guarded_ctx(ctx, [&]() {
    ctx->finish();
    return RYUJIN_OK;
  });
}

int ryujin_hip_event_record(ryujin_hip_ctx *ctx, int which)
{
  return guarded_ctx(ctx, [&]() {
    if (which < 0 || which > 1)
      throw HipError(RYUJIN_ERR_ARG, "which must be 0 or 1");
    HIP_CHECK(hipEventRecord(ctx->ev_user[which], ctx->stream));
    return RYUJIN_OK;
  });
}

int ryujin_hip_event_elapsed_ms(ryujin_hip_ctx *ctx, double *ms)
{
  return guarded_ctx(ctx, [&]() {
    HIP_CHECK(hipEventSynchronize(ctx->ev_user[1]));
    float f = 0.f;
    HIP_CHECK(hipEventElapsedTime(&f, ctx->ev_user[0], ctx->ev_user[1]));
    *ms = f;
    return RYUJIN_OK;
  });
}

int ryujin_hip_postprocess_configure(ryujin_hip_ctx *ctx, int n_quantities,
                                     const ryujin_hip_postprocess_quantity *quantities, double beta,
                                     int recompute_bounds)
{
  return guarded_ctx(ctx, [&]() {
    if (n_quantities < 1 || n_quantities > RYUJIN_PP_MAX_QUANTITIES || !quantities)
      throw HipError(RYUJIN_ERR_ARG, "postprocess_configure: n_quantities must be in [1, " +
                                         std::to_string(RYUJIN_PP_MAX_QUANTITIES) + "]");
    if (std::isnan(beta))
      throw HipError(RYUJIN_ERR_ARG, "postprocess_configure: beta is NaN");
    static_assert(RYUJIN_PP_MAX_QUANTITIES == kPostprocessMaxQuantities, "header and kernels agree");
    static_assert(RYUJIN_PP_SCHLIEREN == kPostprocessSchlieren && RYUJIN_PP_VORTICITY == kPostprocessVorticity,
                  "header and kernels agree");
    PostprocessDesc d{};
    d.n = n_quantities;
    for (int q = 0; q < n_quantities; ++q) {
      const auto &in = quantities[q];
      if (in.kind != RYUJIN_PP_SCHLIEREN && in.kind != RYUJIN_PP_VORTICITY)
        throw HipError(RYUJIN_ERR_ARG, "postprocess_configure: unknown kind " + std::to_string(in.kind));
      if (in.component < 0 || in.component >= ctx->K)
        throw HipError(RYUJIN_ERR_ARG, "postprocess_configure: component " + std::to_string(in.component) +
                                           " out of range [0, " + std::to_string(ctx->K) + ")");
      if (in.kind == RYUJIN_PP_VORTICITY) {
        if (ctx->dim == 1)
          throw HipError(RYUJIN_ERR_ARG, "postprocess_configure: vorticity is not defined in 1-D");
        if (in.component + ctx->dim > ctx->K)
          throw HipError(RYUJIN_ERR_ARG, "postprocess_configure: the dim components of a vorticity starting at " +
                                             std::to_string(in.component) + " do not fit the state");
      }
      d.kind[q] = in.kind;
      d.select[q] = (in.is_primitive ? ctx->K : 0) + in.component;
      d.any_primitive = d.any_primitive || in.is_primitive;
      const int n_components = in.kind == RYUJIN_PP_VORTICITY ? ctx->dim : 1;
      for (int c = in.component; c < in.component + n_components; ++c)
        d.load_mask |= 1 << (c / 2);
    }
    if (d.any_primitive) /* a primitive state needs all of U_j */
      d.load_mask = (1 << (ctx->KP / 2)) - 1;
    ctx->pp_desc = d;
    ctx->pp_beta = beta;
    ctx->pp_recompute_bounds = recompute_bounds != 0;
    ctx->pp_configured = true;
    ctx->pp_have_bounds = false;
    ctx->pp_computed = false;
    return RYUJIN_OK;
  });
}

int ryujin_hip_postprocess_compute(ryujin_hip_ctx *ctx, int handle)
{
  return guarded_ctx(ctx, [&]() {
    if (!ctx->pp_configured)
      throw HipError(RYUJIN_ERR_ARG, "postprocess_compute before postprocess_configure");
    dispatch_equation(ctx->params.equation, ctx->dim, [&](auto tag) {
      ctx->template postprocess_compute<typename decltype(tag)::type>(handle);
      return 0;
    });
    return RYUJIN_OK;
  });
}

int ryujin_hip_postprocess_download(ryujin_hip_ctx *ctx, int q, double *out, int raw)
{
  return guarded_ctx(ctx, [&]() {
    if (!ctx->pp_computed)
      throw HipError(RYUJIN_ERR_ARG, "postprocess_download before postprocess_compute");
    if (q < 0 || q >= ctx->pp_desc.n || !out)
      throw HipError(RYUJIN_ERR_ARG, "postprocess_download: quantity " + std::to_string(q) + " out of range");
    ctx->finish();
    const size_t n = ctx->L.n_owned;
    const double *src = (raw ? ctx->d_pp_raw.ptr : ctx->d_pp_normalised.ptr) + (size_t)q * n;
    HIP_CHECK(hipMemcpy(out, src, n * sizeof(double), hipMemcpyDeviceToHost));
    return RYUJIN_OK;
  });
}

int ryujin_hip_postprocess_bounds(ryujin_hip_ctx *ctx, int q, double *q_max, double *q_min)
{
  return guarded_ctx(ctx, [&]() {
    if (!ctx->pp_computed)
      throw HipError(RYUJIN_ERR_ARG, "postprocess_bounds before postprocess_compute");
    if (q < 0 || q >= ctx->pp_desc.n || !q_max || !q_min)
      throw HipError(RYUJIN_ERR_ARG, "postprocess_bounds: quantity " + std::to_string(q) + " out of range");
    ctx->finish();
    const double *b = reinterpret_cast<const double *>(ctx->d_pp_bounds.ptr);
    HIP_CHECK(hipMemcpy(q_max, b + q, sizeof(double), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(q_min, b + kPostprocessMaxQuantities + q, sizeof(double), hipMemcpyDeviceToHost));
    return RYUJIN_OK;
  });
}

/* ---- Quantities ---------------------------------------------------------- */

int ryujin_hip_quantities_add_manifold(ryujin_hip_ctx *ctx, uint32_t n_points, const uint32_t *index,
                                       const double *weight, int options, int *manifold_out)
{
  return guarded_ctx(ctx, [&]() {
    constexpr int known = RYUJIN_Q_INSTANTANEOUS | RYUJIN_Q_TIME_AVERAGED | RYUJIN_Q_SPACE_AVERAGED;
    if (!manifold_out)
      throw HipError(RYUJIN_ERR_ARG, "quantities_add_manifold: null argument");
    if (options == 0 || (options & ~known) != 0)
      throw HipError(RYUJIN_ERR_ARG, "quantities_add_manifold: options " + std::to_string(options) +
                                         " are not a combination of RYUJIN_Q_INSTANTANEOUS, _TIME_AVERAGED, "
                                         "_SPACE_AVERAGED");
    if (ctx->manifolds.size() >= RYUJIN_Q_MAX_MANIFOLDS)
      throw HipError(RYUJIN_ERR_ARG, "quantities_add_manifold: more than RYUJIN_Q_MAX_MANIFOLDS = " +
                                         std::to_string(RYUJIN_Q_MAX_MANIFOLDS) + " manifolds");
    if (n_points > 0 && (!index || !weight))
      throw HipError(RYUJIN_ERR_ARG, "quantities_add_manifold: null index or weight with n_points > 0");
    bool contiguous = n_points > 0;
    for (uint32_t p = 0; p < n_points; ++p) {
      if (index[p] >= ctx->L.n_owned)
        throw HipError(RYUJIN_ERR_ARG, "quantities_add_manifold: index " + std::to_string(index[p]) + " of point " +
                                           std::to_string(p) + " is not an owned row (n_owned = " +
                                           std::to_string(ctx->L.n_owned) + ")");
      if (!std::isfinite(weight[p]) || !(weight[p] > 0.))
        throw HipError(RYUJIN_ERR_ARG, "quantities_add_manifold: weight of point " + std::to_string(p) +
                                           " is not a positive finite number");
      contiguous = contiguous && index[p] == index[0] + p;
    }
    auto m = std::make_unique<ryujin_hip_ctx::Manifold>();
    m->n_points = n_points;
    m->options = options;
    m->contiguous = contiguous;
    m->first = contiguous ? index[0] : 0u;
    const size_t width = 2 * (size_t)ctx->K;
    m->n_blocks = (uint32_t)std::min<size_t>(kQuantitiesMaxBlocks, ((size_t)n_points + kBlock - 1) / kBlock);
    if (n_points > 0) {
      if (!contiguous)
        m->d_index.upload(index, n_points);
      m->d_weight.upload(weight, n_points);
      /* the values are kept where something reads them later: the trapezoid rule and "instantaneous" */
      if (options & (RYUJIN_Q_TIME_AVERAGED | RYUJIN_Q_INSTANTANEOUS))
        m->d_values.alloc(n_points * width);
      if (options & RYUJIN_Q_TIME_AVERAGED)
        m->d_sum.alloc(n_points * width);
    }
    m->d_partial.alloc(((size_t)m->n_blocks + 1) * (1 + width));
    *manifold_out = (int)ctx->manifolds.size();
    ctx->manifolds.push_back(std::move(m));
    return RYUJIN_OK;
  });
}

int ryujin_hip_quantities_reset(ryujin_hip_ctx *ctx)
{
  return guarded_ctx(ctx, [&]() {
    ctx->finish(); /* the buffers may be in use */
    ctx->manifolds.clear();
    return RYUJIN_OK;
  });
}

int ryujin_hip_quantities_clear_statistics(ryujin_hip_ctx *ctx)
{
  return guarded_ctx(ctx, [&]() {
    for (auto &m : ctx->manifolds) {
      m->t_old = m->t_new = m->t_sum = 0.;
      m->have_values = false;
      m->n_rows = 0;
      if (m->d_sum.n)
        HIP_CHECK(hipMemsetAsync(m->d_sum.ptr, 0, m->d_sum.n * sizeof(double), ctx->stream));
    }
    return RYUJIN_OK;
  });
}

int ryujin_hip_quantities_accumulate(ryujin_hip_ctx *ctx, int state_handle, double t)
{
  return guarded_ctx(ctx, [&]() {
    (void)ctx->state(state_handle);
    /* RCCL orders the operations of a communicator in issue order whatever stream they are on (allreduce_scalar) */
    ctx->wait_comm();
    for (auto &m : ctx->manifolds) {
      if (!(m->options & (RYUJIN_Q_TIME_AVERAGED | RYUJIN_Q_SPACE_AVERAGED)))
        continue; /* (:511-514) */
      dispatch_equation(ctx->params.equation, ctx->dim, [&](auto tag) {
        ctx->template quantities_evaluate<typename decltype(tag)::type>(*m, state_handle, true, t);
        return 0;
      });
    }
    return RYUJIN_OK;
  });
}

int ryujin_hip_quantities_instantaneous(ryujin_hip_ctx *ctx, int manifold, int state_handle, double t, double *out)
{
  return guarded_ctx(ctx, [&]() {
    auto &m = ctx->manifold(manifold);
    if (!(m.options & RYUJIN_Q_INSTANTANEOUS))
      throw HipError(RYUJIN_ERR_ARG, "quantities_instantaneous: manifold " + std::to_string(manifold) +
                                         " was added without RYUJIN_Q_INSTANTANEOUS");
    if (m.n_points > 0 && !out)
      throw HipError(RYUJIN_ERR_ARG, "quantities_instantaneous: null argument");
    if (m.options & (RYUJIN_Q_TIME_AVERAGED | RYUJIN_Q_SPACE_AVERAGED)) {
      /* AssertThrow(t_new == t) (:619) */
      if (!m.have_values || m.t_new != t)
        throw HipError(RYUJIN_ERR_ARG, "quantities_instantaneous: the latest accumulate of manifold " +
                                           std::to_string(manifold) + " is not one at t = " + std::to_string(t));
    } else {
      (void)ctx->state(state_handle);
      ctx->wait_comm();
      dispatch_equation(ctx->params.equation, ctx->dim, [&](auto tag) {
        ctx->template quantities_evaluate<typename decltype(tag)::type>(m, state_handle, false, t);
        return 0;
      });
    }
    if (m.n_points > 0) {
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
      HIP_CHECK(hipMemcpy(out, m.d_values.ptr, m.d_values.n * sizeof(double), hipMemcpyDeviceToHost));
    }
    return RYUJIN_OK;
  });
}

int ryujin_hip_quantities_time_averaged(ryujin_hip_ctx *ctx, int manifold, double *out, double *t_begin,
                                        double *t_end)
{
  return guarded_ctx(ctx, [&]() {
    auto &m = ctx->manifold(manifold);
    if (!(m.options & RYUJIN_Q_TIME_AVERAGED))
      throw HipError(RYUJIN_ERR_ARG, "quantities_time_averaged: manifold " + std::to_string(manifold) +
                                         " was added without RYUJIN_Q_TIME_AVERAGED");
    if ((m.n_points > 0 && !out) || !t_begin || !t_end)
      throw HipError(RYUJIN_ERR_ARG, "quantities_time_averaged: null argument");
    if (m.t_sum == 0.)
      return (int)RYUJIN_Q_NONE_YET; /* (:636) */
    *t_begin = m.t_new - m.t_sum;
    *t_end = m.t_new;
    if (m.n_points > 0) {
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
      HIP_CHECK(hipMemcpy(out, m.d_sum.ptr, m.d_sum.n * sizeof(double), hipMemcpyDeviceToHost));
      const double scale = 1. / m.t_sum; /* (:643): the reference multiplies by the reciprocal */
      for (size_t e = 0; e < m.d_sum.n; ++e)
        out[e] = scale * out[e];
    }
    return (int)RYUJIN_OK;
  });
}

int ryujin_hip_quantities_time_series(ryujin_hip_ctx *ctx, int manifold, double *rows, size_t capacity_rows,
                                      size_t *n_rows, int clear)
{
  return guarded_ctx(ctx, [&]() {
    auto &m = ctx->manifold(manifold);
    if (!n_rows)
      throw HipError(RYUJIN_ERR_ARG, "quantities_time_series: null argument");
    *n_rows = m.n_rows;
    if (!rows && capacity_rows == 0)
      return RYUJIN_OK; /* a query for the number of rows */
    if (capacity_rows < m.n_rows || (m.n_rows > 0 && !rows))
      throw HipError(RYUJIN_ERR_ARG, "quantities_time_series: " + std::to_string(m.n_rows) +
                                         " rows do not fit a capacity of " + std::to_string(capacity_rows));
    const size_t width = 1 + 2 * (size_t)ctx->K;
    if (m.n_rows > 0)
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (size_t r = 0, c = 0; r < m.n_rows; r += ryujin_hip_ctx::kSeriesChunkRows, ++c) {
      const size_t n = std::min(ryujin_hip_ctx::kSeriesChunkRows, m.n_rows - r);
      HIP_CHECK(hipMemcpy(rows + r * width, m.series[c]->ptr, n * width * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (clear)
      m.n_rows = 0; /* series.clear() (:665) */
    return RYUJIN_OK;
  });
}

} /* extern "C" */

/* ---- InitialValues: analytic initial and Dirichlet states, device resident -------------------------------- */

namespace
{
  /* the Descriptions that have analytic states here: everything but scalar conservation, which has the function
   * state (ryujin_hip_initial_values_configure_function) and nothing else */
  template <typename F>
  auto dispatch_initial_values(ryujin_hip_ctx *ctx, F &&f)
  {
    if (ctx->params.equation == RYUJIN_EQ_SCALAR_CONSERVATION && ctx->iv.state != kIvFunction)
      throw HipError(RYUJIN_ERR_UNSUPPORTED,
                     "initial values: scalar conservation has the function state only "
                     "(ryujin_hip_initial_values_configure_function)");
    return dispatch_equation(ctx->params.equation, ctx->dim, [&](auto tag) { return f(tag); });
  }

  /* n points of the caller through a points kernel that writes `width` doubles per point: upload into d_iv_points,
   * launch() from there into d_iv_values, download, synchronise. On the compute stream, in order with whatever it
   * holds; may be called from a Dirichlet callback inside a Runge-Kutta step (nothing of the exchange bookkeeping is
   * touched). */
  template <typename Launch>
  void initial_values_round_trip(ryujin_hip_ctx *ctx, const double *points, const size_t n, const size_t width,
                                 double *out, Launch &&launch)
  {
    const size_t dim = (size_t)ctx->dim;
    if (ctx->d_iv_points.n < n * dim)
      ctx->d_iv_points.alloc(n * dim, false);
    if (ctx->d_iv_values.n < n * width)
      ctx->d_iv_values.alloc(n * width, false);
    HIP_CHECK(hipMemcpyAsync(ctx->d_iv_points.ptr, points, n * dim * sizeof(double), hipMemcpyHostToDevice,
                             ctx->stream));
    launch();
    HIP_CHECK(hipMemcpyAsync(out, ctx->d_iv_values.ptr, n * width * sizeof(double), hipMemcpyDeviceToHost,
                             ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }

  /* InitialValues::parse_parameters_callback (initial_values.template.h:154-196): `position`, and the rolls of
   * affine_transform (:78-106) that take the normalised `direction` onto the x-axis */
  void set_initial_values_frame(InitialValuesParams &P, const int dim, const double *direction,
                                const double *position)
  {
    for (int d = 0; d < dim; ++d)
      P.position[d] = position[d];
    double n[3] = {0., 0., 0.}, norm2 = 0.;
    for (int d = 0; d < dim; ++d)
      norm2 += direction[d] * direction[d];
    const double norm = std::sqrt(norm2);
    if (!(norm > 0.) || std::isinf(norm))
      throw HipError(RYUJIN_ERR_ARG, "initial values: direction is the zero vector (or not finite)");
    for (int d = 0; d < dim; ++d)
      n[d] = direction[d] / norm;
    if (dim == 3) {
      const double r = std::sqrt(n[0] * n[0] + n[2] * n[2]);
      P.roll_z = r > 1.0e-14;
      P.nz_x = n[0] / r;
      P.nz_z = n[2] / r;
    }
    if (dim >= 2) {
      const double r = std::sqrt(n[0] * n[0] + n[1] * n[1]);
      P.roll_y = r > 1.0e-14;
      P.ny_x = n[0] / r;
      P.ny_y = n[1] / r;
    }
  }

  /* the node positions and the boundary positions in the library's grouped order; a second configure replaces the
   * first: nothing enqueued may still read the old positions or programs */
  void upload_initial_values_positions(ryujin_hip_ctx *ctx, const double *positions, const double *b_positions)
  {
    const size_t dim = (size_t)ctx->dim;
    ctx->d_iv_positions.upload(positions, (size_t)ctx->L.n_relevant * dim);
    std::vector<double> grouped((size_t)ctx->bdry.n_bdry * dim);
    ctx->bdry.permute(b_positions, ctx->dim, grouped.data());
    ctx->d_iv_b_positions.upload(grouped);
  }

  /* InitialValues::parse_parameters_callback (initial_values.template.h:154-196) and the constructors of the
   * InitialState classes: everything that does not depend on (x, t) */
  InitialValuesParams make_initial_values_params(const ryujin_hip_ctx &ctx, const ryujin_hip_initial_values &in)
  {
    const int dim = ctx.dim, eq = ctx.params.equation;
    InitialValuesParams P{};
    const bool library_state = iv_is_library_state(in.state), bathymetry_state = iv_is_bathymetry_state(in.state);
    if ((in.state < RYUJIN_IV_UNIFORM || in.state > RYUJIN_IV_SLOPING_FRICTION) && !library_state && !bathymetry_state)
      throw HipError(RYUJIN_ERR_ARG, "initial values: unknown state " + std::to_string(in.state));
    const bool sw_state = bathymetry_state || (library_state ? in.state >= RYUJIN_IV_SW_UNIFORM
                                                             : in.state >= RYUJIN_IV_CIRCULAR_DAM_BREAK);
    if (sw_state != (eq == RYUJIN_EQ_SHALLOW_WATER))
      throw HipError(RYUJIN_ERR_ARG, "initial values: the Description of this context has no such state");
    if (in.perturbation != 0.)
      throw HipError(RYUJIN_ERR_UNSUPPORTED,
                     "initial values: perturbation != 0 draws from an unseeded generator in the reference");
    if ((in.state == RYUJIN_IV_ISENTROPIC_VORTEX || in.state == RYUJIN_IV_SMOOTH_VORTEX) && dim != 2)
      throw HipError(RYUJIN_ERR_UNSUPPORTED, "initial values: the vortex states are defined for dim = 2");
    if (in.state == RYUJIN_IV_PARABOLOID && dim != 1)
      throw HipError(RYUJIN_ERR_UNSUPPORTED, "initial values: paraboloid is offered for dim = 1");
    if ((in.state == RYUJIN_IV_FOUR_STATE_CONTRAST || in.state == RYUJIN_IV_ASTRO_JET) && dim == 1)
      throw HipError(RYUJIN_ERR_UNSUPPORTED,
                     "initial values: four state contrast and astro jet are defined for dim >= 2");
    if (sw_state && (library_state || bathymetry_state) && dim == 3)
      throw HipError(RYUJIN_ERR_UNSUPPORTED, "initial values: shallow water is defined for dim = 1 and 2");
    if ((in.state == RYUJIN_IV_SW_HOU_TEST || in.state == RYUJIN_IV_SW_TRANSIENT) && dim != 2)
      throw HipError(RYUJIN_ERR_UNSUPPORTED,
                     "initial values: hou test and transient experiments are defined for dim = 2");
    /* the selector slots: a string of the reference each, one of its integer values here */
    const auto require_selector = [&](const int slot, const int n_values, const char *what) {
      const double value = in.params[slot];
      if (!(value >= 0. && value < (double)n_values && value == std::floor(value)))
        throw HipError(RYUJIN_ERR_ARG, std::string("initial values: ") + what + " is none of 0, ..., " +
                                           std::to_string(n_values - 1));
    };
    if (in.state == RYUJIN_IV_SW_FLOW_OVER_BUMP)
      require_selector(0, 2, "flow type");
    if (in.state == RYUJIN_IV_SW_THREE_BUMPS_DAM_BREAK)
      require_selector(0, 2, "well balancing validation");
    if (in.state == RYUJIN_IV_SW_TRANSIENT)
      require_selector(4, 4, "experimental configuration");
    for (int q = 0; q < 16; ++q)
      if (std::isnan(in.params[q]))
        throw HipError(RYUJIN_ERR_ARG, "initial values: NaN parameter");

    P.state = in.state;
    for (int q = 0; q < 16; ++q)
      P.p[q] = in.params[q];
    set_initial_values_frame(P, dim, in.direction, in.position);

    const ryujin_hip_params &hp = ctx.params;
    if (eq == RYUJIN_EQ_EULER_AEOS) {
      P.eos = ctx.aeosparams.eos; /* RYUJIN_EOS_FUNCTION after ryujin_hip_eos_configure_function: the kernels of the
                                   * sie program run, no closed-form switch is reached with it */
      P.eos_gamma = hp.gamma;
      P.eos_b = hp.eos_covolume_b;
      P.eos_q = hp.eos_q;
      P.eos_pinf = hp.eos_pinf;
      P.eos_a = hp.eos_vdw_a;
      P.jwl_A = hp.jwl_A;
      P.jwl_B = hp.jwl_B;
      P.jwl_R1 = hp.jwl_R1;
      P.jwl_R2 = hp.jwl_R2;
      P.jwl_omega = hp.jwl_omega;
      P.jwl_rho_0 = hp.jwl_rho_0;
    }
    /* gamma of the state itself: the system's for Euler; for EulerAEOS the states that need one take it as their
     * own parameter "gamma" (`if constexpr (!View::have_gamma)` in the reference) */
    double *c = P.c;
    switch (in.state) {
    case RYUJIN_IV_UNIFORM:
    case RYUJIN_IV_RADIAL_CONTRAST:
    case RYUJIN_IV_LEBLANC:
      c[0] = hp.gamma;
      break;
    case RYUJIN_IV_ISENTROPIC_VORTEX: {
      const double gamma = eq == RYUJIN_EQ_EULER ? hp.gamma : in.params[2];
      if (!(gamma > 1.))
        throw HipError(RYUJIN_ERR_ARG, "initial values: isentropic vortex needs gamma > 1");
      c[0] = gamma;
      c[1] = in.params[1] / (2.0 * M_PI);
      c[2] = (gamma - 1.0) / (2.0 * gamma);
      c[3] = 1.0 / (gamma - 1.0);
      break;
    }
    case RYUJIN_IV_RAREFACTION: {
      const double gamma = eq == RYUJIN_EQ_EULER ? hp.gamma : in.params[0];
      if (!(gamma > 1.))
        throw HipError(RYUJIN_ERR_ARG, "initial values: rarefaction needs gamma > 1");
      const double rho_l = 3.0, p_l = 1.0;
      const double c_l = std::sqrt(gamma * p_l / rho_l);
      const double u_l = c_l;
      const double rho_r = 0.5;
      const double p_r = std::pow(rho_r / rho_l, gamma) * p_l;
      const double c_r = std::sqrt(gamma * p_r / rho_r);
      const double u_r = u_l + 2.0 * (c_l - c_r) / (gamma - 1.0);
      c[0] = gamma;
      c[1] = rho_l;
      c[2] = u_l;
      c[3] = p_l;
      c[4] = c_l;
      c[5] = rho_r;
      c[6] = u_r;
      c[7] = p_r;
      c[8] = c_r;
      c[9] = 2.0 / (gamma + 1.0);
      c[10] = (gamma - 1.0) / ((gamma + 1.0) * c_l);
      c[11] = c_l + ((gamma - 1.0) / 2.0) * u_l;
      c[12] = 2.0 / (gamma - 1.0);
      c[13] = 2.0 * gamma / (gamma - 1.0);
      c[14] = 0.2 / (u_r - u_l);
      break;
    }
    case RYUJIN_IV_CIRCULAR_DAM_BREAK:
      break;
    case RYUJIN_IV_PARABOLOID: {
      const double a = in.params[0], h0 = in.params[1], B = in.params[3];
      const double g = hp.gravity, k = hp.manning_friction_coefficient;
      const double p = std::sqrt(8.0 * g * h0) / a;
      const double s = std::sqrt(p * p - k * k) / 2.0;
      c[0] = g;
      c[1] = k;
      c[2] = h0 / (a * a);
      c[3] = s;
      c[4] = (a * a * B * B) / (8.0 * g * g * h0);
      c[5] = 1.0 / 4.0 * k * k - s * s;
      c[6] = s * k;
      c[7] = -(B * B / (4.0 * g));
      c[8] = -(B / g);
      break;
    }
    case RYUJIN_IV_RITTER_DAM_BREAK:
      c[0] = hp.gravity;
      c[1] = std::sqrt(hp.gravity * in.params[1]);
      c[2] = 4.0 / (9.0 * hp.gravity);
      break;
    case RYUJIN_IV_SMOOTH_VORTEX:
      c[0] = hp.gravity;
      c[1] = in.params[2] / (2.0 * M_PI);
      c[2] = 1.0 / (2.0 * hp.gravity);
      break;
    case RYUJIN_IV_SLOPING_FRICTION: {
      const double n_m = hp.manning_friction_coefficient, slope = in.params[0], q0 = in.params[1];
      const double exponent = 1.0 / (2.0 + 4.0 / 3.0);
      const double profile = n_m * n_m * q0 * q0 / slope;
      c[0] = std::pow(profile, exponent);
      break;
    }
    /* the states of initial_states_library_device.hpp (its table of c[]); c[0]: the system's gamma, which
     * from_primitive_state of Euler divides by */
    case RYUJIN_IV_THREE_STATE_CONTRAST:
      c[0] = hp.gamma;
      c[1] = in.params[3] + in.params[7];
      break;
    case RYUJIN_IV_SHOCK_FRONT: {
      /* the constructor of initial_state_shock_front.h, as initial_states.euler_shock_front_constants */
      const double gamma = eq == RYUJIN_EQ_EULER ? hp.gamma : in.params[4];
      const double b = eq == RYUJIN_EQ_EULER ? 0. : ctx.aeosparams.b; /* eos_interpolation_b */
      const double rho_R = in.params[0], u_R = in.params[1], p_R = in.params[2], mach = in.params[3];
      const double a_R = std::sqrt(gamma * p_R / rho_R / (1.0 - b * rho_R));
      const double mach_R = u_R / a_R;
      const double S3 = mach * a_R;
      const double delta_mach = mach_R - mach;
      const double rho_L =
          rho_R * (gamma + 1.0) * delta_mach * delta_mach / ((gamma - 1.0) * delta_mach * delta_mach + 2.0);
      const double u_L = (1.0 - rho_R / rho_L) * S3 + rho_R / rho_L * u_R;
      const double p_L = p_R * (2.0 * gamma * delta_mach * delta_mach - (gamma - 1.0)) / (gamma + 1.0);
      if (!std::isfinite(rho_L) || !std::isfinite(u_L) || !std::isfinite(p_L) || !std::isfinite(S3))
        throw HipError(RYUJIN_ERR_ARG, "initial values: shock front: the state behind the shock is not finite");
      c[0] = hp.gamma;
      c[1] = rho_L;
      c[2] = u_L;
      c[3] = p_L;
      c[4] = S3;
      break;
    }
    case RYUJIN_IV_NOH: {
      /* initial_states.euler_noh_constants: pow(., dim) and pow(., dim - 1) as products, left to right */
      const double gamma = eq == RYUJIN_EQ_EULER ? hp.gamma : in.params[3];
      if (!(gamma > 1.))
        throw HipError(RYUJIN_ERR_ARG, "initial values: noh needs gamma > 1");
      const double rho0 = in.params[0], u0 = in.params[1];
      const double ratio = (gamma + 1.0) / (gamma - 1.0);
      double ratio_dim = ratio, plus_dim = gamma + 1.0, minus_dim1 = 1.0;
      for (int d = 1; d < dim; ++d) {
        ratio_dim = ratio_dim * ratio;
        plus_dim = plus_dim * (gamma + 1.0);
        minus_dim1 = minus_dim1 * (gamma - 1.0);
      }
      double p_in = 0.5 * rho0 * u0 * u0;
      p_in = p_in * (plus_dim / minus_dim1);
      c[0] = hp.gamma;
      c[1] = u0 * (gamma - 1.0) / 2.0;
      c[2] = rho0 * ratio_dim;
      c[3] = p_in;
      c[4] = 10. * std::numeric_limits<double>::min();
      break;
    }
    case RYUJIN_IV_SMOOTH_WAVE: {
      const double left = 0.1, right = 0.3;
      const double width2 = (right - left) * (right - left);
      c[0] = hp.gamma;
      c[1] = width2 * (width2 * width2); /* fixed_power<6>(right - left) */
      c[2] = left;
      c[3] = right;
      break;
    }
    /* the states of initial_states_bathymetry_device.hpp (its table of c[]) */
    case RYUJIN_IV_SW_FLOW_OVER_BUMP: {
      /* initial_state_flow_over_bump.h:62-80, as initial_states.sw_flow_over_bump_constants */
      const double g = hp.gravity;
      double h_inflow = 0.28205279813802181, q_inflow = 0.18;
      double cBer = 0.2 + 1.5 * std::pow(q_inflow * q_inflow / g, 1. / 3.);
      if (in.params[0] == 1.) { /* subsonic */
        q_inflow = 4.42;
        h_inflow = 2.;
        const double ratio = q_inflow / h_inflow;
        cBer = ratio * ratio / (2. * g) + h_inflow;
      }
      c[0] = h_inflow;
      c[1] = q_inflow;
      c[2] = cBer;
      c[3] = q_inflow * q_inflow / (2. * g);
      break;
    }
    case RYUJIN_IV_SW_THREE_BUMPS_DAM_BREAK:
      c[0] = in.params[1] * std::sqrt(hp.gravity * in.params[1]); /* h_L speed_of_sound((h_L, 0)) */
      break;
    case RYUJIN_IV_SW_HOU_TEST:
    case RYUJIN_IV_SW_TRANSIENT:
      break;
    case RYUJIN_IV_SW_SOLITON: {
      const double depth = in.params[0], amplitude = in.params[1];
      c[0] = std::sqrt(hp.gravity * (amplitude + depth));
      c[1] = std::sqrt(3. * amplitude / (4. * depth * depth * (amplitude + depth)));
      break;
    }
    default: /* contrast, four state contrast, ramp up, astro jet; uniform and contrast of shallow water */
      c[0] = hp.gamma;
      break;
    }
    return P;
  }
} // namespace

extern "C" {

int ryujin_hip_initial_values_configure(ryujin_hip_ctx *ctx, const ryujin_hip_initial_values *initial_values,
                                        const double *positions, const double *b_positions)
{
  return guarded_ctx(ctx, [&]() {
    if (!initial_values)
      throw HipError(RYUJIN_ERR_ARG, "initial values: null argument");
    if (ctx->params.equation == RYUJIN_EQ_SCALAR_CONSERVATION)
      throw HipError(RYUJIN_ERR_UNSUPPORTED, "initial values: scalar conservation is not offered");
    const InitialValuesParams P = make_initial_values_params(*ctx, *initial_values);
    if ((!positions && ctx->L.n_relevant > 0) || (!b_positions && ctx->bdry.n_bdry > 0))
      throw HipError(RYUJIN_ERR_ARG, "initial values: positions missing");
    ctx->finish();
    ctx->iv_configured = false;
    upload_initial_values_positions(ctx, positions, b_positions);
    ctx->iv = P;
    ctx->iv_configured = true;
    return RYUJIN_OK;
  });
}

int ryujin_hip_initial_values_configure_function(ryujin_hip_ctx *ctx, int n_expressions,
                                                 const char *const *expressions, const double direction[3],
                                                 const double position[3], const double *positions,
                                                 const double *b_positions)
{
  return guarded_ctx(ctx, [&]() {
    static_assert(kExprOk == RYUJIN_OK && kExprErrArg == RYUJIN_ERR_ARG && kExprErrUnsupported == RYUJIN_ERR_UNSUPPORTED,
                  "expression.hpp and the header agree");
    if (!expressions || !direction || !position)
      throw HipError(RYUJIN_ERR_ARG, "initial values: null argument");
    if (n_expressions != ctx->K)
      throw HipError(RYUJIN_ERR_ARG, "initial values: " + std::to_string(n_expressions) + " expressions for " +
                                         std::to_string(ctx->K) + " primitive components");
    /* everything that can be refused comes first: a refused call leaves the previous configuration in place */
    auto program = std::make_unique<IvFunctionProgram>();
    program->n = 0;
    program->pad = 0;
    auto one = std::make_unique<ExprProgram>();
    for (int q = 0; q < n_expressions; ++q) {
      std::string error;
      if (const int status = expr_compile(expressions[q], ctx->dim, *one, error))
        throw HipError(status, "initial values: component " + std::to_string(q) + ": " + error);
      std::copy(one->code, one->code + one->n, program->code + program->n);
      program->n += one->n;
      program->code[program->n++] = ExprInstruction{kExResult, q, 0.};
    }
    InitialValuesParams P{};
    P.state = kIvFunction;
    P.c[0] = ctx->params.gamma; /* Euler: from_primitive_state */
    set_initial_values_frame(P, ctx->dim, direction, position);
    if ((!positions && ctx->L.n_relevant > 0) || (!b_positions && ctx->bdry.n_bdry > 0))
      throw HipError(RYUJIN_ERR_ARG, "initial values: positions missing");
    ctx->finish();
    ctx->iv_configured = false;
    upload_initial_values_positions(ctx, positions, b_positions);
    ctx->d_iv_function.upload(program.get(), 1);
    ctx->iv = P;
    ctx->iv_configured = true;
    return RYUJIN_OK;
  });
}

int ryujin_hip_expression_evaluate(const char *expression, int dim, const double *points, size_t n, double t,
                                   double *out)
{
  return guarded([&]() {
    if (!expression || (n > 0 && (!points || !out)))
      throw HipError(RYUJIN_ERR_ARG, "expression_evaluate: null argument");
    auto program = std::make_unique<ExprProgram>();
    std::string error;
    if (const int status = expr_compile(expression, dim, *program, error))
      throw HipError(status, error);
    expr_evaluate_points(*program, dim, points, n, t, out);
    return RYUJIN_OK;
  });
}

/* ---- FluxLibrary "function" of the scalar conservation equation ---- */

int ryujin_hip_flux_configure_function(ryujin_hip_ctx *ctx, const char *expression,
                                       double derivative_approximation_delta)
{
  return guarded_ctx(ctx, [&]() {
    if (ctx->params.equation != RYUJIN_EQ_SCALAR_CONSERVATION)
      throw HipError(RYUJIN_ERR_UNSUPPORTED, "flux: only the scalar conservation equation takes a flux");
    /* everything that can be refused comes first: a refused call leaves the earlier flux in place */
    if (!expression)
      throw HipError(RYUJIN_ERR_ARG, "flux: null expression");
    if (!(derivative_approximation_delta > 0.) || !std::isfinite(derivative_approximation_delta))
      throw HipError(RYUJIN_ERR_ARG, "flux: derivative approximation delta must be positive and finite");
    auto program = std::make_unique<FluxProgram>();
    std::string error;
    if (const int status = flux_compile(expression, ctx->dim, *program, error))
      throw HipError(status, error);
    ctx->finish(); /* nothing enqueued may still read the earlier programs */
    ctx->d_flux_function.upload(program.get(), 1);
    ctx->flux_n_instructions = program->n_instructions;
    ctx->scparams.flux = RYUJIN_FLUX_FUNCTION;
    ctx->scparams.delta = derivative_approximation_delta;
    for (auto &s : ctx->states) /* (scalar conservation leaves no precomputed values behind a step; all the same) */
      if (s)
        s->precomputed = false;
    return RYUJIN_OK;
  });
}

int ryujin_hip_flux_function_evaluate(const char *expression, int dim, double delta, const double *u, size_t n,
                                      double *value, double *gradient)
{
  return guarded([&]() {
    if (!expression || (n > 0 && (!u || !value)))
      throw HipError(RYUJIN_ERR_ARG, "flux_function_evaluate: null argument");
    if (!(delta > 0.) || !std::isfinite(delta))
      throw HipError(RYUJIN_ERR_ARG, "flux_function_evaluate: delta must be positive and finite");
    auto program = std::make_unique<FluxProgram>();
    std::string error;
    if (const int status = flux_compile(expression, dim, *program, error))
      throw HipError(status, error);
    flux_evaluate_points(*program, dim, delta, u, n, value, gradient);
    return RYUJIN_OK;
  });
}

int ryujin_hip_flux_info(ryujin_hip_ctx *ctx, int *kind, int *n_instructions, int *step2_interpreted)
{
  return guarded_ctx(ctx, [&]() {
    if (ctx->params.equation != RYUJIN_EQ_SCALAR_CONSERVATION)
      throw HipError(RYUJIN_ERR_UNSUPPORTED, "flux: only the scalar conservation equation takes a flux");
    const bool ran = ctx->last_flux_kind >= 0;
    if (kind)
      *kind = ran ? ctx->last_flux_kind : ctx->scparams.flux;
    if (n_instructions)
      *n_instructions = ran ? ctx->last_flux_n_instructions
                            : (ctx->scparams.flux == RYUJIN_FLUX_FUNCTION ? ctx->flux_n_instructions : 0);
    if (step2_interpreted)
      *step2_interpreted = ran ? ctx->last_step2_interpreted : 0;
    return RYUJIN_OK;
  });
}

/* ---- EquationOfStateLibrary "function" of EulerAEOS ---- */

int ryujin_hip_eos_configure_function(ryujin_hip_ctx *ctx, const char *pressure, const char *specific_internal_energy,
                                      const char *temperature, const char *speed_of_sound, double interpolation_b,
                                      double interpolation_pinfty, double interpolation_q)
{
  return guarded_ctx(ctx, [&]() {
    if (ctx->params.equation != RYUJIN_EQ_EULER_AEOS)
      throw HipError(RYUJIN_ERR_UNSUPPORTED, "eos: only EulerAEOS takes an equation of state");
    /* everything that can be refused comes first: a refused call leaves the earlier equation of state in place */
    const char *const expressions[kEosPrograms] = {pressure, specific_internal_energy, temperature, speed_of_sound};
    auto program = std::make_unique<EosProgram>();
    std::string error;
    if (const int status =
            eos_compile(expressions, interpolation_b, interpolation_pinfty, interpolation_q, *program, error))
      throw HipError(status, error);
    ctx->finish();
    ctx->set_eos_function(*program, interpolation_b, interpolation_pinfty, interpolation_q);
    return RYUJIN_OK;
  });
}

int ryujin_hip_eos_function_evaluate(int which, const char *expression, const double *rho, const double *second,
                                     size_t n, double *out)
{
  return guarded([&]() {
    if (which < 0 || which >= kEosPrograms)
      throw HipError(RYUJIN_ERR_ARG, "eos_function_evaluate: which outside 0 .. 3");
    if (n > 0 && (!rho || !second || !out))
      throw HipError(RYUJIN_ERR_ARG, "eos_function_evaluate: null argument");
    const char *expressions[kEosPrograms] = {nullptr, nullptr, nullptr, nullptr};
    expressions[which] = expression; /* NULL: the default */
    auto program = std::make_unique<EosProgram>();
    std::string error;
    if (const int status = eos_compile(expressions, 0., 0., 0., *program, error))
      throw HipError(status, error);
    eos_evaluate_points(*program, which, rho, second, n, out);
    return RYUJIN_OK;
  });
}

int ryujin_hip_eos_function_evaluate_device(ryujin_hip_ctx *ctx, int which, const double *rho, const double *second,
                                            size_t n, double *out)
{
  return guarded_ctx(ctx, [&]() {
    if (ctx->params.equation != RYUJIN_EQ_EULER_AEOS)
      throw HipError(RYUJIN_ERR_UNSUPPORTED, "eos: only EulerAEOS takes an equation of state");
    if (ctx->aeosparams.eos != RYUJIN_EOS_FUNCTION)
      throw HipError(RYUJIN_ERR_ARG, "eos: the function equation of state is not configured");
    if (which < 0 || which >= kEosPrograms)
      throw HipError(RYUJIN_ERR_ARG, "eos_function_evaluate_device: which outside 0 .. 3");
    if (n == 0)
      return RYUJIN_OK;
    if (!rho || !second || !out || n > 0x7fffffffull)
      throw HipError(RYUJIN_ERR_ARG, "eos_function_evaluate_device: bad argument");
    DeviceBuffer<double> d_in, d_out;
    d_in.alloc(2 * n, false);
    d_out.alloc(n, false);
    HIP_CHECK(hipMemcpyAsync(d_in.ptr, rho, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(d_in.ptr + n, second, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_eos_function_points, dim3(grid_for(n, kEosFunctionBlock)), dim3(kEosFunctionBlock), 0,
                       ctx->stream, ctx->d_eos_function.ptr, which, (uint32_t)n, d_in.ptr, d_in.ptr + n, d_out.ptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, d_out.ptr, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RYUJIN_OK;
  });
}

int ryujin_hip_eos_info(ryujin_hip_ctx *ctx, int *kind, int *n_instructions, int *precompute_interpreted)
{
  return guarded_ctx(ctx, [&]() {
    if (ctx->params.equation != RYUJIN_EQ_EULER_AEOS)
      throw HipError(RYUJIN_ERR_UNSUPPORTED, "eos: only EulerAEOS takes an equation of state");
    const bool ran = ctx->last_eos_kind >= 0;
    const bool function = ctx->aeosparams.eos == RYUJIN_EOS_FUNCTION;
    if (kind)
      *kind = ran ? ctx->last_eos_kind : ctx->aeosparams.eos;
    if (n_instructions)
      for (int w = 0; w < kEosPrograms; ++w)
        n_instructions[w] = ran ? ctx->last_eos_n_instructions[w] : (function ? ctx->eos_n_instructions[w] : 0);
    if (precompute_interpreted)
      *precompute_interpreted = ran ? ctx->last_precompute_interpreted : 0;
    return RYUJIN_OK;
  });
}

int ryujin_hip_initial_values_evaluate(ryujin_hip_ctx *ctx, const double *points, size_t n, double t, double *out)
{
  return guarded_ctx(ctx, [&]() {
    ctx->require_initial_values();
    if (n == 0)
      return RYUJIN_OK;
    if (!points || !out || n > 0xffffffffull)
      throw HipError(RYUJIN_ERR_ARG, "initial values: bad argument");
    initial_values_round_trip(ctx, points, n, (size_t)ctx->K, out, [&]() {
      dispatch_initial_values(ctx, [&](auto tag) {
        ctx->template initial_values_points<typename decltype(tag)::type>(ctx->d_iv_points.ptr, n, t, ctx->K,
                                                                          ctx->d_iv_values.ptr);
        return RYUJIN_OK;
      });
    });
    return RYUJIN_OK;
  });
}

int ryujin_hip_initial_values_interpolate(ryujin_hip_ctx *ctx, int handle, double t)
{
  return guarded_ctx(ctx, [&]() {
    ctx->require_initial_values();
    auto &s = ctx->state(handle);
    ctx->wait_comm(); /* an exchange of this vector may still be in flight */
    s.precomputed = false;
    return dispatch_initial_values(ctx, [&](auto tag) {
      ctx->template initial_values_points<typename decltype(tag)::type>(ctx->d_iv_positions.ptr, ctx->L.n_relevant, t,
                                                                        ctx->KP, s.U.ptr);
      return RYUJIN_OK;
    });
  });
}

int ryujin_hip_initial_values_interpolate_initial_precomputed(ryujin_hip_ctx *ctx)
{
  return guarded_ctx(ctx, [&]() {
    ctx->require_initial_precomputed();
    /* on the compute stream, behind every kernel that reads the bathymetry (step 4, the output extraction) */
    ctx->initial_precomputed_points(ctx->d_iv_positions.ptr, ctx->L.n_relevant, ctx->d_Z.ptr);
    return RYUJIN_OK;
  });
}

int ryujin_hip_initial_values_evaluate_initial_precomputed(ryujin_hip_ctx *ctx, const double *points, size_t n,
                                                           double *out)
{
  return guarded_ctx(ctx, [&]() {
    ctx->require_initial_precomputed();
    if (n == 0)
      return RYUJIN_OK;
    if (!points || !out || n > 0xffffffffull)
      throw HipError(RYUJIN_ERR_ARG, "initial values: bad argument");
    initial_values_round_trip(ctx, points, n, 1, out, [&]() {
      ctx->initial_precomputed_points(ctx->d_iv_points.ptr, n, ctx->d_iv_values.ptr);
    });
    return RYUJIN_OK;
  });
}

int ryujin_hip_get_initial_precomputed(ryujin_hip_ctx *ctx, double *out)
{
  return guarded_ctx(ctx, [&]() {
    ctx->require_initial_precomputed();
    if (ctx->L.n_relevant == 0)
      return RYUJIN_OK;
    if (!out)
      throw HipError(RYUJIN_ERR_ARG, "initial values: bad argument");
    HIP_CHECK(hipMemcpyAsync(out, ctx->d_Z.ptr, (size_t)ctx->L.n_relevant * sizeof(double), hipMemcpyDeviceToHost,
                             ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RYUJIN_OK;
  });
}

int ryujin_hip_prepare_state_vector_iv(ryujin_hip_ctx *ctx, int handle, double t)
{
  return guarded_ctx(ctx, [&]() {
    ctx->require_initial_values();
    return dispatch_initial_values(ctx, [&](auto tag) {
      ctx->template prepare_state_vector<typename decltype(tag)::type>(handle, nullptr,
                                                                       ryujin_hip_ctx::IvStage{true, t, 0.});
      return RYUJIN_OK;
    });
  });
}

int ryujin_hip_time_step_iv(ryujin_hip_ctx *ctx, int scheme, int h_state, int n_tmp, const int *h_tmp, double t,
                            double tau_max, int cfl_recovery, double cfl_min, double cfl_max, double *tau_out)
{
  return guarded_ctx(ctx, [&]() {
    ctx->require_initial_values();
    if (const int status = check_time_step_args(ctx, h_state, n_tmp, h_tmp, tau_max, tau_out))
      return status;
    return dispatch_initial_values(ctx, [&](auto tag) {
      return ctx->template time_step<typename decltype(tag)::type>(scheme, h_state, n_tmp, h_tmp, nullptr, tau_max,
                                                                   cfl_recovery, cfl_min, cfl_max, tau_out, t,
                                                                   nullptr, nullptr, true);
    });
  });
}

} /* extern "C" */

/* ---- Error norms --------------------------------------------------------- */

extern "C" {

int ryujin_hip_error_norms_configure(ryujin_hip_ctx *ctx, uint32_t n_cells, int dofs_per_cell,
                                     const uint32_t *cell_dofs, int n_q, const double *shape, const double *weights,
                                     const double *jxw, int jxw_per_cell)
{
  return guarded_ctx(ctx, [&]() {
    static_assert(RYUJIN_EN_MAX_DOFS_PER_CELL == kErrorNormsMaxDofs && RYUJIN_EN_MAX_POINTS == kErrorNormsMaxPoints,
                  "header and kernels agree");
    if (dofs_per_cell < 2 || dofs_per_cell > kErrorNormsMaxDofs)
      throw HipError(RYUJIN_ERR_ARG, "error_norms_configure: dofs_per_cell " + std::to_string(dofs_per_cell) +
                                         " outside [2, " + std::to_string(kErrorNormsMaxDofs) + "]");
    if (n_q < 1 || n_q > kErrorNormsMaxPoints)
      throw HipError(RYUJIN_ERR_ARG, "error_norms_configure: n_q " + std::to_string(n_q) + " outside [1, " +
                                         std::to_string(kErrorNormsMaxPoints) + "]");
    if (!shape)
      throw HipError(RYUJIN_ERR_ARG, "error_norms_configure: null shape table");
    if (jxw_per_cell && !weights)
      throw HipError(RYUJIN_ERR_ARG, "error_norms_configure: null weights with jxw_per_cell");
    if (n_cells > 0 && (!cell_dofs || !jxw))
      throw HipError(RYUJIN_ERR_ARG, "error_norms_configure: null cell_dofs or jxw with n_cells > 0");
    const size_t n = n_cells, dpc = (size_t)dofs_per_cell, nq = (size_t)n_q;
    for (size_t e = 0; e < nq * dpc; ++e)
      if (!std::isfinite(shape[e]))
        throw HipError(RYUJIN_ERR_ARG, "error_norms_configure: shape value " + std::to_string(e) + " is not finite");
    if (weights)
      for (size_t q = 0; q < nq; ++q)
        if (!std::isfinite(weights[q]))
          throw HipError(RYUJIN_ERR_ARG, "error_norms_configure: weights entry " + std::to_string(q) + " is not finite");
    const size_t n_jxw = jxw_per_cell ? n : n * nq;
    for (size_t e = 0; e < n_jxw; ++e)
      if (!std::isfinite(jxw[e]))
        throw HipError(RYUJIN_ERR_ARG, "error_norms_configure: jxw entry " + std::to_string(e) + " is not finite");
    const uint32_t n_relevant = ctx->L.n_relevant;
    for (size_t e = 0; e < n * dpc; ++e)
      if (cell_dofs[e] >= n_relevant)
        throw HipError(RYUJIN_ERR_ARG, "error_norms_configure: index " + std::to_string(cell_dofs[e]) + " of cell " +
                                           std::to_string(e / dpc) + " is not below n_relevant = " +
                                           std::to_string(n_relevant));
    /* both cell streams transposed: lane = cell reads them coalesced */
    std::vector<uint32_t> dofs_t(n * dpc);
    for (size_t c = 0; c < n; ++c)
      for (size_t v = 0; v < dpc; ++v)
        dofs_t[v * n + c] = cell_dofs[c * dpc + v];
    std::vector<double> jxw_t(n_jxw);
    if (jxw_per_cell)
      std::copy(jxw, jxw + n, jxw_t.begin());
    else
      for (size_t c = 0; c < n; ++c)
        for (size_t q = 0; q < nq; ++q)
          jxw_t[q * n + c] = jxw[c * nq + q];
    std::vector<double> w(nq, 0.);
    if (weights)
      std::copy(weights, weights + nq, w.begin());
    auto en = std::make_unique<ryujin_hip_ctx::ErrorNorms>();
    en->n_cells = n_cells;
    en->n_blocks = (uint32_t)std::min<size_t>(kErrorNormsMaxBlocks, (n + kBlock - 1) / kBlock);
    en->dofs_per_cell = dofs_per_cell;
    en->n_q = n_q;
    en->jxw_per_cell = jxw_per_cell ? 1 : 0;
    en->d_cell_dofs.upload(dofs_t);
    en->d_jxw.upload(jxw_t);
    en->d_shape.upload(shape, nq * dpc);
    en->d_weights.upload(w);
    en->d_work.alloc((size_t)en->n_blocks * kErrorNormsSums + kErrorNormsSums + 2 * kErrorNormsMaxComponents +
                     kErrorNormsResult);
    /* a second configure replaces the first: nothing enqueued may still read the old arrays */
    ctx->finish();
    ctx->error_norms = std::move(en);
    return RYUJIN_OK;
  });
}

int ryujin_hip_error_norms_compute(ryujin_hip_ctx *ctx, int h_state, int h_analytic, int n_components,
                                   const int *components, int normalize, double out[3], double *detail)
{
  return guarded_ctx(ctx, [&]() {
    if (!ctx->error_norms)
      throw HipError(RYUJIN_ERR_ARG, "error_norms_compute before error_norms_configure");
    if (!components || !out)
      throw HipError(RYUJIN_ERR_ARG, "error_norms_compute: null argument");
    static_assert(RYUJIN_EN_MAX_COMPONENTS == kErrorNormsMaxComponents, "header and kernels agree");
    if (n_components < 1 || n_components > ctx->K || n_components > kErrorNormsMaxComponents)
      throw HipError(RYUJIN_ERR_ARG, "error_norms_compute: n_components " + std::to_string(n_components) +
                                         " outside [1, " + std::to_string(ctx->K) + "]");
    ErrorNormsDesc D{};
    D.n = n_components;
    D.stride = ctx->KP;
    D.normalize = normalize ? 1 : 0;
    for (int c = 0; c < n_components; ++c) {
      if (components[c] < 0 || components[c] >= ctx->K)
        throw HipError(RYUJIN_ERR_ARG, "error_norms_compute: component " + std::to_string(components[c]) +
                                           " outside the state");
      D.component[c] = components[c];
    }
    ctx->state(h_state);
    ctx->state(h_analytic);
    double host[kErrorNormsResult];
    ctx->error_norms_compute(h_state, h_analytic, D, host);
    for (int q = 0; q < 3; ++q)
      out[q] = host[q];
    if (detail)
      for (int q = 0; q < 6 * n_components; ++q)
        detail[q] = host[3 + q];
    return RYUJIN_OK;
  });
}

} /* extern "C" */

/* ---- VTUOutput: selected fields and level-set cell output ------------------------------------------------- */

/* One output (source/vtu_output.template.h:98-123, selected_components_extractor.h:91-123): the ghost range of the
 * state vector and of the per-node columns (alpha, the postprocessed fields) exchanged, then ONE sweep over the output
 * nodes. Every rank makes the exchanges, whatever it selected; a rank without output nodes launches nothing else. */
template <typename E>
void ryujin_hip_ctx::output_extract(Output &o, int h, bool levelsets, bool float64, void *host_out)
{
  State &s = state(h);
  OutputDesc D = o.desc;
  wait_comm();
  if (D.any_state) {
    exchange_vector(s.U.ptr, KP, false);
    wait_comm();
  }
  /* alpha and the postprocessed fields: where this rank has ghost rows, a copy of the owned values whose ghost range
   * the context's vector exchange fills with the owners' */
  const size_t n_relevant = L.n_relevant, n_owned = L.n_owned;
  size_t column = 0;
  for (int q = 0; q < D.n; ++q) {
    if (D.kind[q] != kOutAlpha && D.kind[q] != kOutPostprocessed)
      continue;
    const double *source = D.kind[q] == kOutAlpha ? d_alpha.ptr : d_pp_normalised.ptr + (size_t)D.index[q] * n_owned;
    if (exch.n_nbr == 0) {
      D.column[q] = source;
      continue;
    }
    double *copy = o.d_columns.ptr + column++ * n_relevant;
    HIP_CHECK(hipMemcpyAsync(copy, source, n_owned * sizeof(double), hipMemcpyDeviceToDevice, stream));
    exchange_vector(copy, 1, false);
    wait_comm();
    D.column[q] = copy;
  }

  const uint32_t n_nodes = levelsets ? o.n_selected_nodes : L.n_relevant;
  if (n_nodes == 0)
    return;
  const size_t bytes = (size_t)D.n * n_nodes * (float64 ? sizeof(double) : sizeof(float));
  if (o.d_out.n < bytes)
    o.d_out.alloc(bytes, false);
  HIP_CHECK(hipMemcpyAsync(o.d_desc.ptr, &D, sizeof(OutputDesc), hipMemcpyHostToDevice, stream));
  const uint32_t *node_ids = levelsets ? o.d_node_ids.ptr : nullptr;
  const dim3 grid(grid_for(n_nodes)), block(kBlock);
  if (float64)
    hipLaunchKernelGGL((k_output_extract<E, double>), grid, block, 0, stream, eq_params<E>(), o.d_desc.ptr, n_nodes,
                       node_ids, s.U.ptr, s.prec.ptr, d_Z.ptr, reinterpret_cast<double *>(o.d_out.ptr));
  else
    hipLaunchKernelGGL((k_output_extract<E, float>), grid, block, 0, stream, eq_params<E>(), o.d_desc.ptr, n_nodes,
                       node_ids, s.U.ptr, s.prec.ptr, d_Z.ptr, reinterpret_cast<float *>(o.d_out.ptr));
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(host_out, o.d_out.ptr, bytes, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream));
}

namespace
{
  /* flags [n] -> the ascending list of the set ones (and, unless NULL, the map item -> position): count, scan in a
   * launch of its own, the total to the host (the list is allocated from it), compaction. n > 0. */
  uint32_t compact_flags(ryujin_hip_ctx *ctx, const uint32_t n, const uint8_t *flags, DeviceBuffer<uint32_t> &scan,
                         DeviceBuffer<uint32_t> &list, uint32_t *map)
  {
    const uint32_t n_blocks = (uint32_t)output_compaction_blocks(n, kBlock);
    scan.alloc(2 * (size_t)n_blocks + 1, false); /* counts [n_blocks], offsets [n_blocks + 1] */
    uint32_t *counts = scan.ptr, *offsets = scan.ptr + n_blocks;
    hipLaunchKernelGGL(k_output_count, dim3(n_blocks), dim3(kBlock), 0, ctx->stream, n, flags, counts);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_output_scan, dim3(1), dim3(kBlock), 0, ctx->stream, n_blocks, counts, offsets);
    HIP_CHECK(hipGetLastError());
    uint32_t total = 0;
    HIP_CHECK(hipMemcpyAsync(&total, offsets + n_blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (total > n)
      throw HipError(RYUJIN_ERR_HIP, "output: the compaction counted more items than there are");
    list.alloc(total, false);
    hipLaunchKernelGGL(k_output_compact, dim3(n_blocks), dim3(kBlock), 0, ctx->stream, n, flags, offsets, list.ptr, map);
    HIP_CHECK(hipGetLastError());
    return total;
  }

  ryujin_hip_ctx::Output &require_output(ryujin_hip_ctx *ctx, const char *what)
  {
    if (!ctx->output)
      throw HipError(RYUJIN_ERR_ARG, std::string(what) + " before output_configure");
    return *ctx->output;
  }
} // namespace

extern "C" {

int ryujin_hip_output_configure(ryujin_hip_ctx *ctx, int n_quantities, const char *const *names,
                                const double *positions, uint32_t n_cells, int dofs_per_cell,
                                const uint32_t *cell_dofs, int n_manifolds, const char *const *manifolds)
{
  return guarded_ctx(ctx, [&]() {
    static_assert(RYUJIN_OUT_MAX_QUANTITIES == kOutputMaxQuantities && RYUJIN_OUT_MAX_MANIFOLDS == kOutputMaxManifolds,
                  "header and kernels agree");
    static_assert(kOutEqEuler == RYUJIN_EQ_EULER && kOutEqShallowWater == RYUJIN_EQ_SHALLOW_WATER &&
                      kOutEqEulerAeos == RYUJIN_EQ_EULER_AEOS &&
                      kOutEqScalarConservation == RYUJIN_EQ_SCALAR_CONSERVATION &&
                      kOutPpSchlieren == RYUJIN_PP_SCHLIEREN && kOutPpVorticity == RYUJIN_PP_VORTICITY,
                  "output_selection.hpp and the header agree");
    /* everything that can be refused comes first: a refused call leaves the previous configuration in place */
    if (n_quantities < 1 || n_quantities > kOutputMaxQuantities || !names)
      throw HipError(RYUJIN_ERR_ARG, "output_configure: n_quantities must be in [1, " +
                                         std::to_string(kOutputMaxQuantities) + "] and names given");
    if (n_manifolds < 0 || n_manifolds > kOutputMaxManifolds || (n_manifolds > 0 && !manifolds))
      throw HipError(RYUJIN_ERR_ARG, "output_configure: n_manifolds must be in [0, " +
                                         std::to_string(kOutputMaxManifolds) + "] and manifolds given");
    const int dim = ctx->dim;
    if (dofs_per_cell != (1 << dim))
      throw HipError(RYUJIN_ERR_UNSUPPORTED, "output_configure: dofs_per_cell " + std::to_string(dofs_per_cell) +
                                                 " is not 2^dim: patches of higher-order elements are not subdivided");
    const uint32_t n_relevant = ctx->L.n_relevant;
    if ((!positions && n_relevant > 0) || (!cell_dofs && n_cells > 0))
      throw HipError(RYUJIN_ERR_ARG, "output_configure: null positions or cell_dofs with a non-zero count");

    auto o = std::make_unique<ryujin_hip_ctx::Output>();
    OutputNames tables;
    if (!output_names(ctx->params.equation, dim, tables))
      throw HipError(RYUJIN_ERR_ARG, "output_configure: no name tables for this Description");
    std::vector<OutputPostprocessQuantity> pp;
    if (ctx->pp_configured)
      for (int q = 0; q < ctx->pp_desc.n; ++q) {
        const int select = ctx->pp_desc.select[q];
        pp.push_back(OutputPostprocessQuantity{ctx->pp_desc.kind[q], select >= ctx->K ? 1 : 0, select % ctx->K});
        o->pp_kind[q] = ctx->pp_desc.kind[q];
        o->pp_select[q] = select;
      }
    o->n_postprocess = (int)pp.size();
    const std::vector<std::string> pp_names = output_postprocess_names(tables, pp.data(), (int)pp.size());
    OutputDesc &D = o->desc;
    D.n = n_quantities;
    D.n_precomputed = ctx->NPREC;
    D.n_initial_precomputed = 1; /* the bathymetry: d_Z holds one double per node */
    size_t n_columns = 0;
    for (int q = 0; q < n_quantities; ++q) {
      if (!names[q])
        throw HipError(RYUJIN_ERR_ARG, "output_configure: name " + std::to_string(q) + " is null");
      OutputResolved r{};
      std::string error;
      if (!output_resolve(tables, pp_names, names[q], r, error))
        throw HipError(RYUJIN_ERR_ARG, error);
      if ((r.kind == kOutPrecomputed && r.index >= ctx->NPREC) || (r.kind == kOutInitialPrecomputed && r.index >= 1) ||
          ((r.kind == kOutConserved || r.kind == kOutPrimitive) && r.index >= ctx->K))
        throw HipError(RYUJIN_ERR_ARG, "output_configure: \"" + std::string(names[q]) + "\" is outside the arrays of the context");
      D.kind[q] = r.kind;
      D.index[q] = r.index;
      D.any_state = D.any_state || r.kind == kOutConserved || r.kind == kOutPrimitive;
      D.any_primitive = D.any_primitive || r.kind == kOutPrimitive;
      o->needs_precomputed = o->needs_precomputed || r.kind == kOutPrecomputed;
      o->needs_postprocessed = o->needs_postprocessed || r.kind == kOutPostprocessed;
      n_columns += (r.kind == kOutAlpha || r.kind == kOutPostprocessed) ? 1 : 0;
    }
    auto program = std::make_unique<OutputManifoldProgram>();
    program->n = 0;
    program->n_manifolds = n_manifolds;
    {
      static const char *const xyz[3] = {"x", "y", "z"}; /* FunctionParser<dim>(expression): no time */
      const ExprVariables variables{xyz, 3, 3};
      auto one = std::make_unique<ExprProgram>();
      for (int m = 0; m < n_manifolds; ++m) {
        std::string error;
        if (const int status = expr_compile(manifolds[m], dim, *one, error, variables))
          throw HipError(status, "output_configure: manifold " + std::to_string(m) + ": " + error);
        std::copy(one->code, one->code + one->n, program->code + program->n);
        program->n += one->n;
        program->code[program->n++] = ExprInstruction{kExResult, m, 0.};
      }
    }
    const size_t n = n_cells, dpc = (size_t)dofs_per_cell;
    for (size_t e = 0; e < n * dpc; ++e)
      if (cell_dofs[e] >= n_relevant)
        throw HipError(RYUJIN_ERR_ARG, "output_configure: index " + std::to_string(cell_dofs[e]) + " of cell " +
                                           std::to_string(e / dpc) + " is not below n_relevant = " +
                                           std::to_string(n_relevant));

    /* the selection, on the device; nothing of the context changes before it is complete */
    o->n_manifolds = n_manifolds;
    o->dofs_per_cell = dofs_per_cell;
    o->n_cells = n_cells;
    o->d_desc.alloc(1, false);
    if (ctx->exch.n_nbr > 0)
      o->d_columns.alloc(n_columns * n_relevant);
    if (n_manifolds > 0 && n_relevant > 0) {
      DeviceBuffer<double> d_positions;
      DeviceBuffer<OutputManifoldProgram> d_program;
      d_positions.upload(positions, (size_t)n_relevant * dim);
      d_program.upload(program.get(), 1);
      o->d_levelsets.alloc((size_t)n_manifolds * n_relevant, false);
      const dim3 grid(grid_for(n_relevant, kOutputLevelsetBlock)), block(kOutputLevelsetBlock);
      if (dim == 1)
        hipLaunchKernelGGL(k_output_levelsets<1>, grid, block, 0, ctx->stream, d_program.ptr, n_relevant,
                           d_positions.ptr, o->d_levelsets.ptr);
      else if (dim == 2)
        hipLaunchKernelGGL(k_output_levelsets<2>, grid, block, 0, ctx->stream, d_program.ptr, n_relevant,
                           d_positions.ptr, o->d_levelsets.ptr);
      else
        hipLaunchKernelGGL(k_output_levelsets<3>, grid, block, 0, ctx->stream, d_program.ptr, n_relevant,
                           d_positions.ptr, o->d_levelsets.ptr);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipStreamSynchronize(ctx->stream)); /* the positions and the programs go out of scope */
    }
    if (n_manifolds > 0 && n_cells > 0) {
      std::vector<uint32_t> dofs_t(n * dpc); /* transposed: lane = cell reads it coalesced */
      for (size_t c = 0; c < n; ++c)
        for (size_t v = 0; v < dpc; ++v)
          dofs_t[v * n + c] = cell_dofs[c * dpc + v];
      DeviceBuffer<uint32_t> d_cell_dofs, d_scan, d_node_map;
      DeviceBuffer<uint8_t> d_cell_flags, d_node_flags;
      d_cell_dofs.upload(dofs_t);
      d_cell_flags.alloc(n, false);
      hipLaunchKernelGGL(k_output_cell_flags, dim3(grid_for(n)), dim3(kBlock), 0, ctx->stream, n_cells, dofs_per_cell,
                         d_cell_dofs.ptr, n_manifolds, n_relevant, o->d_levelsets.ptr, d_cell_flags.ptr);
      HIP_CHECK(hipGetLastError());
      o->n_selected_cells = compact_flags(ctx, n_cells, d_cell_flags.ptr, d_scan, o->d_cell_ids, nullptr);
      if (o->n_selected_cells > 0) {
        d_node_flags.alloc(n_relevant); /* zeroed */
        d_node_map.alloc(n_relevant, false);
        hipLaunchKernelGGL(k_output_mark_nodes, dim3(grid_for(o->n_selected_cells)), dim3(kBlock), 0, ctx->stream,
                           o->n_selected_cells, n_cells, dofs_per_cell, o->d_cell_ids.ptr, d_cell_dofs.ptr,
                           d_node_flags.ptr);
        HIP_CHECK(hipGetLastError());
        o->n_selected_nodes = compact_flags(ctx, n_relevant, d_node_flags.ptr, d_scan, o->d_node_ids, d_node_map.ptr);
        o->d_connectivity.alloc((size_t)o->n_selected_cells * dpc, false);
        hipLaunchKernelGGL(k_output_connectivity, dim3(grid_for(o->n_selected_cells)), dim3(kBlock), 0, ctx->stream,
                           o->n_selected_cells, n_cells, dofs_per_cell, o->d_cell_ids.ptr, d_cell_dofs.ptr,
                           d_node_map.ptr, o->d_connectivity.ptr);
        HIP_CHECK(hipGetLastError());
      }
      HIP_CHECK(hipStreamSynchronize(ctx->stream)); /* the scratch arrays go out of scope */
    }
    /* a second configure replaces the first: nothing enqueued may still read the old arrays */
    ctx->finish();
    ctx->output = std::move(o);
    return RYUJIN_OK;
  });
}

int ryujin_hip_output_info(ryujin_hip_ctx *ctx, uint32_t *n_selected_cells, uint32_t *n_selected_nodes)
{
  return guarded_ctx(ctx, [&]() {
    const ryujin_hip_ctx::Output &o = require_output(ctx, "output_info");
    if (n_selected_cells)
      *n_selected_cells = o.n_selected_cells;
    if (n_selected_nodes)
      *n_selected_nodes = o.n_selected_nodes;
    return RYUJIN_OK;
  });
}

int ryujin_hip_output_selection(ryujin_hip_ctx *ctx, uint32_t *cell_ids, uint32_t *node_ids, uint32_t *connectivity)
{
  return guarded_ctx(ctx, [&]() {
    const ryujin_hip_ctx::Output &o = require_output(ctx, "output_selection");
    ctx->finish();
    if (cell_ids && o.n_selected_cells)
      HIP_CHECK(hipMemcpy(cell_ids, o.d_cell_ids.ptr, sizeof(uint32_t) * o.n_selected_cells, hipMemcpyDeviceToHost));
    if (node_ids && o.n_selected_nodes)
      HIP_CHECK(hipMemcpy(node_ids, o.d_node_ids.ptr, sizeof(uint32_t) * o.n_selected_nodes, hipMemcpyDeviceToHost));
    if (connectivity && o.n_selected_cells)
      HIP_CHECK(hipMemcpy(connectivity, o.d_connectivity.ptr,
                          sizeof(uint32_t) * o.n_selected_cells * (size_t)o.dofs_per_cell, hipMemcpyDeviceToHost));
    return RYUJIN_OK;
  });
}

int ryujin_hip_output_levelset_values(ryujin_hip_ctx *ctx, int manifold, double *out)
{
  return guarded_ctx(ctx, [&]() {
    const ryujin_hip_ctx::Output &o = require_output(ctx, "output_levelset_values");
    if (manifold < 0 || manifold >= o.n_manifolds)
      throw HipError(RYUJIN_ERR_ARG, "output_levelset_values: unknown manifold " + std::to_string(manifold));
    const size_t n = ctx->L.n_relevant;
    if (n == 0)
      return RYUJIN_OK;
    if (!out)
      throw HipError(RYUJIN_ERR_ARG, "output_levelset_values: null argument");
    ctx->finish();
    HIP_CHECK(hipMemcpy(out, o.d_levelsets.ptr + (size_t)manifold * n, n * sizeof(double), hipMemcpyDeviceToHost));
    return RYUJIN_OK;
  });
}

int ryujin_hip_output_extract(ryujin_hip_ctx *ctx, int h_state, int levelsets, int precision, void *out)
{
  return guarded_ctx(ctx, [&]() {
    ryujin_hip_ctx::Output &o = require_output(ctx, "output_extract");
    if (levelsets && o.n_manifolds == 0)
      throw HipError(RYUJIN_ERR_ARG, "output_extract: level-set output without a manifold");
    if (precision != RYUJIN_OUT_FLOAT32 && precision != RYUJIN_OUT_FLOAT64)
      throw HipError(RYUJIN_ERR_ARG, "output_extract: unknown precision " + std::to_string(precision));
    const ryujin_hip_ctx::State &s = ctx->state(h_state);
    const size_t n_nodes = levelsets ? o.n_selected_nodes : ctx->L.n_relevant;
    if (!out && n_nodes > 0)
      throw HipError(RYUJIN_ERR_ARG, "output_extract: null output array");
    if (o.needs_precomputed && !s.prepared && !s.precomputed)
      throw HipError(RYUJIN_ERR_ARG, "output_extract: a precomputed quantity of a state vector that no "
                                     "prepare_state_vector has run on");
    if (o.needs_postprocessed) {
      bool same = ctx->pp_configured && ctx->pp_desc.n == o.n_postprocess;
      for (int q = 0; same && q < o.n_postprocess; ++q)
        same = ctx->pp_desc.kind[q] == o.pp_kind[q] && ctx->pp_desc.select[q] == o.pp_select[q];
      if (!same)
        throw HipError(RYUJIN_ERR_ARG, "output_extract: the postprocessor was configured anew since output_configure");
      if (!ctx->pp_computed)
        throw HipError(RYUJIN_ERR_ARG, "output_extract: a postprocessed quantity before postprocess_compute");
    }
    dispatch_equation(ctx->params.equation, ctx->dim, [&](auto tag) {
      ctx->template output_extract<typename decltype(tag)::type>(o, h_state, levelsets != 0,
                                                                 precision == RYUJIN_OUT_FLOAT64, out);
      return 0;
    });
    return RYUJIN_OK;
  });
}

} /* extern "C" */
