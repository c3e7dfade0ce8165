/*
 * ryujin_hip.h -- C ABI of the MI355X-native hyperbolic update.
 *
 * This is the drop-in boundary for ONE hot path of conservation-laws/ryujin:
 * HyperbolicModule::prepare_state_vector() + HyperbolicModule::step<stages>()
 * (reference: source/hyperbolic_module.h:110-278,
 *  source/hyperbolic_module.template.h:96-193,234-1211).
 *
 * The reference has no FFI layer; its boundary is the C++ class template
 * ryujin::HyperbolicModule<Description,dim,Number>. A maintainer binds this
 * header from a thin C++ shim with the same member signatures (shown in
 * INTEGRATION.md, shipped as ryujin_amd/csrc/hyperbolic_module_shim.hpp).
 *
 * Conventions
 *  - plain C, no torch / HIP types in any signature;
 *  - every function returns an int status (never throws across the ABI);
 *  - all arrays are HOST pointers in the reference's own layouts (cited per
 *    field); the library converts them once to its device layout in create();
 *  - state vectors live in device memory behind integer handles; the caller
 *    moves data explicitly with state_upload()/state_download().
 */
#ifndef RYUJIN_HIP_H
#define RYUJIN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------- */
#define RYUJIN_OK 0
/* invariant-domain violation with id_violation_strategy == warn
 * (hyperbolic_module.template.h:1198-1202: n_warnings_++) */
#define RYUJIN_WARN 1
/* ... with id_violation_strategy == raise_exception; the C++ shim converts
 * this into `throw Restart()` (hyperbolic_module.template.h:1203-1205) */
#define RYUJIN_RESTART 2
/* tau_max is NaN/inf/<=0 (AssertThrow at hyperbolic_module.template.h:573) */
#define RYUJIN_ERR_TAU (-1)
#define RYUJIN_ERR_ARG (-2)
#define RYUJIN_ERR_HIP (-3)
#define RYUJIN_ERR_COMM (-4)
#define RYUJIN_ERR_UNSUPPORTED (-5)

/* ---- enums -------------------------------------------------------------- */
/* Description (source/<eq>/description.h) */
enum {
  RYUJIN_EQ_EULER = 0,
  RYUJIN_EQ_SHALLOW_WATER = 1,
  RYUJIN_EQ_EULER_AEOS = 2,
  RYUJIN_EQ_SCALAR_CONSERVATION = 3
};

/* FluxLibrary (source/scalar_conservation/flux_library.h). "function" takes a muparser expression in u in the
 * reference, with the central-difference gradient of dealii::FunctionParser (flux_function.h:80-84). Here it comes
 * twice: RYUJIN_FLUX_POLYNOMIAL, its polynomial subset sum_n c_n u^n per direction in closed form, and
 * RYUJIN_FLUX_FUNCTION, any expression of the grammar table under "The function state" below in the single variable
 * u -- THAT TABLE IS THE CONTRACT here too --, evaluated by the library's interpreter on the device
 * (ryujin_hip_flux_configure_function below). Both form the gradient as (f(u + delta) - f(u - delta)) / (2 * delta). */
enum { RYUJIN_FLUX_BURGERS = 0, RYUJIN_FLUX_KPP = 1, RYUJIN_FLUX_POLYNOMIAL = 2, RYUJIN_FLUX_FUNCTION = 3 };

/* EquationOfStateLibrary (source/euler_aeos/equation_of_state_library.h): the four closed-form members, and
 * "function" (muparser in the reference): four expressions of the grammar table under "The function state" below,
 * evaluated by the library's interpreter on the device (ryujin_hip_eos_configure_function below). "sesame"
 * (tabulated, needs EOSPAC) is host-library bound and not offered. */
enum {
  RYUJIN_EOS_POLYTROPIC_GAS = 0,             /* equation_of_state_polytropic_gas.h */
  RYUJIN_EOS_NOBLE_ABEL_STIFFENED_GAS = 1,   /* equation_of_state_noble_abel_stiffened_gas.h */
  RYUJIN_EOS_VAN_DER_WAALS = 2,              /* equation_of_state_van_der_waals.h */
  RYUJIN_EOS_JONES_WILKINS_LEE = 3,          /* equation_of_state_jones_wilkins_lee.h */
  RYUJIN_EOS_FUNCTION = 4                    /* equation_of_state_function.h */
};

/* ryujin::Boundary (source/discretization.h:28-112) */
enum {
  RYUJIN_BC_DO_NOTHING = 0,
  RYUJIN_BC_PERIODIC = 1,
  RYUJIN_BC_SLIP = 2,
  RYUJIN_BC_NO_SLIP = 3,
  RYUJIN_BC_DIRICHLET = 4,
  RYUJIN_BC_DYNAMIC = 5,
  RYUJIN_BC_DIRICHLET_MOMENTUM = 6
};

/* IDViolationStrategy (source/hyperbolic_module.h:32-47) */
enum { RYUJIN_IDV_WARN = 0, RYUJIN_IDV_RAISE_EXCEPTION = 1 };

/* ---- run-time parameters ------------------------------------------------ */
/*
 * Everything the reference keeps in ParameterAcceptor subsections that the
 * hot path reads. Defaults (ryujin_hip_default_params) are the reference's.
 */
typedef struct ryujin_hip_params {
  int equation; /* RYUJIN_EQ_* */
  int dim;      /* 1, 2, 3 */

  /* "B - Equation" Euler: source/euler/hyperbolic_system.h:665-699 */
  double gamma;                          /* 7/5 */
  double reference_density;              /* 1 */
  double vacuum_state_relaxation_small;  /* 1e2 */
  double vacuum_state_relaxation_large;  /* 1e4 */

  /* "B - Equation" shallow water: source/shallow_water/hyperbolic_system.h:643-673 */
  double gravity;                        /* 9.81 */
  double manning_friction_coefficient;   /* 0 */
  double reference_water_depth;          /* 1 */
  double dry_state_relaxation_factor;    /* 0.2 */
  double dry_state_relaxation_small;     /* 1e2 */
  double dry_state_relaxation_large;     /* 1e4 */

  /* HyperbolicModule: hyperbolic_module.template.h:36,45 */
  double cfl;                /* 0.2 until the TimeIntegrator sets it */
  int id_violation_strategy; /* RYUJIN_IDV_WARN */

  /* "/indicator": source/euler/indicator.h:28 */
  double indicator_evc_factor; /* 1 */

  /* "/limiter": source/euler/limiter.h:26-49, shallow_water/limiter.h:27-59 */
  int limiter_iterations;             /* 2, must be in [0,2] */
  double limiter_newton_tolerance;    /* 1e-10 */
  int limiter_newton_max_iterations;  /* 2 */
  double limiter_relaxation_factor;   /* 1 */
  int limiter_limit_on_kinetic_energy;  /* SW: 0 */
  int limiter_limit_on_square_velocity; /* SW: 1 */

  /* "/riemann solver": source/euler/riemann_solver.h:27-38 */
  int riemann_newton_max_iterations; /* 0 */
  double riemann_newton_tolerance;   /* 1e-10 */

  /* "B - Equation" Euler with arbitrary equation of state (RYUJIN_EQ_EULER_AEOS):
   * source/euler_aeos/hyperbolic_system.h:766-812; `gamma`, `reference_density`,
   * `vacuum_state_relaxation_*` above are shared with Euler */
  int eos;                    /* RYUJIN_EOS_*: "equation of state", polytropic gas */
  int compute_strict_bounds;  /* 1 */
  double eos_covolume_b;      /* NASG, van der Waals: "covolume b", 0 */
  double eos_q;               /* NASG: "reference specific internal energy", 0 */
  double eos_pinf;            /* NASG: "reference pressure", 0 */
  double eos_vdw_a;           /* van der Waals: "vdw a", 0 */
  double eos_gas_constant_R;  /* 287.052874 (van der Waals: 0.4); only temperature() uses it */
  /* Jones-Wilkins-Lee (equation_of_state_jones_wilkins_lee.h:38-66) */
  double jwl_A, jwl_B, jwl_R1, jwl_R2, jwl_omega, jwl_rho_0, jwl_q_0, jwl_cv;

  /* "B - Equation" scalar conservation (RYUJIN_EQ_SCALAR_CONSERVATION):
   * source/scalar_conservation/hyperbolic_system.h:510-540 and "/riemann solver" riemann_solver.h:26-55 */
  int sc_flux;                                /* RYUJIN_FLUX_*: burgers */
  double sc_flux_polynomial[3][4];            /* RYUJIN_FLUX_POLYNOMIAL: c_0..c_3 per direction */
  double sc_derivative_approximation_delta;   /* "function" (POLYNOMIAL and FUNCTION): 1e-10 */
  int sc_use_greedy_wavespeed;                /* 0 */
  int sc_use_averaged_entropy;                /* 0 */
  int sc_random_entropies;                    /* 0; > 0 is not reproducible in the reference: rejected */

  /* Run-time switches of the library itself (no ParameterAcceptor counterpart; all default to 0).
   * system_scope_events: the events that tie the compute stream and the exchange stream of ONE device are
   *   created without the system-scope fence by default (the RCCL kernels carry their own system-scope
   *   semantics); nonzero selects plain hipEventDisableTiming events -- the conservative choice, selectable
   *   without a rebuild should a multi-GPU run ever show stale ghost data (bench.py --gpus N runs both and
   *   compares bitwise before it times anything).
   * debug_*: test hooks that select code branches the mesh would otherwise select (results are identical):
   *   debug_join_exchanges != 0: every sweep joins the ghost exchanges (the choreography of a non-symmetric
   *   stencil); debug_bc_fold_max_slices: boundary conditions ride on the pre-pass kernel up to n slices of
   *   64 rows (0 = default 4096, < 0 = always a launch of their own); debug_no_small_mesh_split != 0: meshes
   *   that do not fill the device run the same step-5/6 kernels as large ones; debug_pij_storage: the matrix
   *   P_ij of an update without stage vectors is stored only where steps 6 and 7 read it (0, the default): up to
   *   two dimensions per (slice, column) tile of 64 entries -- where one of the tile's own l_ij comes out limited
   *   or step 6 read the tile in one of the last updates; step 6 forms the few that are missing --, in 3-D per
   *   64-row slice while few slices hold a limited pair (where the slice held one in the previous update or one of
   *   its own l_ij comes out limited; the rest completed by the repair launch of step 6) and everywhere after
   *   that. 1: always per slice and no slice predicted limited (every stored slice goes through the trigger in
   *   step 5 or the repair launch of step 6); 2: per tile and no tile predicted (every tile the neighbour's l_ji
   *   limits is formed by step 6; per slice as 1 in 3-D); < 0: always stored everywhere. Other values are refused
   *   with RYUJIN_ERR_ARG. */
  int system_scope_events;
  int debug_join_exchanges;
  int debug_bc_fold_max_slices;
  int debug_no_small_mesh_split;
  int debug_pij_storage;
  /* != 0: the reference's EXPENSIVE_BOUNDS_CHECK build (CMakeLists.txt / compile_time_options.h.in:13-16) as a
   * run-time option, for every Description: View::is_admissible() on every new state after steps 4, 6 and 7
   * (hyperbolic_module.template.h:851-855,1121-1126), the limiter's checked control flow -- its additional
   * high-order density and entropy checks (limiter.template.h:110-134,244-252,291-322) -- and the second limiter
   * pass's `success` counted (:1155-1161): any of them raises the restart flag. Evaluated by separate kernels
   * between the sweeps (P_ij is stored in full then); the l_ij themselves are the same in both control flows.
   * (limiter.template.h of euler/, euler_aeos/, shallow_water/ and scalar_conservation/; is_admissible() of the
   * Description's view: trivially true for a scalar equation.) */
  int debug_expensive_bounds_check;
  /* The tile map: column indices and transposed positions of structured 64-row tiles come from a 16-byte descriptor
   * per tile instead of the explicit index arrays (ryujin_amd/csrc/host_layout.hpp, TileDesc; the 1-D / 2-D sweeps 3,
   * 5, 6, 7), and step 5 takes the node data of runs of consecutive neighbours from a neighbouring lane instead of
   * gathering it (TileDesc::chain, every dimension). 0: on (default); < 0: off -- every sweep reads the explicit
   * arrays and gathers every neighbour, as for an unstructured mesh. Results are identical. */
  int debug_tile_map;
  /* Stacked blocks: the four waves of a workgroup take 64-row slices that are one lattice row (2-D) / lattice plane
   * (3-D) of a structured mesh apart instead of four consecutive ones, so that their vertical neighbour rows are
   * served by one L2 (ryujin_amd/csrc/kernels_euler.hpp, row_context()). 0: chosen from the mesh (or off, see
   * DESIGN.md section 3); > 0: that many slices; < 0: off. Results are identical: every slice is processed by exactly
   * one wave either way. */
  int debug_band_stride;
  /* XCD-local block ranges: the hardware deals the workgroups of a launch out to the eight XCDs round robin (block b
   * runs on XCD b % 8 -- observed, relied on for speed only), so that the rows one L2 serves are scattered over the
   * whole mesh and every L2 fetches every node's data. With debug_xcd_chunk = C > 0 the blocks of a launch are
   * renumbered in chunks of 8 C: inside a chunk XCD x takes the C consecutive blocks [x C, (x + 1) C) -- each L2
   * then serves a contiguous range of 4 C slices at a time, and the eight XCDs still advance through the mesh
   * together, chunk by chunk (one contiguous eighth of the mesh per XCD would put a shock on one XCD).
   * 0: chosen by the library; < 0: off. Results are identical: every slice is processed by
   * exactly one wave either way (ryujin_amd/csrc/kernels_euler.hpp, row_context()). */
  int debug_xcd_chunk;
  /* Stencil classes: on a uniform structured patch the 64 rows of a SELL-64 slice hold, column by column, the same
   * c_ij, the same m_ij and the same column offset j - i. create() finds those slices by exact bit comparison and
   * keeps one table entry per class of slices and column (ryujin_amd/csrc/host_layout.hpp); the 1-D / 2-D sweeps
   * that gain from it (steps 2 and 4) take c_ij and the column offset of such a slice from the table with scalar loads
   * instead of streaming 64 copies of them (m_ij is part of the key but read by no kernel). 0: on where it pays (default); < 0: off -- no table is built and
   * every sweep streams the explicit arrays, as for an unstructured mesh. Results are identical: the same bits reach
   * the same operations. Euler's step 2 in 1-D / 2-D also reads |c_ij| and 1 / |c_ij| of such a slice from a second
   * table, computed on the host by the operations the kernel would use; 1: the classes without that table (to
   * measure it alone). Values above 1 are refused. */
  int debug_stencil_classes;
  /* The tile mask from step 6 to step 7: the first of two limiter passes knows, per (64-row slice, column) tile, whether
   * some pair of the tile is limited; the second-pass l'_ij of every other tile are exact zeros. Up to two dimensions
   * its single-launch cached kernel leaves that mask (one word per slice), and the last pass requests the tile
   * descriptor, l'_ij and the transposed l'_ji only of the tiles the mask names (ryujin_amd/csrc/kernels_limiter.hpp,
   * SliceFlags::next_tiles; step_plan.hpp says which updates take it), and the first pass does not store the zeros of
   * the other tiles outside the export slices. 0: on where the plan allows it (default); > 0: the mask, with every
   * zero stored; < 0: off. Results are identical for finite data: min(0, l'_ji) = 0. */
  int debug_next_tile_mask;
} ryujin_hip_params;

/* ---- offline data (input contract) ------------------------------------- */
/*
 * Read-only stencil/geometry data, the output of OfflineData::prepare()
 * (source/offline_data.h:121-264), in the reference's local numbering
 *    [0,n_export) c [0,n_internal) c [0,n_owned) c [0,n_relevant)
 * (source/offline_data.template.h:210-272) and in the SparsityPatternSIMD
 * storage scheme (source/sparse_matrix_simd.h:311-350,403-418):
 *   rows [0,n_internal): groups of simd_length rows of equal length,
 *     entry (row,col_idx,comp) at
 *       data[(row_starts[row/sl] + col_idx*sl)*n_comp + comp*sl + row%sl]
 *     column index at columns[row_starts[row/sl] + col_idx*sl + row%sl];
 *     row_starts has one entry per group, i.e. indices 0..n_internal/sl;
 *   rows [n_internal,n_relevant): plain CSR,
 *       data[(row_starts[row] + col_idx)*n_comp + comp],
 *     where row_starts is indexed by the row itself (the reference re-bases
 *     row_starts[n_internal] := row_starts[n_internal/sl],
 *     sparse_matrix_simd.template.h:127).
 *   row_starts therefore has n_relevant+1 entries of which only
 *   [0, n_internal/sl] and [n_internal, n_relevant] are meaningful.
 *   simd_length == 1 (or n_internal == 0) is plain CSR.
 * Column 0 of every row is the diagonal, the rest ascend by local index
 * (deal.II square SparsityPattern; relied on at
 * hyperbolic_module.template.h:394-396). Ghost rows [n_owned,n_relevant)
 * hold the diagonal and those entries whose transpose is locally owned
 * (sparse_matrix_simd.template.h:61-74).
 */
typedef struct ryujin_hip_offline {
  uint32_t n_export, n_internal, n_owned, n_relevant;
  uint32_t simd_length;
  const uint64_t *row_starts; /* [n_relevant+1], see above */
  const uint32_t *columns;    /* [nnz] */
  const double *cij;          /* [nnz*dim]  c_ij = int phi_i grad phi_j  (offline_data.template.h:566-576) */
  const double *mij;          /* [nnz]      m_ij = int phi_i phi_j */
  const double *mi;           /* [n_relevant] lumped mass  (offline_data.template.h:790-802) */
  const double *mi_inv;       /* [n_relevant] */
  double measure_of_omega;

  /* boundary_map() (offline_data.h:66-72), SoA, in application order */
  uint32_t n_bdry;
  const uint32_t *b_i;      /* [n_bdry] local index (owned) */
  const double *b_normal;   /* [n_bdry*dim] unit normal */
  const uint8_t *b_id;      /* [n_bdry] RYUJIN_BC_* */

  /* coupling_boundary_pairs() (offline_data.h:74-82) */
  uint32_t n_pairs;
  const uint32_t *p_i, *p_col, *p_j; /* [n_pairs] each */

  /* initial_precomputed (shallow water bathymetry Z_i); NULL for Euler.
   * hyperbolic_module.template.h:84-85 */
  const double *initial_precomputed; /* [n_relevant * n_initial_precomputed] */

  /*
   * Exchange pattern (all zero / NULL for a single rank). Neighbour ranks in
   * ascending order. Vector exchange = dealii Partitioner semantics
   * (ghost range sorted by owner, receive in place):
   *   send to nbr p the owned entries send_idx[send_off[p]..send_off[p+1]),
   *   receive from nbr p into ghost rows [recv_off[p], recv_off[p+1])
   *   (recv_off[0] == n_owned, recv_off[n_nbr] == n_relevant).
   * Matrix ghost-row exchange (sparse_matrix_simd.h:649-763):
   *   send to nbr p the entries (row_send_row[e], row_send_col[e]),
   *   e in [row_send_off[p], row_send_off[p+1]); received values fill the
   *   ghost rows of that neighbour contiguously in storage order.
   */
  int n_nbr;
  const int *nbr_rank;       /* [n_nbr] */
  const uint32_t *send_off;  /* [n_nbr+1] */
  const uint32_t *send_idx;  /* [send_off[n_nbr]] */
  const uint32_t *recv_off;  /* [n_nbr+1] */
  const uint32_t *row_send_off; /* [n_nbr+1] */
  const uint32_t *row_send_row; /* [row_send_off[n_nbr]] */
  const uint32_t *row_send_col; /* [row_send_off[n_nbr]] */

  /*
   * Discontinuous finite element ansatz (Discretization::have_discontinuous_ansatz(), SURVEY.md
   * section 8 f-4). When nonzero the step uses the incidence matrix in the high-order viscosity
   * (hyperbolic_module.template.h:733-737), the full block-diagonal inverse mass matrix instead of the
   * Neumann series (:976-986) and extends the limiter bounds over the stencil (:938-948).
   * Both matrices in the storage scheme of mij. Any number of ranks (the limiter bounds are exchanged,
   * :601-613); Euler, EulerAEOS and shallow water. Scalar conservation is refused with RYUJIN_ERR_UNSUPPORTED:
   * the reference's scalar Riemann solver is 0/0 on the structural zeros of a dG stencil (n_ij = c_ij / |c_ij|
   * with c_ij = 0; scalar_conservation/riemann_solver.template.h:63,95-96), tests/test_dg_q1.py.
   */
  int discontinuous_ansatz;
  const double *incidence;           /* [nnz] OfflineData::incidence_matrix() */
  const double *mass_matrix_inverse; /* [nnz] OfflineData::mass_matrix_inverse() */
} ryujin_hip_offline;

typedef struct ryujin_hip_ctx ryujin_hip_ctx; /* opaque; one per (rank, GPU) */

/* ---- communicator (RCCL over xGMI) -------------------------------------- */
/*
 * One process per GPU. Rank 0 calls comm_unique_id(), the caller broadcasts
 * the 128 bytes by whatever means it has (MPI_Bcast in ryujin, a
 * torch.distributed broadcast in bench.py), every rank calls comm_init().
 * Replaces the reference's MPI calls listed in SURVEY.md section 2.2.
 */
#define RYUJIN_HIP_UNIQUE_ID_BYTES 128
typedef struct ryujin_hip_comm ryujin_hip_comm;
int ryujin_hip_comm_unique_id(char id[RYUJIN_HIP_UNIQUE_ID_BYTES]);
int ryujin_hip_comm_init(ryujin_hip_comm **comm, const char id[RYUJIN_HIP_UNIQUE_ID_BYTES],
                         int rank, int n_ranks, int device);
/* number of HIP devices visible to this process (a host application picks rank % count) */
int ryujin_hip_device_count(int *n_devices);
/* Test facility: n_ranks communicators of ONE process (one host thread per rank, all on `device`)
 * that exchange ghost data with device-to-device copies instead of RCCL. comms: [n_ranks]. */
int ryujin_hip_comm_init_local(ryujin_hip_comm **comms, int n_ranks, int device);
/* Measurement facility: a communicator for ONE rank of an n_ranks slab partition that is run alone; every
 * neighbour is replaced by the rank itself (what it packs for the opposite neighbour arrives in its ghost range,
 * i.e. a periodic channel). All launches, pack kernels, copies, events and reductions of a middle rank of a real
 * run, without the network: what the multi-rank choreography costs per rank (scripts/overhead_loopback.py). The
 * offline data must have two neighbours with equally sized send / ghost ranges (uniform cross-section). */
int ryujin_hip_comm_init_loopback(ryujin_hip_comm **comm, int rank, int n_ranks, int device);
void ryujin_hip_comm_destroy(ryujin_hip_comm *comm);
/* What the communicator itself reports: rank / n_ranks as passed to comm_init and -- RCCL communicators only,
 * -1 otherwise -- ncclCommUserRank / ncclCommCount / ncclCommCuDevice as RCCL sees them (bench.py prints them
 * so that "RCCL saw N ranks" can be read off the JSON line). Any pointer may be NULL. */
int ryujin_hip_comm_info(const ryujin_hip_comm *comm, int *rank, int *n_ranks, int *rccl_rank,
                         int *rccl_count, int *rccl_device);

/* ---- lifecycle ----------------------------------------------------------- */
void ryujin_hip_default_params(ryujin_hip_params *params, int equation, int dim);

/* HyperbolicModule ctor + prepare() (hyperbolic_module.template.h:28-86).
 * `comm` may be NULL for a single rank. `device` is the HIP device ordinal. The library reads no
 * environment variables; its run-time switches are the last four fields of ryujin_hip_params. */
int ryujin_hip_create(ryujin_hip_ctx **ctx, const ryujin_hip_offline *offline,
                      const ryujin_hip_params *params, ryujin_hip_comm *comm, int device);
/* The exchange pattern of a context and what it has done so far: neighbour ranks (at most max_nbr written),
 * number of point-to-point ghost exchanges (vector or matrix; one grouped send/recv set per neighbour each)
 * and of scalar all-reduces enqueued since create(). Any pointer may be NULL. */
int ryujin_hip_exchange_info(ryujin_hip_ctx *ctx, int *n_nbr, int *nbr_rank, int max_nbr,
                             unsigned long long *n_exchanges, unsigned long long *n_allreduces);
void ryujin_hip_destroy(ryujin_hip_ctx *ctx);

/* ---- state vectors (StateVector = U + precomputed, source/state_vector.h:47-51) */
int ryujin_hip_state_alloc(ryujin_hip_ctx *ctx, int *handle);
int ryujin_hip_state_free(ryujin_hip_ctx *ctx, int handle);
/* U_aos: MultiComponentVector layout U[i*k + d], i < n_relevant
 * (source/multicomponent_vector.h:55-183) */
int ryujin_hip_state_upload(ryujin_hip_ctx *ctx, int handle, const double *U_aos);
int ryujin_hip_state_download(ryujin_hip_ctx *ctx, int handle, double *U_aos);
int ryujin_hip_state_download_precomputed(ryujin_hip_ctx *ctx, int handle, double *prec_aos);

/* ---- host-mirrored state vectors: the unmodified reference caller ----------------------------------------
 * The reference's StateVector lives on the HOST and is read and written there by its caller between the calls
 * into HyperbolicModule (TimeIntegrator: sadd(), swap(); time_integrator.template.h:18-25,300-328). An adapter
 * that keeps such a caller unchanged mirrors every call over PCIe; these entry points move only what the
 * contract of the call can have changed, straight between the caller's arrays and HBM:
 *   host_register(ptr, bytes)       pin the caller's array IN PLACE (hipHostRegister): uploads and downloads of
 *                                   that memory are then direct DMA instead of a pageable staged copy.
 *                                   Registrations belong to the context and end with it (or with
 *                                   host_unregister). THE CALLER GUARANTEES that the memory stays allocated while
 *                                   it is registered: a range that is freed and handed out again by the allocator
 *                                   is not covered by the old pinning (registering the same address again renews
 *                                   it). RYUJIN_WARN (not an error): the pages could not be pinned; transfers
 *                                   still work, staged by the runtime.
 *   state_download_owned(h, U)      rows [0, n_owned) only: what step() is allowed to write
 *                                   (hyperbolic_module.h:207-213); U_aos has room for n_relevant rows, the
 *                                   ghost rows are left untouched.
 *   state_download_prepared(h, U)   the rows prepare_state_vector() can have changed in a vector the caller
 *                                   has just uploaded: the boundary_map rows (boundary conditions,
 *                                   hyperbolic_module.template.h:119-147) and the ghost range (:152-159).
 *                                   Everything else in U_aos is left untouched. */
int ryujin_hip_host_register(ryujin_hip_ctx *ctx, const void *ptr, size_t bytes);
int ryujin_hip_host_unregister(ryujin_hip_ctx *ctx, const void *ptr);
int ryujin_hip_state_download_owned(ryujin_hip_ctx *ctx, int handle, double *U_aos);
int ryujin_hip_state_download_prepared(ryujin_hip_ctx *ctx, int handle, double *U_aos);

/* ---- the hot path -------------------------------------------------------- */
/*
 * prepare_state_vector(state_vector, t) (hyperbolic_module.template.h:96-193).
 * dirichlet_aos: [n_bdry*k] the value of initial_values_->initial_state(
 * position, t) for every boundary_map entry (only read for dirichlet /
 * dynamic / dirichlet_momentum ids); may be NULL if none of those ids occur
 * or to re-use the data passed in the previous call.
 */
int ryujin_hip_prepare_state_vector(ryujin_hip_ctx *ctx, int handle, double t,
                                    const double *dirichlet_aos);

/*
 * step<stages>(old, stage_state_vectors, stage_weights, new, tau, tau_max)
 * (hyperbolic_module.template.h:234-1211). stages in [0,4]. Writes only
 * new.U on [0,n_owned). *tau_out = the tau actually used. Returns RYUJIN_OK,
 * RYUJIN_WARN, RYUJIN_RESTART or RYUJIN_ERR_TAU; counters as the reference.
 */
int ryujin_hip_step(ryujin_hip_ctx *ctx, int h_old, int stages, const int *h_stage,
                    const double *stage_weights, int h_new, double tau_in,
                    double tau_max_in, double *tau_out);

/* TimeIntegrator helpers that touch the device-resident vectors:
 * sadd(dst,s,b,src): dst.U = s*dst.U + b*src.U (time_integrator.template.h:18-25) */
int ryujin_hip_sadd(ryujin_hip_ctx *ctx, int h_dst, double s, double b, int h_src);

/* Device-resident TimeIntegrator::step (source/time_integrator.template.h:207-403) for the explicit
 * schemes built from prepare_state_vector + step<s> + sadd. One host synchronisation per RK step: the
 * tau of the first stage and the restart flags of all stages stay on the device. h_state names the
 * solution before and after the call (state_vector.swap(temp) is done on the handles); h_tmp are three
 * scratch state vectors (temp_[0..2]). dirichlet_aos as in prepare_state_vector (time independent;
 * ryujin_hip_time_step_fn below takes time-dependent Dirichlet data). tau_max = t_final - t. With
 * RYUJIN_CFL_RECOVERY_BANG_BANG the reference's bang-bang control (:250-274) is applied internally.
 * *tau_out = the time increment of the whole RK step (3 tau for ERK33). */
enum {
  RYUJIN_SCHEME_SSPRK_22 = 0,
  RYUJIN_SCHEME_SSPRK_33 = 1,
  RYUJIN_SCHEME_ERK_11 = 2,
  RYUJIN_SCHEME_ERK_22 = 3,
  RYUJIN_SCHEME_ERK_33 = 4,
  RYUJIN_SCHEME_ERK_43 = 5, /* step_erk_43, :405-440: 4 temporaries */
  RYUJIN_SCHEME_ERK_54 = 6  /* step_erk_54, :443-510: 5 temporaries */
};
enum { RYUJIN_CFL_RECOVERY_NONE = 0, RYUJIN_CFL_RECOVERY_BANG_BANG = 1 };
int ryujin_hip_time_step(ryujin_hip_ctx *ctx, int scheme, int h_state, const int h_tmp[3],
                         const double *dirichlet_aos, double tau_max, int cfl_recovery, double cfl_min,
                         double cfl_max, double *tau_out);
/* the same with n_tmp temporaries (ERK43 needs 4, ERK54 needs 5; TimeIntegrator::prepare :163-205) */
int ryujin_hip_time_step_n(ryujin_hip_ctx *ctx, int scheme, int h_state, int n_tmp, const int *h_tmp,
                           const double *dirichlet_aos, double tau_max, int cfl_recovery,
                           double cfl_min, double cfl_max, double *tau_out);

/* The same with TIME-DEPENDENT Dirichlet data: the reference evaluates initial_state(position, t + c_s tau) for
 * every stage (hyperbolic_module.template.h:137-139 called with the stage times of
 * time_integrator.template.h:279-510). `dirichlet_fn(user, time, values)` fills values[n_bdry * k] (the layout of
 * prepare_state_vector's dirichlet_aos; entries whose boundary id does not read Dirichlet data may be left
 * untouched) and is called once per stage from the calling thread: for the first stage at `t` before anything is
 * enqueued, for the later stages as soon as tau exists on the host -- behind step 3 of the first stage, while its
 * remaining sweeps run. NULL: no boundary id reads Dirichlet data, or the data of an earlier call is kept. */
typedef void (*ryujin_hip_dirichlet_fn)(void *user, double time, double *dirichlet_aos);
int ryujin_hip_time_step_fn(ryujin_hip_ctx *ctx, int scheme, int h_state, int n_tmp, const int *h_tmp, double t,
                            ryujin_hip_dirichlet_fn dirichlet_fn, void *user, double tau_max, int cfl_recovery,
                            double cfl_min, double cfl_max, double *tau_out);

/* Conservation monitor on the device (the interior integrals of ryujin::Quantities,
 * source/quantities.template.h): out[q] = sum over ALL ranks of
 * sum_{i < n_owned} m_i U_i[q], q < k. Fixed summation order: bitwise reproducible for a given
 * partition. Collective when the context has a communicator. */
int ryujin_hip_state_integrals(ryujin_hip_ctx *ctx, int handle, double *out /* [k] */);

/* ---- accessors of HyperbolicModule (hyperbolic_module.h:225-278) --------- */
int ryujin_hip_set_cfl(ryujin_hip_ctx *ctx, double cfl);
int ryujin_hip_get_cfl(ryujin_hip_ctx *ctx, double *cfl);
int ryujin_hip_set_id_violation_strategy(ryujin_hip_ctx *ctx, int strategy);
int ryujin_hip_get_alpha(ryujin_hip_ctx *ctx, double *alpha /* [n_relevant] */);
int ryujin_hip_get_counters(ryujin_hip_ctx *ctx, unsigned *n_restarts, unsigned *n_warnings);
/* What the data-dependent limiter sweeps saw between the two latest host synchronisations: the fraction of
 * (sampled) 64-row slices in which the first high-order sweep found a limited pair; how the latest step kept the
 * matrix P_ij (hyperbolic_module.template.h:795-846): 1 stored everywhere, 2 stored per slice -- only where steps
 * 6 and 7 read it --, 3 stored per (slice, column) tile (up to two dimensions); and the fraction
 * of slices (tiles) it was stored in. The results are the same bit for bit whatever is
 * stored -- FOR A GIVEN LAYOUT: which rows share a 64-row slice decides, through wave-uniform
 * masks, which of two roundings of the same sum a row's high-order update takes (V_i - sum (1 - l) lambda P over the
 * limited tiles, or the reference's U_low + sum l lambda P where every tile of the row is limited), so another
 * numbering, partition or rank count reproduces a run to round-off (1e-11 on U per update, the stated contract), not
 * to the bit. Diagnostics; any pointer may be NULL. */
int ryujin_hip_limiter_statistics(ryujin_hip_ctx *ctx, double *limited_slice_fraction, int *pij_stored,
                                  double *stored_slice_fraction);
/* The tile map of the context (ryujin_amd/csrc/host_layout.hpp, TileDesc): number of 64-entry tiles of the owned rows
 * and how many of them are served by a 16-byte descriptor instead of the explicit index arrays (0 where the sweeps
 * keep streaming the indices: 3-D, debug_tile_map < 0). bench.py takes the index bytes the sweeps no longer read out of their own
 * compulsory bytes with it. Any pointer may be NULL. */
int ryujin_hip_layout_info(ryujin_hip_ctx *ctx, unsigned long long *n_tiles, unsigned long long *n_regular_tiles);
/* Chained gathers (ryujin_amd/csrc/host_layout.hpp, TileDesc::chain): the number of tiles whose node data step 5 takes
 * from the previous column of the slice or from the slice's own rows, one lane over, instead of gathering it, and the
 * number of matrix entries (lanes of those tiles) that are served that way -- the others fetch their node as ever. On a
 * lattice-numbered mesh six of the eight off-diagonal columns of a 2-D Q1 row, 18 of 26 in 3-D; 0 on a mesh without
 * such runs and with debug_tile_map < 0. The results do not depend on it (the same values reach the same operations).
 * Diagnostics; any pointer may be NULL. */
int ryujin_hip_chain_info(ryujin_hip_ctx *ctx, unsigned long long *n_chained_tiles,
                          unsigned long long *n_chained_entries);
/* Stencil classes (ryujin_hip_params::debug_stencil_classes; ryujin_amd/csrc/host_layout.hpp): the number of 64-row
 * slices whose c_ij and column offsets steps 2 and 4 take from the class table, the number of classes in it, and
 * the fraction of the matrix entries of the owned rows (padding included) that lie in such slices. All 0 where there
 * is no table: no uniform slice on the mesh (an unstructured mesh; a partition whose numbering starts with its export
 * rows may have none either), 3-D, debug_stencil_classes < 0. Diagnostics; any pointer may be NULL. */
int ryujin_hip_stencil_class_info(ryujin_hip_ctx *ctx, unsigned long long *n_uniform_slices,
                                  unsigned long long *n_classes, double *uniform_entry_fraction);
/* The tile mask of the latest step (ryujin_hip_params::debug_next_tile_mask): whether its plan handed the mask from
 * step 6 to step 7, the number of off-diagonal (slice, column) tiles of the owned rows, and how many of them the mask
 * named -- the others step 7 did not read. 0 / n_tiles / n_tiles where the plan did not take it. Synchronises and
 * downloads one word per slice. Diagnostics; any pointer may be NULL. */
int ryujin_hip_next_tile_mask_info(ryujin_hip_ctx *ctx, int *active, unsigned long long *n_tiles,
                                   unsigned long long *n_named);
/* Where the latest step stored P_ij per tile (pij_stored == 3): of the (slice, column) tiles between the two latest
 * host synchronisations, the fractions step 5 stored, step 6 read, and step 6 had to form itself because step 5 had
 * not stored them (ryujin_amd/csrc/kernels_limiter_stage0.hpp). 1 / 1 / 0 otherwise. Any pointer may be NULL. */
int ryujin_hip_tile_statistics(ryujin_hip_ctx *ctx, double *stored_fraction, double *read_fraction,
                               double *formed_by_step6_fraction);

/* ---- introspection for parity tests and profiling ------------------------ */
/* Module-owned intermediates of the LAST step() in the reference's logical
 * (row, col_idx) order as plain CSR over owned rows (nnz_owned entries):
 * what: 0 d_ij, 1 l_ij (after the last pass = lij_matrix_), 2 p_ij (k comps),
 *       3 bounds (n_bounds per row), 4 r_i (k per row), 5 lij_next;
 * over ALL locally relevant rows -- the ghost rows / ghost range a rank received included (multi-rank parity
 * tests): 6 d_ij, 7 l_ij, 8 lij_next (plain CSR over n_relevant rows; d_ij is never exchanged, its ghost rows
 * stay zero as in the reference), 9 r_i (k per row, n_relevant rows) */
int ryujin_hip_debug_fetch(ryujin_hip_ctx *ctx, int what, double *out, size_t n_doubles);
/* Test hook: every off-diagonal slot of the owned rows of a module-owned matrix, padding included, set to `value` (a
 * NaN included). what: 5 lij_next -- the buffer
 * the next update's first high-order pass writes its l'_ij to (under the tile mask it leaves the slots of the unlimited
 * tiles as they are: tests/test_gpu_next_tile_mask.py). */
int ryujin_hip_debug_fill(ryujin_hip_ctx *ctx, int what, double value);
/* Which kernels the LAST step() ran (ryujin_amd/csrc/step_plan.hpp: the plan decided once per update) and what its
 * sweeps of steps 5 and 6 launched, as RYUJIN_DEBUG_PLAN_LENGTH ints in this order:
 *    0 step2 (0 alpha_then_dij, 1 dij_alpha_sc, 2 records, 3 dij_alpha)   1 step2_split   2 fast_riemann
 *    3 diag_width   4 step4_single_walk   5 step4_has_stages   6 step4_friction   7 step4_stores_p   8 dg
 *    9 step5 (0 none, 1 stage0_per_tile, 2 stage0_per_slice, 3 stage0_groups, 4 recompute, 5 pij_lij)
 *   10 step5_groups   11 wide   12 has_V   13 pij_stored (as ryujin_hip_limiter_statistics)
 *   14 tiles_predicted_from_history   15 step6 (0 none, 1 per_slice, 2 cached, 3 high_order)   16 step6_flags
 *   17 step7 (0 none, 1 last_cached, 2 high_order)   18 fuse_precompute   19 checked
 *   20 number of launches of the step-5 sweep, 21 of the step-6 sweep (one on one rank; on several the export part,
 *      then the interior part; an empty part is not launched)
 *   22, 23 and 24, 25: per launch of step 5 its number of slices and gridDim.y (the waves that share a slice)
 *   26 - 28 and 29 - 31: per launch of step 6 its number of slices, gridDim.y, and whether the four waves of a block
 *      shared a slice (per slice -- the three kernels light, repair, heavy -- counts as one launch)
 * The per-launch values are recorded where the kernels are launched, not evaluated again. Host values only: no
 * synchronisation, no device work. Writes min(n, RYUJIN_DEBUG_PLAN_LENGTH) ints, returns RYUJIN_DEBUG_PLAN_LENGTH
 * (a negative status on error). All zero before the first step(). */
#define RYUJIN_DEBUG_PLAN_LENGTH 32
int ryujin_hip_debug_plan(ryujin_hip_ctx *ctx, int *out, int n);
/* device time [ms] of the sweeps of the last step (hipEvent pairs; ms[n] = the reference's Scope timer
 * "time step [H] n", n = 2..7; ms[1] unused (step 1 is a separate call); ms[0] = the indicator kernel
 * alone when step 2 runs as two kernels, else 0); enable = nonzero switches the event recording on. */
int ryujin_hip_set_timers(ryujin_hip_ctx *ctx, int enable);
int ryujin_hip_get_timers(ryujin_hip_ctx *ctx, double ms[8]);
/* sums over all updates since the last reset (also filled by ryujin_hip_time_step) */
int ryujin_hip_get_timers_accum(ryujin_hip_ctx *ctx, double ms[8], unsigned *n_updates, int reset);
/* Block until all device work of this context has finished. */
int ryujin_hip_synchronize(ryujin_hip_ctx *ctx);
/* Record start/stop HIP events on the context's compute stream and read the elapsed ms. */
int ryujin_hip_event_record(ryujin_hip_ctx *ctx, int which /*0 start, 1 stop*/);
int ryujin_hip_event_elapsed_ms(ryujin_hip_ctx *ctx, double *ms);
/* Host-only check of the layout import (no GPU needed): converts `offline` into the device layout
 * (SELL-64 + ghost CSR) and back, and reports the logical (row, col_idx) view over ALL n_relevant
 * rows: ptr [n_relevant+1], col [nnz], transposed [nnz] = logical index of the (j,i) entry.
 * If data != NULL, the n_comp-component matrix `data` (reference layout) is scattered into the
 * device layout and gathered back into out [nnz*n_comp] (AoS per entry). Any pointer may be NULL. */
int ryujin_hip_debug_layout(const ryujin_hip_offline *offline, uint64_t *ptr, uint32_t *col,
                            uint64_t *transposed, const double *data, uint32_t n_comp, double *out);
/* Device addresses of the stencil streams of a context (cols, c_ij, m_ij, d_ij, l_ij, l'_ij, p_ij, idx_t): for
 * the placement study of scripts/placement_probe.py (how the kernel times depend on where the allocator put them). */
int ryujin_hip_debug_addresses(ryujin_hip_ctx *ctx, uint64_t out[8]);
/* Evaluate the device implementation of ryujin::pow (source/simd.template.h:196-272) on n pairs:
 * out[i] = pow(x[i], y[i]). Needs a GPU; used by the parity tests only. */
int ryujin_hip_debug_pow(int device, const double *x, const double *y, double *out, size_t n);
/* Evaluate a device function of the Euler / shallow-water Description on n independent items (needs a GPU;
 * parity tests only): the device code is pinned directly against the baselines of the reference's unit tests.
 *   RYUJIN_DEBUG_EULER_RIEMANN   in: rd_i[4], rd_j[4] = (rho, u, p, a)      out: lambda_max
 *                                (RiemannSolver::compute(rd_i, rd_j), riemann_solver.template.h:406-582;
 *                                 tests/euler/riemann_solver.cc:79-98)
 *   RYUJIN_DEBUG_EULER_LIMIT_1D  in: bounds[3], U[3], P[3] (dim = 1)        out: l, success, took the Newton tail
 *                                (Limiter::limit, limiter.template.h:15-327; tests/euler/limiter.cc:61-139)
 *   RYUJIN_DEBUG_EULER_LIMIT_CHECKED_1D  the same through the EXPENSIVE_BOUNDS_CHECK control flow (the build that
 *                                wrote tests/euler/limiter.output)           out: l, success, 0
 *   RYUJIN_DEBUG_SW_RIEMANN      in: rd_i[3], rd_j[3] = (h, u, a)           out: h_star, lambda_max
 *                                (shallow_water/riemann_solver.template.h:110-251;
 *                                 tests/shallow_water/riemann_solver.cc:75-77)
 *   RYUJIN_DEBUG_EULER_DIJ_2D/3D in: U_i[k], U_j[k], c_ij[dim]              out: d_ij = |c_ij| lambda_max
 *                                (hyperbolic_module.template.h:402-406) */
enum {
  RYUJIN_DEBUG_EULER_RIEMANN = 0,
  RYUJIN_DEBUG_EULER_LIMIT_1D = 1,
  RYUJIN_DEBUG_SW_RIEMANN = 2,
  RYUJIN_DEBUG_EULER_DIJ_2D = 3,
  RYUJIN_DEBUG_EULER_DIJ_3D = 4,
  RYUJIN_DEBUG_EULER_DIJ_RECORDS_2D = 5, /* the same through the per-node Riemann records the sweep uses */
  RYUJIN_DEBUG_EULER_DIJ_RECORDS_3D = 6,
  RYUJIN_DEBUG_SW_DIJ_2D = 7,          /* in: U_i[3], U_j[3], c_ij[2]   out: d_ij (shallow water, dim = 2) */
  RYUJIN_DEBUG_SW_DIJ_RECORDS_2D = 8,  /* the same through the per-node Riemann records the sweep uses */
  /* the production evaluation path of the sweeps -- per-node Riemann records, dij_from_records -- fed with the
   * reference's 1-D Riemann data: in as RYUJIN_DEBUG_EULER_RIEMANN / RYUJIN_DEBUG_SW_RIEMANN, out: lambda_max */
  RYUJIN_DEBUG_EULER_RIEMANN_RECORDS = 9,
  RYUJIN_DEBUG_SW_RIEMANN_RECORDS = 10,
  /* EulerAEOS (params->eos etc. select the equation of state):
   *   RYUJIN_DEBUG_AEOS_RIEMANN  in: rd_i[5], rd_j[5] = (rho, u, p, gamma, a)   out: lambda_max, evaluated through
   *                              the per-node records of the sweep (EulerAeos::dij_from_records with n = 1)
   *                              (euler_aeos/riemann_solver.template.h:443-560; tests/euler_aeos/riemann_solver*.cc)
   *   RYUJIN_DEBUG_AEOS_LIMIT_1D in: bounds[4], U[3], P[3] (dim = 1)            out: l, success, took the Newton tail
   *                              (euler_aeos/limiter.template.h:15-360; tests/euler_aeos/limiter*.cc) */
  RYUJIN_DEBUG_AEOS_RIEMANN = 11,
  RYUJIN_DEBUG_AEOS_LIMIT_1D = 12,
  /* EulerAEOS d_ij from two states (dim = 2; p from the equation of state): in U_i[4], U_j[4], c_ij[2], out d_ij --
   * in the reference's operation order and through the per-node Riemann records the sweep uses */
  RYUJIN_DEBUG_AEOS_DIJ_2D = 13,
  RYUJIN_DEBUG_AEOS_DIJ_RECORDS_2D = 14,
  RYUJIN_DEBUG_EULER_LIMIT_CHECKED_1D = 15,
  /* the limiter as the sweeps compose it, dim = 2: in bounds[3], U[4], P[4]; out l, success, took the Newton tail,
   * t_r behind the density clip, psi_r of the first Newton iteration (as the device evaluates it) */
  RYUJIN_DEBUG_EULER_LIMIT_2D = 16,
  /* The limiter of every other Description and dimension, pair by pair (a kernel of its own, one thread per item):
   * in bounds[NB], U[K], P[K]; out l, success, took the Newton tail -- Euler and EulerAEOS also t_r behind the density
   * clip and psi_r there, as RYUJIN_DEBUG_EULER_LIMIT_2D. Evaluated as the sweeps compose it: limit_fast(), and
   * limit() for the undecided pairs. With params->debug_expensive_bounds_check != 0 these six evaluate limit_checked()
   * instead (the EXPENSIVE_BOUNDS_CHECK control flow: the same l, `success` has more ways to be false; "took the
   * Newton tail" is 0 then).
   *   EULER_LIMIT_3D   NB = 3 (rho_min, rho_max, s_min), K = 5
   *   AEOS_LIMIT_2D/3D NB = 4 (rho_min, rho_max, s_min, gamma_min), K = 4 / 5
   *   SW_LIMIT_1D/2D   NB = 5 (h_min, h_max, h_small, kin_max, v2_max), K = 2 / 3; limiter_limit_on_kinetic_energy and
   *                    limiter_limit_on_square_velocity select the constraints
   *   SCALAR_LIMIT     NB = 2 (u_min, u_max), K = 1 */
  RYUJIN_DEBUG_EULER_LIMIT_3D = 17,
  RYUJIN_DEBUG_AEOS_LIMIT_2D = 18,
  RYUJIN_DEBUG_AEOS_LIMIT_3D = 19,
  RYUJIN_DEBUG_SW_LIMIT_1D = 20,
  RYUJIN_DEBUG_SW_LIMIT_2D = 21,
  RYUJIN_DEBUG_SCALAR_LIMIT = 22
};
int ryujin_hip_debug_function(int device, const ryujin_hip_params *params, int which, const double *in,
                              double *out, size_t n);
/* Host logic of ryujin_hip_time_step, exposed for the CPU test-suite: what the end-of-step flags mean.
 * restart_accum / tau_invalid_accum: 0 = never raised, else 100 - (index of the first RK stage that raised it).
 * Returns RYUJIN_ERR_TAU, RYUJIN_RESTART, RYUJIN_WARN or RYUJIN_OK. Under raise_exception the reference throws
 * Restart at the end of the offending stage (hyperbolic_module.template.h:1194-1207) and never evaluates tau_max
 * of a later stage (:573-576); here all stages are enqueued before the flags are read, so an invalid tau_max of a
 * stage LATER than the first Restart must not turn the recoverable Restart into the fatal error. */
int ryujin_hip_debug_rk_outcome(int restart_accum, int tau_invalid_accum, int id_violation_strategy);
const char *ryujin_hip_last_error(void);
const char *ryujin_hip_version(void);

/* ---- Postprocessor: schlieren and vorticity fields, device resident ------ */
/* Postprocessor::compute() of the reference (source/postprocessor.template.h:108-271, steps 1 - 3) on the state
 * vector behind a handle. For every owned row i with more than one stencil entry and every configured quantity q
 * -- a component of the conserved state U_j, or of to_primitive_state(U_j) of the context's Description
 * (Euler (rho, v, p); EulerAEOS (rho, v, e), e the specific internal energy; shallow water (h, v) with the sharp
 * inverse water depth; scalar conservation u), computed from U itself, whether or not prepare_state_vector has
 * run on that vector:
 *   schlieren  s_i = | sum_j c_ij q_j | / m_i
 *   vorticity  of the dim consecutive components starting at `component`:
 *              dim = 2: w_i = sum_j (c_ij,x q_j,y - c_ij,y q_j,x) / m_i, SIGNED (a counter-clockwise rigid rotation
 *              of angular speed omega gives +2 omega); dim = 3: w_i = | sum_j c_ij x q_j | / m_i; refused in 1-D.
 * Rows of length 1 (constrained DoFs) get 0. ryujin_hip_offline carries no affine constraints, so step 4 of the
 * reference (AffineConstraints::distribute) has no counterpart here.
 * Bounds per quantity over the owned rows of ALL ranks: q_max = max |.| starting from 0, q_min = min |.|; with
 * recompute_bounds = 0 the bounds of the first compute() after configure() are kept for the later ones
 * ("schlieren recompute bounds" of the reference). Normalised value, with eps = DBL_EPSILON, floor = 1e-10:
 *   r = max(0, |v| - q_min - floor) / max(q_max - q_min, eps),   copysign(1 - exp(-beta r), v).
 * compute() is collective over the ranks of the context's communicator (it exchanges the ghost range of the state
 * vector and reduces the bounds); on one rank and over RCCL it is asynchronous on the context's stream.
 * RYUJIN_ERR_ARG: n_quantities outside [1, RYUJIN_PP_MAX_QUANTITIES], an unknown kind, a component outside the
 * state, a vorticity in 1-D or one whose dim components do not fit the state, compute() before configure(),
 * download() / bounds() before compute() or for a quantity that was not configured. */
#define RYUJIN_PP_MAX_QUANTITIES 8
enum { RYUJIN_PP_SCHLIEREN = 0, RYUJIN_PP_VORTICITY = 1 };
typedef struct ryujin_hip_postprocess_quantity {
  int kind;         /* RYUJIN_PP_SCHLIEREN, RYUJIN_PP_VORTICITY */
  int is_primitive; /* 0: component of U, 1: of to_primitive_state(U) */
  int component;    /* index; vorticity: the first of dim consecutive components */
} ryujin_hip_postprocess_quantity;
/* reference defaults: beta = 10, recompute_bounds = 1 */
int ryujin_hip_postprocess_configure(ryujin_hip_ctx *ctx, int n_quantities,
                                     const ryujin_hip_postprocess_quantity *quantities, double beta,
                                     int recompute_bounds);
int ryujin_hip_postprocess_compute(ryujin_hip_ctx *ctx, int state_handle);
/* out [n_owned]: quantity q of the latest compute(); raw != 0: the values before the normalisation */
int ryujin_hip_postprocess_download(ryujin_hip_ctx *ctx, int q, double *out, int raw);
int ryujin_hip_postprocess_bounds(ryujin_hip_ctx *ctx, int q, double *q_max, double *q_min);

/* ---- Quantities: point maps, space and time averages, device resident ---- */
/* Quantities::prepare / accumulate / write_out / clear_statistics of the reference (source/quantities.template.h)
 * on the state vector behind a handle. A MANIFOLD is a list of points of this rank: owned local indices and a
 * positive weight per point. The library evaluates no level sets: the caller selects the points (prepare(),
 * :111-226) and hands over the interior mass m_i (interior maps) or the boundary mass (boundary maps) as weights.
 * Indices need not be sorted and may repeat (boundary_map() is a multimap). Manifold ids count from 0 in the order
 * of the add_manifold calls.
 * The value of a point is (V, V o V), V = to_primitive_state(U_i) of the context's Description (see the
 * Postprocessor block), 2k doubles; `out` arrays are [n_points][2k] in manifold order.
 *   accumulate      acts on every manifold with TIME_AVERAGED or SPACE_AVERAGED (:511-514). The first call after a
 *                   clear (the reference's test: t_old == 0 && t_new == 0) only sets t_old = t - 1, t_new = t; later
 *                   calls add, in this order per point, sum += 0.5 tau old; sum += 0.5 tau new with
 *                   tau = t - t_old, and t_sum += tau. Every call appends one row (t, mean V, mean V o V) to the
 *                   manifold's time series, mean x = sum_p w_p x_p / sum_p w_p over the points of ALL ranks; a
 *                   manifold without a point on any rank gives the reference's 0/0 (NaN). Collective over the
 *                   context's communicator. On one rank and over RCCL it is an enqueue on the context's stream: no
 *                   host synchronisation, no copy to the host (the in-process test transport meets on the host). The
 *                   sums are formed in a fixed order (no floating-point atomics): for a given partition the series
 *                   is reproducible bit for bit.
 *   instantaneous   needs INSTANTANEOUS. Without TIME_/SPACE_AVERAGED it evaluates the given state; with, it returns
 *                   the values of the latest accumulate and fails unless t equals that call's t (:615-619).
 *   time_averaged   out = sum * (1 / t_sum), t_begin = t_new - t_sum, t_end = t_new (:628-645); returns
 *                   RYUJIN_Q_NONE_YET and leaves out, t_begin, t_end untouched while t_sum == 0.
 *   time_series     rows [n_rows][1 + 2k] since the last clear; clear != 0 empties it (:663-665). The series lives on
 *                   the device between calls; reading it is the only call that waits for the stream. rows = NULL
 *                   with capacity_rows = 0 only reports the number of rows.
 *   clear_statistics  t_old = t_new = t_sum = 0, sums zeroed, series emptied (:341-364).
 *   reset           drops all manifolds (prepare()).
 * RYUJIN_ERR_ARG: an index >= n_owned, a non-finite or non-positive weight, options zero or with unknown bits, more
 * than RYUJIN_Q_MAX_MANIFOLDS manifolds, an unknown manifold id, NULL pointers with n_points > 0, instantaneous /
 * time_averaged on a manifold without that option, instantaneous with a stale t, capacity_rows smaller than the
 * number of rows (which *n_rows then reports). */
enum { RYUJIN_Q_INSTANTANEOUS = 1, RYUJIN_Q_TIME_AVERAGED = 2, RYUJIN_Q_SPACE_AVERAGED = 4 };
#define RYUJIN_Q_MAX_MANIFOLDS 16
#define RYUJIN_Q_NONE_YET 3 /* time_averaged: nothing accumulated yet (distinct from RYUJIN_WARN, RYUJIN_RESTART) */
int ryujin_hip_quantities_add_manifold(ryujin_hip_ctx *ctx, uint32_t n_points, const uint32_t *index,
                                       const double *weight, int options, int *manifold_out);
int ryujin_hip_quantities_reset(ryujin_hip_ctx *ctx);
int ryujin_hip_quantities_clear_statistics(ryujin_hip_ctx *ctx);
int ryujin_hip_quantities_accumulate(ryujin_hip_ctx *ctx, int state_handle, double t);
int ryujin_hip_quantities_instantaneous(ryujin_hip_ctx *ctx, int manifold, int state_handle, double t, double *out);
int ryujin_hip_quantities_time_averaged(ryujin_hip_ctx *ctx, int manifold, double *out, double *t_begin,
                                        double *t_end);
int ryujin_hip_quantities_time_series(ryujin_hip_ctx *ctx, int manifold, double *rows, size_t capacity_rows,
                                      size_t *n_rows, int clear);

/* ---- InitialValues: analytic initial and Dirichlet states, device resident -- */
/* InitialValues::initial_state(position, t) of the reference (source/initial_values.template.h:154-196) for its
 * analytic InitialState classes, evaluated by ONE device function (ryujin_amd/csrc/initial_states_device.hpp) for
 * every use: at arbitrary points, at the mesh nodes (interpolate_hyperbolic_vector, :222-262) and at the
 * boundary_map entries at the stage times of a Runge-Kutta step (hyperbolic_module.template.h:137-139 called from
 * time_integrator.template.h:279-510). The point is translated by `position`, `direction` is rolled onto the x-axis
 * (z first, then y), the state's momentum is rotated back (affine_transform / affine_transform_vector, :66-148);
 * `direction` is normalised at configure time. A 1-D profile in 2-D / 3-D is evaluated on the first coordinate
 * behind the transform, momentum along `direction`. In 1-D `direction` only has to be non-zero, as in the reference.
 *
 * States and their `params` (the reference's parameter names; its defaults in brackets -- the library applies
 * none, the caller passes every value). Euler and EulerAEOS (the conserved state through the context's equation of
 * state, from_initial_state, euler_aeos/hyperbolic_system.h:1470-1512):
 *   RYUJIN_IV_UNIFORM            euler/initial_state_uniform.h:36-50            0-2 "primitive state" (rho, u, p)
 *   RYUJIN_IV_RADIAL_CONTRAST    euler/initial_state_radial_contrast.h:29-62    0-2 "primitive state inner",
 *                                                                               3-5 "primitive state outer", 6 "radius"
 *   RYUJIN_IV_ISENTROPIC_VORTEX  euler/initial_state_isentropic_vortex.h:54-92  0 "mach number" [2], 1 "beta" [5],
 *                                (dim = 2)                                      2 "gamma" [1.4] (EulerAEOS only)
 *   RYUJIN_IV_LEBLANC            euler/initial_state_leblanc.h:63-120           none (gamma = 5/3 is part of the state)
 *   RYUJIN_IV_RAREFACTION        euler/initial_state_rarefaction.h:40-160       0 "gamma" [1.4] (EulerAEOS only)
 * Euler takes gamma from ryujin_hip_params. Shallow water (gravity and the Manning coefficient from ryujin_hip_params;
 * the bathymetry stays what ryujin_hip_create was given as initial_precomputed until
 * ryujin_hip_initial_values_interpolate_initial_precomputed below replaces it):
 *   RYUJIN_IV_CIRCULAR_DAM_BREAK shallow_water/initial_state_circular_dam_break.h:48-54   0 "still water depth",
 *                                                                               1 "radius", 2 "dam amplitude"
 *   RYUJIN_IV_PARABOLOID         shallow_water/initial_state_paraboloid.h:66-101 (dim = 1)  0 "free surface radius",
 *                                                                               1 "water height", 2 "paraboloid length",
 *                                                                               3 "speed"
 *   RYUJIN_IV_RITTER_DAM_BREAK   shallow_water/initial_state_ritter_dam_break.h:58-80    0 "time initial",
 *                                                                               1 "left water depth"
 *   RYUJIN_IV_SMOOTH_VORTEX      shallow_water/initial_state_smooth_vortex.h:55-85 (dim = 2, without bathymetry)
 *                                                                               0 "reference depth", 1 "mach number",
 *                                                                               2 "beta"
 *   RYUJIN_IV_SLOPING_FRICTION   shallow_water/initial_state_sloping_friction.h:50-85    0 "ramp slope",
 *                                                                               1 "initial discharge"
 * The formulas, statement by statement, are those of ryujin_amd/initial_states.py.
 *
 * The Riemann-data, shock-front, ramp-up and Noh states (values from 11 on; 10 is the library's own id of the function
 * state below and RYUJIN_ERR_ARG here). They have a device function of their own, initial_state_library<E>()
 * (ryujin_amd/csrc/initial_states_library_device.hpp), and kernels of their own; everything said above holds for
 * them. Euler and EulerAEOS (from_initial_state through the context's equation of state, the function one included):
 *   RYUJIN_IV_CONTRAST             euler/initial_state_contrast.h            0-2 "primitive state left", 3-5 "primitive
 *                                                                            state right"; right where x > 0
 *   RYUJIN_IV_THREE_STATE_CONTRAST euler/initial_state_three_state_contrast.h  0-2 "primitive state left", 3 "left
 *                                  region length", 4-6 "primitive state middle", 7 "middle region length", 8-10
 *                                  "primitive state right"; x >= left + middle: right, x >= left: middle
 *   RYUJIN_IV_FOUR_STATE_CONTRAST  euler/initial_state_four_state_contrast.h (dim >= 2)  0-3 "primitive state bottom
 *                                  left", 4-7 "... bottom right", 8-11 "... top left", 12-15 "... top right", each
 *                                  (rho, u, v, p); x >= 0: right, y >= 0: top
 *   RYUJIN_IV_SHOCK_FRONT          euler/initial_state_shock_front.h         0-2 "primitive state" (before the shock, to
 *                                  the right), 3 "mach number" [2], 4 "gamma" [1.4] (EulerAEOS only); the state behind
 *                                  the shock and its speed S3 are formed at configure time, for EulerAEOS with the
 *                                  covolume b of the interpolatory equation of state the context has THEN; right where
 *                                  x - S3 t > 0
 *   RYUJIN_IV_RAMP_UP              euler/initial_state_ramp_up.h             0-2 "primitive state initial", 3-5
 *                                  "primitive state final", 6 "time initial" [0], 7 "time final" [1]: the two
 *                                  CONSERVED states blended with cos^2 in between
 *   RYUJIN_IV_NOH                  euler/initial_state_noh.h                 0 "reference density" [1], 1 "reference
 *                                  velocity magnitude" [1], 2 "reference pressure" [1e-12], 3 "gamma" [1.4] (EulerAEOS
 *                                  only); the velocity is radial, in all dim components
 *   RYUJIN_IV_SMOOTH_WAVE          euler/initial_state_smooth_wave.h         0 "reference density" [1], 1 "reference
 *                                  pressure" [1], 2 "mach number" [1]; x_0 = 0.1 and x_1 = 0.3 are fixed
 *   RYUJIN_IV_ASTRO_JET            euler/initial_state_astro_jet.h (dim >= 2)  0 "jet width" [0.05], 1-3 "primitive jet
 *                                  state", 4-6 "primitive ambient right", 7 "gamma" [5/3] (EulerAEOS only; read by
 *                                  nothing, as in the reference)
 * Shallow water, zero bathymetry, dim = 1 and 2:
 *   RYUJIN_IV_SW_UNIFORM           shallow_water/initial_state_uniform.h     0-1 "primitive state" (h, u) [1, 1]
 *   RYUJIN_IV_SW_CONTRAST          shallow_water/initial_state_contrast.h    0-1 "primitive state left", 2-3 "primitive
 *                                  state right"; right where x > 0
 * The shallow-water states that bring their own bathymetry (values from 21 on; shallow water only, gravity from
 * ryujin_hip_params). They have a device function of their own, initial_state_sw_bathymetry<dim>()
 * (ryujin_amd/csrc/initial_states_bathymetry_device.hpp), and kernels of their own. A state is (h, q): depth and
 * discharge along the first axis behind the transform. A selector slot takes one of its integer values:
 *   RYUJIN_IV_SW_FLOW_OVER_BUMP          shallow_water/initial_state_flow_over_bump.h (dim = 1, 2)
 *                                        0 "flow type": 0 transcritical [default], 1 subsonic
 *   RYUJIN_IV_SW_THREE_BUMPS_DAM_BREAK   shallow_water/initial_state_three_bumps_dam_break.h (dim = 1: one cone; 2)
 *                                        0 "well balancing validation": 0 false [default], 1 true; 1 "left water depth"
 *                                        [1.875]; 2 "right water depth" [0]; 3 "cone magnitude" [1]
 *   RYUJIN_IV_SW_HOU_TEST                shallow_water/initial_state_hou_test.h (dim = 2)
 *                                        0 "reservoir water depth" [35]
 *   RYUJIN_IV_SW_TRANSIENT               shallow_water/initial_state_transient.h, "transient experiments" (dim = 2)
 *                                        0-1 "flow state left" (h, q) [1, 0]; 2-3 "flow state right" [1, 0];
 *                                        4 "experimental configuration": 0 G1 [default], 1 G2, 2 G3, 3 none
 *   RYUJIN_IV_SW_SOLITON                 shallow_water/initial_state_soliton.h (dim = 1, 2)
 *                                        0 "still water depth" [1]; 1 "amplitude" [0.1]
 * Not offered: "icf like", "becker solution" (it needs the Navier-Stokes parameters), "geotiff" (it needs GDAL),
 * perturbation != 0.
 *
 *   configure     positions [n_relevant * dim]: the node positions of this rank, ghost rows included;
 *                 b_positions [n_bdry * dim]: the positions of the boundary_map entries in boundary_map order (NULL
 *                 if n_bdry == 0). Copied to the device once. A second configure replaces the first. Every rank of a
 *                 partitioned run configures with its own positions.
 *   evaluate      out [n * k] = initial_state(points [n * dim], t), AoS; n = 0 returns RYUJIN_OK and writes nothing.
 *                 Waits for the context's stream.
 *   interpolate   the state vector behind `handle` := initial_state(position_i, t) for ALL n_relevant rows (ghost
 *                 rows are evaluated like owned ones: nothing to exchange). An enqueue.
 *   prepare_state_vector_iv   prepare_state_vector with the Dirichlet data evaluated on the device at t.
 *   time_step_iv  ryujin_hip_time_step_n with the Dirichlet data of every stage evaluated on the device at
 *                 t + c_s tau (SSPRK22 c = 0, 1; SSPRK33 0, 1, 1/2; ERK stage s at s), tau read from the device where
 *                 the first stage left it: unlike ryujin_hip_time_step_fn nothing on the host waits for tau, no
 *                 host function is called and nothing crosses PCIe; one host synchronisation per RK step, at its
 *                 end. All seven schemes, bang-bang recovery with its internal re-run included. A rank without
 *                 boundary entries launches nothing for it.
 *
 * The bathymetry: InitialValues::interpolate_initial_precomputed_vector (initial_values.template.h:181-185, 270-300),
 * initial_precomputations(affine_transform(point)) of the configured state. Valid after any configure or
 * configure_function; RYUJIN_ERR_UNSUPPORTED on a Description with n_initial_precomputed == 0 (everything but shallow
 * water). "paraboloid", "sloping friction", "flow over bump", "three bumps dam break", "hou test" and "transient
 * experiments" have a bed; every other state -- "soliton" and the function state included, whose bathymetry member the
 * reference never reads -- gives exact zeros, the default of the base class.
 *   interpolate_initial_precomputed   the context's bathymetry := the bed at ALL n_relevant node positions (ghost
 *                 rows are evaluated like owned ones: nothing to exchange). An enqueue on the context's stream. It
 *                 replaces what ryujin_hip_create was given as initial_precomputed.
 *   evaluate_initial_precomputed      out [n * n_initial_precomputed] = the bed at points [n * dim]; n = 0 returns
 *                 RYUJIN_OK and writes nothing. Waits for the context's stream.
 *   ryujin_hip_get_initial_precomputed   out [n_relevant * n_initial_precomputed] = what the context holds now: until
 *                 interpolate_initial_precomputed is called, what ryujin_hip_create was given, or zeros. Like the
 *                 other two it needs a configure or configure_function first (RYUJIN_ERR_ARG before one), also to
 *                 read back what create was given.
 *
 * RYUJIN_ERR_ARG: an unknown state or one the context's Description does not have, a zero direction, NULL positions,
 * a selector slot that is not one of its integer values, any entry but configure before configure.
 * RYUJIN_ERR_UNSUPPORTED: scalar conservation (its only state in the reference is the expression-defined "function"
 * state: ryujin_hip_initial_values_configure_function below), perturbation != 0 (an unseeded generator in the
 * reference), a state in a dimension it is not defined for. */
enum {
  RYUJIN_IV_UNIFORM = 0,
  RYUJIN_IV_RADIAL_CONTRAST = 1,
  RYUJIN_IV_ISENTROPIC_VORTEX = 2,
  RYUJIN_IV_LEBLANC = 3,
  RYUJIN_IV_RAREFACTION = 4,
  RYUJIN_IV_CIRCULAR_DAM_BREAK = 5,
  RYUJIN_IV_PARABOLOID = 6,
  RYUJIN_IV_RITTER_DAM_BREAK = 7,
  RYUJIN_IV_SMOOTH_VORTEX = 8,
  RYUJIN_IV_SLOPING_FRICTION = 9,
  /* 10: the function state, ryujin_hip_initial_values_configure_function */
  RYUJIN_IV_CONTRAST = 11,
  RYUJIN_IV_THREE_STATE_CONTRAST = 12,
  RYUJIN_IV_FOUR_STATE_CONTRAST = 13,
  RYUJIN_IV_SHOCK_FRONT = 14,
  RYUJIN_IV_RAMP_UP = 15,
  RYUJIN_IV_NOH = 16,
  RYUJIN_IV_SMOOTH_WAVE = 17,
  RYUJIN_IV_ASTRO_JET = 18,
  RYUJIN_IV_SW_UNIFORM = 19,
  RYUJIN_IV_SW_CONTRAST = 20,
  RYUJIN_IV_SW_FLOW_OVER_BUMP = 21,
  RYUJIN_IV_SW_THREE_BUMPS_DAM_BREAK = 22,
  RYUJIN_IV_SW_HOU_TEST = 23,
  RYUJIN_IV_SW_TRANSIENT = 24,
  RYUJIN_IV_SW_SOLITON = 25
};
typedef struct ryujin_hip_initial_values {
  int state;           /* RYUJIN_IV_*: "configuration" of subsection "E - InitialValues" */
  double params[16];   /* see above; unused entries 0 */
  double direction[3]; /* "initial - direction"; the first dim entries are read */
  double position[3];  /* "initial - position" */
  double perturbation; /* "perturbation": must be 0 */
} ryujin_hip_initial_values;
int ryujin_hip_initial_values_configure(ryujin_hip_ctx *ctx, const ryujin_hip_initial_values *initial_values,
                                        const double *positions, const double *b_positions);
int ryujin_hip_initial_values_evaluate(ryujin_hip_ctx *ctx, const double *points, size_t n, double t, double *out);
int ryujin_hip_initial_values_interpolate(ryujin_hip_ctx *ctx, int handle, double t);
int ryujin_hip_initial_values_interpolate_initial_precomputed(ryujin_hip_ctx *ctx);
int ryujin_hip_initial_values_evaluate_initial_precomputed(ryujin_hip_ctx *ctx, const double *points, size_t n,
                                                           double *out);
int ryujin_hip_get_initial_precomputed(ryujin_hip_ctx *ctx, double *out /* [n_relevant * n_initial_precomputed] */);
int ryujin_hip_prepare_state_vector_iv(ryujin_hip_ctx *ctx, int handle, double t);
int ryujin_hip_time_step_iv(ryujin_hip_ctx *ctx, int scheme, int h_state, int n_tmp, const int *h_tmp, double t,
                            double tau_max, int cfl_recovery, double cfl_min, double cfl_max, double *tau_out);

/* ---- The function state: configuration = function, one expression per primitive component ---- */
/* source/{euler,shallow_water,scalar_conservation}/initial_state_function.h: the primitive state at (x, t) is one
 * expression per component in the variables x [y [z]] and t, evaluated behind the affine transform above, turned
 * into the conserved state by the Description's from_primitive_state, the momentum rotated back:
 *   Euler                (density, velocity x [y [z]], pressure)   E = p / (gamma - 1) + 1/2 rho |v|^2
 *   EulerAEOS            the same parameters, but from_primitive_state (euler_aeos/hyperbolic_system.h:1473-1493)
 *                        reads the LAST component as the specific internal energy e: E = rho e + 1/2 rho |v|^2; the
 *                        equation of state does not enter (unlike the analytic states, which go through
 *                        from_initial_state)
 *   shallow water        (water depth, velocity x [y])             (h, h v)
 *   scalar conservation  (the value)
 * The reference parses with dealii::FunctionParser (muparser). This library has a parser of its own
 * (ryujin_amd/csrc/expression.hpp) for the following subset; THIS TABLE IS THE CONTRACT. deal.II is not available
 * to this project's builds, so its exact choices -- above all the rounding in front of if, |, & and int, and that a
 * literal exponent 2, 3, 4 is multiplied out -- are restated from its documentation and are not checked against it.
 *
 *   literals     decimal numbers with optional fraction and exponent (2, .5, 1.5, 1e-3, 1.5E+2); _pi, _e
 *   variables    x, then y (dim >= 2), z (dim = 3), and t
 *   binary operators by rising precedence, left-associative unless noted:
 *     c ? a : b          right-associative; c is tested != 0
 *     ||  |              1 or 0; || tests != 0, | rounds its operands first
 *     &&  &              1 or 0; && tests != 0, & rounds its operands first
 *     <  >  <=  >=  ==  !=      one level; 1 or 0
 *     +  -
 *     *  /
 *     ^                  right-associative. A literal exponent 2, 3 or 4 is multiplied out from the left (a*a*a*a);
 *                        everything else is pow(a, b)
 *   unary - +    bind weaker than ^ (-x^2 = -(x^2)) and stronger than * /; also in an exponent (2^-x)
 *   functions of one argument
 *     sin cos tan asin acos atan sinh cosh tanh asinh acosh atanh exp log ln log2 log10 sqrt abs erf erfc
 *                        (log and ln: the natural logarithm)
 *     cot csc sec        1 / tan, 1 / sin, 1 / cos
 *     sign               -1, 0 or 1
 *     floor ceil         ; rint(a) = floor(a + 1/2); int(a) = a rounded
 *   functions of several arguments
 *     pow(a, b)          ; min(a, ...), max(a, ...) with one or more arguments, folded from the left with < ;
 *     if(c, a, b)        c is rounded first, then tested != 0
 *   "rounded": to the nearest integer, halves away from zero, trunc(a + (a >= 0 ? 1/2 : -1/2)).
 *   ?: and if evaluate BOTH arms and then select: the same value for these side-effect free operands, and a NaN of
 *   the arm not taken is discarded. Space, tab and line ends separate tokens.
 * RYUJIN_ERR_UNSUPPORTED: rand, rand_seed, sum, avg, string arguments, assignment. RYUJIN_ERR_ARG: everything else
 * outside the table -- an unknown identifier (pi without the underscore), y in 1-D, unbalanced parentheses, a wrong
 * number of arguments, an empty string, text behind the expression --, a program of more than
 * RYUJIN_EXPR_MAX_INSTRUCTIONS instructions (one per literal, variable, operator and function call), more than
 * RYUJIN_EXPR_MAX_STACK operands alive at once (1+(1+(1+ ... nests one per level), parentheses and calls nested
 * deeper than 64. ryujin_hip_last_error names the character (counted from 0) where the refusal arose.
 * Arithmetic: + - * /, sqrt, comparisons, selection and rounding give the same bits on the host and on the device;
 * pow is the library's own on the device and the C library's on the host, the other functions are each side's.
 *
 *   configure_function   n_expressions = the number of primitive components, in the order above; direction,
 *                        position, positions and b_positions as ryujin_hip_initial_values_configure takes them. It
 *                        replaces an earlier configure or configure_function, and configure replaces it. A refused
 *                        call leaves the earlier configuration in place. Afterwards evaluate, interpolate,
 *                        prepare_state_vector_iv and time_step_iv work as for the analytic states, for scalar
 *                        conservation too. The programs are evaluated by an interpreter on the device: the operand
 *                        stack in LDS, the program read through the scalar cache.
 *   expression_evaluate  needs no context and no device: out[i] = expression(points [n * dim], t) with the host's
 *                        interpreter (the same source as the device's). n = 0 returns RYUJIN_OK and writes nothing. */
#define RYUJIN_EXPR_MAX_INSTRUCTIONS 256
#define RYUJIN_EXPR_MAX_STACK 16
int ryujin_hip_initial_values_configure_function(ryujin_hip_ctx *ctx, int n_expressions,
                                                 const char *const *expressions, const double direction[3],
                                                 const double position[3], const double *positions,
                                                 const double *b_positions);
int ryujin_hip_expression_evaluate(const char *expression, int dim, const double *points, size_t n, double t,
                                   double *out);

/* ---- The function flux: FluxLibrary "function" of the scalar conservation equation ---- */
/* source/scalar_conservation/flux_function.h: ONE expression string in the variable u, its components separated by
 * ';', exactly one per space dimension ("sin(u); cos(u)" in 2-D); the gradient is the central difference quotient
 * (f(u + delta) - f(u - delta)) / (2 * delta). The grammar is the table above with the single variable u: x, y, z and
 * t are unknown identifiers here (RYUJIN_ERR_ARG). Any other number of components, an empty component included (a
 * trailing ';'), is RYUJIN_ERR_ARG; the limits -- RYUJIN_EXPR_MAX_INSTRUCTIONS, RYUJIN_EXPR_MAX_STACK, nesting 64 --
 * hold per component; ryujin_hip_last_error names the character, counted from 0 in the WHOLE string. A context created
 * with sc_flux = RYUJIN_FLUX_FUNCTION starts from the reference's default "0.5*u*u" (in every direction) and
 * sc_derivative_approximation_delta.
 *   flux_configure_function   valid on a scalar conservation context created with any flux (RYUJIN_ERR_UNSUPPORTED for
 *                             the other Descriptions, and for what the table refuses with that status); afterwards the
 *                             context uses the function flux. RYUJIN_ERR_ARG: delta <= 0 or not finite, a parse error.
 *                             A refused call leaves the earlier flux in place. It may be called between updates (it
 *                             waits for the stream) and takes effect at the next prepare_state_vector; on several
 *                             ranks every rank's context is configured by its own call.
 *                             On the device f(u) and the difference quotient are formed once per node by the
 *                             interpreter (three runs of the programs); everything behind the precomputed values is
 *                             the code of the other fluxes. With sc_use_averaged_entropy the Riemann solver evaluates
 *                             f((u_i + u_j) / 2) per pair as well: steps 2 and 3 then run kernels with the interpreter
 *                             in their column loop (ryujin_hip_flux_info: step2_interpreted).
 *   flux_function_evaluate    needs no context and no device: the host interpreter of the same source. value and
 *                             gradient are [n][dim]; gradient may be NULL; n = 0 returns RYUJIN_OK and writes nothing.
 *   flux_info                 what the latest update ran, from host values (before the first update: what the next
 *                             one would run, step2_interpreted = 0): kind = RYUJIN_FLUX_*, n_instructions = the
 *                             instructions of all components (0 unless the function flux), step2_interpreted = 1 if
 *                             step 2 ran the interpreter kernel. Any of the three pointers may be NULL. */
int ryujin_hip_flux_configure_function(ryujin_hip_ctx *ctx, const char *expression,
                                       double derivative_approximation_delta);
int ryujin_hip_flux_function_evaluate(const char *expression, int dim, double delta, const double *u, size_t n,
                                      double *value, double *gradient);
int ryujin_hip_flux_info(ryujin_hip_ctx *ctx, int *kind, int *n_instructions, int *step2_interpreted);

/* ---- The function equation of state: EquationOfStateLibrary "function" of EulerAEOS ---- */
/* source/euler_aeos/equation_of_state_function.h: FOUR expression strings,
 *   which = 0   pressure                   in rho, e      default "(1.4 - 1.0) * rho * e"
 *   which = 1   specific internal energy   in rho, p      default "p / (rho * (1.4 - 1.0))"
 *   which = 2   temperature                in rho, e      default "e / 718."
 *   which = 3   speed of sound             in rho, e      default "sqrt(1.4 * (1.4 - 1.0) * e)"
 * and the three interpolation parameters of the surrogate (interpolatory covolume b, reference pressure, reference
 * specific internal energy; default 0). The grammar is the table above with these variables: `e` and `p` are
 * variables here, each in its own programs only, Euler's number stays `_e`; x, y, z, t and u are unknown identifiers
 * (RYUJIN_ERR_ARG). The limits -- RYUJIN_EXPR_MAX_INSTRUCTIONS, RYUJIN_EXPR_MAX_STACK, nesting 64 -- hold per
 * expression. ryujin_hip_last_error names the parameter ("pressure", ...) and the character, counted from 0 within
 * that string. The reference checks no consistency between the four, and neither does the library. A context created
 * with eos = RYUJIN_EOS_FUNCTION starts from the defaults.
 *   eos_configure_function   valid on an EulerAEOS context created with any equation of state
 *                            (RYUJIN_ERR_UNSUPPORTED for the other Descriptions, and for what the table refuses with
 *                            that status); a NULL string is that function's default. RYUJIN_ERR_ARG: a parse error, a
 *                            non-finite interpolation parameter. A refused call leaves the earlier equation of state
 *                            in place. It waits for the stream and takes effect at the next prepare_state_vector; on
 *                            several ranks every rank's context is configured by its own call. The surrogate
 *                            (gamma, the Riemann records, the indicator, the bounds, the limiter) reads the three
 *                            interpolation parameters given here.
 *                            On the device the pressure program runs once per node in cycle 0 of the precomputation
 *                            (a kernel of its own); everything behind the precomputed pressure is the code of the
 *                            closed-form members. The analytic initial and Dirichlet states
 *                            (ryujin_hip_initial_values_configure) take specific_internal_energy(rho, p) from the sie
 *                            program: a state configured BEFORE this call is switched over by it, one configured
 *                            afterwards sees it -- both orders give the same values. The function state
 *                            (configure_function above) needs no equation of state.
 *                            NOTHING in the update, or in any feature of this library, reads temperature or speed of
 *                            sound: they are parsed and checked, and eos_function_evaluate_device is their only use
 *                            on the device.
 *   eos_function_evaluate    needs no context and no device: out[i] = expression(rho[i], second[i]) with the host
 *                            interpreter, read with the variables of function `which`; expression = NULL: the
 *                            default. n = 0 returns RYUJIN_OK and writes nothing.
 *   eos_function_evaluate_device   program `which` of the context's configured function equation of state at n
 *                            host points through the device interpreter (RYUJIN_ERR_ARG if the context runs a
 *                            closed-form member).
 *   eos_info                 what the latest prepare_state_vector ran, from host values (before the first one: what
 *                            the next would run, precompute_interpreted = 0): kind = RYUJIN_EOS_*, n_instructions[4]
 *                            (0 unless the function equation of state), precompute_interpreted = 1 if cycle 0 ran the
 *                            interpreter kernel. Any of the three pointers may be NULL.
 * ryujin_hip_debug_function with RYUJIN_DEBUG_AEOS_DIJ_2D / _RECORDS_2D forms p from a closed-form member inside its
 * kernel: with eos = RYUJIN_EOS_FUNCTION it returns RYUJIN_ERR_UNSUPPORTED. */
int ryujin_hip_eos_configure_function(ryujin_hip_ctx *ctx, const char *pressure, const char *specific_internal_energy,
                                      const char *temperature, const char *speed_of_sound, double interpolation_b,
                                      double interpolation_pinfty, double interpolation_q);
int ryujin_hip_eos_function_evaluate(int which, const char *expression, const double *rho, const double *second,
                                     size_t n, double *out);
int ryujin_hip_eos_function_evaluate_device(ryujin_hip_ctx *ctx, int which, const double *rho, const double *second,
                                            size_t n, double *out);
int ryujin_hip_eos_info(ryujin_hip_ctx *ctx, int *kind, int *n_instructions, int *precompute_interpreted);

/* ---- Error norms: analytic-solution error of a verification run, device resident -- */
/* The norms of TimeLoop::compute_error() of the reference (source/time_loop.template.h:692-833) between the state
 * vector behind h_state (U) and the analytic vector behind h_analytic (A), e = U - A per node, for a list of
 * components of the conserved state. ryujin_hip_offline carries no cells, so the CELLS are an input of their own:
 *   configure   n_cells cells of this rank with dofs_per_cell local indices each (< n_relevant: a cell may reach into
 *               the ghost range), cell_dofs [n_cells][dofs_per_cell]; a quadrature of n_q points given by the TABLE
 *               shape [n_q][dofs_per_cell] = phi_v(x_q) on the reference cell, so that one kernel serves Q1 in 1-D,
 *               2-D and 3-D, Q2 stencils and a dG numbering with any quadrature (Q1 with QGauss(3) -- 2 x 3, 4 x 9,
 *               8 x 27 -- runs out of registers, any other table through run-time loops); and JxW in one of two forms:
 *                 jxw_per_cell == 0   jxw [n_cells][n_q]: |det J(x_q)| w_q, general non-affine cells; weights unused
 *                                     (may be NULL)
 *                 jxw_per_cell != 0   jxw [n_cells]: the cell measure, JxW_q = weights[q] * jxw[cell] with the weights
 *                                     [n_q] of the reference cell (sum 1): affine cells
 *               Every cell belongs to exactly ONE rank (the reference: locally owned cells); a rank with n_cells == 0
 *               is legal and launches nothing. Everything is copied; a second configure replaces the first, a refused
 *               one leaves the previous configuration in place.
 *   compute     detail [n_components][6] (may be NULL) = (Linf, L1, L2 of e; Linf, L1, L2 of A) of component
 *               components[c], over ALL ranks:
 *                 Linf = max |x_i| over the owned rows (:740, :774)
 *                 L1   = sum_cells sum_q |sum_v N_qv x_v| JxW_q,  L2 = sqrt(sum_cells sum_q (sum_v N_qv x_v)^2 JxW_q)
 *               (integrate_difference against the zero function, :743-795; the root behind the sum over the ranks), and
 *               out [3] the consolidated (Linf, L1, L2) of :797-805: with normalize != 0 the sum over the components, in
 *               the given order, of the ratios error norm / analytic norm, without it the sum of the error norms. A
 *               component whose analytic norm is zero gives the reference's IEEE result (x / 0 = inf, 0 / 0 = NaN), and
 *               the consolidated sum inherits it; it is not an error.
 *               Collective over the ranks of the context's communicator: it exchanges the ghost range of h_state as
 *               ryujin_hip_postprocess_compute does, and reads h_analytic AS IT IS (initial_values_interpolate fills
 *               its ghost rows, an uploaded vector carries them). Over the ranks the integrals are summed and the
 *               maxima taken the way Quantities reduces (in-process transport, RCCL). The sums are formed in a fixed
 *               order (no floating-point atomics): reproducible bit for bit for a given partition. The call itself
 *               runs no prepare_state_vector (:701): the caller does, as for a step. It returns the numbers, so it
 *               waits for the stream -- the one copy to the host is 33 doubles.
 * ryujin_hip_offline carries no affine constraints, so AffineConstraints::distribute (:770) has no counterpart here.
 * RYUJIN_ERR_ARG: compute before configure, an index >= n_relevant, dofs_per_cell outside
 * [2, RYUJIN_EN_MAX_DOFS_PER_CELL], n_q outside [1, RYUJIN_EN_MAX_POINTS], a non-finite shape, weights or jxw entry,
 * weights == NULL with jxw_per_cell != 0, NULL arrays with n_cells > 0 (shape: always), a component outside [0, k),
 * n_components outside [1, k], an unknown handle. */
#define RYUJIN_EN_MAX_DOFS_PER_CELL 27
#define RYUJIN_EN_MAX_POINTS 64
#define RYUJIN_EN_MAX_COMPONENTS 5
int ryujin_hip_error_norms_configure(ryujin_hip_ctx *ctx, uint32_t n_cells, int dofs_per_cell,
                                     const uint32_t *cell_dofs, int n_q, const double *shape, const double *weights,
                                     const double *jxw, int jxw_per_cell);
int ryujin_hip_error_norms_compute(ryujin_hip_ctx *ctx, int h_state, int h_analytic, int n_components,
                                   const int *components, int normalize, double out[3], double *detail);

/* ---- VTUOutput: selected fields and level-set cell output, device resident ---- */
/* VTUOutput::schedule_output() of the reference (source/vtu_output.template.h:80-205) up to the writer: the values of
 * "vtu output quantities" at the nodes that go into a file -- all locally relevant nodes (output_full, :142-154) or
 * the nodes of the cells a level set of "manifolds" cuts (output_levelsets, :156-201) -- formed and gathered on the
 * device, so that one output moves [n_quantities][n_nodes] values over PCIe instead of the state vector. The file
 * itself (VTK XML) is written by the caller (ryujin_amd/vtu_output.py).
 *
 * NAMES (source/selected_components_extractor.h:77-88, in this search order; ryujin_amd/csrc/output_selection.hpp):
 *   1 View::component_names            the conserved state, read from U
 *   2 View::primitive_component_names  to_primitive_state(U) as the Postprocessor block above forms it; a name that is
 *                                      both ("rho", "h", "u") is the conserved component
 *   3 View::precomputed_names          Euler "s", "eta_h"; EulerAEOS "p", "surrogate_gamma",
 *                                      "surrogate_specific_entropy", "surrogate_harten_entropy"; shallow water "eta_m",
 *                                      "h_star"; scalar conservation "f[_d]", "df[_d]": what
 *                                      ryujin_hip_state_download_precomputed returns
 *   4 View::initial_precomputed_names  shallow water "bathymetry" (the context's initial_precomputed); the other
 *                                      Descriptions have none, so the name is unknown there
 *   5 "alpha"                          ryujin_hip_get_alpha
 *   6 the postprocessed fields, which the reference always appends (:119-123), by the names of
 *     Postprocessor::component_names() (source/postprocessor.template.h:74-97) -- "schlieren_rho", "vorticity_v_1" --
 *     for the quantities ryujin_hip_postprocess_configure holds WHEN output_configure IS CALLED; the normalised values
 *     of ryujin_hip_postprocess_download(raw = 0)
 * An unknown name is RYUJIN_ERR_ARG with the message of SelectedComponentsExtractor::check (:38-43):
 *   Invalid component name: "<name>" is not a valid conserved/primitive/precomputed/initial component name.
 *
 * MANIFOLDS (:162-165): level-set expressions of the grammar table under "The function state" above in the variables
 * x [y [z]] -- FunctionParser<dim>(expression) has no time, so `t` is an unknown identifier here (RYUJIN_ERR_ARG). The
 * limits RYUJIN_EXPR_MAX_INSTRUCTIONS, RYUJIN_EXPR_MAX_STACK and nesting 64 hold per manifold; a refused manifold is
 * reported as "manifold <index>: ... at character <position>" (counted from 0 within that string). A cell is selected
 * if for SOME manifold one of its vertices has f >= -100 eps and one has f <= +100 eps, eps = DBL_EPSILON (:171-187; a
 * NaN is neither). The level sets are evaluated at the nodes by the device interpreter: the arithmetic subset gives
 * the bits of ryujin_hip_expression_evaluate, a library function differs from the host's by its few ulp (see the
 * table), which can move a cell in or out only where a vertex value lies that close to +-100 eps.
 *
 *   output_configure  names [n_quantities]; positions [n_relevant * dim] of this rank's nodes, ghost rows included;
 *                     the cells of this rank as ryujin_hip_error_norms_configure takes them (cell_dofs
 *                     [n_cells][dofs_per_cell], indices < n_relevant, every cell on exactly ONE rank; the vertex order
 *                     is the caller's and is kept); manifolds [n_manifolds], 0 for the full output only. Everything
 *                     is copied. All that depends on the mesh and the manifolds alone is done HERE, once: the level
 *                     sets at the nodes, the selected cells (ascending cell index), their nodes (ascending local
 *                     index), the map to the new node numbers and the cells' connectivity in it. The lists are formed
 *                     by an order-preserving compaction (ballots inside a block, block offsets from a scan in a launch
 *                     of its own: no block waits for another) and are equal to numpy.flatnonzero of the flags. A second
 *                     configure replaces the first, a refused one leaves the previous configuration in place. A rank
 *                     with n_cells == 0, or none of whose cells is cut, is legal: the counts are 0.
 *   output_info       the counts of the configure-time selection; either pointer may be NULL
 *   output_selection  cell_ids [n_selected_cells] (positions in the caller's cell list), node_ids [n_selected_nodes]
 *                     (local indices) and connectivity [n_selected_cells][dofs_per_cell] in the NEW numbering, i.e.
 *                     indices into node_ids. Any pointer may be NULL.
 *   output_levelset_values   out [n_relevant] = manifold `manifold` at the nodes as the device evaluated it (tests)
 *   output_extract    out [n_quantities][n_nodes], n_nodes = n_relevant (levelsets == 0) or n_selected_nodes, as
 *                     double (RYUJIN_OUT_FLOAT64) or float (RYUJIN_OUT_FLOAT32, what deal.II's writer stores: ONE IEEE
 *                     conversion of the same device value, round to nearest, overflow to inf). One sweep over the
 *                     output nodes forms all quantities: U is read once per node, to_primitive_state evaluated once.
 *                     COLLECTIVE over the ranks of the context's communicator: it exchanges the ghost range of the
 *                     state vector as ryujin_hip_postprocess_compute does (when a conserved or primitive name is
 *                     requested) and, where the rank has ghost rows, fills the ghost range of alpha and of the
 *                     postprocessed fields through the context's vector exchange; a rank without output nodes takes
 *                     part in the exchanges and launches nothing else. It returns the values, so it waits for the
 *                     stream. The precomputed names need a state vector that prepare_state_vector has run on -- the
 *                     caller's duty, as for a step; the values are those of ryujin_hip_state_download_precomputed,
 *                     ghost rows as that call returns them. What the context can tell: RYUJIN_ERR_ARG for a vector whose
 *                     storage no prepare_state_vector (and no update that leaves the precomputed values behind) has
 *                     touched since ryujin_hip_state_alloc; it cannot tell whether U was changed since (an upload, a
 *                     sadd), nor which storage a Runge-Kutta step's swap of the handles left behind the handle.
 *                     The postprocessed names need a ryujin_hip_postprocess_compute since the latest
 *                     ryujin_hip_postprocess_configure, and that configuration to be the one output_configure saw.
 * RYUJIN_ERR_ARG: n_quantities outside [1, RYUJIN_OUT_MAX_QUANTITIES], n_manifolds outside
 * [0, RYUJIN_OUT_MAX_MANIFOLDS], an unknown name, a refused manifold (RYUJIN_ERR_UNSUPPORTED for what the table
 * refuses with that status), a cell index >= n_relevant, NULL arrays with non-zero counts, any other entry before
 * output_configure, levelsets != 0 with no manifold configured, an unknown precision, manifold or handle.
 * RYUJIN_ERR_UNSUPPORTED: dofs_per_cell other than 2^dim (patches of higher-order elements, patch_order > 0 at
 * :137-138, are not subdivided). ryujin_hip_offline carries no affine constraints, so
 * AffineConstraints::distribute (:112) has no counterpart here. */
#define RYUJIN_OUT_MAX_QUANTITIES 32
#define RYUJIN_OUT_MAX_MANIFOLDS 8
enum { RYUJIN_OUT_FLOAT32 = 0, RYUJIN_OUT_FLOAT64 = 1 };
int ryujin_hip_output_configure(ryujin_hip_ctx *ctx, int n_quantities, const char *const *names,
                                const double *positions, uint32_t n_cells, int dofs_per_cell,
                                const uint32_t *cell_dofs, int n_manifolds, const char *const *manifolds);
int ryujin_hip_output_info(ryujin_hip_ctx *ctx, uint32_t *n_selected_cells, uint32_t *n_selected_nodes);
int ryujin_hip_output_selection(ryujin_hip_ctx *ctx, uint32_t *cell_ids, uint32_t *node_ids, uint32_t *connectivity);
int ryujin_hip_output_levelset_values(ryujin_hip_ctx *ctx, int manifold, double *out);
int ryujin_hip_output_extract(ryujin_hip_ctx *ctx, int h_state, int levelsets, int precision, void *out);

#ifdef __cplusplus
}
#endif
#endif /* RYUJIN_HIP_H */
