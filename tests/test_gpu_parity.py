"""Parity of the HIP path (libryujin_hip.so through the C ABI) against the CPU oracle on the same
seeded inputs, plus the reference's integration goldens run on the GPU.

Stated tolerances (BASELINE.md / SURVEY.md Appendix E): d_ij, alpha 1e-12 relative;
U_new 1e-11 relative (per component, scaled by max|U|); l_ij 1e-10 absolute; conservation
defect 1e-13 relative; invariant-domain bounds preserved in sign.
"""
import numpy as np
import pytest

from ryujin_amd import HyperbolicModule, TimeIntegrator, capi, offline
from ryujin_amd.initial_states import euler_radial_contrast, euler_uniform

pytestmark = pytest.mark.gpu


def _perturbed(U, seed=42, amp=1e-3):
    """multiplicative 1 + 1e-3 U(-1,1) perturbation as initial_values.template.h:198-218"""
    rng = np.random.default_rng(seed)
    return U * (1.0 + amp * rng.uniform(-1.0, 1.0, size=U.shape))


class _Mods(list):
    """[(hip module, old, new), (oracle module, old, new)] plus what the l_ij outlier classification needs"""
    oracle = None
    params = None


def _both(spec, U0, oracle, n_warm=0, dirichlet=None, params_edit=None, equation=capi.EQ_EULER, bathymetry=None,
          off=None):
    """Warm up on the GPU (lets shocks form so that the limiter branches are exercised), then hand the
    SAME state to both backends so that one update is compared on identical inputs. `off`: offline data that do not
    come from a recipe (an imported dump, a converted layout) instead of `spec`."""
    if off is None:
        off = offline.SyntheticOffline(spec)
    if bathymetry is not None:
        off.set_initial_precomputed(bathymetry(off.positions))
    mods = _Mods()
    mods.oracle = oracle
    U_start = U0
    for backend in ("hip", oracle.backend()):
        p = oracle.default_params(equation, off.dim)
        p.cfl = 0.9
        if params_edit:
            params_edit(p)
        m = HyperbolicModule(off, p, backend=backend)
        old = m.new_state_vector(U_start)
        new = m.new_state_vector()
        if backend == "hip":
            for _ in range(n_warm):
                m.prepare_state_vector(old, 0.0, dirichlet)
                m.step(old, [], [], new)
                old, new = new, old
            U_start = old.download()
        mods.append((m, old, new))
        mods.params = p
    return off, mods


def _compare_step(off, mods, dirichlet=None, tau=0.0, stage_vectors=None, stage_weights=()):
    """One update on both backends, every intermediate array compared: tests/helpers_parity.py states the
    tolerances and classifies every l_ij outlier as a psi_r = 0 branch flip (no quota)."""
    import inspect

    from helpers_parity import compare_step
    label = next((f.function for f in inspect.stack() if f.function.startswith("test_")), "")
    return compare_step(off, mods, dirichlet, tau, oracle=getattr(mods, "oracle", None),
                        params=getattr(mods, "params", None), label=label, stage_vectors=stage_vectors,
                        stage_weights=stage_weights)


def test_step_parity_2d_step_geometry(oracle):
    """C1-like: Mach-3 forward-facing step, Dirichlet/slip/do-nothing, after shocks formed."""
    spec = offline.mach3_step_2d(40)
    off0 = offline.SyntheticOffline(spec)
    U0 = _perturbed(euler_uniform(off0.positions))
    dirichlet = euler_uniform(off0.b_positions)
    off, mods = _both(spec, U0, oracle, n_warm=12, dirichlet=dirichlet)
    g, c = _compare_step(off, mods, dirichlet)
    # conservation is exercised in test_conservation_closed_box; here: invariant domain in sign
    rho, E = g["U"][: off.n_owned, 0], g["U"][: off.n_owned, 3]
    m2 = (g["U"][: off.n_owned, 1:3] ** 2).sum(1)
    assert (rho > 0).all() and (E - 0.5 * m2 / rho > 0).all()
    assert (np.sign(rho) == np.sign(c["U"][: off.n_owned, 0])).all()


def test_step_parity_c1_size(oracle):
    """BASELINE.json configs[0] at its own size: the mesh of `bench.py --cells-per-unit 130` (43 109 gridpoints) takes
    another column split of the small-mesh kernels of steps 5 and 6 than either the 4 k point mesh above or the
    2.5 M point mesh of the full-size test. A developed bow shock (300 updates), then one update against the oracle."""
    spec = offline.mach3_step_2d(130)
    off0 = offline.SyntheticOffline(spec)
    assert off0.n_owned == 43109
    U0 = euler_uniform(off0.positions)
    dirichlet = euler_uniform(off0.b_positions)
    off, mods = _both(spec, U0, oracle, n_warm=300, dirichlet=dirichlet)
    g, c = _compare_step(off, mods, dirichlet)
    rho, E = g["U"][: off.n_owned, 0], g["U"][: off.n_owned, 3]
    m2 = (g["U"][: off.n_owned, 1:3] ** 2).sum(1)
    assert (rho > 0).all() and (E - 0.5 * m2 / rho > 0).all()


def _checked_case(equation):
    """(mesh, initial state, Dirichlet data, parameter edit) of the checked-build test, per Description"""
    if equation == "euler":
        off = offline.SyntheticOffline(offline.mach3_step_2d(40))
        return off, _perturbed(euler_uniform(off.positions)), euler_uniform(off.b_positions), None, capi.EQ_EULER
    if equation == "euler_aeos":  # the same problem through the EulerAEOS Description (polytropic gas, strict bounds)
        off = offline.SyntheticOffline(offline.mach3_step_2d(40))
        return off, _perturbed(euler_uniform(off.positions)), euler_uniform(off.b_positions), None, capi.EQ_EULER_AEOS
    if equation == "shallow_water":
        from ryujin_amd.initial_states import sw_circular_dam_break
        off = offline.SyntheticOffline(offline.rectangle_2d(48, (-5.0, -5.0), (5.0, 5.0)))
        return off, sw_circular_dam_break(off.positions), None, None, capi.EQ_SHALLOW_WATER
    off = offline.SyntheticOffline(offline.rectangle_2d(48, (-2.0, -2.5), (2.0, 1.5), bc=capi.BC_DIRICHLET))
    r = np.linalg.norm(off.positions, axis=1)
    U0 = np.where(r < 1.0, 1.0, -0.5).reshape(-1, 1)
    return off, U0, U0[off.b_i], None, capi.EQ_SCALAR_CONSERVATION


@pytest.mark.parametrize("cfl", [0.9, 4.0])
@pytest.mark.parametrize("equation", ["euler", "euler_aeos", "shallow_water", "scalar_conservation"])
def test_expensive_bounds_check_as_a_run_time_option(oracle, equation, cfl):
    """ryujin_hip_params::debug_expensive_bounds_check: the reference's EXPENSIVE_BOUNDS_CHECK build (is_admissible
    behind steps 4, 6 and 7, the limiter's checked control flow in both passes,
    hyperbolic_module.template.h:851-855,1121-1126,1155-1161 -- generic over the Description; the limiters:
    euler/, euler_aeos/, shallow_water/, scalar_conservation/limiter.template.h) against the oracle's, for every
    Description. The l_ij and the new state are those of the production flow (the checked flow returns the same t_l);
    what differs is when a violation is reported: at cfl 0.9 nothing is, at four times the admissible step both
    backends raise it in the same steps."""
    off, U0, dirichlet, edit, eq = _checked_case(equation)
    results = []
    for backend in ("hip", oracle.backend()):
        p = oracle.default_params(eq, 2)
        p.cfl = cfl
        p.id_violation_strategy = capi.IDV_WARN
        if edit:
            edit(p)
        if backend == "hip":
            p.debug_expensive_bounds_check = 1
        m = HyperbolicModule(off, p, backend=backend)
        if backend != "hip":
            oracle.lib().ryujin_oracle_set_expensive_bounds_check(m._ctx, 1)
        a, b = m.new_state_vector(U0), m.new_state_vector()
        statuses = []
        for _ in range(3):
            m.prepare_state_vector(a, 0.0, dirichlet)
            m.step(a, [], [], b)
            statuses.append(m.last_status)
            a, b = b, a
        results.append((statuses, a.download()[: off.n_owned], m.n_warnings()))
    (st_g, U_g, w_g), (st_c, U_c, w_c) = results
    assert st_g == st_c and w_g == w_c, (st_g, st_c)
    if cfl <= 1.0:
        assert w_g == 0
        assert (np.abs(U_g - U_c) / np.abs(U_c).max(axis=0)).max() <= 1e-10
    elif equation != "scalar_conservation":  # (a scalar clip has no invariant domain to leave: nothing need be raised)
        assert w_g > 0


def test_step_parity_3d_radial_contrast(oracle, n=12, warm=(4,)):
    """C3-like: 3-D box, slip walls, strong radial pressure contrast (limiter active). (Several warm-up counts: the
    tiles of P_ij step 5 stores follow what step 6 read in the last three updates.)"""
    spec = offline.box_3d(n)
    off0 = offline.SyntheticOffline(spec)
    U0 = euler_radial_contrast(off0.positions, radius=0.4)
    for n_warm in warm:
        off, mods = _both(spec, U0, oracle, n_warm=n_warm)
        _compare_step(off, mods)


def test_create_refuses_the_retired_pij_storage_modes():
    """debug_pij_storage 3 and 4 selected P_ij per tile in 3-D, measured as a loss and retired
    (profiles/variant_r06_tile_pij_3d_deferred.patch): create() refuses them."""
    import ctypes as C
    lib = capi.load_hip()
    off = offline.SyntheticOffline(offline.box_3d(4))
    for storage in (3, 4):
        p = capi.Params()
        lib.ryujin_hip_default_params(C.byref(p), capi.EQ_EULER, 3)
        p.debug_pij_storage = storage
        ctx = C.c_void_p()
        rc = lib.ryujin_hip_create(C.byref(ctx), off.c, C.byref(p), None, 0)
        if rc >= 0:
            lib.ryujin_hip_destroy(ctx)
        assert rc == capi.RYUJIN_ERR_ARG, (storage, rc)


def test_step_parity_1d(oracle):
    spec = offline.MeshSpec(1, (200,), (0.0,), (1.0,), (capi.BC_DIRICHLET, capi.BC_DO_NOTHING))
    off0 = offline.SyntheticOffline(spec)
    x = off0.positions[:, 0]
    from ryujin_amd.initial_states import euler_from_primitive
    U0 = euler_from_primitive(np.where(x < 0.5, 1.0, 0.125), np.zeros((len(x), 1)), np.where(x < 0.5, 1.0, 0.1))
    dirichlet = U0[off0.b_i]
    off, mods = _both(spec, U0, oracle, n_warm=10, dirichlet=dirichlet)
    _compare_step(off, mods, dirichlet)


def test_multistage_parity_erk33(oracle):
    """step<1>, step<2> with stage weights (time_integrator.template.h:373-403)."""
    spec = offline.mach3_step_2d(20)
    off = offline.SyntheticOffline(spec)
    U0 = _perturbed(euler_uniform(off.positions))
    dirichlet = euler_uniform(off.b_positions)
    finals = []
    for backend in ("hip", oracle.backend()):
        m = HyperbolicModule(off, equation=capi.EQ_EULER, backend=backend)
        sv = m.new_state_vector(U0)
        ti = TimeIntegrator(m, "erk 33", dirichlet_fn=lambda t: dirichlet)
        t = 0.0
        for _ in range(4):
            sv, tau = ti.step(sv, t)
            t += tau
        finals.append((t, sv.download()[: off.n_owned]))
    assert abs(finals[0][0] - finals[1][0]) < 1e-12 * finals[1][0]
    scale = np.abs(finals[1][1]).max(axis=0)
    assert (np.abs(finals[0][1] - finals[1][1]) / scale).max() < 5e-11


def test_conservation_closed_box(oracle):
    """sum_i m_i U_i is conserved on a closed slip box for rho and E (c_ij = -c_ji, d_ij = d_ji,
    symmetric l_ij): defect <= 1e-13 relative, as check-mass-conservation_01."""
    spec = offline.rectangle_2d(48, (0.0, 0.0), (1.0, 1.0))
    off = offline.SyntheticOffline(spec)
    U0 = euler_radial_contrast(off.positions, inner=(1.0, 0.0, 10.0), outer=(0.125, 0.0, 0.1), radius=0.3,
                               center=(0.5, 0.5))
    m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip")
    sv = m.new_state_vector(U0)
    ti = TimeIntegrator(m, "ssprk 33", cfl_min=0.9, cfl_max=0.9, cfl_recovery_strategy="none")
    mi = off.mi[: off.n_owned]
    m.prepare_state_vector(sv, 0.0)
    before = (mi[:, None] * sv.download()[: off.n_owned]).sum(0)
    t = 0.0
    for _ in range(10):
        sv, tau = ti.step(sv, t)
        t += tau
    after = (mi[:, None] * sv.download()[: off.n_owned]).sum(0)
    for comp in (0, 3):
        assert abs(after[comp] - before[comp]) <= 1e-13 * abs(before[comp])


def test_near_vacuum_rows_keep_their_bounds_after_the_high_order_update(oracle):
    """Steps 6/7 next to vacuum (a 2-D Le Blanc-like contrast: density 1 : 1e-6, pressure 1e10 : 1). Strongly limited
    rows -- l_ij = 0 or tiny against an unlimited flux lambda P_ij that is orders larger than U_i^low -- must come out
    as the reference forms them, U_i^low + sum_j l_ij lambda P_ij: inside their bounds up to the limiter's relaxation
    (limiter.template.h:24-27), not displaced by the rounding of V_i - sum_j (1 - l_ij) lambda P_ij.
    Compared array by array with the oracle, then the bounds are checked on the device's own new state."""
    spec = offline.rectangle_2d(40, (0.0, 0.0), (1.0, 1.0))
    off0 = offline.SyntheticOffline(spec)
    U0 = euler_radial_contrast(off0.positions, inner=(1.0, 0.0, 1.0e-1), outer=(1.0e-6, 0.0, 1.0e-11), radius=0.3,
                               center=(0.5, 0.5))
    for n_warm in (3, 9):
        off, mods = _both(spec, U0, oracle, n_warm=n_warm)
        g, c = _compare_step(off, mods)
        n = off.n_owned
        assert g["status"] == 0 and (g["U"][:n, 0] > 0).all()
        eps = np.finfo(np.float64).eps
        relax = 1.0e4 * eps  # vacuum_state_relaxation_large * eps
        b = g["bounds"].reshape(-1, 3)[:n]   # rho_min, rho_max, s_min per row, already relaxed by step 4
        rho_min, rho_max, s_min = b[:, 0], b[:, 1], b[:, 2]
        rho = g["U"][:n, 0]
        e = g["U"][:n, 3] - 0.5 * (g["U"][:n, 1:3] ** 2).sum(1) / rho
        assert (rho >= rho_min * (1.0 - relax)).all(), float((rho / rho_min).min() - 1.0)
        assert (rho <= rho_max * (1.0 + relax)).all(), float((rho / rho_max).max() - 1.0)
        assert (e > 0).all()
        s = rho * e / rho ** (mods.params.gamma + 1.0)   # specific entropy rho e / rho^(gamma+1) = e rho^-gamma
        assert (s >= s_min * (1.0 - 100.0 * relax)).all(), float((s / s_min).min() - 1.0)
        # the strongly limited rows are there: pairs limited to (almost) nothing next to the vacuum
        assert (np.minimum(c["lij"], 1.0) < 1e-3).mean() > 1e-3


@pytest.mark.parametrize("kernels", ["small_mesh", "large_mesh"])
def test_random_vacuum_and_shock_patches_keep_their_bounds(oracle, monkeypatch, kernels):
    """A randomised probe of the MIXED rows of steps 6/7: a row with some unlimited (slice,
    column) tiles and a strongly limited pair elsewhere takes the cancelling form V_i - sum (1 - l) lambda P_ij, only
    rows ALL of whose columns lie in limited tiles the reference's sum (kernels_limiter.hpp, ref_order). Random patches
    of near vacuum (density down to 1e-6), high pressure (up to 1e4) and moving gas on a 48 x 48 slip box, a few
    updates of development, then one update against the oracle array by array -- and the bounds the limiter promises,
    checked on the DEVICE's own new state: density within [rho_min, rho_max] (1 +- relax), specific entropy above s_min,
    positive internal energy; the rows the probe is about (some pair limited to < 1e-3, another not limited at all)
    must be there (some pair limited to < 1e-2 next to an unlimited one in the same row)."""
    from ryujin_amd.initial_states import euler_from_primitive
    if kernels == "large_mesh":  # the kernels of BASELINE-sized meshes (P_ij per tile, V_i, the tile-predicated update)
        monkeypatch.setattr(HyperbolicModule, "library_switches",
                            {"debug_no_small_mesh_split": 1, "debug_bc_fold_max_slices": -1})
    spec = offline.rectangle_2d(48, (0.0, 0.0), (1.0, 1.0))
    off0 = offline.SyntheticOffline(spec)
    x = off0.positions
    n_mixed, statuses = 0, []
    for seed in (1, 2, 3, 4):
        rng = np.random.default_rng(1000 + seed)
        n_mixed_seed, statuses_seed = _random_patches_case(oracle, spec, x, rng)
        n_mixed += n_mixed_seed
        statuses += statuses_seed
    assert 0 in statuses and n_mixed >= 5, (statuses, n_mixed)


def _random_patches_case(oracle, spec, x, rng):
    from ryujin_amd.initial_states import euler_from_primitive
    rho, p, vel = np.full(len(x), 1.0), np.full(len(x), 1.0), np.zeros((len(x), 2))
    for _ in range(24):  # patches: boxes with their own state
        lo = rng.uniform(0.0, 0.9, size=2)
        hi = lo + rng.uniform(0.05, 0.3, size=2)
        inside = ((x >= lo) & (x <= hi)).all(axis=1)
        rho[inside] = 10.0 ** rng.uniform(-6.0, 0.5)
        p[inside] = 10.0 ** rng.uniform(-8.0, 2.0)
        vel[inside] = rng.uniform(-1.0, 1.0, size=2) * np.sqrt(1.4 * p[inside][0] / rho[inside][0]) * rng.uniform(0.0, 0.7)
    U0 = euler_from_primitive(rho, vel, p)
    n_mixed, statuses = 0, []
    for n_warm in (2, 5):
        off, mods = _both(spec, U0, oracle, n_warm=n_warm)
        g, c = _compare_step(off, mods)
        n = off.n_owned
        assert g["status"] == c["status"]
        statuses.append(g["status"])
        if g["status"] != 0:
            continue  # (both sides asked for a restart: the limiter's bounds are not promised then)
        eps = np.finfo(np.float64).eps
        relax = 1.0e4 * eps
        b = g["bounds"].reshape(-1, 3)[:n]
        rho_n = g["U"][:n, 0]
        e = g["U"][:n, 3] - 0.5 * (g["U"][:n, 1:3] ** 2).sum(1) / rho_n
        assert (rho_n > 0).all() and (e > 0).all()
        assert (rho_n >= b[:, 0] * (1.0 - relax)).all(), float((rho_n / b[:, 0]).min() - 1.0)
        assert (rho_n <= b[:, 1] * (1.0 + relax)).all(), float((rho_n / b[:, 1]).max() - 1.0)
        s = e * rho_n ** (-mods.params.gamma)
        assert (s >= b[:, 2] * (1.0 - 100.0 * relax)).all(), float((s / b[:, 2]).min() - 1.0)
        # mixed rows: the symmetrised l of the first pass has an (almost) closed pair and an open one in the same row
        rs = off.row_starts.astype(np.int64)
        l = np.minimum(c["lij"], 1.0)
        for i in range(n):
            li = l[rs[i] + 1: rs[i + 1]]
            if li.size and li.min() < 1e-2 and li.max() == 1.0:
                n_mixed += 1
    return n_mixed, statuses


def test_tile_map_gives_the_same_bits_as_the_index_arrays(oracle):
    """The tile map (host_layout.hpp: TileDesc): column indices and transposed positions of structured 64-row tiles from
    a 16-byte descriptor in the 2-D sweeps 3, 5, 6, 7. Same indices, so the same bits as with the map switched off
    (ryujin_hip_params::debug_tile_map = -1; likewise the stacked slice-to-wave mapping, debug_band_stride = -1),
    stage-wise and through the device-resident driver, on a mesh whose rows
    are mostly regular (Mach-3 step) and on one partition of it (export rows first: the ragged end of the numbering)."""
    for n_ranks, rank in ((1, 0), (3, 1)):
        spec = offline.mach3_step_2d(60, n_ranks=n_ranks, rank=rank)
        off = offline.SyntheticOffline(spec)
        U0 = _perturbed(euler_uniform(off.positions))
        dirichlet = euler_uniform(off.b_positions) if off.n_bdry else None
        results = []
        for switch, xcd_chunk in ((0, -1), (-1, -1), (0, 2), (-1, 5)):
            p = oracle.default_params(capi.EQ_EULER, 2)
            p.cfl = 0.9
            p.debug_tile_map = switch
            p.debug_band_stride = switch  # stacked blocks (row_context()): which wave takes which slice
            p.debug_xcd_chunk = xcd_chunk  # XCD-local block ranges (row_context()): which block takes which slices
            comm = None
            if n_ranks > 1:  # a middle rank on its own: the loopback communicator stands in for its neighbours
                import ctypes as C
                comm = C.c_void_p()
                assert capi.load_hip().ryujin_hip_comm_init_loopback(C.byref(comm), rank, n_ranks, 0) == 0
            m = HyperbolicModule(off, p, backend="hip", comm=comm)
            info = m.layout_info()
            assert (info["n_regular_tiles"] > 0) == (switch == 0), info  # (C2: 0.977 of the tiles; these small meshes 0.65 / 0.11)
            a, b = m.new_state_vector(U0), m.new_state_vector()
            for _ in range(6):
                m.prepare_state_vector(a, 0.0, dirichlet)
                m.step(a, [], [], b)
                a, b = b, a
            temps = [b, m.new_state_vector(), m.new_state_vector()]
            for _ in range(2):
                m.time_step("ssprk 33", a, temps, dirichlet)
            results.append((a.download(), m.alpha().copy(), m.debug_fetch("lij")))
            m.close()
        for other in results[1:]:
            for x, y in zip(results[0], other):
                assert np.array_equal(x, y)


@pytest.mark.parametrize("case", ["euler_3d", "shallow_water_2d", "euler_aeos_2d"])
def test_chained_gathers_give_the_same_bits_as_the_gathers(oracle, case):
    """Chained gathers (host_layout.hpp, TileDesc::chain; kernels_euler.hpp): where the columns of a slice are a run of
    consecutive node indices, step 5 takes the neighbour's node data from the previous column's -- or the slice's own
    rows' -- registers one lane over (DPP / LDS) and only the lane at the end of the wave fetches its node. The same
    values into the same operations: the same bits as with the map -- and with it the chains -- switched off
    (debug_tile_map = -1), in 3-D (parked rows, explicit column indices), for the Description with a stored first
    part of P_ij (k_pij_lij) and for EulerAEOS; and most tiles of a lattice-numbered mesh are chained."""
    from ryujin_amd.initial_states import euler_radial_contrast, sw_circular_dam_break
    dirichlet = None
    if case == "euler_3d":
        off = offline.SyntheticOffline(offline.box_3d(6, nx=200))  # (lattice rows of 201 nodes: most slices lie inside one)
        U0 = _perturbed(euler_radial_contrast(off.positions, inner=(1.0, 0.0, 10.0), outer=(1.0, 0.0, 0.1), radius=0.4))
        equation, dim = capi.EQ_EULER, 3
    elif case == "shallow_water_2d":
        off = offline.SyntheticOffline(offline.rectangle_2d(200, (-5.0, -5.0), (5.0, 5.0), ny=24))
        U0 = sw_circular_dam_break(off.positions)
        equation, dim = capi.EQ_SHALLOW_WATER, 2
    else:
        off = offline.SyntheticOffline(offline.mach3_step_2d(60))
        U0 = _perturbed(euler_uniform(off.positions))
        dirichlet = euler_uniform(off.b_positions)
        equation, dim = capi.EQ_EULER_AEOS, 2
    results = []
    for switch in (0, -1):
        p = oracle.default_params(equation, dim)
        p.cfl = 0.9
        p.debug_tile_map = switch
        m = HyperbolicModule(off, p, backend="hip")
        info = m.layout_info()
        if switch == 0:  # (C2: 0.65 of all tiles -- the diagonal column included --, 6 of the 8 off-diagonal columns)
            assert info["chained_tile_fraction"] > 0.4 and info["chained_entry_fraction"] > 0.35, info
        else:
            assert info["n_chained_tiles"] == 0, info
        a, b = m.new_state_vector(U0), m.new_state_vector()
        for _ in range(5):
            m.prepare_state_vector(a, 0.0, dirichlet)
            m.step(a, [], [], b)
            a, b = b, a
        temps = [b, m.new_state_vector(), m.new_state_vector()]
        m.time_step("ssprk 33", a, temps, dirichlet)
        results.append((a.download(), m.alpha().copy(), m.debug_fetch("lij"), m.debug_fetch("pij")))
        m.close()
    for x, y in zip(*results):
        assert np.array_equal(x, y)


def test_mass_conservation_01_golden_on_gpu(golden_dir):
    """The reference's own integration baseline, reproduced by the HIP path."""
    from test_oracle_golden_integration import golden_mass_conservation, run_mass_conservation
    gold = golden_mass_conservation(golden_dir)
    got, m = run_mass_conservation("hip")
    assert m.n_warnings() == 0
    np.testing.assert_allclose(got[:, 0], gold[:, 0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got[:, [1, 2, 4]], gold[:, [1, 2, 4]], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got[:, [5, 6, 8]], gold[:, [5, 6, 8]], rtol=1e-11, atol=0)
    assert np.abs(got[:, 1] - 1.4).max() < 1e-13


@pytest.mark.parametrize("scheme", ["ssprk 33", "erk 33"])
def test_isentropic_vortex_golden_on_gpu(golden_dir, scheme):
    from test_oracle_golden_integration import _golden_vortex, run_isentropic_vortex
    dofs, t_ref, linf_ref, l1_ref, l2_ref = _golden_vortex(golden_dir, scheme, 5)
    t, linf, l1, l2, n = run_isentropic_vortex("hip", scheme, 5)
    assert n == dofs
    assert abs(t - t_ref) < 1e-10
    assert abs(linf - linf_ref) < 1e-8 * linf_ref
    assert abs(l1 - l1_ref) < 1e-8 * l1_ref
    assert abs(l2 - l2_ref) < 1e-8 * l2_ref


def test_restart_signalling(oracle):
    """An over-aggressive CFL violates the limiter bounds: RYUJIN_WARN / Restart exactly when the
    oracle reports it, counters as hyperbolic_module.template.h:1198-1207."""
    from ryujin_amd import Restart
    spec = offline.rectangle_2d(24, (0.0, 0.0), (1.0, 1.0))
    off = offline.SyntheticOffline(spec)
    U0 = euler_radial_contrast(off.positions, inner=(1.0, 0.0, 1000.0), outer=(0.01, 0.0, 0.01), radius=0.3,
                               center=(0.5, 0.5))
    res = []
    for backend in ("hip", oracle.backend()):
        m = HyperbolicModule(off, equation=capi.EQ_EULER, backend=backend)
        m.cfl = 3.0
        old, new = m.new_state_vector(U0), m.new_state_vector()
        m.prepare_state_vector(old, 0.0)
        m.step(old, [], [], new)
        w = m.n_warnings()
        m.id_violation_strategy = capi.IDV_RAISE_EXCEPTION
        raised = False
        try:
            m.step(old, [], [], new)
        except Restart:
            raised = True
        res.append((w, raised, m.n_restarts()))
    assert res[0] == res[1]
    assert res[0][0] == 1 and res[0][1] and res[0][2] == 1


def test_reference_simd_layout_import(oracle):
    """The C ABI accepts the reference's SIMD-interleaved storage (simd_length 4 and 8): same
    results as with the plain CSR input."""
    import ctypes as C
    spec = offline.rectangle_2d(20, (0.0, 0.0), (1.0, 1.0))
    off = offline.SyntheticOffline(spec)
    U0 = _perturbed(euler_uniform(off.positions))
    m0 = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip")
    a, b = m0.new_state_vector(U0), m0.new_state_vector()
    m0.prepare_state_vector(a, 0.0)
    m0.step(a, [], [], b)
    ref = b.download()
    from helpers_layout import to_simd_layout
    scale = np.abs(ref).max(axis=0)
    for sl in (4, 8):
        off_simd = to_simd_layout(off, sl)   # renumbered: rows of equal stencil size first
        assert off_simd.n_internal > 0
        m1 = HyperbolicModule(off_simd, equation=capi.EQ_EULER, backend="hip")
        a1, b1 = m1.new_state_vector(U0[off_simd.order]), m1.new_state_vector()
        m1.prepare_state_vector(a1, 0.0)
        m1.step(a1, [], [], b1)
        got = b1.download()[off_simd.new_index]
        # same mesh, different numbering: stencil summation order differs -> round-off only
        assert (np.abs(got - ref) / scale).max() < 1e-12
        # the ORACLE on the same SIMD-interleaved arrays, sweep by sweep (it reads the layout through its own
        # restatement of sparse_matrix_simd.h:403-418, oracle/csr.hpp)
        _, mods = _both(None, U0[off_simd.order], oracle, n_warm=3, off=off_simd)
        _compare_step(off_simd, mods)


def test_device_pow_accuracy():
    """ryujin::pow on the device (exp(y log x) with explicit FMA polynomials, special cases resolved by
    selects, no call into ocml): a few ulp for the argument ranges of the hot path, std::pow's special-case
    behaviour (zero, negative base with integer exponent, inf, nan, subnormal base)."""
    import math
    lib = capi.load_hip()
    rng = np.random.default_rng(7)
    n = 200000
    x = np.exp(rng.uniform(-12, 12, n))
    fixed = np.array([1.4, -1.4, 1 / 2.4, -1.4 / 2.4, 2.4, 1 / 7.0, 7.0, -1 / 7.0, 2.5])
    y = np.where(np.arange(n) % 2 == 0, fixed[np.arange(n) % 9], rng.uniform(-3, 3, n))
    # special cases: x = 0, negative, inf, nan, subnormal
    x[:6] = [0.0, -1.0, np.inf, np.nan, 5e-324, 1.0]
    y[:6] = [1.4, 2.0, 1.4, 1.4, 0.5, 123.0]
    out = np.empty(n)
    rc = lib.ryujin_hip_debug_pow(0, capi.as_ptr(x, capi.c_double_p), capi.as_ptr(y, capi.c_double_p),
                                  capi.as_ptr(out, capi.c_double_p), n)
    assert rc == 0
    ref = np.array([math.pow(a, b) if (a >= 0 or float(b).is_integer()) and not math.isnan(a) else float("nan")
                    for a, b in zip(x[6:].tolist(), y[6:].tolist())])
    rel = np.abs(out[6:] - ref) / np.abs(ref)
    budget = 2.5 * 1.1e-16 * (1.0 + np.abs(y[6:] * np.log(x[6:])))
    assert (rel <= budget).all(), (rel / budget).max()
    assert out[0] == 0.0 and out[1] == 1.0 and out[2] == np.inf and np.isnan(out[3])
    # subnormal base: renormalised, then the same budget as everywhere (|y log x| = 372 here)
    assert abs(out[4] - math.sqrt(5e-324)) <= 2.5 * 1.1e-16 * (1.0 + 0.5 * 744.44) * math.sqrt(5e-324)
    assert out[5] == 1.0


@pytest.mark.parametrize("n_ranks,mode", [(2, ""), (3, ""), (3, "join_exchanges"), (3, "bc_launch"),
                                          (3, "system_events"), (3, "per_slice_pij")])
def test_partitioned_hip_matches_single_rank(n_ranks, mode, monkeypatch):
    """Multi-rank code path of the library on ONE GPU: n contexts (one host thread each) own x-slabs of
    the mesh and exchange ghosts through the in-process transport (ryujin_hip_comm_init_local), which
    shares pack kernels, send/receive offsets and the ghost-row layout with the RCCL transport. The
    partitioned run must reproduce the single-rank run (same tau; U to round-off).
    mode: the branches small meshes do not take by themselves -- "join_exchanges": the fallback
    choreography of an asymmetric stencil (every sweep joins the exchanges); "bc_launch": boundary
    conditions as a launch of their own in front of the pre-pass (large meshes); "system_events": the events
    between the two streams created with the system-scope fence (ryujin_hip_params::system_scope_events);
    "per_slice_pij": the kernels of large meshes with P_ij stored per 64-row slice and no slice predicted limited."""
    import ctypes as C
    import threading

    if mode == "join_exchanges":
        monkeypatch.setattr(HyperbolicModule, "library_switches", {"debug_join_exchanges": 1})
    elif mode == "bc_launch":
        monkeypatch.setattr(HyperbolicModule, "library_switches", {"debug_bc_fold_max_slices": -1})
    elif mode == "system_events":
        monkeypatch.setattr(HyperbolicModule, "library_switches", {"system_scope_events": 1})
    elif mode == "per_slice_pij":  # nothing predicted: trigger, repair prologue, two-launch step 6 in both parts
        monkeypatch.setattr(HyperbolicModule, "library_switches",
                            {"debug_pij_storage": 1, "debug_no_small_mesh_split": 1, "debug_bc_fold_max_slices": -1})

    lib = capi.load_hip()
    cpu, n_updates = 40, 6

    def initial(off):
        U0 = euler_uniform(off.positions)
        return U0 * (1.0 + 1e-3 * np.sin(7.0 * off.positions[:, :1] + 3.0 * off.positions[:, 1:2]))

    def run(off, comm, out, key):
        try:
            m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip", comm=comm)
            m.cfl = 0.9
            dirichlet = euler_uniform(off.b_positions) if off.n_bdry else None
            a, b = m.new_state_vector(initial(off)), m.new_state_vector()
            taus = []
            for _ in range(n_updates):
                m.prepare_state_vector(a, 0.0, dirichlet)
                taus.append(m.step(a, [], [], b))
                a, b = b, a
            out[key] = (off.global_ids[: off.n_owned].astype(np.int64), a.download()[: off.n_owned], taus,
                        m.alpha()[: off.n_owned])
        except Exception as e:  # surface errors of worker threads in the main thread
            out[key] = e

    ref = {}
    run(offline.SyntheticOffline(offline.mach3_step_2d(cpu)), None, ref, 0)
    assert not isinstance(ref[0], Exception), ref[0]
    gid, U, taus, alpha = ref[0]

    comms = (C.c_void_p * n_ranks)()
    assert lib.ryujin_hip_comm_init_local(comms, n_ranks, 0) == 0
    parts = [offline.SyntheticOffline(offline.mach3_step_2d(cpu, n_ranks=n_ranks, rank=r)) for r in range(n_ranks)]
    out = {}
    threads = [threading.Thread(target=run, args=(parts[r], C.c_void_p(comms[r]), out, r)) for r in range(n_ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
        assert not t.is_alive(), "rank thread hung"
    for r in range(n_ranks):
        assert not isinstance(out[r], Exception), out[r]
        assert np.allclose(out[r][2], taus, rtol=1e-13, atol=0)
    g = np.concatenate([out[r][0] for r in range(n_ranks)])
    Up = np.concatenate([out[r][1] for r in range(n_ranks)])
    ap = np.concatenate([out[r][3] for r in range(n_ranks)])
    o1, o2 = np.argsort(gid), np.argsort(g)
    assert np.array_equal(gid[o1], g[o2])
    scale = np.abs(U).max(axis=0)
    assert (np.abs(Up[o2] - U[o1]) / scale).max() < 1e-12
    assert np.abs(ap[o2] - alpha[o1]).max() < 1e-10
    for r in range(n_ranks):
        lib.ryujin_hip_comm_destroy(C.c_void_p(comms[r]))


# ----------------------------------------------------------------------------- shallow water

def _bump(pos):
    return 0.8 * np.exp(-1.5 * ((pos[:, 0] - 1.5) ** 2 + (pos[:, 1] + 1.0) ** 2)) + 0.02 * pos[:, 0]


def test_sw_step_parity_2d_dam_break_over_bathymetry(oracle):
    """BASELINE configs[4]-like: circular dam break (initial_state_circular_dam_break.h) over an uneven,
    partly dry bed; slip walls; Manning friction on. Every sweep of the shallow-water path vs the oracle."""
    from ryujin_amd.initial_states import sw_circular_dam_break
    spec = offline.rectangle_2d(48, (-5.0, -5.0), (5.0, 5.0))
    off0 = offline.SyntheticOffline(spec)
    Z = _bump(off0.positions)
    U0 = sw_circular_dam_break(off0.positions, h_outer=0.5)
    U0[:, 0] = np.maximum(U0[:, 0] - Z, 0.0)      # free surface at h+Z, dry where the bump pierces it

    def edit(p):
        p.manning_friction_coefficient = 0.03
    off, mods = _both(spec, U0, oracle, n_warm=8, equation=capi.EQ_SHALLOW_WATER, bathymetry=_bump,
                      params_edit=edit)
    g, c = _compare_step(off, mods)
    assert (g["U"][: off.n_owned, 0] >= 0.0).all()
    assert (np.sign(g["U"][: off.n_owned, 0]) == np.sign(c["U"][: off.n_owned, 0])).all()


def test_sw_step_parity_1d(oracle):
    spec = offline.MeshSpec(1, (160,), (-1.0,), (1.0,), (capi.BC_SLIP, capi.BC_SLIP))
    off0 = offline.SyntheticOffline(spec)
    x = off0.positions[:, 0]
    U0 = np.zeros((len(x), 2))
    U0[:, 0] = np.where(x < 0.0, 1.0, 0.2)
    off, mods = _both(spec, U0, oracle, n_warm=6, equation=capi.EQ_SHALLOW_WATER)
    _compare_step(off, mods)


def test_sw_multistage_and_lake_at_rest(oracle):
    """ERK33 (step<1>, step<2> incl. the stage source terms) on the GPU vs the oracle, and the
    well-balancedness invariant: a lake at rest over an uneven bed stays at rest."""
    from ryujin_amd.initial_states import sw_circular_dam_break
    spec = offline.rectangle_2d(32, (-5.0, -5.0), (5.0, 5.0))
    off = offline.SyntheticOffline(spec)
    off.set_initial_precomputed(_bump(off.positions))
    Z = _bump(off.positions)
    U0 = sw_circular_dam_break(off.positions)
    finals = []
    for backend in ("hip", oracle.backend()):
        p = oracle.default_params(capi.EQ_SHALLOW_WATER, 2)
        p.manning_friction_coefficient = 0.02
        m = HyperbolicModule(off, p, backend=backend)
        sv = m.new_state_vector(U0)
        ti = TimeIntegrator(m, "erk 33", cfl_recovery_strategy="none")
        t = 0.0
        for _ in range(4):
            sv, tau = ti.step(sv, t)
            t += tau
        finals.append((t, sv.download()[: off.n_owned]))
    assert abs(finals[0][0] - finals[1][0]) < 1e-12 * finals[1][0]
    assert np.abs(finals[0][1] - finals[1][1]).max() < 5e-11 * np.abs(finals[1][1]).max()

    m = HyperbolicModule(off, oracle.default_params(capi.EQ_SHALLOW_WATER, 2), backend="hip")
    U_rest = np.zeros((off.n_relevant, 3))
    U_rest[:, 0] = np.maximum(1.0 - Z, 0.0)
    wet = 1.0 - Z > 0
    sv = m.new_state_vector(U_rest)
    ti = TimeIntegrator(m, "ssprk 33", cfl_recovery_strategy="none")
    t = 0.0
    for _ in range(5):
        sv, tau = ti.step(sv, t)
        t += tau
    U = sv.download()
    assert np.abs(U[wet, 0] + Z[wet] - 1.0).max() < 1e-13
    assert np.abs(U[:, 1:]).max() < 1e-13


@pytest.mark.parametrize("scheme", ["ssprk 33", "erk 33", "ssprk 22", "erk 22", "erk 11", "erk 43", "erk 54"])
def test_device_resident_time_step_equals_stagewise_driver(scheme):
    """ryujin_hip_time_step (one host synchronisation per RK step, tau kept on the device) must give
    bit-identical results to the stage-by-stage driver that mirrors TimeIntegrator::step_*."""
    spec = offline.mach3_step_2d(30)
    off = offline.SyntheticOffline(spec)
    U0 = _perturbed(euler_uniform(off.positions))
    dirichlet = euler_uniform(off.b_positions)
    m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip")
    sv = m.new_state_vector(U0)
    ti = TimeIntegrator(m, scheme, cfl_min=0.9, cfl_max=0.9, cfl_recovery_strategy="none",
                        dirichlet_fn=lambda t: dirichlet)
    t_a = 0.0
    for _ in range(5):
        sv, tau = ti.step(sv, t_a)
        t_a += tau
    ref = sv.download()

    m2 = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip")
    m2.cfl = 0.9
    state = m2.new_state_vector(U0)
    temps = [m2.new_state_vector() for _ in range({"erk 43": 4, "erk 54": 5}.get(scheme, 3))]
    t_b = 0.0
    for n in range(5):
        t_b += m2.time_step(scheme, state, temps, dirichlet if n == 0 else None)
    assert t_a == t_b
    np.testing.assert_array_equal(state.download()[: off.n_owned], ref[: off.n_owned])


def test_device_resident_time_step_bang_bang_recovery(oracle):
    """Restart is detected at the end of the RK step and the step is repeated with cfl_min, as
    TimeIntegrator::step does (time_integrator.template.h:250-274)."""
    spec = offline.rectangle_2d(24, (0.0, 0.0), (1.0, 1.0))
    off = offline.SyntheticOffline(spec)
    U0 = euler_radial_contrast(off.positions, inner=(1.0, 0.0, 1000.0), outer=(0.01, 0.0, 0.01), radius=0.3,
                               center=(0.5, 0.5))
    m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip")
    state = m.new_state_vector(U0)
    temps = [m.new_state_vector() for _ in range(3)]
    tau = m.time_step("ssprk 33", state, temps, None, cfl_recovery="bang bang control", cfl_min=0.45, cfl_max=3.0)
    assert m.n_restarts() == 1 and tau > 0.0
    assert abs(m.cfl - 0.45) < 1e-15
    # same as the stage-wise driver with the reference's try/catch
    m2 = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip")
    sv = m2.new_state_vector(U0)
    ti = TimeIntegrator(m2, "ssprk 33", cfl_min=0.45, cfl_max=3.0)
    sv, tau2 = ti.step(sv, 0.0)
    assert tau == tau2
    np.testing.assert_array_equal(state.download()[: off.n_owned], sv.download()[: off.n_owned])


def test_imported_offline_dump_is_bit_identical_on_the_gpu(tmp_path, oracle):
    """a context created from an OfflineData dump (include/ryujin_offline_io.h) computes
    exactly what the context created from the in-memory arrays computes (Euler step mesh with
    Dirichlet/slip/do-nothing boundaries and coupling pairs; shallow water with bathymetry)."""
    from ryujin_amd.initial_states import sw_circular_dam_break
    cases = []
    off = offline.SyntheticOffline(offline.mach3_step_2d(20))
    cases.append((off, capi.EQ_EULER, _perturbed(euler_uniform(off.positions)), euler_uniform(off.b_positions)))
    off = offline.SyntheticOffline(offline.rectangle_2d(40, (-5.0, -5.0), (5.0, 5.0)))
    off.set_initial_precomputed(0.2 * np.cos(off.positions[:, 0]) * np.sin(0.7 * off.positions[:, 1]))
    cases.append((off, capi.EQ_SHALLOW_WATER, sw_circular_dam_break(off.positions), None))
    for n, (off, equation, U0, dirichlet) in enumerate(cases):
        path = str(tmp_path / f"case{n}.ryjoffl")
        off.save(path)
        imp = offline.ImportedOffline(path)
        res = []
        for o in (off, imp):
            m = HyperbolicModule(o, equation=equation, backend="hip")
            m.cfl = 0.9
            a, b = m.new_state_vector(U0), m.new_state_vector()
            taus = []
            for _ in range(4):
                m.prepare_state_vector(a, 0.0, dirichlet)
                taus.append(m.step(a, [], [], b))
                a, b = b, a
            res.append((taus, a.download()))
        assert res[0][0] == res[1][0]
        assert np.array_equal(res[0][1], res[1][1])
        # ... and what it computes is what the ORACLE computes from the same dump, sweep by sweep (round 5: the f-2
        # tests compared HIP with HIP only)
        # (the dump carries the bathymetry: ryujin_hip_offline::initial_precomputed of the imported view)
        _, mods = _both(None, U0, oracle, n_warm=4, dirichlet=dirichlet, equation=equation, off=imp)
        _compare_step(imp, mods, dirichlet)


@pytest.mark.parametrize("scheme", ["erk 33", "ssprk 33"])
def test_partitioned_3d_cylinder_erk33_matches_single_rank(scheme):
    """BASELINE.json configs[3] in miniature: 3-D Mach-3 cylinder channel (staircase cylinder, Dirichlet
    inflow, do-nothing outflow, slip walls), ERK33 (the prm's scheme) and SSPRK33 (bench.py's sequence, with
    sadd over vectors whose ghosts are stale until the next prepare_state_vector) through the
    device-resident driver, x-slab partition over 2 and 4 ranks with the in-process transport: identical
    tau sequence, U to round-off."""
    import ctypes as C
    import threading

    lib = capi.load_hip()
    cpu, n_steps = 6, 3

    def prim(pos):
        return euler_uniform(pos, rho=1.4, u=3.0, p=1.0)

    def run(off, comm, out, key):
        try:
            m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip", comm=comm)
            m.cfl = 0.9
            U0 = prim(off.positions)
            U0 *= 1.0 + 1e-3 * np.sin(5.0 * off.positions[:, :1] + 3.0 * off.positions[:, 1:2] +
                                      2.0 * off.positions[:, 2:3])
            dirichlet = prim(off.b_positions) if off.n_bdry else None
            state = m.new_state_vector(U0)
            temps = [m.new_state_vector() for _ in range(3)]
            taus = [m.time_step(scheme, state, temps, dirichlet) for _ in range(n_steps)]
            out[key] = (off.global_ids[: off.n_owned].astype(np.int64), state.download()[: off.n_owned], taus)
        except Exception as e:
            out[key] = e

    ref = {}
    run(offline.SyntheticOffline(offline.cylinder_channel_3d(cpu)), None, ref, 0)
    assert not isinstance(ref[0], Exception), ref[0]
    gid, U, taus = ref[0]
    assert np.all(np.isfinite(U)) and U[:, 0].min() > 0
    scale = np.abs(U).max(axis=0)
    for n_ranks in (2, 4):
        comms = (C.c_void_p * n_ranks)()
        assert lib.ryujin_hip_comm_init_local(comms, n_ranks, 0) == 0
        parts = [offline.SyntheticOffline(offline.cylinder_channel_3d(cpu, n_ranks=n_ranks, rank=r))
                 for r in range(n_ranks)]
        out = {}
        threads = [threading.Thread(target=run, args=(parts[r], C.c_void_p(comms[r]), out, r))
                   for r in range(n_ranks)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
            assert not t.is_alive(), "rank thread hung"
        for r in range(n_ranks):
            assert not isinstance(out[r], Exception), out[r]
            assert np.allclose(out[r][2], taus, rtol=1e-13, atol=0)
        g = np.concatenate([out[r][0] for r in range(n_ranks)])
        Up = np.concatenate([out[r][1] for r in range(n_ranks)])
        o1, o2 = np.argsort(gid), np.argsort(g)
        assert np.array_equal(gid[o1], g[o2])
        assert (np.abs(Up[o2] - U[o1]) / scale).max() < 1e-11
        for r in range(n_ranks):
            lib.ryujin_hip_comm_destroy(C.c_void_p(comms[r]))


# ------------------------------------------------------------------ Euler with arbitrary equation of state

def _aeos_edit(eos=capi.EOS_POLYTROPIC_GAS, strict=True, **kw):
    def edit(p):
        p.eos = eos
        p.compute_strict_bounds = 1 if strict else 0
        for k, v in kw.items():
            setattr(p, k, v)
    return edit


@pytest.mark.parametrize("strict", [True, False])
def test_aeos_step_parity_2d_step_geometry(oracle, strict):
    """EulerAEOS Description (source/euler_aeos/), polytropic gas EOS, Mach-3 forward-facing step with
    developed shocks: four precomputed values after two cycles, surrogate-gamma Riemann solver,
    indicator, four limiter bounds, both `compute strict bounds` settings."""
    spec = offline.mach3_step_2d(40)
    off0 = offline.SyntheticOffline(spec)
    U0 = _perturbed(euler_uniform(off0.positions))
    dirichlet = euler_uniform(off0.b_positions)
    off, mods = _both(spec, U0, oracle, n_warm=12, dirichlet=dirichlet, equation=capi.EQ_EULER_AEOS,
                      params_edit=_aeos_edit(strict=strict))
    g, c = _compare_step(off, mods, dirichlet)
    assert g["prec"].shape[1] == 4 and g["bounds"].size == off.n_owned * 4
    n = off.n_owned
    # polytropic gas: precomputed p equals (gamma-1) rho e; gamma_min == 1.4 up to round-off
    rho_e = g["U_old"][:n, 3] - 0.5 * (g["U_old"][:n, 1:3] ** 2).sum(1) / g["U_old"][:n, 0]
    np.testing.assert_allclose(g["prec"][:n, 0], 0.4 * rho_e, rtol=1e-13)
    assert np.abs(g["prec"][:n, 1] - 1.4).max() < 1e-12
    assert (g["U"][:n, 0] > 0).all()


@pytest.mark.parametrize("eos_name", ["nasg", "vdw", "jwl"])
def test_aeos_step_parity_equations_of_state(oracle, eos_name):
    """Noble-Abel stiffened gas, van der Waals and Jones-Wilkins-Lee equations of state (non-trivial
    interpolation b, pinf, q; varying surrogate gamma): radial pressure/density contrast in a slip box."""
    from ryujin_amd.initial_states import aeos_from_primitive
    eos_kw = {
        "nasg": dict(eos=capi.EOS_NOBLE_ABEL_STIFFENED_GAS, eos_covolume_b=0.05, eos_pinf=0.5, eos_q=0.1),
        "vdw": dict(eos=capi.EOS_VAN_DER_WAALS, eos_covolume_b=0.1, eos_vdw_a=0.01),
        "jwl": dict(eos=capi.EOS_JONES_WILKINS_LEE, jwl_A=1.0, jwl_B=-0.1, jwl_R1=4.0, jwl_R2=1.0,
                    jwl_omega=0.4, jwl_rho_0=1.0, jwl_q_0=0.0, jwl_cv=1.0),
    }[eos_name]
    edit = _aeos_edit(**eos_kw)
    spec = offline.rectangle_2d(48, (-1.0, -1.0), (1.0, 1.0))
    off0 = offline.SyntheticOffline(spec)
    p = oracle.default_params(capi.EQ_EULER_AEOS, 2)
    edit(p)
    r = np.linalg.norm(off0.positions, axis=1)
    rho = np.where(r < 0.4, 2.0, 1.0)
    pr = np.where(r < 0.4, 10.0, 1.0)
    U0 = _perturbed(aeos_from_primitive(p, rho, np.zeros((off0.n_relevant, 2)), pr))
    off, mods = _both(spec, U0, oracle, n_warm=15, equation=capi.EQ_EULER_AEOS, params_edit=edit)
    g, c = _compare_step(off, mods)
    n = off.n_owned
    assert np.ptp(g["prec"][:n, 1]) > 1e-3 or eos_name == "nasg"   # the surrogate gamma varies
    assert (g["U"][:n, 0] > 0).all()


def test_aeos_step_parity_1d_and_3d(oracle, dims=(1, 3)):
    from ryujin_amd.initial_states import aeos_from_primitive
    edit = _aeos_edit(eos=capi.EOS_NOBLE_ABEL_STIFFENED_GAS, eos_covolume_b=0.1, eos_pinf=0.2, eos_q=0.05)
    for dim in dims:
        if dim == 1:
            spec = offline.MeshSpec(1, (200,), (0.0,), (1.0,), (capi.BC_DIRICHLET, capi.BC_DO_NOTHING))
        else:
            spec = offline.box_3d(10)
        off0 = offline.SyntheticOffline(spec)
        p = oracle.default_params(capi.EQ_EULER_AEOS, dim)
        edit(p)
        x = off0.positions
        inner = (x[:, 0] < 0.5) if dim == 1 else (np.linalg.norm(x, axis=1) < 0.4)
        U0 = aeos_from_primitive(p, np.where(inner, 1.0, 0.125), np.zeros((len(x), dim)), np.where(inner, 1.0, 0.1))
        dirichlet = U0[off0.b_i] if dim == 1 else None
        off, mods = _both(spec, U0, oracle, n_warm=8, dirichlet=dirichlet, equation=capi.EQ_EULER_AEOS,
                          params_edit=edit)
        _compare_step(off, mods, dirichlet)


@pytest.mark.parametrize("scheme", ["ssprk 33", "erk 33"])
def test_aeos_isentropic_vortex_golden_on_gpu(golden_dir, scheme):
    """tests/euler_aeos/verification-isentropic_vortex-pge-2d-*-l5 on the GPU (ERK33: multi-stage fluxes
    from the stage vectors' precomputed pressures)."""
    from test_oracle_golden_integration import _golden_vortex, run_isentropic_vortex
    prefix = "euler_aeos_verification-isentropic_vortex-pge-2d"
    dofs, t_ref, linf_ref, l1_ref, l2_ref = _golden_vortex(golden_dir, scheme, 5, prefix)
    t, linf, l1, l2, n = run_isentropic_vortex("hip", scheme, 5, equation=capi.EQ_EULER_AEOS)
    assert n == dofs
    assert abs(t - t_ref) < 1e-10
    assert abs(linf - linf_ref) < 1e-8 * linf_ref
    assert abs(l1 - l1_ref) < 1e-8 * l1_ref
    assert abs(l2 - l2_ref) < 1e-8 * l2_ref


def test_aeos_rejects_what_the_reference_does_not_implement():
    """`dynamic` boundary conditions are __builtin_trap() in euler_aeos/hyperbolic_system.h:1337."""
    spec = offline.rectangle_2d(8, bc=(capi.BC_DYNAMIC, capi.BC_SLIP, capi.BC_SLIP, capi.BC_SLIP))
    off = offline.SyntheticOffline(spec)
    with pytest.raises(RuntimeError, match="dynamic"):
        HyperbolicModule(off, equation=capi.EQ_EULER_AEOS, backend="hip")


def test_device_integrals_conservation_monitor():
    """ryujin_hip_state_integrals (Quantities-style interior integrals): equals
    sum_i m_i U_i computed on the host to round-off, is bitwise reproducible, stays constant to 1e-13 over
    SSPRK33 steps in a closed box, and the partitioned run (collective sum over 3 in-process ranks)
    agrees with the single-rank value."""
    import ctypes as C
    import threading
    spec = offline.rectangle_2d(64, (0.0, 0.0), (1.0, 1.0))
    off = offline.SyntheticOffline(spec)
    U0 = euler_radial_contrast(off.positions, inner=(1.0, 0.0, 10.0), outer=(0.5, 0.0, 1.0), radius=0.3,
                               center=(0.5, 0.5))
    m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip")
    m.cfl = 0.9
    state = m.new_state_vector(U0)
    I0 = m.integrals(state)
    ref = (off.mi[: off.n_owned, None] * U0[: off.n_owned]).sum(axis=0)
    np.testing.assert_allclose(I0, ref, rtol=1e-13)
    assert np.array_equal(I0, m.integrals(state))
    temps = [m.new_state_vector() for _ in range(3)]
    for _ in range(10):
        m.time_step("ssprk 33", state, temps)
    I1 = m.integrals(state)
    assert np.abs(I1[[0, 3]] - I0[[0, 3]]).max() <= 1e-13 * np.abs(I0[[0, 3]]).max()   # mass, energy
    # momentum is not conserved at slip walls, but symmetric data keep it at round-off of the mass scale
    assert np.abs(I1[1:3]).max() <= 1e-10

    n_ranks = 3
    lib = capi.load_hip()
    comms = (C.c_void_p * n_ranks)()
    assert lib.ryujin_hip_comm_init_local(comms, n_ranks, 0) == 0
    parts = [offline.SyntheticOffline(offline.rectangle_2d(64, (0.0, 0.0), (1.0, 1.0), n_ranks=n_ranks, rank=r))
             for r in range(n_ranks)]
    out = {}

    def run(r):
        try:
            o = parts[r]
            mm = HyperbolicModule(o, equation=capi.EQ_EULER, backend="hip", comm=C.c_void_p(comms[r]))
            sv = mm.new_state_vector(euler_radial_contrast(o.positions, inner=(1.0, 0.0, 10.0),
                                                           outer=(0.5, 0.0, 1.0), radius=0.3, center=(0.5, 0.5)))
            out[r] = mm.integrals(sv)
        except Exception as e:
            out[r] = e
    threads = [threading.Thread(target=run, args=(r,)) for r in range(n_ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
        assert not t.is_alive()
    for r in range(n_ranks):
        assert not isinstance(out[r], Exception), out[r]
        np.testing.assert_allclose(out[r], I0, rtol=1e-13)
        assert np.array_equal(out[r], out[0])
    for r in range(n_ranks):
        lib.ryujin_hip_comm_destroy(C.c_void_p(comms[r]))


@pytest.mark.parametrize("scheme", ["erk 43", "erk 54"])
def test_erk43_erk54_parity_with_the_oracle(oracle, scheme):
    """step<1> ... step<4> with the ERK43 / ERK54 stage vectors and weights (time_integrator.template.h:405-510):
    the flow is developed by two Runge-Kutta steps on the GPU, then every stage of the third one is compared with
    the oracle ON IDENTICAL INPUTS through compare_step -- all intermediates, the stated per-update contract, l_ij
    outliers classified -- and the oracle's stage result is handed to both backends for the next stage."""
    spec = offline.mach3_step_2d(20)
    dirichlet = euler_uniform(offline.SyntheticOffline(spec).b_positions)
    off, mods = _both(spec, _perturbed(euler_uniform(offline.SyntheticOffline(spec).positions)), oracle,
                      dirichlet=dirichlet)
    (mg, og, ng), (mc, oc, nc) = mods
    ti = TimeIntegrator(mg, scheme, cfl_min=0.9, cfl_max=0.9, cfl_recovery_strategy="none",
                        dirichlet_fn=lambda t: dirichlet)
    sv, t = og, 0.0
    for _ in range(2):
        sv, tau = ti.step(sv, t)
        t += tau
    U_start = sv.download()
    # stage table: (indices of the stage vectors among [U, T0, T1, ...], weights) -- TimeIntegrator._erk43/_erk54
    a = TimeIntegrator.ERK54
    c54 = a["c"]
    table = {"erk 43": [((), ()), ((0,), (-1.0,)), ((1,), (-1.0,)), ((1, 2), (5.0 / 3.0, -10.0 / 3.0))],
             "erk 54": [((), ()), ((0,), ((a["a_31"] - a["a_21"]) / c54,)),
                        ((0, 1), ((a["a_41"] - a["a_31"]) / c54, (a["a_42"] - a["a_32"]) / c54)),
                        ((0, 1, 2), ((a["a_51"] - a["a_41"]) / c54, (a["a_52"] - a["a_42"]) / c54,
                                     (a["a_53"] - a["a_43"]) / c54)),
                        ((0, 1, 2, 3), ((a["a_61"] - a["a_51"]) / c54, (a["a_62"] - a["a_52"]) / c54,
                                        (a["a_63"] - a["a_53"]) / c54, (a["a_64"] - a["a_54"]) / c54))]}[scheme]
    vec = {id(mg): [mg.new_state_vector(U_start)], id(mc): [mc.new_state_vector(U_start)]}
    tau = 0.0
    for stage, (idx, weights) in enumerate(table):
        for m in (mg, mc):
            vec[id(m)].append(m.new_state_vector())
            for q in idx:   # stage vectors must be prepared state vectors (hyperbolic_module.h:207-213)
                m.prepare_state_vector(vec[id(m)][q], 0.0, dirichlet)
        step_mods = _Mods([(mg, vec[id(mg)][stage], vec[id(mg)][stage + 1]),
                           (mc, vec[id(mc)][stage], vec[id(mc)][stage + 1])])
        step_mods.oracle, step_mods.params = mods.oracle, mods.params
        g, c = _compare_step(off, step_mods, dirichlet, tau,
                             stage_vectors=([vec[id(mg)][q] for q in idx], [vec[id(mc)][q] for q in idx]),
                             stage_weights=weights)
        tau = c["tau"]
        vec[id(mg)][stage + 1].upload(vec[id(mc)][stage + 1].download())   # identical inputs for the next stage


# ------------------------------------------------------------------ scalar conservation equations

def _scalar_both(off, U0, oracle, edit, n_warm=0, dirichlet=None):
    dim = off.dim
    mods = []
    U_start = U0
    for backend in ("hip", oracle.backend()):
        p = oracle.default_params(capi.EQ_SCALAR_CONSERVATION, dim)
        p.cfl = 0.9
        edit(p)
        m = HyperbolicModule(off, p, backend=backend)
        old, new = m.new_state_vector(U_start), m.new_state_vector()
        if backend == "hip":
            for _ in range(n_warm):
                m.prepare_state_vector(old, 0.0, dirichlet)
                m.step(old, [], [], new)
                old, new = new, old
            U_start = old.download()
        mods.append((m, old, new))
    return mods


def _scalar_compare(off, mods, dirichlet=None, stages=(), weights=(), tau=0.0, noisy_flux=False):
    """noisy_flux: the flux is transcendental (KPP: sin, cos differ in the last bit between ocml and libm).
    The Roe average |f_i - f_j| / max(|u_i - u_j|, 2 delta) with delta = 1e4 eps amplifies a last-bit
    difference of f by 1/(2e4 eps) wherever the state is constant -- by design of the reference
    (riemann_solver.template.h:48-49) -- so d_ij and tau are compared to 1e-4 there and the rest of the
    update is compared at the SAME tau."""
    if noisy_flux and tau == 0.0:
        taus = []
        for m, old, new in mods:
            m.prepare_state_vector(old, 0.0, dirichlet)
            taus.append(m.step(old, list(stages), list(weights), new, 0.0))
        assert abs(taus[0] - taus[1]) <= 1e-4 * taus[1]
        tau = taus[1]
    out = []
    for m, old, new in mods:
        m.prepare_state_vector(old, 0.0, dirichlet)
        tau_used = m.step(old, list(stages), list(weights), new, tau)
        out.append(dict(tau=tau_used, prec=old.download_precomputed(), U=new.download(), alpha=m.alpha(),
                        dij=m.debug_fetch("dij"), lij=m.debug_fetch("lij"), pij=m.debug_fetch("pij"),
                        bounds=m.debug_fetch("bounds"), r=m.debug_fetch("r"),
                        lij_next=m.debug_fetch("lij_next"), status=m.last_status))
    g, c = out
    n = off.n_owned
    active = np.diff(np.asarray(off._keep["row_starts"] if hasattr(off, "_keep") else off.row_starts).astype(np.int64))[:n] > 1
    scale = np.abs(c["U"][:n]).max()
    rs_diag = np.asarray(off._keep["row_starts"] if hasattr(off, "_keep") else off.row_starts).astype(np.int64)[:n]
    assert g["status"] == c["status"]
    np.testing.assert_allclose(g["prec"][:n][active], c["prec"][:n][active], rtol=1e-13, atol=1e-15 * scale)
    assert np.abs(g["alpha"][:n][active] - c["alpha"][:n][active]).max() <= (1e-9 if noisy_flux else 1e-12)
    np.testing.assert_allclose(g["dij"], c["dij"], rtol=1e-12,
                               atol=1e-4 * np.abs(c["dij"]).max() if noisy_flux else 1e-300)
    assert abs(g["tau"] - c["tau"]) <= 1e-12 * c["tau"]
    np.testing.assert_allclose(g["bounds"].reshape(n, -1)[active], c["bounds"].reshape(n, -1)[active], rtol=1e-12,
                               atol=1e-14 * scale)
    # r_i, P_ij: 1e-12 of the largest entry (the contract of helpers_parity.py; the never-read diagonal P_ii aside)
    assert np.abs(g["r"] - c["r"]).max() <= 1e-12 * max(np.abs(c["r"]).max(), 1e-300)
    g["pij"][rs_diag] = c["pij"][rs_diag]
    assert np.abs(g["pij"] - c["pij"]).max() <= 1e-12 * max(np.abs(c["pij"]).max(), 1e-300)
    # l_ij of the scalar limiter is a quotient (u_max - u) / P_ij: where P_ij is round-off sized it is undefined in
    # the reference itself. Every pair beyond 1e-10 must be inert: |dl| lambda |P_ij| below the U_new contract.
    rs_ = np.asarray(off._keep["row_starts"] if hasattr(off, "_keep") else off.row_starts).astype(np.int64)[: n + 1]
    lam = np.repeat(1.0 / np.maximum(np.diff(rs_) - 1, 1), np.diff(rs_))
    for name in ("lij", "lij_next"):
        dl = np.abs(g[name] - c[name])
        effect = dl * lam * np.abs(c["pij"]) / scale
        assert effect[dl > 1e-10].max(initial=0.0) <= 1e-12, (name, float(effect[dl > 1e-10].max(initial=0.0)))
    err = np.abs(g["U"][:n] - c["U"][:n]) / scale
    assert err.max() <= 1e-12, err.max()
    return g, c


def test_scalar_linear_transport_parity_periodic_1d(oracle):
    """Scalar conservation (source/scalar_conservation/), 'function' flux u with its central-difference
    gradient, periodic interval with a constrained DoF (row of length 1): one update and an ERK33 stage
    with stage vectors compared sweep by sweep."""
    from test_oracle_golden_scalar import periodic_interval
    off, h = periodic_interval(256, 6.28318530718)

    def edit(p):
        p.sc_flux = capi.FLUX_POLYNOMIAL
        for d in range(3):
            for n in range(4):
                p.sc_flux_polynomial[d][n] = 0.0
        p.sc_flux_polynomial[0][1] = 1.0
        p.indicator_evc_factor = 1.0
    x = off.positions
    U0 = np.sin(x - 1.0) + 0.3 * np.sign(np.sin(3 * x))   # smooth + jumps: limiter and indicator active
    mods = _scalar_both(off, U0, oracle, edit, n_warm=6)
    _scalar_compare(off, mods)


@pytest.mark.parametrize("flux", ["burgers", "kpp"])
def test_scalar_parity_2d(oracle, flux):
    """Burgers and KPP fluxes in 2-D with Dirichlet boundaries, greedy wavespeed off and on with the
    averaged Kruzkov entropy (riemann_solver.template.h:60-140)."""
    spec = offline.rectangle_2d(48, (-2.0, -2.5), (2.0, 1.5), bc=capi.BC_DIRICHLET)
    off = offline.SyntheticOffline(spec)
    r = np.linalg.norm(off.positions, axis=1)
    # KPP rotating-wave data, shifted off the values where f'(u).n vanishes for a stencil direction
    # (u = pi/4, 3.5 pi: there d_ij is pure round-off and the bar states c_ij/d_ij (f_j - f_i) are
    # 0/0 in the reference as well)
    u0 = np.where(r < 1.0, 3.4 * np.pi, 0.3 * np.pi) if flux == "kpp" else np.where(r < 1.0, 1.0, -0.5)
    U0 = u0.reshape(-1, 1)
    dirichlet = U0[off.b_i]
    for greedy, averaged in ((0, 0), (1, 1)):
        def edit(p):
            p.sc_flux = capi.FLUX_KPP if flux == "kpp" else capi.FLUX_BURGERS
            p.sc_use_greedy_wavespeed = greedy
            p.sc_use_averaged_entropy = averaged
        mods = _scalar_both(off, U0, oracle, edit, n_warm=10, dirichlet=dirichlet)
        _scalar_compare(off, mods, dirichlet, noisy_flux=(flux == "kpp"))


@pytest.mark.parametrize("scheme", ["ssprk 22", "ssprk 33", "erk 11", "erk 22", "erk 33", "erk 43", "erk 54"])
def test_scalar_linear_transport_golden_on_gpu(golden_dir, scheme):
    """tests/scalar_conservation/verification-linear_transport-*.output on the GPU: every explicit
    Runge-Kutta scheme of the reference's TimeIntegrator against the reference's own numbers."""
    from test_oracle_golden_scalar import golden_linear_transport, run_linear_transport

    def default_params(equation, dim):
        p = capi.Params()
        capi.load_hip().ryujin_hip_default_params(p, equation, dim)
        return p
    dofs, t_ref, linf_ref, l1_ref, l2_ref = golden_linear_transport(golden_dir, scheme)
    t, linf, l1, l2, n, _ = run_linear_transport("hip", scheme, default_params=default_params)
    assert n == dofs
    assert abs(t - t_ref) < 1e-10
    assert abs(linf - linf_ref) < 2e-5 * linf_ref
    assert abs(l1 - l1_ref) < 2e-5 * l1_ref
    assert abs(l2 - l2_ref) < 2e-5 * l2_ref


def test_scalar_rejects_what_the_reference_rejects():
    spec = offline.rectangle_2d(8, bc=capi.BC_SLIP)
    off = offline.SyntheticOffline(spec)
    with pytest.raises(RuntimeError, match="unavailable for scalar conservation"):
        HyperbolicModule(off, equation=capi.EQ_SCALAR_CONSERVATION, backend="hip")


def test_wide_ragged_stencil_generic_kernels(oracle):
    """Stencils wider than anything a Q1 mesh produces (up to 49 entries per row, strongly ragged near
    the boundary): exercises the generic, non-unrolled sweeps (k_dij_alpha, k_dij_diag, the two-pass
    k_high_order) and the 64-entry limit of a SELL-64 slice. The matrices are synthetic but consistent
    (c_ij = -c_ji, m_ij = m_ji > 0, m_i = sum_j m_ij), which is all step() relies on: the lattice generator of
    tests/helpers_row_width.py."""
    import helpers_row_width as rw
    # 7 x 7 stencils, 49 entries in the interior, on a 24 x 24 lattice open in both directions
    off = rw.lattice_offline((24, 24), 49, open_axes=(0, 1), norm="max")
    rows = np.split(off.columns, off.row_starts[1:-1].astype(np.int64))
    assert max(len(r) for r in rows) == 49 and min(len(r) for r in rows) == 16
    pos = off.positions
    U0 = _perturbed(euler_radial_contrast(pos, inner=(1.0, 0.0, 5.0), outer=(0.5, 0.0, 0.5), radius=0.25,
                                          center=(0.5, 0.5)))
    mods = []
    U_start = U0
    for backend in ("hip", oracle.backend()):
        m = HyperbolicModule(off, equation=capi.EQ_EULER, backend=backend)
        m.cfl = 0.5
        old, new = m.new_state_vector(U_start), m.new_state_vector()
        if backend == "hip":
            for _ in range(5):
                m.prepare_state_vector(old, 0.0)
                m.step(old, [], [], new)
                old, new = new, old
            U_start = old.download()
        mods.append((m, old, new))
    _compare_step(off, mods)


def test_discontinuous_ansatz_branch(oracle, tmp_path):
    """have_discontinuous_ansatz (hyperbolic_module.template.h:733-737, 938-948, 976-986):
    incidence matrix in the high-order viscosity, limiter bounds extended over the stencil, full inverse
    mass matrix instead of the Neumann series. Finite-volume-like (dG Q0) couplings on a Cartesian grid:
    c_ij = n_ij |F_ij| / 2 across faces, incidence (m_ij-average / |Omega|)^(1/4); the inverse mass matrix
    gets synthetic symmetric off-diagonal entries so that the b_ij F_j - b_ji F_i term is exercised.
    Also checks that the dump format carries the two extra matrices."""
    from helpers_layout import OfflineView
    nx = ny = 32
    h = 1.0 / nx
    idx = lambda ix, iy: iy * nx + ix       # noqa: E731
    rows, cij, mij, inc, minv = [], [], [], [], []
    r_ij = (h * h / 1.0) ** (0.5 / 2)
    for iy in range(ny):
        for ix in range(nx):
            i = idx(ix, iy)
            nb = []
            for (dx, dy) in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                jx, jy = ix + dx, iy + dy
                if 0 <= jx < nx and 0 <= jy < ny:
                    nb.append((idx(jx, jy), (0.5 * h * dx, 0.5 * h * dy)))
            nb.sort()
            cii = (-sum(c[0] for _, c in nb), -sum(c[1] for _, c in nb))
            rows.append([i] + [j for j, _ in nb])
            cij.extend([cii] + [c for _, c in nb])
            mij.extend([h * h] + [0.0] * len(nb))
            inc.extend([0.0] + [r_ij] * len(nb))
            minv.extend([1.0 / (h * h)] + [-0.1 / (h * h)] * len(nb))
    n = nx * ny
    row_starts = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    columns = np.concatenate([np.array(r, dtype=np.uint32) for r in rows])
    mi = np.full(n, h * h)
    off = OfflineView(2, 0, 0, n, n, 1, row_starts, columns, np.array(cij), np.array(mij), mi, 1.0 / mi, 1.0,
                      [], np.zeros((0, 2)), [], [], [], [])
    off._dg = (np.ascontiguousarray(inc), np.ascontiguousarray(minv))
    off._o.discontinuous_ansatz = 1
    off._o.incidence = capi.as_ptr(off._dg[0], capi.c_double_p)
    off._o.mass_matrix_inverse = capi.as_ptr(off._dg[1], capi.c_double_p)
    off.row_starts = row_starts
    pos = np.array([[(ix + 0.5) * h, (iy + 0.5) * h] for iy in range(ny) for ix in range(nx)])
    U0 = _perturbed(euler_radial_contrast(pos, inner=(1.0, 0.0, 5.0), outer=(0.5, 0.0, 0.5), radius=0.25,
                                          center=(0.5, 0.5)))

    def run_pair(o):
        mods = []
        U_start = U0
        for backend in ("hip", oracle.backend()):
            m = HyperbolicModule(o, equation=capi.EQ_EULER, backend=backend)
            m.cfl = 0.5
            old, new = m.new_state_vector(U_start), m.new_state_vector()
            if backend == "hip":
                for _ in range(6):
                    m.prepare_state_vector(old, 0.0)
                    m.step(old, [], [], new)
                    old, new = new, old
                U_start = old.download()
            mods.append((m, old, new))
        return mods
    g, c = _compare_step(off, run_pair(off))

    # the branch really is different from the continuous one
    off._o.discontinuous_ansatz = 0
    m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip")
    m.cfl = 0.5
    a, b = m.new_state_vector(g["U_old"]), m.new_state_vector()
    m.prepare_state_vector(a, 0.0)
    m.step(a, [], [], b)
    assert np.abs(b.download() - g["U"]).max() > 1e-6
    off._o.discontinuous_ansatz = 1

    # dump round trip keeps the two matrices
    lib = capi.load_synth()
    path = str(tmp_path / "dg.ryjoffl")
    assert lib.ryujin_offline_write(path.encode(), off.c, 2, 0, None, None) == 0
    imp = offline.ImportedOffline(path)
    assert imp.c.contents.discontinuous_ansatz == 1
    assert np.array_equal(capi.np_from_ptr(imp.c.contents.incidence, imp.nnz, np.float64), off._dg[0])
    assert np.array_equal(capi.np_from_ptr(imp.c.contents.mass_matrix_inverse, imp.nnz, np.float64), off._dg[1])
    m2 = HyperbolicModule(imp, equation=capi.EQ_EULER, backend="hip")
    m2.cfl = 0.5
    a2, b2 = m2.new_state_vector(g["U_old"]), m2.new_state_vector()
    m2.prepare_state_vector(a2, 0.0)
    m2.step(a2, [], [], b2)
    assert np.array_equal(b2.download(), g["U"])


def test_partitioned_bang_bang_recovery_is_collective():
    """Device-resident RK step on 3 in-process ranks with a violation that happens on ONE rank only
    (off-centre blast): the flags accumulated over the stages are OR-ed over the ranks once per RK step, so
    every rank restarts with cfl_min together and the result equals the single-rank run."""
    import ctypes as C
    import threading
    lib = capi.load_hip()

    def initial(off):
        return euler_radial_contrast(off.positions, inner=(1.0, 0.0, 1000.0), outer=(0.01, 0.0, 0.01),
                                     radius=0.12, center=(0.15, 0.5))

    def run(off, comm, out, key):
        try:
            m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip", comm=comm)
            state = m.new_state_vector(initial(off))
            temps = [m.new_state_vector() for _ in range(3)]
            taus = [m.time_step("ssprk 33", state, temps, None, cfl_recovery="bang bang control", cfl_min=0.45,
                                cfl_max=3.0) for _ in range(2)]
            out[key] = (off.global_ids[: off.n_owned].astype(np.int64), state.download()[: off.n_owned], taus,
                        m.n_restarts(), m.cfl)
        except Exception as e:
            out[key] = e

    ref = {}
    run(offline.SyntheticOffline(offline.rectangle_2d(36, (0.0, 0.0), (1.0, 1.0))), None, ref, 0)
    assert not isinstance(ref[0], Exception), ref[0]
    gid, U, taus, n_restarts, cfl = ref[0]
    assert n_restarts >= 1 and abs(cfl - 0.45) < 1e-15
    n_ranks = 3
    comms = (C.c_void_p * n_ranks)()
    assert lib.ryujin_hip_comm_init_local(comms, n_ranks, 0) == 0
    parts = [offline.SyntheticOffline(offline.rectangle_2d(36, (0.0, 0.0), (1.0, 1.0), n_ranks=n_ranks, rank=r))
             for r in range(n_ranks)]
    out = {}
    threads = [threading.Thread(target=run, args=(parts[r], C.c_void_p(comms[r]), out, r)) for r in range(n_ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
        assert not t.is_alive(), "rank thread hung"
    for r in range(n_ranks):
        assert not isinstance(out[r], Exception), out[r]
        assert np.allclose(out[r][2], taus, rtol=1e-13, atol=0)
        assert out[r][3] == n_restarts and abs(out[r][4] - 0.45) < 1e-15
    g = np.concatenate([out[r][0] for r in range(n_ranks)])
    Up = np.concatenate([out[r][1] for r in range(n_ranks)])
    o1, o2 = np.argsort(gid), np.argsort(g)
    scale = np.abs(U).max(axis=0)
    assert (np.abs(Up[o2] - U[o1]) / scale).max() < 1e-10
    for r in range(n_ranks):
        lib.ryujin_hip_comm_destroy(C.c_void_p(comms[r]))


@pytest.mark.parametrize("iterations", [0, 1])
def test_limiter_iterations_0_and_1(oracle, iterations):
    """'limiter iterations' = 0 (low-order update only: steps 5-7 are skipped, :892, :1053) and 1 (a single
    high-order pass): the module allows [0, 2] (hyperbolic_module.template.h:246-249)."""
    spec = offline.mach3_step_2d(30)
    off0 = offline.SyntheticOffline(spec)
    U0 = _perturbed(euler_uniform(off0.positions))
    dirichlet = euler_uniform(off0.b_positions)

    def edit(p):
        p.limiter_iterations = iterations
    off, mods = _both(spec, U0, oracle, n_warm=8, dirichlet=dirichlet, params_edit=edit)
    _compare_step(off, mods, dirichlet)   # the stated contract, l_ij outliers classified, no quota


def test_riemann_newton_iterations_and_tau_max(oracle):
    """'riemann solver / newton max iterations' = 2 (quadratic Newton refinement of the two-rarefaction
    guess, riemann_solver.template.h:540-575) through a whole step, and the tau_max argument of step()
    clipping the CFL time step (tau = min(tau_max, CFL tau), :571-578; TimeLoop's final step)."""
    spec = offline.mach3_step_2d(30)
    off0 = offline.SyntheticOffline(spec)
    U0 = _perturbed(euler_uniform(off0.positions))
    dirichlet = euler_uniform(off0.b_positions)

    def edit(p):
        p.riemann_newton_max_iterations = 2
    off, mods = _both(spec, U0, oracle, n_warm=8, dirichlet=dirichlet, params_edit=edit)
    g, c = _compare_step(off, mods, dirichlet)
    # the refined wavespeeds are never larger than the unrefined upper bound
    off_b, mods_b = _both(spec, g["U_old"], oracle, dirichlet=dirichlet)
    g0, _ = _compare_step(off_b, mods_b, dirichlet)
    offd = g0["dij"] > 0.0   # off-diagonal entries (d_ii = -sum_j d_ij < 0)
    assert (g["dij"][offd] <= g0["dij"][offd] * (1 + 1e-12)).all()
    assert (g["dij"][offd] < g0["dij"][offd] * (1 - 1e-6)).any()
    for m, old, new in mods:
        m.prepare_state_vector(old, 0.0, dirichlet)
        assert m.step(old, [], [], new, 0.0, 1e-7) == 1e-7
        with pytest.raises(Exception):
            m.step(old, [], [], new, 0.0, -1.0)       # AssertThrow at :573-576


@pytest.mark.parametrize("gamma", [1.3, 5.0 / 3.0, 2.0])
def test_step_parity_other_ratios_of_specific_heats(oracle, gamma):
    """The Riemann sweep evaluates p_star_two_rarefaction's exponent 2 gamma / (gamma - 1) by multiplications
    when it is integral (7/5 -> 7, 5/3 -> 5, 2 -> 4) and with pow otherwise (1.3 -> 8.67: the general kernel,
    split from the indicator sweep). Every path against the oracle, developed flow in 2-D and 3-D."""
    from ryujin_amd.initial_states import euler_from_primitive

    def edit(p):
        p.gamma = gamma

    spec = offline.mach3_step_2d(30)
    off0 = offline.SyntheticOffline(spec)

    def prim(pos):   # Mach 3 for this gamma
        n = len(pos)
        v = np.zeros((n, pos.shape[1]))
        v[:, 0] = 3.0
        return euler_from_primitive(np.full(n, gamma), v, np.ones(n), gamma=gamma)
    U0 = _perturbed(prim(off0.positions))
    dirichlet = prim(off0.b_positions)
    off, mods = _both(spec, U0, oracle, n_warm=10, dirichlet=dirichlet, params_edit=edit)
    _compare_step(off, mods, dirichlet)

    spec3 = offline.box_3d(10)
    off3 = offline.SyntheticOffline(spec3)
    U3 = euler_radial_contrast(off3.positions, radius=0.4, gamma=gamma)
    off, mods = _both(spec3, U3, oracle, n_warm=4, params_edit=edit)
    _compare_step(off, mods)


@pytest.mark.parametrize("kinetic,square", [(1, 0), (1, 1), (0, 0)])
def test_sw_limiter_options(oracle, kinetic, square):
    """Shallow-water limiter with 'limit on kinetic energy' / 'limit on square velocity' in the three
    non-default combinations (shallow_water/limiter.h:51-59, limiter.template.h:120-449)."""
    from ryujin_amd.initial_states import sw_circular_dam_break
    spec = offline.rectangle_2d(40, (-5.0, -5.0), (5.0, 5.0))
    off0 = offline.SyntheticOffline(spec)
    U0 = sw_circular_dam_break(off0.positions, h_outer=0.5)

    def edit(p):
        p.limiter_limit_on_kinetic_energy = kinetic
        p.limiter_limit_on_square_velocity = square
    off, mods = _both(spec, U0, oracle, n_warm=10, equation=capi.EQ_SHALLOW_WATER, params_edit=edit)
    g, c = _compare_step(off, mods)
    assert (g["U"][: off.n_owned, 0] > 0.0).all()


@pytest.mark.parametrize("mach", [0.5, 3.0])
def test_euler_dynamic_and_no_slip_boundaries(oracle, mach):
    """Boundary ids `dynamic` (sub-/supersonic in- and outflow via Riemann
    characteristics, euler/hyperbolic_system.h:1040-1159) and `no_slip` through whole updates."""
    spec = offline.rectangle_2d(40, (0.0, 0.0), (2.0, 1.0), ny=20,
                                bc=(capi.BC_DYNAMIC, capi.BC_DYNAMIC, capi.BC_NO_SLIP, capi.BC_SLIP))
    off0 = offline.SyntheticOffline(spec)
    U0 = _perturbed(euler_uniform(off0.positions, rho=1.4, u=mach, p=1.0))      # speed of sound 1
    dirichlet = euler_uniform(off0.b_positions, rho=1.4, u=mach, p=1.0)
    ids = set(int(b) for b in off0.b_id)
    assert capi.BC_DYNAMIC in ids and capi.BC_NO_SLIP in ids
    off, mods = _both(spec, U0, oracle, n_warm=10, dirichlet=dirichlet)
    g, c = _compare_step(off, mods, dirichlet)
    # no-slip rows carry no momentum after the boundary pass
    ns = off.b_i[off.b_id == capi.BC_NO_SLIP]
    assert np.abs(g["U_old"][ns, 1:3]).max() == 0.0


@pytest.mark.parametrize("u", [0.5, 6.0])
def test_sw_dynamic_dirichlet_momentum_no_slip_boundaries(oracle, u):
    """Shallow-water boundary ids `dynamic` (sub- and supercritical), `dirichlet momentum` and `no_slip`
    (shallow_water/hyperbolic_system.h:905-1015) through whole updates."""
    spec = offline.rectangle_2d(40, (0.0, 0.0), (2.0, 1.0), ny=20,
                                bc=(capi.BC_DYNAMIC, capi.BC_DIRICHLET_MOMENTUM, capi.BC_NO_SLIP, capi.BC_DYNAMIC))
    off0 = offline.SyntheticOffline(spec)

    def state(pos):
        U = np.zeros((len(pos), 3))
        U[:, 0] = 1.0 + 0.05 * np.sin(3.0 * pos[:, 0])
        U[:, 1] = u * U[:, 0]
        return U
    U0 = _perturbed(state(off0.positions))
    dirichlet = state(off0.b_positions)
    off, mods = _both(spec, U0, oracle, n_warm=8, dirichlet=dirichlet, equation=capi.EQ_SHALLOW_WATER)
    g, c = _compare_step(off, mods, dirichlet)
    assert (g["U"][: off.n_owned, 0] > 0).all()


@pytest.mark.parametrize("equation", ["aeos", "scalar", "sw"])
def test_partitioned_other_descriptions_match_single_rank(equation):
    """The ghost exchange carries n_precomputed_values = 4 (EulerAEOS), 2*dim (scalar conservation) and 2
    (shallow water) doubles per DoF and k = 4 / 1 / 3 state components: 3 in-process ranks == single rank."""
    import ctypes as C
    import threading
    from ryujin_amd.initial_states import sw_circular_dam_break
    lib = capi.load_hip()
    n_steps = 5
    eq = {"aeos": capi.EQ_EULER_AEOS, "scalar": capi.EQ_SCALAR_CONSERVATION, "sw": capi.EQ_SHALLOW_WATER}[equation]

    def mesh(n_ranks, rank):
        if equation == "aeos":
            return offline.mach3_step_2d(20, n_ranks=n_ranks, rank=rank)
        bc = capi.BC_DIRICHLET if equation == "scalar" else capi.BC_SLIP
        return offline.rectangle_2d(48, (-5.0, -5.0), (5.0, 5.0), bc=bc, n_ranks=n_ranks, rank=rank)

    def initial(pos):
        if equation == "aeos":
            U = euler_uniform(pos)
            return U * (1.0 + 1e-3 * np.sin(7.0 * pos[:, :1] + 3.0 * pos[:, 1:2]))
        if equation == "scalar":
            # smooth, nowhere constant: in constant regions the Roe average |f_i-f_j| / max(|u_i-u_j|, 2e4 eps)
            # amplifies last-bit differences (different local numbering = different summation order) by 1e11
            return (1.0 + 0.5 * np.sin(0.7 * pos[:, 0]) * np.cos(0.9 * pos[:, 1] + 0.3)).reshape(-1, 1)
        return sw_circular_dam_break(pos)

    def run(off, comm, out, key):
        try:
            p = capi.Params()
            lib.ryujin_hip_default_params(p, eq, 2)
            p.cfl = 0.9
            if equation == "aeos":
                p.eos, p.eos_covolume_b, p.eos_pinf, p.eos_q = capi.EOS_NOBLE_ABEL_STIFFENED_GAS, 0.02, 0.1, 0.05
            m = HyperbolicModule(off, p, backend="hip", comm=comm)
            U0 = initial(off.positions)
            d = initial(off.b_positions) if off.n_bdry and equation != "sw" else None
            state = m.new_state_vector(U0)
            temps = [m.new_state_vector() for _ in range(3)]
            taus = [m.time_step("erk 33", state, temps, d if k == 0 else None) for k in range(n_steps)]
            out[key] = (off.global_ids[: off.n_owned].astype(np.int64), state.download()[: off.n_owned], taus,
                        m.integrals(state))
        except Exception as e:
            out[key] = e

    ref = {}
    run(offline.SyntheticOffline(mesh(1, 0)), None, ref, 0)
    assert not isinstance(ref[0], Exception), ref[0]
    gid, U, taus, integ = ref[0]
    assert np.all(np.isfinite(U))
    n_ranks = 3
    comms = (C.c_void_p * n_ranks)()
    assert lib.ryujin_hip_comm_init_local(comms, n_ranks, 0) == 0
    parts = [offline.SyntheticOffline(mesh(n_ranks, r)) for r in range(n_ranks)]
    out = {}
    threads = [threading.Thread(target=run, args=(parts[r], C.c_void_p(comms[r]), out, r)) for r in range(n_ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
        assert not t.is_alive(), "rank thread hung"
    for r in range(n_ranks):
        assert not isinstance(out[r], Exception), out[r]
        assert np.allclose(out[r][2], taus, rtol=1e-13, atol=0)
        np.testing.assert_allclose(out[r][3], integ, rtol=1e-12, atol=1e-12 * np.abs(integ).max())
    g = np.concatenate([out[r][0] for r in range(n_ranks)])
    Up = np.concatenate([out[r][1] for r in range(n_ranks)])
    o1, o2 = np.argsort(gid), np.argsort(g)
    assert np.array_equal(gid[o1], g[o2])
    scale = np.maximum(np.abs(U).max(axis=0), 1e-3 * np.abs(U).max())
    assert (np.abs(Up[o2] - U[o1]) / scale).max() < 1e-11
    for r in range(n_ranks):
        lib.ryujin_hip_comm_destroy(C.c_void_p(comms[r]))


# slack on the CPU oracle's tolerances (tests/test_oracle_golden_verification.py): the round-off-amplifying
# runs get a factor 5, the ones the oracle matches to 1e-13 .. 1e-15 are held to 100x that, i.e. still 1e-11
VERIFICATION_SLACK = {"euler_leblanc_1d": 5.0, "sw_paraboloid_1d": 3.0, "sw_ritter_dam_break": 5.0,
                      "euler_aeos_leblanc_1d": 100.0, "sw_smooth_vortex": 1000.0, "sw_steady_incline": 10.0}


@pytest.mark.parametrize("case", ["euler_leblanc_1d", "euler_rarefaction_1d", "euler_aeos_leblanc_1d",
                                  "euler_aeos_leblanc_1d_strict", "euler_aeos_rarefaction_1d",
                                  "sw_paraboloid_1d", "sw_ritter_dam_break", "sw_smooth_vortex",
                                  "sw_steady_incline"])
def test_verification_golden_on_gpu(oracle, golden_dir, case):
    """The reference's 1-D / shallow-water verification baselines (final time = every tau of up to 8600
    Runge-Kutta steps, normalised error norms against the analytic solution) reproduced by the HIP path:
    Le Blanc and single-rarefaction tubes (Euler and EulerAEOS, strict and non-strict bounds), the
    oscillating lake with wetting and drying, Ritter's dry-bed dam break, the smooth vortex and the
    Manning-friction steady state with dynamic boundaries."""
    from test_oracle_golden_verification import CASES
    fn, args = CASES[case]
    fn("hip", oracle.default_params, golden_dir, *args, slack=VERIFICATION_SLACK.get(case, 1.0))


@pytest.mark.parametrize("case", ["euler_leblanc_1d", "euler_rarefaction_1d", "euler_aeos_leblanc_1d",
                                  "sw_steady_incline", "sw_ritter_dam_break"])
def test_verification_golden_through_the_device_resident_driver(oracle, golden_dir, case):
    """The same baselines with every Runge-Kutta step executed INSIDE the library (ryujin_hip_time_step_fn: one
    host synchronisation per step) and the exact solution supplied as time-dependent Dirichlet data at the stage
    times t + c_s tau (time_integrator.template.h:373-403; hyperbolic_module.template.h:137-139): the tubes have
    Dirichlet ends that move with the exact solution, the incline has `dynamic` boundaries. Same tolerances as the
    stage-wise run above."""
    from test_oracle_golden_verification import CASES
    fn, args = CASES[case]
    fn("hip-device", oracle.default_params, golden_dir, *args, slack=VERIFICATION_SLACK.get(case, 1.0))


@pytest.mark.parametrize("description,scheme,level", [("euler", "ssprk 33", 6), ("euler", "erk 33", 7),
                                                      ("euler", "ssprk 33", 7), ("euler_aeos", "erk 33", 6),
                                                      ("euler_aeos", "ssprk 33", 7), ("euler_aeos", "erk 33", 7)])
def test_isentropic_vortex_fine_golden_on_gpu(golden_dir, description, scheme, level):
    """The 64^2 and 128^2 isentropic-vortex baselines (l7: the reference's MPI runs) on the HIP path."""
    from test_oracle_golden_integration import check_fine_vortex
    check_fine_vortex("hip", golden_dir, description, scheme, level, rtol=1e-8)


def _unstructured_both(oracle, off, U0, equation, n_warm, dirichlet=None, params_edit=None):
    mods, U_start = [], U0
    for backend in ("hip", oracle.backend()):
        p = oracle.default_params(equation, off.dim)
        p.cfl = 0.5
        if params_edit:
            params_edit(p)
        m = HyperbolicModule(off, p, backend=backend)
        old, new = m.new_state_vector(U_start), m.new_state_vector()
        if backend == "hip":
            for _ in range(n_warm):
                m.prepare_state_vector(old, 0.0, dirichlet)
                m.step(old, [], [], new)
                old, new = new, old
            U_start = old.download()
        mods.append((m, old, new))
    return mods


def test_unstructured_p1_mesh_euler(oracle):
    """Continuous P1 triangles on a Delaunay triangulation of a disk (tests/helpers_unstructured.py): row
    lengths 4 .. 10, c_ij antisymmetric only in the interior, boundary normals in every direction, coupling
    boundary pairs along the whole rim. A blast wave reflecting off slip walls, compared sweep by sweep; then
    the rim split into slip / dynamic / dirichlet / no-slip quarters."""
    from helpers_unstructured import disk_points, p1_offline
    off, info = p1_offline(disk_points(24))
    assert off.n_owned > 1800 and off.n_pairs > 200
    U0 = euler_radial_contrast(off.positions, inner=(1.0, 0.0, 10.0), outer=(0.125, 0.0, 0.1), radius=0.35)
    mods = _unstructured_both(oracle, off, U0, capi.EQ_EULER, n_warm=120)     # the shock has hit the wall
    g, c = _compare_step(off, mods)
    mi = off.mi
    for comp in (0, 3):
        before, after = (mi * g["U_old"][:, comp]).sum(), (mi * g["U"][:, comp]).sum()
        assert abs(after - before) < 1e-13 * abs(before)

    bpos = off.positions[off._keep["b_i"]]
    quarter = (np.arctan2(bpos[:, 1], bpos[:, 0]) // (0.5 * np.pi)).astype(int) % 4
    ids = np.array([capi.BC_SLIP, capi.BC_DYNAMIC, capi.BC_DIRICHLET, capi.BC_NO_SLIP], dtype=np.uint8)[quarter]
    off2, _ = p1_offline(disk_points(24))
    off2._keep["b_id"][:] = ids
    far = euler_uniform(bpos, rho=0.5, u=0.3, p=0.4)
    mods = _unstructured_both(oracle, off2, U0, capi.EQ_EULER, n_warm=120, dirichlet=far)
    _compare_step(off2, mods, dirichlet=far)


def test_unstructured_p1_mesh_shallow_water_and_aeos(oracle):
    """The same mesh for the shallow-water Description (bathymetry, m_ij in the source term, dry rim) and
    for EulerAEOS with the van der Waals EOS."""
    from helpers_unstructured import disk_points, p1_offline
    from ryujin_amd.initial_states import aeos_from_primitive
    off, _ = p1_offline(disk_points(20))
    x = off.positions
    r = np.linalg.norm(x, axis=1)
    Z = 0.6 * r ** 2 + 0.05 * np.cos(5.0 * x[:, 0]) * np.sin(3.0 * x[:, 1])
    off.set_initial_precomputed(Z)
    U0 = np.zeros((off.n_owned, 3))
    U0[:, 0] = np.maximum(np.where(r < 0.3, 0.9, 0.45) - Z, 0.0)            # dry towards the rim
    assert (U0[:, 0] == 0).sum() > 50

    def friction(p):
        p.manning_friction_coefficient = 0.03
    mods = _unstructured_both(oracle, off, U0, capi.EQ_SHALLOW_WATER, n_warm=60, params_edit=friction)
    g, c = _compare_step(off, mods)
    assert (g["U"][:, 0] >= 0.0).all()

    off, _ = p1_offline(disk_points(20))

    def vdw(p):
        p.eos = capi.EOS_VAN_DER_WAALS
        p.eos_vdw_a, p.eos_covolume_b = 0.02, 0.05
    p = oracle.default_params(capi.EQ_EULER_AEOS, 2)
    vdw(p)
    inside = r < 0.35
    U0 = aeos_from_primitive(p, np.where(inside, 1.0, 0.2), np.zeros((off.n_owned, 2)), np.where(inside, 8.0, 0.2))
    mods = _unstructured_both(oracle, off, U0, capi.EQ_EULER_AEOS, n_warm=100, params_edit=vdw)
    _compare_step(off, mods)


def test_unstructured_mesh_in_the_numbering_and_layout_of_offline_data(oracle):
    """What OfflineData hands over on an unstructured mesh, as far as it can be had without deal.II: the P1 disk
    renumbered the way OfflineData::setup() does it (tests/helpers_layout.py::offline_data_numbering: Cuthill-McKee,
    then DoFRenumbering::internal_range's bins of equal stencil size in groups of simd_length -- 143 changes of the
    row length from one group of 8 to the next, the 25 rows that fill no group behind n_internal) and stored in the
    reference's SIMD-interleaved layout with simd_length 8. A blast wave off the slip rim, every sweep against the
    oracle on the same numbering; and the update equals the one on the mesh as generated up to summation order."""
    from helpers_layout import offline_data_numbering, to_simd_layout
    from helpers_unstructured import disk_points, p1_offline
    off0, info = p1_offline(disk_points(24))
    order, n_internal = offline_data_numbering(info["rows"], 8)
    off = to_simd_layout(off0, 8, order, n_internal)
    assert 0 < off.n_internal < off.n_owned and (np.diff(off.new_lengths[:n_internal:8]) != 0).sum() > 100
    off.positions = off0.positions[order]
    U0 = euler_radial_contrast(off0.positions, inner=(1.0, 0.0, 10.0), outer=(0.125, 0.0, 0.1), radius=0.35)
    mods = _unstructured_both(oracle, off, U0[order], capi.EQ_EULER, n_warm=120)
    g, _ = _compare_step(off, mods)
    U_start = g["U_old"][: off.n_owned][off.new_index]             # the developed state in the generated numbering
    p = oracle.default_params(capi.EQ_EULER, 2)
    p.cfl = 0.5
    m0 = HyperbolicModule(off0, p, backend="hip")
    a, b = m0.new_state_vector(U_start), m0.new_state_vector()
    m0.prepare_state_vector(a, 0.0)
    m0.step(a, [], [], b)
    ref = b.download()
    got = g["U"][: off.n_owned][off.new_index]
    assert (np.abs(got - ref) / np.abs(ref).max(axis=0)).max() < 1e-12


def test_q1_annulus_between_curved_walls(oracle):
    """Continuous Q1 on general quadrilaterals: the annulus of tests/helpers_q1_quads.py (no cell a parallelogram,
    Jacobians varying inside the cells, two slip walls of opposite curvature -- the geometry family of the reference's
    check-mass-conservation_02 and cylinder benchmarks, not deal.II's mesh of it). A blast between the walls after
    both reflections, every sweep against the oracle; then the outer wall as a `dynamic` far field and the inner wall
    no-slip."""
    from helpers_q1_quads import annulus_mesh, q1_quads_offline
    pts, quads, edges = annulus_mesh(20, 96)
    off, _ = q1_quads_offline(pts, quads, edges)
    assert off.n_owned == 21 * 96 and off.n_pairs > 300
    U0 = euler_radial_contrast(off.positions, inner=(1.0, 0.0, 10.0), outer=(0.125, 0.0, 0.1), radius=0.2,
                               center=(0.7, 0.0))
    mods = _unstructured_both(oracle, off, U0, capi.EQ_EULER, n_warm=240)
    g, _ = _compare_step(off, mods)
    mi = off.mi
    for comp in (0, 3):
        before, after = (mi * g["U_old"][:, comp]).sum(), (mi * g["U"][:, comp]).sum()
        assert abs(after - before) < 1e-13 * abs(before)
    bi = off._keep["b_i"]
    bpos = off.positions[bi]
    outer = np.linalg.norm(bpos, axis=1) > 0.7
    off2, _ = q1_quads_offline(pts, quads, edges)
    off2._keep["b_id"][:] = np.where(outer, capi.BC_DYNAMIC, capi.BC_NO_SLIP).astype(np.uint8)
    far = euler_uniform(bpos, rho=0.5, u=0.3, p=0.4)
    mods = _unstructured_both(oracle, off2, U0, capi.EQ_EULER, n_warm=240, dirichlet=far)
    _compare_step(off2, mods, dirichlet=far)


def test_q1_annulus_shallow_water(oracle):
    """The shallow-water Description on the skewed-quadrilateral annulus: a bathymetry that rises towards the outer
    wall (dry there), Manning friction, a dam break between the walls -- the m_ij-weighted source terms and the
    hydrostatic reconstruction on non-Cartesian c_ij."""
    from helpers_q1_quads import annulus_mesh, q1_quads_offline
    pts, quads, edges = annulus_mesh(20, 96)
    off, _ = q1_quads_offline(pts, quads, edges)
    x = off.positions
    r = np.linalg.norm(x, axis=1)
    Z = 0.9 * (r - 0.4) ** 2 / 0.36 + 0.04 * np.cos(5.0 * x[:, 0]) * np.sin(3.0 * x[:, 1])
    off.set_initial_precomputed(Z)
    near = np.linalg.norm(x - np.array([0.6, 0.0]), axis=1) < 0.2
    U0 = np.zeros((off.n_owned, 3))
    U0[:, 0] = np.maximum(np.where(near, 0.9, 0.35) - Z, 0.0)
    assert (U0[:, 0] == 0).sum() > 100 and (U0[:, 0] > 0.5).sum() > 20

    def friction(p):
        p.manning_friction_coefficient = 0.03
    mods = _unstructured_both(oracle, off, U0, capi.EQ_SHALLOW_WATER, n_warm=80, params_edit=friction)
    g, _ = _compare_step(off, mods)
    assert (g["U"][:, 0] >= 0.0).all() and np.abs(g["U"][:, 1:]).max() > 1e-2


def test_q1_hexahedra_between_curved_walls(oracle):
    """Trilinear Q1 on skewed hexahedra with non-planar faces between two curved and two flat slip walls
    (tests/helpers_q1_quads.py::annulus_mesh_3d): rows of 12 / 18 / 27 entries in the 3-D kernels, c_ij of a genuinely
    trilinear geometry. A blast after its reflections, every sweep against the oracle."""
    from helpers_q1_quads import annulus_mesh_3d, q1_hexes_offline
    pts, hexes, faces = annulus_mesh_3d(7, 32, 5)
    off, _ = q1_hexes_offline(pts, hexes, faces)
    assert off.n_owned == 8 * 32 * 6
    U0 = euler_radial_contrast(off.positions, inner=(1.0, 0.0, 10.0), outer=(0.125, 0.0, 0.1), radius=0.25,
                               center=(0.7, 0.0, 0.25))
    mods = _unstructured_both(oracle, off, U0, capi.EQ_EULER, n_warm=100)
    g, _ = _compare_step(off, mods)
    for comp in (0, 4):
        before, after = (off.mi * g["U_old"][:, comp]).sum(), (off.mi * g["U"][:, comp]).sum()
        assert abs(after - before) < 1e-13 * abs(before)


@pytest.mark.parametrize("case", ["euler_3d", "euler_3d_erk33", "shallow_water_3d_stencil_2d", "euler_2d"])
def test_rows_wider_than_64_entries(oracle, case):
    """The reference's step() is ansatz agnostic: continuous Q2 elements give rows of 27 ... 125 entries in 3-D
    (9 ... 25 in 2-D; source/discretization.h:131-151, sparse_matrix_simd.h:340-350) -- wider than a SELL-64 slice
    has lanes. A periodic Q2 mesh assembled by tests/helpers_q2.py (tensor products of the 1-D element matrices;
    c_ij antisymmetric, some m_ij negative, lumped masses of two sizes), a smooth density and pressure wave on a
    uniform flow: every sweep against the oracle, single update and an ERK33 stage with stage vectors (the generic
    kernels: k_dij_alpha, k_low_order, k_pij_lij / k_high_order in blocks of 63 columns)."""
    from helpers_q2 import q2_periodic_offline
    dim = 2 if case.endswith("2d") else 3
    off, x = q2_periodic_offline(dim, 3 if dim == 3 else 5)
    assert off.max_row_len == (125 if dim == 3 else 25)
    w = np.sin(2.0 * np.pi * x[:, 0]) * np.cos(2.0 * np.pi * x[:, 1])
    if case.startswith("shallow_water"):
        eq = capi.EQ_SHALLOW_WATER
        U0 = np.zeros((off.n_owned, dim + 1))
        U0[:, 0] = 1.0 + 0.3 * w
        U0[:, 1] = 0.2 * U0[:, 0]
        off.set_initial_precomputed(0.05 * np.cos(2.0 * np.pi * x[:, 0]))
    else:
        eq = capi.EQ_EULER
        rho, p = 1.0 + 0.4 * w, 1.0 + 0.3 * w
        v = np.zeros((off.n_owned, dim))
        v[:, 0], v[:, 1] = 0.5, -0.25
        U0 = np.concatenate([rho[:, None], rho[:, None] * v, (p / 0.4 + 0.5 * rho * (v ** 2).sum(1))[:, None]], axis=1)
    if case.endswith("erk33"):
        # whole ERK33 steps: step<1>, step<2> with stage vectors (time_integrator.template.h:373-403)
        finals = []
        for backend in ("hip", oracle.backend()):
            m = HyperbolicModule(off, equation=eq, backend=backend)
            sv = m.new_state_vector(U0)
            ti = TimeIntegrator(m, "erk 33", cfl_min=0.5, cfl_max=0.5, cfl_recovery_strategy="none")
            t = 0.0
            for _ in range(3):
                sv, tau = ti.step(sv, t)
                t += tau
            finals.append((t, sv.download()[: off.n_owned]))
        assert abs(finals[0][0] - finals[1][0]) < 1e-12 * finals[1][0]
        scale = np.maximum(np.abs(finals[1][1]).max(axis=0), 1e-3 * np.abs(finals[1][1]).max())   # (m_z is 0 to round-off)
        assert (np.abs(finals[0][1] - finals[1][1]) / scale).max() < 5e-11
        return
    for n_warm in (0, 6):     # the first update from the initial data, and one a few updates later
        mods = _unstructured_both(oracle, off, U0, eq, n_warm=n_warm)
        _compare_step(off, mods)


@pytest.mark.parametrize("equation", ["euler", "shallow_water"])
def test_unstructured_arbitrary_partition_on_gpu(oracle, equation):
    """The multi-rank code path on a partition the mesh generator cannot produce: the P1 disk cut into 5
    angular sectors around an off-centre point -- up to 4 neighbours per rank, nodes exported to several
    ranks, exchange lists built by tests/helpers_unstructured.py::partition from the contract in
    include/ryujin_hip.h. Five contexts (one host thread each) on one GPU with the in-process transport must
    reproduce the single-context run, through prepare_state_vector/step and through the device-resident
    SSPRK33 driver (deferred collectives)."""
    import ctypes as C
    import threading

    from helpers_unstructured import disk_points, p1_offline, partition
    from test_oracle_unstructured import sector_owner
    lib = capi.load_hip()
    n_ranks = 5
    off, info = p1_offline(disk_points(22))
    x = off.positions
    if equation == "euler":
        eq = capi.EQ_EULER
        Z = None
        U0 = euler_radial_contrast(x, inner=(1.0, 0.0, 10.0), outer=(0.125, 0.0, 0.1), radius=0.35,
                                   center=(0.1, -0.05))
    else:
        eq = capi.EQ_SHALLOW_WATER
        r = np.linalg.norm(x - np.array([0.1, -0.05]), axis=1)
        Z = 0.5 * np.linalg.norm(x, axis=1) ** 2 + 0.03 * np.cos(6.0 * x[:, 0])
        off.set_initial_precomputed(Z)
        U0 = np.zeros((off.n_owned, 3))
        U0[:, 0] = np.maximum(np.where(r < 0.3, 0.8, 0.4) - Z, 0.0)
    views = partition(off, info, sector_owner(x, n_ranks), bathymetry=Z)
    assert max(v._o.n_nbr for v in views) >= 3
    p = oracle.default_params(eq, 2)
    p.cfl = 0.5
    n_updates, n_rk = 12, 4

    def run(view, comm, out, key, U_init):
        try:
            m = HyperbolicModule(view, p, backend="hip", comm=comm)
            a, b = m.new_state_vector(U_init), m.new_state_vector()
            taus = []
            for _ in range(n_updates):
                m.prepare_state_vector(a, 0.0)
                taus.append(m.step(a, [], [], b))
                a, b = b, a
            temps = [b, m.new_state_vector(), m.new_state_vector()]
            for _ in range(n_rk):
                taus.append(m.time_step("ssprk 33", a, temps))
            out[key] = (a.download()[: view.n_owned], taus, m.integrals(a))
        except Exception as e:  # noqa: BLE001
            out[key] = e

    ref = {}
    run(off, None, ref, 0, U0)
    assert not isinstance(ref[0], Exception), ref[0]
    U_ref, taus, integ = ref[0]
    comms = (C.c_void_p * n_ranks)()
    assert lib.ryujin_hip_comm_init_local(comms, n_ranks, 0) == 0
    out = {}
    threads = [threading.Thread(target=run, args=(views[r], C.c_void_p(comms[r]), out, r, U0[views[r].global_ids]))
               for r in range(n_ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
        assert not t.is_alive(), "rank thread hung"
    U = np.empty_like(U0)
    for r in range(n_ranks):
        assert not isinstance(out[r], Exception), out[r]
        np.testing.assert_allclose(out[r][1], taus, rtol=1e-13)
        np.testing.assert_allclose(out[r][2], integ, rtol=1e-11, atol=1e-12 * np.abs(integ).max())
        U[views[r].global_ids[: views[r].n_owned]] = out[r][0]
    # Partitioned against single-rank HIP after 24 updates of a blast wave. A partition renumbers the rows, which
    # changes the order of every stencil sum: the two runs differ by round-off from the first update on and the
    # flow amplifies it. The yardstick is what the SAME renumbering does to the reference algorithm itself -- the
    # partitioned oracle against the single-rank oracle over the same sequence of updates: the HIP pair may not
    # drift apart more than 4x as far (plus the per-update contract, 1e-11 each; the one-update comparison of every
    # rank against the oracle, ghost rows included, is tests/test_partitioned_vs_oracle.py).
    from helpers_partitioned import run_oracle_ranks

    def oracle_sequence(m, part, r, U_init=None):
        a, b = m.new_state_vector(U0[part.global_ids] if U_init is None else U_init), m.new_state_vector()
        for _ in range(n_updates):
            m.prepare_state_vector(a, 0.0)
            m.step(a, [], [], b)
            a, b = b, a
        ti = TimeIntegrator(m, "ssprk 33", cfl_min=p.cfl, cfl_max=p.cfl, cfl_recovery_strategy="none")
        for _ in range(n_rk):
            a, _tau = ti.step(a, 0.0)
        return a.download()[: part.n_owned]
    parts_U = run_oracle_ranks(oracle, views, lambda: p, oracle_sequence)
    U_oracle_part = np.empty_like(U0)
    for r in range(n_ranks):
        U_oracle_part[views[r].global_ids[: views[r].n_owned]] = parts_U[r]
    m_single = HyperbolicModule(off, p, backend=oracle.backend())
    U_oracle_single = oracle_sequence(m_single, off, 0, U_init=U0)
    drift_oracle = (np.abs(U_oracle_part - U_oracle_single).max(axis=0) / np.abs(U_ref).max(axis=0)).max()
    drift_hip = (np.abs(U - U_ref).max(axis=0) / np.abs(U_ref).max(axis=0)).max()
    n_total = n_updates + 3 * n_rk
    assert drift_hip <= 4.0 * drift_oracle + 1e-11 * n_total, (drift_hip, drift_oracle)
    for r in range(n_ranks):
        lib.ryujin_hip_comm_destroy(C.c_void_p(comms[r]))


@pytest.mark.parametrize("equation", ["euler", "euler_aeos"])
def test_unstructured_p1_tetrahedra_3d(oracle, equation):
    """P1 tetrahedra on a Delaunay tetrahedralisation of a ball: rows of 6 .. 30 entries (never the 27 of a
    Q1 hexahedral mesh), lumped masses over two orders of magnitude, slip walls on a sphere: the generic
    (non-unrolled) 3-D sweeps against the oracle, single stage and with ERK stage weights."""
    from helpers_unstructured import ball_points, p1_offline
    from ryujin_amd.initial_states import aeos_from_primitive
    off, _ = p1_offline(ball_points(2500, 900))
    x = off.positions
    inside = np.linalg.norm(x, axis=1) < 0.5
    if equation == "euler":
        eq, edit = capi.EQ_EULER, None
        U0 = euler_radial_contrast(x, inner=(1.0, 0.0, 10.0), outer=(0.125, 0.0, 0.1), radius=0.5)
    else:
        eq = capi.EQ_EULER_AEOS

        def edit(p):
            p.eos = capi.EOS_NOBLE_ABEL_STIFFENED_GAS
            p.eos_covolume_b, p.eos_q, p.eos_pinf = 0.1, 0.05, 0.2
        p = oracle.default_params(eq, 3)
        edit(p)
        U0 = aeos_from_primitive(p, np.where(inside, 1.0, 0.2), np.zeros((off.n_owned, 3)),
                                 np.where(inside, 8.0, 0.2))

    def params(p):
        p.cfl = 0.5
        if edit:
            edit(p)
    mods, U_start = [], U0
    for backend in ("hip", oracle.backend()):
        p = oracle.default_params(eq, 3)
        params(p)
        m = HyperbolicModule(off, p, backend=backend)
        old, new = m.new_state_vector(U_start), m.new_state_vector()
        if backend == "hip":
            for _ in range(60):
                m.prepare_state_vector(old, 0.0)
                m.step(old, [], [], new)
                old, new = new, old
            U_start = old.download()
        mods.append((m, old, new))
    _compare_step(off, mods)
    # four ERK33 steps (step<1>, step<2> with stage weights) from the warmed-up state
    finals = []
    for m, old, new in mods:
        sv = m.new_state_vector(U_start)
        ti = TimeIntegrator(m, "erk 33", cfl_min=0.5, cfl_max=0.5, cfl_recovery_strategy="none")
        t = 0.0
        for _ in range(4):
            sv, tau = ti.step(sv, t)
            t += tau
        finals.append((t, sv.download()))
    assert abs(finals[0][0] - finals[1][0]) < 1e-12 * finals[1][0]
    scale = np.abs(finals[1][1]).max(axis=0)
    assert (np.abs(finals[0][1] - finals[1][1]) / scale).max() < 1e-10


def test_unstructured_p1_mesh_scalar_conservation(oracle):
    """Burgers' equation (K = 1, 2 dim precomputed flux-gradient values) on the P1 disk with Dirichlet data
    on the whole rim: the scalar Description on ragged rows."""
    from helpers_unstructured import disk_points, p1_offline
    off, _ = p1_offline(disk_points(20), boundary_id=capi.BC_DIRICHLET)
    x = off.positions
    u0 = np.where(np.linalg.norm(x - np.array([0.2, 0.1]), axis=1) < 0.4, 1.0, -0.5) + 0.1 * np.sin(4.0 * x[:, 0])
    U0 = u0.reshape(-1, 1)
    dirichlet = U0[off._keep["b_i"]]
    for greedy, averaged in ((0, 0), (1, 1)):
        def edit(p):
            p.cfl = 0.5
            p.sc_flux = capi.FLUX_BURGERS
            p.sc_use_greedy_wavespeed = greedy
            p.sc_use_averaged_entropy = averaged
        mods = _scalar_both(off, U0, oracle, edit, n_warm=15, dirichlet=dirichlet)
        _scalar_compare(off, mods, dirichlet)


@pytest.mark.parametrize("which", ["euler_2d", "euler_1d", "euler_erk33", "sw_2d", "sw_1d", "aeos_2d", "scalar_2d",
                                   "euler_2d:no_prediction", "euler_1d:no_prediction", "euler_erk33:no_prediction",
                                   "aeos_2d:no_prediction", "euler_2d:always_store", "aeos_2d:always_store",
                                   "euler_2d:no_tile_prediction", "euler_1d:no_tile_prediction",
                                   "aeos_2d:no_tile_prediction",
                                   "euler_3d", "euler_3d:no_prediction", "euler_3d:always_store", "aeos_3d",
                                   "aeos_3d:no_prediction"])
def test_step_parity_with_the_kernels_of_large_meshes(oracle, monkeypatch, which):
    """The meshes of this file do not fill an MI355X, so they take the small-mesh branches of the library
    (boundary conditions folded into the pre-pass, steps 5 and 6 with the columns of a slice spread over several
    waves). Re-run one case per Description with those branches switched off: the kernels BASELINE-sized meshes
    run (also covered at full size for Euler and shallow water in test_gpu_parity_fullsize.py).
    An update without stage vectors stores P_ij only where steps 6 and 7 read it (kernels_limiter_stage0.hpp): per
    (slice, column) tile -- the default up to two dimensions: where one of the tile's own l_ij comes out limited or
    step 6 read the tile in one of the last updates, step 6 forming what is missing inside its sweep;
    `:no_tile_prediction` predicts no tile (every tile that the neighbour's l_ji alone limits goes through step 6's
    repair). Per 64-row slice
    (3-D, and `:no_prediction` here): where the slice
    held a limited pair in the previous update -- the first update of a context stores everywhere --, or where one
    of its own l_ij comes out limited (stored from that column on, the columns before it formed a second time);
    a slice limited through a neighbour's l_ji alone gets its P_ij from the repair prologue of step 6, which runs as a
    light and a heavy launch. `:no_prediction` predicts no slice limited (every stored slice goes through the
    trigger or the repair prologue), `:always_store` all of them. The P_ij the comparison fetches is what the sweeps
    stored, completed through the same device function for the slices they left out (ryujin_hip_debug_fetch)."""
    switches = {"debug_no_small_mesh_split": 1, "debug_bc_fold_max_slices": -1}
    which, _, variant = which.partition(":")
    if variant:
        switches["debug_pij_storage"] = {"no_prediction": 1, "always_store": -1, "no_tile_prediction": 2}[variant]
    monkeypatch.setattr(HyperbolicModule, "library_switches", switches)
    {
        "euler_2d": lambda: test_step_parity_2d_step_geometry(oracle),
        "euler_1d": lambda: test_step_parity_1d(oracle),
        "euler_erk33": lambda: test_multistage_parity_erk33(oracle),
        "sw_2d": lambda: test_sw_step_parity_2d_dam_break_over_bathymetry(oracle),
        "sw_1d": lambda: test_sw_step_parity_1d(oracle),
        "aeos_2d": lambda: test_aeos_step_parity_2d_step_geometry(oracle, False),
        "scalar_2d": lambda: test_scalar_parity_2d(oracle, "kpp"),
        "euler_3d": lambda: test_step_parity_3d_radial_contrast(oracle, 20, (4, 7)),
        "aeos_3d": lambda: test_aeos_step_parity_1d_and_3d(oracle, dims=(3,)),
    }[which]()
