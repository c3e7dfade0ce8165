"""Device-resident Postprocessor (ryujin_hip_postprocess_*, HyperbolicModule.postprocess) against the numpy restatement
of tests/helpers_postprocessor.py: raw values row by row, bounds, normalised values -- 100 % of the owned rows, with
the derived tolerances stated there (raw: 1e-13 x sum_j |c_ij| |q_j| / m_i per row; bounds: that of the rows that attain
them; normalised: beta (delta_i + 2 delta_bounds) / (q_max - q_min) + 4 eps)."""
import ctypes as C

import numpy as np
import pytest

import helpers_postprocessor as hp
from helpers_partitioned import run_hip_ranks
from ryujin_amd import HyperbolicModule, capi, offline
from ryujin_amd.initial_states import euler_radial_contrast, euler_uniform, sw_circular_dam_break

pytestmark = pytest.mark.gpu


def _params(equation, dim, **edits):
    p = capi.Params()
    capi.load_hip().ryujin_hip_default_params(C.byref(p), equation, dim)
    p.cfl = 0.9
    for name, value in edits.items():
        setattr(p, name, value)
    return p


def _copy_params(p):
    q = capi.Params()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(capi.Params))
    return q


def _develop(m, U0, dirichlet, n_updates):
    a, b = m.new_state_vector(U0), m.new_state_vector()
    for _ in range(n_updates):
        m.prepare_state_vector(a, 0.0, dirichlet)
        m.step(a, [], [], b)
        a, b = b, a
    return a


def _compare(label, off, U, names, quantities, equation, params, dev_raw, dev_bounds, dev_norm, beta,
             reference_rows=None, reference=None):
    """device results of one rank against numpy. reference = (raw, scale) of the mesh the bounds are taken over
    (the single-rank mesh of a partitioned run; default: this one), reference_rows: this rank's rows in it."""
    raw, scale = hp.raw_values(off, U, quantities, equation, params)
    ref_raw, ref_scale = (raw, scale) if reference is None else reference
    for k, name in enumerate(names):
        tol = hp.raw_tolerance(scale[k])
        err = np.abs(dev_raw[name] - raw[k])
        worst = int((err - tol).argmax())
        print(f"{label} {name}: raw max err {err.max():.3e} (worst row {worst}: err {err[worst]:.3e}, "
              f"tol {tol[worst]:.3e}, value {raw[k][worst]:.6e})")
        assert np.isfinite(dev_raw[name]).all()
        assert (err <= tol).all(), (name, worst, err[worst], tol[worst])
        if reference_rows is not None:  # the same values as the single-rank mesh gives for these rows
            both = hp.raw_tolerance(ref_scale[k][reference_rows]) + tol
            assert (np.abs(raw[k] - ref_raw[k][reference_rows]) <= both).all()
        q_max, q_min = hp.bounds(ref_raw[k])
        d_max, d_min = hp.bounds_tolerance(ref_raw[k], ref_scale[k])
        g_max, g_min = dev_bounds[name]
        print(f"{label} {name}: q_max {g_max:.17g} (numpy {q_max:.17g}, tol {d_max:.3e}), "
              f"q_min {g_min:.17g} (numpy {q_min:.17g}, tol {d_min:.3e})")
        assert abs(g_max - q_max) <= d_max and abs(g_min - q_min) <= d_min
        assert g_max >= g_min >= 0.0
        expected = hp.normalise(raw[k], q_max, q_min, beta)
        ntol = hp.normalised_tolerance(scale[k], max(d_max, d_min), q_max, q_min, beta)
        nerr = np.abs(dev_norm[name] - expected)
        worst = int((nerr - ntol).argmax())
        print(f"{label} {name}: normalised max err {nerr.max():.3e} (worst row {worst}: err {nerr[worst]:.3e}, "
              f"tol {ntol[worst]:.3e})")
        assert (nerr <= ntol).all(), (name, worst, nerr[worst], ntol[worst])
        assert (np.abs(dev_norm[name]) < 1.0).all()


def _run_and_compare(label, off, m, state, schlieren, vorticity, beta=10.0):
    quantities, names = hp.resolve(m.equation, off.dim, schlieren, vorticity)
    dev_norm = m.postprocess(state, schlieren=schlieren, vorticity=vorticity, beta=beta)
    assert list(dev_norm) == names
    dev_raw = m.postprocess_download(raw=True)
    dev_bounds = m.postprocess_bounds()
    U = state.download()
    _compare(label, off, U, names, quantities, m.equation, m.params, dev_raw, dev_bounds, dev_norm, beta)
    return dev_raw, dev_bounds, dev_norm


def _euler_case(dim):
    if dim == 2:
        off = offline.SyntheticOffline(offline.mach3_step_2d(40))
        rng = np.random.default_rng(11)
        U0 = euler_uniform(off.positions)
        U0 *= 1.0 + 1e-3 * rng.uniform(-1, 1, size=U0.shape)
        return off, U0, euler_uniform(off.b_positions)
    off = offline.SyntheticOffline(offline.box_3d(20))
    return off, euler_radial_contrast(off.positions, radius=0.3), None


@pytest.mark.parametrize("dim", [2, 3])
def test_euler_several_quantities_in_one_sweep(dim):
    """conserved and primitive components, schlieren and vorticity, five quantities in one call"""
    off, U0, dirichlet = _euler_case(dim)
    m = HyperbolicModule(off, _params(capi.EQ_EULER, dim), backend="hip")
    state = _develop(m, U0, dirichlet, 6)
    raw, bounds, norm = _run_and_compare(f"euler {dim}d", off, m, state, ("rho", "p", "E"), ("m_1", "v_1"))
    assert bounds["schlieren_rho"][0] > 0.0 and bounds["vorticity_v_1"][0] > 0.0  # a flow with something in it
    if dim == 2:  # the 2-D vorticity is signed
        assert (raw["vorticity_v_1"] < 0).any() and (raw["vorticity_v_1"] > 0).any()
        assert (np.signbit(norm["vorticity_v_1"]) == np.signbit(raw["vorticity_v_1"])).all()
    for name in ("schlieren_rho", "schlieren_p", "schlieren_E"):
        assert (raw[name] >= 0).all() and (norm[name] >= 0).all()
    # the default call: schlieren of rho alone, the same field
    alone = m.postprocess(state)
    assert list(alone) == ["schlieren_rho"] and np.array_equal(alone["schlieren_rho"], norm["schlieren_rho"])
    m.close()


def test_euler_1d_schlieren_and_no_vorticity():
    off = offline.SyntheticOffline(offline.MeshSpec(1, (160,), (-1.0,), (1.0,), (capi.BC_SLIP, capi.BC_SLIP)))
    x = off.positions[:, 0]
    U0 = np.zeros((len(x), 3))
    U0[:, 0] = np.where(x < 0.0, 1.0, 0.125)
    U0[:, 2] = np.where(x < 0.0, 2.5, 0.25)
    m = HyperbolicModule(off, _params(capi.EQ_EULER, 1), backend="hip")
    state = _develop(m, U0, None, 5)
    _run_and_compare("euler 1d", off, m, state, ("rho", "v", "p"), ())
    with pytest.raises(RuntimeError, match="status -2"):
        m.postprocess(state, schlieren=(), vorticity=("m",))
    m.close()


def test_shallow_water_with_dry_nodes():
    """(h, v) with the sharp inverse water depth: dry nodes (h = 0, with and without a residual momentum) next to
    wet ones; the state is never prepared (the primitive state comes from U itself)"""
    off = offline.SyntheticOffline(offline.rectangle_2d(48, (-5.0, -5.0), (5.0, 5.0)))
    x = off.positions
    U0 = sw_circular_dam_break(x)
    U0[:, 1] = U0[:, 0] * 0.3 * np.sin(0.7 * x[:, 1])
    U0[:, 2] = U0[:, 0] * 0.2 * np.cos(0.5 * x[:, 0])
    dry = x[:, 0] > 3.0
    U0[dry, 0] = 0.0
    U0[dry, 1:] = 0.0
    U0[dry & (x[:, 1] > 0.0), 1] = 1.0e-18
    m = HyperbolicModule(off, _params(capi.EQ_SHALLOW_WATER, 2), backend="hip")
    state = m.new_state_vector(U0)
    raw, _, _ = _run_and_compare("shallow water", off, m, state, ("h", "v_2"), ("v_1", "m_1"))
    assert np.abs(raw["vorticity_v_1"]).max() > 0.0
    m.close()


def test_euler_aeos_specific_internal_energy():
    off = offline.SyntheticOffline(offline.mach3_step_2d(30))
    U0 = euler_uniform(off.positions)
    U0 *= 1.0 + 1e-3 * np.sin(7.0 * off.positions[:, :1] + 3.0 * off.positions[:, 1:2])
    m = HyperbolicModule(off, _params(capi.EQ_EULER_AEOS, 2), backend="hip")
    state = _develop(m, U0, euler_uniform(off.b_positions), 5)
    raw, _, _ = _run_and_compare("euler aeos", off, m, state, ("e", "rho"), ("v_1",))
    assert raw["schlieren_e"].max() > 0.0
    m.close()


def test_scalar_conservation():
    off = offline.SyntheticOffline(offline.rectangle_2d(48, (-2.0, -2.5), (2.0, 1.5), bc=capi.BC_DIRICHLET))
    r = np.linalg.norm(off.positions, axis=1)
    U0 = np.where(r < 1.0, 1.0, -0.5).reshape(-1, 1)
    m = HyperbolicModule(off, _params(capi.EQ_SCALAR_CONSERVATION, 2), backend="hip")
    state = _develop(m, U0, U0[off.b_i], 4)
    _run_and_compare("scalar", off, m, state, ("u",), ())
    with pytest.raises(RuntimeError, match="status -2"):  # dim components do not fit a one-component state
        m.postprocess(state, schlieren=(), vorticity=("u",))
    m.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_without_the_tile_map_bitwise_equal(dim):
    off, U0, dirichlet = _euler_case(dim)
    out = []
    for tile_map in (0, -1):
        m = HyperbolicModule(off, _params(capi.EQ_EULER, dim, debug_tile_map=tile_map), backend="hip")
        state = m.new_state_vector(U0)
        norm = m.postprocess(state, schlieren=("rho", "p"), vorticity=("v_1",))
        out.append((norm, m.postprocess_download(raw=True), m.postprocess_bounds()))
        m.close()
    for name in out[0][0]:
        assert np.array_equal(out[0][0][name], out[1][0][name])
        assert np.array_equal(out[0][1][name], out[1][1][name])
        assert out[0][2][name] == out[1][2][name]


def test_compute_twice_is_bitwise_reproducible_and_bounds_can_be_kept():
    off, U0, dirichlet = _euler_case(2)
    m = HyperbolicModule(off, _params(capi.EQ_EULER, 2), backend="hip")
    a = _develop(m, U0, dirichlet, 6)
    first = m.postprocess(a, schlieren=("rho",), vorticity=("v_1",))
    first_raw, first_bounds = m.postprocess_download(raw=True), m.postprocess_bounds()
    second = m.postprocess(a, schlieren=("rho",), vorticity=("v_1",))
    second_raw, second_bounds = m.postprocess_download(raw=True), m.postprocess_bounds()
    for name in first:
        assert np.array_equal(first[name], second[name]) and np.array_equal(first_raw[name], second_raw[name])
        assert first_bounds[name] == second_bounds[name]

    # recompute_bounds = 0: the bounds of the first call are kept for a different state
    b = _develop(m, a.download(), dirichlet, 12)
    kept = m.postprocess(a, schlieren=("rho",), vorticity=("v_1",), recompute_bounds=False)
    bounds_a = m.postprocess_bounds()
    assert bounds_a == first_bounds and all(np.array_equal(kept[k], first[k]) for k in first)
    later = m.postprocess(b, schlieren=("rho",), vorticity=("v_1",), recompute_bounds=False)
    assert m.postprocess_bounds() == bounds_a
    raw_b = m.postprocess_download(raw=True)
    quantities, names = hp.resolve(capi.EQ_EULER, 2, ("rho",), ("v_1",))
    np_raw, np_scale = hp.raw_values(off, b.download(), quantities, capi.EQ_EULER, m.params)
    for k, name in enumerate(names):
        own = hp.bounds(np_raw[k])
        assert own != bounds_a[name]  # the second state has other bounds of its own ...
        q_max, q_min = bounds_a[name]  # ... and is normalised with the first call's (the device's, exactly)
        assert (np.abs(raw_b[name] - np_raw[k]) <= hp.raw_tolerance(np_scale[k])).all()
        ntol = hp.normalised_tolerance(np_scale[k], 0.0, q_max, q_min)
        assert (np.abs(later[name] - hp.normalise(np_raw[k], q_max, q_min)) <= ntol).all()
    # Postprocessor::reset_bounds(): the next call takes its bounds afresh, and keeps them again
    m.postprocess_reset_bounds()
    m.postprocess(b, schlieren=("rho",), vorticity=("v_1",), recompute_bounds=False)
    reset = m.postprocess_bounds()
    m.postprocess(a, schlieren=("rho",), vorticity=("v_1",), recompute_bounds=False)
    assert m.postprocess_bounds() == reset and reset != bounds_a
    # ... and recompute_bounds = 1 takes the second state's own
    m.postprocess(b, schlieren=("rho",), vorticity=("v_1",), recompute_bounds=True)
    fresh = m.postprocess_bounds()
    for k, name in enumerate(names):
        d_max, d_min = hp.bounds_tolerance(np_raw[k], np_scale[k])
        own = hp.bounds(np_raw[k])
        assert abs(fresh[name][0] - own[0]) <= d_max and abs(fresh[name][1] - own[1]) <= d_min
        assert reset[name] == fresh[name]
    m.close()


from postprocessor_rccl_worker import partition_state as _partition_state  # noqa: E402


def test_partitioned_on_three_ranks_with_stale_ghosts():
    n_ranks, cpu = 3, 30
    schlieren, vorticity, beta = ("rho", "p"), ("v_1",), 10.0
    single = offline.SyntheticOffline(offline.mach3_step_2d(cpu))
    parts = [offline.SyntheticOffline(offline.mach3_step_2d(cpu, n_ranks=n_ranks, rank=r)) for r in range(n_ranks)]
    assert all(p.n_relevant > p.n_owned for p in parts)
    params = _params(capi.EQ_EULER, 2)
    quantities, names = hp.resolve(capi.EQ_EULER, 2, schlieren, vorticity)
    U_single = _partition_state(single.positions)
    reference = hp.raw_values(single, U_single, quantities, capi.EQ_EULER, params)

    def body(m, part, r):
        U = _partition_state(part.positions)
        stale = U.copy()
        stale[part.n_owned:] = 0.0  # the ghost range is NOT current: compute() has to exchange it
        state = m.new_state_vector(stale)
        norm = m.postprocess(state, schlieren=schlieren, vorticity=vorticity, beta=beta)
        return norm, m.postprocess_download(raw=True), m.postprocess_bounds(), state.download()

    ranks = run_hip_ranks(parts, lambda: _copy_params(params), body)
    lookup = {int(g): i for i, g in enumerate(single.global_ids)}
    for r, (norm, raw, bounds, U_after) in enumerate(ranks):
        part = parts[r]
        # the exchange filled the ghost range with the owners' values
        assert np.allclose(U_after, _partition_state(part.positions), rtol=1e-14, atol=0.0)
        U = U_after
        rows = np.array([lookup[int(g)] for g in part.global_ids[: part.n_owned]])
        assert bounds == ranks[0][2]  # every rank holds the same bounds, bit by bit
        _compare(f"rank {r}", part, U, names, quantities, capi.EQ_EULER, params, raw, bounds, norm, beta,
                 reference_rows=rows, reference=reference)
    # the bounds are those of ALL ranks: no rank's own rows give them
    own = [hp.bounds(ranks[r][1]["schlieren_rho"]) for r in range(n_ranks)]
    assert len({o[0] for o in own}) == n_ranks

    # ... and the single-rank device run gives the same bounds and fields
    m = HyperbolicModule(single, _copy_params(params), backend="hip")
    norm_1 = m.postprocess(m.new_state_vector(U_single), schlieren=schlieren, vorticity=vorticity, beta=beta)
    bounds_1 = m.postprocess_bounds()
    m.close()
    for k, name in enumerate(names):
        d_max, d_min = hp.bounds_tolerance(reference[0][k], reference[1][k])
        assert abs(bounds_1[name][0] - ranks[0][2][name][0]) <= 2 * d_max
        assert abs(bounds_1[name][1] - ranks[0][2][name][1]) <= 2 * d_min
        q_max, q_min = hp.bounds(reference[0][k])
        ntol = hp.normalised_tolerance(reference[1][k], max(d_max, d_min), q_max, q_min, beta)
        for r in range(n_ranks):
            rows = np.array([lookup[int(g)] for g in parts[r].global_ids[: parts[r].n_owned]])
            assert (np.abs(ranks[r][0][name] - norm_1[name][rows]) <= 2 * ntol[rows]).all()


def test_rccl_leg_over_the_test_double(tmp_path):
    """the same partitioned case through the library's RCCL calls (ncclSend / ncclRecv of the ghost range,
    ncclAllReduce max / min of the bounds): three processes on one GPU over tests/cpp/librccl_stub.so"""
    import postprocessor_rccl_worker as worker
    import test_rccl_stub
    world, cpu = 3, 30
    prefix = str(tmp_path / "pp")
    test_rccl_stub.launch(world, [prefix, str(cpu)], tmp_path, timeout=300, worker=worker.__file__)

    single = offline.SyntheticOffline(offline.mach3_step_2d(cpu))
    params = _params(capi.EQ_EULER, 2)
    quantities, names = hp.resolve(capi.EQ_EULER, 2, worker.SCHLIEREN, worker.VORTICITY)
    reference = hp.raw_values(single, _partition_state(single.positions), quantities, capi.EQ_EULER, params)
    lookup = {int(g): i for i, g in enumerate(single.global_ids)}
    first = None
    for r in range(world):
        part = offline.SyntheticOffline(offline.mach3_step_2d(cpu, n_ranks=world, rank=r))
        got = np.load(f"{prefix}.rank{r}.npz")
        assert list(got["names"]) == names
        assert np.allclose(got["U"], _partition_state(part.positions), rtol=1e-14, atol=0.0)
        first = got["bounds"] if first is None else first
        assert np.array_equal(got["bounds"], first)  # every rank holds the same bounds, bit by bit
        rows = np.array([lookup[int(g)] for g in part.global_ids[: part.n_owned]])
        _compare(f"rccl rank {r}", part, got["U"], names, quantities, capi.EQ_EULER, params,
                 dict(zip(names, got["raw"])), {k: tuple(b) for k, b in zip(names, got["bounds"])},
                 dict(zip(names, got["norm"])), worker.BETA, reference_rows=rows, reference=reference)


def test_argument_errors():
    off = offline.SyntheticOffline(offline.mach3_step_2d(20))
    m = HyperbolicModule(off, _params(capi.EQ_EULER, 2), backend="hip")
    lib, ctx = capi.load_hip(), m._ctx
    state = m.new_state_vector(euler_uniform(off.positions))
    out = np.zeros(off.n_owned)
    hi, lo = C.c_double(), C.c_double()
    Q = capi.PostprocessQuantity

    def configure(*entries, n=None):
        q = (Q * max(1, len(entries)))(*[Q(*e) for e in entries])
        return lib.ryujin_hip_postprocess_configure(ctx, len(entries) if n is None else n, q, 10.0, 1)

    # compute before configure, download / bounds before compute
    assert lib.ryujin_hip_postprocess_compute(ctx, state.handle) == capi.RYUJIN_ERR_ARG
    assert configure((capi.PP_SCHLIEREN, 0, 0)) == capi.RYUJIN_OK
    assert lib.ryujin_hip_postprocess_download(ctx, 0, capi.as_ptr(out, capi.c_double_p), 0) == capi.RYUJIN_ERR_ARG
    assert lib.ryujin_hip_postprocess_bounds(ctx, 0, C.byref(hi), C.byref(lo)) == capi.RYUJIN_ERR_ARG
    # a component out of range, a vorticity whose dim components do not fit, an unknown kind, too many quantities
    assert configure((capi.PP_SCHLIEREN, 0, 4)) == capi.RYUJIN_ERR_ARG
    assert configure((capi.PP_SCHLIEREN, 1, -1)) == capi.RYUJIN_ERR_ARG
    assert configure((capi.PP_VORTICITY, 0, 3)) == capi.RYUJIN_ERR_ARG
    assert configure((capi.PP_VORTICITY, 0, 2)) == capi.RYUJIN_OK
    assert configure((7, 0, 0)) == capi.RYUJIN_ERR_ARG
    assert configure(*[(capi.PP_SCHLIEREN, 0, 0)] * (capi.PP_MAX_QUANTITIES + 1)) == capi.RYUJIN_ERR_ARG
    assert configure(*[(capi.PP_SCHLIEREN, 0, 0)] * capi.PP_MAX_QUANTITIES) == capi.RYUJIN_OK
    assert configure(n=0) == capi.RYUJIN_ERR_ARG
    # a failed configure leaves the last good configuration in place; an invalid handle is refused
    assert lib.ryujin_hip_postprocess_compute(ctx, 99) == capi.RYUJIN_ERR_ARG
    assert lib.ryujin_hip_postprocess_compute(ctx, state.handle) == capi.RYUJIN_OK
    assert lib.ryujin_hip_postprocess_download(ctx, capi.PP_MAX_QUANTITIES, capi.as_ptr(out, capi.c_double_p),
                                               0) == capi.RYUJIN_ERR_ARG
    assert lib.ryujin_hip_postprocess_download(ctx, capi.PP_MAX_QUANTITIES - 1, capi.as_ptr(out, capi.c_double_p),
                                               0) == capi.RYUJIN_OK
    assert (out == 0.0).all()  # a uniform state
    # the eight-quantity sweep: every copy of the quantity holds the same field
    U0 = _partition_state(off.positions)
    state.upload(U0)
    assert lib.ryujin_hip_postprocess_compute(ctx, state.handle) == capi.RYUJIN_OK
    fields = []
    for q in range(capi.PP_MAX_QUANTITIES):
        a = np.zeros(off.n_owned)
        assert lib.ryujin_hip_postprocess_download(ctx, q, capi.as_ptr(a, capi.c_double_p), 1) == capi.RYUJIN_OK
        fields.append(a)
    raw, scale = hp.raw_values(off, U0, [(hp.SCHLIEREN, 0, 0)])
    assert all(np.array_equal(f, fields[0]) for f in fields)
    assert (np.abs(fields[0] - raw[0]) <= hp.raw_tolerance(scale[0])).all()
    # unknown names are refused before anything reaches the library
    with pytest.raises(ValueError):
        m.postprocess(state, schlieren=("temperature",))
    m.close()


def test_full_size_c2_mesh_schlieren_of_rho():
    """the C2 mesh of bench.py (2.5 M gridpoints): the large-grid launch path, against numpy on every row"""
    off = offline.SyntheticOffline(offline.mach3_step_2d(995))
    assert off.n_owned > 2_400_000
    m = HyperbolicModule(off, _params(capi.EQ_EULER, 2), backend="hip")
    U0 = euler_uniform(off.positions)
    U0 *= 1.0 + 1e-3 * np.sin(7.0 * off.positions[:, :1] + 3.0 * off.positions[:, 1:2])
    dirichlet = euler_uniform(off.b_positions)
    state = m.new_state_vector(U0)
    temps = [m.new_state_vector() for _ in range(3)]
    for k in range(10):
        m.time_step("ssprk 33", state, temps, dirichlet if k == 0 else None)
    _, bounds, _ = _run_and_compare("C2", off, m, state, ("rho",), ())
    assert bounds["schlieren_rho"][0] > 1.0  # the shock off the step
    m.close()
