"""The shallow-water states that bring their own bathymetry, and the bed of every shallow-water state, on the device
(capi.IV_BATHYMETRY_STATES; ryujin_amd/csrc/initial_states_bathymetry_device.hpp, kernels_initial_values.hpp).

A  state and bed against ryujin_amd.initial_states, tolerances DERIVED in tests/helpers_initial_values_bathymetry.py; the
   piecewise-polynomial beds bit for bit
B  the consumers' bits: evaluate, interpolate and the Dirichlet kernel; the two bed kernels and the output extraction
C  the beds of the earlier states: paraboloid and sloping friction, exact zeros for every state without a bed
D  the update sees a device-made bed exactly as a bed given at create, and agrees with the CPU oracle on it
E  time_step_iv against the callback path, bit for bit, with data that switches in time
F  interpolate_initial_precomputed on a 2 x 2 partition and on three slabs: owned and ghost rows
G  the lake at rest over a device-made bed against the CPU oracle
H  the reference's paraboloid_1d and steady_incline baselines from a flat-bed context and a device-made bed
I  refusals, and what they leave behind
Every test fails at its first configure or bed call on a library without the five states and the three entry points."""
import ctypes as C

import numpy as np
import pytest

import helpers_initial_values as hiv
import helpers_initial_values_bathymetry as hb
from helpers_initial_values_bathymetry import Case
from ryujin_amd import HyperbolicModule, TimeIntegrator, capi, offline
from ryujin_amd import initial_states as ist

pytestmark = pytest.mark.gpu

CASES = hb.function_cases()
SW = capi.EQ_SHALLOW_WATER
D, S = capi.BC_DIRICHLET, capi.BC_SLIP
N_STEPS = 20
SW_EDITS = dict(gravity=9.81, reference_water_depth=1.0, dry_state_relaxation_factor=0.2, dry_state_relaxation_small=1e4,
                dry_state_relaxation_large=1e4, cfl=0.25)


# --------------------------------------------------------------------------- A

@pytest.mark.parametrize("case", CASES, ids=[c.label for c in CASES])
def test_states_and_beds_against_the_numpy_restatement(case):
    """evaluate() and evaluate_initial_precomputed() at 1000 points, the state at three times (0, one below and one
    above the state's switch), against ryujin_amd.initial_states behind the affine transform; every point clear of
    every region boundary ON THE HOST VALUES (asserted); tolerance per point and component from the error arithmetic.
    Where the transform is a subtraction alone, the piecewise-polynomial beds are demanded bit for bit."""
    m = hb.module_for(case)
    X = hb.points_for(case)
    assert X.shape == (1000, case.dim)
    hb.assert_clear_of_jumps(case, X)
    bed = m.initial_values_evaluate_initial_precomputed(X)
    for t in case.times:
        got = m.initial_values_evaluate(X, t)
        ref, ref_bed = hb.reference(case, X, t)
        tol, tol_bed = hb.tolerance(case, X, t)
        err = np.abs(got - ref)
        worst = np.unravel_index(int(np.argmax(err - tol)), err.shape)
        scale = np.maximum(np.abs(ref).max(axis=0), 1e-300)
        print(f"{case.label} t={t:g}: max err / scale {err.max(axis=0) / scale}, max tol / scale "
              f"{tol.max(axis=0) / scale}; worst point {worst[0]} component {worst[1]}: err {err[worst]:.3e} "
              f"tol {tol[worst]:.3e} value {ref[worst]:.17g}")
        assert np.isfinite(got).all()
        assert (err <= tol).all(), (case.label, t, worst, float(err[worst]), float(tol[worst]))
        bed_err = np.abs(bed - ref_bed)
        print(f"{case.label}: bed max err {bed_err.max():.3e}, max tol {tol_bed.max():.3e}, "
              f"{int((bed != ref_bed).sum())} of 1000 differ")
        assert (bed_err <= tol_bed).all(), (case.label, int(np.argmax(bed_err - tol_bed)))
    mask = hb.bitwise_bed_mask(case, X)
    if mask is not None and hb.exact_transform(case):
        assert mask.sum() >= 300
        np.testing.assert_array_equal(bed[mask], hb.reference_bed(case, X)[mask])
    if case.name == "soliton":
        assert (bed == 0.0).all() and not np.signbit(bed).any()
    # ... and the node kernel, on the module's own nodes: the same function behind the same transform
    nodes = m.offline.positions
    m.initial_values_interpolate_initial_precomputed()
    held = m.initial_precomputed()
    assert (np.abs(held - hb.reference_bed(case, nodes)) <= hb.bed_tolerance(case, nodes)).all()
    np.testing.assert_array_equal(held, m.initial_values_evaluate_initial_precomputed(nodes))
    m.close()


# --------------------------------------------------------------------------- B

# the smallest mesh of the dimension is [0, 1]^dim: `position` moves its corner onto this point of the state's frame
CONSUMER_TARGETS = {"flow over bump": (9.5, -0.25), "three bumps dam break": (29.5, 5.5), "hou test": (-200.5, -0.5),
                    "transient experiments": (2.0, -0.5), "soliton": (-0.25, 0.125)}


def _consumer_case(c):
    target = (47.0,) if (c.name, c.dim) == ("three bumps dam break", 1) else CONSUMER_TARGETS[c.name][: c.dim]
    position = -hiv.affine_transform_vector(c.dir(), np.array([target]))[0]
    return Case(c.label, c.equation, c.dim, c.name, c.params, c.direction, tuple(float(p) for p in position), edits=c.edits,
                times=c.times)


CONSUMER_CASES = [_consumer_case(c) for c in CASES]


@pytest.mark.parametrize("case", CONSUMER_CASES, ids=[c.label for c in CONSUMER_CASES])
def test_consumers_give_the_same_bits(case):
    """on the smallest mesh of the dimension, all ends Dirichlet: interpolate + download == evaluate(positions);
    prepare_state_vector with dirichlet="device" leaves evaluate(b_positions) in the boundary rows and the same state
    as the host path fed with it. The bed: evaluate_initial_precomputed(positions) == interpolate_initial_precomputed
    + initial_precomputed() == the "bathymetry" quantity of the output extraction."""
    off = hiv.tiny_mesh(case.dim)
    m = hb.module_for(case, off)
    for t in case.times:
        expected = m.initial_values_evaluate(off.positions, t)
        assert np.isfinite(expected).all()
        sv = m.new_state_vector(np.full((off.n_relevant, m.k), np.nan))
        m.initial_values_interpolate(sv, t)
        np.testing.assert_array_equal(sv.download(), expected)
        U0 = 1.5 * m.initial_values_evaluate(off.positions, 0.0)     # admissible, and not the boundary data:
        U0[:, 0] += 1.0                                              # (a dry node of the state is wet here)
        boundary = m.initial_values_evaluate(off.b_positions, t)
        a, b = m.new_state_vector(U0), m.new_state_vector(U0)
        m.prepare_state_vector(a, t, "device")
        m.prepare_state_vector(b, t, boundary)
        A = a.download()
        np.testing.assert_array_equal(A, b.download())
        assert (off.b_id == D).all()
        np.testing.assert_array_equal(A[off.b_i], boundary)
        assert (U0[off.b_i, 0] != boundary[:, 0]).all()
        for s in (sv, a, b):
            s.free()
    before = m.initial_precomputed()
    assert (before == 0.0).all()
    want = m.initial_values_evaluate_initial_precomputed(off.positions)
    m.initial_values_interpolate_initial_precomputed()
    held = m.initial_precomputed()
    np.testing.assert_array_equal(held, want)
    if case.name != "soliton":
        assert np.abs(held).max() > 0.0
    m.output_configure(["bathymetry"])
    sv = m.new_state_vector(m.initial_values_evaluate(off.positions, 0.0))
    m.prepare_state_vector(sv, 0.0, "device")
    np.testing.assert_array_equal(m.output_extract(sv, precision="float64")[0], held)
    m.close()


# --------------------------------------------------------------------------- C

EARLIER_BEDS = [
    Case("paraboloid", SW, 1, "paraboloid", {"free surface radius": 3000.0, "water height": 10.0,
                                             "paraboloid length": 10000.0, "speed": 2.0}, position=(12.5,),
         edits=dict(gravity=9.81)),
    Case("sloping friction", SW, 1, "sloping friction", {"ramp slope": 1.0e-2, "initial discharge": 1.0e-1},
         position=(-0.75,), edits=dict(gravity=9.81, manning_friction_coefficient=1.0e-2)),
    Case("sloping friction 2d (1,1)", SW, 2, "sloping friction", {"ramp slope": 1.0e-2, "initial discharge": 1.0e-1},
         (1.0, 1.0), (0.25, -0.125), edits=dict(gravity=9.81, manning_friction_coefficient=1.0e-2)),
]


def _mesh_with_a_given_bed(dim, seed=11):
    lower, upper = ((0.0,), (10000.0,)) if dim == 1 else ((0.0, 0.0), (20.0, 10.0))
    spec = offline.MeshSpec(1, (130,), lower, upper, (D, D)) if dim == 1 else \
        offline.rectangle_2d(12, lower, upper, bc=D, ny=9)
    off = offline.SyntheticOffline(spec)
    given = np.random.default_rng(seed).uniform(-1.0, 1.0, off.n_relevant)
    off.set_initial_precomputed(given)
    return off, given


@pytest.mark.parametrize("case", EARLIER_BEDS, ids=[c.label for c in EARLIER_BEDS])
def test_paraboloid_and_sloping_friction_get_their_reference_bed(case):
    off, given = _mesh_with_a_given_bed(case.dim)
    m = hb.module_for(case, off)
    np.testing.assert_array_equal(m.initial_precomputed(), given)         # what create was given, bit for bit
    m.initial_values_interpolate_initial_precomputed()
    got, ref, tol = m.initial_precomputed(), hb.reference_bed(case, off.positions), hb.bed_tolerance(case, off.positions)
    print(f"{case.label}: bed max err {np.abs(got - ref).max():.3e}, max tol {tol.max():.3e}, max |bed| "
          f"{np.abs(ref).max():.3e}")
    assert np.abs(ref).max() > 0.1 and (np.abs(got - ref) <= tol).all()
    np.testing.assert_array_equal(m.initial_values_evaluate_initial_precomputed(off.positions), got)
    m.close()


ZERO_BEDS = [("uniform", 1, {}), ("contrast", 2, {}), ("circular dam break", 2, {}), ("soliton", 1, {}),
             ("ritter dam break", 1, {}), ("smooth vortex", 2, {}), ("function", 2, {})]


@pytest.mark.parametrize("name,dim,params", ZERO_BEDS, ids=[z[0] for z in ZERO_BEDS])
def test_states_without_a_bed_write_exact_zeros(name, dim, params):
    off, given = _mesh_with_a_given_bed(dim)
    m = HyperbolicModule(off, hiv.make_params(SW, dim, gravity=9.81), backend="hip")
    if name == "function":
        m.initial_values_configure_function(["1 + x*x", "y", "t"], position=(0.5, 0.25))
    else:
        m.initial_values_configure(name, position=(0.5, 0.25)[:dim], **params)
    np.testing.assert_array_equal(m.initial_precomputed(), given)
    m.initial_values_interpolate_initial_precomputed()
    bed = m.initial_precomputed()
    assert (bed == 0.0).all() and not np.signbit(bed).any()
    points = np.random.default_rng(1).uniform(-5.0, 5.0, (100, dim))
    assert (m.initial_values_evaluate_initial_precomputed(points) == 0.0).all()
    m.close()


# --------------------------------------------------------------------------- D

def _lattice_2d():
    """33 x 31 nodes; the tank of three bumps dam break, [0, 75] x [0, 30], behind position = (-10, -5)"""
    return offline.SyntheticOffline(offline.rectangle_2d(32, (-10.0, -5.0), (65.0, 25.0), bc=S, ny=30))


DAM = Case("three bumps dam break 33x31", SW, 2, "three bumps dam break",
           {"left water depth": 1.875, "right water depth": 0.5, "cone magnitude": 0.2}, None, (-10.0, -5.0),
           edits=SW_EDITS)
BUMP_1D = Case("flow over bump 130 cells", SW, 1, "flow over bump", {}, None, (-0.5,), edits=SW_EDITS)
UPDATE_CASES = {
    "three bumps dam break 33x31": (_lattice_2d, DAM),
    "flow over bump 130 cells": (lambda: hiv.interval(130, -0.5, 24.5, D, D), BUMP_1D),
}


def _steps(m, U0, scheme, n_steps, dirichlet=None):
    m.cfl = SW_EDITS["cfl"]
    state = m.new_state_vector(U0)
    temps = [m.new_state_vector() for _ in range(3)]
    states, taus, t = [], [], 0.0
    for _ in range(n_steps):
        tau = m.time_step(scheme, state, temps, dirichlet, t=t)
        t += tau
        taus.append(tau)
        states.append(state.download())
    return states, taus


@pytest.mark.parametrize("name", sorted(UPDATE_CASES))
def test_the_update_sees_a_device_made_bed_like_a_given_one(name, oracle):
    """20 SSPRK33 steps on a flat-bed context after interpolate_initial_precomputed, and on a second context created
    with the first one's downloaded bed: U and tau bit for bit at every step. The mesh is shifted by `position`: a
    node kernel without the transform gives another bed. 2-D: one update of the first context through
    helpers_parity.compare_step against the CPU oracle created with the downloaded bed."""
    make, case = UPDATE_CASES[name]
    off = make()
    assert off.n_relevant == (33 * 31 if case.dim == 2 else 131)
    m1 = hb.module_for(case, off)
    m1.initial_values_interpolate_initial_precomputed()
    bed = m1.initial_precomputed()
    ref = hb.reference_bed(case, off.positions)
    assert (np.abs(bed - ref) <= hb.bed_tolerance(case, off.positions)).all() and (bed > 0.01).sum() >= 10
    U0 = m1.initial_values_evaluate(off.positions, 0.0)
    dirichlet = m1.initial_values_evaluate(off.b_positions, 0.0) if case.dim == 1 else None
    states1, taus1 = _steps(m1, U0, "ssprk 33", N_STEPS, dirichlet)

    off2 = make()
    off2.set_initial_precomputed(bed)
    m2 = HyperbolicModule(off2, hiv.make_params(case.equation, case.dim, **case.edits), backend="hip")
    states2, taus2 = _steps(m2, U0, "ssprk 33", N_STEPS, dirichlet)
    assert taus1 == taus2 and all(tau > 0.0 for tau in taus1)
    for step, (a, b) in enumerate(zip(states1, states2)):
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b, err_msg=f"{name}: after step {step}")
    assert not np.array_equal(states1[0], states1[-1])

    # the bed matters: a flat-bed context takes another path from the first step on
    m0 = HyperbolicModule(make(), hiv.make_params(case.equation, case.dim, **case.edits), backend="hip")
    states0, _ = _steps(m0, U0, "ssprk 33", 1, dirichlet)
    assert not np.array_equal(states0[0], states1[0])
    m0.close()

    if case.dim == 2:
        from helpers_parity import compare_step
        params = hiv.make_params(case.equation, case.dim, **case.edits)
        mo = HyperbolicModule(off2, params, backend=oracle.backend())
        mods = [(m1, m1.new_state_vector(U0), m1.new_state_vector()),
                (mo, mo.new_state_vector(U0), mo.new_state_vector())]
        g, c = compare_step(off, mods, None, oracle=oracle, params=params, label=name)
        assert g["status"] == 0 and c["status"] == 0
        print(f"{name}: " + " ".join(f"{k}={v:.2e}" for k, v in sorted(g["measured"].items())))
        mo.close()
    m1.close()
    m2.close()


# --------------------------------------------------------------------------- E

def _driver_case(name):
    """(mesh factory, case, scheme) of a driver run"""
    if name == "flow over bump 1d":
        return (lambda: hiv.interval(130, -0.5, 24.5, D, D)), BUMP_1D, "erk 33"
    if name == "three bumps dam break 2d inflow":
        # -x Dirichlet, the three other sides slip
        return (lambda: offline.SyntheticOffline(offline.rectangle_2d(32, (-10.0, -5.0), (65.0, 25.0),
                                                                      bc=(D, S, S, S), ny=12))), DAM, "erk 33"
    scheme = {"soliton 1d erk33": "erk 33", "soliton 1d ssprk33": "ssprk 33"}[name]
    return (lambda: hiv.interval(200, 0.0, 40.0, D, D)), Case(
        name, SW, 1, "soliton", {"still water depth": 1.0, "amplitude": 0.2}, None, (-3.0,), edits=SW_EDITS), scheme


def _run_both(make, case, scheme):
    results = []
    for device in (True, False):
        off = make()
        m = hb.module_for(case, off)
        m.initial_values_interpolate_initial_precomputed()
        U0 = m.initial_values_evaluate(off.positions, 0.0)
        results.append(hiv.run_driver(m, case, U0, scheme, N_STEPS, device) + (U0,))
        m.close()
    (states_iv, taus_iv, restarts_iv, U0), (states_fn, taus_fn, restarts_fn, _) = results
    assert taus_iv == taus_fn, (taus_iv, taus_fn)
    assert all(tau > 0.0 for tau in taus_iv)
    for step, (a, b) in enumerate(zip(states_iv, states_fn)):
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b, err_msg=f"{case.label}: after step {step}")
    assert not np.array_equal(states_iv[0], states_iv[-1])
    assert restarts_iv == restarts_fn
    return U0, states_iv, taus_iv


@pytest.mark.parametrize("name", ["flow over bump 1d", "three bumps dam break 2d inflow", "soliton 1d erk33",
                                  "soliton 1d ssprk33"])
def test_time_step_iv_equals_the_callback_path_bit_for_bit(name):
    """20 Runge-Kutta steps twice from the same uploaded state over the device-made bed: ryujin_hip_time_step_iv, and
    ryujin_hip_time_step_fn whose callback returns initial_values_evaluate(b_positions, time). States after every
    step and every tau equal; the boundary rows show the data switching in time."""
    make, case, scheme = _driver_case(name)
    U0, states, taus = _run_both(make, case, scheme)
    off = make()
    rows = np.asarray(off.b_i)[np.asarray(off.b_id) == D]
    left = rows[off.positions[rows, 0] == off.positions[:, 0].min()]
    assert len(left) >= 1
    # the same step with the data FROZEN at t = 0 takes another path: the switch in time reached the device's stages
    m = hb.module_for(case, make())
    m.initial_values_interpolate_initial_precomputed()
    frozen_data = m.initial_values_evaluate(off.b_positions, 0.0)
    m.cfl = case.edits["cfl"]
    state, temps = m.new_state_vector(U0), [m.new_state_vector() for _ in range(3)]
    m.time_step(scheme, state, temps, None, cfl_min=m.cfl, cfl_max=m.cfl, t=0.0, dirichlet_fn=lambda time: frozen_data)
    frozen = state.download()
    m.close()
    assert not np.array_equal(frozen, states[0])
    if name == "flow over bump 1d":
        # the first stage (t = 0 < 1e-12) sees the initial state h_inflow, every later one the steady solution, which
        # is subcritical upstream of the bump: the depth at the inflow end stays nearer to it than to h_inflow
        assert (U0[left, 0] == 0.28205279813802181).all() and taus[0] > 1.0e-12
        steady = ist.sw_flow_over_bump(np.zeros((1, 1)), 1.0)[0][0, 0]
        assert steady > 0.4
        assert all(abs(s[left[0], 0] - steady) < abs(s[left[0], 0] - U0[left[0], 0]) for s in states)
    elif name.startswith("three bumps"):
        # the inflow switches on behind t = 1e-10: with the frozen data the inflow side stays at rest, the dam is far
        assert (U0[left, 1] == 0.0).all() and taus[0] > 1.0e-10
        assert np.abs(frozen[left, 1]).max() < 1e-12 and (states[0][left, 1] > 0.1).all()
    else:
        # the crest, 3 to the left of the inflow end at t = 0, approaches: the depth there rises
        depth = [s[left[0], 0] for s in states]
        assert depth[-1] > depth[0] > 1.0


def _disk():
    from helpers_unstructured import disk_points, p1_offline
    points = 5.0 * disk_points(18)
    off, info = p1_offline(points, boundary_id=D)
    off.b_positions = points[np.flatnonzero(info["is_bdry"])]
    return points, off, info


def test_time_step_iv_on_three_ranks_one_without_boundary():
    """three bumps dam break on three in-process ranks, every rank configured with its own positions: P1 elements on a
    disk of radius 5 moved onto the dam (position = (-16, -15)), the outer ring Dirichlet, rank 1 the inner disk r < 2,
    which owns NO boundary entry (asserted). The gathered states after every step and every tau equal the callback
    run's; every rank makes its own bed."""
    from helpers_partitioned import run_hip_ranks
    from helpers_unstructured import partition
    points, off, info = _disk()
    r = np.linalg.norm(points, axis=1)
    owner = np.where(r < 2.0, 1, np.where(points[:, 0] < 0.0, 0, 2))
    views = partition(off, info, owner)
    assert [v.n_bdry > 0 for v in views] == [True, False, True]
    case = Case("three bumps 3 ranks", SW, 2, "three bumps dam break",
                {"left water depth": 1.875, "right water depth": 0.5, "cone magnitude": 0.2}, None, (-16.0, -15.0),
                edits=SW_EDITS)

    def body(device):
        def run(m, part, rank):
            hiv.configure(m, case)
            m.initial_values_interpolate_initial_precomputed()
            U0 = m.initial_values_evaluate(part.positions, 0.0)
            states, taus, _ = hiv.run_driver(m, case, U0, "erk 33", N_STEPS, device, b_positions=part.b_positions)
            return [s[: part.n_owned] for s in states], taus
        return run

    params = lambda: hiv.make_params(case.equation, case.dim, **case.edits)  # noqa: E731
    out_iv = run_hip_ranks(views, params, body(True))
    out_fn = run_hip_ranks(views, params, body(False))
    for rank in range(3):
        assert out_iv[rank][1] == out_fn[rank][1] == out_iv[0][1]
    for step in range(N_STEPS):
        gathered = []
        for out in (out_iv, out_fn):
            U = np.full((len(points), 3), np.nan)
            for rank, v in enumerate(views):
                U[v.global_ids[: v.n_owned]] = out[rank][0][step]
            gathered.append(U)
        assert np.isfinite(gathered[0]).all()
        np.testing.assert_array_equal(gathered[0], gathered[1], err_msg=f"after step {step}")


# --------------------------------------------------------------------------- F

@pytest.mark.parametrize("layout", ["2 x 2", "three slabs"])
def test_every_rank_makes_the_single_rank_bed(layout):
    """flow over bump along (1, 1) from position (-7, -7) on the disk: every rank's owned rows equal the single-rank
    array, every ghost row its owner's value, bit for bit; nothing is exchanged"""
    from helpers_partitioned import run_hip_ranks
    from helpers_unstructured import partition
    points, off, info = _disk()
    if layout == "2 x 2":
        owner = (points[:, 0] >= 0.0).astype(np.int64) + 2 * (points[:, 1] >= 0.0)
    else:
        owner = (points[:, 0] >= -5.0 / 3.0).astype(np.int64) + (points[:, 0] >= 5.0 / 3.0)
    views = partition(off, info, owner)
    assert len(views) == (4 if layout == "2 x 2" else 3) and all(v.n_relevant > v.n_owned for v in views)
    case = Case("flow over bump on the disk", SW, 2, "flow over bump", {}, (1.0, 1.0), (-7.0, -7.0),
                edits=dict(gravity=9.81))
    params = lambda: hiv.make_params(case.equation, case.dim, **case.edits)  # noqa: E731
    single = HyperbolicModule(off, params(), backend="hip")
    hiv.configure(single, case)
    single.initial_values_interpolate_initial_precomputed()
    whole = single.initial_precomputed()
    ref = hb.reference_bed(case, points)
    assert (np.abs(whole - ref) <= hb.bed_tolerance(case, points)).all() and (whole > 0.01).sum() >= 100
    single.close()

    def run(m, part, rank):
        hiv.configure(m, case)
        exchanges = m.exchange_info()["n_exchanges"]
        m.initial_values_interpolate_initial_precomputed()
        bed = m.initial_precomputed()
        assert m.exchange_info()["n_exchanges"] == exchanges
        return bed

    beds = run_hip_ranks(views, params, run)
    for rank, v in enumerate(views):
        n = v.n_owned
        np.testing.assert_array_equal(beds[rank][:n], whole[v.global_ids[:n]], err_msg=f"rank {rank}: owned rows")
        np.testing.assert_array_equal(beds[rank][n:], whole[v.global_ids[n:]], err_msg=f"rank {rank}: ghost rows")
        assert np.abs(beds[rank][n:]).max() > 0.0


# --------------------------------------------------------------------------- G

LAKE_DEPTH = 1.875
LAKE_VARIANTS = {"all wet": 0.5, "dry island": 1.0}


def _lake_case(magnitude):
    return Case(f"lake at rest, cone magnitude {magnitude}", SW, 2, "three bumps dam break",
                {"well balancing validation": True, "left water depth": LAKE_DEPTH, "right water depth": LAKE_DEPTH,
                 "cone magnitude": magnitude}, None, (-10.0, -5.0), edits=SW_EDITS)


def _lake_maxima(U, bed):
    """(max |q|, max |h + Z - H|) over the wet nodes: those whose bed lies below the surface"""
    wet = bed < LAKE_DEPTH
    return float(np.abs(U[:, 1:]).max()), float(np.abs(U[wet, 0] + bed[wet] - LAKE_DEPTH).max())


@pytest.mark.parametrize("variant", sorted(LAKE_VARIANTS))
def test_lake_at_rest_over_a_device_made_bed(variant, oracle):
    """20 SSPRK33 steps on the 33 x 31 lattice from interpolate and interpolate_initial_precomputed, no host-made
    array. The CPU oracle runs the same setup on the downloaded bed first and sets the yardstick: max |q| and
    max |h + Z - H| over the wet nodes. Step by step the device's update of the oracle's state agrees with the
    oracle's within the U and tau tolerances of helpers_parity.compare_step; the free-running device keeps both maxima
    within 10 times the oracle's (floors 1e-13 H sqrt(g H) and 1e-13 H for an oracle value of exactly 0)."""
    from helpers_parity import U_TOL
    case = _lake_case(LAKE_VARIANTS[variant])
    off = _lattice_2d()
    m = hb.module_for(case, off)
    m.initial_values_interpolate_initial_precomputed()
    sv = m.new_state_vector()
    m.initial_values_interpolate(sv, 0.0)
    bed, U0 = m.initial_precomputed(), sv.download()
    assert (bed.max() > LAKE_DEPTH) == (variant == "dry island") and (U0[:, 1:] == 0.0).all()
    assert ((U0[:, 0] == 0.0) == (bed >= LAKE_DEPTH)).all()

    cfl = SW_EDITS["cfl"]
    off_o = _lattice_2d()
    off_o.set_initial_precomputed(bed)
    params = hiv.make_params(case.equation, case.dim, **case.edits)
    mo = HyperbolicModule(off_o, params, backend=oracle.backend())
    ti_o = TimeIntegrator(mo, "ssprk 33", cfl_min=cfl, cfl_max=cfl, cfl_recovery_strategy="none")
    ti_d = TimeIntegrator(m, "ssprk 33", cfl_min=cfl, cfl_max=cfl, cfl_recovery_strategy="none")
    so, t, worst_U, worst_tau = mo.new_state_vector(U0), 0.0, 0.0, 0.0
    for step in range(N_STEPS):
        before = so.download()
        so, tau_o = ti_o.step(so, t)
        sd, tau_d = ti_d.step(m.new_state_vector(before), t)       # the device's step from the oracle's state
        Uo, Ud = so.download(), sd.download()
        scale = np.maximum(np.abs(Uo).max(axis=0), 1e-3 * np.abs(Uo).max())
        worst_U = max(worst_U, float((np.abs(Ud - Uo) / scale).max()))
        worst_tau = max(worst_tau, abs(tau_d - tau_o) / tau_o)
        assert abs(tau_d - tau_o) <= 1e-12 * tau_o, (step, tau_d, tau_o)
        assert (np.abs(Ud - Uo) / scale <= U_TOL).all(), (step, float((np.abs(Ud - Uo) / scale).max()))
        t += tau_o
    q_o, eta_o = _lake_maxima(so.download(), bed)

    ti = TimeIntegrator(m, "ssprk 33", cfl_min=cfl, cfl_max=cfl, cfl_recovery_strategy="none")
    t = 0.0
    for _ in range(N_STEPS):
        sv, tau = ti.step(sv, t)
        t += tau
    q_d, eta_d = _lake_maxima(sv.download(), bed)
    floor_q, floor_eta = 1e-13 * LAKE_DEPTH * float(np.sqrt(9.81 * LAKE_DEPTH)), 1e-13 * LAKE_DEPTH
    print(f"lake at rest, {variant}: oracle max |q| {q_o:.3e} max |h + Z - H| {eta_o:.3e}; device max |q| {q_d:.3e} "
          f"max |h + Z - H| {eta_d:.3e}; per step max |dU| / scale {worst_U:.3e}, max |dtau| / tau {worst_tau:.3e}")
    assert q_d <= max(10.0 * q_o, floor_q) and eta_d <= max(10.0 * eta_o, floor_eta)
    mo.close()
    m.close()


# --------------------------------------------------------------------------- H

BASELINES = {
    "sw_paraboloid_1d": ("paraboloid", dict(free_surface_radius=3000.0, water_height=10.0, paraboloid_length=10000.0,
                                            speed=2.0)),
    "sw_steady_incline": hiv.VERIFICATION["sw_steady_incline"],
}


@pytest.mark.parametrize("name", sorted(BASELINES))
def test_recorded_baselines_from_a_device_made_bed(oracle, golden_dir, monkeypatch, name):
    """The reference's paraboloid_1d and steady_incline verification runs with the driver of
    tests/helpers_initial_values.py (run_verification_on_device) and the tolerances of
    tests/test_oracle_golden_verification.py and tests/test_gpu_parity.py, imported and not edited -- but the context
    is created over a FLAT bed: the host-made bathymetry the set-up passes is withheld from the driver, and the bed
    comes from interpolate_initial_precomputed right after the configure."""
    import test_oracle_golden_verification as tv
    from test_gpu_parity import VERIFICATION_SLACK
    inner = hiv.run_verification_on_device(BASELINES[name])
    seen = {}

    def run(backend, off, params, exact, components, bathymetry=None, **kw):
        assert bathymetry is not None
        seen["host bed"] = np.array(bathymetry)
        return inner(backend, off, params, exact, components, bathymetry=None, **kw)

    configure = HyperbolicModule.initial_values_configure

    def configure_then_make_the_bed(self, *args, **kw):
        configure(self, *args, **kw)
        assert (self.initial_precomputed() == 0.0).all()              # created flat
        self.initial_values_interpolate_initial_precomputed()
        seen["device bed"] = self.initial_precomputed()

    monkeypatch.setattr(HyperbolicModule, "initial_values_configure", configure_then_make_the_bed)
    monkeypatch.setattr(tv, "run_verification", run)
    fn, args = tv.CASES[name]
    fn("hip-iv", oracle.default_params, golden_dir, *args, slack=VERIFICATION_SLACK.get(name, 1.0))
    host, device = seen["host bed"], seen["device bed"]
    print(f"{name}: {inner.seconds:.2f} s wall; device-made bed against the host-made one: max |difference| "
          f"{np.abs(device - host).max():.3e} of max |bed| {np.abs(host).max():.3e}")
    assert np.abs(host).max() > 0.1 and np.abs(device - host).max() <= 8.0 * hiv.EPS * np.abs(host).max()


# --------------------------------------------------------------------------- I

def _configure_status(module, iv):
    off = module.offline
    pos = np.ascontiguousarray(off.positions).reshape(-1)
    bpos = np.ascontiguousarray(off.b_positions).reshape(-1)
    return module._lib.ryujin_hip_initial_values_configure(
        module._ctx, C.byref(iv), capi.as_ptr(pos, capi.c_double_p), capi.as_ptr(bpos, capi.c_double_p))


def _bed_entry_statuses(m):
    x, out = np.zeros(m.dim), np.zeros(m.n_relevant + 1)
    lib = m._lib
    return [lib.ryujin_hip_initial_values_interpolate_initial_precomputed(m._ctx),
            lib.ryujin_hip_initial_values_evaluate_initial_precomputed(m._ctx, capi.as_ptr(x, capi.c_double_p), 1,
                                                                       capi.as_ptr(out, capi.c_double_p)),
            lib.ryujin_hip_get_initial_precomputed(m._ctx, capi.as_ptr(out, capi.c_double_p))]


def test_refusals_leave_the_previous_configuration_and_bed_in_place():
    off2, off1 = hiv.tiny_mesh(2), hiv.tiny_mesh(1)
    X2 = np.random.default_rng(2).uniform(-1.0, 1.0, (100, 2)) + np.array([30.0, 6.0])
    X1 = np.linspace(7.0, 13.0, 100)[:, None]
    names = [n for _, n in capi.IV_BATHYMETRY_STATES]
    assert sorted(names) == sorted(hb.NEW_STATES)

    # before a configure: RYUJIN_ERR_ARG, on shallow water and on Euler alike
    msw = HyperbolicModule(off2, hiv.make_params(SW, 2, gravity=9.81), backend="hip")
    assert _bed_entry_statuses(msw) == [capi.RYUJIN_ERR_ARG] * 3
    assert b"configure" in msw._lib.ryujin_hip_last_error()

    msw.initial_values_configure("three bumps dam break", cone_magnitude=0.75)
    msw.initial_values_interpolate_initial_precomputed()
    state_before, bed_before = msw.initial_values_evaluate(X2, 0.0), msw.initial_precomputed()
    points_before = msw.initial_values_evaluate_initial_precomputed(X2)
    assert np.abs(points_before).max() > 0.5

    def refused(module, iv, status, X, state, bed):
        assert _configure_status(module, iv) == status
        np.testing.assert_array_equal(module.initial_values_evaluate(X, 0.0), state)
        np.testing.assert_array_equal(module.initial_precomputed(), bed)

    def struct(name, dim, **kw):
        return capi.initial_values_struct(name, dim, equation=SW, **kw)

    # a selector slot that is none of its integer values
    for value in (0.5, 4.0, -1.0, 2.0):
        refused(msw, struct("flow over bump", 2, flow_type=value), capi.RYUJIN_ERR_ARG, X2, state_before, bed_before)
        refused(msw, struct("three bumps dam break", 2, well_balancing_validation=value), capi.RYUJIN_ERR_ARG, X2,
                state_before, bed_before)
    for value in (0.5, 4.0, 5.0, -1.0):
        refused(msw, struct("transient experiments", 2, experimental_configuration=value), capi.RYUJIN_ERR_ARG, X2,
                state_before, bed_before)
    # ... NaN, perturbation != 0, shallow water in 3-D does not exist; every valid value is taken
    refused(msw, struct("soliton", 2, perturbation=1e-3), capi.RYUJIN_ERR_UNSUPPORTED, X2, state_before, bed_before)
    refused(msw, struct("soliton", 2, amplitude=float("nan")), capi.RYUJIN_ERR_ARG, X2, state_before, bed_before)
    np.testing.assert_array_equal(msw.initial_values_evaluate_initial_precomputed(X2), points_before)
    for value in (0, 1, 2, 3):
        assert _configure_status(msw, struct("transient experiments", 2, experimental_configuration=value)) == 0
    for value in (0, 1):
        assert _configure_status(msw, struct("flow over bump", 2, flow_type=value)) == 0
    # a configure alone does not touch the bed
    np.testing.assert_array_equal(msw.initial_precomputed(), bed_before)
    # n = 0 is fine and writes nothing
    guard = np.full(4, 7.0)
    assert msw._lib.ryujin_hip_initial_values_evaluate_initial_precomputed(
        msw._ctx, None, 0, capi.as_ptr(guard, capi.c_double_p)) == capi.RYUJIN_OK
    assert (guard == 7.0).all()
    assert msw._lib.ryujin_hip_initial_values_evaluate_initial_precomputed(
        msw._ctx, None, 1, capi.as_ptr(guard, capi.c_double_p)) == capi.RYUJIN_ERR_ARG
    msw.close()

    # hou test and transient experiments have no 1-D form
    m1 = HyperbolicModule(off1, hiv.make_params(SW, 1, gravity=9.81), backend="hip")
    m1.initial_values_configure("flow over bump", flow_type="subsonic")
    m1.initial_values_interpolate_initial_precomputed()
    state1, bed1 = m1.initial_values_evaluate(X1, 0.0), m1.initial_precomputed()
    assert len(set(state1[:, 0].tolist())) > 10
    for name in ("hou test", "transient experiments"):
        refused(m1, struct(name, 1), capi.RYUJIN_ERR_UNSUPPORTED, X1, state1, bed1)
    m1.close()

    # an Euler or EulerAEOS context: every new id is a state of another Description (RYUJIN_ERR_ARG, in front of the
    # dimension check: hou test in 1-D is refused for the Description), the three entry points RYUJIN_ERR_UNSUPPORTED
    for eq in (capi.EQ_EULER, capi.EQ_EULER_AEOS):
        for off, X in ((off2, X2), (off1, X1)):
            m = HyperbolicModule(off, hiv.make_params(eq, off.dim), backend="hip")
            assert _bed_entry_statuses(m) == [capi.RYUJIN_ERR_ARG] * 3
            m.initial_values_configure("uniform", primitive_state=(1.25, 0.5, 2.0))
            before = m.initial_values_evaluate(X, 0.0)
            for name in names:
                assert _configure_status(m, struct(name, off.dim)) == capi.RYUJIN_ERR_ARG, name
                np.testing.assert_array_equal(m.initial_values_evaluate(X, 0.0), before)
            assert _bed_entry_statuses(m) == [capi.RYUJIN_ERR_UNSUPPORTED] * 3
            with pytest.raises(RuntimeError, match="status -5"):
                m.initial_precomputed()
            m.close()
    # a scalar context: its function state, and no initial_precomputed values either
    msc = HyperbolicModule(off2, hiv.make_params(capi.EQ_SCALAR_CONSERVATION, 2), backend="hip")
    msc.initial_values_configure_function(["x + 2*y"])
    for name in names:
        assert _configure_status(msc, struct(name, 2)) == capi.RYUJIN_ERR_UNSUPPORTED
    assert _bed_entry_statuses(msc) == [capi.RYUJIN_ERR_UNSUPPORTED] * 3
    msc.close()
