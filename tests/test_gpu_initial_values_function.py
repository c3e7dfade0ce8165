"""The expression-defined "function" state on the device (ryujin_hip_initial_values_configure_function;
ryujin_amd/csrc/expression.hpp, initial_states_device.hpp::initial_state_function, kernels_initial_values.hpp::IvFunctionSource).

1  the device interpreter against the host interpreter (ryujin_hip_expression_evaluate) composed in numpy with the
   affine transform and from_primitive_state: every Description, arithmetic bit for bit, library functions within
   the bounds of tests/helpers_expression.py
2  one function, three consumers: evaluate, interpolate and the Dirichlet kernel give the same bits
3  against the built-in states: constants = uniform bit for bit, the two vortices within the derived tolerance
4  ryujin_hip_time_step_iv against ryujin_hip_time_step_fn fed with initial_values_evaluate, bit for bit
5  the reference's linear-transport baselines from a device-made initial state; compute_error without a download
6  refusals on a live context leave the previous configuration in place
Every test fails on a library without the new entry points (the symbols are missing)."""
import ctypes as C

import numpy as np
import pytest

import helpers_expression as hx
import helpers_initial_values as hiv
from helpers_initial_values import EPS, Case, Err
from ryujin_amd import HyperbolicModule, capi, offline
from ryujin_amd import initial_states as ist
from ryujin_amd.module import StateVector

pytestmark = pytest.mark.gpu

D, DYN = capi.BC_DIRICHLET, capi.BC_DYNAMIC
G = dict(gravity=9.81)
PG = dict(eos=capi.EOS_POLYTROPIC_GAS)

# every Description, with a direction and position that are not the identity (3-D: both rolls)
DESCRIPTIONS = [
    Case("euler 1d", capi.EQ_EULER, 1, "function", {}, (-2.0,), (0.25,)),
    Case("euler 2d", capi.EQ_EULER, 2, "function", {}, (1.0, 1.0), (0.25, -0.125)),
    Case("euler 3d", capi.EQ_EULER, 3, "function", {}, (1.0, 1.0, 1.0), (0.25, -0.125, 0.0625)),
    Case("aeos polytropic 2d", capi.EQ_EULER_AEOS, 2, "function", {}, (1.0, 1.0), (0.25, -0.125), edits=PG),
    Case("aeos nasg 2d", capi.EQ_EULER_AEOS, 2, "function", {}, (1.0, -1.0), (0.25, -0.125), edits=hiv.NASG),
    Case("sw 1d", capi.EQ_SHALLOW_WATER, 1, "function", {}, (1.0,), (-0.5,), edits=G),
    Case("sw 2d", capi.EQ_SHALLOW_WATER, 2, "function", {}, (1.0, 1.0), (0.25, -0.125), edits=G),
    Case("scalar 1d", capi.EQ_SCALAR_CONSERVATION, 1, "function", {}, (1.0,), (1.0,)),
    Case("scalar 2d", capi.EQ_SCALAR_CONSERVATION, 2, "function", {}, (1.0, 1.0), (0.25, -0.125)),
]
IDS = [c.label for c in DESCRIPTIONS]


def n_primitive(case):
    return len(capi.function_expression_names(case.equation, case.dim))


def module_for(case, expressions, off=None):
    off = hiv.tiny_mesh(case.dim) if off is None else off
    m = HyperbolicModule(off, hiv.make_params(case.equation, case.dim, **case.edits), backend="hip")
    m.initial_values_configure_function(expressions, direction=case.direction, position=case.position)
    return m


def from_primitive(case, prim):
    """the Description's from_primitive_state (ryujin_amd.initial_states), the momentum still in the state's frame"""
    p = hiv.make_params(case.equation, case.dim, **case.edits)
    if case.equation == capi.EQ_SCALAR_CONSERVATION:
        return prim[0].reshape(-1, 1)
    vel = np.column_stack(prim[1:1 + case.dim])
    if case.equation == capi.EQ_SHALLOW_WATER:
        return np.column_stack([prim[0], prim[0][:, None] * vel])
    if case.equation == capi.EQ_EULER_AEOS:
        return ist.aeos_from_primitive_state(prim[0], vel, prim[-1])
    return ist.euler_from_primitive(prim[0], vel, prim[-1], p.gamma)


def expected_states(case, expressions, X, t):
    """host interpreter at the transformed points, from_primitive_state, momentum rotated back"""
    Xt = hiv.affine_transform(case.dir(), case.pos(), X)
    U = from_primitive(case, [capi.expression_evaluate(e, case.dim, Xt, t) for e in expressions])
    if case.equation != capi.EQ_SCALAR_CONSERVATION:
        U[:, 1:1 + case.dim] = hiv.affine_transform_vector(case.dir(), U[:, 1:1 + case.dim])
    return U


def points(case, n=1000):
    X = hx.arithmetic_points(case.dim, n)
    return X + np.asarray(case.pos())      # (not exact: the special points move; the comparison is bitwise anyway)


# --------------------------------------------------------------------------- 1

def arithmetic_set(case):
    pool = [e for e, dim, _ in hx.ARITHMETIC if dim <= case.dim][::-1]   # the highest dimension first
    return [pool[q % len(pool)] for q in range(n_primitive(case))]


@pytest.mark.parametrize("case", DESCRIPTIONS, ids=IDS)
def test_arithmetic_sets_equal_the_host_interpreter_bit_for_bit(case):
    """comparisons, if, ?:, min / max, sqrt, rounding and the power rewrite, one expression per primitive component;
    1000 points at two times, and the block edges 1, 63, 64, 65"""
    expressions = arithmetic_set(case)
    m = module_for(case, expressions)
    X = points(case)
    for t in (0.0, 0.375):
        want = expected_states(case, expressions, X, t)
        got = m.initial_values_evaluate(X, t)
        assert got.shape == want.shape == (1000, m.k)
        np.testing.assert_array_equal(got, want, err_msg=f"{case.label} t = {t}")
        for n in (1, 63, 64, 65):
            np.testing.assert_array_equal(m.initial_values_evaluate(X[:n], t), want[:n])
    m.close()


def composite_set(case):
    pool = [(e, fn) for e, dim, fn in hx.COMPOSITES if dim <= case.dim]
    # density-like first component: keep it positive (2 + ... in 1-D, exp(...) sin + cos may change sign in 2-D: fine,
    # from_primitive_state is arithmetic)
    return [pool[q % len(pool)] for q in range(n_primitive(case))]


def composite_bound(case, fns, X, t):
    """(values [n, k], bound [n, k]): the COMPOSITES in the error arithmetic at the transformed points -- which the
    device and numpy form with the same operations on the same doubles: exact --, from_primitive_state and the
    rotation of the momentum in the same arithmetic"""
    p = hiv.make_params(case.equation, case.dim, **case.edits)
    Xt = hiv.affine_transform(case.dir(), case.pos(), X)
    cols = [Err(Xt[:, d]) if d < case.dim else None for d in range(3)]
    prim = [fn(cols[0], cols[1], cols[2], t) for fn in fns]
    prim = [Err(q.v + np.zeros(len(X)), q.e + np.zeros(len(X))) for q in prim]
    if case.equation == capi.EQ_SCALAR_CONSERVATION:
        comps = prim
    else:
        vel = prim[1:1 + case.dim]
        m = hiv._rotate_err(case, [prim[0] * v for v in vel])
        comps = [prim[0], *m]
        if case.equation != capi.EQ_SHALLOW_WATER:
            v2 = vel[0] * vel[0]
            for v in vel[1:]:
                v2 = v2 + v * v
            kinetic = 0.5 * prim[0] * v2
            comps.append(prim[0] * prim[-1] + kinetic if case.equation == capi.EQ_EULER_AEOS
                         else prim[-1] / (Err(p.gamma) - 1.0) + kinetic)
    return np.column_stack([c.v for c in comps]), np.column_stack([c.e for c in comps])


@pytest.mark.parametrize("case", DESCRIPTIONS, ids=IDS)
def test_exp_sin_cos_pow_sets_within_the_error_arithmetic(case):
    chosen = composite_set(case)
    expressions, fns = [e for e, _ in chosen], [fn for _, fn in chosen]
    m = module_for(case, expressions)
    X = points(case)
    for t in (0.0, 0.375):
        want = expected_states(case, expressions, X, t)
        values, bound = composite_bound(case, fns, X, t)
        got = m.initial_values_evaluate(X, t)
        assert np.isfinite(got).all()
        # the error arithmetic reproduces the host interpreter's values up to its own bound
        assert (np.abs(values - want) <= bound).all()
        err = np.abs(got - want)
        print(f"{case.label} t={t}: max err / bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
        assert (err <= bound).all(), (case.label, t, float((err - bound).max()))
        assert (bound <= 1e-12 * (1.0 + np.abs(want))).all()      # (the bound is no licence: a few hundred ulp at most)
    m.close()


def test_every_library_function_against_the_host_interpreter():
    """One function per configure on a scalar 1-D context, 1000 arguments each from the interval where its condition
    number is at most 4 (tests/helpers_expression.py). The argument is the same double on both sides (position 0,
    direction 1: x - 0 is exact), so the conditioning term is zero and the cap is B_f EPS |result|: the project's B_f
    for exp, sin, cos, sqrt, pow; 16 for the functions it states none for -- a condition that catches a wrong opcode
    or a wrong function, not an accuracy claim. Prints the measured maximum per function in ulp
    (profiles/initial_values_function_timing.md)."""
    case = Case("scalar 1d", capi.EQ_SCALAR_CONSERVATION, 1, "function")
    m = module_for(case, ["x"])
    failures = []
    for name, expr, lower, upper, _, b_f in hx.FUNCTIONS:
        X = hx.function_points(lower, upper)
        m.initial_values_configure_function([expr])
        got = m.initial_values_evaluate(X, 0.0)[:, 0]
        want = capi.expression_evaluate(expr, 1, X, 0.0)
        ulp = np.abs(got - want) / np.spacing(np.abs(want))
        print(f"{name}: max |device - host| = {ulp.max():.2f} ulp on [{lower}, {upper}] (cap {2 * b_f:g} ulp)")
        if not (np.abs(got - want) <= hx.function_bound(want, b_f)).all():
            failures.append((name, float(ulp.max())))
    for expr, _, exponent in hx.POW:
        X = hx.pow_points()
        x = X[:, 0]
        m.initial_values_configure_function([expr])
        got = m.initial_values_evaluate(X, 0.0)[:, 0]
        want = capi.expression_evaluate(expr, 1, X, 0.0)
        ulp = np.abs(got - want) / np.spacing(np.abs(want))
        print(f"{expr}: max |device - host| = {ulp.max():.2f} ulp")
        if not (np.abs(got - want) <= hx.pow_bound(x, exponent(x), want)).all():
            failures.append((expr, float(ulp.max())))
    m.close()
    assert not failures, failures


# --------------------------------------------------------------------------- 2

TRAVELLING_WAVE = ["1.5 + 0.5 * sin(_pi * (x - t))", "1", "1"]     # an exact solution of the Euler equations
CONSUMER_CASES = {
    # odd states (k = 1, 3, 5) carry a pad lane in the state vector
    "scalar 1d 65 nodes": (lambda: hiv.interval(64, 0.0, 1.0, D, D), DESCRIPTIONS[7], ["sin(x - t)"]),
    "euler 2d 40x33": (lambda: hiv.vortex_mesh(40, 33), DESCRIPTIONS[1],
                       ["1.5 + 0.5 * sin(x - t)", "1 + 0.1 * y", "0.25 * cos(x)", "1 + 0.1 * exp(-x*x)"]),
    "euler 3d 5x4x3": (lambda: offline.SyntheticOffline(offline.MeshSpec(3, (5, 4, 3), (-1.0,) * 3, (1.0,) * 3,
                                                                         (D,) * 6)), DESCRIPTIONS[2],
                       ["1.5 + 0.5 * sin(x - t)", "1", "0.1 * z", "y * t", "2 + x * y * z"]),
    "sw 2d 9x7": (lambda: hiv.vortex_mesh(9, 7), DESCRIPTIONS[6], ["1 + 0.1 * sin(x - t)", "0.5", "0.1 * y"]),
}


@pytest.mark.parametrize("name", sorted(CONSUMER_CASES))
def test_three_consumers_give_the_same_bits(name):
    """interpolate + download == evaluate(positions) on every row; prepare_state_vector with dirichlet="device"
    leaves the same state as the host path fed with evaluate(b_positions), and evaluate(b_positions) itself at the
    boundary rows of these all-Dirichlet meshes"""
    make, case, expressions = CONSUMER_CASES[name]
    off = make()
    if name == "euler 2d 40x33":
        assert off.n_bdry > 2 * 64 and off.n_bdry % 64 != 0
    m = module_for(case, expressions, off)
    t = 0.3
    expected = m.initial_values_evaluate(off.positions, t)
    assert np.isfinite(expected).all() and np.abs(expected).max() > 0.0
    sv = m.new_state_vector(np.full((off.n_relevant, m.k), np.nan))
    m.initial_values_interpolate(sv, t)
    np.testing.assert_array_equal(sv.download(), expected)

    U0 = 1.5 * m.initial_values_evaluate(off.positions, 0.0) + 0.01
    boundary = m.initial_values_evaluate(off.b_positions, t)
    a, b = m.new_state_vector(U0), m.new_state_vector(U0)
    m.prepare_state_vector(a, t, "device")
    m.prepare_state_vector(b, t, boundary)
    A = a.download()
    np.testing.assert_array_equal(A, b.download())
    np.testing.assert_array_equal(A[off.b_i], boundary)
    assert (U0[off.b_i, 0] != boundary[:, 0]).all()
    m.close()


# --------------------------------------------------------------------------- 3

@pytest.mark.parametrize("case", DESCRIPTIONS[:3], ids=IDS[:3])
def test_constant_expressions_equal_uniform_bit_for_bit(case):
    m = module_for(case, {})                     # the reference's defaults: 1.4, 3.0, 0.0 ..., 1.0
    X = points(case, 200)
    got = m.initial_values_evaluate(X, 0.25)
    m.initial_values_configure("uniform", primitive_state=(1.4, 3.0, 1.0), direction=case.direction,
                               position=case.position)
    np.testing.assert_array_equal(got, m.initial_values_evaluate(X, 0.25))
    assert (got[:, 1:-1] != 0.0).all()           # the rotated direction reaches every momentum component
    m.close()


def _vortex_expressions(beta, mach):
    xb = f"(x - {mach!r} * t)"
    F = f"({beta!r} / (2 * _pi) * exp(0.5 - 0.5 * ({xb} * {xb} + y * y)))"
    return xb, F


def test_isentropic_vortex_as_expressions_against_the_built_in():
    case = next(c for c in hiv.function_cases() if c.label == "euler isentropic vortex")
    xb, F = _vortex_expressions(5.0, 1.0)
    T = f"(1 - (1.4 - 1) / (2 * 1.4) * {F} * {F})"
    rho = f"pow({T}, 1 / (1.4 - 1))"
    expressions = [rho, f"1.0 - {F} * y", f"{F} * {xb}", f"pow({rho}, 1.4)"]
    _against_built_in(case, expressions)


def test_smooth_vortex_as_expressions_against_the_built_in():
    case = next(c for c in hiv.function_cases() if c.label == "sw smooth vortex")
    xb, F = _vortex_expressions(2.0, 1.0)
    expressions = [f"2.0 - 1 / (2 * 9.81) * {F} * {F}", f"1.0 - {F} * y", f"{F} * {xb}"]
    _against_built_in(case, expressions)


def _against_built_in(case, expressions):
    """the expressions follow ryujin_amd.initial_states statement by statement: within the derived tolerance of the
    numpy restatement (helpers_initial_values.tolerance), and within twice that of the built-in state, which is held
    to the same tolerance"""
    m = hiv.module_for(case)
    X = hiv.points_for(case)
    for t in case.times:
        built_in = m.initial_values_evaluate(X, t)
        m.initial_values_configure_function(expressions, direction=case.direction, position=case.position)
        got = m.initial_values_evaluate(X, t)
        hiv.configure(m, case)
        ref = hiv.reference(case, X, t)
        _, tol = hiv.tolerance(case, X, t)
        print(f"{case.label} t={t}: max |function - numpy| / tol {(np.abs(got - ref) / np.maximum(tol, 1e-300)).max():.3f}, "
              f"rows identical to the built-in: {int((got == built_in).all(axis=1).sum())} of {len(X)}")
        assert (np.abs(got - ref) <= tol).all()
        assert (np.abs(got - built_in) <= 2.0 * tol).all()
    m.close()


# --------------------------------------------------------------------------- 4

def scalar_params(dim, cfl=0.5):
    """flux "function: u" in x, as the reference's linear-transport runs"""
    p = hiv.make_params(capi.EQ_SCALAR_CONSERVATION, dim)
    p.sc_flux = capi.FLUX_POLYNOMIAL
    for d in range(3):
        for n in range(4):
            p.sc_flux_polynomial[d][n] = 0.0
    p.sc_flux_polynomial[0][1] = 1.0
    p.sc_derivative_approximation_delta = 1e-10
    p.indicator_evc_factor = 0.0
    p.cfl = cfl
    return p


def drive(m, scheme, n_steps, device, cfl, b_positions=None, cfl_recovery="none", cfl_min=None, cfl_max=None):
    """n_steps Runge-Kutta steps of the configured function state from t = 0. device: the initial state from
    initial_values_interpolate, every step ryujin_hip_time_step_iv; otherwise the uploaded evaluate(positions, 0) and
    ryujin_hip_time_step_fn with a callback that returns evaluate(b_positions, time)."""
    cfl_min = cfl if cfl_min is None else cfl_min
    cfl_max = cfl if cfl_max is None else cfl_max
    m.cfl = cfl_max
    bpos = m.offline.b_positions if b_positions is None else b_positions
    if device:
        state = m.new_state_vector()
        m.initial_values_interpolate(state, 0.0)
    else:
        state = m.new_state_vector(m.initial_values_evaluate(m.offline.positions, 0.0))
    temps = [m.new_state_vector() for _ in range(hiv.N_TEMPS.get(scheme, 3))]
    fn = None if device else (lambda time: m.initial_values_evaluate(bpos, time))
    states, taus, t = [], [], 0.0
    for _ in range(n_steps):
        tau = m.time_step(scheme, state, temps, "device" if device else None, cfl_recovery=cfl_recovery,
                          cfl_min=cfl_min, cfl_max=cfl_max, t=t, dirichlet_fn=fn)
        t += tau
        taus.append(tau)
        states.append(state.download())
    return states, taus, m.n_restarts()


SW_EDITS = dict(gravity=9.81, reference_water_depth=1.0, dry_state_relaxation_factor=0.2,
                dry_state_relaxation_small=1e4, dry_state_relaxation_large=1e4)
XB, F_VORTEX = _vortex_expressions(5.0, 1.0)
T_VORTEX = f"(1 - (1.4 - 1) / (2 * 1.4) * {F_VORTEX} * {F_VORTEX})"
VORTEX_EXPRESSIONS = [f"pow({T_VORTEX}, 1 / (1.4 - 1))", f"1.0 - {F_VORTEX} * y", f"{F_VORTEX} * {XB}",
                      f"pow(pow({T_VORTEX}, 1 / (1.4 - 1)), 1.4)"]
VORTEX_FRAME = dict(direction=(1.0, 1.0), position=(-1.0, -1.0))

DRIVER_CASES = {
    # name: (mesh, params, expressions, frame, scheme, cfl, recovery)
    **{f"euler 1d travelling wave {s}": (
        lambda: hiv.interval(100, 0.0, 2.0, D, D), lambda: hiv.make_params(capi.EQ_EULER, 1), TRAVELLING_WAVE, {}, s,
        0.2, {}) for s in ("ssprk 33", "erk 33", "erk 54")},
    "scalar 2d sin(x - t)": (lambda: offline.SyntheticOffline(offline.rectangle_2d(16, (0.0, 0.0), (2.0, 1.0), bc=D)),
                             lambda: scalar_params(2), ["sin(x - t)"], {}, "erk 33", 0.5, {}),
    "shallow water 1d dynamic": (lambda: hiv.interval(100, 0.0, 10.0, DYN, DYN),
                                 lambda: hiv.make_params(capi.EQ_SHALLOW_WATER, 1, **SW_EDITS),
                                 ["1 + 0.2 * sin(0.5 * (x - t))", "1"], {}, "erk 33", 0.5, {}),
    "euler 2d vortex bang bang": (lambda: hiv.vortex_mesh(32), lambda: hiv.make_params(capi.EQ_EULER, 2),
                                  VORTEX_EXPRESSIONS, VORTEX_FRAME, "erk 33", 0.3,
                                  dict(cfl_recovery="bang bang control", cfl_min=0.3, cfl_max=3.0)),
}
N_STEPS = 20


@pytest.mark.parametrize("name", sorted(DRIVER_CASES))
def test_time_step_iv_equals_the_callback_path_bit_for_bit(name):
    """20 Runge-Kutta steps twice: on the device from start (interpolate, time_step_iv) and through the callback path
    (upload, time_step_fn with evaluate) -- the same device function on the same doubles. Every state and every tau
    identical; the bang-bang case restarts."""
    make, params, expressions, frame, scheme, cfl, recovery = DRIVER_CASES[name]
    results = []
    for device in (True, False):
        off = make()
        m = HyperbolicModule(off, params(), backend="hip")
        m.initial_values_configure_function(expressions, **frame)
        results.append(drive(m, scheme, N_STEPS, device, cfl, **recovery))
        m.close()
    (states_iv, taus_iv, restarts_iv), (states_fn, taus_fn, restarts_fn) = results
    assert taus_iv == taus_fn, (taus_iv, taus_fn)
    assert all(tau > 0.0 for tau in taus_iv)
    for step, (a, b) in enumerate(zip(states_iv, states_fn)):
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b, err_msg=f"{name}: after step {step}")
    assert not np.array_equal(states_iv[0], states_iv[-1])
    assert restarts_iv == restarts_fn
    if recovery:
        assert restarts_iv > 0


def test_three_ranks_one_without_boundary():
    """The vortex as expressions on three in-process ranks, every rank configured with its own positions; rank 1 owns
    no boundary entry (asserted). interpolate fills the ghost rows with evaluate's bits; the gathered states after
    every step and every tau equal the three-rank callback run."""
    from helpers_partitioned import run_hip_ranks
    from helpers_unstructured import disk_points, p1_offline, partition
    pts = 5.0 * disk_points(18)
    off, info = p1_offline(pts, boundary_id=D)
    r = np.linalg.norm(pts, axis=1)
    owner = np.where(r < 2.0, 1, np.where(pts[:, 0] < 0.0, 0, 2))
    views = partition(off, info, owner)
    assert [v.n_bdry > 0 for v in views] == [True, False, True]
    n_steps = 10

    def body(device):
        def run(m, part, rank):
            m.initial_values_configure_function(VORTEX_EXPRESSIONS, **VORTEX_FRAME)
            assert part.n_relevant > part.n_owned
            sv = m.new_state_vector(np.full((part.n_relevant, m.k), np.nan))
            m.initial_values_interpolate(sv, 0.3)
            np.testing.assert_array_equal(sv.download(), m.initial_values_evaluate(part.positions, 0.3))
            states, taus, _ = drive(m, "erk 33", n_steps, device, 0.3, b_positions=part.b_positions)
            return [s[: part.n_owned] for s in states], taus
        return run

    params = lambda: hiv.make_params(capi.EQ_EULER, 2)  # noqa: E731
    out_iv = run_hip_ranks(views, params, body(True))
    out_fn = run_hip_ranks(views, params, body(False))
    for rank in range(3):
        assert out_iv[rank][1] == out_fn[rank][1] == out_iv[0][1]
    for step in range(n_steps):
        gathered = []
        for out in (out_iv, out_fn):
            U = np.full((len(pts), 4), np.nan)
            for rank, v in enumerate(views):
                U[v.global_ids[: v.n_owned]] = out[rank][0][step]
            gathered.append(U)
        assert np.isfinite(gathered[0]).all()
        np.testing.assert_array_equal(gathered[0], gathered[1], err_msg=f"after step {step}")


# --------------------------------------------------------------------------- 5

@pytest.mark.parametrize("scheme", ["ssprk 22", "ssprk 33", "erk 11", "erk 22", "erk 33", "erk 43", "erk 54"])
def test_linear_transport_golden_from_a_device_made_initial_state(golden_dir, scheme):
    """tests/scalar_conservation/verification-linear_transport-*.prm with the initial state of its parameter file --
    configuration = function, expression sin(x-t), position 1, direction 1 -- interpolated on the device; the run,
    the norms and the tolerances of test_gpu_parity.test_scalar_linear_transport_golden_on_gpu. One download at the
    end: the periodic mesh carries a constrained DoF that the device's error norms have no counterpart for."""
    from ryujin_amd import TimeIntegrator
    from test_oracle_golden_scalar import _norms_1d, golden_linear_transport, periodic_interval
    dofs, t_ref, linf_ref, l1_ref, l2_ref = golden_linear_transport(golden_dir, scheme)
    n_cells = 2 ** 9
    off, h = periodic_interval(n_cells, 6.28318530718)
    p = scalar_params(1)
    p.limiter_iterations = 2
    p.limiter_relaxation_factor = 1.0
    m = HyperbolicModule(off, p, backend="hip")
    m.initial_values_configure_function({"expression": "sin(x-t)"}, position=(1.0,), direction=(1.0,))
    sv = m.new_state_vector()
    m.initial_values_interpolate(sv, 0.0)
    cfl = {"erk 11": 0.05, "erk 22": 0.20}.get(scheme, 0.80)
    ti = TimeIntegrator(m, scheme, cfl_min=cfl, cfl_max=cfl, cfl_recovery_strategy="none")
    t = 0.0
    while t < 2.0:
        sv, tau = ti.step(sv, t)
        t += tau
    U = sv.download()[:, 0].copy()
    U[n_cells] = U[0]
    A = np.sin((off.positions - 1.0) - t)[:, 0]
    e = U - A
    (l1a, l2a), (l1e, l2e) = _norms_1d(A, h), _norms_1d(e, h)
    linf, l1, l2 = np.abs(e).max() / np.abs(A).max(), l1e / l1a, l2e / l2a
    print(f"{scheme}: t {t!r} ({t_ref!r}), Linf {linf!r} ({linf_ref!r}), L1 {l1!r} ({l1_ref!r}), L2 {l2!r} ({l2_ref!r})")
    assert off.n_owned == dofs
    assert abs(t - t_ref) < 1e-10
    assert abs(linf - linf_ref) < 2e-5 * linf_ref
    assert abs(l1 - l1_ref) < 2e-5 * l1_ref
    assert abs(l2 - l2_ref) < 2e-5 * l2_ref
    m.close()


def test_compute_error_on_the_scalar_dirichlet_case_without_a_download(monkeypatch):
    """the 2-D scalar case of test 4 through DeviceResidentTimeIntegrator(dirichlet="device") and compute_error(state,
    t) with StateVector.download refused; afterwards both vectors are downloaded for the numpy restatement of
    tests/helpers_error_norms.py and compared under its derived bounds"""
    import helpers_error_norms as hen
    from ryujin_amd import error_norms
    from ryujin_amd.module import DeviceResidentTimeIntegrator
    off = offline.SyntheticOffline(offline.rectangle_2d(16, (0.0, 0.0), (2.0, 1.0), bc=D))
    m = HyperbolicModule(off, scalar_params(2), backend="hip")
    m.initial_values_configure_function(["sin(x - t)"])
    shape, weights = error_norms.q1_tables(2)
    measure = np.full(off.n_cells, off.cell_measure)
    m.error_norms_configure(off.cells, shape, measure, weights)
    download = StateVector.download

    def refuse(self):
        raise AssertionError("the state is never downloaded in this run")
    monkeypatch.setattr(StateVector, "download", refuse)
    sv = m.new_state_vector()
    m.initial_values_interpolate(sv, 0.0)
    ti = DeviceResidentTimeIntegrator(m, "erk 33", cfl_min=0.5, cfl_max=0.5, cfl_recovery_strategy="none",
                                      dirichlet="device")
    t = 0.0
    for _ in range(N_STEPS):
        sv, tau = ti.step(sv, t)
        t += tau
    out, detail = m.compute_error(sv, t)
    monkeypatch.setattr(StateVector, "download", download)

    analytic = m.new_state_vector()
    m.initial_values_interpolate(analytic, t)
    U, A = sv.download(), analytic.download()
    np.testing.assert_array_equal(A, m.initial_values_evaluate(off.positions, t))
    ref = hen.restatement(U, A, off.n_owned, off.cells, shape, measure, [0], True, weights,
                          D=hen.chain_length([off.n_cells], shape.shape[0]))
    hen.compare("scalar 2d sin(x - t)", out, detail, ref)
    assert 0.0 < out[1] < 0.1           # a first-order error of a resolved wave, not zero and not O(1)
    m.close()


# --------------------------------------------------------------------------- 6

def _configure_function_status(m, expressions):
    off = m.offline
    texts = (C.c_char_p * len(expressions))(*[e.encode() for e in expressions])
    d, x = np.array([1.0, 0.0, 0.0]), np.zeros(3)
    pos = np.ascontiguousarray(off.positions, dtype=np.float64).reshape(-1)
    bpos = np.ascontiguousarray(off.b_positions, dtype=np.float64).reshape(-1)
    p = lambda a: capi.as_ptr(a, capi.c_double_p)  # noqa: E731
    return m._lib.ryujin_hip_initial_values_configure_function(m._ctx, len(expressions), texts, p(d), p(x), p(pos),
                                                               p(bpos))


@pytest.mark.parametrize("previous", ["function", "analytic"])
def test_refusals_leave_the_previous_configuration_in_place(previous):
    lib = capi.load_hip()
    off = hiv.tiny_mesh(2)
    m = HyperbolicModule(off, hiv.make_params(capi.EQ_EULER, 2), backend="hip")
    good = ["1 + x*x", "y", "t", "2 + x"]
    if previous == "function":
        m.initial_values_configure_function(good, direction=(1.0, 1.0), position=(0.5, 0.25))
    else:
        m.initial_values_configure("isentropic vortex", mach_number=1.0, beta=5.0, direction=(1.0, 1.0))
    X = hx.arithmetic_points(2, 100)
    before = m.initial_values_evaluate(X, 0.5)
    for expressions, status, needle in ((good[:3], capi.RYUJIN_ERR_ARG, b"expressions"),
                                        (good + ["1"], capi.RYUJIN_ERR_ARG, b"expressions"),
                                        (["1", "x + foo", "0", "1"], capi.RYUJIN_ERR_ARG, b"at character 4"),
                                        (["1", "0", "z", "1"], capi.RYUJIN_ERR_ARG, b"at character 0"),
                                        (["1", "0", "0", "1 + rand(1)"], capi.RYUJIN_ERR_UNSUPPORTED,
                                         b"at character 4")):
        assert _configure_function_status(m, expressions) == status
        assert needle in lib.ryujin_hip_last_error(), lib.ryujin_hip_last_error()
        np.testing.assert_array_equal(m.initial_values_evaluate(X, 0.5), before)
    with pytest.raises(RuntimeError, match="direction"):
        m.initial_values_configure_function(good, direction=(0.0, 0.0))
    np.testing.assert_array_equal(m.initial_values_evaluate(X, 0.5), before)
    m.close()


def test_configure_and_configure_function_replace_each_other():
    off = hiv.tiny_mesh(2)
    m = HyperbolicModule(off, hiv.make_params(capi.EQ_EULER, 2), backend="hip")
    X = hx.arithmetic_points(2, 100)
    m.initial_values_configure("uniform", primitive_state=(1.0, 2.0, 3.0))
    uniform = m.initial_values_evaluate(X, 0.0)
    m.initial_values_configure_function(["1 + x*x", "y", "t", "2 + x"])
    function = m.initial_values_evaluate(X, 0.0)
    assert not np.array_equal(uniform, function)
    np.testing.assert_array_equal(function[:, 0], 1.0 + X[:, 0] * X[:, 0])
    m.initial_values_configure("uniform", primitive_state=(1.0, 2.0, 3.0))
    np.testing.assert_array_equal(m.initial_values_evaluate(X, 0.0), uniform)
    m.initial_values_configure_function(["2", "0", "0", "1"])
    np.testing.assert_array_equal(m.initial_values_evaluate(X, 0.0)[:, 0], np.full(100, 2.0))
    m.close()


def test_scalar_context_takes_the_function_state_only():
    off = hiv.tiny_mesh(2)
    m = HyperbolicModule(off, scalar_params(2), backend="hip")
    X = hx.arithmetic_points(2, 100)
    with pytest.raises(RuntimeError, match="status -5"):
        m.initial_values_configure("uniform")
    with pytest.raises(RuntimeError, match="status -2"):
        m.initial_values_evaluate(X, 0.0)                      # nothing configured
    m.initial_values_configure_function([hx.KPP])
    got = m.initial_values_evaluate(X, 0.0)
    np.testing.assert_array_equal(got[:, 0], capi.expression_evaluate(hx.KPP, 2, X, 0.0))
    assert set(got[:, 0].tolist()) == {0.78539816339, 0.78539816339 * 14.0}
    with pytest.raises(RuntimeError, match="status -5"):
        m.initial_values_configure("uniform")                  # ... and the function state stays
    np.testing.assert_array_equal(m.initial_values_evaluate(X, 0.0), got)
    m.close()
