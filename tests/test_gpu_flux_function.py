"""The expression-defined flux "function" of the scalar conservation equation on the device (RYUJIN_FLUX_FUNCTION,
ryujin_hip_flux_configure_function; kernels k_precompute_sc_function, k_dij_alpha_sc_function,
k_dij_boundary_sc_function of ryujin_amd/csrc/scalar_conservation_device.hpp).

 1  the precomputed values f(u) and (f(u + d) - f(u - d)) / (2 d) against the host interpreter of the same source
 2  one update against the oracle (helpers_parity.compare_step, unchanged): the oracle runs RYUJIN_FLUX_POLYNOMIAL, the
    device the same polynomial written as an expression in Horner form -- the same IEEE operations in the same order
 3  d_ij of a non-polynomial flux (Buckley-Leverett) with averaged entropy against the Riemann solver restated in numpy
 4  20 Runge-Kutta steps, function flux against polynomial flux on the device, bit for bit; three ranks
 5  the linear-transport baselines with the flux "u" given as an expression
 6  Buckley-Leverett in 1-D: maximum principle and mass balance
 7  life cycle: refusals, replacement, the Descriptions without a flux
The oracle refuses every flux kind above POLYNOMIAL (oracle/scalar_conservation.hpp); non-polynomial fluxes are checked
where the flux enters -- the precomputed values (1) and d_ij (3) --, everything behind those two arrays is the code the
polynomial cases of (2) and (4) cover."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import helpers_expression as hx
import helpers_flux_function as hf
from helpers_parity import compare_step
from ryujin_amd import HyperbolicModule, capi

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def function_module(off, p_polynomial, expression, delta=hf.DELTA, **kw):
    """a device module with RYUJIN_FLUX_FUNCTION and otherwise the parameters of `p_polynomial`"""
    m = HyperbolicModule(off, hf.function_params(p_polynomial), backend="hip", **kw)
    m.flux_configure_function(expression, delta)
    return m


def scalar_params(dim, *, averaged=False, greedy=False, cfl=0.5):
    lib = capi.load_hip()
    p = capi.Params()
    lib.ryujin_hip_default_params(C.byref(p), capi.EQ_SCALAR_CONSERVATION, dim)
    p.cfl = cfl
    p.sc_use_averaged_entropy = 1 if averaged else 0
    p.sc_use_greedy_wavespeed = 1 if greedy else 0
    return p


# --------------------------------------------------------------------------- 1

def precomputed_on_the_device(mesh, expression, delta, fold=True):
    """(u [n], prec [n, 2 dim]) of random states in [-2, 2] on a mesh with a Dirichlet boundary"""
    off = hf.mesh(mesh)
    p = scalar_params(off.dim)
    p.sc_flux = capi.FLUX_FUNCTION
    if not fold:
        p.debug_bc_fold_max_slices = -1
    m = HyperbolicModule(off, p, backend="hip")
    m.flux_configure_function(expression, delta)
    U = np.random.default_rng(13).uniform(-2.0, 2.0, size=(off.n_owned, 1))
    sv = m.new_state_vector(U)
    m.prepare_state_vector(sv, 0.0, U[np.asarray(off.b_i).astype(np.int64)])
    prec = sv.download_precomputed()[: off.n_owned].reshape(off.n_owned, 2 * off.dim)
    np.testing.assert_array_equal(sv.download()[: off.n_owned], U)   # (the Dirichlet data is the state's own)
    assert m.flux_info()["kind"] == capi.FLUX_FUNCTION
    m.close()
    return off, U[:, 0], prec


@pytest.mark.parametrize("name", sorted(hf.ARITHMETIC_SETS))
@pytest.mark.parametrize("fold", [True, False], ids=["bc-folded", "bc-launch"])
def test_precomputed_values_of_arithmetic_fluxes_bit_for_bit(name, fold):
    """40 x 48 nodes, 1920 states: exactly rounded operations only, so the device and the host interpreter give the same
    bits for the value and for the difference quotient (and the host interpreter equals numpy: test_flux_function_cpu)"""
    expression, fns = hf.ARITHMETIC_SETS[name]
    off, u, prec = precomputed_on_the_device("plane", expression, hf.DELTA, fold)
    assert len(u) == 1920
    value, gradient = capi.flux_function_evaluate(expression, 2, u, hf.DELTA)
    np.testing.assert_array_equal(prec[:, :2], value)
    np.testing.assert_array_equal(prec[:, 2:], gradient)
    for d, fn in enumerate(fns):
        np.testing.assert_array_equal(prec[:, d], fn(u))


@pytest.mark.parametrize("name", sorted(hf.LIBRARY_SETS))
def test_precomputed_values_of_library_fluxes_within_the_function_caps(name):
    """sin, cos, exp, tanh: the device's library against the host's. Value: B_f eps |f| (helpers_expression.py).
    Gradient, with delta = 1e-5: both f(u + d) and f(u - d) may differ by the cap, (B_f ulp(|f|) 2) / (2 delta) with
    ulp(|f|) = eps max(|f(u + d)|, |f(u - d)|) -- 6.7e-11 where |f| = 1 and B_f = 3."""
    expression, parts = hf.LIBRARY_SETS[name]
    delta = hf.DELTA_LIBRARY
    off, u, prec = precomputed_on_the_device("plane", expression, delta)
    value, gradient = capi.flux_function_evaluate(expression, 2, u, delta)
    plus, _ = capi.flux_function_evaluate(expression, 2, u + delta, delta, gradient=False)
    minus, _ = capi.flux_function_evaluate(expression, 2, u - delta, delta, gradient=False)
    for d, (_, b_f) in enumerate(parts):
        excess = np.abs(prec[:, d] - value[:, d]) / np.maximum(hx.function_bound(value[:, d], b_f), 1e-300)
        bound = hf.library_gradient_bound(plus[:, d], minus[:, d], b_f, delta)
        g_excess = np.abs(prec[:, 2 + d] - gradient[:, d]) / np.maximum(bound, 1e-300)
        print(f"{name} component {d}: value {excess.max():.3f} of its bound, gradient {g_excess.max():.3f} of its bound, "
              f"identical values {int((prec[:, d] == value[:, d]).sum())} of {len(u)}")
        assert excess.max() <= 1.0
        assert g_excess.max() <= 1.0


def test_precomputed_values_in_1d_and_3d():
    """400 nodes with Buckley-Leverett; 8^3 nodes with three different cubics"""
    off, u, prec = precomputed_on_the_device("line", hf.BUCKLEY_LEVERETT, hf.DELTA)
    assert len(u) == 400
    value, gradient = capi.flux_function_evaluate(hf.BUCKLEY_LEVERETT, 1, u, hf.DELTA)
    np.testing.assert_array_equal(prec, np.concatenate([value, gradient], axis=1))
    np.testing.assert_array_equal(prec[:, 0], hf.buckley_leverett(u))
    expression, fns = hf.polynomial_flux(hf.CUBIC, 3)
    off, u, prec = precomputed_on_the_device("box", expression, hf.DELTA)
    assert len(u) == 512
    value, gradient = capi.flux_function_evaluate(expression, 3, u, hf.DELTA)
    np.testing.assert_array_equal(prec, np.concatenate([value, gradient], axis=1))
    assert len({fn(0.75) for fn in fns}) == 3


# --------------------------------------------------------------------------- 2

def lattice_case(width, coefficients, averaged, greedy):
    """the width-10 / width-65 lattice of helpers_row_width_cases.py with its data, the flux a polynomial"""
    import helpers_row_width_cases as rwc

    def edit(p):
        q = hf.polynomial_params(None, 2, coefficients, averaged=averaged, greedy=greedy, base=p)
        assert q is p
    return dict(rwc.CASES[f"scalar_2d_{width}"], edit=edit)


UPDATE_CASES = [
    # (mesh, coefficients, averaged entropy, greedy wavespeed)
    ("line", hf.TRANSPORT, False, False), ("line", hf.TRANSPORT, True, False),
    ("plane", hf.BURGERS, False, False), ("plane", hf.BURGERS, True, False), ("plane", hf.BURGERS, True, True),
    ("plane", hf.CUBIC, False, False), ("plane", hf.CUBIC, True, False), ("plane", hf.CUBIC, True, True),
    (10, hf.CUBIC, False, False), (10, hf.CUBIC, True, False),
    (65, hf.CUBIC, False, False), (65, hf.CUBIC, True, False),
    ("box", hf.CUBIC, False, False), ("box", hf.CUBIC, True, False),
]
NAMES = {id(hf.TRANSPORT): "transport", id(hf.BURGERS): "burgers", id(hf.CUBIC): "cubic"}


@pytest.mark.parametrize("mesh, coefficients, averaged, greedy", UPDATE_CASES,
                         ids=[f"{m}-{NAMES[id(c)]}-avg{int(a)}" + ("-greedy" if g else "") for m, c, a, g in UPDATE_CASES])
def test_one_update_against_the_oracle(oracle, mesh, coefficients, averaged, greedy):
    """compare_step with its own tolerances: the device runs RYUJIN_FLUX_FUNCTION with the polynomial in Horner form, the
    oracle RYUJIN_FLUX_POLYNOMIAL with the coefficients, on a state developed on the oracle. With averaged entropy step 2
    and the boundary pairs run the interpreter kernels (flux_info), and the data must let lambda_left / lambda_right
    decide d_ij -- in interior pairs and, on a mesh with boundary pairs, in boundary pairs -- wherever the flux allows it
    at all (helpers_flux_function.CUBIC: a convex flux only with the greedy wavespeed, the linear flux never)."""
    row_slack = None
    if isinstance(mesh, int):
        import helpers_row_width_cases as rwc
        case = lattice_case(mesh, coefficients, averaged, greedy)
        off, dirichlet, states, _, tau = rwc.develop(case, oracle)
        U = states[-1]
        import helpers_plan_cases as plan_cases
        p = plan_cases.params_of(case, oracle, off.dim)
        row_slack = rwc.summation_slack(off, "scalar")
    else:
        off = hf.mesh(mesh)
        p = hf.polynomial_params(oracle, off.dim, coefficients, averaged=averaged, greedy=greedy)
        U, dirichlet = hf.develop(off, p, oracle)
        tau = 0.0
    expression, _ = hf.polynomial_flux(coefficients, off.dim)
    label = f"flux function {mesh} {NAMES[id(coefficients)]} averaged={int(averaged)} greedy={int(greedy)}"

    if averaged and (coefficients is hf.CUBIC or greedy):
        counts = hf.averaged_entropy_coverage(off, hf.oracle_arrays(off, p, oracle, U, dirichlet), expression, hf.DELTA,
                                              greedy)
        print(f"\n{label}: {counts}")
        assert all(v > 0 for v in counts.values()), counts
        assert (off.n_pairs > 0) == (len(counts) == 2)

    mg = function_module(off, p, expression, p.sc_derivative_approximation_delta)
    mc = HyperbolicModule(off, p, backend=oracle.backend())
    mods = [(m, m.new_state_vector(U), m.new_state_vector()) for m in (mg, mc)]
    g, c = compare_step(off, mods, dirichlet, tau, oracle=oracle, params=p, label=label, row_slack=row_slack)
    print(f"{label}: " + " ".join(f"{k}={v:.2e}" for k, v in g["measured"].items()) + f" slack_used={g['slack_used']}")
    assert g["status"] == 0
    # the same operations in the same order: the precomputed values carry the same bits
    np.testing.assert_array_equal(g["prec"], c["prec"])
    info = mg.flux_info()
    assert info["kind"] == capi.FLUX_FUNCTION and info["n_instructions"] > 0
    assert info["step2_interpreted"] == (1 if averaged else 0)
    for m in (mg, mc):
        m.close()


# --------------------------------------------------------------------------- 3

def test_buckley_leverett_dij_against_the_restated_riemann_solver():
    """40 x 48 nodes, Buckley-Leverett in both directions (mobility ratios 0.25 and 0.5), averaged entropy: d_ij of the
    device against lambda_max / dij_from_states restated in numpy, fed the device's own U and precomputed values and
    f((u_i + u_j) / 2) of the host interpreter; rtol 1e-12, the bound of compare_step. Both arms of
    max(lambda, lambda_left, lambda_right) are taken."""
    off = hf.mesh("plane")
    expression, _ = hf.ARITHMETIC_SETS["buckley leverett"]
    p = scalar_params(2, averaged=True)
    p.sc_flux = capi.FLUX_FUNCTION
    m = HyperbolicModule(off, p, backend="hip")
    m.flux_configure_function(expression, hf.DELTA)
    U = np.clip(hf.extrema_next_to_the_boundary(off, (hf.smooth_state(off) - 0.5) / 2.0), -0.25, 1.25)
    b_i = np.asarray(off.b_i).astype(np.int64)
    old, new = m.new_state_vector(U), m.new_state_vector()
    m.prepare_state_vector(old, 0.0, U[b_i])
    m.step(old, [], [], new)
    assert m.last_status == 0 and m.flux_info()["step2_interpreted"] == 1
    n = off.n_owned
    U_old, prec, dij = old.download()[:n], old.download_precomputed()[:n], m.debug_fetch("dij")
    r = hf.upper_dij(off, U_old, prec, expression, hf.DELTA, False, True)
    got = dij[r["entries"]]
    rel = np.abs(got - r["d"]) / np.abs(r["d"])
    arms = dict(average=int(r["by_average"].sum()), other=int((~r["by_average"]).sum()),
                boundary_average=int((r["by_average"] & r["boundary"]).sum()))
    print(f"\nBuckley-Leverett d_ij: {len(got)} pairs, max relative difference {rel.max():.3e}, arms {arms}")
    np.testing.assert_allclose(got, r["d"], rtol=1e-12, atol=1e-300)
    assert all(v > 0 for v in arms.values()), arms
    # ... and the transposed entries carry the same numbers
    rows, cols, tr = hf.transposed_entries(off)
    np.testing.assert_array_equal(dij[tr[r["entries"]]], got)
    m.close()


# --------------------------------------------------------------------------- 4

def plane_wave(positions):
    """a function of the position alone: the same on every partition"""
    x = np.asarray(positions)
    return (1.5 + 0.9 * np.sin(2.0 * np.pi * x[:, 0]) * np.cos(2.0 * np.pi * x[:, 1] + 0.3)).reshape(-1, 1)


def twenty_steps(m, part, scheme):
    U0 = plane_wave(part.positions)
    dirichlet = U0[np.asarray(part.b_i).astype(np.int64)] if part.n_bdry else None
    state = m.new_state_vector(U0)
    temps = [m.new_state_vector() for _ in range(3)]
    states, taus = [], []
    for _ in range(20):
        taus.append(m.time_step(scheme, state, temps, dirichlet, cfl_min=0.5, cfl_max=0.5))
        states.append(state.download()[: part.n_owned])
    return states, taus


@pytest.mark.parametrize("scheme, fold", [("ssprk 33", True), ("erk 33", True), ("erk 33", False)])
def test_twenty_steps_equal_the_polynomial_flux_bit_for_bit(scheme, fold):
    """the Horner cubic as a function flux against the same coefficients as RYUJIN_FLUX_POLYNOMIAL, both on the device:
    Dirichlet boundaries (folded into the pre-pass, and as a launch of their own), stage vectors through the function
    pre-pass (ERK33), averaged entropy: every state and every tau identical"""
    off = hf.mesh("plane")
    expression, _ = hf.polynomial_flux(hf.CUBIC, 2)
    p = scalar_params(2, averaged=True)
    p.sc_flux = capi.FLUX_POLYNOMIAL
    for d in range(2):
        for n in range(4):
            p.sc_flux_polynomial[d][n] = hf.CUBIC[d][n]
    if not fold:
        p.debug_bc_fold_max_slices = -1
    m_fn = function_module(off, p, expression, p.sc_derivative_approximation_delta)
    m_poly = HyperbolicModule(off, p, backend="hip")
    (s_fn, t_fn), (s_poly, t_poly) = twenty_steps(m_fn, off, scheme), twenty_steps(m_poly, off, scheme)
    assert t_fn == t_poly and all(t > 0.0 for t in t_fn)
    for step, (a, b) in enumerate(zip(s_fn, s_poly)):
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b, err_msg=f"after step {step}")
    assert not np.array_equal(s_fn[0], s_fn[-1])
    assert m_fn.flux_info() == dict(kind=capi.FLUX_FUNCTION, n_instructions=30, step2_interpreted=1)
    assert m_poly.flux_info() == dict(kind=capi.FLUX_POLYNOMIAL, n_instructions=0, step2_interpreted=0)
    m_fn.close()
    m_poly.close()


def test_three_ranks_equal_the_polynomial_flux_bit_for_bit():
    """three ranks of the in-process transport, every rank's context configured by its own call: U and tau identical to
    the polynomial run on the same partition"""
    from helpers_partitioned import run_hip_ranks
    from ryujin_amd import offline
    parts = [offline.SyntheticOffline(offline.rectangle_2d(39, ny=47, bc=capi.BC_DIRICHLET, n_ranks=3, rank=r))
             for r in range(3)]
    expression, _ = hf.polynomial_flux(hf.CUBIC, 2)

    def params():
        p = scalar_params(2, averaged=True)
        p.sc_flux = capi.FLUX_POLYNOMIAL
        for d in range(2):
            for n in range(4):
                p.sc_flux_polynomial[d][n] = hf.CUBIC[d][n]
        return p

    def body(function):
        def run(m, part, rank):
            if function:
                m.flux_configure_function(expression, hf.DELTA)
            out = twenty_steps(m, part, "erk 33")
            assert m.flux_info()["step2_interpreted"] == (1 if function else 0)
            return out
        return run
    out_fn = run_hip_ranks(parts, params, body(True))
    out_poly = run_hip_ranks(parts, params, body(False))
    for rank in range(3):
        assert out_fn[rank][1] == out_poly[rank][1] == out_fn[0][1]
        for step in range(20):
            np.testing.assert_array_equal(out_fn[rank][0][step], out_poly[rank][0][step],
                                          err_msg=f"rank {rank} after step {step}")


# --------------------------------------------------------------------------- 5

@pytest.mark.parametrize("scheme", ["erk 33", "ssprk 22"])
def test_linear_transport_golden_with_the_flux_as_an_expression(golden_dir, scheme):
    """tests/scalar_conservation/verification-linear_transport-*.prm as its parameter file states it: flux "function"
    with the expression u, initial state sin(x-t) made on the device. The run, the norms and the tolerances of
    test_gpu_initial_values_function.test_linear_transport_golden_from_a_device_made_initial_state (one download at the
    end: the periodic mesh carries a constrained DoF that the device's error norms have no counterpart for)."""
    from ryujin_amd import TimeIntegrator
    from test_gpu_initial_values_function import scalar_params as transport_params
    from test_oracle_golden_scalar import _norms_1d, golden_linear_transport, periodic_interval
    dofs, t_ref, linf_ref, l1_ref, l2_ref = golden_linear_transport(golden_dir, scheme)
    n_cells = 2 ** 9
    off, h = periodic_interval(n_cells, 6.28318530718)
    p = transport_params(1)
    p.limiter_iterations = 2
    p.limiter_relaxation_factor = 1.0
    m = function_module(off, p, "u", 1e-10)
    m.initial_values_configure_function({"expression": "sin(x-t)"}, position=(1.0,), direction=(1.0,))
    sv = m.new_state_vector()
    m.initial_values_interpolate(sv, 0.0)
    cfl = {"erk 11": 0.05, "erk 22": 0.20}.get(scheme, 0.80)
    ti = TimeIntegrator(m, scheme, cfl_min=cfl, cfl_max=cfl, cfl_recovery_strategy="none")
    t = 0.0
    while t < 2.0:
        sv, tau = ti.step(sv, t)
        t += tau
    assert m.flux_info()["kind"] == capi.FLUX_FUNCTION
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


# --------------------------------------------------------------------------- 6

def test_buckley_leverett_riemann_problem_in_1d():
    """400 nodes, u = 1 | 0 with the jump at x = 1/4, averaged entropy, 200 forward Euler updates (t = 0.057, the front
    at x = 0.34; the left state has f'(1) = 0 and stays). Neither wave reaches a boundary -- asserted on the end state:
    the ten nodes next to either end hold the Riemann data to the roundings of their own updates, 8 eps per update (in
    the constant state 1 an update forms (1 + X) - X with X = tau f / m_i: 1 - 1e-15 after 200 of them, on the device
    as in the reference).
    Maximum principle: 0 <= u <= 1 within the limiter's own relaxation, 1 + 10000 eps. That is the relaxation of
    Limiter::limit; the limiter BOUNDS have a window of their own, limiter_relaxation_factor * (m_i / |Omega|)^(3/2) =
    1.25e-4 per update here, which admits an overshoot of that order by design (measured with the default factor 1:
    max u = 1 + 8.4e-4). The run therefore sets limiter_relaxation_factor = 0: the local bounds as they are.
    Mass balance: sum m_i u_i(t) - sum m_i u_i(0) = t (f(1) - f(0)) = t (the boundary nodes keep 1 and 0), within the
    forward bound of the updates' own roundings, 8 eps steps sum m_i |u_i| (the sums themselves are formed exactly,
    math.fsum)."""
    off = hf.mesh("line")
    p = scalar_params(1, averaged=True)
    p.sc_flux = capi.FLUX_FUNCTION
    p.limiter_relaxation_factor = 0.0
    m = HyperbolicModule(off, p, backend="hip")
    m.flux_configure_function(hf.BUCKLEY_LEVERETT, hf.DELTA)
    x = np.asarray(off.positions).reshape(-1)[: off.n_owned]
    U0 = np.where(x < 0.25, 1.0, 0.0).reshape(-1, 1)
    b_i = np.asarray(off.b_i).astype(np.int64)
    dirichlet = U0[b_i]
    a, b = m.new_state_vector(U0), m.new_state_vector()
    t, steps = 0.0, 200
    for _ in range(steps):
        m.prepare_state_vector(a, 0.0, dirichlet)
        t += m.step(a, [], [], b)
        assert m.last_status == 0
        a, b = b, a
    U = a.download()[: off.n_owned, 0]
    order = np.argsort(x)
    relax = 1.0 + 10000.0 * EPS
    front = x[order][np.flatnonzero(U[order] > 1e-3)[-1]]
    print(f"\nBuckley-Leverett 1-D: t = {t!r}, min u = {U.min()!r}, max u - 1 = {U.max() - 1.0!r}, front at x = {front!r}, "
          f"left end {U[order[:10]].tolist()}, right end {U[order[-10:]].tolist()}")
    untouched = 8.0 * EPS * steps
    assert (np.abs(U[order[:10]] - 1.0) <= untouched).all() and (np.abs(U[order[-10:]]) <= untouched).all()
    assert 0.25 < front < 0.75 and 0.03 < t < 0.2
    assert U.min() >= -10000.0 * EPS and U.max() <= relax
    mi = np.asarray(off.mi)[: off.n_owned]
    mass = math.fsum(mi * U) - math.fsum(mi * U0[:, 0])
    bound = 8.0 * EPS * steps * math.fsum(mi * np.abs(U))
    print(f"mass balance: {mass!r} - t = {mass - t!r}, bound {bound!r}")
    assert abs(mass - t) <= bound
    assert m.flux_info()["step2_interpreted"] == 1
    m.close()


# --------------------------------------------------------------------------- 7

def one_update(m, off, U):
    old, new = m.new_state_vector(U), m.new_state_vector()
    m.prepare_state_vector(old, 0.0, U[np.asarray(off.b_i).astype(np.int64)])
    m.step(old, [], [], new)
    out = new.download()[: off.n_owned].copy(), old.download_precomputed()[: off.n_owned].copy()
    old.free()
    new.free()
    return out


def test_refused_configure_leaves_the_flux_and_configure_replaces_it():
    lib = capi.load_hip()
    off = hf.mesh("plane")
    U = hf.smooth_state(off)
    p = scalar_params(2, averaged=True)   # created with "burgers"
    m = HyperbolicModule(off, p, backend="hip")
    burgers = one_update(m, off, U)
    assert m.flux_info() == dict(kind=capi.FLUX_BURGERS, n_instructions=0, step2_interpreted=0)
    for expression, delta, status, needle in (("u", hf.DELTA, capi.RYUJIN_ERR_ARG, b"component"),
                                              ("u; x", hf.DELTA, capi.RYUJIN_ERR_ARG, b"at character 3 "),
                                              ("u; rand()", hf.DELTA, capi.RYUJIN_ERR_UNSUPPORTED, b"at character 3 "),
                                              ("u; u", 0.0, capi.RYUJIN_ERR_ARG, b"delta"),
                                              ("u; u", float("nan"), capi.RYUJIN_ERR_ARG, b"delta")):
        assert lib.ryujin_hip_flux_configure_function(m._ctx, expression.encode(), delta) == status
        assert needle in lib.ryujin_hip_last_error(), lib.ryujin_hip_last_error()
        again = one_update(m, off, U)
        np.testing.assert_array_equal(again[0], burgers[0])
        np.testing.assert_array_equal(again[1], burgers[1])
    # configure after create with "burgers" switches the flux ...
    m.flux_configure_function("sin(u); cos(u)", hf.DELTA)
    kpp = one_update(m, off, U)
    assert m.flux_info() == dict(kind=capi.FLUX_FUNCTION, n_instructions=4, step2_interpreted=1)
    assert not np.array_equal(kpp[0], burgers[0])
    value, _ = capi.flux_function_evaluate("sin(u); cos(u)", 2, U[:, 0], hf.DELTA)
    assert (np.abs(kpp[1][:, :2] - value) <= hx.function_bound(value, 3.0)).all()
    # ... a refused one leaves THAT flux running, and a second one replaces the first
    assert lib.ryujin_hip_flux_configure_function(m._ctx, b"u; pi", hf.DELTA) == capi.RYUJIN_ERR_ARG
    again = one_update(m, off, U)
    np.testing.assert_array_equal(again[0], kpp[0])
    np.testing.assert_array_equal(again[1], kpp[1])
    m.flux_configure_function("0.5*u*u; 0.5*u*u", 1e4 * EPS)   # Burgers as an expression, with the built-in's delta
    replaced = one_update(m, off, U)
    np.testing.assert_array_equal(replaced[1][:, :2], burgers[1][:, :2])
    np.testing.assert_allclose(replaced[1][:, 2:], burgers[1][:, 2:], rtol=1e-3)   # (u against a difference quotient)
    assert not np.array_equal(replaced[0], kpp[0])
    m.close()


def test_created_with_the_function_flux_starts_from_the_default_expression():
    """RYUJIN_FLUX_FUNCTION at create: 0.5*u*u in every direction with sc_derivative_approximation_delta"""
    off = hf.mesh("plane")
    U = hf.smooth_state(off)
    p = scalar_params(2)
    p.sc_flux = capi.FLUX_FUNCTION
    p.sc_derivative_approximation_delta = 1e-7
    m = HyperbolicModule(off, p, backend="hip")
    assert m.flux_info() == dict(kind=capi.FLUX_FUNCTION, n_instructions=10, step2_interpreted=0)
    _, prec = one_update(m, off, U)
    value, gradient = capi.flux_function_evaluate("0.5*u*u; 0.5*u*u", 2, U[:, 0], 1e-7)
    np.testing.assert_array_equal(prec, np.concatenate([value, gradient], axis=1))
    m.close()
    p.sc_derivative_approximation_delta = 0.0
    with pytest.raises(RuntimeError, match="status -2"):
        HyperbolicModule(off, p, backend="hip")


def test_other_descriptions_and_the_discontinuous_ansatz_are_refused():
    import helpers_initial_values as hiv
    lib = capi.load_hip()
    off = hiv.tiny_mesh(2)
    m = HyperbolicModule(off, hiv.make_params(capi.EQ_EULER, 2), backend="hip")
    assert lib.ryujin_hip_flux_configure_function(m._ctx, b"u; u", 1e-10) == capi.RYUJIN_ERR_UNSUPPORTED
    kind = C.c_int(0)
    assert lib.ryujin_hip_flux_info(m._ctx, C.byref(kind), None, None) == capi.RYUJIN_ERR_UNSUPPORTED
    m.close()
    from helpers_dg import dg_q1_offline
    dg, _ = dg_q1_offline((8, 8), 1.0 / 8, boundary_id=capi.BC_DIRICHLET)
    p = scalar_params(2)
    p.sc_flux = capi.FLUX_FUNCTION
    with pytest.raises(RuntimeError, match="0/0"):
        HyperbolicModule(dg, p, backend="hip")
