"""The Riemann-data, shock-front, ramp-up and Noh states on the device (capi.IV_LIBRARY_STATES;
ryujin_amd/csrc/initial_states_library_device.hpp, kernels_initial_values.hpp).

A  the device function against ryujin_amd.initial_states, tolerances DERIVED in tests/helpers_initial_values_library.py
B  three consumers, one function: evaluate at the nodes, interpolate and the Dirichlet kernel give the same bits
C  the driver: time_step_iv against time_step_fn fed with initial_values_evaluate -- bit for bit
D  the reference's smooth-wave and shock-front verification setups, start to finish on the device
E  refusals, and what a refused or a later configure leaves behind
F  contrast and ramp up on a function-EOS context (NASG as expressions) against the closed-form NASG context
Every test fails at its first configure on a library without these states (ValueError or status -2)."""
import ctypes as C

import numpy as np
import pytest

import helpers_eos_function as he
import helpers_initial_values as hiv
import helpers_initial_values_library as hl
from helpers_initial_values_library import Case
from ryujin_amd import HyperbolicModule, capi, error_norms
from ryujin_amd.module import StateVector

pytestmark = pytest.mark.gpu

CASES = hl.function_cases()
D = capi.BC_DIRICHLET


# --------------------------------------------------------------------------- A

@pytest.mark.parametrize("case", CASES, ids=[c.label for c in CASES])
def test_states_against_the_numpy_restatement(case):
    """evaluate() at 1000 points and three times against ryujin_amd.initial_states behind the affine transform; every
    one of the points clear of every region boundary (asserted, nothing dropped); tolerance per point and component
    from the error arithmetic of the helper"""
    m = hl.module_for(case)
    X = hl.points_for(case)
    assert X.shape == (1000, case.dim)
    for t in case.times:
        hl.assert_clear_of_jumps(case, X, t)
        got = m.initial_values_evaluate(X, t)
        ref = hl.reference(case, X, t)
        _, tol = hl.tolerance(case, X, t)
        err = np.abs(got - ref)
        worst = np.unravel_index(int(np.argmax(err - tol)), err.shape)
        scale = np.maximum(np.abs(ref).max(axis=0), 1e-300)
        print(f"{case.label} t={t:g}: max err / scale {err.max(axis=0) / scale}, max tol / scale "
              f"{tol.max(axis=0) / scale}; worst point {worst[0]} component {worst[1]}: err {err[worst]:.3e} "
              f"tol {tol[worst]:.3e} value {ref[worst]:.17g}")
        assert np.isfinite(got).all()
        assert (err <= tol).all(), (case.label, t, worst, float(err[worst]), float(tol[worst]))
    m.close()


# --------------------------------------------------------------------------- B

CONSUMER_CASES = [c for c in CASES if c.label.startswith(("euler ", "aeos-fn ", "sw ", "aeos-nasg ramp up",
                                                          "aeos-nasg noh"))]


@pytest.mark.parametrize("case", CONSUMER_CASES, ids=[c.label for c in CONSUMER_CASES])
def test_three_consumers_give_the_same_bits(case):
    """on the smallest mesh of the dimension, all ends Dirichlet: interpolate + download == evaluate(positions);
    prepare_state_vector with dirichlet="device" leaves evaluate(b_positions) in the boundary rows and the same state
    as the host path fed with it"""
    off = hiv.tiny_mesh(case.dim)
    m = hl.module_for(case, off)
    for t in case.times[1:]:
        expected = m.initial_values_evaluate(off.positions, t)
        assert np.isfinite(expected).all() and np.abs(expected).max() > 0.0
        sv = m.new_state_vector(np.full((off.n_relevant, m.k), np.nan))
        m.initial_values_interpolate(sv, t)
        np.testing.assert_array_equal(sv.download(), expected)
        U0 = 1.5 * m.initial_values_evaluate(off.positions, 0.0)     # admissible, and not the boundary data
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
    m.close()


# --------------------------------------------------------------------------- C

N_STEPS = 20
SW_EDITS = dict(gravity=9.81, reference_water_depth=1.0, dry_state_relaxation_factor=0.2, dry_state_relaxation_small=1e4,
                dry_state_relaxation_large=1e4, cfl=0.5)
RAMP = {"primitive state initial": (1.4, 0.5, 1.0), "primitive state final": (1.4, 3.0, 1.0)}


def _driver_case(name):
    """(mesh factory, case, scheme) of a driver run"""
    interval = lambda bc=D: hiv.interval(200, 0.0, 1.0, bc, bc)  # noqa: E731
    if name.startswith("shock front"):
        # S3 = 2 and tau = 1.5e-4 .. 2e-4 (cfl 0.1, h = 1/200): the front moves by 0.007 in 20 steps. From 0.25 it
        # meets no boundary; from 0.998 the node x = 1 changes sides at t = 1e-3, within the run (asserted)
        position = (0.25,) if name.endswith("interior") else (0.998,)
        return interval, Case(name, capi.EQ_EULER, 1, "shock front", {}, None, position,
                              edits=dict(cfl=0.1, limiter_relaxation_factor=8.0)), "erk 33"
    if name == "noh 2d":
        return (lambda: hiv.vortex_mesh(16)), Case(name, capi.EQ_EULER, 2, "noh", {"reference pressure": 1.0e-6},
                                                   edits=dict(cfl=0.2)), "erk 33"
    if name == "aeos nasg contrast ssprk33":
        return interval, Case(name, capi.EQ_EULER_AEOS, 1, "contrast",
                              {"primitive state left": (1.0, 0.0, 1.0), "primitive state right": (0.125, 0.0, 0.1)},
                              None, (0.5,), edits=dict(hiv.NASG, cfl=0.1)), "ssprk 33"
    if name == "sw contrast dynamic ends":
        return (lambda: interval(capi.BC_DYNAMIC)), Case(
            name, capi.EQ_SHALLOW_WATER, 1, "contrast",
            {"primitive state left": (2.0, 0.5), "primitive state right": (1.0, 0.25)}, None, (0.5,),
            edits=SW_EDITS), "erk 33"
    raise KeyError(name)


def _run_both(make, case, scheme):
    results = []
    for device in (True, False):
        off = make()
        m = hl.module_for(case, off)
        U0 = m.initial_values_evaluate(off.positions, 0.0)
        results.append(hiv.run_driver(m, case, U0, scheme, N_STEPS, device))
        m.close()
    (states_iv, taus_iv, restarts_iv), (states_fn, taus_fn, restarts_fn) = results
    assert taus_iv == taus_fn, (taus_iv, taus_fn)
    assert all(tau > 0.0 for tau in taus_iv)
    for step, (a, b) in enumerate(zip(states_iv, states_fn)):
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b, err_msg=f"{case.label}: after step {step}")
    assert not np.array_equal(states_iv[0], states_iv[-1])
    assert restarts_iv == restarts_fn
    return states_iv, taus_iv


@pytest.mark.parametrize("name", ["shock front interior", "shock front leaves through the right end", "noh 2d",
                                  "aeos nasg contrast ssprk33", "sw contrast dynamic ends"])
def test_time_step_iv_equals_the_callback_path_bit_for_bit(name):
    """20 Runge-Kutta steps twice from the same uploaded state: ryujin_hip_time_step_iv, and ryujin_hip_time_step_fn
    whose callback returns initial_values_evaluate(b_positions, time). States after every step and every tau equal."""
    make, case, scheme = _driver_case(name)
    states, taus = _run_both(make, case, scheme)
    if name.startswith("shock front"):
        # the row of x = 1: next to the pre-shock density until the front has passed, the post-shock one after
        off = make()
        right = int(np.argmax(off.positions[:, 0]))
        t_exit = (1.0 - case.pos()[0]) / 2.0
        t_end = float(np.sum(taus))
        print(f"{name}: t_end {t_end:.3e}, the front reaches x = 1 at {t_exit:.3e}")
        if name.endswith("interior"):
            assert t_end < t_exit and all(s[right, 0] == 1.4 for s in states)
        else:
            assert taus[0] < t_exit < t_end
            assert states[0][right, 0] < 2.0 and states[-1][right, 0] > 3.0


def test_ramp_up_inflow_with_stage_times_before_inside_and_after_the_ramp():
    """ramp up on the 32 x 32 Dirichlet box of the vortex tests. The ramp is placed from the first step's tau0 of
    the same mesh and initial state (time initial = 1.5 tau0, time final = 5.5 tau0; tau only shrinks as the inflow
    accelerates), so that the 60 stage times of 20 ERK33 steps fall before, inside and after it -- asserted."""
    def case_with(t_initial, t_final):
        return Case("ramp up inflow", capi.EQ_EULER, 2, "ramp up",
                    dict(RAMP, **{"time initial": t_initial, "time final": t_final}), edits=dict(cfl=0.2))

    probe = case_with(1.0e9, 2.0e9)
    m = hl.module_for(probe, hiv.vortex_mesh(32))
    _, (tau0,), _ = hiv.run_driver(m, probe, m.initial_values_evaluate(m.offline.positions, 0.0), "erk 33", 1, True)
    m.close()
    t_initial, t_final = 1.5 * tau0, 5.5 * tau0
    case = case_with(t_initial, t_final)
    states, taus = _run_both(lambda: hiv.vortex_mesh(32), case, "erk 33")
    starts = np.concatenate([[0.0], np.cumsum(taus)[:-1]])
    stage_times = np.concatenate([starts + s * np.asarray(taus) for s in range(3)])
    print(f"tau0 {tau0:.4e}, ramp [{t_initial:.4e}, {t_final:.4e}], stage times {stage_times.min():.4e} .. "
          f"{stage_times.max():.4e}")
    assert (stage_times <= t_initial).sum() >= 2
    assert ((stage_times > t_initial) & (stage_times < t_final)).sum() >= 3
    assert (stage_times >= t_final).sum() >= 3
    # the boundary rows follow the ramp: the inflow momentum grows from 1.4 * 0.5 towards 1.4 * 3
    rows = np.asarray(hiv.vortex_mesh(32).b_i)
    assert states[0][rows, 1].max() < 1.0 and states[-1][rows, 1].max() > 4.0


def test_noh_on_three_ranks_one_without_boundary():
    """noh on three in-process ranks, every rank configured with its own positions: P1 elements on a disk of radius
    5, the outer ring Dirichlet, rank 1 the inner disk r < 2, which owns NO boundary entry (asserted) and launches
    nothing for the Dirichlet kernel. The gathered states after every step and every tau equal the callback run's."""
    from helpers_partitioned import run_hip_ranks
    from helpers_unstructured import disk_points, p1_offline, partition
    points = 5.0 * disk_points(18)
    off, info = p1_offline(points, boundary_id=D)
    r = np.linalg.norm(points, axis=1)
    owner = np.where(r < 2.0, 1, np.where(points[:, 0] < 0.0, 0, 2))
    views = partition(off, info, owner)
    assert [v.n_bdry > 0 for v in views] == [True, False, True]
    case = Case("noh 3 ranks", capi.EQ_EULER, 2, "noh", {"reference pressure": 1.0e-6}, position=(0.3, -0.2),
                edits=dict(cfl=0.2))

    def body(device):
        def run(m, part, rank):
            hiv.configure(m, case)
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
            U = np.full((len(points), 4), np.nan)
            for rank, v in enumerate(views):
                U[v.global_ids[: v.n_owned]] = out[rank][0][step]
            gathered.append(U)
        assert np.isfinite(gathered[0]).all()
        np.testing.assert_array_equal(gathered[0], gathered[1], err_msg=f"after step {step}")


# --------------------------------------------------------------------------- D

@pytest.mark.parametrize("name", sorted(hl.VERIFICATION))
def test_verification_setups_start_to_finish_on_the_device(oracle, golden_dir, monkeypatch, name):
    """prm/verification/euler-{smooth_wave,shock_front}-erk33.prm at 401 DoFs: initial_values_interpolate ->
    DeviceResidentTimeIntegrator(dirichlet="device") -> compute_error, the state never downloaded; against the
    reference's recorded results with the tolerances of the CPU test. The difference to the oracle's run of the same
    setup is printed, not asserted."""
    import test_oracle_golden_verification as tv
    from ryujin_amd.module import DeviceResidentTimeIntegrator
    gold, state, kwargs, cfl, relaxation, t_final = hl.VERIFICATION[name]
    res_oracle = tv.run_verification(oracle.backend(), hl.verification_mesh(), hl.verification_params(
        oracle.default_params, relaxation), hl.verification_exact(name), (0, 1, 2), cfl=cfl, t_final=t_final)

    def refuse(self):
        raise AssertionError("the state is never downloaded in this run")
    monkeypatch.setattr(StateVector, "download", refuse)
    off = hl.verification_mesh()
    m = HyperbolicModule(off, hl.verification_params(oracle.default_params, relaxation), backend="hip")
    m.initial_values_configure(state, **kwargs)
    shape, weights = error_norms.q1_tables(1)
    m.error_norms_configure(off.cells, shape, np.full(off.n_cells, off.cell_measure), weights)
    sv = m.new_state_vector()
    m.initial_values_interpolate(sv, 0.0)
    ti = DeviceResidentTimeIntegrator(m, "erk 33", cfl_min=cfl, cfl_max=cfl, cfl_recovery_strategy="none",
                                      dirichlet="device")
    t, n_steps = 0.0, 0
    while t < t_final:
        sv, tau = ti.step(sv, t)
        t += tau
        n_steps += 1
    (linf, l1, l2), _ = m.compute_error(sv, t)
    res = dict(t=t, linf=linf, l1=l1, l2=l2, dofs=off.n_owned)
    g = tv.golden(golden_dir, gold)
    rel = lambda a, b: abs(a - b) / abs(b)  # noqa: E731
    print(f"{name}: {n_steps} steps, t {t!r} Linf {linf!r} L1 {l1!r} L2 {l2!r}")
    print(f"{name}: relative to the baseline "
          f"{[rel(res[k], b) for k, b in zip(('t', 'linf', 'l1', 'l2'), g[1:])]}")
    print(f"{name}: relative to the oracle {[rel(res[k], res_oracle[k]) for k in ('t', 'linf', 'l1', 'l2')]}")
    print(f"{name}: steps of the oracle {res_oracle['n_steps']}")
    tv.check(res, g, **hl.VERIFICATION_TOL)
    m.close()


# --------------------------------------------------------------------------- E

def _configure_status(module, iv):
    off = module.offline
    pos = np.ascontiguousarray(off.positions).reshape(-1)
    bpos = np.ascontiguousarray(off.b_positions).reshape(-1)
    return module._lib.ryujin_hip_initial_values_configure(
        module._ctx, C.byref(iv), capi.as_ptr(pos, capi.c_double_p), capi.as_ptr(bpos, capi.c_double_p))


def test_refusals_leave_the_previous_configuration_in_place():
    euler_names = [n for f, n in capi.IV_LIBRARY_STATES if f == "euler"]
    sw_names = [n for f, n in capi.IV_LIBRARY_STATES if f == "shallow water"]
    assert sorted(euler_names) == sorted(hl.EULER_STATES) and sorted(sw_names) == sorted(hl.SW_STATES)
    off2, off1 = hiv.tiny_mesh(2), hiv.tiny_mesh(1)
    X2, X1 = hiv.points_for(Case("", capi.EQ_EULER, 2, "contrast"), 100), np.linspace(-1.0, 1.0, 100)[:, None]

    def refused(module, iv, status, X, before):
        assert _configure_status(module, iv) == status
        np.testing.assert_array_equal(module.initial_values_evaluate(X, 0.25), before)

    # a shallow-water context: every new Euler state is a state of another Description
    msw = HyperbolicModule(off2, hiv.make_params(capi.EQ_SHALLOW_WATER, 2, gravity=9.81), backend="hip")
    msw.initial_values_configure("contrast", primitive_state_left=(2.0, 0.5), primitive_state_right=(0.5, -0.25))
    before = msw.initial_values_evaluate(X2, 0.25)
    assert set(before[:, 0].tolist()) == {2.0, 0.5}
    for name in euler_names:
        refused(msw, capi.initial_values_struct(name, 2, equation=capi.EQ_EULER), capi.RYUJIN_ERR_ARG, X2, before)
    # ... and the reverse, for Euler and EulerAEOS
    for eq in (capi.EQ_EULER, capi.EQ_EULER_AEOS):
        m = HyperbolicModule(off2, hiv.make_params(eq, 2), backend="hip")
        m.initial_values_configure("ramp up", time_initial=0.125, time_final=0.5)
        before = m.initial_values_evaluate(X2, 0.25)
        for name in sw_names:
            refused(m, capi.initial_values_struct(name, 2, equation=capi.EQ_SHALLOW_WATER), capi.RYUJIN_ERR_ARG, X2,
                    before)
        # state 10 is the library's own id of the function state, 99 is unknown
        for state in (10, 99):
            iv = capi.initial_values_struct("contrast", 2, equation=eq)
            iv.state = state
            refused(m, iv, capi.RYUJIN_ERR_ARG, X2, before)
        # perturbation != 0
        refused(m, capi.initial_values_struct("noh", 2, equation=eq, perturbation=1e-3), capi.RYUJIN_ERR_UNSUPPORTED,
                X2, before)
        m.close()
    # four state contrast and astro jet have no 1-D form
    m1 = HyperbolicModule(off1, hiv.make_params(capi.EQ_EULER, 1), backend="hip")
    m1.initial_values_configure("shock front", position=(0.1,))
    before = m1.initial_values_evaluate(X1, 0.25)
    assert len(set(before[:, 0].tolist())) == 2
    for name in ("four state contrast", "astro jet"):
        refused(m1, capi.initial_values_struct(name, 1, equation=capi.EQ_EULER), capi.RYUJIN_ERR_UNSUPPORTED, X1,
                before)
    m1.close()
    # a scalar context refuses every analytic state, the new ones included, and keeps its function state
    msc = HyperbolicModule(off2, hiv.make_params(capi.EQ_SCALAR_CONSERVATION, 2), backend="hip")
    msc.initial_values_configure_function(["x + 2*y"])
    before = msc.initial_values_evaluate(X2, 0.25)
    for family, name in capi.IV_LIBRARY_STATES:
        eq = capi.EQ_EULER if family == "euler" else capi.EQ_SHALLOW_WATER
        refused(msc, capi.initial_values_struct(name, 2, equation=eq), capi.RYUJIN_ERR_UNSUPPORTED, X2, before)
    with pytest.raises(RuntimeError, match="status -5"):
        msc.initial_values_configure("noh")
    msc.close()
    msw.close()


def test_configures_replace_each_other():
    off = hiv.tiny_mesh(2)
    m = HyperbolicModule(off, hiv.make_params(capi.EQ_EULER, 2), backend="hip")
    X = hiv.points_for(Case("", capi.EQ_EULER, 2, "contrast"), 100)
    m.initial_values_configure("uniform", primitive_state=(1.0, 2.0, 3.0))
    old = m.initial_values_evaluate(X, 0.25)
    m.initial_values_configure("contrast", primitive_state_left=(2.0, 0.5, 1.0), primitive_state_right=(0.5, 0.0, 0.25))
    new = m.initial_values_evaluate(X, 0.25)
    assert set(new[:, 0].tolist()) == {2.0, 0.5} and (old[:, 0] == 1.0).all()
    m.initial_values_configure("uniform", primitive_state=(1.0, 2.0, 3.0))
    np.testing.assert_array_equal(m.initial_values_evaluate(X, 0.25), old)
    # a new state and the function state
    m.initial_values_configure("contrast", primitive_state_left=(2.0, 0.5, 1.0), primitive_state_right=(0.5, 0.0, 0.25))
    m.initial_values_configure_function(["1 + x*x", "y", "t", "2 + x"])
    function = m.initial_values_evaluate(X, 0.25)
    np.testing.assert_array_equal(function[:, 0], 1.0 + X[:, 0] * X[:, 0])
    m.initial_values_configure("contrast", primitive_state_left=(2.0, 0.5, 1.0), primitive_state_right=(0.5, 0.0, 0.25))
    np.testing.assert_array_equal(m.initial_values_evaluate(X, 0.25), new)
    m.initial_values_configure_function(["1 + x*x", "y", "t", "2 + x"])
    np.testing.assert_array_equal(m.initial_values_evaluate(X, 0.25), function)
    # ... and after all of it output_extract-free consumers still run: interpolate and the Dirichlet kernel
    m.initial_values_configure("noh")
    sv = m.new_state_vector()
    m.initial_values_interpolate(sv, 0.25)
    np.testing.assert_array_equal(sv.download(), m.initial_values_evaluate(off.positions, 0.25))
    m.close()


# --------------------------------------------------------------------------- F

FUNCTION_EOS_CASES = [
    Case("contrast 1d", capi.EQ_EULER_AEOS, 1, "contrast", dict(hl.PARAMS["contrast"]), None, (0.5,), edits=hiv.NASG,
         box=(0.0, 1.0)),
    Case("ramp up 2d (1,1)", capi.EQ_EULER_AEOS, 2, "ramp up", dict(hl.PARAMS["ramp up"]), (1.0, 1.0), (0.25, -0.125),
         edits=hiv.NASG, times=hl.TIMES["ramp up"]),
]


@pytest.mark.parametrize("order", ["eos-first", "state-first"])
@pytest.mark.parametrize("case", FUNCTION_EOS_CASES, ids=[c.label for c in FUNCTION_EOS_CASES])
def test_function_eos_context_equals_the_closed_form_context_bit_for_bit(case, order):
    """NASG as expressions against the closed-form NASG kernels: evaluate at 1000 points (no multiple of the block),
    interpolate and the Dirichlet kernel give the same bits, in both orders of initial_values_configure and
    eos_configure_function"""
    off = hiv.tiny_mesh(case.dim)
    p = hiv.make_params(case.equation, case.dim, **case.edits)
    m_closed = HyperbolicModule(off, p, backend="hip")
    hiv.configure(m_closed, case)
    m_fn = HyperbolicModule(off, p, backend="hip")
    if order == "eos-first":
        m_fn.eos_configure_function(**he.member_expressions(p))
        hiv.configure(m_fn, case)
    else:
        hiv.configure(m_fn, case)
        m_fn.eos_configure_function(**he.member_expressions(p))
    X = hiv.points_for(case)
    for t in case.times:
        want = m_closed.initial_values_evaluate(X, t)
        assert np.isfinite(want).all()
        np.testing.assert_array_equal(m_fn.initial_values_evaluate(X, t), want)
        a, b = m_fn.new_state_vector(), m_closed.new_state_vector()
        m_fn.initial_values_interpolate(a, t)
        m_closed.initial_values_interpolate(b, t)
        nodes = a.download()
        np.testing.assert_array_equal(nodes, b.download())
        np.testing.assert_array_equal(nodes, m_fn.initial_values_evaluate(off.positions, t))
        m_fn.prepare_state_vector(a, t, "device")
        m_closed.prepare_state_vector(b, t, "device")
        np.testing.assert_array_equal(a.download(), b.download())
        a.free()
        b.free()
    m_fn.close()
    m_closed.close()
