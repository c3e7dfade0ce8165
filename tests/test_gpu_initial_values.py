"""Device-resident InitialValues (ryujin_hip_initial_values_*, ryujin_hip_prepare_state_vector_iv,
ryujin_hip_time_step_iv; ryujin_amd/csrc/initial_states_device.hpp, kernels_initial_values.hpp).

A  the device function against ryujin_amd.initial_states, with the tolerances DERIVED in tests/helpers_initial_values.py
B  one function, three consumers: evaluate, interpolate and the Dirichlet kernel give the same bits
C  the driver: ryujin_hip_time_step_iv against ryujin_hip_time_step_fn fed with initial_values_evaluate -- bit for bit
D  the reference's 1-D verification baselines, start to finish on the device, with the tolerances those cases have
and the argument errors. Every test fails on a library without the new entry points (the symbols are missing)."""
import ctypes as C

import numpy as np
import pytest

import helpers_initial_values as hiv
from helpers_initial_values import Case
from ryujin_amd import HyperbolicModule, capi, offline

pytestmark = pytest.mark.gpu

FUNCTION_CASES = hiv.function_cases()


# --------------------------------------------------------------------------- A

def _compare(case, m, X, t):
    got = m.initial_values_evaluate(X, t)
    ref = hiv.reference(case, X, t)
    _, tol = hiv.tolerance(case, X, t)
    err = np.abs(got - ref)
    excess = err - tol
    worst = np.unravel_index(int(np.argmax(excess)), excess.shape)
    scale = np.maximum(np.abs(ref).max(axis=0), 1e-300)
    print(f"{case.label} t={t:g}: max err / scale per component {(err.max(axis=0) / scale)}, "
          f"max tol / scale {(tol.max(axis=0) / scale)}; worst point {worst[0]} component {worst[1]}: "
          f"err {err[worst]:.3e} tol {tol[worst]:.3e} value {ref[worst]:.17g}")
    assert np.isfinite(got).all()
    assert (err <= tol).all(), (case.label, t, worst, float(err[worst]), float(tol[worst]))


@pytest.mark.parametrize("case", FUNCTION_CASES, ids=[c.label for c in FUNCTION_CASES])
def test_states_against_the_numpy_restatement(case):
    """evaluate() at 1000 points and three times (t = 0 and two positive ones) against ryujin_amd.initial_states
    composed with the affine transform; every point further than 1e-9 (1 + |x|) from every region boundary (asserted
    for all 1000, nothing left out); tolerance per point and component from the error arithmetic of the helper."""
    m = hiv.module_for(case)
    X = hiv.points_for(case)
    assert X.shape == (1000, case.dim)
    for t in case.times:
        hiv.assert_clear_of_jumps(case, X, t)
        _compare(case, m, X, t)
    m.close()


JUMP_CASES = [c for c in FUNCTION_CASES if c.name in hiv.JUMP_STATES]


@pytest.mark.parametrize("case", JUMP_CASES, ids=[c.label for c in JUMP_CASES])
def test_point_exactly_on_the_jump_takes_numpys_side(case):
    """a point exactly on `position` at t = 0 sits ON the jump of the tubes and the dam (x' = 0 exactly: the
    translation is exact, the rolls of a zero vector too): `<=` against `<` as the restatement writes them. Le Blanc's
    x / t must not reach the result."""
    m = hiv.module_for(case)
    X = np.array([case.pos(), case.pos()], dtype=np.float64)
    got = m.initial_values_evaluate(X, 0.0)
    ref = hiv.reference(case, X, 0.0)
    _, tol = hiv.tolerance(case, X, 0.0)
    assert np.isfinite(got).all()
    assert (np.abs(got - ref) <= tol).all(), (got, ref)
    if case.name == "leblanc":
        assert got[0, 0] == 1.0           # x <= -t / 3 at x = 0, t = 0: the left state
    if case.name == "rarefaction":
        assert got[0, 0] == 3.0           # x <= tt (u_l - c_l) = 0: the left state
    m.close()


# --------------------------------------------------------------------------- B

def _leblanc_nd(dim):
    return Case(f"leblanc {dim}d", capi.EQ_EULER, dim, "leblanc", {}, (1.0,) * dim, (0.25, -0.125, 0.0625)[:dim],
                edits=dict(gamma=5.0 / 3.0))


D, S, N = capi.BC_DIRICHLET, capi.BC_SLIP, capi.BC_DO_NOTHING
CONSUMER_MESHES = {
    # (mesh, state, number of boundary NODES; the boundary map holds one entry more per corner of the 2-D meshes)
    "1d 65 nodes": (lambda: hiv.interval(64, 0.0, 1.0, D, D), hiv.LEBLANC, 2),
    "2d 9x7": (lambda: hiv.vortex_mesh(9, 7), hiv.VORTEX, 32),                # fewer than a wave
    "2d 40x33": (lambda: hiv.vortex_mesh(40, 33), hiv.VORTEX, 146),            # several blocks, no multiple of 64
    "3d 5x4x3": (lambda: offline.SyntheticOffline(offline.MeshSpec(3, (5, 4, 3), (-1.0,) * 3, (1.0,) * 3, (D,) * 6)),
                 _leblanc_nd(3), 6 * 5 * 4 - (4 * 3 * 2)),
    "2d 9x7 dirichlet/slip/do nothing": (lambda: hiv.vortex_mesh(9, 7, bc=(D, S, N, D)), hiv.VORTEX, 32),
}


@pytest.mark.parametrize("mesh", sorted(CONSUMER_MESHES))
def test_three_consumers_give_the_same_bits(mesh):
    """interpolate + download == evaluate(positions), ghost-free single rank, every row; prepare_state_vector with
    dirichlet="device" leaves evaluate(b_positions) at the boundary rows of an all-Dirichlet mesh, and on every mesh
    -- the one with mixed ids included -- the same state as the host path fed with evaluate(b_positions): the
    permutation into the library's boundary order and the skipped entries."""
    make, case, n_bdry = CONSUMER_MESHES[mesh]
    off = make()
    assert len(set(off.b_i.tolist())) == n_bdry and off.n_bdry >= n_bdry
    if mesh == "2d 40x33":
        assert off.n_bdry > 2 * 64 and off.n_bdry % 64 != 0
    m = hiv.module_for(case, off)
    t = 0.3
    expected = m.initial_values_evaluate(off.positions, t)
    assert np.isfinite(expected).all() and np.abs(expected).max() > 0.0
    sv = m.new_state_vector(np.full((off.n_relevant, m.k), np.nan))
    m.initial_values_interpolate(sv, t)
    np.testing.assert_array_equal(sv.download(), expected)

    # the Dirichlet kernel: from a state that differs from the boundary data everywhere
    U0 = 1.5 * m.initial_values_evaluate(off.positions, 0.0)     # (admissible, and not the boundary data anywhere)
    boundary = m.initial_values_evaluate(off.b_positions, t)
    a, b = m.new_state_vector(U0), m.new_state_vector(U0)
    m.prepare_state_vector(a, t, "device")
    m.prepare_state_vector(b, t, boundary)
    A = a.download()
    np.testing.assert_array_equal(A, b.download())
    ids, rows = off.b_id, off.b_i
    if (ids == D).all():
        np.testing.assert_array_equal(A[rows], boundary)
        assert (U0[rows, 0] != boundary[:, 0]).all()
    else:
        assert {D, S, N} <= set(ids.tolist())
        only_dirichlet = [e for e in range(off.n_bdry) if (ids[rows == rows[e]] == D).all()]
        assert only_dirichlet
        np.testing.assert_array_equal(A[rows[only_dirichlet]], boundary[only_dirichlet])
    m.close()


# --------------------------------------------------------------------------- C

DRIVER_CASES = {
    "leblanc 1d erk33": (lambda: hiv.interval(400, 0.0, 1.0, D, D), hiv.LEBLANC, "erk 33", {}),
    "leblanc 1d ssprk33": (lambda: hiv.interval(400, 0.0, 1.0, D, D), hiv.LEBLANC, "ssprk 33", {}),
    "vortex 2d ssprk22": (lambda: hiv.vortex_mesh(32), hiv.VORTEX, "ssprk 22", {}),
    "vortex 2d erk43": (lambda: hiv.vortex_mesh(32), hiv.VORTEX, "erk 43", {}),
    "vortex 2d erk54": (lambda: hiv.vortex_mesh(32), hiv.VORTEX, "erk 54", {}),
    "vortex 2d erk33 bang bang": (lambda: hiv.vortex_mesh(32), hiv.VORTEX, "erk 33",
                                  dict(cfl_recovery="bang bang control", cfl_min=0.3, cfl_max=3.0)),
    "steady incline 1d erk33": (lambda: hiv.incline_mesh(200), hiv.INCLINE, "erk 33", {}),
    "aeos leblanc 1d erk33": (lambda: hiv.interval(400, 0.0, 1.0, D, D), hiv.AEOS_LEBLANC, "erk 33", {}),
}
N_STEPS = 20


@pytest.mark.parametrize("name", sorted(DRIVER_CASES))
def test_time_step_iv_equals_the_callback_path_bit_for_bit(name, oracle):
    """20 Runge-Kutta steps twice from the same uploaded state: ryujin_hip_time_step_iv, and ryujin_hip_time_step_fn
    whose callback returns initial_values_evaluate(b_positions, time) -- the same device function on the same doubles.
    States after every step and every tau identical: a wrong stage coefficient, a stage time formed with another
    rounding, a wrong boundary order or stale data of the previous stage would show. No library function's accuracy
    enters."""
    make, case, scheme, recovery = DRIVER_CASES[name]
    results = []
    for device in (True, False):
        off = make()
        m = hiv.module_for(case, off)
        if name.startswith("leblanc 1d erk33"):
            assert off.n_relevant == 401
        U0 = m.initial_values_evaluate(off.positions, 0.0)
        results.append(hiv.run_driver(m, case, U0, scheme, N_STEPS, device, **recovery))
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
        # ... and the CPU oracle restarts at this CFL as well (the choice is not an artefact of the device path)
        from ryujin_amd import TimeIntegrator
        off = make()
        mo = HyperbolicModule(off, oracle.default_params(case.equation, case.dim), backend=oracle.backend())
        bpos = off.b_positions
        ti = TimeIntegrator(mo, scheme, cfl_min=recovery["cfl_min"], cfl_max=recovery["cfl_max"],
                            cfl_recovery_strategy="bang bang control",
                            dirichlet_fn=lambda time: hiv.reference(case, bpos, time))
        sv, t = mo.new_state_vector(hiv.reference(case, off.positions, 0.0)), 0.0
        for _ in range(N_STEPS):
            sv, tau = ti.step(sv, t)
            t += tau
        assert mo.n_restarts() > 0


def test_time_step_iv_on_three_ranks_one_without_boundary():
    """The vortex on three in-process ranks (ryujin_hip_comm_init_local), every rank configured with its own
    positions. The mesh generator only cuts slabs, which all touch the boundary, so the partition comes from
    tests/helpers_unstructured.py: P1 elements on a disk of radius 5 (1027 nodes, the size of the 32 x 32 mesh), the
    outer ring Dirichlet, rank 1 the inner disk r < 2 -- it owns NO boundary entry (asserted) and launches nothing for
    the Dirichlet kernel -- ranks 0 and 2 the two halves of the rest. The gathered states after every step and every
    tau are identical to the three-rank callback run."""
    from helpers_partitioned import run_hip_ranks
    from helpers_unstructured import disk_points, p1_offline, partition
    points = 5.0 * disk_points(18)
    off, info = p1_offline(points, boundary_id=D)
    r = np.linalg.norm(points, axis=1)
    owner = np.where(r < 2.0, 1, np.where(points[:, 0] < 0.0, 0, 2))
    views = partition(off, info, owner)
    assert [v.n_bdry > 0 for v in views] == [True, False, True]
    assert all(v._o.n_nbr == 2 for v in views)
    case, scheme, n_steps = hiv.VORTEX, "erk 33", N_STEPS

    def body(device):
        def run(m, part, rank):
            hiv.configure(m, case)
            U0 = m.initial_values_evaluate(part.positions, 0.0)
            states, taus, _ = hiv.run_driver(m, case, U0, scheme, n_steps, device, b_positions=part.b_positions)
            return [s[: part.n_owned] for s in states], taus
        return run

    params = lambda: hiv.make_params(case.equation, case.dim, **case.edits)  # noqa: E731
    out_iv = run_hip_ranks(views, params, body(True))
    out_fn = run_hip_ranks(views, params, body(False))
    for rank in range(3):
        assert out_iv[rank][1] == out_fn[rank][1] == out_iv[0][1]
    for step in range(n_steps):
        gathered = []
        for out in (out_iv, out_fn):
            U = np.full((len(points), 4), np.nan)
            for rank, v in enumerate(views):
                U[v.global_ids[: v.n_owned]] = out[rank][0][step]
            gathered.append(U)
        assert np.isfinite(gathered[0]).all()
        np.testing.assert_array_equal(gathered[0], gathered[1], err_msg=f"after step {step}")


# --------------------------------------------------------------------------- D

@pytest.mark.parametrize("case", sorted(hiv.VERIFICATION))
def test_verification_baselines_start_to_finish_on_the_device(oracle, golden_dir, monkeypatch, case):
    """The reference's 1-D verification runs with initial_values_interpolate for the initial state and
    ryujin_hip_time_step_iv for every step: final time and error norms against the baselines under tests/golden/, with
    the set-up, norms (norms_1d), golden() and check() of tests/test_oracle_golden_verification.py and the slack of
    tests/test_gpu_parity.py -- imported, not copied. Wall times: profiles/initial_values_timing.md."""
    import test_oracle_golden_verification as tv
    from test_gpu_parity import VERIFICATION_SLACK
    run = hiv.run_verification_on_device(hiv.VERIFICATION[case])
    monkeypatch.setattr(tv, "run_verification", run)
    fn, args = tv.CASES[case]
    fn("hip-iv", oracle.default_params, golden_dir, *args, slack=VERIFICATION_SLACK.get(case, 1.0))
    print(f"{case}: {run.seconds:.2f} s wall")


# --------------------------------------------------------------------------- argument errors

def _status(m, fn, *args):
    return getattr(m._lib, "ryujin_hip_" + fn)(m._ctx, *args)


def test_argument_errors():
    lib = capi.load_hip()
    off = hiv.tiny_mesh(2)
    m = HyperbolicModule(off, hiv.make_params(capi.EQ_EULER, 2), backend="hip")
    sv = m.new_state_vector(np.ones((off.n_relevant, 4)))
    temps = [m.new_state_vector() for _ in range(3)]
    hs = (C.c_int * 3)(*[x.handle for x in temps])
    x, out, tau = np.zeros(2), np.zeros(4), C.c_double()
    px, pout = capi.as_ptr(x, capi.c_double_p), capi.as_ptr(out, capi.c_double_p)
    # every entry but configure before configure
    assert _status(m, "initial_values_evaluate", px, 1, 0.0, pout) == capi.RYUJIN_ERR_ARG
    assert _status(m, "initial_values_evaluate", None, 0, 0.0, None) == capi.RYUJIN_ERR_ARG
    assert _status(m, "initial_values_interpolate", sv.handle, 0.0) == capi.RYUJIN_ERR_ARG
    assert _status(m, "prepare_state_vector_iv", sv.handle, 0.0) == capi.RYUJIN_ERR_ARG
    assert _status(m, "time_step_iv", capi.SCHEME_ERK_33, sv.handle, 3, hs, 0.0, 1.0, 0, 0.2, 0.2,
                   C.byref(tau)) == capi.RYUJIN_ERR_ARG
    assert b"configure" in lib.ryujin_hip_last_error()

    pos = np.ascontiguousarray(off.positions).reshape(-1)
    bpos = np.ascontiguousarray(off.b_positions).reshape(-1)

    def configure(iv, module=m, positions=pos, b_positions=bpos):
        return _status(module, "initial_values_configure", C.byref(iv), capi.as_ptr(positions, capi.c_double_p),
                       capi.as_ptr(b_positions, capi.c_double_p))

    good = capi.initial_values_struct("uniform", 2)
    unknown = capi.initial_values_struct("uniform", 2)
    unknown.state = 99
    assert configure(unknown) == capi.RYUJIN_ERR_ARG
    with pytest.raises(ValueError):
        m.initial_values_configure("no such state")
    # a state of another Description
    assert configure(capi.initial_values_struct("ritter dam break", 2)) == capi.RYUJIN_ERR_ARG
    # a zero direction
    assert configure(capi.initial_values_struct("uniform", 2, direction=(0.0, 0.0))) == capi.RYUJIN_ERR_ARG
    # a non-zero perturbation
    assert configure(capi.initial_values_struct("uniform", 2, perturbation=1e-3)) == capi.RYUJIN_ERR_UNSUPPORTED
    # missing positions
    assert _status(m, "initial_values_configure", C.byref(good), None, None) == capi.RYUJIN_ERR_ARG
    # nothing of this configured the context
    assert _status(m, "initial_values_evaluate", px, 1, 0.0, pout) == capi.RYUJIN_ERR_ARG
    # a state in a dimension it is not defined for
    m1 = HyperbolicModule(hiv.tiny_mesh(1), hiv.make_params(capi.EQ_EULER, 1), backend="hip")
    p1 = np.ascontiguousarray(m1.offline.positions).reshape(-1)
    b1 = np.ascontiguousarray(m1.offline.b_positions).reshape(-1)
    assert configure(capi.initial_values_struct("isentropic vortex", 1), m1, p1, b1) == capi.RYUJIN_ERR_UNSUPPORTED
    msw = HyperbolicModule(off, hiv.make_params(capi.EQ_SHALLOW_WATER, 2), backend="hip")
    assert configure(capi.initial_values_struct("paraboloid", 2), msw) == capi.RYUJIN_ERR_UNSUPPORTED
    # scalar conservation
    msc = HyperbolicModule(off, hiv.make_params(capi.EQ_SCALAR_CONSERVATION, 2), backend="hip")
    assert configure(good, msc) == capi.RYUJIN_ERR_UNSUPPORTED

    # configured: n = 0 is fine and writes nothing; a second configure replaces the first
    assert configure(good) == capi.RYUJIN_OK
    guard = np.full(4, 7.0)
    assert _status(m, "initial_values_evaluate", None, 0, 0.0, capi.as_ptr(guard, capi.c_double_p)) == capi.RYUJIN_OK
    assert (guard == 7.0).all()
    assert _status(m, "initial_values_evaluate", None, 1, 0.0, pout) == capi.RYUJIN_ERR_ARG
    first = m.initial_values_evaluate(off.positions, 0.0)
    m.initial_values_configure("uniform", primitive_state=(2.0, 1.0, 3.0))
    second = m.initial_values_evaluate(off.positions, 0.0)
    assert (first[:, 0] == 1.4).all() and (second[:, 0] == 2.0).all()
    assert _status(m, "initial_values_interpolate", 12345, 0.0) == capi.RYUJIN_ERR_ARG
    for module in (m, m1, msw, msc):
        module.close()
