"""Device-resident Quantities (ryujin_hip_quantities_*) against the numpy restatement of tests/helpers_quantities.py and
the reference's own tests/golden/euler_check-mass-conservation_01.output. Tolerances are the derived ones stated in
the helper: FUNCTION_LEVEL |V_c| per point (2 FUNCTION_LEVEL V_c^2 for a second moment), (FUNCTION_LEVEL + D eps) S_c
for a mean (D from the library's launch shape), (FUNCTION_LEVEL + 2 N eps) max |x_c| for a time-averaged value."""
import ctypes as C

import numpy as np
import pytest

import helpers_quantities as hq
from helpers_partitioned import run_hip_ranks
from ryujin_amd import HyperbolicModule, StateVector, TimeIntegrator, capi, offline, quantities
from ryujin_amd.initial_states import euler_radial_contrast, euler_uniform, sw_circular_dam_break

pytestmark = pytest.mark.gpu

I, T, S = capi.Q_INSTANTANEOUS, capi.Q_TIME_AVERAGED, capi.Q_SPACE_AVERAGED
ALL_OPTIONS = [I, T, S, I | T, I | S, T | S, I | T | S]
TIMES = (0.25, 0.3125, 0.5, 0.53125, 1.0, 1.75, 1.875)  # irregular, exactly representable


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


def _developed_states(m, U0, dirichlet, n_first, n_states):
    """host copies of n_states states of a run: n_first updates, then one more update between two of them"""
    a, b = m.new_state_vector(U0), m.new_state_vector()
    out = []
    for k in range(n_first + n_states - 1):
        m.prepare_state_vector(a, 0.0, dirichlet)
        m.step(a, [], [], b)
        a, b = b, a
        if k >= n_first - 1:
            out.append(a.download())
    a.free()
    b.free()
    return out


def _line_level_set(off):
    """an interior line-out on a mesh line: the line along x through an interior node (1-D: that node)"""
    pos = off.positions[: off.n_owned]
    centre = pos[np.abs(pos - pos.mean(axis=0)).sum(axis=1).argmin()].copy()
    if off.dim == 1:
        return lambda x: x[:, 0] - centre[0]
    return lambda x: np.abs(x[:, 1:] - centre[1:]).sum(axis=1)


def _manifolds(off):
    """(label, index, weight): the full interior (one contiguous run), a line-out, the whole boundary map weighted by
    the boundary mass (a corner node once per face)"""
    lengths = np.diff(off.row_starts.astype(np.int64))
    full = quantities.select_interior_points(0.0, off.positions, lengths, off.n_owned)
    line = quantities.select_interior_points(_line_level_set(off), off.positions, lengths, off.n_owned)
    assert 1 <= len(line) < len(full)
    e = quantities.select_boundary_entries(0.0, off.b_i, off.b_positions, off.n_owned)
    assert len(e) == off.n_bdry > 0
    if off.dim > 1:
        assert len(set(off.b_i[e].tolist())) < len(e)  # repeated indices
    return [("interior", full, off.mi[full]), ("line", line, off.mi[line]), ("boundary", off.b_i[e], off.b_mass[e])]


def _compare_points(label, got, expected, tol):
    err = np.abs(got - expected)
    print(f"{label}: max err {err.max() if err.size else 0.0:.3e}, max err / tol "
          f"{(err / np.maximum(tol, 1e-300)).max() if err.size else 0.0:.3e}")
    assert np.isfinite(got).all() and (err <= tol).all(), label


def _compare_series(label, got, stats, D):
    expected = stats.series_array()
    assert got.shape == expected.shape, (label, got.shape, expected.shape)
    assert np.array_equal(got[:, 0], expected[:, 0]), label  # the time column is handed through
    for r, row in enumerate(stats.series_values):
        tol = hq.mean_tolerance(stats.weight, row, D)
        err = np.abs(got[r, 1:] - expected[r, 1:])
        print(f"{label} row {r}: max err / tol {(err / np.maximum(tol, 1e-300)).max():.3e} (D = {D})")
        assert (err <= tol).all(), (label, r, err, tol)


class _Stats(hq.Statistics):
    """keeps the point values of every accumulate (the mean tolerance is formed from them)"""

    def clear(self):
        super().clear()
        self.series_values = []

    def accumulate(self, U, t):
        super().accumulate(U, t)
        self.series_values.append(self.val_new.copy())


def _run_case(label, off, m, U_list, times=TIMES):
    """every option combination on the three manifolds, >= 6 accumulations at irregular t: instantaneous after
    every call, the time average with its interval and the series at the end, point by point"""
    assert len(U_list) >= 6 and len(U_list) == len(times)
    state = m.new_state_vector()
    manifolds = _manifolds(off)
    for options in ALL_OPTIONS:
        m.quantities_reset()
        ids = [m.quantities_add_manifold(index, weight, options) for _, index, weight in manifolds]
        stats = [_Stats(m.equation, off.dim, m.params, index, weight) for _, index, weight in manifolds]
        averaged = bool(options & (T | S))
        for U, t in zip(U_list, times):
            state.upload(U)
            m.quantities_accumulate(state, t)
            for (name, _, _), mid, st in zip(manifolds, ids, stats):
                if averaged:
                    st.accumulate(U, t)
                if options & I:
                    values = st.values(U)
                    _compare_points(f"{label} {name} options {options} instantaneous t={t}",
                                    m.quantities_instantaneous(mid, state, t), values, hq.point_tolerance(values))
        for (name, index, _), mid, st in zip(manifolds, ids, stats):
            tag = f"{label} {name} options {options}"
            series = m.quantities_time_series(mid)
            if averaged:
                _compare_series(tag, series, st, hq.chain_length([len(index)]))
            else:
                assert series.shape == (0, 1 + 2 * m.k)  # (:511-514) accumulate skips it
            if options & T:
                got, t_begin, t_end = m.quantities_time_averaged(mid)
                expected, e_begin, e_end = st.time_averaged()
                assert (t_begin, t_end) == (e_begin, e_end) == (times[0], times[-1])
                _compare_points(tag + " time averaged", got, expected, st.time_averaged_tolerance())
            else:
                out = np.zeros((len(index), 2 * m.k))
                t0, t1 = C.c_double(), C.c_double()
                assert capi.load_hip().ryujin_hip_quantities_time_averaged(
                    m._ctx, mid, capi.as_ptr(out, capi.c_double_p), C.byref(t0), C.byref(t1)) == capi.RYUJIN_ERR_ARG
    state.free()


# ------------------------------------------------------------------------------------------------ 1. golden

def _mass_conservation_run(download_forbidden, monkeypatch=None):
    off = offline.SyntheticOffline(offline.rectangle_2d(64, (0.0, 0.0), (20.0, 20.0)))
    m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip")
    lengths = np.diff(off.row_starts.astype(np.int64))
    index = quantities.select_interior_points(0.0, off.positions, lengths, off.n_owned)
    mid = m.quantities_add_manifold(index, off.mi[index], S)  # interior : 0. : space_averaged
    sv = m.new_state_vector(euler_uniform(off.positions))
    ti = TimeIntegrator(m, "ssprk 33", cfl_min=0.9, cfl_max=0.9, cfl_recovery_strategy="none")
    if download_forbidden:
        def refuse(self):
            raise AssertionError("the state is never downloaded in this run")
        monkeypatch.setattr(StateVector, "download", refuse)
    stats = _Stats(capi.EQ_EULER, 2, m.params, index, off.mi[index])
    t = 0.0
    for _ in range(19):
        m.quantities_accumulate(sv, t)
        if not download_forbidden:
            stats.accumulate(sv.download(), t)
        sv, tau = ti.step(sv, t)
        t += tau
    series = m.quantities_time_series(mid)  # read once, at the end
    assert m.n_warnings() == 0
    m.close()
    return series, stats, len(index)


def test_mass_conservation_01_golden_series_from_the_device(golden_dir, monkeypatch):
    """tests/euler/check-mass-conservation_01: the 19 rows of the reference's space_averaged_time_series, accumulated
    on the device after every step of a run whose state never leaves it"""
    from test_oracle_golden_integration import golden_mass_conservation
    gold = golden_mass_conservation(golden_dir)
    got, _, _ = _mass_conservation_run(True, monkeypatch)
    assert got.shape == gold.shape == (19, 9)
    for c in range(9):
        print(f"column {c}: max abs diff {np.abs(got[:, c] - gold[:, c]).max():.3e}")
    # exactly the tolerances of test_gpu_parity.test_mass_conservation_01_golden_on_gpu
    np.testing.assert_allclose(got[:, 0], gold[:, 0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got[:, [1, 2, 4]], gold[:, [1, 2, 4]], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got[:, [5, 6, 8]], gold[:, [5, 6, 8]], rtol=1e-11, atol=0)
    assert np.abs(got[:, 1] - 1.4).max() < 1e-13
    monkeypatch.undo()
    # the two v_2 columns (means ~ 1e-18 of terms ~ 1e-3): against the helper on the states of a second run
    again, stats, n = _mass_conservation_run(False)
    assert np.array_equal(again, got)
    _compare_series("golden run", again, stats, hq.chain_length([n]))


# ------------------------------------------------------------------------------------------------ 2. descriptions

def test_euler_1d():
    off = offline.SyntheticOffline(offline.MeshSpec(1, (160,), (-1.0,), (1.0,), (capi.BC_SLIP, capi.BC_SLIP)))
    x = off.positions[:, 0]
    U0 = np.zeros((len(x), 3))
    U0[:, 0] = np.where(x < 0.0, 1.0, 0.125)
    U0[:, 2] = np.where(x < 0.0, 2.5, 0.25)
    m = HyperbolicModule(off, _params(capi.EQ_EULER, 1), backend="hip")
    _run_case("euler 1d", off, m, _developed_states(m, U0, None, 4, len(TIMES)))
    m.close()


def test_euler_2d():
    off = offline.SyntheticOffline(offline.mach3_step_2d(40))
    rng = np.random.default_rng(11)
    U0 = euler_uniform(off.positions)
    U0 *= 1.0 + 1e-3 * rng.uniform(-1, 1, size=U0.shape)
    m = HyperbolicModule(off, _params(capi.EQ_EULER, 2), backend="hip")
    _run_case("euler 2d", off, m, _developed_states(m, U0, euler_uniform(off.b_positions), 6, len(TIMES)))
    m.close()


def test_euler_3d():
    off = offline.SyntheticOffline(offline.box_3d(20))
    m = HyperbolicModule(off, _params(capi.EQ_EULER, 3), backend="hip")
    U0 = euler_radial_contrast(off.positions, radius=0.3)
    _run_case("euler 3d", off, m, _developed_states(m, U0, None, 4, len(TIMES)))
    m.close()


def test_shallow_water_with_dry_nodes():
    """(h, v) with the sharp inverse water depth: the developed dam break, and in the later states a dry strip (h = 0,
    with and without a residual momentum) next to it"""
    off = offline.SyntheticOffline(offline.rectangle_2d(48, (-5.0, -5.0), (5.0, 5.0)))
    x = off.positions
    m = HyperbolicModule(off, _params(capi.EQ_SHALLOW_WATER, 2), backend="hip")
    U_list = _developed_states(m, sw_circular_dam_break(x), None, 4, len(TIMES))
    dry = x[:, 0] > 3.0
    for U in U_list[2:]:
        U[dry, :] = 0.0
        U[dry & (x[:, 1] > 0.0), 1] = 1.0e-18
    assert (U_list[-1][: off.n_owned, 0] == 0.0).any() and (U_list[-1][: off.n_owned, 0] > 1.0).any()
    _run_case("shallow water", off, m, U_list)
    m.close()


def test_euler_aeos():
    off = offline.SyntheticOffline(offline.mach3_step_2d(30))
    U0 = euler_uniform(off.positions)
    U0 *= 1.0 + 1e-3 * np.sin(7.0 * off.positions[:, :1] + 3.0 * off.positions[:, 1:2])
    m = HyperbolicModule(off, _params(capi.EQ_EULER_AEOS, 2), backend="hip")
    _run_case("euler aeos", off, m, _developed_states(m, U0, euler_uniform(off.b_positions), 5, len(TIMES)))
    m.close()


def test_scalar_conservation():
    off = offline.SyntheticOffline(offline.rectangle_2d(48, (-2.0, -2.5), (2.0, 1.5), bc=capi.BC_DIRICHLET))
    r = np.linalg.norm(off.positions, axis=1)
    U0 = np.where(r < 1.0, 1.0, -0.5).reshape(-1, 1)
    m = HyperbolicModule(off, _params(capi.EQ_SCALAR_CONSERVATION, 2), backend="hip")
    _run_case("scalar", off, m, _developed_states(m, U0, U0[off.b_i], 4, len(TIMES)))
    m.close()


# ------------------------------------------------------------------------------------------------ 3. reference rules

def _small_euler():
    off = offline.SyntheticOffline(offline.mach3_step_2d(20))
    m = HyperbolicModule(off, _params(capi.EQ_EULER, 2), backend="hip")
    from quantities_rccl_worker import partition_state
    return off, m, partition_state


def _time_averaged_rc(m, mid, n_points):
    out = np.full((n_points, 2 * m.k), -7.0)
    t0, t1 = C.c_double(-7.0), C.c_double(-7.0)
    rc = capi.load_hip().ryujin_hip_quantities_time_averaged(m._ctx, mid, capi.as_ptr(out, capi.c_double_p),
                                                             C.byref(t0), C.byref(t1))
    return rc, out, t0.value, t1.value


@pytest.mark.parametrize("t0", [0.0, 0.375])
def test_first_call_clear_and_stale_instantaneous(t0):
    off, m, state_of = _small_euler()
    _, index, weight = _manifolds(off)[1]
    mid = m.quantities_add_manifold(index, weight, I | T | S)
    stats = _Stats(capi.EQ_EULER, 2, m.params, index, weight)
    state = m.new_state_vector()
    # nothing accumulated yet: "none yet", out untouched; no values to return either
    rc, out, a, b = _time_averaged_rc(m, mid, len(index))
    assert rc == capi.Q_NONE_YET and (out == -7.0).all() and (a, b) == (-7.0, -7.0)
    with pytest.raises(RuntimeError, match="status -2"):
        m.quantities_instantaneous(mid, state, t0)
    # the first call accumulates nothing (also when the run starts at t = 0) ...
    U = [state_of(off.positions, s) for s in range(4)]
    state.upload(U[0])
    m.quantities_accumulate(state, t0)
    stats.accumulate(U[0], t0)
    rc, out, a, b = _time_averaged_rc(m, mid, len(index))
    assert rc == capi.Q_NONE_YET and (out == -7.0).all()
    _compare_points("first call", m.quantities_instantaneous(mid, state, t0), stats.val_new,
                    hq.point_tolerance(stats.val_new))
    # ... the second one the first interval
    state.upload(U[1])
    m.quantities_accumulate(state, t0 + 0.5)
    stats.accumulate(U[1], t0 + 0.5)
    got, t_begin, t_end = m.quantities_time_averaged(mid)
    expected, e_begin, e_end = stats.time_averaged()
    assert (t_begin, t_end) == (e_begin, e_end) == (t0, t0 + 0.5)
    _compare_points("second call", got, expected, stats.time_averaged_tolerance())
    # a stale t is refused (AssertThrow(t_new == t)), the current one served
    with pytest.raises(RuntimeError, match="status -2"):
        m.quantities_instantaneous(mid, state, t0)
    assert m.quantities_instantaneous(mid, state, t0 + 0.5).shape == (len(index), 8)
    # clear_statistics: sums, times and series start over; the first call after it accumulates nothing again
    m.quantities_clear_statistics()
    stats.clear()
    assert m.quantities_time_series(mid).shape == (0, 9)
    assert _time_averaged_rc(m, mid, len(index))[0] == capi.Q_NONE_YET
    for s, t in ((2, t0 + 1.0), (3, t0 + 1.25), (0, t0 + 2.0)):
        state.upload(U[s])
        m.quantities_accumulate(state, t)
        stats.accumulate(U[s], t)
        if s == 2:
            assert _time_averaged_rc(m, mid, len(index))[0] == capi.Q_NONE_YET
    got, t_begin, t_end = m.quantities_time_averaged(mid)
    expected, e_begin, e_end = stats.time_averaged()
    assert (t_begin, t_end) == (e_begin, e_end) == (t0 + 1.0, t0 + 2.0)
    _compare_points("after clear", got, expected, stats.time_averaged_tolerance())
    _compare_series("after clear", m.quantities_time_series(mid), stats, hq.chain_length([len(index)]))
    m.close()


def test_series_read_with_clear_and_beyond_its_first_allocation():
    off, m, state_of = _small_euler()
    _, index, weight = _manifolds(off)[1]
    mid = m.quantities_add_manifold(index, weight, S)
    U = [state_of(off.positions, s) for s in range(3)]
    states = [m.new_state_vector(u) for u in U]
    means = [hq.weighted_mean(weight, hq.point_values(capi.EQ_EULER, 2, m.params, u, index)) for u in U]
    tols = [hq.mean_tolerance(weight, hq.point_values(capi.EQ_EULER, 2, m.params, u, index),
                              hq.chain_length([len(index)])) for u in U]
    n = 5200
    for r in range(n):
        m.quantities_accumulate(states[r % 3], 0.125 * r)
    got = m.quantities_time_series(mid, clear=True)
    assert got.shape == (n, 9)
    assert np.array_equal(got[:, 0], 0.125 * np.arange(n))  # complete and in order
    for s in range(3):
        assert (np.abs(got[s::3, 1:] - means[s]) <= tols[s]).all()
        assert (got[s::3, 1:] == got[s, 1:]).all()  # the same state gives the same bits every time
    # read with clear: the series restarts empty and fills from its first row again
    assert m.quantities_time_series(mid).shape == (0, 9)
    m.quantities_accumulate(states[1], 99.0)
    again = m.quantities_time_series(mid)
    assert again.shape == (1, 9) and again[0, 0] == 99.0 and np.array_equal(again[0, 1:], got[1, 1:])
    m.close()


# ------------------------------------------------------------------------------------------------ 4. bits

def _all_outputs(off, manifolds, options, U_list):
    m = HyperbolicModule(off, _params(capi.EQ_EULER, 2), backend="hip")
    ids = [m.quantities_add_manifold(index, weight, options) for index, weight in manifolds]
    state = m.new_state_vector()
    for s, U in enumerate(U_list):
        state.upload(U)
        m.quantities_accumulate(state, TIMES[s])
    out = []
    for mid in ids:
        averaged, t_begin, t_end = m.quantities_time_averaged(mid)
        out.append((m.quantities_instantaneous(mid, state, TIMES[len(U_list) - 1]), averaged, (t_begin, t_end),
                    m.quantities_time_series(mid)))
    m.close()
    return out


def test_two_runs_agree_bit_for_bit_and_gather_equals_contiguous():
    off = offline.SyntheticOffline(offline.mach3_step_2d(40))
    from quantities_rccl_worker import partition_state
    U_list = [partition_state(off.positions, s) for s in range(4)]
    (_, full, w_full), _, (_, b_index, b_weight) = _manifolds(off)
    swapped = full.copy()
    swapped[-2:] = full[-2:][::-1]  # no longer one contiguous run: the gather path
    w_swapped = off.mi[swapped]
    manifolds = [(full, w_full), (swapped, w_swapped), (b_index, b_weight)]
    first = _all_outputs(off, manifolds, I | T | S, U_list)
    second = _all_outputs(off, manifolds, I | T | S, U_list)
    for a, b in zip(first, second):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        assert np.array_equal(a[3], b[3])
    contiguous, gathered = first[0], first[1]
    order = np.arange(len(full))
    order[-2:] = order[-2:][::-1]
    assert np.array_equal(contiguous[0][order], gathered[0]) and np.array_equal(contiguous[1][order], gathered[1])
    D = hq.chain_length([len(full)])
    m_params = _params(capi.EQ_EULER, 2)
    for r, U in enumerate(U_list):
        tol = hq.mean_tolerance(w_full, hq.point_values(capi.EQ_EULER, 2, m_params, U, full), D)
        assert (np.abs(contiguous[3][r, 1:] - gathered[3][r, 1:]) <= tol).all()


# ------------------------------------------------------------------------------------------------ 5. ranks

def test_three_ranks_with_a_manifold_that_is_empty_on_one():
    import quantities_rccl_worker as worker
    n_ranks, cpu = 3, 30
    single = offline.SyntheticOffline(offline.mach3_step_2d(cpu))
    parts = [offline.SyntheticOffline(offline.mach3_step_2d(cpu, n_ranks=n_ranks, rank=r)) for r in range(n_ranks)]
    params = _params(capi.EQ_EULER, 2)
    indices = [worker.select(p) for p in parts]
    assert len(indices[0]) > 0 and len(indices[1]) > 0 and len(indices[2]) == 0

    def body(m, part, r):
        index = indices[r]
        mid = m.quantities_add_manifold(index, part.mi[index], worker.OPTIONS)
        none = m.quantities_add_manifold([], [], S)  # empty on all ranks
        state = m.new_state_vector()
        for s, t in enumerate(worker.TIMES):
            state.upload(worker.partition_state(part.positions, s))
            m.quantities_accumulate(state, t)
        return (m.quantities_time_series(mid), m.quantities_time_series(none),
                m.quantities_instantaneous(mid, state, worker.TIMES[-1]), m.quantities_time_averaged(mid))

    ranks = run_hip_ranks(parts, lambda: _copy_params(params), body)
    _check_ranks(single, parts, indices, params,
                 [dict(series=r[0], series_none=r[1], instantaneous=r[2], averaged=r[3][0],
                       interval=np.array(r[3][1:])) for r in ranks])


def _check_ranks(single, parts, indices, params, ranks):
    import quantities_rccl_worker as worker
    n_ranks = len(parts)
    # the one-rank device run on the global mesh, the same manifold
    g_index = worker.select(single)
    m = HyperbolicModule(single, _copy_params(params), backend="hip")
    mid = m.quantities_add_manifold(g_index, single.mi[g_index], worker.OPTIONS)
    stats = _Stats(capi.EQ_EULER, 2, params, g_index, single.mi[g_index])
    state = m.new_state_vector()
    for s, t in enumerate(worker.TIMES):
        U = worker.partition_state(single.positions, s)
        state.upload(U)
        m.quantities_accumulate(state, t)
        stats.accumulate(U, t)
    inst_1 = m.quantities_instantaneous(mid, state, worker.TIMES[-1])
    avg_1, t_begin, t_end = m.quantities_time_averaged(mid)
    m.close()
    point_of = {int(g): p for p, g in enumerate(single.global_ids[g_index])}
    assert sum(len(i) for i in indices) == len(g_index)
    D = hq.chain_length([len(i) for i in indices])
    for r in range(n_ranks):
        got = ranks[r]
        rows = np.array([point_of[int(g)] for g in parts[r].global_ids[indices[r]]], dtype=np.int64)
        # per point: bitwise the one-rank device run at the same global nodes
        assert np.array_equal(got["instantaneous"], inst_1[rows]) and np.array_equal(got["averaged"], avg_1[rows])
        assert tuple(got["interval"]) == (t_begin, t_end) == (worker.TIMES[0], worker.TIMES[-1])
        # the series: the helper on the global mesh, and the same bits on every rank
        _compare_series(f"rank {r}", got["series"], stats, D)
        assert np.array_equal(got["series"], ranks[0]["series"])
        # empty on all ranks: the reference's 0/0
        none = got["series_none"]
        assert none.shape == (len(worker.TIMES), 9) and np.array_equal(none[:, 0], worker.TIMES)
        assert np.isnan(none[:, 1:]).all()


def test_rccl_leg_over_the_test_double(tmp_path):
    """the same partitioned case through the library's ncclAllReduce(sum) of the weighted sums: three processes on one
    GPU over tests/cpp/librccl_stub.so"""
    import quantities_rccl_worker as worker
    import test_rccl_stub
    world, cpu = 3, 30
    prefix = str(tmp_path / "q")
    test_rccl_stub.launch(world, [prefix, str(cpu)], tmp_path, timeout=300, worker=worker.__file__)
    single = offline.SyntheticOffline(offline.mach3_step_2d(cpu))
    parts = [offline.SyntheticOffline(offline.mach3_step_2d(cpu, n_ranks=world, rank=r)) for r in range(world)]
    ranks = [dict(np.load(f"{prefix}.rank{r}.npz")) for r in range(world)]
    indices = [worker.select(p) for p in parts]
    for r in range(world):
        assert np.array_equal(ranks[r]["index"], indices[r])
    assert len(indices[2]) == 0 < len(indices[1])
    _check_ranks(single, parts, indices, _params(capi.EQ_EULER, 2), ranks)


# ------------------------------------------------------------------------------------------------ 6. argument errors

def test_argument_errors():
    off, m, state_of = _small_euler()
    lib, ctx = capi.load_hip(), m._ctx
    state = m.new_state_vector(state_of(off.positions))
    n = off.n_owned
    mid = C.c_int(-1)

    def refused(rc, *words):
        assert rc == capi.RYUJIN_ERR_ARG, rc
        message = lib.ryujin_hip_last_error().decode()
        assert message and all(w in message for w in words), message

    def add(index, weight, options, out=mid):
        index = np.asarray(index, dtype=np.uint32)
        weight = np.asarray(weight, dtype=np.float64)
        return lib.ryujin_hip_quantities_add_manifold(ctx, len(index), capi.as_ptr(index, capi.c_u32_p),
                                                      capi.as_ptr(weight, capi.c_double_p), options,
                                                      C.byref(out) if out is not None else None)

    refused(add([0, n], [1.0, 1.0], S), "index", str(n))
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(add([0, 1], [1.0, bad], S), "weight")
    refused(add([0], [1.0], 0), "options")
    refused(add([0], [1.0], 8), "options")
    refused(add([0], [1.0], S | 16), "options")
    refused(lib.ryujin_hip_quantities_add_manifold(ctx, 2, None, None, S, C.byref(mid)), "null")
    refused(add([0], [1.0], S, out=None), "null")
    assert mid.value == -1  # nothing was added
    refused(lib.ryujin_hip_quantities_accumulate(ctx, 99, 0.0), "handle")
    assert lib.ryujin_hip_quantities_accumulate(ctx, state.handle, 0.0) == capi.RYUJIN_OK  # no manifolds: nothing to do
    # unknown manifold ids
    out = np.zeros((2, 8))
    t0, t1, n_rows = C.c_double(), C.c_double(), C.c_size_t()
    for bad in (-1, 0, 3):
        refused(lib.ryujin_hip_quantities_instantaneous(ctx, bad, state.handle, 0.0, capi.as_ptr(out, capi.c_double_p)),
                "manifold")
        refused(lib.ryujin_hip_quantities_time_averaged(ctx, bad, capi.as_ptr(out, capi.c_double_p), C.byref(t0),
                                                        C.byref(t1)), "manifold")
        refused(lib.ryujin_hip_quantities_time_series(ctx, bad, None, 0, C.byref(n_rows), 0), "manifold")
    # options a call needs
    assert add([0, 1], [1.0, 2.0], S) == capi.RYUJIN_OK and mid.value == 0
    assert add([0, 1], [1.0, 2.0], I | T) == capi.RYUJIN_OK and mid.value == 1
    refused(lib.ryujin_hip_quantities_time_averaged(ctx, 0, capi.as_ptr(out, capi.c_double_p), C.byref(t0),
                                                    C.byref(t1)), "TIME_AVERAGED")
    refused(lib.ryujin_hip_quantities_instantaneous(ctx, 0, state.handle, 0.0, capi.as_ptr(out, capi.c_double_p)),
            "INSTANTANEOUS")
    refused(lib.ryujin_hip_quantities_instantaneous(ctx, 1, state.handle, 0.0, None), "null")
    refused(lib.ryujin_hip_quantities_time_averaged(ctx, 1, None, C.byref(t0), C.byref(t1)), "null")
    refused(lib.ryujin_hip_quantities_time_series(ctx, 0, None, 0, None, 0), "null")
    # a capacity that is too small reports the rows it needs
    for t in (0.5, 1.0, 1.5):
        assert lib.ryujin_hip_quantities_accumulate(ctx, state.handle, t) == capi.RYUJIN_OK
    rows = np.zeros((3, 9))
    refused(lib.ryujin_hip_quantities_time_series(ctx, 0, capi.as_ptr(rows, capi.c_double_p), 2, C.byref(n_rows), 1),
            "3 rows", "capacity of 2")
    assert n_rows.value == 3 and (rows == 0.0).all()
    assert lib.ryujin_hip_quantities_time_series(ctx, 0, capi.as_ptr(rows, capi.c_double_p), 3, C.byref(n_rows),
                                                 0) == capi.RYUJIN_OK
    assert n_rows.value == 3 and np.array_equal(rows[:, 0], [0.5, 1.0, 1.5])  # the refused call cleared nothing
    # more than RYUJIN_Q_MAX_MANIFOLDS; reset makes room again
    for _ in range(capi.Q_MAX_MANIFOLDS - 2):
        assert add([0], [1.0], S) == capi.RYUJIN_OK
    assert mid.value == capi.Q_MAX_MANIFOLDS - 1
    refused(add([0], [1.0], S), "RYUJIN_Q_MAX_MANIFOLDS")
    assert lib.ryujin_hip_quantities_reset(ctx) == capi.RYUJIN_OK
    refused(lib.ryujin_hip_quantities_time_series(ctx, 0, None, 0, C.byref(n_rows), 0), "manifold")
    assert add([0], [1.0], S) == capi.RYUJIN_OK and mid.value == 0
    assert lib.ryujin_hip_quantities_reset(None) == capi.RYUJIN_ERR_ARG
    m.close()


# ------------------------------------------------------------------------------------------------ 7. full size

def test_full_size_c2_mesh_time_and_space_averaged():
    """the C2 mesh of bench.py (2.5 M gridpoints) on its developed state: the full-interior manifold, four
    accumulations with an update between them, every point and every mean against the helper"""
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
    lengths = np.diff(off.row_starts.astype(np.int64))
    index = quantities.select_interior_points(0.0, off.positions, lengths, off.n_owned)
    assert np.array_equal(index, np.arange(off.n_owned))
    mid = m.quantities_add_manifold(index, off.mi[index], T | S)
    stats = _Stats(capi.EQ_EULER, 2, m.params, index, off.mi[index])
    t = 0.0
    for _ in range(4):
        m.quantities_accumulate(state, t)
        stats.accumulate(state.download(), t)
        t += m.time_step("ssprk 33", state, temps, None)
    D = hq.chain_length([len(index)])
    assert D * hq.EPS <= hq.FUNCTION_LEVEL
    _compare_series("C2", m.quantities_time_series(mid), stats, D)
    got, t_begin, t_end = m.quantities_time_averaged(mid)
    expected, e_begin, e_end = stats.time_averaged()
    assert (t_begin, t_end) == (e_begin, e_end) and t_begin == 0.0 and t_end > 0.0
    _compare_points("C2 time averaged", got, expected, stats.time_averaged_tolerance())
    m.close()
