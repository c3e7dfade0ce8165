"""Device-resident TimeLoop::compute_error() (ryujin_hip_error_norms_*) against the numpy restatement of
tests/helpers_error_norms.py, the independent norms_1d / norms_2d of tests/test_oracle_golden_verification.py and the
reference's own verification baselines under tests/golden/. Linf values are compared bit for bit, integrals within the
bound the helper derives from the kernel's launch shape."""
import ctypes as C

import numpy as np
import pytest

import helpers_error_norms as hen
import helpers_q1_quads as hq1
from helpers_partitioned import run_hip_ranks
from ryujin_amd import HyperbolicModule, StateVector, capi, error_norms, offline
from ryujin_amd.initial_states import euler_uniform

pytestmark = pytest.mark.gpu


def _params(equation, dim):
    p = capi.Params()
    capi.load_hip().ryujin_hip_default_params(C.byref(p), equation, dim)
    return p


def _copy_params(p):
    q = capi.Params()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(capi.Params))
    return q


def _lattice(dim, n_cells, bc=capi.BC_SLIP):
    lower, upper = (0.0, -1.0, 0.5)[:dim], (2.0, 0.25, 1.25)[:dim]
    return offline.SyntheticOffline(offline.MeshSpec(dim, tuple(n_cells), lower, upper, (bc,) * (2 * dim)))


def _quads():
    points, quads, edges = hq1.annulus_mesh(4, 12)
    off, _ = hq1.q1_quads_offline(points, quads, edges)
    return off, hen.lexicographic_quads(quads)


def _hexes():
    points, hexes, faces = hq1.annulus_mesh_3d(3, 8, 2)
    off, _ = hq1.q1_hexes_offline(points, hexes, faces)
    return off, hexes


def _gauss2_tables():
    """Q1 in 2-D with QGauss(2): four points -- none of the register instantiations, the run-time table path"""
    g = 0.5 + np.array([-0.5, 0.5]) / np.sqrt(3.0)
    points = np.array([(a, b) for b in g for a in g])
    shape = np.array([[(x if v & 1 else 1.0 - x) * (y if v & 2 else 1.0 - y) for v in range(4)] for x, y in points])
    return shape, np.full(4, 0.25)


# name -> (equation, dim, mesh): a lattice (both JxW forms) or (offline, cells) of skewed cells (JxW per point)
CASES = {
    "euler_1d_17": (capi.EQ_EULER, 1, lambda: _lattice(1, (17,))),
    "euler_2d_7x5": (capi.EQ_EULER, 2, lambda: _lattice(2, (7, 5))),          # less than one wave of cells
    "euler_2d_40x30": (capi.EQ_EULER, 2, lambda: _lattice(2, (40, 30))),      # 1200 cells: blocks, no multiple of 64
    "euler_3d_5x4x3": (capi.EQ_EULER, 3, lambda: _lattice(3, (5, 4, 3))),
    "euler_2d_quads": (capi.EQ_EULER, 2, _quads),
    "euler_3d_hexes": (capi.EQ_EULER, 3, _hexes),
    "shallow_water_2d": (capi.EQ_SHALLOW_WATER, 2, lambda: _lattice(2, (7, 5))),
    # scalar conservation has no slip boundary: Dirichlet all round
    "scalar_2d": (capi.EQ_SCALAR_CONSERVATION, 2, lambda: _lattice(2, (7, 5), bc=capi.BC_DIRICHLET)),
}
FORMS = [(name, form) for name in CASES for form in (("per point",) if "quads" in name or "hexes" in name
                                                      else ("per point", "per cell"))]


def _tables(off, cells, dim, form, table="gauss3"):
    shape, weights = error_norms.q1_tables(dim) if table == "gauss3" else _gauss2_tables()
    if form == "per cell":
        return shape, weights, np.full(len(cells), off.cell_measure)
    if table == "gauss3":
        return shape, None, error_norms.q1_jxw(off.positions, cells)
    return shape, None, np.outer(np.full(len(cells), off.cell_measure), weights)


def _run_against_restatement(label, equation, dim, off, cells, shape, weights, jxw, seed):
    m = HyperbolicModule(off, _params(equation, dim), backend="hip")
    U, A = hen.random_vectors(off.n_relevant, m.k, seed)
    state, analytic = m.new_state_vector(U), m.new_state_vector(A)
    m.error_norms_configure(cells, shape, jxw, weights)
    names = capi.component_names(equation, dim)[0]
    D = hen.chain_length([len(cells)], shape.shape[0])
    selections = [None] + ([[names[-1], names[0]]] if m.k > 1 else [])  # all, and a reordered subset
    for components in selections:
        index = list(range(m.k)) if components is None else [names.index(c) for c in components]
        for normalize in (True, False):
            out, detail = m.error_norms_compute(state, analytic, components, normalize)
            ref = hen.restatement(U, A, off.n_owned, cells, shape, jxw, index, normalize, weights, D)
            hen.compare(f"{label} components {index} normalize {normalize}", out, detail, ref)
            again = m.error_norms_compute(state, analytic, components, normalize)
            assert np.array_equal(again[0], out) and np.array_equal(again[1], detail)  # the same bits
    m.close()


# ------------------------------------------------------------------------------------------------ A. restatement

@pytest.mark.parametrize("name,form", FORMS)
def test_against_the_numpy_restatement(name, form):
    equation, dim, mesh = CASES[name]
    made = mesh()
    off, cells = made if isinstance(made, tuple) else (made, made.cells)
    shape, weights, jxw = _tables(off, cells, dim, form)
    _run_against_restatement(f"{name} {form}", equation, dim, off, cells, shape, weights, jxw, seed=len(name))


@pytest.mark.parametrize("form", ["per point", "per cell"])
def test_a_table_outside_the_register_instantiations(form):
    off = _lattice(2, (40, 30))
    shape, weights, jxw = _tables(off, off.cells, 2, form, table="gauss2")
    _run_against_restatement(f"gauss2 {form}", capi.EQ_EULER, 2, off, off.cells, shape, weights, jxw, seed=3)


# ------------------------------------------------------------------------------------------------ B. independent norms

def _sorted_grid(off, values):
    n = off.spec.n_cells
    if off.dim == 1:
        return values[np.argsort(off.positions[:, 0])]
    order = np.lexsort((off.positions[:, 0], off.positions[:, 1]))
    return values[order].reshape(n[1] + 1, n[0] + 1).T


@pytest.mark.parametrize("dim,n_cells,upper", [(1, (17,), (3.4,)), (2, (40, 30), (4.0, 3.0))])
def test_uniform_meshes_against_the_independent_norms(dim, n_cells, upper):
    from test_oracle_golden_verification import norms_1d, norms_2d
    norms = norms_1d if dim == 1 else norms_2d
    off = offline.SyntheticOffline(offline.MeshSpec(dim, n_cells, (0.0,) * dim, upper, (capi.BC_SLIP,) * (2 * dim)))
    h = upper[0] / n_cells[0]
    m = HyperbolicModule(off, _params(capi.EQ_EULER, dim), backend="hip")
    U, A = hen.random_vectors(off.n_relevant, m.k, seed=17)
    state, analytic = m.new_state_vector(U), m.new_state_vector(A)
    shape, weights = error_norms.q1_tables(dim)
    cells, measure = off.cells, np.full(off.n_cells, off.cell_measure)
    m.error_norms_configure(cells, shape, measure, weights)
    out, detail = m.error_norms_compute(state, analytic, None, True)
    # the derived bounds of the helper, around the independent norms
    ref = hen.restatement(U, A, off.n_owned, cells, shape, measure, list(range(m.k)), True, weights,
                          hen.chain_length([len(cells)], shape.shape[0]))
    linf = l1 = l2 = 0.0
    for c in range(m.k):
        a, e = A[:, c], U[:, c] - A[:, c]
        (l1a, l2a), (l1e, l2e) = norms(_sorted_grid(off, a), h), norms(_sorted_grid(off, e), h)
        independent = np.array([np.abs(e).max(), l1e, l2e, np.abs(a).max(), l1a, l2a])
        err = np.abs(detail[c] - independent)
        print(f"component {c}: err / tol {err[[1, 2, 4, 5]] / ref['tol_detail'][c, [1, 2, 4, 5]]}")
        assert detail[c, 0] == independent[0] and detail[c, 3] == independent[3]
        assert (err[[1, 2, 4, 5]] <= ref["tol_detail"][c, [1, 2, 4, 5]]).all(), (c, err, ref["tol_detail"][c])
        linf += np.abs(e).max() / np.abs(a).max()
        l1 += l1e / l1a
        l2 += l2e / l2a
    assert out[0] == linf
    assert abs(out[1] - l1) <= ref["tol_out"][1] and abs(out[2] - l2) <= ref["tol_out"][2], (out, l1, l2)
    m.close()


# ------------------------------------------------------------------------------------------------ C. the reference

def _refuse_download(monkeypatch):
    def refuse(self):
        raise AssertionError("the state is never downloaded in this run")
    monkeypatch.setattr(StateVector, "download", refuse)


def _configure_q1(m, off):
    shape, weights = error_norms.q1_tables(off.dim)
    m.error_norms_configure(off.cells, shape, np.full(off.n_cells, off.cell_measure), weights)


@pytest.mark.parametrize("scheme", ["ssprk 33", "erk 33"])
def test_isentropic_vortex_golden_without_a_download(golden_dir, monkeypatch, scheme):
    """tests/euler/verification-isentropic_vortex-2d-*-l5 (1089 dofs): initial_values_interpolate -> time_step_iv ->
    compute_error; tolerances of test_gpu_parity.test_isentropic_vortex_golden_on_gpu"""
    from test_oracle_golden_integration import _golden_vortex
    from ryujin_amd.module import DeviceResidentTimeIntegrator
    dofs, t_ref, linf_ref, l1_ref, l2_ref = _golden_vortex(golden_dir, scheme, 5)
    _refuse_download(monkeypatch)
    off = offline.SyntheticOffline(offline.rectangle_2d(32, (-5.0, -5.0), (5.0, 5.0), bc=capi.BC_DIRICHLET))
    m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip")
    m.initial_values_configure("isentropic vortex", mach_number=1.0, beta=5.0, direction=(1.0, 1.0),
                               position=(-1.0, -1.0))
    _configure_q1(m, off)
    sv = m.new_state_vector()
    m.initial_values_interpolate(sv, 0.0)
    ti = DeviceResidentTimeIntegrator(m, scheme, cfl_min=0.2, cfl_max=0.2, cfl_recovery_strategy="none",
                                      dirichlet="device")
    t = 0.0
    while t < 2.0:
        sv, tau = ti.step(sv, t)
        t += tau
    (linf, l1, l2), detail = m.compute_error(sv, t)
    print(f"t {t!r} ({t_ref!r}), Linf {linf!r} ({linf_ref!r}), L1 {l1!r} ({l1_ref!r}), L2 {l2!r} ({l2_ref!r})")
    assert off.n_owned == dofs == 1089 and detail.shape == (4, 6)
    assert abs(t - t_ref) < 1e-10
    assert abs(linf - linf_ref) < 1e-8 * linf_ref
    assert abs(l1 - l1_ref) < 1e-8 * l1_ref
    assert abs(l2 - l2_ref) < 1e-8 * l2_ref
    m.close()


def _run_with_compute_error(config):
    """run_verification of tests/test_oracle_golden_verification.py, start to finish on the device: the stand-in of
    helpers_initial_values.run_verification_on_device with compute_error in place of the download and the host norms"""
    name, kwargs = config

    def run(backend, off, params, exact, components, scheme="erk 33", cfl=0.1, t_final=1.0, bathymetry=None,
            with_dirichlet=True):
        assert backend == "hip-error-norms" and off.dim == 1
        from ryujin_amd.module import DeviceResidentTimeIntegrator
        if bathymetry is not None:
            off.set_initial_precomputed(bathymetry)
        m = HyperbolicModule(off, params, backend="hip")
        m.initial_values_configure(name, **kwargs)
        _configure_q1(m, off)
        sv = m.new_state_vector()
        m.initial_values_interpolate(sv, 0.0)
        ti = DeviceResidentTimeIntegrator(m, scheme, cfl_min=cfl, cfl_max=cfl, cfl_recovery_strategy="none",
                                          dirichlet="device")
        t, n_steps = 0.0, 0
        while t < t_final:
            sv, tau = ti.step(sv, t)
            t += tau
            n_steps += 1
        names = capi.component_names(m.equation, 1)[0]
        (linf, l1, l2), _ = m.compute_error(sv, t, components=[names[c] for c in components])
        print(f"t {t!r}, Linf {linf!r}, L1 {l1!r}, L2 {l2!r} after {n_steps} steps")
        return dict(t=t, linf=linf, l1=l1, l2=l2, dofs=off.n_owned, n_steps=n_steps, warnings=m.n_warnings(),
                    restarts=m.n_restarts())

    return run


def _verification_cases():
    import helpers_initial_values as hiv
    return sorted(hiv.VERIFICATION)


@pytest.mark.parametrize("case", _verification_cases())
def test_verification_baselines_with_compute_error(oracle, golden_dir, monkeypatch, case):
    import helpers_initial_values as hiv
    import test_oracle_golden_verification as tv
    from test_gpu_parity import VERIFICATION_SLACK
    _refuse_download(monkeypatch)
    monkeypatch.setattr(tv, "run_verification", _run_with_compute_error(hiv.VERIFICATION[case]))
    fn, args = tv.CASES[case]
    fn("hip-error-norms", oracle.default_params, golden_dir, *args, slack=VERIFICATION_SLACK.get(case, 1.0))


# ------------------------------------------------------------------------------------------------ D. ranks

def test_three_ranks_one_of_which_owns_no_cell():
    import error_norms_rccl_worker as worker
    n_ranks, cpu = 3, 30
    single = offline.SyntheticOffline(offline.mach3_step_2d(cpu))
    parts = [offline.SyntheticOffline(offline.mach3_step_2d(cpu, n_ranks=n_ranks, rank=r)) for r in range(n_ranks)]
    cells = [worker.select_cells(p, worker.X_CUT) for p in parts]
    assert len(cells[0]) > 0 and len(cells[1]) > 0 and len(cells[2]) == 0
    shape, weights = error_norms.q1_tables(2)
    params = _params(capi.EQ_EULER, 2)

    def body(m, part, r):
        m.error_norms_configure(cells[r], shape, np.full(len(cells[r]), part.cell_measure), weights)
        state = m.new_state_vector(worker.state(part.positions))
        analytic = m.new_state_vector(worker.analytic(part.positions))
        return [m.error_norms_compute(state, analytic, None, normalize) for normalize in (True, False)]

    ranks = run_hip_ranks(parts, lambda: _copy_params(params), body)
    _check_ranks(single, parts, cells, worker.X_CUT, [[(np.array(o), d) for o, d in r] for r in ranks])


def _check_ranks(single, parts, cells, x_cut, ranks):
    import error_norms_rccl_worker as worker
    shape, weights = error_norms.q1_tables(2)
    g_cells = worker.select_cells(single, x_cut)
    assert sum(len(c) for c in cells) == len(g_cells)
    measure = np.full(len(g_cells), single.cell_measure)
    U, A = worker.state(single.positions), worker.analytic(single.positions)
    m = HyperbolicModule(single, _params(capi.EQ_EULER, 2), backend="hip")
    m.error_norms_configure(g_cells, shape, measure, weights)
    state, analytic = m.new_state_vector(U), m.new_state_vector(A)
    D_1 = hen.chain_length([len(g_cells)], 9)
    D_n = hen.chain_length([len(c) for c in cells], 9)
    for which, normalize in enumerate((True, False)):
        out_1, detail_1 = m.error_norms_compute(state, analytic, None, normalize)
        ref_1 = hen.restatement(U, A, single.n_owned, g_cells, shape, measure, [0, 1, 2, 3], normalize, weights, D_1)
        ref_n = hen.restatement(U, A, single.n_owned, g_cells, shape, measure, [0, 1, 2, 3], normalize, weights, D_n)
        hen.compare(f"one rank normalize {normalize}", out_1, detail_1, ref_1)
        for r, got in enumerate(ranks):
            out, detail = got[which]
            hen.compare(f"rank {r} of {len(ranks)} normalize {normalize}", out, detail, ref_n)
            assert np.array_equal(out, ranks[0][which][0]) and np.array_equal(detail, ranks[0][which][1])
            # against the one-rank device run: Linf equal, integrals within the two derived bounds
            assert np.array_equal(detail[:, [0, 3]], detail_1[:, [0, 3]]) and out[0] == out_1[0]
            assert (np.abs(detail - detail_1) <= ref_1["tol_detail"] + ref_n["tol_detail"]).all()
            assert (np.abs(np.array(out) - np.array(out_1)) <= ref_1["tol_out"] + ref_n["tol_out"]).all()
    m.close()


def test_rccl_leg_over_the_test_double(tmp_path):
    """two ranks through the library's ncclAllReduce (sum of the integrals, max of the nodal maxima): two processes on
    one GPU over tests/cpp/librccl_stub.so"""
    import error_norms_rccl_worker as worker
    import test_rccl_stub
    world, cpu = 2, 30
    prefix = str(tmp_path / "en")
    test_rccl_stub.launch(world, [prefix, str(cpu)], tmp_path, timeout=300, worker=worker.__file__)
    single = offline.SyntheticOffline(offline.mach3_step_2d(cpu))
    parts = [offline.SyntheticOffline(offline.mach3_step_2d(cpu, n_ranks=world, rank=r)) for r in range(world)]
    files = [dict(np.load(f"{prefix}.rank{r}.npz")) for r in range(world)]
    cells = [worker.select_cells(p, worker.X_ALL) for p in parts]
    for r in range(world):
        assert np.array_equal(files[r]["cells"], cells[r]) and len(cells[r]) > 0
    ranks = [[(f["out_normalized"], f["detail_normalized"]), (f["out_plain"], f["detail_plain"])] for f in files]
    _check_ranks(single, parts, cells, worker.X_ALL, ranks)


# ------------------------------------------------------------------------------------------------ E. zero analytic norm

def test_a_zero_analytic_component_gives_the_ieee_result():
    """the y-momentum of a uniform flow along x: 0 / 0 = NaN with zero error, x / 0 = inf with a non-zero one, as
    numpy's division; the consolidated sum inherits it"""
    off = _lattice(2, (7, 5))
    m = HyperbolicModule(off, _params(capi.EQ_EULER, 2), backend="hip")
    shape, weights = error_norms.q1_tables(2)
    measure = np.full(off.n_cells, off.cell_measure)
    m.error_norms_configure(off.cells, shape, measure, weights)
    A = euler_uniform(off.positions)
    assert (A[:, 2] == 0.0).all() and (A[:, 1] != 0.0).all()
    analytic = m.new_state_vector(A)
    D = hen.chain_length([off.n_cells], 9)
    for bump, expected in ((0.0, np.nan), (0.01, np.inf)):
        U = A.copy()
        U[:, 2] += bump
        U[:, 0] *= 1.001
        state = m.new_state_vector(U)
        for components, index in ((["m_2"], [2]), (None, [0, 1, 2, 3])):
            out, detail = m.error_norms_compute(state, analytic, components, True)
            ref = hen.restatement(U, A, off.n_owned, off.cells, shape, measure, index, True, weights, D)
            hen.compare(f"bump {bump} components {index}", out, detail, ref)
            row = detail[index.index(2)]
            assert (row[3:] == 0.0).all() and ((row[:3] == 0.0).all() if bump == 0.0 else (row[:3] > 0.0).all())
            assert np.array_equal(np.array(out), np.full(3, expected), equal_nan=True), out
        # without the normalisation nothing is divided: finite
        out, _ = m.error_norms_compute(state, analytic, None, False)
        assert np.isfinite(out).all()
    m.close()


# ------------------------------------------------------------------------------------------------ F. argument errors

def test_argument_errors():
    off = _lattice(2, (7, 5))
    m = HyperbolicModule(off, _params(capi.EQ_EULER, 2), backend="hip")
    lib, ctx = capi.load_hip(), m._ctx
    U, A = hen.random_vectors(off.n_relevant, 4, seed=1)
    state, analytic = m.new_state_vector(U), m.new_state_vector(A)
    shape, weights = error_norms.q1_tables(2)
    cells = np.ascontiguousarray(off.cells, dtype=np.uint32)
    n = len(cells)
    measure = np.full(n, off.cell_measure)
    jxw = np.ascontiguousarray(np.outer(measure, weights))
    out, detail = np.zeros(3), np.zeros((4, 6))
    dp, up = capi.c_double_p, capi.c_u32_p

    def refused(rc, *words):
        assert rc == capi.RYUJIN_ERR_ARG, rc
        message = lib.ryujin_hip_last_error().decode()
        assert message and all(w in message for w in words), message

    def configure(cells=cells, n_cells=n, dofs=4, n_q=9, shape=shape, weights=weights, jxw=measure, per_cell=1):
        ptr = lambda a, t: capi.as_ptr(np.ascontiguousarray(a), t) if a is not None else None  # noqa: E731
        return lib.ryujin_hip_error_norms_configure(ctx, n_cells, dofs, ptr(cells, up), n_q, ptr(shape, dp),
                                                    ptr(weights, dp), ptr(jxw, dp), per_cell)

    def compute(h_state=None, h_analytic=None, components=(0, 1, 2, 3), n_components=None):
        comp = (C.c_int * 8)(*components)
        return lib.ryujin_hip_error_norms_compute(
            ctx, state.handle if h_state is None else h_state, analytic.handle if h_analytic is None else h_analytic,
            len(components) if n_components is None else n_components, comp, 1, capi.as_ptr(out, dp),
            capi.as_ptr(detail, dp))

    refused(compute(), "before")
    bad = cells.copy()
    bad[3, 2] = off.n_relevant
    refused(configure(cells=bad), "index", str(off.n_relevant))
    for dofs in (1, 28):
        refused(configure(dofs=dofs, shape=np.ones((9, 28))), "dofs_per_cell")
    for n_q in (0, 65):
        refused(configure(n_q=n_q, shape=np.ones((65, 4)), weights=np.ones(65)), "n_q")
    for value in (np.nan, np.inf):
        broken = shape.copy()
        broken[4, 1] = value
        refused(configure(shape=broken), "shape")
        broken = weights.copy()
        broken[8] = value
        refused(configure(weights=broken), "weights")
        broken = measure.copy()
        broken[n - 1] = value
        refused(configure(jxw=broken), "jxw")
        broken = jxw.copy()
        broken[n - 1, 8] = value
        refused(configure(jxw=broken, per_cell=0, weights=None), "jxw")
    refused(configure(weights=None), "weights")
    refused(configure(cells=None), "null")
    refused(configure(jxw=None), "null")
    refused(configure(shape=None), "null")
    refused(compute(), "before")  # nothing of the above configured anything
    # a rank without cells is legal; so are NULL arrays then
    assert configure(cells=None, n_cells=0, jxw=None) == capi.RYUJIN_OK
    assert compute() == capi.RYUJIN_OK and (detail[:, [1, 2, 4, 5]] == 0.0).all() and (detail[:, [0, 3]] > 0.0).all()
    assert configure() == capi.RYUJIN_OK and compute() == capi.RYUJIN_OK
    first = (out.copy(), detail.copy())
    assert (first[1] > 0.0).all()
    refused(compute(components=(0, 4)), "component")
    refused(compute(components=(-1,)), "component")
    refused(compute(components=(0,), n_components=0), "n_components")
    refused(compute(components=(0, 1, 2, 3, 0), n_components=5), "n_components")
    refused(compute(h_state=99), "handle")
    refused(compute(h_analytic=-1), "handle")
    assert lib.ryujin_hip_error_norms_compute(None, 0, 0, 1, (C.c_int * 1)(0), 1, capi.as_ptr(out, dp),
                                              None) == capi.RYUJIN_ERR_ARG
    # a refused configure leaves the previous configuration working; a second one replaces the first
    refused(configure(cells=bad), "index")
    out[:], detail[:] = 0.0, 0.0
    assert compute() == capi.RYUJIN_OK
    assert np.array_equal(out, first[0]) and np.array_equal(detail, first[1])
    assert configure(cells=cells[: n // 2], n_cells=n // 2, jxw=measure[: n // 2]) == capi.RYUJIN_OK
    assert compute() == capi.RYUJIN_OK
    assert (detail[:, [1, 2, 4, 5]] < first[1][:, [1, 2, 4, 5]]).all()
    assert np.array_equal(detail[:, [0, 3]], first[1][:, [0, 3]])
    # the Python layer: unknown names, a primitive name
    with pytest.raises(ValueError):
        m.error_norms_compute(state, analytic, ["p"])
    m.close()
