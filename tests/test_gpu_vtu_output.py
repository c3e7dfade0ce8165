"""Device-resident VTUOutput (ryujin_hip_output_*, HyperbolicModule.output_*, ryujin_amd.vtu_output.VTUOutput) against
the numpy restatement of tests/helpers_vtu_output.py: level-set values bit for bit against the host interpreter, the
selection -- cells, nodes, renumbered connectivity -- by equality, the extracted quantities bit for bit against what the
module's own downloads return at those nodes (the primitive state within the tolerance derived there), Float32 as the
IEEE conversion of the Float64 output, ranks on the in-process transport, the refusals, and the files read back."""
import ctypes as C

import numpy as np
import pytest

import helpers_error_norms as hen
import helpers_q1_quads as hq1
import helpers_vtu_output as hv
from helpers_partitioned import run_hip_ranks
from ryujin_amd import HyperbolicModule, capi, offline
from ryujin_amd.initial_states import euler_uniform, sw_circular_dam_break
from ryujin_amd.vtu_output import VTUOutput

pytestmark = pytest.mark.gpu

BLOCK = 256   # kBlock: items per block of the compaction


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


def _lattice(dim, n_cells, bc=capi.BC_SLIP):
    lower, upper = (0.0, -1.0, 0.5)[:dim], (2.0, 0.25, 1.25)[:dim]
    return offline.SyntheticOffline(offline.MeshSpec(dim, tuple(n_cells), lower, upper, (bc,) * (2 * dim)))


def _quads():
    points, quads, edges = hq1.annulus_mesh(5, 16)
    off, _ = hq1.q1_quads_offline(points, quads, edges)
    return off, hen.lexicographic_quads(quads)


# name -> (dim, mesh). "big": the smallest 2-D lattice with more than BLOCK^2 cells: 257 blocks of cells, so the
# offset scan makes a second round with a carry
MESHES = {
    "line_130": (1, lambda: _lattice(1, (130,))),
    "lattice_33x31": (2, lambda: _lattice(2, (33, 31))),      # 1023 cells: blocks, no multiple of 64
    "lattice_9x10x11": (3, lambda: _lattice(3, (9, 10, 11))),
    "skewed_quads": (2, _quads),
    "big_257x256": (2, lambda: _lattice(2, (257, 256))),
}
assert 257 * 256 > BLOCK * BLOCK >= 256 * 256


@pytest.fixture(scope="module")
def mesh_modules():
    """name -> (offline data, cells, Euler module); built on first use, shared by the selection tests"""
    built = {}

    def get(name):
        if name not in built:
            dim, make = MESHES[name]
            made = make()
            off, cells = made if isinstance(made, tuple) else (made, made.cells)
            cells = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1, 2 ** dim)
            built[name] = (off, cells, HyperbolicModule(off, _params(capi.EQ_EULER, dim), backend="hip"))
        return built[name]
    yield get
    for _, _, m in built.values():
        m.close()


# ------------------------------------------------------------------------------------------------ A. level-set values

ARITHMETIC = {1: ["x - 0.37"],
              2: ["x - 0.37", "x*x + y*y - 0.25", "if(x > 0.5, x - 0.75, 0.25 - x) + 0.5*y"],
              3: ["x - 0.37", "x*x + y*y - 0.25", "x + 2*y - z - 0.1", "if(z > 0.9, x - 0.75, 0.25 - y)"]}


@pytest.mark.parametrize("name", ["line_130", "lattice_33x31", "lattice_9x10x11", "skewed_quads"])
def test_level_set_values_equal_the_host_interpreter(mesh_modules, name):
    off, cells, m = mesh_modules(name)
    manifolds = ARITHMETIC[off.dim]
    m.output_configure(["rho"], cells, manifolds)
    expected = hv.levelsets(manifolds, off.dim, off.positions)
    for q in range(len(manifolds)):
        got = m.output_levelset_values(q)
        assert got.shape == (off.n_relevant,) and np.array_equal(got, expected[q]), manifolds[q]
    assert (expected[0] > 0).any() and (expected[0] < 0).any()


# ------------------------------------------------------------------------------------------------ B. selection

def _node_exact(off):
    """a plane x = const through a lattice line of nodes: f is exactly 0 at those vertices (both counters rise)"""
    x = np.sort(np.unique(off.positions[:, 0]))
    return f"x - {float(x[len(x) // 3])!r}"


def _cases(off):
    lo = float(off.positions[:, 0].min())
    cut = {1: "x - 0.37", 2: "x*x + y*y - 0.25", 3: "x + 2*y - z - 0.1"}[off.dim]
    if off.dim == 2 and lo < 0.0:   # the annulus: a line through it
        cut = "x + 2*y - 0.1"
    return {"node exact": [_node_exact(off)], "misses": ["x + 200"], "all": ["0*x"], "cut": [cut],
            "two manifolds": ["x + 200", cut], "two that cut": [cut, _node_exact(off)]}


def _check_selection(m, off, cells, manifolds, label):
    n_cells, n_nodes = m.output_configure(["rho"], cells, manifolds)
    F = hv.levelsets(manifolds, off.dim, off.positions)
    cell_ids, node_ids, connectivity = hv.select(cells, F)
    got_cells, got_nodes, got_connectivity = m.output_selection()
    print(f"{label}: {n_cells} of {len(cells)} cells, {n_nodes} of {off.n_relevant} nodes")
    assert (n_cells, n_nodes) == (len(cell_ids), len(node_ids)), label
    assert np.array_equal(got_cells, cell_ids), label
    assert np.array_equal(got_nodes, node_ids), label
    assert np.array_equal(got_connectivity, connectivity), label
    return F, cell_ids, node_ids


@pytest.mark.parametrize("name", sorted(MESHES))
def test_selection_equals_the_numpy_restatement(mesh_modules, name):
    off, cells, m = mesh_modules(name)
    counts = {}
    for case, manifolds in _cases(off).items():
        F, cell_ids, node_ids = _check_selection(m, off, cells, manifolds, f"{name} {case}")
        counts[case] = len(cell_ids)
        if case == "node exact":
            assert (F[0][cells] == 0.0).any(), "the plane goes through vertices"
    assert counts["misses"] == 0 and counts["all"] == len(cells)
    assert 0 < counts["cut"] < len(cells) and counts["two manifolds"] == counts["cut"]
    assert counts["two that cut"] > counts["cut"] and counts["node exact"] > 0
    if name == "big_257x256":
        assert len(cells) > BLOCK * BLOCK   # more block counts than one round of the scan takes
    if name in ("lattice_33x31", "lattice_9x10x11", "big_257x256"):
        # the cut crosses block boundaries: selected cells in more than one block of BLOCK cells
        assert len(set(hv.select(cells, hv.levelsets(_cases(off)["cut"], off.dim, off.positions))[0] // BLOCK)) > 1


def test_selection_with_library_functions(mesh_modules):
    """sqrt and sin differ between device and host by their few ulp; the manifold is chosen so that no vertex value
    lies near +-100 eps (asserted on the HOST values alone, before anything is compared): then no cell is excused"""
    off, cells, m = mesh_modules("lattice_33x31")
    manifolds = ["sqrt(x*x + y*y) - 0.8 + 0.05*sin(3*x)"]
    F = hv.levelsets(manifolds, off.dim, off.positions)
    assert hv.margin_to_thresholds(F, cells) > 1e-12
    _, cell_ids, _ = _check_selection(m, off, cells, manifolds, "library functions")
    assert 0 < len(cell_ids) < len(cells)
    device = m.output_levelset_values(0)
    print(f"library functions: device against host, max difference {np.abs(device - F[0]).max():.3e}")


# ------------------------------------------------------------------------------------------------ C. extract

def _develop(m, U0, dirichlet, n_updates):
    a, b = m.new_state_vector(U0), m.new_state_vector()
    for _ in range(n_updates):
        m.prepare_state_vector(a, 0.0, dirichlet)
        m.step(a, [], [], b)
        a, b = b, a
    m.prepare_state_vector(a, 0.0, dirichlet)   # the precomputed values of the vector that is written out
    return a


def _euler_like(equation, **edits):
    off = offline.SyntheticOffline(offline.mach3_step_2d(20))
    U0 = euler_uniform(off.positions)
    U0 *= 1.0 + 1e-3 * np.sin(7.0 * off.positions[:, :1] + 3.0 * off.positions[:, 1:2])
    return off, _params(equation, 2, **edits), U0, euler_uniform(off.b_positions), ("rho", "E"), ("v_1",)


def _shallow_water():
    off = offline.SyntheticOffline(offline.rectangle_2d(24, (-5.0, -5.0), (5.0, 5.0)))
    x = off.positions
    off.set_initial_precomputed(0.05 * np.sin(0.6 * x[:, 0]) * np.cos(0.4 * x[:, 1]))
    U0 = sw_circular_dam_break(x)
    dry = x[:, 0] > 3.0
    U0[dry] = 0.0
    U0[dry & (x[:, 1] > 0.0), 1] = 1.0e-18   # a residual momentum on a dry node
    return off, _params(capi.EQ_SHALLOW_WATER, 2), U0, None, ("h",), ("v_1",)


def _scalar():
    off = offline.SyntheticOffline(offline.rectangle_2d(24, (-2.0, -2.5), (2.0, 1.5), bc=capi.BC_DIRICHLET))
    r = np.linalg.norm(off.positions, axis=1)
    U0 = np.where(r < 1.0, 1.0, -0.5).reshape(-1, 1)
    return off, _params(capi.EQ_SCALAR_CONSERVATION, 2), U0, U0[off.b_i], ("u",), ()


DESCRIPTIONS = {
    "euler": lambda: _euler_like(capi.EQ_EULER),
    "euler_aeos": lambda: _euler_like(capi.EQ_EULER_AEOS),
    "euler_aeos_nasg": lambda: _euler_like(capi.EQ_EULER_AEOS, eos=capi.EOS_NOBLE_ABEL_STIFFENED_GAS,
                                           eos_covolume_b=0.05, eos_pinf=0.5, eos_q=0.1),
    "shallow_water": _shallow_water,
    "scalar_conservation": _scalar,
}


def _all_names(equation, dim, pp_names):
    tables = capi.output_names(equation, dim)
    names = [*tables["conserved"], *tables["primitive"], *tables["precomputed"], *tables["initial_precomputed"],
             "alpha", *pp_names]
    return names[::-1]   # (not in the order of the arrays)


@pytest.fixture(scope="module")
def developed():
    """name -> (off, module, state, names, expected Float64 [n_quantities, n_relevant], tolerance): a developed state
    of every Description, with everything extract() reads downloaded through the module's own calls"""
    built = {}

    def get(name):
        if name not in built:
            off, params, U0, dirichlet, schlieren, vorticity = DESCRIPTIONS[name]()
            m = HyperbolicModule(off, params, backend="hip")
            state = _develop(m, U0, dirichlet, 4)
            pp_names = m.postprocess_configure(schlieren, vorticity)
            names = _all_names(m.equation, off.dim, pp_names)
            m.output_configure(names, off.cells, ["x*x + y*y - 1.5", "y - 0.3*x"])
            m.postprocess_compute(state)
            U = state.download()
            assert np.isfinite(U).all()
            Z = capi.np_from_ptr(off.c.contents.initial_precomputed, off.n_relevant, np.float64) \
                if m.equation == capi.EQ_SHALLOW_WATER else None
            expected, tol = hv.extract(m.equation, off.dim, m.params, names, U, state.download_precomputed(), Z,
                                       m.alpha(), m.postprocess_download())
            built[name] = (off, m, state, names, expected, tol)
        return built[name]
    yield get
    for entry in built.values():
        entry[1].close()


@pytest.mark.parametrize("name", sorted(DESCRIPTIONS))
def test_extract_float64_against_the_modules_own_downloads(developed, name):
    off, m, state, names, expected, tol = developed(name)
    got = m.output_extract(state, levelsets=False, precision="float64")
    assert got.shape == (len(names), off.n_relevant) and got.dtype == np.float64
    hv.compare(name, names, got, expected, tol)
    assert np.array_equal(got, m.output_extract(state, levelsets=False, precision="float64"), equal_nan=True)
    if name == "shallow_water":
        assert (expected[names.index("h")] == 0.0).any() and (expected[names.index("bathymetry")] != 0.0).any()
    assert np.abs(expected[names.index("alpha")]).max() > 0.0


@pytest.mark.parametrize("name", sorted(DESCRIPTIONS))
def test_level_set_output_is_the_full_output_at_node_ids(developed, name):
    off, m, state, names, expected, tol = developed(name)
    cell_ids, node_ids, connectivity = m.output_selection()
    ref = hv.select(off.cells, hv.levelsets(["x*x + y*y - 1.5", "y - 0.3*x"], off.dim, off.positions))
    assert np.array_equal(cell_ids, ref[0]) and np.array_equal(node_ids, ref[1]) and np.array_equal(connectivity, ref[2])
    assert 0 < len(node_ids) < off.n_relevant
    for precision in ("float64", "float32"):
        full = m.output_extract(state, levelsets=False, precision=precision)
        cut = m.output_extract(state, levelsets=True, precision=precision)
        assert cut.shape == (len(names), len(node_ids))
        assert np.array_equal(cut, full[:, node_ids], equal_nan=True)


@pytest.mark.parametrize("name", sorted(DESCRIPTIONS))
def test_extract_float32_is_the_conversion_of_float64(developed, name):
    off, m, state, names, expected, tol = developed(name)
    single = m.output_extract(state, precision="float32")
    double = m.output_extract(state, precision="float64")
    assert single.dtype == np.float32
    assert single.tobytes() == double.astype(np.float32).tobytes()


def test_float32_beyond_its_range_and_denormals():
    off = _lattice(2, (7, 5))
    m = HyperbolicModule(off, _params(capi.EQ_EULER, 2), backend="hip")
    rng = np.random.default_rng(3)
    U = rng.normal(size=(off.n_relevant, 4))
    U[0] = [1e300, -1e39, 3.5e38, -3.5e38]                     # beyond FLT_MAX = 3.4e38: +-inf
    U[1] = [1e-40, -1e-44, 7e-46, -1e-50]                      # Float32 denormals, and below the smallest one
    U[2] = [np.finfo(np.float32).max, float(np.finfo(np.float32).tiny), -0.0, 2.0 ** -149]
    U[3] = [np.nextafter(2.0 ** -126, 0.0), 2.0 ** -150, 1.5 * 2.0 ** -149, 16777217.0]   # ties, and a rounding case
    state = m.new_state_vector(U)
    names = ["rho", "m_1", "m_2", "E"]
    m.output_configure(names, off.cells)
    double = m.output_extract(state, precision="float64")
    single = m.output_extract(state, precision="float32")
    assert np.array_equal(double, U.T)
    with np.errstate(over="ignore", under="ignore"):
        converted = double.astype(np.float32)
    assert single.tobytes() == converted.tobytes()
    assert np.isinf(single[:, 0]).all() and (single[0, 1] != 0.0) and (0.0 < abs(single[0, 1]) < np.finfo(np.float32).tiny)
    assert single[3, 1] == 0.0 and np.signbit(single[3, 1])
    m.close()


# ------------------------------------------------------------------------------------------------ D. ranks

def _annulus():
    points, quads, edges = hq1.annulus_mesh(6, 24)
    off, info = hq1.q1_quads_offline(points, quads, edges)
    return points, hen.lexicographic_quads(quads), off, info


def _cells_of_rank(view, cells_global, owner):
    """the cells of a rank: those whose vertex of smallest global id it owns; local indices, and their global ids"""
    local = np.full(len(owner), -1, dtype=np.int64)
    local[view.global_ids] = np.arange(len(view.global_ids))
    mine = np.flatnonzero(owner[cells_global.min(axis=1)] == view.rank)
    cells = local[cells_global[mine]]
    assert (cells >= 0).all(), "every vertex of an owned cell is locally relevant"
    return cells.astype(np.uint32), mine


def _rank_state(points):
    x, y = points[:, 0], points[:, 1]
    rho = 1.4 + 0.2 * np.sin(2.0 * x + y)
    u, v = 0.3 * np.cos(3.0 * y), 0.2 * np.sin(2.0 * x)
    p = 1.0 + 0.1 * np.cos(x - 2.0 * y)
    return np.stack([rho, rho * u, rho * v, p / 0.4 + 0.5 * rho * (u * u + v * v)], axis=1)


RANK_NAMES = ["rho", "m_2", "v_1", "p", "s", "alpha", "schlieren_rho", "vorticity_v_1"]
EXCHANGED = [n for n in RANK_NAMES if n != "s"]   # the precomputed values of a ghost row are the rank's own


def _run_ranks(owner, manifolds):
    from helpers_unstructured import partition
    points, cells_global, off, info = _annulus()
    views = partition(off, info, owner)
    for r, v in enumerate(views):
        v.rank = r
    rank_cells = [_cells_of_rank(v, cells_global, owner) for v in views]
    params = _params(capi.EQ_EULER, 2)

    def body(m, part, r):
        U = _rank_state(part.positions)
        U[part.n_owned:] = 0.0   # the ghost range is NOT current: extract has to exchange it
        a, b = m.new_state_vector(U), m.new_state_vector()
        m.prepare_state_vector(a, 0.0)
        m.step(a, [], [], b)
        m.prepare_state_vector(b, 0.0)
        m.postprocess_configure(("rho",), ("v_1",))
        counts = m.output_configure(RANK_NAMES, rank_cells[r][0], manifolds, part.positions)
        m.postprocess_compute(b)
        selection = m.output_selection()
        full = m.output_extract(b, levelsets=False, precision="float64")
        cut = m.output_extract(b, levelsets=True, precision="float64")
        return dict(counts=counts, selection=selection, full=full, cut=cut, prec=b.download_precomputed())

    ranks = run_hip_ranks(views, lambda: _copy_params(params), body)
    # the single-rank selection
    F = hv.levelsets(manifolds, 2, points)
    single_cells, _, _ = hv.select(cells_global, F)
    union = np.concatenate([rank_cells[r][1][ranks[r]["selection"][0]] for r in range(len(views))])
    assert len(union) == len(set(union.tolist())), "every cell is on exactly one rank"
    assert np.array_equal(np.sort(union), single_cells)
    # ghost-node values are the owner's, bit for bit
    owned = {}
    for r, v in enumerate(views):
        for q, name in enumerate(RANK_NAMES):
            owned.setdefault(name, np.full(len(points), np.nan))[v.global_ids[: v.n_owned]] = ranks[r]["full"][q, : v.n_owned]
    n_ghost_checked = 0
    for r, v in enumerate(views):
        out = ranks[r]
        assert np.array_equal(out["full"][RANK_NAMES.index("s")], out["prec"][:, 0])
        for name in EXCHANGED:
            q = RANK_NAMES.index(name)
            assert np.isfinite(owned[name]).all()
            assert np.array_equal(out["full"][q], owned[name][v.global_ids]), (r, name)
        n_ghost_checked += v.n_relevant - v.n_owned
        cell_ids, node_ids, connectivity = out["selection"]
        local = hv.select(rank_cells[r][0], F[:, v.global_ids])
        assert np.array_equal(cell_ids, local[0]) and np.array_equal(node_ids, local[1])
        assert np.array_equal(connectivity, local[2])
        assert np.array_equal(out["cut"], out["full"][:, node_ids])
    assert n_ghost_checked > 0
    assert np.abs(owned["alpha"]).max() > 0.0 and np.abs(owned["schlieren_rho"]).max() > 0.0
    return views, ranks


def test_three_ranks_one_of_which_selects_nothing():
    points, _, _, _ = _annulus()
    angle = np.arctan2(points[:, 1], points[:, 0])
    owner = np.where(np.abs(angle) > 2.0 * np.pi / 3.0, 0, np.where(angle >= 0.0, 1, 2))   # rank 0: around x < 0
    views, ranks = _run_ranks(owner, ["x - 0.7"])
    counts = [r["counts"][0] for r in ranks]
    assert counts[0] == 0 and counts[1] > 0 and counts[2] > 0, counts
    assert ranks[0]["cut"].shape == (len(RANK_NAMES), 0)


def test_two_by_two_partition_where_selected_cells_reach_ghost_nodes():
    points, _, _, _ = _annulus()
    owner = (points[:, 0] > 0.0).astype(np.int64) + 2 * (points[:, 1] > 0.0).astype(np.int64)
    views, ranks = _run_ranks(owner, ["y - 0.05*x - 0.01", "x + 0.02"])
    reached = 0
    for v, out in zip(views, ranks):
        assert out["counts"][0] > 0
        reached += int((out["selection"][1] >= v.n_owned).sum())
    assert reached > 0, "selected nodes in the ghost range"


# ------------------------------------------------------------------------------------------------ E. life cycle

def test_refusals_and_reconfiguration():
    off = _lattice(2, (7, 5))
    m = HyperbolicModule(off, _params(capi.EQ_EULER, 2), backend="hip")
    lib, ctx = capi.load_hip(), m._ctx
    state = m.new_state_vector(euler_uniform(off.positions))
    cells = np.ascontiguousarray(off.cells, dtype=np.uint32)
    pos = np.ascontiguousarray(off.positions, dtype=np.float64)
    n_nodes = off.n_relevant
    out = np.zeros((8, n_nodes))

    def refused(rc, *words, status=capi.RYUJIN_ERR_ARG):
        assert rc == status, (rc, lib.ryujin_hip_last_error().decode())
        message = lib.ryujin_hip_last_error().decode()
        assert message and all(w in message for w in words), message

    def configure(names=("rho", "p"), manifolds=("x - 0.9",), cells=cells, n_cells=len(cells), dofs=4, positions=pos,
                  n_names=None, n_manifolds=None):
        c_names = (C.c_char_p * max(1, len(names)))(*[n.encode() for n in names]) if names is not None else None
        c_man = (C.c_char_p * max(1, len(manifolds)))(*[x.encode() for x in manifolds]) if manifolds is not None else None
        return lib.ryujin_hip_output_configure(
            ctx, len(names) if n_names is None else n_names, c_names,
            capi.as_ptr(positions, capi.c_double_p) if positions is not None else None, n_cells, dofs,
            capi.as_ptr(cells, capi.c_u32_p) if cells is not None else None,
            len(manifolds) if n_manifolds is None else n_manifolds, c_man)

    def extract(handle=None, levelsets=0, precision=capi.OUT_FLOAT64, out=out):
        return lib.ryujin_hip_output_extract(ctx, state.handle if handle is None else handle, levelsets, precision,
                                             out.ctypes.data_as(C.c_void_p) if out is not None else None)

    # before configure
    refused(extract(), "before output_configure")
    refused(lib.ryujin_hip_output_info(ctx, None, None), "before output_configure")
    refused(lib.ryujin_hip_output_selection(ctx, None, None, None), "before output_configure")
    # names
    refused(configure(names=("rho", "pressure")), "Invalid component name: \"pressure\" is not a valid "
            "conserved/primitive/precomputed/initial component name.")
    refused(configure(names=("bathymetry",)), "bathymetry")         # Euler has no initial precomputed values
    refused(configure(names=("schlieren_rho",)), "schlieren_rho")   # no postprocessor configured
    refused(configure(names=()), "n_quantities")
    refused(configure(names=("rho",) * 33), "n_quantities")
    refused(configure(names=None, n_names=1), "n_quantities")
    # manifolds: the index and the character position; t is unknown here
    refused(configure(manifolds=("x - 0.9", "x + t")), "manifold 1", "character 4")
    refused(configure(manifolds=("x - 0.9", "x +* y")), "manifold 1", "character")
    refused(configure(manifolds=("z - 1",)), "manifold 0", "dimension 2")
    refused(configure(manifolds=("rand(x)",)), "manifold 0", status=capi.RYUJIN_ERR_UNSUPPORTED)
    refused(configure(manifolds=("x",) * 9), "n_manifolds")
    refused(configure(manifolds=None, n_manifolds=1), "n_manifolds")
    # cells
    bad = cells.copy()
    bad[3, 2] = n_nodes
    refused(configure(cells=bad), "index", str(n_nodes))
    refused(configure(cells=None), "null")
    refused(configure(positions=None), "null")
    refused(configure(dofs=9, cells=np.zeros((len(cells), 9), dtype=np.uint32)), "dofs_per_cell",
            status=capi.RYUJIN_ERR_UNSUPPORTED)
    refused(extract(), "before output_configure")   # nothing of the above configured anything
    # the full output only: no manifold, level sets refused; zero cells are legal
    assert configure(manifolds=(), cells=None, n_cells=0) == capi.RYUJIN_OK
    refused(extract(levelsets=1), "without a manifold")
    assert extract() == capi.RYUJIN_OK and np.array_equal(out[0], euler_uniform(off.positions)[:, 0])
    refused(extract(out=None), "null")
    refused(extract(precision=2), "precision")
    refused(extract(handle=99), "handle")
    # a manifold that misses the mesh: counts of 0, an empty level-set output
    assert configure(manifolds=("x + 100",)) == capi.RYUJIN_OK
    assert m.output_info() == (0, 0)
    assert extract(levelsets=1, out=None) == capi.RYUJIN_OK
    # a configuration that works; a refused one leaves it in place; another one replaces it
    assert configure() == capi.RYUJIN_OK
    m._out_names, m._out_dofs_per_cell = ["rho", "p"], 4
    first = (m.output_info(), m.output_selection(), m.output_extract(state, True, "float64"))
    assert first[0][0] > 0
    refused(configure(names=("rho", "nothing")), "nothing")
    refused(configure(manifolds=("x - ",)), "manifold 0")
    again = (m.output_info(), m.output_selection(), m.output_extract(state, True, "float64"))
    assert again[0] == first[0] and all(np.array_equal(a, b) for a, b in zip(again[1], first[1]))
    assert np.array_equal(again[2], first[2])
    assert configure(manifolds=("y + 0.4",)) == capi.RYUJIN_OK
    other = m.output_selection()
    ref = hv.select(cells, hv.levelsets(["y + 0.4"], 2, pos))
    assert all(np.array_equal(a, b) for a, b in zip(other, ref)) and not np.array_equal(other[0], first[1][0])
    # precomputed names: a vector no prepare_state_vector ever ran on is refused
    assert configure(names=("s", "rho")) == capi.RYUJIN_OK
    fresh = m.new_state_vector(euler_uniform(off.positions))
    refused(extract(handle=fresh.handle), "prepare_state_vector")
    m.prepare_state_vector(fresh, 0.0)
    assert extract(handle=fresh.handle) == capi.RYUJIN_OK
    assert np.array_equal(out[0], fresh.download_precomputed()[:, 0])
    # postprocessed names: need a compute since the configure, and the configuration output_configure saw
    m.postprocess_configure(("rho",), ())
    assert configure(names=("schlieren_rho",)) == capi.RYUJIN_OK
    refused(extract(), "postprocess_compute")
    m.postprocess_compute(state)
    assert extract() == capi.RYUJIN_OK and np.array_equal(out[0], m.postprocess_download()["schlieren_rho"])
    m.postprocess_configure(("p",), ())
    m.postprocess_compute(state)
    refused(extract(), "configured anew")
    assert lib.ryujin_hip_output_extract(None, 0, 0, 0, None) == capi.RYUJIN_ERR_ARG
    m.close()


def test_extract_right_after_time_step_iv():
    from ryujin_amd.module import DeviceResidentTimeIntegrator
    off = offline.SyntheticOffline(offline.rectangle_2d(16, (-5.0, -5.0), (5.0, 5.0), bc=capi.BC_DIRICHLET))
    m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip")
    m.initial_values_configure("isentropic vortex", mach_number=1.0, beta=5.0)
    names = ["rho", "v_1", "v_2", "p", "alpha"]
    m.output_configure(names, off.cells, ["x*x + y*y - 4"])
    sv = m.new_state_vector()
    m.initial_values_interpolate(sv, 0.0)
    ti = DeviceResidentTimeIntegrator(m, "erk 33", cfl_min=0.2, cfl_max=0.2, cfl_recovery_strategy="none",
                                      dirichlet="device")
    t = 0.0
    for _ in range(3):
        sv, tau = ti.step(sv, t)
        t += tau
    got = m.output_extract(sv, levelsets=False, precision="float64")
    expected, tol = hv.extract(m.equation, 2, m.params, names, sv.download(), alpha=m.alpha())
    hv.compare("after time_step_iv", names, got, expected, tol)
    _, node_ids, _ = m.output_selection()
    assert np.array_equal(m.output_extract(sv, True, "float64"), got[:, node_ids]) and len(node_ids) > 0
    m.close()


# ------------------------------------------------------------------------------------------------ F. end to end

def test_schedule_output_writes_both_files(tmp_path, developed):
    from test_vtu_writer_cpu import read
    off, m, state, _, _, _ = developed("euler")
    m.postprocess_configure(("rho",), ())
    names = ["rho", "m_1", "p", "alpha", "schlieren_rho"]
    writer = VTUOutput(m, names, manifolds=["x - 1.1", "y - 0.5"], directory=str(tmp_path))
    m.postprocess_compute(state)
    written = writer.schedule_output(state, "solution", 0.25, 123, output_full=True, output_levelsets=True)
    assert [p.split("/")[-1] for p in written] == ["solution_000123.vtu", "solution-levelsets_000123.vtu"]
    full = m.output_extract(state, levelsets=False, precision="float32")
    cut = m.output_extract(state, levelsets=True, precision="float32")
    cell_ids, node_ids, connectivity = m.output_selection()
    assert 0 < len(cell_ids) < len(off.cells)
    for path, values, points, cells in ((written[0], full, off.positions, off.cells),
                                        (written[1], cut, off.positions[node_ids], connectivity)):
        got = read(path)
        assert got["n_points"] == len(points) and got["n_cells"] == len(cells)
        assert list(got["point_data"]) == names
        for q, name in enumerate(names):
            assert got["point_data"][name].tobytes() == values[q].tobytes()
        assert np.array_equal(got["points"][:, :2], points.astype(np.float32)) and (got["points"][:, 2] == 0).all()
        assert np.array_equal(got["connectivity"].reshape(-1, 4), np.asarray(cells)[:, [0, 1, 3, 2]])
        assert float(got["field"]["TIME"]) == 0.25 and int(got["field"]["CYCLE"]) == 123
    # without manifolds the level-set file is not written (vtu_output.template.h:156)
    plain = VTUOutput(m, ["rho"], directory=str(tmp_path))
    assert [p.split("/")[-1] for p in plain.schedule_output(state, "plain", 0.0, 0, True, True)] == ["plain_000000.vtu"]
    # restore what the other tests of this module configured on the shared module
    off, m, state, names, _, _ = developed("euler")
    m.postprocess_configure(("rho", "E"), ("v_1",))
    m.output_configure(names, off.cells, ["x*x + y*y - 1.5", "y - 0.3*x"])
    m.postprocess_compute(state)
