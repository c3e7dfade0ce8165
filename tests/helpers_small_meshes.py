"""The case table of tests/test_gpu_small_meshes.py: meshes at and below one 64-row slice, where every kernel of the update
takes a launch shape of its own -- one partial slice, exactly one slice, one slice plus one row, two slices --, rows
narrower than the unrolled width the plan picks from the widest row (2, 4, 8 and 18 entries under k_dij_diag_unrolled<3 |
9 | 27>), ranks with fewer than 64 owned rows, ranks whose every owned row is exported and ranks without a boundary row.

An entry holds, as tests/helpers_plan_cases.py: the mesh recipe, the Description, the number of rows and the widest row
as literals, and per RUN the plan the update must take and what each launch of steps 5 and 6 must have been given, as
literals. tests/test_step_plan.py pins the literals against plan_step() on the CPU, the GPU test asserts them against
HyperbolicModule.last_plan(). Nothing here evaluates a threshold. The two runs of a case:
  run 0   as the mesh selects its kernels: step 5 with four waves per slice (k_lij_stage0<E, 4>) or k_pij_lij, step 6
          with the four waves of a block sharing a slice (up to two dimensions), boundary conditions on the pre-pass
  run 1   the kernels of large meshes (debug_no_small_mesh_split = 1, debug_bc_fold_max_slices = -1): one wave per
          slice, P_ij per tile (up to two dimensions), the tile mask, a boundary launch of its own

The data of every case: s the position scaled to the unit box, a jump across s_x + 0.3 s_y + 0.2 s_z = 0.45 under a
smooth wave w = 1 + 0.05 sin(5 s_x + 3 s_y + 2 s_z); two warm-up updates ON THE ORACLE, the third is compared."""
from __future__ import annotations

import numpy as np

import helpers_plan_cases as plan_cases
from helpers_plan_cases import _aeos_edit, _one, _plan
from ryujin_amd import capi, offline
from ryujin_amd.initial_states import aeos_from_primitive, euler_from_primitive

SLIP, DIRICHLET, DO_NOTHING = capi.BC_SLIP, capi.BC_DIRICHLET, capi.BC_DO_NOTHING
EQUATIONS = {"euler": capi.EQ_EULER, "euler_aeos": capi.EQ_EULER_AEOS, "scalar": capi.EQ_SCALAR_CONSERVATION,
             "shallow_water": capi.EQ_SHALLOW_WATER}
JUMP = 0.45
ALPHA_TOL = 1e-12   # helpers_parity.py: alpha is compared to 1e-12 absolute
RUNS = ("as_selected", "large_mesh_kernels")


# ------------------------------------------------------------------ meshes

def interval(cells, bc, n_ranks=1, rank=0):
    return offline.MeshSpec(1, (cells,), (0.0,), (1.0,), tuple(bc), n_ranks=n_ranks, rank=rank)


def rectangle(nx, ny, bc=SLIP, n_ranks=1, rank=0):
    return offline.rectangle_2d(nx, ny=ny, bc=bc, n_ranks=n_ranks, rank=rank)


def box(nx, ny, nz, n_ranks=1, rank=0):
    if ny == nz:
        return offline.box_3d(ny, nx=nx, n_ranks=n_ranks, rank=rank)
    return offline.MeshSpec(3, (nx, ny, nz), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (SLIP,) * 6, n_ranks=n_ranks, rank=rank)


# ------------------------------------------------------------------ data

def profile(spec, x, jump=JUMP):
    """(left of the jump, the smooth wave) at the positions x [n, dim] of a mesh of `spec`"""
    lower, upper = np.asarray(spec.lower[: spec.dim]), np.asarray(spec.upper[: spec.dim])
    s = np.zeros((len(x), 3))
    s[:, : spec.dim] = (np.asarray(x).reshape(len(x), spec.dim) - lower) / (upper - lower)
    return s[:, 0] + 0.3 * s[:, 1] + 0.2 * s[:, 2] < jump, 1.0 + 0.05 * np.sin(5.0 * s[:, 0] + 3.0 * s[:, 1] + 2.0 * s[:, 2])


def state(equation, spec, x, params=None, jump=JUMP):
    """the conserved state [n, k] at the positions x; `params`: EulerAEOS (the equation of state)"""
    left, w = profile(spec, x, jump)
    n, dim = len(w), spec.dim
    if equation in ("euler", "euler_aeos"):
        rho, p = np.where(left, 1.0, 0.125) * w, np.where(left, 1.0, 0.1) * w
        v = np.zeros((n, dim))
        v[:, 0] = 0.3 * w
        return euler_from_primitive(rho, v, p) if equation == "euler" else aeos_from_primitive(params, rho, v, p)
    if equation == "shallow_water":
        U = np.zeros((n, dim + 1))
        U[:, 0] = np.where(left, 1.0, 0.2) * w
        U[:, 1] = 0.1 * U[:, 0]
        return U
    return (np.where(left, 1.0, 0.2) * w).reshape(-1, 1)


def _data(equation, spec, has_dirichlet):
    def data(off):
        p = None
        if equation == "euler_aeos":
            import oracle_py
            p = oracle_py.default_params(capi.EQ_EULER_AEOS, spec.dim)
            _aeos_edit(p)
        dirichlet = state(equation, spec, off.b_positions, p) if has_dirichlet else None
        return dict(U0=state(equation, spec, off.positions, p), dirichlet=dirichlet)
    return data


# ------------------------------------------------------------------ expected plans (literals)

def _stage0(step2, diag_width, dim, **kw):
    """Euler, EulerAEOS without stage vectors: per run the plan. Run 0: k_lij_stage0<E, 4>, no V_i; run 1: one wave per
    slice -- P_ij per tile and the tiles predicted from the history up to two dimensions, P_ij everywhere in 3-D (the
    first update of a context)"""
    small = _plan(step2, diag_width, "stage0_groups", 4, False, 1, "cached", False, step4_stores_p=False, **kw)
    if dim <= 2:
        large = _plan(step2, diag_width, "stage0_per_tile", 1, True, 3, "cached", True, step4_stores_p=False,
                      tiles_predicted_from_history=True, **kw)
    else:
        large = _plan(step2, diag_width, "stage0_groups", 1, True, 1, "cached", True, step4_stores_p=False, **kw)
    return [small, large]


def _euler(diag_width, dim):
    return _stage0("records", diag_width, dim, fast_riemann=True)


def _aeos(diag_width, dim):
    return _stage0("alpha_then_dij", diag_width, dim, step2_split=True)


def _stored(step2, diag_width, **kw):
    """shallow water, scalar conservation, Euler with stage vectors: step 4 stores P_ij, step 5 is k_pij_lij (V_i); the
    same plan in both runs"""
    return [_plan(step2, diag_width, "pij_lij", 1, True, 1, "cached", True, **kw)] * 2


def _sw(diag_width, dim):
    return _stored("records", diag_width, step4_single_walk=True)


def _scalar(diag_width, dim):
    return _stored("dij_alpha_sc", diag_width, step2_split=True)


def _launches(n_slices, dim, stage0):
    """per run: step 5 with four waves per slice only in k_lij_stage0; step 6 shares slices up to two dimensions; run
    1: one wave per slice everywhere"""
    return [_one(n_slices, 4 if stage0 else 1, dim <= 2), _one(n_slices, 1, False)]


PLANS = {"euler": _euler, "euler_aeos": _aeos, "shallow_water": _sw, "scalar": _scalar}


# ------------------------------------------------------------------ the table

def _entry(name, spec, equation, n_rows, width, diag_width, n_slices, *, dirichlet, alpha_positive=True):
    dim = spec.dim
    case = plan_cases._case(lambda: offline.SyntheticOffline(spec), equation, _data(equation, spec, dirichlet), n_rows,
                            None, {}, warm=2, edit=_aeos_edit if equation == "euler_aeos" else None, cfl=0.9)
    CASES[name] = dict(case, spec=spec, dim=dim, width=width, n_slices=n_slices, alpha_positive=alpha_positive,
                       plans=PLANS[equation](diag_width, dim), tile_mask=[False, dim <= 2],
                       launches=_launches(n_slices, dim, equation in ("euler", "euler_aeos")))


CASES = {}

# 1-D: (cells, rows, widest row, slices); one cell: two rows of two entries under k_dij_diag_unrolled<3>
LINE = ((1, 2, 2, 1), (2, 3, 3, 1), (3, 4, 3, 1), (62, 63, 3, 1), (63, 64, 3, 1), (64, 65, 3, 2), (65, 66, 3, 2),
        (127, 128, 3, 2), (128, 129, 3, 3))
for _cells, _rows, _width, _slices in LINE:
    for _equation in ("euler", "euler_aeos", "scalar", "shallow_water"):
        _bc = (SLIP, SLIP) if _equation == "shallow_water" else (DIRICHLET, DO_NOTHING)
        # (one cell of shallow water between slip walls: the oracle's alpha is 8e-17)
        _entry(f"{_equation}_1d_{_cells}", interval(_cells, _bc), _equation, _rows, _width, 3, _slices,
               dirichlet=_equation != "shallow_water", alpha_positive=(_equation, _cells) != ("shallow_water", 1))

# 2-D: (cells, rows, widest row, slices); one cell: four rows of four entries under the unrolled width 9
PLANE = (((1, 1), 4, 4, 1), ((2, 2), 9, 9, 1), ((8, 6), 63, 9, 1), ((7, 7), 64, 9, 1), ((12, 4), 65, 9, 2),
         ((15, 7), 128, 9, 2), ((15, 8), 144, 9, 3))
for (_nx, _ny), _rows, _width, _slices in PLANE:
    for _equation in ("euler", "euler_aeos", "scalar", "shallow_water"):
        # the single cell between slip walls: every node is a corner and its stencil the whole mesh -- the oracle's
        # alpha is 0 (scalar conservation, Dirichlet data at all four nodes: 0.32)
        _entry(f"{_equation}_2d_{_nx}x{_ny}", rectangle(_nx, _ny, DIRICHLET if _equation == "scalar" else SLIP),
               _equation, _rows, _width, 9, _slices, dirichlet=_equation == "scalar",
               alpha_positive=(_nx, _ny) != (1, 1) or _equation == "scalar")

# 3-D: (cells, rows, widest row, unrolled width, slices); one cell: eight rows of eight entries (width 9); one cell
# thick: rows of at most 18 entries (width 27). The single cell: the oracle's alpha is 3e-16
BOX = (((1, 1, 1), 8, 8, 9, 1), ((2, 2, 2), 27, 27, 27, 1), ((6, 2, 2), 63, 27, 27, 1), ((3, 3, 3), 64, 27, 27, 1),
       ((10, 2, 1), 66, 18, 27, 2), ((7, 3, 3), 128, 27, 27, 2))
for (_nx, _ny, _nz), _rows, _width, _diag, _slices in BOX:
    for _equation in ("euler", "euler_aeos"):
        _entry(f"{_equation}_3d_{_nx}x{_ny}x{_nz}", box(_nx, _ny, _nz), _equation, _rows, _width, _diag, _slices,
               dirichlet=False, alpha_positive=(_nx, _ny, _nz) != (1, 1, 1))

del _cells, _rows, _width, _slices, _equation, _bc, _nx, _ny, _nz, _diag

# the cases that also run the two ERK33 stage updates with stage vectors (step<1>, step<2>: step 4 stores P_ij, step 5
# is k_pij_lij) and one update with debug_expensive_bounds_check on both backends (the plan of run 0, checked)
SUBSET = ("euler_1d_63","euler_2d_7x7", "shallow_water_2d_8x6", "euler_3d_3x3x3")


def stage_plan(name):
    """(plan, launches) of step<1> and step<2> of a SUBSET case, as the mesh selects its kernels"""
    case = CASES[name]
    diag = case["plans"][0]["diag_width"]
    if case["equation"] == "shallow_water":
        plan = _stored("records", diag, step4_single_walk=True, step4_has_stages=True)[0]
    else:
        plan = _stored("records", diag, fast_riemann=True, step4_has_stages=True)[0]
    return plan, _one(case["n_slices"], 1, case["dim"] <= 2)


def checked_plan(name):
    case = CASES[name]
    return dict(case["plans"][0], checked=True), case["launches"][0]


# the meshes of the bit-identity test under the layout switches, and of the device-resident driver and the integrals
LAYOUT_SWITCH_CASES = ("euler_2d_2x2", "euler_2d_7x7", "euler_2d_12x4", "euler_3d_2x2x2", "euler_3d_10x2x1",
                       "shallow_water_2d_8x6")
LAYOUT_SWITCHES = (dict(debug_tile_map=-1), dict(debug_stencil_classes=-1), dict(debug_next_tile_mask=-1),
                   dict(debug_next_tile_mask=1), dict(debug_band_stride=2), dict(debug_band_stride=5),
                   dict(debug_xcd_chunk=1), dict(debug_xcd_chunk=5))
DRIVER_CASES = ("euler_1d_2", "euler_2d_2x2", "euler_2d_7x7", "euler_3d_2x2x2")


# ------------------------------------------------------------------ ranks smaller than a slice, ranks that export everything

def _rank_specs(make, n_ranks):
    return [make(n_ranks, r) for r in range(n_ranks)]


# name -> (dim, recipe(n_ranks, rank), ranks, per rank (n_export, n_owned, n_relevant, n_bdry, neighbours) or None where
# only n_owned is pinned, equations). x-slabs of the generator, which refuses fewer than two node planes per rank.
RANK_CASES = {
    # the middle rank exports both of its rows and has no boundary row
    "line_5_of_3": (1, lambda n, r: interval(5, (SLIP, SLIP), n, r), 3,
                    [(1, 2, 3, 1, 1), (2, 2, 4, 0, 2), (1, 2, 3, 1, 1)], ("euler",)),
    "line_8_of_4": (1, lambda n, r: interval(8, (SLIP, SLIP), n, r), 4, None, ("euler",)),   # two such middle ranks
    "line_130_of_3": (1, lambda n, r: interval(130, (SLIP, SLIP), n, r), 3, None, ("euler",)),   # 43 or 44 rows per rank
    # the two middle ranks export every row
    "plane_7x7_of_4": (2, lambda n, r: rectangle(7, 7, SLIP, n, r), 4,
                       [(8, 16, 24, 12, 1), (16, 16, 32, 4, 2), (16, 16, 32, 4, 2), (8, 16, 24, 12, 1)],
                       ("euler", "shallow_water")),
    "plane_10x10_of_3": (2, lambda n, r: rectangle(10, 10, SLIP, n, r), 3, None, ("euler", "shallow_water")),
    "box_4_of_2": (3, lambda n, r: box(4, 4, 4, n, r), 2, [(25, 50, 75, 65, 1), (25, 75, 100, 85, 1)], ("euler",)),
}
RANK_N_OWNED = {"line_8_of_4": (2, 2, 2, 3), "line_130_of_3": (43, 44, 44), "plane_10x10_of_3": (33, 44, 44)}
RANK_N_EXPORT = {"plane_10x10_of_3": (11, 22, 11)}


def rank_parts(name):
    dim, recipe, n_ranks, counts, _ = RANK_CASES[name]
    specs = _rank_specs(recipe, n_ranks)
    return specs, [offline.SyntheticOffline(s) for s in specs]


def rank_counts(part):
    return (part.n_export, part.n_owned, part.n_relevant, part.n_bdry, int(part.c.contents.n_nbr))


def rank_states(equation, specs, parts, jump=JUMP):
    return [state(equation, s, p.positions, None, jump) for s, p in zip(specs, parts)]


# ------------------------------------------------------------------ running a case

_developed = {}


def developed(name, oracle):
    """(offline data, Dirichlet data, the state after the warm-up ON THE ORACLE) of a case; computed once and shared by
    every test of the case -- nobody changes the arrays"""
    if name not in _developed:
        case = CASES[name]
        off, U0, dirichlet, after_warm = plan_cases.build(case)
        assert off.n_owned == case["n_points"] and int(plan_cases.widths_of(off).max()) == case["width"]
        U_start = plan_cases.warm_up(case, oracle, off, U0, dirichlet, after_warm)
        assert np.isfinite(U_start).all()
        U_start.setflags(write=False)
        _developed[name] = (off, dirichlet, U_start)
    return _developed[name]


def _large_mesh_kernels(p):
    p.debug_no_small_mesh_split = 1
    p.debug_bc_fold_max_slices = -1


def for_run(case, run, more=None):
    """the case with the parameter edits of run 0 / 1 (and `more`, a dict of further parameters)"""
    def edit(p):
        if case["edit"]:
            case["edit"](p)
        if run == 1:
            _large_mesh_kernels(p)
        for key, value in (more or {}).items():
            setattr(p, key, value)
    return dict(case, edit=edit)


def assert_not_vacuous(case, off, c):
    """On the ORACLE's arrays of the compared update (c: alpha, "lij_next" the first pass, "lij" the second). From 63
    rows on: some off-diagonal first-pass l_ij strictly between 0 and 1, some off-diagonal second-pass entry above 0,
    alpha above 0 somewhere. Below 63 rows the case tests addressing: alpha above 0 where the table says the oracle
    shows it, and at round-off where it says that (the single-cell meshes between slip walls)."""
    n = off.n_owned
    widths = plan_cases.widths_of(off)
    rs = np.concatenate([[0], np.cumsum(widths)])
    off_diagonal = np.arange(rs[-1]) - np.repeat(rs[:-1], widths) > 0
    alpha = np.asarray(c["alpha"])[:n]
    # (above 0: above 1e-12, the bound alpha is compared to -- at or below it the comparison of alpha says nothing)
    assert (alpha.max() > ALPHA_TOL) == case["alpha_positive"], float(alpha.max())
    if n >= 63:
        first, second = np.asarray(c["lij_next"])[: rs[-1]], np.asarray(c["lij"])[: rs[-1]]
        n_first = int(((first > 0.0) & (first < 1.0) & off_diagonal).sum())
        n_second = int(((second > 0.0) & off_diagonal).sum())
        assert n_first > 0 and n_second > 0 and case["alpha_positive"], (n_first, n_second)
        return n_first, n_second
    return None
