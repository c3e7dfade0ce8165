"""The case table of tests/test_gpu_postprocessor_meshes.py: the postprocessor sweep (k_postprocess_sweep) on every mesh
family the update is tested on. The sweep takes its rows from row_context(), its columns from tile_column(), pre-loads
column c + 1 inside the slice's width and masks with the row's own length, clamps rows beyond n_owned and folds the
bounds per wave: all of it depends on the mesh, none of it on the flow. Families:

  A  at and below one 64-row slice                 helpers_small_meshes.CASES
  B  the layout switches the sweep reads           helpers_small_meshes.LAYOUT_SWITCH_CASES and three larger, bit for bit
  C  prescribed widest rows, 4 ... 1023 entries    helpers_row_width_cases.CASES (narrow rows padded next to full ones)
  D  periodic Q2 lattices                          helpers_q2 (rows of 9 | 15 | 25, and 27 ... 125 entries)
  E  Delaunay P1 triangles and tetrahedra          helpers_unstructured.p1_offline (irregular tiles, ragged rows)
  F  partitions                                    helpers_unstructured.partition by sectors; x-slabs of 16 rows
  G  rows of length 1 (constrained DoFs)           a lattice and the P1 disk with a handful of rows cut to the diagonal

An entry holds the mesh recipe, the Description and, as literals, n_owned, the widest row and the number of slices;
tests/test_postprocessor_cases_cpu.py pins the literals against the mesh and asserts on the numpy field of every
requested quantity that the case is not vacuous. Nothing here needs a GPU.

The data of every case is helpers_small_meshes.state() on the bounding box of the mesh: a jump under a smooth wave, so
that every row has a value of its own. No update is run: the sweep does not care whether the flow is developed. (Shallow
water: state() moves the water at 0.1 everywhere -- a primitive velocity without a gradient --, the velocity here
follows the wave; EulerAEOS: the pressure follows the square of the wave, so that e varies.)

G. The library's layout (host_layout.hpp) refuses a pattern that is not structurally symmetric: a row cut down to its
diagonal leaves its neighbours' rows as well -- cut_rows() --, the one-sided cut is kept as what create() must go on
refusing -- cut_rows(one_sided=True)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import helpers_postprocessor as hp
import helpers_small_meshes as sm
from helpers_layout import OfflineView
from ryujin_amd import capi, offline

EQUATIONS = sm.EQUATIONS


# ------------------------------------------------------------------ parameters, quantities, data

def params(equation: str, dim: int, **edits):
    p = capi.Params()
    capi.load_hip().ryujin_hip_default_params(C.byref(p), EQUATIONS[equation], dim)
    p.cfl = 0.9
    if equation == "euler_aeos":
        sm._aeos_edit(p)
    for name, value in edits.items():
        setattr(p, name, value)
    return p


def quantities(equation: str, dim: int):
    """(schlieren names, vorticity names): a conserved and a primitive component each, in ONE call, so that load_mask
    has several bits"""
    if equation in ("euler", "euler_aeos"):
        schlieren = ("rho", "p" if equation == "euler" else "e")
        return schlieren, (("m_1", "v_1") if dim >= 2 else ())
    if equation == "shallow_water":
        return ("h", "v_1" if dim >= 2 else "v"), ()
    return ("u",), ()


class Box:
    """what helpers_small_meshes.profile() reads of a MeshSpec"""

    def __init__(self, lower, upper):
        self.dim, self.lower, self.upper = len(lower), tuple(lower), tuple(upper)


def box_of(off):
    x = np.asarray(off.positions).reshape(-1, off.dim)
    return Box(x.min(axis=0), x.max(axis=0))


def state(equation: str, box, x, p=None):
    x = np.asarray(x).reshape(-1, box.dim)
    U = sm.state(equation, box, x, p)
    left, w = sm.profile(box, x)
    if equation == "euler_aeos":   # (density and pressure of state() follow the same wave: e = p / ((gamma - 1) rho)
        from ryujin_amd.initial_states import aeos_from_primitive   # would be constant on either side of the jump)
        v = np.zeros((len(w), box.dim))
        v[:, 0] = 0.3 * w
        U = aeos_from_primitive(p, np.where(left, 1.0, 0.125) * w, v, np.where(left, 1.0, 0.1) * w * w)
    if equation == "shallow_water":
        U[:, 1] = U[:, 0] * 0.3 * (w - 0.9)
        if box.dim > 1:
            U[:, 2] = U[:, 0] * 0.2 * (1.1 - w)
    return U


def dry_patch(U, x):
    """as test_shallow_water_with_dry_nodes: h = 0 beyond x = 0.4, without and (upper half) with a residual momentum"""
    dry = x[:, 0] > 0.4
    U[dry, :] = 0.0
    U[dry & (x[:, 1] > 0.0), 1] = 1.0e-18
    return U


# ------------------------------------------------------------------ meshes

def _small(name):
    return lambda: sm.CASES[name]["mesh"]()


def _row_width(name):
    import helpers_row_width_cases as rwc
    return lambda: rwc.CASES[name]["mesh"]()


def _q2(dim, n_elements):
    import helpers_q2
    if dim == 2:
        return lambda: helpers_q2.q2_periodic_offline_sparse(2, n_elements)[0]
    return lambda: helpers_q2.q2_periodic_offline(3, n_elements)[0]


BALL = (2500, 900)   # ball_points(...) of test_unstructured_p1_tetrahedra_3d


@functools.lru_cache(maxsize=None)
def p1(which):
    """(offline data, info) of the P1 disk with six rings / the P1 ball; shared, nobody changes the arrays"""
    from helpers_unstructured import ball_points, disk_points, p1_offline
    return p1_offline(disk_points(6)) if which == "disk" else p1_offline(ball_points(*BALL))


def _p1(which):
    return lambda: p1(which)[0]


def cut_rows(off, cut, one_sided=False):
    """the single-rank mesh `off` with the rows `cut` reduced to their diagonal entry: row_starts, columns, c_ij and
    m_ij recomputed, m_i kept, no boundary map. The cut nodes leave the other rows too (the layout wants a symmetric
    pattern); one_sided: they stay there."""
    assert off.n_relevant == off.n_owned
    rows, cols, c, mi, lens = hp.csr(off)
    keep_ = getattr(off, "_keep", None)
    mij = np.asarray(keep_["mij"] if keep_ is not None else off.mij)[: len(rows)]
    n, dim = off.n_owned, off.dim
    gone = np.zeros(n, dtype=bool)
    gone[np.asarray(cut)] = True
    drop = gone[rows] if one_sided else gone[rows] | gone[cols]
    keep = (rows == cols) | ~drop
    widths = np.bincount(rows[keep], minlength=n)
    row_starts = np.concatenate([[0], np.cumsum(widths)]).astype(np.uint64)
    out = OfflineView(dim, 0, 0, n, n, 1, row_starts, cols[keep].astype(np.uint32), c[keep], mij[keep], mi, 1.0 / mi,
                      float(mi.sum()), [], np.zeros((0, dim)), [], [], [], [])
    out.positions = np.asarray(off.positions).reshape(-1, dim)[:n]
    out.cut = np.flatnonzero(gone)
    return out


# rows cut in family G: 63 is the last lane of slice 0 and the only cut row there -- the slice is otherwise full --, 100
# sits in the middle of a slice (full but for it on the lattice, the partial last one on the disk); the last row of the
# mesh ends a partial slice
CUT_LATTICE, CUT_DISK = (63, 100, 130, 143), (63, 100, 126)


def _cut(base, cut):
    return lambda: cut_rows(base(), cut)


# ------------------------------------------------------------------ the table

def _entry(name, family, mesh, equation, n_owned, width, n_slices, **more):
    CASES[name] = dict(name=name, family=family, mesh=mesh, equation=equation, n_owned=n_owned, width=width,
                       n_slices=n_slices, **more)


CASES = {}

# A. (shape, n_owned, widest row, slices): Euler on all, the other Descriptions on 63 cells and 12 x 4
for _shape, _n, _w, _s in (("1d_1", 2, 2, 1), ("1d_2", 3, 3, 1), ("1d_62", 63, 3, 1), ("1d_63", 64, 3, 1),
                           ("1d_64", 65, 3, 2), ("1d_65", 66, 3, 2),
                           ("2d_1x1", 4, 4, 1), ("2d_2x2", 9, 9, 1), ("2d_8x6", 63, 9, 1), ("2d_7x7", 64, 9, 1),
                           ("2d_12x4", 65, 9, 2), ("2d_15x8", 144, 9, 3),
                           ("3d_1x1x1", 8, 8, 1), ("3d_2x2x2", 27, 27, 1), ("3d_6x2x2", 63, 27, 1),
                           ("3d_3x3x3", 64, 27, 1), ("3d_10x2x1", 66, 18, 2)):
    _entry(f"A_euler_{_shape}", "A", _small(f"euler_{_shape}"), "euler", _n, _w, _s)
for _equation in ("euler_aeos", "shallow_water", "scalar"):
    _entry(f"A_{_equation}_1d_63", "A", _small(f"{_equation}_1d_63"), _equation, 64, 3, 1)
    _entry(f"A_{_equation}_2d_12x4", "A", _small(f"{_equation}_2d_12x4"), _equation, 65, 9, 2)

# the single-cell meshes: every row sees the whole mesh, a linear field has ONE gradient -- q_max == q_min to round-off
# and the normalised field is what numpy gives for it. Exempt from the vacuity rule BY NAME.
SINGLE_CELL = ("A_euler_1d_1", "A_euler_2d_1x1", "A_euler_3d_1x1x1")

# C. the recipes of helpers_row_width_cases at widths 4, 10, 28, 33, 64, 65, 127, 128 and 1023: LINE (640 rows), PLANE
# (960), PLANE_1023 (1600) and BOX (1024)
for _case, _n, _w, _s in (("euler_1d_4", 640, 4, 10), ("euler_2d_10", 960, 10, 15), ("euler_3d_28", 1024, 28, 16),
                          ("euler_2d_33", 960, 33, 15), ("euler_2d_64", 960, 64, 15), ("euler_1d_65", 640, 65, 10),
                          ("euler_2d_127", 960, 127, 15), ("euler_3d_128", 1024, 128, 16),
                          ("euler_2d_1023", 1600, 1023, 25)):
    _entry(f"C_{_case}", "C", _row_width(_case), "euler", _n, _w, _s)
_entry("C_sw_2d_10", "C", _row_width("sw_2d_10"), "shallow_water", 960, 10, 15)

# D. Q2: five elements per direction is the smallest 2-D lattice with more than one slice (100 rows of 9, 15 and 25
# entries; four elements give exactly 64); three per direction in 3-D (216 rows of 27 ... 125 entries)
_entry("D_q2_2d_5", "D", _q2(2, 5), "euler", 100, 25, 2, widths=(9, 15, 25))
_entry("D_q2_3d_3", "D", _q2(3, 3), "euler", 216, 125, 4, widths=(27, 45, 75, 125))

# E. P1: the disk with six rings (127 nodes: the second slice is partial), the ball; shallow water with a dry patch
_entry("E_disk_euler", "E", _p1("disk"), "euler", 127, 8, 2)
_entry("E_disk_sw_dry", "E", _p1("disk"), "shallow_water", 127, 8, 2, dry=True)
_entry("E_ball_euler", "E", _p1("ball"), "euler", 3401, 28, 54)

# G. rows of length 1
_entry("G_lattice_15x8", "G", _cut(_small("euler_2d_15x8"), CUT_LATTICE), "euler", 144, 9, 3, cut=CUT_LATTICE)
_entry("G_disk", "G", _cut(_p1("disk"), CUT_DISK), "euler", 127, 8, 2, cut=CUT_DISK)

del _shape, _n, _w, _s, _equation, _case

# B. the layout switches the postprocessor reads, on helpers_small_meshes.LAYOUT_SWITCH_CASES (the meshes of family A)
LAYOUT_SWITCHES = (dict(debug_tile_map=-1), dict(debug_band_stride=2), dict(debug_band_stride=5),
                   dict(debug_xcd_chunk=1), dict(debug_xcd_chunk=5))
assert all(s in sm.LAYOUT_SWITCHES for s in LAYOUT_SWITCHES)
# ... and on three cases of this table with enough slices for a renumbering to act: 15 slices hold one band of stride 2
# and a remainder; the 54 slices of the ball (14 blocks) hold whole bands of both strides and a whole chunk span of 8
# blocks, each with a partial tail; the disk has irregular tiles for debug_tile_map to switch off
LAYOUT_SWITCH_CASES = sm.LAYOUT_SWITCH_CASES + ("C_euler_2d_10", "E_disk_euler", "E_ball_euler")

# F. (n_ranks, per rank n_owned, the largest number of neighbours of a rank)
RANK_CASES = {"F_disk_sectors": (5, (23, 29, 31, 24, 20), 4), "F_plane_7x7_of_4": (4, (16, 16, 16, 16), 2)}


@functools.lru_cache(maxsize=None)
def mesh(name):
    """the offline data of a case; built once and shared by every test of the case -- nobody changes the arrays"""
    return CASES[name]["mesh"]()


def case_state(name, p=None):
    """the state [n_relevant, k] of a single-rank case"""
    case, off = CASES[name], mesh(name)
    x = np.asarray(off.positions).reshape(-1, off.dim)
    U = state(case["equation"], box_of(off), x, p if p is not None else params(case["equation"], off.dim))
    return dry_patch(U, x) if case.get("dry") else U


def rank_case(name):
    """(single-rank offline data, parts, the box of the whole mesh) of a family-F case"""
    if name == "F_disk_sectors":
        from helpers_unstructured import partition
        from test_oracle_unstructured import sector_owner
        off, info = p1("disk")
        return off, partition(off, info, sector_owner(off.positions, RANK_CASES[name][0])), box_of(off)
    _, parts = sm.rank_parts("plane_7x7_of_4")
    single = offline.SyntheticOffline(sm.rectangle(7, 7))
    return single, parts, box_of(single)


def global_rows(single, part):
    """the rows of the single-rank mesh that a rank owns, in the rank's order"""
    ids = getattr(single, "global_ids", None)
    if ids is None:   # (a numpy-backed view is numbered 0 ... n - 1)
        return np.asarray(part.global_ids[: part.n_owned], dtype=np.int64)
    lookup = {int(g): i for i, g in enumerate(ids)}
    return np.array([lookup[int(g)] for g in part.global_ids[: part.n_owned]], dtype=np.int64)


# ------------------------------------------------------------------ the numpy field of a case

def reference(name, U=None, p=None):
    """(quantities, names, raw, scale, widths) of a single-rank case on numpy"""
    case, off = CASES[name], mesh(name)
    p = p if p is not None else params(case["equation"], off.dim)
    quantities_, names = hp.resolve(EQUATIONS[case["equation"]], off.dim, *quantities(case["equation"], off.dim))
    raw, scale = hp.raw_values(off, case_state(name, p) if U is None else U, quantities_, EQUATIONS[case["equation"]], p)
    return quantities_, names, raw, scale, hp.csr(off)[4]


def interior_rows(info):
    return np.flatnonzero(~info["is_bdry"])


def linear_density_rigid_rotation(x, a, b, omega):
    """Euler state with rho = a . x + b and the velocity of a rigid rotation: omega (-y, x) in 2-D (omega a number),
    omega x x in 3-D (omega a vector). sum_j c_ij q_j = m_i grad q for a linear q at every interior node of a continuous
    P1 mesh: schlieren(rho) = |a|, 2-D vorticity(v) = 2 omega, 3-D |vorticity(v)| = 2 |omega| there."""
    from ryujin_amd.initial_states import euler_from_primitive
    dim = x.shape[1]
    v = omega * np.stack([-x[:, 1], x[:, 0]], axis=1) if dim == 2 else np.cross(np.asarray(omega), x)
    return euler_from_primitive(x @ np.asarray(a) + b, v, np.full(len(x), 2.0))
