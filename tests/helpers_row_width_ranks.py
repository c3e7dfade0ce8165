"""The lattices with a prescribed widest row (tests/helpers_row_width.py) ON SEVERAL RANKS: an adapter that lets
helpers_unstructured.partition() take a lattice, the ownership maps, the case table RANK_CASES and what a case must show
before it counts (tests/test_gpu_row_widths_ranks.py: the GPU run; tests/test_row_width_ranks_cpu.py: the partition
contract, the literals, the partitioned against the single-rank oracle and the coverage, on the CPU).

On a rank the widest row meets what no single-rank case has: ghost columns are numbered behind the owned rows, so in a
row sorted by local index they fill its LAST blocks of 63 columns; l_ji of a ghost column is read from a ghost row --
plain CSR behind the SELL region, filled by the pack kernels and the transport --, hundreds of entries long here; and a
sweep is two launches, slices [0, ceil(n_export / 64)) and the rest, the last export slice mixing exported and interior
rows, or ONE launch where a wide stencil makes every owned row an export row.

An entry of RANK_CASES is built on an entry of helpers_row_width_cases.CASES: same data recipe, same warm-up ON THE
SINGLE-RANK ORACLE, same parameter edits. It adds the lattice shape, the ownership map and, as literals per rank,
n_owned, n_export and the launches of steps 5 and 6 in the form of helpers_plan_cases.TWO_RANK_CASE: (slices, gridDim.y
of step 5, step 6 shares) of the export and of the interior part."""
from __future__ import annotations

import numpy as np

import helpers_row_width as rw
import helpers_row_width_cases as cases
from helpers_row_width_cases import BLOCK, CASES


# ------------------------------------------------------------------ the adapter and the ownership maps

def partition_lattice(off, owner):
    """per-rank views of a lattice_offline() lattice through helpers_unstructured.partition: the rows as lists taken
    from the CSR arrays, no boundary, c_ij and m_ij under the names partition() reads, and the bathymetry the data recipe
    left in the offline data (shallow water) passed through to every rank's locally relevant range"""
    from helpers_unstructured import partition
    rs = np.asarray(off.row_starts).astype(np.int64)
    cols = np.asarray(off.columns).astype(np.int64).tolist()
    info = dict(rows=[cols[rs[i]:rs[i + 1]] for i in range(off.n_owned)], is_bdry=np.zeros(off.n_owned, dtype=bool))
    off.cij_csr, off.mij_csr = off.cij, off.mij
    off.row_starts = np.asarray(off.row_starts).astype(np.uint64)
    return partition(off, info, np.asarray(owner, dtype=np.int64), bathymetry=off._keep.get("initial_precomputed"))


def _coordinates(off):
    return rw._unravel(off.lattice_shape, np.arange(off.n_owned))


def slabs(n_ranks):
    """equal cuts of the last (periodic) axis; in 1-D: contiguous parts of the ring"""
    def owner(off):
        return _coordinates(off)[:, -1] * n_ranks // off.lattice_shape[-1]
    return owner


def halves_from(start):
    """1-D: the contiguous half of the ring that begins at node `start`, and the rest. (slabs(2) cuts a ring of whole
    slices between two slices, where no widened row of a ring of at most 64 entries reaches: with `start` inside the
    widened run both cuts pass through rows of the widest width.)"""
    def owner(off):
        n = off.lattice_shape[0]
        return (((np.arange(off.n_owned) - start) % n) >= n // 2).astype(np.int64)
    return owner


def uneven(off):
    """three ranks: cuts at 1/8 and 1/2 of the last axis, one node further wherever the axis-0 index is a multiple of 7
    -- a ragged cut; the small first rank has nothing but export rows, and not a multiple of 64 of them"""
    ix = _coordinates(off)
    length = off.lattice_shape[-1]
    moved = ix[:, -1] + (ix[:, 0] % 7 == 0)
    return (moved >= length // 8).astype(np.int64) + (moved >= length // 2)


def quadrants(off):
    """2 x 2 over the first and the last axis: three neighbours per rank, nodes exported to several ranks"""
    ix = _coordinates(off)
    shape = off.lattice_shape
    return (ix[:, 0] >= shape[0] // 2).astype(np.int64) + 2 * (ix[:, -1] >= shape[-1] // 2)


def last_ghost_columns(off, owner, per_rank=24):
    """For up to `per_rank` rows of the widest width on every rank that couple to another rank, spread over them: the
    node of the row's LAST column in the rank's numbering -- ghosts are numbered behind the owned rows, by (owner, the
    owner's local index), and a rank numbers its exported rows first, both parts in ascending order. The cases with few
    widest rows (the even widths: a dozen widened pairs) make these nodes extrema, so that the limiter is undecided in
    the last column of a widest row on every rank."""
    owner = np.asarray(owner, dtype=np.int64)
    n = off.n_owned
    rs = np.asarray(off.row_starts).astype(np.int64)
    cols = np.asarray(off.columns).astype(np.int64)
    rows = np.repeat(np.arange(n), np.diff(rs))
    foreign = owner[cols] != owner[rows]
    exported = np.bincount(rows[foreign], minlength=n) > 0
    order = np.lexsort((np.arange(n), ~exported, owner))   # by owner; exported rows first; ascending
    key = np.empty(n, dtype=np.int64)
    key[order] = np.arange(n)                              # (owner, local index) as one number
    widths = np.diff(rs)
    nodes = []
    for r in range(int(owner.max()) + 1):
        candidates = np.flatnonzero((owner == r) & exported & (widths == widths.max()))
        assert len(candidates), ("no widest row next to a cut on rank", r)
        for i in candidates[np.unique(np.linspace(0, len(candidates) - 1, min(per_rank, len(candidates))).astype(int))]:
            e = np.arange(rs[i], rs[i + 1])
            e = e[owner[cols[e]] != r]
            nodes.append(cols[e[np.argmax(key[cols[e]])]])
    return np.unique(np.asarray(nodes, dtype=np.int64))


# ------------------------------------------------------------------ the case table

LINE, PLANE, PLANE_LONG, PLANE_1023, BOX_LONG = (640,), (40, 24), (40, 48), (40, 40), (16, 8, 16)

RANK_CASES = {}


def _rank_entry(name, basis, shape, owner, ranks, *, no_split=False, n_pairs=None, ghost_extrema=False):
    """ranks: per rank (n_owned, n_export, [(slices, gridDim.y of step 5, step 6 shares) per launch]); n_pairs (an even
    width): that many widened pairs, so that every rank has widest rows next to a cut, and the nodes of their last
    columns made extrema (last_ghost_columns); ghost_extrema: those extrema on the mesh as it is"""
    base = CASES[basis]
    data = base["data"]
    if ghost_extrema:
        def data(off, inner=base["data"]):
            return inner(off, more=lambda o: last_ghost_columns(o, owner(o)))
    if len(shape) == 1:
        mesh = cases._ring(shape[0], base["request"])   # (the width asked of the recipe: aeos_1d_31 asks for 32)
    elif n_pairs is None:
        mesh = cases._lattice(shape, base["width"])
    else:
        mesh = cases._lattice(shape, base["width"], n_pairs)

        def data(off, inner=base["data"]):
            return inner(off, more=lambda o: last_ghost_columns(o, owner(o)))
    edit = base["edit"]
    if no_split:
        def edit(p, inner=base["edit"]):
            if inner:
                inner(p)
            cases._no_split(p)
    RANK_CASES[name] = dict(
        basis=basis, owner=owner, width=base["width"], equation=base["equation"], plan=base["plan"],
        options=base["options"] + (("no_split=1",) if no_split else ()),
        single=dict(base, mesh=mesh, data=data, n_points=int(np.prod(shape)), edit=edit),
        ranks=[dict(n_owned=n, n_export=x, launches=launches) for n, x, launches in ranks])


def _two(n_owned, n_export, export_slices, slices, grid_y=1):
    """a rank of a case whose ranks are alike: an export and an interior launch (one launch if every slice exports)"""
    launches = [(export_slices, grid_y, False)]
    if slices > export_slices:
        launches.append((slices - export_slices, grid_y, False))
    return (n_owned, n_export, launches)


# Euler 2-D up to 64 entries: k_pij_lij_recompute<2, 4>, at 64 once more with debug_no_small_mesh_split (<2, 1>)
_rank_entry("euler_2d_10", "euler_2d_10", PLANE_LONG, slabs(2), [_two(960, 80, 2, 15, 4)] * 2, n_pairs=96)
_rank_entry("euler_2d_28", "euler_2d_28", PLANE_LONG, quadrants, [_two(480, 143, 3, 8, 4), _two(480, 142, 3, 8, 4)] * 2,
            n_pairs=96)
_rank_entry("euler_2d_33", "euler_2d_33", PLANE_LONG, uneven,
            [_two(234, 234, 4, 4, 4), _two(720, 240, 4, 12, 4), _two(966, 240, 4, 16, 4)])
_rank_entry("euler_2d_64", "euler_2d_64", PLANE_LONG, slabs(2), [_two(960, 320, 5, 15, 4)] * 2)
_rank_entry("euler_2d_64_no_split", "euler_2d_64", PLANE_LONG, slabs(2), [_two(960, 320, 5, 15, 1)] * 2, no_split=True)
# Euler 2-D wide: k_pij_lij<Euler<2>, false, true>
_rank_entry("euler_2d_65", "euler_2d_65", PLANE_LONG, quadrants, [_two(480, 224, 4, 8)] * 4)
_rank_entry("euler_2d_127", "euler_2d_127", PLANE_LONG, uneven,
            [_two(234, 234, 4, 4), _two(720, 503, 8, 12), _two(966, 486, 8, 16)])
_rank_entry("euler_2d_128", "euler_2d_128", PLANE_LONG, slabs(2), [_two(960, 480, 8, 15)] * 2)
_rank_entry("euler_2d_128_all_export", "euler_2d_128", PLANE, slabs(2), [_two(480, 480, 8, 8)] * 2)
_rank_entry("euler_2d_1023", "euler_2d_1023", PLANE_1023, slabs(2), [_two(800, 800, 13, 13)] * 2)
_rank_entry("euler_2d_checked_65", "euler_2d_checked_65", PLANE_LONG, slabs(2), [_two(960, 320, 5, 15)] * 2)
# Euler 3-D
_rank_entry("euler_3d_33", "euler_3d_33", BOX_LONG, slabs(2), [_two(1024, 512, 8, 16)] * 2)
_rank_entry("euler_3d_128", "euler_3d_128", BOX_LONG, slabs(2), [_two(1024, 768, 12, 16)] * 2)
# shallow water: 10 entries leave the single walk of step 4; 65 with bathymetry on the ragged cut; 33 with friction
_rank_entry("sw_2d_10", "sw_2d_10", PLANE_LONG, quadrants,
            [_two(480, 62, 1, 8), _two(480, 62, 1, 8), _two(480, 64, 1, 8), _two(480, 67, 2, 8)], n_pairs=160)
_rank_entry("sw_2d_65", "sw_2d_65", PLANE_LONG, uneven,
            [_two(234, 234, 4, 4), _two(720, 337, 6, 12), _two(966, 326, 6, 16)])
_rank_entry("sw_2d_33", "sw_2d_33", PLANE_LONG, slabs(2), [_two(960, 240, 4, 15)] * 2)
# scalar conservation (KPP), EulerAEOS
_rank_entry("scalar_2d_65", "scalar_2d_65", PLANE_LONG, slabs(2), [_two(960, 320, 5, 15)] * 2)
_rank_entry("aeos_2d_32", "aeos_2d_32", PLANE_LONG, slabs(2), [_two(960, 240, 4, 15)] * 2)
# a ring of rows of up to 65 entries, cut into two contiguous halves: k_pij_lij<Euler<1>, false, true>
_rank_entry("euler_1d_65", "euler_1d_65", LINE, slabs(2), [_two(320, 62, 1, 5)] * 2)
# EulerAEOS in 3-D and 1-D: four bound vectors and four precomputed values per node in the ghost range
_rank_entry("aeos_3d_28", "aeos_3d_28", BOX_LONG, slabs(2), [_two(1024, 256, 4, 16)] * 2, n_pairs=96)
_rank_entry("aeos_1d_31", "aeos_1d_31", LINE, halves_from(24), [_two(320, 30, 1, 5)] * 2, ghost_extrema=True)


# ------------------------------------------------------------------ building and running a case (shared by the tests)

_BUILT = {}


def built(name, oracle):
    """What every test of a case needs, computed ONCE per process and never modified: the single-rank offline data, the
    state developed on the single-rank oracle, the rank views, every rank's share of the state, the single-rank oracle's
    update from it (tau, U_new) and the partitioned oracle's update with every intermediate array."""
    if name in _BUILT:
        return _BUILT[name]
    import helpers_plan_cases as plan_cases
    from helpers_partitioned import one_update_with_intermediates, run_oracle_ranks
    from ryujin_amd import HyperbolicModule
    case = RANK_CASES[name]
    single = case["single"]
    off, dirichlet, states, weights, tau = cases.develop(single, oracle)
    assert dirichlet is None and len(states) == 1 and weights == () and tau == 0.0
    U_start = states[0]
    views = partition_lattice(off, case["owner"](off))
    U_local = [U_start[v.global_ids] for v in views]

    m = HyperbolicModule(off, plan_cases.params_of(single, oracle, off.dim), backend=oracle.backend())
    _oracle_checked(case, oracle, m)
    old, new = m.new_state_vector(U_start), m.new_state_vector()
    m.prepare_state_vector(old, 0.0, None)
    tau_single = m.step(old, [], [], new)
    assert m.last_status == 0
    U_single = new.download()[: off.n_owned]
    m.close()

    ref = run_oracle_ranks(oracle, views, make_params(name, oracle, off.dim), oracle_body(case, oracle, U_local))
    _BUILT[name] = dict(case=case, off=off, views=views, U_local=U_local, tau_single=tau_single, U_single=U_single,
                        ref=ref, k=U_start.shape[1])
    return _BUILT[name]


def make_params(name, oracle, dim):
    import helpers_plan_cases as plan_cases
    return lambda: plan_cases.params_of(RANK_CASES[name]["single"], oracle, dim)


def _oracle_checked(case, oracle, m):
    if case["plan"]["checked"]:   # the checked case switches the oracle to its checked control flow as well
        oracle.lib().ryujin_oracle_set_expensive_bounds_check(m._ctx, 1)


def oracle_body(case, oracle, U_local):
    from helpers_partitioned import one_update_with_intermediates
    inner = one_update_with_intermediates(U_local)

    def body(m, part, r):
        _oracle_checked(case, oracle, m)
        return inner(m, part, r)
    return body


def hip_body(U_local):
    """one update with every intermediate array, and the plan and the launches as the library reports them"""
    from helpers_partitioned import one_update_with_intermediates
    inner = one_update_with_intermediates(U_local)

    def body(m, part, r):
        out = inner(m, part, r)
        out["plan"] = m.last_plan()
        return out
    return body


# ------------------------------------------------------------------ what a case must show before it counts

def _local_pattern(view):
    """(ptr over the locally relevant rows, columns, row of every entry, column position of every entry)"""
    ptr = np.asarray(view.row_starts).astype(np.int64)
    cols = np.asarray(view._keep["columns"]).astype(np.int64)
    lengths = np.diff(ptr)
    rows = np.repeat(np.arange(len(lengths)), lengths)
    return ptr, cols, rows, np.arange(ptr[-1]) - np.repeat(ptr[:-1], lengths)


def ghost_coverage(view, first_pass_lij, width):
    """The condition on ONE rank's inputs (the partitioned oracle's first-pass l_ij over the rank's locally relevant
    rows), as a dict of counts that must all be positive:
      a ghost-column entry strictly between 0 and 1 -- a pair the fast path of the limiter did not decide, whose l_ji is
      read from a ghost row -- in every block of 63 column positions in which some owned row has a ghost column (the
      leading blocks of a very wide row hold owned columns only), and in the last column of a widest row;
      a ghost-ROW entry below 1 and, with 1023 entries, one at position >= 64 of its ghost row."""
    n = view.n_owned
    ptr, cols, rows, position = _local_pattern(view)
    l = np.asarray(first_pass_lij)
    assert l.size == ptr[-1]
    owned, ghost_col = rows < n, cols >= n
    undecided = (l > 0.0) & (l < 1.0)
    out = {}
    for first in range(1, width, BLOCK):
        in_block = owned & ghost_col & (position >= first) & (position < first + BLOCK)
        if in_block.any():
            out[f"ghost columns in block {first}..{min(first + BLOCK, width) - 1}"] = int((in_block & undecided).sum())
    assert out, "a rank without ghost columns"
    lengths = np.diff(ptr)
    last_of_widest = owned & ghost_col & (position == width - 1) & (lengths[rows] == width)
    out[f"ghost column in the last column {width - 1} of a widest row"] = int((last_of_widest & undecided).sum())
    ghost_row = ~owned & (position > 0)
    out["ghost-row entries below 1"] = int((ghost_row & (l < 1.0)).sum())
    if width >= 1023:
        out["ghost-row entries below 1 at position >= 64"] = int((ghost_row & (position >= 64) & (l < 1.0)).sum())
    return out


def first_pass_on_the_single_rank_pattern(off, views, first_pass_of_rank):
    """the first-pass l_ij of the owned rows of all ranks, in the entry order of the single-rank lattice"""
    n = off.n_owned
    rs = np.asarray(off.row_starts).astype(np.int64)
    g_rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rs))
    g_keys = g_rows * n + np.asarray(off.columns).astype(np.int64)
    order = np.argsort(g_keys, kind="stable")
    out = np.full(len(g_keys), np.nan)
    for view, l in zip(views, first_pass_of_rank):
        ptr, cols, rows, _ = _local_pattern(view)
        nnz = int(ptr[view.n_owned])
        gid = np.asarray(view.global_ids).astype(np.int64)
        keys = gid[rows[:nnz]] * n + gid[cols[:nnz]]
        at = order[np.searchsorted(g_keys, keys, sorter=order)]
        assert np.array_equal(g_keys[at], keys)
        out[at] = np.asarray(l)[:nnz]
    assert not np.isnan(out).any(), "an entry no rank owns"
    return out


def assert_coverage(name, b, ref):
    """every condition of a case on the partitioned oracle's arrays `ref`; returns the counts per rank for the log"""
    case, counts = b["case"], []
    for r, view in enumerate(b["views"]):
        covered = ghost_coverage(view, ref[r]["lij_next"], case["width"])
        assert min(covered.values()) > 0, (name, r, {k: v for k, v in covered.items() if v == 0})
        counts.append(covered)
    union = first_pass_on_the_single_rank_pattern(b["off"], b["views"], [x["lij_next"] for x in ref])
    covered = cases.coverage(b["off"], union, case["width"])
    assert min(covered.values()) > 0, (name, "union of the owned rows", {k: v for k, v in covered.items() if v == 0})
    return counts


# ------------------------------------------------------------------ the figures of the log

def measured(part, g, c, k, scales):
    """the largest difference of every array compare_rank holds to a bound, in that bound's units"""
    n, nr = part.n_owned, part.n_relevant
    ptr = np.asarray(part.row_starts).astype(np.int64)
    nnz_owned = int(ptr[n])

    def rel(a, b):
        return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-300)).max()) if a.size else 0.0
    scale = np.maximum(np.abs(c["U"]).max(axis=0), 1e-3 * np.abs(c["U"]).max())
    off_diag = np.ones(nnz_owned, dtype=bool)   # ("pij" holds the owned rows)
    off_diag[ptr[:n]] = False   # (P_ii is never read: compare_rank overwrites it)
    return dict(
        tau=abs(g["tau"] - c["tau"]) / c["tau"], U_old=float(np.abs(g["U_old"] - c["U_old"]).max()),
        prec=rel(g["prec"], c["prec"]), alpha=float(np.abs(g["alpha"] - c["alpha"]).max()), dij=rel(g["dij"], c["dij"]),
        bounds=rel(g["bounds"], c["bounds"]),
        r=float((np.abs(g["r"] - c["r"]).reshape(nr, k) / scales[0]).max()),
        pij=float((np.abs(g["pij"] - c["pij"]).reshape(-1, k)[off_diag] / scales[1]).max()),
        lij=float(np.abs(g["lij"][:nnz_owned] - c["lij"][:nnz_owned]).max()),
        lij_next=float(np.abs(g["lij_next"][:nnz_owned] - c["lij_next"][:nnz_owned]).max()),
        U=float((np.abs(g["U"] - c["U"]) / scale).max()))
