"""Consistent offline data with a PRESCRIBED widest stencil row, for the tests of the row-width thresholds of
ryujin_amd/csrc/step_plan.hpp (tests/helpers_row_width_cases.py: the case table).

A lattice in one, two or three dimensions, axis 0 fastest in the numbering. Every node is coupled to the nodes at a
symmetric set of integer offsets: the first (W - 1) / 2 vectors of a half-space ordering (by length, then
lexicographically) and their negatives -- W entries per row with the diagonal. The lattice is periodic, or open along
chosen axes: there the rows lose the columns that fall off the lattice, and with axis 0 open -- the fastest one -- every
slice of 64 consecutive rows holds rows of many widths next to full ones (padding inside a slice). Extra symmetric pairs between
chosen nodes widen those two rows by one entry each: even widths are reached this way.

What the data satisfies is what step() relies on: c_ij = -c_ji, c_ii = 0, m_ij = m_ji > 0, m_i = sum_j m_ij, columns
sorted with the diagonal first -- and sum_j c_ij = 0 in every row, without which the low-order update is no convex
combination of the bar states and every update of a rough flow reports an invariant-domain violation. The weights
depend on the offset vector d alone,
    c0_ij = beta h^(dim-1) d / |d|,  beta = dim / sum_d |d|     (sum_j c0_ij (x_j - x_i) = dim h^dim in a full row),
    m_ij = h^dim / (2 (W - 1)) (1 + 1 / (2 (1 + |d|^2))),  m_ii = h^dim / 2,
so that the far columns weigh as much as the near ones: with decaying weights the far P_ij would be negligible and the
limiter would never act there. Where rows are cut off (an open end) or widened, the c0_ij of a row do not sum to zero:
c_ij = c0_ij + phi_j - phi_i with the node vectors phi that solve the graph Laplacian system L phi = (row sums of c0)
-- the antisymmetric correction of least squares. No boundary map."""
from __future__ import annotations

import numpy as np

from helpers_layout import OfflineView


def half_space_offsets(dim, count, norm="euclid"):
    """the first `count` integer vectors of the half space (last non-zero component positive), by length -- Euclidean,
    or the largest component ("max": the stencil fills squares / cubes) --, then lexicographically: [count, dim]"""
    if count == 0:
        return np.zeros((0, dim), dtype=np.int64)
    R = 1
    while True:
        axes = np.meshgrid(*([np.arange(-R, R + 1)] * dim), indexing="ij")
        d = np.stack([a.reshape(-1) for a in axes], axis=1)
        sign = np.zeros(len(d), dtype=np.int64)
        for a in range(dim):                       # the last non-zero component decides
            sign = np.where(d[:, a] != 0, np.sign(d[:, a]), sign)
        d = d[sign > 0]
        length = (d * d).sum(axis=1) if norm == "euclid" else np.abs(d).max(axis=1) ** 2
        d, length = d[length <= R * R], length[length <= R * R]   # (a box of half width R holds every such vector)
        if len(d) >= count:
            break
        R += 1
    keys = [d[:, a] for a in range(dim)] + [length]
    return d[np.lexsort(keys)][:count]


def _ravel(shape, ix):
    """node number of the lattice coordinates ix[..., dim]: axis 0 fastest"""
    out = np.zeros(ix.shape[:-1], dtype=np.int64)
    for a in reversed(range(len(shape))):
        out = out * shape[a] + ix[..., a]
    return out


def _unravel(shape, i):
    ix = np.zeros((len(i), len(shape)), dtype=np.int64)
    rest = np.asarray(i, dtype=np.int64).copy()
    for a in range(len(shape)):
        ix[:, a] = rest % shape[a]
        rest //= shape[a]
    return ix


def widening_pairs(shape, width, n_pairs, open_axes=(0,)):
    """`n_pairs` node pairs (a, a + d) with d the first offset BEYOND the stencil of odd width `width`, both nodes rows
    of full width and no node used twice, spread over the lattice (a stride that is prime to its size): [n_pairs, 2]"""
    dim = len(shape)
    H = (width - 1) // 2
    offsets = half_space_offsets(dim, H + 1)
    d, reach = offsets[H], np.abs(offsets[:H]).max(axis=0)
    n = int(np.prod(shape))
    used, pairs = set(), []
    stride = 193 if n % 193 else 197
    for q in range(n):
        a = (q * stride + n // 3) % n
        xa = _unravel(shape, [a])[0]
        xb = xa + d
        if any(not (reach[q] <= x[q] < shape[q] - reach[q]) for q in open_axes for x in (xa, xb)):
            continue
        b = int(_ravel(shape, xb % np.asarray(shape)))
        if a in used or b in used or a == b:
            continue
        used.update((a, b))
        pairs.append((a, b))
        if len(pairs) == n_pairs:
            return np.asarray(pairs, dtype=np.int64)
    raise ValueError("lattice too small for that many widening pairs")


def lattice_offline(shape, width, *, open_axes=(0,), extra_pairs=None, norm="euclid"):
    """OfflineView of the lattice `shape` (axis 0 fastest) with rows of `width` entries (odd) where the stencil is
    complete; open along `open_axes`, periodic along the others; `extra_pairs` [n, 2]: further symmetric pairs of
    nodes; `norm`: the ordering of half_space_offsets(). Carries .positions, .columns, .cij, .mij, .mi,
    .max_row_len and the empty boundary map of a SyntheticOffline."""
    shape = tuple(int(s) for s in shape)
    dim, n = len(shape), int(np.prod(shape))
    assert width % 2 == 1 and width >= 3
    half = half_space_offsets(dim, (width - 1) // 2, norm)
    offsets = np.concatenate([half, -half])
    for a in range(dim):   # offsets stay distinct modulo the period; an open axis keeps rows of full width
        reach = int(np.abs(offsets[:, a]).max())
        assert shape[a] >= 2 * reach + 1 + (2 if a in open_axes else 0), (a, shape[a], reach)
    h = 1.0 / shape[0]
    ix = _unravel(shape, np.arange(n))
    shape_a = np.asarray(shape)
    is_open = np.isin(np.arange(dim), list(open_axes))
    rows, cols, vecs = [], [], []
    for d in offsets:
        jx = ix + d
        ok = ((jx[:, is_open] >= 0) & (jx[:, is_open] < shape_a[is_open])).all(axis=1)
        rows.append(np.flatnonzero(ok))
        cols.append(_ravel(shape, jx[ok] % shape_a))
        vecs.append(np.broadcast_to(d, (int(ok.sum()), dim)))
    if extra_pairs is not None and len(extra_pairs):
        pairs = np.asarray(extra_pairs, dtype=np.int64)
        xa, xb = _unravel(shape, pairs[:, 0]), _unravel(shape, pairs[:, 1])
        d = xb - xa
        d -= np.round(d / shape_a).astype(np.int64) * shape_a * ~is_open   # the short way round a periodic axis
        rows += [pairs[:, 0], pairs[:, 1]]
        cols += [pairs[:, 1], pairs[:, 0]]
        vecs += [d, -d]
    rows.append(np.arange(n))
    cols.append(np.arange(n))
    vecs.append(np.zeros((n, dim), dtype=np.int64))
    rows, cols, vecs = np.concatenate(rows), np.concatenate(cols), np.concatenate(vecs).astype(np.float64)
    order = np.lexsort((cols, rows != cols, rows))    # by row; the diagonal first, then ascending columns
    rows, cols, vecs = rows[order], cols[order], vecs[order]
    assert not ((rows[1:] == rows[:-1]) & (cols[1:] == cols[:-1])).any(), "a pair given twice"
    widths = np.bincount(rows, minlength=n)
    row_starts = np.concatenate([[0], np.cumsum(widths)]).astype(np.uint64)
    length2 = (vecs * vecs).sum(axis=1)
    off_diag = length2 > 0
    beta = dim / np.sqrt((offsets * offsets).sum(axis=1)).sum()
    cij = np.zeros((len(rows), dim))
    cij[off_diag] = beta * h ** (dim - 1) * vecs[off_diag] / np.sqrt(length2[off_diag])[:, None]
    cij = _without_row_sums(rows, cols, cij, n)
    mij = np.where(off_diag, h ** dim / (2.0 * (width - 1)) * (1.0 + 0.5 / (1.0 + length2)), 0.5 * h ** dim)
    mi = np.add.reduceat(mij, row_starts[:-1].astype(np.int64))
    off = OfflineView(dim, 0, 0, n, n, 1, row_starts, cols.astype(np.uint32), cij, mij, mi, 1.0 / mi, mi.sum(),
                      [], np.zeros((0, dim)), [], [], [], [])
    off.positions = (ix + 0.5) * h
    off.columns, off.cij, off.mij = off._keep["columns"], off._keep["cij"], off._keep["mij"]
    off.max_row_len = int(widths.max())
    off.b_i, off.b_positions = np.zeros(0, dtype=np.int64), np.zeros((0, dim))
    off.lattice_shape = shape
    return off


def _without_row_sums(rows, cols, c0, n):
    """c0_ij + phi_j - phi_i with L phi = (row sums of c0), L the Laplacian of the stencil graph: antisymmetric as c0,
    every row sums to zero (to round-off). A dense solve with phi_0 = 0 (the graph is connected, the right-hand side
    sums to zero over it) and one step of iterative refinement: a few thousand nodes at the most."""
    dim = c0.shape[1]

    def row_sums(c):
        return np.stack([np.bincount(rows, weights=c[:, a], minlength=n) for a in range(dim)], axis=1)
    scale = np.bincount(rows, weights=np.abs(c0).sum(axis=1), minlength=n).max()
    if np.abs(row_sums(c0)).max() <= 1e-14 * scale:
        return c0
    off_diag = rows != cols
    L = np.zeros((n, n))
    L[rows[off_diag], cols[off_diag]] = -1.0
    L[np.arange(n), np.arange(n)] = np.bincount(rows[off_diag], minlength=n)
    out = c0.copy()
    for _ in range(2):
        phi = np.zeros((n, dim))
        phi[1:] = np.linalg.solve(L[1:, 1:], row_sums(out)[1:])
        out += (phi[cols] - phi[rows]) * off_diag[:, None]
    assert np.abs(row_sums(out)).max() <= 1e-13 * scale, np.abs(row_sums(out)).max() / scale
    return out


def widths_of(off):
    return np.diff(np.asarray(off.row_starts[: off.n_owned + 1]).astype(np.int64))


def transposed_entries(off):
    """for every entry (i, j) the index of (j, i): numpy only"""
    widths = widths_of(off)
    rows = np.repeat(np.arange(off.n_owned, dtype=np.int64), widths)
    cols = np.asarray(off.columns).astype(np.int64)
    n = off.n_owned
    forward, backward = np.argsort(rows * n + cols, kind="stable"), np.argsort(cols * n + rows, kind="stable")
    tr = np.empty(len(rows), dtype=np.int64)
    tr[forward] = backward
    return tr


def check_consistency(off, width):
    """the properties the module docstring states; raises AssertionError"""
    n = off.n_owned
    widths = widths_of(off)
    rs = np.asarray(off.row_starts).astype(np.int64)
    cols = np.asarray(off.columns).astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), widths)
    assert widths.max() == width and widths.min() >= 3, (widths.max(), widths.min())
    assert (cols[rs[:-1]] == np.arange(n)).all(), "diagonal first"
    is_diag = np.zeros(len(cols), dtype=bool)
    is_diag[rs[:-1]] = True
    assert (np.diff(cols)[~is_diag[1:] & ~is_diag[:-1]] > 0).all(), "columns ascending behind the diagonal"
    assert (cols[~is_diag] != rows[~is_diag]).all(), "one diagonal entry per row"
    tr = transposed_entries(off)
    assert (rows[tr] == cols).all() and (cols[tr] == rows).all(), "the pattern is symmetric"
    assert (tr[tr] == np.arange(len(tr))).all()
    assert (off.cij[tr] == -off.cij).all() and (off.cij[rs[:-1]] == 0.0).all()
    row_sums = np.add.reduceat(off.cij, rs[:-1], axis=0)
    assert np.abs(row_sums).max() <= 1e-13 * np.add.reduceat(np.abs(off.cij).sum(axis=1), rs[:-1]).max(), "row sums"
    assert (off.mij[tr] == off.mij).all() and (off.mij > 0.0).all()
    np.testing.assert_allclose(np.add.reduceat(off.mij, rs[:-1]), off.mi, rtol=0, atol=0)
    # rows of the widest width in at least two slices, sharing slices with rows of several narrower widths
    slices = np.arange(n) // 64
    widest = np.unique(slices[widths == width])
    assert len(widest) >= 2, widest
    # (several: the widest and at least two narrower widths; rows of 3 or 4 entries are all a widest row of 4 admits)
    several = min(3, width - 2)
    mixed = [s for s in widest if len(np.unique(widths[slices == s])) >= several]
    assert len(mixed) >= 2, "no padding of several widths next to a widest row"
    return widths
