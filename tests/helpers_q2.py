"""Continuous Q2 elements on a periodic Cartesian mesh, assembled for the tests the way the reference assembles its
matrices (source/offline_data.template.h:560-674: c_ij = int phi_i grad phi_j, m_ij = int phi_i phi_j, lumped masses
m_i = sum_j m_ij): rows of 27 ... 125 entries in 3-D (9 ... 25 in 2-D) -- the stencil sizes of the reference's higher
order ansatz spaces (source/discretization.h:131-151), wider than one SELL-64 slice has lanes. Tensor products of the
1-D element matrices; periodic in every direction (no boundary map, c_ij antisymmetric everywhere)."""
import numpy as np

from helpers_layout import OfflineView


def _q2_1d(n_elements, h):
    """Assembled periodic 1-D Q2 matrices on n_elements elements of size h: nodes 2e (vertex), 2e + 1 (mid point)."""
    M_loc = h / 30.0 * np.array([[4.0, 2.0, -1.0], [2.0, 16.0, 2.0], [-1.0, 2.0, 4.0]])
    D_loc = np.array([[-3.0, 4.0, -1.0], [-4.0, 0.0, 4.0], [1.0, -4.0, 3.0]]) / 6.0   # int phi_a phi_b'
    n = 2 * n_elements
    M, D = np.zeros((n, n)), np.zeros((n, n))
    for e in range(n_elements):
        idx = [2 * e, 2 * e + 1, (2 * e + 2) % n]
        for a in range(3):
            for b in range(3):
                M[idx[a], idx[b]] += M_loc[a, b]
                D[idx[a], idx[b]] += D_loc[a, b]
    return M, D


def q2_periodic_offline(dim, n_elements, length=1.0):
    """(OfflineView, positions): periodic Q2 mesh of n_elements^dim elements on [0, length)^dim."""
    assert n_elements >= 3, "five distinct nodes per direction in a vertex row"
    h = length / n_elements
    M1, D1 = _q2_1d(n_elements, h)
    n1 = M1.shape[0]
    pattern1 = M1 != 0.0
    n = n1 ** dim

    def kron(mats):
        out = mats[0]
        for m in mats[1:]:
            out = np.kron(out, m)
        return out
    M = kron([M1] * dim)
    C = [kron([D1 if e == d else M1 for e in range(dim)]) for d in range(dim)]
    pattern = kron([pattern1.astype(float)] * dim) != 0.0
    rows = []
    for i in range(n):
        js = np.flatnonzero(pattern[i])
        rows.append([i] + [int(j) for j in js if j != i])          # diagonal first, then ascending
    row_starts = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    columns = np.concatenate([np.array(r, dtype=np.uint32) for r in rows])
    ii = np.repeat(np.arange(n), [len(r) for r in rows])
    cij = np.stack([Cd[ii, columns] for Cd in C], axis=1)
    mij = M[ii, columns]
    mi = M.sum(axis=1)
    assert (mi > 0).all() and np.abs(sum(Cd.sum(axis=1) for Cd in C)).max() < 1e-13
    off = OfflineView(dim, 0, 0, n, n, 1, row_starts, columns, cij, mij, mi, 1.0 / mi, mi.sum(), [],
                      np.zeros((0, dim)), [], [], [], [])
    # node coordinates, first index slowest (np.kron ordering)
    x1 = 0.5 * h * np.arange(n1)
    grids = np.meshgrid(*([x1] * dim), indexing="ij")
    positions = np.stack([g.reshape(-1) for g in grids], axis=1)
    off.positions = positions
    off.row_starts, off.columns, off.mi = row_starts, columns, mi
    off.max_row_len = max(len(r) for r in rows)
    return off, positions


def q2_periodic_offline_sparse(dim, n_elements, length=1.0):
    """q2_periodic_offline without the dense n x n matrices (2-D only): the same rows, columns, c_ij and m_ij entry by
    entry from the 1-D factors, for lattices of tens of thousands of nodes (tests/test_step_plan.py compares the two on
    a small lattice)."""
    assert dim == 2 and n_elements >= 3
    h = length / n_elements
    M1, D1 = _q2_1d(n_elements, h)
    n1 = M1.shape[0]
    n = n1 * n1
    nbr = [np.flatnonzero(M1[a] != 0.0) for a in range(n1)]            # ascending
    i0, i1 = np.divmod(np.arange(n), n1)
    counts = np.array([len(nbr[a]) for a in range(n1)])
    widths = counts[i0] * counts[i1]
    row_starts = np.concatenate([[0], np.cumsum(widths)]).astype(np.uint64)
    rows_i, j0, j1 = [], [], []
    for a in range(n1):                                               # all rows with i0 = a at once
        for b in range(n1):
            i = a * n1 + b
            ja, jb = np.meshgrid(nbr[a], nbr[b], indexing="ij")       # ascending in j = ja n1 + jb
            ja, jb = ja.reshape(-1), jb.reshape(-1)
            diag = (ja == a) & (jb == b)
            order = np.concatenate([np.flatnonzero(diag), np.flatnonzero(~diag)])   # diagonal first, then ascending
            rows_i.append(np.full(order.size, i))
            j0.append(ja[order])
            j1.append(jb[order])
    ii, j0, j1 = np.concatenate(rows_i), np.concatenate(j0), np.concatenate(j1)
    e0, e1 = ii // n1, ii % n1
    columns = (j0 * n1 + j1).astype(np.uint32)
    mij = M1[e0, j0] * M1[e1, j1]
    cij = np.stack([D1[e0, j0] * M1[e1, j1], M1[e0, j0] * D1[e1, j1]], axis=1)
    mi = np.add.reduceat(mij, row_starts[:-1].astype(np.int64))
    assert (mi > 0).all()
    off = OfflineView(dim, 0, 0, n, n, 1, row_starts, columns, cij, mij, mi, 1.0 / mi, mi.sum(), [],
                      np.zeros((0, dim)), [], [], [], [])
    x1 = 0.5 * h * np.arange(n1)
    grids = np.meshgrid(x1, x1, indexing="ij")
    positions = np.stack([g.reshape(-1) for g in grids], axis=1)
    off.positions = positions
    off.row_starts, off.columns, off.mi = row_starts, columns, mi
    off.max_row_len = int(widths.max())
    return off, positions
