"""Test helper: OfflineData of a DISCONTINUOUS Q1 or Q2 ansatz (dg_q1, dg_q2) on a tensor-product mesh in one to three
dimensions, uniform or graded, assembled with numpy as the reference assembles its matrices for `have_discontinuous_ansatz()` (source/offline_data.template.h):

  :560-577   cell terms          m_ij = int_K phi_i phi_j,   c_ij = int_K phi_i grad phi_j
  :588-665   interior faces      c_ij -= 1/2 int_F phi_i phi_j n            (i, j in the same cell)
                                 c_ij += 1/2 int_F phi_i phi_j^nb n         (j in the face neighbour)
  :667-674   mass_matrix_inverse = inverse of the cell mass matrix (block diagonal)
  :809-906   incidence matrix    beta_ij = (0.5 (m_i + m_j) / |Omega|)^(relaxation_odd / dim) = 1 for dg_q1
                                 (`incidence matrix relaxation odd degree` = 0, :53) for the pairs of DoFs of
                                 two face neighbours that sit on the same node of the common face;
  :46-53, 905-925                for dg_q2 the exponent is relaxation_even / dim with relaxation_even = 0.5
  :149-156   stencil             make_extended_sparsity_pattern_dg: all DoFs of the cell and of its face
                                 neighbours (many structural zeros: the limiter bounds are combined over them)

Boundary faces carry no face term (:591-598). DoF numbering is cell-wise ((degree + 1)^dim
consecutive DoFs per cell). dg_q1_offline(n_cells, h) is dg_offline(n_cells, h, 1); tests/test_dg_cases_cpu.py holds it bit
for bit to the loop over dictionaries it replaced."""
import numpy as np

from helpers_layout import OfflineView
from ryujin_amd import capi

M1 = np.array([[2.0, 1.0], [1.0, 2.0]]) / 6.0          # int phi_a phi_b on [0,1]
D1 = np.array([[-0.5, 0.5], [-0.5, 0.5]])              # int phi_a phi_b'  (independent of h)
# degree 2, nodes 0, 1/2, 1 (the Gauss-Lobatto nodes): mass, int phi_a phi_b', int phi_a
M2 = np.array([[4.0, 2.0, -1.0], [2.0, 16.0, 2.0], [-1.0, 2.0, 4.0]]) / 30.0
D2 = np.array([[-3.0, 4.0, -1.0], [-4.0, 0.0, 4.0], [1.0, -4.0, 3.0]]) / 6.0
ELEMENT_1D = {1: (M1, D1, np.array([0.5, 0.5])), 2: (M2, D2, np.array([1.0, 4.0, 1.0]) / 6.0)}
INCIDENCE_RELAXATION = {1: 0.0, 2: 0.5}   # odd / even degree (offline_data.template.h:46-53)


def graded(n, ratio=1.6):
    """n cell widths that sum to 1 and grow geometrically, the last `ratio` times the first: no two alike"""
    w = ratio ** np.linspace(0.0, 1.0, n)
    return w / w.sum()


def dg_offline(n_cells, h, degree=1, boundary_id=capi.BC_DO_NOTHING):
    """dG-Q`degree` (1 or 2) on a tensor-product mesh of n_cells[d] cells per axis, one to three dimensions; h: one
    number (uniform) or a tuple of per-axis arrays of cell widths (a graded mesh: m_i, (M^-1)_ij and, for degree 2, the
    incidence values vary from cell to cell). Tensor products of the 1-D element matrices on equidistant nodes; the
    assembly is the one the module docstring cites, entry by entry over the whole CSR pattern at once. Incidence between
    the two DoFs on the same node of a common face: (1/2 (m_i + m_j) / |Omega|)^(relaxation / dim), relaxation 0 for
    degree 1 (the value is 1) and 0.5 for degree 2 (:905-925). DoF numbering cell-wise, x fastest in the cell and among
    the cells. Returns (offline data, dict(rows, is_bdry, n_per_cell, cell_mass, cell_mass_inverse))."""
    dim, p1 = len(n_cells), degree + 1
    M, D, W = ELEMENT_1D[degree]
    npc, n_cell = p1 ** dim, int(np.prod(n_cells))
    n = n_cell * npc
    uniform = np.isscalar(h)
    hs = [np.full(n_cells[d], float(h)) if uniform else np.asarray(h[d], dtype=np.float64) for d in range(dim)]
    assert all(len(hs[d]) == n_cells[d] for d in range(dim))
    cell_ix = np.stack(np.unravel_index(np.arange(n_cell), tuple(reversed(n_cells)))[::-1], axis=1)   # x fastest
    local_ix = np.stack(np.unravel_index(np.arange(npc), (p1,) * dim)[::-1], axis=1)
    stride = np.concatenate([[1], np.cumprod(n_cells[:-1])]).astype(np.int64)
    end = (0, degree)   # the 1-D node on side 0 / side 1 of a cell

    # slot 0: the cell itself; slot 1 + 2 d + side: its neighbour across the face (d, side), -1 at the boundary
    n_slots = 1 + 2 * dim
    nb = np.full((n_cell, n_slots), -1, dtype=np.int64)
    nb[:, 0] = np.arange(n_cell)
    for d in range(dim):
        for side in (0, 1):
            there = (cell_ix[:, d] > 0) if side == 0 else (cell_ix[:, d] < n_cells[d] - 1)
            nb[there, 1 + 2 * d + side] = np.flatnonzero(there) + (2 * side - 1) * stride[d]
    slot_order = np.argsort(np.where(nb < 0, n_cell, nb), axis=1, kind="stable")   # by cell id: ascending columns
    nb_sorted = np.take_along_axis(nb, slot_order, axis=1)

    # every entry (cell, a, slot, b) of the stencil, rows in order, columns ascending; then the diagonal to the front
    shape = (n_cell, npc, n_slots, npc)
    cell = np.broadcast_to(np.arange(n_cell)[:, None, None, None], shape)
    a = np.broadcast_to(np.arange(npc)[None, :, None, None], shape)
    b = np.broadcast_to(np.arange(npc)[None, None, None, :], shape)
    slot = np.broadcast_to(slot_order[:, None, :, None], shape)
    other = np.broadcast_to(nb_sorted[:, None, :, None], shape)
    present = (other >= 0).reshape(-1)
    cell, a, b, slot, other = (x.reshape(-1)[present] for x in (cell, a, b, slot, other))
    i, j = cell * npc + a, other * npc + b
    order = np.lexsort((np.where(i == j, -1, j), i))
    cell, a, b, slot, i, j = (x[order] for x in (cell, a, b, slot, i, j))
    widths = np.bincount(i, minlength=n)
    row_starts = np.concatenate([[0], np.cumsum(widths)]).astype(np.uint64)
    columns = j.astype(np.uint32)

    al, bl = local_ix[a], local_ix[b]                                   # [nnz, dim]: the 1-D node indices
    F = np.stack([hs[d][cell_ix[cell, d]] * M[al[:, d], bl[:, d]] for d in range(dim)], axis=1)

    def mass1(d_skip):
        """product of the 1-D mass entries over all directions but d_skip"""
        v = np.ones(len(i))
        for d in range(dim):
            if d != d_skip:
                v = v * F[:, d]
        return v

    # cell mass matrices and their inverses (block diagonal)
    Fc = [hs[d][cell_ix[:, d], None, None] * M[local_ix[:, d][:, None], local_ix[:, d][None, :]][None] for d in range(dim)]
    cell_mass = Fc[0]
    for d in range(1, dim):
        cell_mass = cell_mass * Fc[d]
    cell_mass_inverse = np.linalg.inv(cell_mass)
    own = slot == 0
    mij = np.where(own, cell_mass[cell, a, b], 0.0)
    minv = np.where(own, cell_mass_inverse[cell, a, b], 0.0)
    mi = np.add.reduceat(mij, row_starts[:-1].astype(np.int64))

    cij = np.zeros((len(i), dim))
    couples = np.zeros(len(i), dtype=bool)    # the pairs on the same node of a common face
    has_nb = nb >= 0
    for d in range(dim):
        m1 = mass1(d)
        cij[:, d] = np.where(own, D[al[:, d], bl[:, d]] * m1, 0.0)
        same_node = np.ones(len(i), dtype=bool)
        for dd in range(dim):
            if dd != d:
                same_node &= al[:, dd] == bl[:, dd]
        for side, sign in ((0, -1.0), (1, +1.0)):
            s = 1 + 2 * d + side
            on_face = al[:, d] == end[side]
            inner = own & on_face & (bl[:, d] == end[side]) & has_nb[cell, s]          # own cell
            cij[inner, d] = cij[inner, d] - 0.5 * sign * m1[inner]
            across = (slot == s) & on_face & (bl[:, d] == end[1 - side])              # the neighbour's DoFs on the face
            cij[across, d] = cij[across, d] + 0.5 * sign * m1[across]
            couples |= across & same_node
    measure = mi.sum()
    inc = np.zeros(len(i))
    if INCIDENCE_RELAXATION[degree] == 0.0:
        inc[couples] = 1.0
    else:
        inc[couples] = (0.5 * (mi[i[couples]] + mi[j[couples]]) / measure) ** (INCIDENCE_RELAXATION[degree] / dim)

    # boundary faces carry no face term: normals int_F phi_i n only
    nrm = np.zeros((n, dim))
    is_bdry = np.zeros(n, dtype=bool)
    dof_cell, dof_l = np.repeat(np.arange(n_cell), npc), local_ix[np.tile(np.arange(npc), n_cell)]
    for d in range(dim):
        weight = None
        for dd in range(dim):
            if dd != d:
                f = hs[dd][cell_ix[dof_cell, dd]] * W[dof_l[:, dd]]
                weight = f if weight is None else weight * f
        if weight is None:
            weight = np.ones(n)
        for side, sign in ((0, -1.0), (1, +1.0)):
            at = (dof_l[:, d] == end[side]) & ~has_nb[dof_cell, 1 + 2 * d + side]
            nrm[at, d] += sign * weight[at]
            is_bdry |= at

    if uniform:
        positions = (cell_ix[dof_cell] + dof_l / degree) * float(h)
    else:
        edges = [np.concatenate([[0.0], np.cumsum(hs[d])]) for d in range(dim)]
        positions = np.stack([edges[d][cell_ix[dof_cell, d]] + dof_l[:, d] / degree * hs[d][cell_ix[dof_cell, d]]
                              for d in range(dim)], axis=1)

    b_i = np.flatnonzero(is_bdry).astype(np.uint32)
    b_normal = nrm[b_i] / np.linalg.norm(nrm[b_i], axis=1)[:, None]
    col_idx = np.arange(len(i)) - np.repeat(row_starts[:-1].astype(np.int64), widths)
    pair = is_bdry[i] & is_bdry[j] & (col_idx > 0)
    off = OfflineView(dim, 0, 0, n, n, 1, row_starts, columns, cij, mij, mi, 1.0 / mi, measure, b_i, b_normal,
                      np.full(len(b_i), boundary_id, dtype=np.uint8), i[pair], col_idx[pair], j[pair])
    off.positions = positions
    off.row_starts, off.columns, off.cij_csr, off.mij_csr, off.mi = row_starts, columns, cij, mij, mi
    off.max_row_len = int(widths.max())
    attach_dg(off, inc, minv)
    rs = row_starts.astype(np.int64)
    cols = j.tolist()
    rows = [cols[rs[q]:rs[q + 1]] for q in range(n)]
    return off, dict(rows=rows, is_bdry=is_bdry, n_per_cell=npc, cell_mass=cell_mass,
                     cell_mass_inverse=cell_mass_inverse, degree=degree, n_cells=tuple(n_cells))


def dg_q1_offline(n_cells, h, boundary_id=capi.BC_DO_NOTHING):
    return dg_offline(n_cells, h, 1, boundary_id)


def attach_dg(view, incidence, mass_matrix_inverse):
    view._dg = (np.ascontiguousarray(incidence, dtype=np.float64),
                np.ascontiguousarray(mass_matrix_inverse, dtype=np.float64))
    view._o.discontinuous_ansatz = 1
    view._o.incidence = capi.as_ptr(view._dg[0], capi.c_double_p)
    view._o.mass_matrix_inverse = capi.as_ptr(view._dg[1], capi.c_double_p)
