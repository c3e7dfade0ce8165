"""The dG case table (tests/helpers_dg_cases.py) and the generalised dG assembly (tests/helpers_dg.py: dg_offline) on the
CPU, before any GPU run: the properties of the assembled matrices, what every case must show on the oracle alone
(status, coverage of the limiter, both arms of the incidence fmax, the dG branch in effect), conservation of the oracle
on the new stencils, and the partitioned oracle -- the yardstick of the rank cases -- against the single-rank one."""
import itertools
import time

import numpy as np
import pytest

import helpers_dg_cases as cases
from helpers_dg import D1, D2, ELEMENT_1D, M1, M2, dg_offline, dg_q1_offline, graded
from helpers_layout import OfflineView
from ryujin_amd import HyperbolicModule, capi


# ------------------------------------------------------------------ the assembly

def _dg_q1_offline_by_dictionaries(n_cells, h, boundary_id=capi.BC_DO_NOTHING):
    """dg_q1_offline as it was before dg_offline: one Python loop over cells, faces and pairs of local DoFs that collects
    the entries in dictionaries (uniform meshes, degree 1). Kept as the yardstick of the bit-for-bit comparison."""
    dim = len(n_cells)
    loc = [tuple(reversed(t)) for t in itertools.product((0, 1), repeat=dim)]   # local vertices, x fastest
    npc = len(loc)

    def cell_id(c):
        idx = 0
        for d in reversed(range(dim)):
            idx = idx * n_cells[d] + c[d]
        return idx

    def dof(c, a):
        return cell_id(c) * npc + loc.index(tuple(a))

    n = int(np.prod(n_cells)) * npc
    c_acc, m_acc, minv_acc, inc_acc = {}, {}, {}, {}
    nrm = np.zeros((n, dim))
    is_bdry = np.zeros(n, dtype=bool)
    positions = np.zeros((n, dim))

    def mass1(d_skip, a, b):
        v = 1.0
        for d in range(dim):
            if d != d_skip:
                v *= h * M1[a[d]][b[d]]
        return v

    cell_mass = np.array([[np.prod([h * M1[a[d]][b[d]] for d in range(dim)]) for b in loc] for a in loc])
    cell_mass_inverse = np.linalg.inv(cell_mass)
    for c in itertools.product(*[range(k) for k in reversed(n_cells)]):
        c = tuple(reversed(c))
        for ia, a in enumerate(loc):
            i = dof(c, a)
            positions[i] = [(c[d] + a[d]) * h for d in range(dim)]
            for ib, b in enumerate(loc):
                j = dof(c, b)
                m_acc[(i, j)] = cell_mass[ia, ib]
                minv_acc[(i, j)] = cell_mass_inverse[ia, ib]
                grad = np.array([D1[a[d]][b[d]] * mass1(d, a, b) for d in range(dim)])
                c_acc[(i, j)] = c_acc.get((i, j), 0.0) + grad
        for d in range(dim):
            for side, sign in ((0, -1.0), (1, +1.0)):
                nb = list(c)
                nb[d] += 1 if side else -1
                normal = np.zeros(dim)
                normal[d] = sign
                on_face = [a for a in loc if a[d] == side]
                if not (0 <= nb[d] < n_cells[d]):
                    for a in on_face:
                        i = dof(c, a)
                        nrm[i] += normal * np.prod([h * 0.5 for dd in range(dim) if dd != d])
                        is_bdry[i] = True
                    continue
                for a in on_face:
                    i = dof(c, a)
                    for b in on_face:
                        j = dof(c, b)
                        c_acc[(i, j)] = c_acc[(i, j)] - 0.5 * normal * mass1(d, a, b)
                    for b in loc:
                        j = dof(tuple(nb), b)
                        c_acc.setdefault((i, j), np.zeros(dim))
                        if b[d] == 1 - side:
                            c_acc[(i, j)] = c_acc[(i, j)] + 0.5 * normal * mass1(d, a, b)
                            if all(a[dd] == b[dd] for dd in range(dim) if dd != d):
                                inc_acc[(i, j)] = 1.0
                for a in loc:
                    i = dof(c, a)
                    for b in loc:
                        c_acc.setdefault((i, dof(tuple(nb), b)), np.zeros(dim))
    rows = [[i] for i in range(n)]
    for (i, j) in c_acc:
        if i != j:
            rows[i].append(j)
    rows = [[r[0]] + sorted(r[1:]) for r in rows]
    row_starts = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    columns = np.concatenate([np.array(r, dtype=np.uint32) for r in rows])
    pairs = [(i, j) for i, r in enumerate(rows) for j in r]
    cij = np.array([c_acc[p] for p in pairs])
    mij = np.array([m_acc.get(p, 0.0) for p in pairs])
    minv = np.array([minv_acc.get(p, 0.0) for p in pairs])
    inc = np.array([inc_acc.get(p, 0.0) for p in pairs])
    mi = np.add.reduceat(mij, row_starts[:-1].astype(np.int64))
    b_i = np.flatnonzero(is_bdry).astype(np.uint32)
    b_normal = nrm[b_i] / np.linalg.norm(nrm[b_i], axis=1)[:, None]
    p_i, p_col, p_j = [], [], []
    for i in b_i:
        for col_idx, j in enumerate(rows[i]):
            if col_idx > 0 and is_bdry[j]:
                p_i.append(i), p_col.append(col_idx), p_j.append(j)
    off = OfflineView(dim, 0, 0, n, n, 1, row_starts, columns, cij, mij, mi, 1.0 / mi, mi.sum(), b_i, b_normal,
                      np.full(len(b_i), boundary_id, dtype=np.uint8), p_i, p_col, p_j)
    return off, positions, inc, minv, rows, is_bdry


@pytest.mark.parametrize("n_cells,h", [((7,), 1.0 / 7), ((5, 4), 0.2), ((3, 4, 2), 0.3), ((24, 24), 1.0 / 24)])
def test_dg_q1_offline_is_bit_for_bit_what_it_was(n_cells, h):
    new, info = dg_q1_offline(n_cells, h, capi.BC_SLIP)
    old, positions, inc, minv, rows, is_bdry = _dg_q1_offline_by_dictionaries(n_cells, h, capi.BC_SLIP)
    assert sorted(new._keep) == sorted(old._keep)
    for key in old._keep:
        assert new._keep[key].dtype == old._keep[key].dtype and np.array_equal(new._keep[key], old._keep[key]), key
    assert np.array_equal(new._dg[0], inc) and np.array_equal(new._dg[1], minv)
    assert np.array_equal(new.positions, positions) and new.measure_of_omega == old.measure_of_omega
    assert info["rows"] == rows and np.array_equal(info["is_bdry"], is_bdry) and info["n_per_cell"] == 2 ** len(n_cells)
    assert new.c.contents.discontinuous_ansatz == 1 and new.c.contents.n_bdry == old.c.contents.n_bdry


def test_element_matrices_of_degree_two():
    """M2, D2 and the weights against the integrals of the Lagrange polynomials on the nodes 0, 1/2, 1"""
    from numpy.polynomial import polynomial as P
    nodes = np.array([0.0, 0.5, 1.0])
    basis = [P.polyfromroots(np.delete(nodes, a)) / np.prod(nodes[a] - np.delete(nodes, a)) for a in range(3)]

    def integral(p):
        return P.polyval(1.0, P.polyint(p))
    for a in range(3):
        assert abs(integral(basis[a]) - ELEMENT_1D[2][2][a]) < 1e-15
        for b in range(3):
            assert abs(integral(P.polymul(basis[a], basis[b])) - M2[a, b]) < 1e-15
            assert abs(integral(P.polymul(basis[a], P.polyder(basis[b]))) - D2[a, b]) < 1e-15


MESHES = {"q1_3d": ((6, 6, 6), 1, 56), "q2_1d": ((64,), 2, 9), "q2_2d": ((12, 12), 2, 45), "q2_3d": ((4, 4, 4), 2, 189),
          "q1_2d_graded": ((9, 7), 1, 20)}


@pytest.mark.parametrize("key", sorted(MESHES))
def test_properties_of_the_assembled_matrices(key):
    n_cells, degree, widest = MESHES[key]
    dim = len(n_cells)
    h = tuple(graded(k, 1.6 + 0.3 * d) for d, k in enumerate(n_cells))
    start = time.perf_counter()
    off, info = dg_offline(n_cells, h, degree)
    assert time.perf_counter() - start < 2.0   # (measured: 0.2 s for the largest, 4^3 cells of degree 2)
    n, npc = off.n_owned, info["n_per_cell"]
    rs = off.row_starts.astype(np.int64)
    widths = np.diff(rs)
    cols = off.columns.astype(np.int64)
    rows = np.repeat(np.arange(n), widths)
    assert widths.max() == widest == off.max_row_len and npc == (degree + 1) ** dim
    assert (cols[rs[:-1]] == np.arange(n)).all() and all((np.diff(cols[rs[i] + 1:rs[i + 1]]) > 0).all() for i in range(n))
    # the inverse blocks times the cell mass blocks give the identity to round-off; the CSR entries are those blocks
    product = info["cell_mass_inverse"] @ info["cell_mass"]
    assert np.abs(product - np.eye(npc)).max() < 1e-12
    same_cell = rows // npc == cols // npc
    minv, inc = off._dg[1], off._dg[0]
    assert np.array_equal(minv[same_cell], info["cell_mass_inverse"][rows // npc, rows % npc, cols % npc][same_cell])
    assert np.array_equal(off.mij_csr[same_cell], info["cell_mass"][rows // npc, rows % npc, cols % npc][same_cell])
    assert not minv[~same_cell].any() and not off.mij_csr[~same_cell].any()
    # graded: no two cells alike
    volume = info["cell_mass"].sum(axis=(1, 2))
    assert len(np.unique(np.round(volume / volume.max(), 12))) == len(volume) == np.prod(n_cells)
    assert abs(off.mi.sum() - 1.0) < 1e-13 and (off.mi > 0).all()
    # sum_j c_ij = 0 away from the boundary, c_ij = -c_ji between rows away from the boundary
    sums = np.zeros((n, dim))
    np.add.at(sums, rows, off.cij_csr)
    interior = ~info["is_bdry"]
    assert np.abs(sums[interior]).max() < 1e-15
    key_of = rows * n + cols
    order = np.argsort(key_of)   # (within a row the diagonal comes first: not sorted as it stands)
    transposed = order[np.searchsorted(key_of[order], cols * n + rows)]
    assert np.array_equal(key_of[transposed], cols * n + rows)
    both = interior[rows] & interior[cols]
    assert np.abs(off.cij_csr + off.cij_csr[transposed])[both].max() < 1e-16
    # incidence against its closed form: between the two DoFs on the same node of a common face
    x = off.positions
    on_same_node = ~same_cell & (np.abs(x[rows] - x[cols]).max(axis=1) < 1e-14)
    assert np.array_equal(inc != 0.0, on_same_node) and np.array_equal(inc, inc[transposed])
    if degree == 1:
        assert (inc[on_same_node] == 1.0).all()
    else:
        closed = (0.5 * (off.mi[rows] + off.mi[cols]) / off.measure_of_omega) ** (0.5 / dim)
        np.testing.assert_allclose(inc[on_same_node], closed[on_same_node], rtol=1e-15)
        values = inc[on_same_node]
        assert values.max() < 1.0 and len(np.unique(values)) > 8   # fractional and non-uniform on the graded mesh


def test_uniform_and_graded_meshes_agree_where_the_widths_do():
    n_cells = (5, 3)
    a, _ = dg_offline(n_cells, 0.25, 2)
    b, _ = dg_offline(n_cells, (np.full(5, 0.25), np.full(3, 0.25)), 2)
    for key in a._keep:
        assert np.array_equal(a._keep[key], b._keep[key]), key
    assert np.array_equal(a._dg[0], b._dg[0]) and np.array_equal(a._dg[1], b._dg[1])
    np.testing.assert_allclose(a.positions, b.positions, rtol=0, atol=1e-15)


# ------------------------------------------------------------------ conservation of the oracle on the new stencils

@pytest.mark.parametrize("n_cells,degree,updates", [((8, 8, 8), 1, 2), ((48,), 2, 12), ((12, 12), 2, 3), ((4, 4, 4), 2, 1)])
def test_oracle_conserves_on_the_new_stencils(oracle, n_cells, degree, updates):
    """as test_oracle_conserves_on_a_dg_q1_stencil: mass, momentum and energy to round-off while the waves stay away from
    the (do-nothing) boundary; graded meshes"""
    dim = len(n_cells)
    off, info = dg_offline(n_cells, tuple(graded(k, 1.3) for k in n_cells), degree)
    p = oracle.default_params(capi.EQ_EULER, dim)
    p.cfl = 0.5
    m = HyperbolicModule(off, p, backend=oracle.backend())
    U0 = cases._euler_blast(0.5, radius=0.12 if degree == 1 else 0.15)(off)["U0"]
    a, b = m.new_state_vector(U0), m.new_state_vector()
    before = (off.mi[:, None] * U0).sum(0)
    for _ in range(updates):
        m.prepare_state_vector(a, 0.0)
        m.step(a, [], [], b)
        a, b = b, a
    U = a.download()
    assert np.isfinite(U).all() and U[:, 0].min() > 0.5
    assert np.abs(U - U0).max() > 1e-3
    assert np.abs(U - U0)[info["is_bdry"]].max() < 1e-12
    after = (off.mi[:, None] * U).sum(0)
    scale = (off.mi[:, None] * np.abs(U)).sum(0).max()
    assert np.abs(after - before).max() <= 1e-13 * scale, (after - before) / scale
    assert m.n_warnings() == 0


def test_synthetic_dg_matrices():
    """the incidence matrix is symmetric, in [0, 1], 0 on the diagonal; (M^-1)_ij is symmetric, and b_ij = m_i (M^-1)_ij
    is kappa_ij times the Neumann term -m_ij / m_j, kappa_ij in [0.5, 1.5]"""
    import helpers_row_width as rw
    off = cases.CASES["synthetic_euler_2d_65"]["mesh"]()
    tr = rw.transposed_entries(off)
    widths = rw.widths_of(off)
    rows, cols = np.repeat(np.arange(off.n_owned), widths), np.asarray(off.columns).astype(np.int64)
    inc, minv = off._dg
    diag = rows == cols
    assert np.array_equal(inc, inc[tr]) and not inc[diag].any() and 0.0 < inc[~diag].min() and inc.max() < 1.0
    mi = np.asarray(off.mi)
    np.testing.assert_allclose(minv, minv[tr], rtol=1e-14)   # b_ij of row i is b_ji of row j: P_ij = -P_ji
    assert np.array_equal(minv[diag], 1.0 / mi[rows[diag]])
    ratio = (mi[rows] * minv)[~diag] / (-np.asarray(off.mij) / mi[cols])[~diag]
    assert 0.5 <= ratio.min() < 0.6 and 1.4 < ratio.max() <= 1.5
    assert off.c.contents.discontinuous_ansatz == 1


# ------------------------------------------------------------------ what every case must show on the oracle alone

@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_the_oracle_alone_meets_the_conditions(oracle, name):
    """status 0 and no warning in the warm-up (develop asserts it) and in the compared update; the limiter coverage;
    both arms of the incidence fmax (degree 2, synthetic)"""
    case = cases.CASES[name]
    (off, dirichlet, states, weights, tau), alone = cases.developed(name, oracle)
    assert off.n_owned == case["n_points"] and off.max_row_len == case["width"]
    assert len(states) == 1 + case["stages"] and len(weights) == case["stages"]
    assert alone["status"] == 0 and alone["warnings"] == 0
    covered = cases.coverage(off, alone["lij_next"], case["width"])
    assert min(covered.values()) > 0, {k: v for k, v in covered.items() if v == 0}
    decides, loses = cases.incidence_arms(off, alone["alpha"])
    if case["incidence"]:
        assert decides > 0 and loses > 0, (decides, loses)
    else:   # dG-Q1: the incidence is 0 or 1 and alpha <= 1 -- a positive incidence cannot lose
        assert set(np.unique(off._dg[0])) == {0.0, 1.0} and loses == 0 and decides > 0
    if case["kind"] == "synthetic":   # every entry couples: the plain first and last column of every block
        for first in range(1, case["width"], cases.BLOCK):
            last = min(first + cases.BLOCK, case["width"]) - 1
            assert f"first column {first} of block {first}..{last}" in covered
            assert f"last column {last} of block {first}..{last}" in covered
        assert f"last column {case['width'] - 1} of a widest row" in covered


def test_structural_zeros_of_a_dg_stencil_are_never_limited(oracle):
    """why the conditions on single columns are stated for the structurally non-zero entries on a real dG stencil: where
    c_ij = m_ij = (M^-1)_ij = 0 the first-pass l_ij is exactly 1 in every case"""
    for name in ("euler_q1_3d", "euler_q2_3d", "sw_q2_2d"):
        (off, *_), alone = cases.developed(name, oracle)
        held = cases.structurally_nonzero(off)
        assert 0.2 < held.mean() < 0.8
        assert (alone["lij_next"][: len(held)][~held] == 1.0).all()


def test_unit_incidence_pairs_of_a_1d_dg_q1_stencil_are_never_limited(oracle):
    """why coverage() leaves the face pairs of dG-Q1 in one dimension out (helpers_dg_cases.can_be_limited): incidence 1,
    m_ij = (M^-1)_ij = 0 -- without stage vectors the oracle's P_ij is exactly 0 there and its first-pass l_ij exactly 1;
    they are the column positions 2 and 4, every other structurally non-zero entry stays in the condition; and no other
    1-D case of the table has such an entry"""
    import helpers_plan_cases as plan_cases
    name = "aeos_q1_1d"
    case = cases.CASES[name]
    (off, dirichlet, states, _, _), alone = cases.developed(name, oracle)
    widths, rs, rows, position = cases._pattern(off)
    left_out = cases.structurally_nonzero(off) & ~cases.can_be_limited(off)
    assert left_out.sum() == 2 * 63 and set(position[left_out]) == {2, 4} and (off._dg[0][left_out] == 1.0).all()
    m = HyperbolicModule(off, plan_cases.params_of(case, oracle, 1), backend=oracle.backend())
    old, new = m.new_state_vector(states[-1]), m.new_state_vector()
    m.prepare_state_vector(old, 0.0, dirichlet)
    m.step(old, [], [], new)
    pij = np.asarray(m.debug_fetch("pij")).reshape(rs[-1], -1)
    m.close()
    assert not pij[left_out].any() and np.abs(pij[cases.can_be_limited(off) & (position > 0)]).max() > 1.0
    assert (alone["lij_next"][: rs[-1]][left_out] == 1.0).all()
    for other in ("euler_q2_1d", "aeos_q2_1d", "synthetic_euler_1d_65"):
        mesh = cases.CASES[other]["mesh"]()
        assert np.array_equal(cases.can_be_limited(mesh), cases.structurally_nonzero(mesh)), other


@pytest.mark.parametrize("name", ["euler_q2_1d", "euler_q1_2d_checked", "euler_q1_3d", "sw_q1_2d_checked", "sw_q2_2d",
                                  "aeos_q1_2d", "aeos_q1_1d", "aeos_q2_1d", "synthetic_euler_1d_65", "synthetic_euler_2d_65",
                                  "synthetic_euler_3d_65", "synthetic_sw_2d_65"])
def test_the_dg_branch_is_in_effect(oracle, name):
    """once per Description and dimension: the same data with discontinuous_ansatz = 0 changes U_new by more than 1e-6 of
    its scale"""
    (developed, _) = cases.developed(name, oracle)
    assert cases.dg_branch_effect(cases.CASES[name], oracle, developed) > 1e-6


def test_boundary_cases_move_the_boundary_rows(oracle):
    for name in ("euler_q1_2d_slip", "euler_q1_2d_dirichlet"):
        (off, dirichlet, states, _, _), alone = cases.developed(name, oracle)
        assert (dirichlet is not None) == (name == "euler_q1_2d_dirichlet")
        moved = np.abs(alone["U"] - states[-1])[off.dg_info["is_bdry"]].max(axis=0)
        assert (moved > 1e-3 * np.abs(alone["U"]).max(axis=0))[[0, -1]].all(), moved


def test_the_table_holds_what_it_was_built_for():
    c = cases.CASES
    assert {name for name in c if c[name]["plan"]["wide"]} == {
        "euler_q2_3d", "synthetic_euler_1d_65", "synthetic_euler_2d_65", "synthetic_euler_2d_127", "synthetic_euler_2d_128",
        "synthetic_euler_2d_erk33_128", "synthetic_euler_3d_65", "synthetic_sw_2d_65"}
    assert all(case["plan"]["dg"] and case["plan"]["step5"] == "pij_lij" and case["plan"]["step4_stores_p"] and
               case["plan"]["step6"] == case["plan"]["step7"] == "high_order" for case in c.values())
    assert all(case["plan"]["step4_has_stages"] == (case["stages"] != 0) for case in c.values())
    for equation in ("euler", "shallow_water", "euler_aeos"):
        assert any(x["equation"] == equation and x["stages"] == 2 for x in c.values())
        assert any(x["equation"] == equation and x["plan"]["checked"] for x in c.values())
    assert c["euler_q2_3d"]["width"] == 3 * cases.BLOCK and c["euler_q1_3d"]["width"] == 56
    for mesh, width in cases.AEOS_REFUSED["meshes"].values():
        assert mesh().max_row_len == width > 32


# ------------------------------------------------------------------ several ranks

@pytest.mark.parametrize("name", sorted(cases.RANK_CASES))
def test_partitioned_oracle_reproduces_the_single_rank_oracle_on_dg_stencils(oracle, name):
    """the update of the owned rows to 1e-12 of the component's scale, tau to 1e-13; the literals of the table are those of
    the partition; the per-rank coverage of the ghost columns"""
    b = cases.built_ranks(name, oracle)
    single = b["single"]
    assert single["status"] == 0 and single["warnings"] == 0
    scale = np.abs(single["U"]).max(axis=0)
    assert len(b["views"]) == len(b["entry"]["ranks"]) <= 4
    for r, (v, x, (n_owned, n_export, launches)) in enumerate(zip(b["views"], b["ref"], b["entry"]["ranks"])):
        assert x["status"] == 0 and v.c.contents.discontinuous_ansatz == 1
        assert (np.abs(x["U"] - single["U"][v.global_ids[: v.n_owned]]) / scale).max() < 1e-12, r
        assert (v.n_owned, v.n_export) == (n_owned, n_export)
        n_slices, n_export_slices = (n_owned + 63) // 64, (n_export + 63) // 64
        assert [s for s, _, _ in launches] == [n_export_slices, n_slices - n_export_slices]
        widths = np.diff(np.asarray(v.row_starts).astype(np.int64))[:n_owned]
        assert widths.max() == b["case"]["width"]
        assert abs(x["tau"] - single["tau"]) <= 1e-13 * single["tau"]
    cases.assert_rank_coverage(name, b, b["ref"])
    if name == "aeos_q1_2d":   # one small rank
        assert b["entry"]["ranks"][0][0] < b["entry"]["ranks"][1][0] // 3
