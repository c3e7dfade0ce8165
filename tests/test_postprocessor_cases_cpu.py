"""CPU: (1) the numpy restatement of Postprocessor::compute() (tests/helpers_postprocessor.py) on meshes that are not
lattices, pinned by exact identities -- for continuous P1 elements and an interior node i, sum_j c_ij q_j = m_i grad q
for a linear q --, not by another restatement; (2) the case table of tests/test_gpu_postprocessor_meshes.py
(tests/helpers_postprocessor_cases.py): its literals against the meshes, and that no GPU case is vacuous."""
import numpy as np
import pytest

import helpers_postprocessor as hp
import helpers_postprocessor_cases as pc
from ryujin_amd import capi

A2, A3 = np.array([0.7, -1.3]), np.array([0.7, -1.3, 0.4])   # not axis-aligned
OMEGA2, OMEGA3 = -0.8, np.array([0.3, -0.5, 0.9])


def _identity_fields(which):
    off, info = pc.p1(which)
    dim = off.dim
    a, omega = (A2, OMEGA2) if dim == 2 else (A3, OMEGA3)
    U = pc.linear_density_rigid_rotation(off.positions, a, 3.0, omega)
    p = pc.params("euler", dim)
    quantities, names = hp.resolve(capi.EQ_EULER, dim, ("rho",), ("v_1",))
    raw, scale = hp.raw_values(off, U, quantities, capi.EQ_EULER, p)
    rows = pc.interior_rows(info)
    assert 0 < len(rows) < off.n_owned
    return off, rows, raw, hp.raw_tolerance(scale), np.linalg.norm(a), omega


@pytest.mark.parametrize("which", ["disk", "ball"])
def test_schlieren_of_a_linear_density_on_p1(which):
    """rho = a . x + b: |a| at every non-boundary row, to the per-row tolerance of the restatement"""
    off, rows, raw, tol, a_norm, _ = _identity_fields(which)
    err = np.abs(raw[0] - a_norm)
    print(f"{which}: schlieren identity max err / tol {(err[rows] / tol[0][rows]).max():.3f}")
    assert (err[rows] <= tol[0][rows]).all()
    # (c_ij = int phi_i grad phi_j carries no boundary term: sum_j c_ij q_j = int phi_i grad q on the boundary rows too)
    assert (err <= tol[0]).all()


def test_signed_vorticity_of_a_rigid_rotation_on_the_p1_disk():
    """v = omega (-y, x): 2 omega, SIGNED, at every non-boundary row; v is a primitive state here (m = rho v)"""
    off, rows, raw, tol, _, omega = _identity_fields("disk")
    err = np.abs(raw[1] - 2.0 * omega)
    print(f"disk: vorticity identity max err / tol {(err[rows] / tol[1][rows]).max():.3f}")
    assert omega < 0.0 and (err[rows] <= tol[1][rows]).all()


def test_vorticity_norm_of_a_rigid_rotation_on_the_p1_ball():
    """v = w x x: |curl v| = 2 |w| at every non-boundary row"""
    off, rows, raw, tol, _, omega = _identity_fields("ball")
    err = np.abs(raw[1] - 2.0 * np.linalg.norm(omega))
    print(f"ball: vorticity identity max err / tol {(err[rows] / tol[1][rows]).max():.3f}")
    assert (err[rows] <= tol[1][rows]).all()


def test_the_tolerance_is_the_old_one_up_to_450_entries():
    """max(1e-13, 2 W u) sum_j |c_ij| |q_j| / m_i: bit for bit 1e-13 x the row magnitude up to 450 entries, the forward
    bound of recursive summation on both sides above"""
    for name, exact in (("A_euler_3d_3x3x3", True), ("D_q2_3d_3", True), ("C_euler_2d_1023", False)):
        off = pc.mesh(name)
        _, _, raw, scale, widths = pc.reference(name)
        rows, cols, c, mi, _ = hp.csr(off)
        U = pc.case_state(name)
        plain = np.bincount(rows, weights=np.sqrt((c * c).sum(axis=1)) * np.abs(U[cols, 0]), minlength=off.n_owned) / mi
        if exact:
            assert widths.max() <= 450 and np.array_equal(hp.raw_tolerance(scale[0]), 1e-13 * plain)
        else:
            factor = hp.raw_tolerance(scale[0]) / plain
            np.testing.assert_allclose(factor, np.maximum(1e-13, widths * hp.EPS), rtol=1e-12)
            assert factor[widths == 1023][0] == pytest.approx(1023 * 2.0 ** -52) and factor.min() >= 1e-13


# ------------------------------------------------------------------ the case table

@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_case_literals_and_not_vacuous(name):
    """The literals of the table against the mesh. Then, on the numpy raw field of every requested quantity:
    q_max > q_min, a value above its own tolerance in rows of every width that occurs (rows of length 1 give 0 by
    definition), both signs for the signed 2-D vorticity. The single-cell meshes are exempt BY NAME."""
    case, off = pc.CASES[name], pc.mesh(name)
    _, names, raw, scale, widths = pc.reference(name)
    assert (off.n_owned, int(widths.max()), (off.n_owned + 63) // 64) == (case["n_owned"], case["width"], case["n_slices"])
    if "widths" in case:
        assert tuple(np.unique(widths)) == case["widths"]
    assert np.isfinite(raw).all()
    if name in pc.SINGLE_CELL:
        assert off.n_owned == 2 ** off.dim
        return
    for k, quantity in enumerate(names):
        tol = hp.raw_tolerance(scale[k])
        q_max, q_min = hp.bounds(raw[k])
        d_max, d_min = hp.bounds_tolerance(raw[k], scale[k])
        assert q_max - q_min > 1e3 * (d_max + d_min), (quantity, q_max, q_min)
        for w in np.unique(widths):
            if w > 1:
                assert (np.abs(raw[k][widths == w]) > 1e3 * tol[widths == w]).any(), (quantity, int(w))
        if off.dim == 2 and quantity.startswith("vorticity"):
            assert (raw[k] > tol).any() and (raw[k] < -tol).any(), quantity
    if "cut" in case:   # family G: the cut rows give 0 and hold q_min
        assert (widths[list(case["cut"])] == 1).all() and (widths == 1).sum() == len(case["cut"])
        assert (raw[:, list(case["cut"])] == 0.0).all() and all(hp.bounds(r)[1] == 0.0 for r in raw)
        assert 63 in case["cut"] and off.n_owned - 1 in case["cut"]
        assert (widths[:63] > 1).all()   # 63 ends a slice that is otherwise full
    if case.get("dry"):   # dry nodes with and without a residual momentum, next to wet ones
        U = pc.case_state(name)
        assert ((U[:, 0] == 0.0) & (U[:, 1] != 0.0)).any() and ((U[:, 0] == 0.0) & (U[:, 1] == 0.0)).any()
        assert (U[:, 0] > 0.0).any()


def test_a_positive_q_min_where_the_last_slice_is_partial():
    """a fold that lets a lane beyond n_owned into q_min shows only where the true q_min is positive: some case of
    every family with a partial last slice has one (family G holds q_min = 0 by construction)"""
    seen = {}
    for name, case in pc.CASES.items():
        if case["n_owned"] % 64 and name not in pc.SINGLE_CELL:
            _, names, raw, scale, _ = pc.reference(name)
            positive = [hp.bounds(raw[k])[1] > hp.bounds_tolerance(raw[k], scale[k])[1] for k in range(len(names))]
            seen[case["family"]] = seen.get(case["family"], False) or any(positive)
    assert seen == {"A": True, "D": True, "E": True, "G": False}, seen


def test_layout_switch_and_rank_tables():
    import helpers_small_meshes as sm
    for name in pc.LAYOUT_SWITCH_CASES:   # family B: the meshes of helpers_small_meshes and three cases of this table
        assert (name in sm.CASES) != (name in pc.CASES)
    assert set(sm.LAYOUT_SWITCH_CASES) <= set(pc.LAYOUT_SWITCH_CASES)
    assert max(pc.CASES[n]["n_slices"] for n in pc.LAYOUT_SWITCH_CASES if n in pc.CASES) >= 4 * 5 + 1   # a band of stride 5
    for name, (n_ranks, n_owned, most_neighbours) in pc.RANK_CASES.items():
        single, parts, _ = pc.rank_case(name)
        assert len(parts) == n_ranks and tuple(p.n_owned for p in parts) == n_owned
        assert sum(n_owned) == single.n_owned and all(p.n_relevant > p.n_owned for p in parts)
        assert max(int(p.c.contents.n_nbr) for p in parts) == most_neighbours
        rows = np.concatenate([pc.global_rows(single, p) for p in parts])
        assert np.array_equal(np.sort(rows), np.arange(single.n_owned))
    # the sectors: a rank with more than two neighbours, a node exported to more than one of them
    _, parts, _ = pc.rank_case("F_disk_sectors")
    assert any(len(p._keep["send_idx"]) > len(set(p._keep["send_idx"].tolist())) for p in parts)
    # the slabs: a rank of fewer than 64 rows that exports all of them
    _, parts, _ = pc.rank_case("F_plane_7x7_of_4")
    assert any(p.n_export == p.n_owned < 64 for p in parts)


def test_the_one_sided_cut_is_not_symmetric():
    """what family G cannot load (see helpers_postprocessor_cases): the neighbours of a cut row keep its column"""
    base = pc.p1("disk")[0]
    one_sided, both = pc.cut_rows(base, pc.CUT_DISK, one_sided=True), pc.cut_rows(base, pc.CUT_DISK)
    assert (hp.csr(one_sided)[1] == 63).sum() > 1 and (hp.csr(both)[1] == 63).sum() == 1
