"""The yardstick of tests/test_gpu_quantities.py (tests/helpers_quantities.py) and the host-side parts of the Quantities
feature, without a GPU: the helper against the reference's own space_averaged_time_series baseline, the trapezoid
rule, the first-call and clear rules, the file writers of ryujin_amd/quantities.py, the boundary mass of the synthetic
offline data and the ctypes declarations."""
import numpy as np
import pytest

import helpers_quantities as hq
from ryujin_amd import HyperbolicModule, TimeIntegrator, capi, offline, quantities
from ryujin_amd.initial_states import euler_uniform


def test_helper_reproduces_the_mass_conservation_golden(oracle, golden_dir):
    """tests/euler/check-mass-conservation_01 (interior manifolds = interior : 0. : space_averaged): the golden file IS
    the space_averaged_time_series of Quantities. Oracle states, the helper's accumulate after every step; the
    tolerances are those of test_oracle_golden_integration.test_mass_conservation_01_golden."""
    from test_oracle_golden_integration import golden_mass_conservation
    gold = golden_mass_conservation(golden_dir)
    assert gold.shape == (19, 9)
    off = offline.SyntheticOffline(offline.rectangle_2d(64, (0.0, 0.0), (20.0, 20.0)))
    m = HyperbolicModule(off, equation=capi.EQ_EULER, backend=oracle.backend())
    lengths = np.diff(off.row_starts.astype(np.int64))
    index = quantities.select_interior_points(0.0, off.positions, lengths, off.n_owned)
    assert np.array_equal(index, np.arange(off.n_owned))  # no constrained rows: the whole interior
    stats = hq.Statistics(capi.EQ_EULER, 2, m.params, index, off.mi[index])
    sv = m.new_state_vector(euler_uniform(off.positions))
    ti = TimeIntegrator(m, "ssprk 33", cfl_min=0.9, cfl_max=0.9, cfl_recovery_strategy="none")
    t = 0.0
    for _ in range(19):
        stats.accumulate(sv.download(), t)
        sv, tau = ti.step(sv, t)
        t += tau
    got = stats.series_array()
    np.testing.assert_allclose(got[:, 0], gold[:, 0], rtol=0, atol=5e-14)
    np.testing.assert_allclose(got[:, [1, 2, 4]], gold[:, [1, 2, 4]], rtol=0, atol=1e-13)
    np.testing.assert_allclose(got[:, 3], gold[:, 3], rtol=0, atol=1e-15)
    np.testing.assert_allclose(got[:, [5, 6, 8]], gold[:, [5, 6, 8]], rtol=2e-14, atol=0)
    np.testing.assert_allclose(got[:, 7], gold[:, 7], rtol=1e-7, atol=1e-18)
    m.close()


def _scalar_stats(n=7):
    index = np.arange(n)[::-1].copy()
    weight = np.linspace(0.5, 2.0, n)
    return hq.Statistics(capi.EQ_SCALAR_CONSERVATION, 1, None, index, weight)


def test_trapezoid_rule_is_exact_for_values_linear_in_t():
    stats = _scalar_stats()
    a, b = np.linspace(-1.0, 2.0, 7), np.linspace(0.25, 3.0, 7)
    times = [0.5, 0.625, 1.0, 1.03125, 2.5, 2.75, 4.0]
    for t in times:
        stats.accumulate((a + b * t).reshape(-1, 1), t)
    values, t_begin, t_end = stats.time_averaged()
    assert t_begin == times[0] and t_end == times[-1]
    exact = (a + b * 0.5 * (times[0] + times[-1]))[stats.index]
    assert np.abs(values[:, 0] - exact).max() <= 2 * len(times) * hq.EPS * np.abs(a + b * times[-1]).max()
    # and the second moment is the trapezoid sum of the squares, not the square of the mean
    x = np.array([(a + b * t)[stats.index] ** 2 for t in times])
    tau = np.diff(times)
    trapezoid = (0.5 * tau[:, None] * (x[:-1] + x[1:])).sum(axis=0) / (times[-1] - times[0])
    np.testing.assert_allclose(values[:, 1], trapezoid, rtol=1e-14)
    assert (values[:, 1] > exact ** 2).all()


@pytest.mark.parametrize("t0", [0.0, 1.0, 0.375])
def test_first_call_accumulates_nothing_also_when_the_run_starts_at_zero(t0):
    stats = _scalar_stats()
    U = np.linspace(1.0, 2.0, 7).reshape(-1, 1)
    assert stats.time_averaged() is None
    stats.accumulate(U, t0)
    assert stats.time_averaged() is None and (stats.val_sum == 0.0).all()
    assert (stats.t_old, stats.t_new, stats.t_sum) == (t0 - 1.0, t0, 0.0)
    assert len(stats.series) == 1 and stats.series[0][0] == t0
    stats.accumulate(3.0 * U, t0 + 0.5)
    values, t_begin, t_end = stats.time_averaged()
    assert (t_begin, t_end) == (t0, t0 + 0.5)
    np.testing.assert_allclose(values[:, 0], 2.0 * U[stats.index, 0], rtol=1e-15)
    # the mean is the weighted one, in manifold order
    w = stats.weight
    assert abs(stats.series[1][1] - (w * 3.0 * U[stats.index, 0]).sum() / w.sum()) < 1e-14


def test_clear_restarts_the_statistics_and_the_series():
    stats = _scalar_stats()
    U = np.ones((7, 1))
    for t in (0.0, 0.1, 0.4):
        stats.accumulate(U, t)
    assert stats.t_sum == pytest.approx(0.4) and len(stats.series) == 3
    stats.clear()
    assert stats.time_averaged() is None and stats.series == []
    stats.accumulate(2.0 * U, 0.7)
    assert stats.time_averaged() is None  # the first call after a clear adds nothing again
    stats.accumulate(2.0 * U, 0.9)
    values, t_begin, t_end = stats.time_averaged()
    assert t_begin == pytest.approx(0.7) and t_end == 0.9 and np.allclose(values[:, 0], 2.0)


def test_empty_manifold_gives_the_reference_nan():
    stats = hq.Statistics(capi.EQ_EULER, 2, capi.Params(), np.zeros(0, dtype=np.int64), np.zeros(0))
    stats.accumulate(np.ones((3, 4)), 0.25)
    row = stats.series_array()[0]
    assert row[0] == 0.25 and np.isnan(row[1:]).all()


def test_chain_length_stays_within_the_function_level_at_full_size():
    D = hq.chain_length([2_500_000])
    assert D == 10 + 6 + 4 + 16 + 6 + 1
    assert D * hq.EPS <= hq.FUNCTION_LEVEL
    assert hq.chain_length([100, 0, 100]) == 1 + 6 + 4 + 1 + 6 + 3


# ---------------------------------------------------------------------------------------------- file writers

def _parse(text):
    """(comment lines, per rank [rows of tab-separated groups of floats])"""
    comments, ranks = [], []
    for line in text.splitlines():
        if line.startswith("# rank "):
            assert int(line[7:]) == len(ranks)
            ranks.append([])
        elif line.startswith("#"):
            comments.append(line)
        else:
            ranks[-1].append([[float(x) for x in group.split(" ")] for group in line.split("\t")])
    return comments, ranks


def test_header_from_the_primitive_component_names():
    assert quantities.header(capi.EQ_EULER, 2) == "primitive state (rho, v_1, v_2, p)\t and 2nd moments\n"
    assert quantities.header(capi.EQ_EULER_AEOS, 1) == "primitive state (rho, v, e)\t and 2nd moments\n"
    assert quantities.header(capi.EQ_SHALLOW_WATER, 2) == "primitive state (h, v_1, v_2)\t and 2nd moments\n"
    assert quantities.header(capi.EQ_SCALAR_CONSERVATION, 3) == "primitive state (u)\t and 2nd moments\n"


def test_time_series_file_matches_the_golden_text(golden_dir):
    """the writer reproduces the reference's own file: header line and every row, character by character"""
    import os
    lines = [line for line in open(os.path.join(golden_dir, "euler_check-mass-conservation_01.output"))
             if not line.startswith("[INFO]")]
    rows = np.array([[float(x) for x in line.split()] for line in lines[1:]])
    head = quantities.header(capi.EQ_EULER, 2)
    assert quantities.format_time_series(head, rows, append=False) == "".join(lines)
    assert quantities.format_time_series(head, rows[5:], append=True) == "".join(lines[6:])
    assert quantities.format_time_series(head, rows[:0], append=True) == ""


def test_value_files_stamps_rank_sections_and_numbers():
    rng = np.random.default_rng(3)
    per_rank = [rng.normal(size=(4, 8)) * 10.0 ** rng.integers(-20, 20, size=(4, 8)), np.zeros((0, 8)),
                rng.normal(size=(2, 8))]
    head = quantities.header(capi.EQ_EULER, 2)
    text = quantities.format_values(quantities.instantaneous_stamp(0.125), head, per_rank)
    assert text.startswith("# at t = 1.25000000000000e-01\n# primitive state (rho, v_1, v_2, p)\t and 2nd moments\n# rank 0\n")
    comments, ranks = _parse(text)
    assert len(comments) == 2 and [len(r) for r in ranks] == [4, 0, 2]
    for values, rows in zip(per_rank, ranks):
        for v, (state, square) in zip(values, rows):
            assert len(state) == 4 and len(square) == 4
            np.testing.assert_allclose(state + square, v, rtol=5e-15)  # 15 significant digits
    # the time-averaged stamp and the scale of internal_write_out
    text = quantities.format_values(quantities.time_averaged_stamp(0.5, 2.0), head, per_rank[:1], scale=0.25)
    assert text.startswith("# averaged from t = 5.00000000000000e-01 to t = 2.00000000000000e+00\n# primitive")
    _, ranks = _parse(text)
    np.testing.assert_allclose(ranks[0][0][0] + ranks[0][0][1], 0.25 * per_rank[0][0], rtol=5e-15)
    assert "e+00" in text and "E" not in text.split("\n", 2)[2]


def test_points_files():
    pos = np.array([[0.0, 1.5], [2.0, 3.25]])
    text = quantities.format_interior_points([(pos, np.array([0.5, 0.125])), (pos[:0], np.zeros(0))])
    assert text == ("#\n# position\tinterior mass\n# rank 0\n"
                    "0.00000000000000e+00 1.50000000000000e+00\t5.00000000000000e-01\n"
                    "2.00000000000000e+00 3.25000000000000e+00\t1.25000000000000e-01\n# rank 1\n")
    text = quantities.format_boundary_points([(pos[:1], np.array([[0.0, -1.0]]), np.array([0.5]), np.array([0.25]))])
    assert text == ("#\n# position\tnormal\tnormal mass\tboundary mass\n# rank 0\n"
                    "0.00000000000000e+00 1.50000000000000e+00\t0.00000000000000e+00 -1.00000000000000e+00\t"
                    "5.00000000000000e-01\t2.50000000000000e-01\n")


def test_options_and_point_selection():
    assert quantities.parse_options("time_averaged space_averaged") == capi.Q_TIME_AVERAGED | capi.Q_SPACE_AVERAGED
    assert quantities.parse_options("instantaneous") == capi.Q_INSTANTANEOUS
    assert quantities.parse_options(5) == 5
    off = offline.SyntheticOffline(offline.rectangle_2d(8, (0.0, 0.0), (2.0, 1.0)))
    lengths = np.diff(off.row_starts.astype(np.int64))
    # a line-out on the mesh line y = 0.5, ascending local index
    line = quantities.select_interior_points(lambda x: x[:, 1] - 0.5, off.positions, lengths, off.n_owned)
    assert len(line) == 9 and (np.diff(line.astype(np.int64)) > 0).all()
    assert np.allclose(off.positions[line, 1], 0.5)
    # the lower boundary, in the order of the boundary map: the two corners appear once per face they lie on
    lower = quantities.select_boundary_entries(lambda x: x[:, 1], off.b_i, off.b_positions, off.n_owned)
    assert (np.diff(lower) > 0).all() and np.allclose(off.b_positions[lower, 1], 0.0)
    assert len(lower) == 9 + 2 and len(set(off.b_i[lower].tolist())) == 9


# ---------------------------------------------------------------------------------------------- boundary mass

def test_boundary_mass_of_a_rectangle_sums_to_its_perimeter():
    off = offline.SyntheticOffline(offline.rectangle_2d(8, (0.0, 0.0), (2.0, 1.0), ny=5))
    b_mass = off.b_mass
    assert b_mass.shape == (off.n_bdry,) and (b_mass > 0).all()
    assert abs(b_mass.sum() - 6.0) < 1e-14
    # a corner node has one entry per face it lies on, each with that face's share: half a cell edge
    hx, hy = 2.0 / 8, 1.0 / 5
    corner = np.flatnonzero((np.abs(off.b_positions[:, 0]) < 1e-14) & (np.abs(off.b_positions[:, 1]) < 1e-14))
    assert len(corner) == 2 and len(set(off.b_i[corner].tolist())) == 1
    normals = off.b_normal[corner]
    shares = {(round(n[0]), round(n[1])): m for n, m in zip(normals, b_mass[corner])}
    assert shares[(-1, 0)] == pytest.approx(0.5 * hy, rel=1e-15) and shares[(0, -1)] == pytest.approx(0.5 * hx, rel=1e-15)
    # an edge node: two half edges of its face
    edge = np.flatnonzero((np.abs(off.b_positions[:, 1]) < 1e-14) & (np.abs(off.b_positions[:, 0] - 1.0) < 1e-14))
    assert len(edge) == 1 and b_mass[edge[0]] == pytest.approx(hx, rel=1e-15)


def test_boundary_mass_of_a_box_sums_to_its_surface_area():
    off = offline.SyntheticOffline(offline.box_3d(4, (0.0, 0.0, 0.0), (1.0, 2.0, 3.0)))
    assert abs(off.b_mass.sum() - 2.0 * (2.0 + 3.0 + 6.0)) < 1e-13
    corner = np.flatnonzero(np.abs(off.b_positions).max(axis=1) < 1e-14)
    assert len(corner) == 3 and len(set(off.b_i[corner].tolist())) == 1
    h = np.array([1.0, 2.0, 3.0]) / 4
    for e in corner:
        d = int(np.abs(off.b_normal[e]).argmax())  # the face normal to direction d: a quarter of a cell face
        assert off.b_mass[e] == pytest.approx(0.25 * np.prod(np.delete(h, d)), rel=1e-15)


def test_ctypes_mirror_knows_the_quantities_block():
    for name in ("add_manifold", "reset", "clear_statistics", "accumulate", "instantaneous", "time_averaged",
                 "time_series"):
        assert "ryujin_hip_quantities_" + name in capi.HIP_SYMBOLS
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ryujin_hip.h")).read()
    flags = re.search(r"RYUJIN_Q_INSTANTANEOUS = (\d+), RYUJIN_Q_TIME_AVERAGED = (\d+), RYUJIN_Q_SPACE_AVERAGED = (\d+)", text)
    assert tuple(int(g) for g in flags.groups()) == (capi.Q_INSTANTANEOUS, capi.Q_TIME_AVERAGED, capi.Q_SPACE_AVERAGED)
    assert int(re.search(r"#define RYUJIN_Q_MAX_MANIFOLDS (\d+)", text).group(1)) == capi.Q_MAX_MANIFOLDS
    assert int(re.search(r"#define RYUJIN_Q_NONE_YET (\d+)", text).group(1)) == capi.Q_NONE_YET
