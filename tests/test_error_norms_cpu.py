"""The host-side parts of the device-resident compute_error() (ryujin_hip_error_norms_*), without a GPU: the entry
points and their ctypes declarations, the generator's cell list against the offline data's own lumped mass, q1_jxw on
skewed quadrilaterals and hexahedra against those meshes' lumped mass, and the writer of the reference's log block
read back by golden() of tests/test_oracle_golden_verification.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers_error_norms as hen
import helpers_q1_quads as hq1
from ryujin_amd import HyperbolicModule, capi, error_norms, offline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_exported_and_declared():
    for name in ("ryujin_hip_error_norms_configure", "ryujin_hip_error_norms_compute"):
        assert name in capi.HIP_SYMBOLS
    lib = capi.load_hip()
    assert len(lib.ryujin_hip_error_norms_configure.argtypes) == 9
    assert len(lib.ryujin_hip_error_norms_compute.argtypes) == 8
    synth = capi.load_synth()
    assert synth.ryujin_synth_n_cells.restype is C.c_uint64 and synth.ryujin_synth_cells.restype is capi.c_u32_p
    text = open(os.path.join(ROOT, "include", "ryujin_hip.h")).read()
    for macro, value in (("RYUJIN_EN_MAX_DOFS_PER_CELL", capi.EN_MAX_DOFS_PER_CELL),
                         ("RYUJIN_EN_MAX_POINTS", capi.EN_MAX_POINTS),
                         ("RYUJIN_EN_MAX_COMPONENTS", capi.EN_MAX_COMPONENTS)):
        assert int(re.search(rf"#define {macro} (\d+)", text).group(1)) == value
    synth_header = open(os.path.join(ROOT, "include", "ryujin_synth.h")).read()
    assert "ryujin_synth_n_cells" in synth_header and "ryujin_synth_cells" in synth_header


def test_q1_tables_are_a_partition_of_unity_with_unit_weight():
    for dim in (1, 2, 3):
        shape, weights = error_norms.q1_tables(dim)
        assert shape.shape == (3 ** dim, 2 ** dim) and weights.shape == (3 ** dim,)
        assert np.abs(shape.sum(axis=1) - 1.0).max() < 4e-16 and abs(weights.sum() - 1.0) < 4e-16
        assert (shape > 0.0).all()
    # vertex order v = ix + 2 iy, x running fastest over the points: the first point is next to vertex 0, the third
    # next to vertex 1, the seventh next to vertex 2
    shape, _ = error_norms.q1_tables(2)
    assert [int(shape[q].argmax()) for q in (0, 2, 6, 8)] == [0, 1, 2, 3]


MESHES = {
    "rectangle_2d": lambda **kw: offline.rectangle_2d(7, **kw),
    "mach3_step_2d": lambda **kw: offline.mach3_step_2d(5, **kw),  # the smallest grid-aligned step
    "box_3d": lambda **kw: offline.box_3d(4, **kw),
    "interval": lambda **kw: offline.MeshSpec(1, (17,), (0.0,), (1.0,), (capi.BC_SLIP, capi.BC_SLIP), **kw),
}


@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_generator_cells_reproduce_measure_and_lumped_mass(mesh):
    off = offline.SyntheticOffline(MESHES[mesh]())
    cells = off.cells
    assert cells.shape == (off.n_cells, 2 ** off.dim) and cells.max() < off.n_relevant
    shape, weights = error_norms.q1_tables(off.dim)
    affine = np.outer(np.full(len(cells), off.cell_measure), weights)
    general = error_norms.q1_jxw(off.positions, cells)
    for jxw in (affine, general):
        assert abs(jxw.sum() - off.measure_of_omega) <= 1e-13 * off.measure_of_omega
        m = hen.nodal_scatter(off.n_relevant, cells, shape, jxw)
        # pins vertex order and cell assignment against data the project already trusts
        assert np.abs(m - off.mi).max() <= 1e-13 * off.mi.max()


def _partitionable(mesh, **kw):
    """box_3d(4) has five node planes and the generator's slab partition keeps at least two per rank: over three ranks
    the box is six cells long in x (seven planes), still four cells in y and z"""
    if mesh == "box_3d":
        return offline.box_3d(4, nx=6, **kw)
    return MESHES[mesh](**kw)


@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_generator_cells_over_three_ranks(mesh):
    single = offline.SyntheticOffline(_partitionable(mesh))
    key = lambda part: np.sort(part.global_ids[part.cells.astype(np.int64)], axis=1)  # noqa: E731
    seen = []
    for rank in range(3):
        part = offline.SyntheticOffline(_partitionable(mesh, n_ranks=3, rank=rank))
        assert part.n_cells > 0 and part.cells.max() < part.n_relevant
        # each cell is owned by the rank that owns its vertex of smallest global id: the first one
        assert (part.cells[:, 0] < part.n_owned).all()
        assert (part.global_ids[part.cells.astype(np.int64)].argmin(axis=1) == 0).all()
        seen.append(key(part))
    seen = np.concatenate(seen)
    expected = key(single)
    assert len(seen) == len(expected) == single.n_cells
    order = lambda a: a[np.lexsort(a.T[::-1])]  # noqa: E731
    assert np.array_equal(order(seen), order(expected))  # every global cell exactly once


def test_q1_jxw_on_skewed_quadrilaterals():
    points, quads, edges = hq1.annulus_mesh(4, 12)
    off, info = hq1.q1_quads_offline(points, quads, edges)
    cells = hen.lexicographic_quads(quads)
    shape, _ = error_norms.q1_tables(2)
    jxw = error_norms.q1_jxw(points, cells)
    assert (jxw > 0.0).all() and np.ptp(jxw / jxw.mean(axis=1, keepdims=True)) > 1e-2  # not affine
    m = hen.nodal_scatter(len(points), cells, shape, jxw)
    assert np.abs(m - off.mi).max() <= 1e-13 * off.mi.max()
    assert abs(jxw.sum() - info["area"]) <= 1e-13 * info["area"]


def test_q1_jxw_on_skewed_hexahedra():
    points, hexes, faces = hq1.annulus_mesh_3d(3, 8, 2)
    off, info = hq1.q1_hexes_offline(points, hexes, faces)
    shape, _ = error_norms.q1_tables(3)
    jxw = error_norms.q1_jxw(points, hexes)
    assert (jxw > 0.0).all()
    m = hen.nodal_scatter(len(points), hexes, shape, jxw)
    assert np.abs(m - off.mi).max() <= 1e-13 * off.mi.max()
    assert abs(jxw.sum() - info["volume"]) <= 1e-13 * info["volume"]


@pytest.mark.parametrize("normalize", [True, False])
def test_log_block_is_read_back_by_golden(tmp_path, normalize):
    from test_oracle_golden_verification import golden
    values = (1089, 2.000123456789012345, 0.0123456789012345678, 3.4567890123456789e-05, 1.0 / 3.0)
    error_norms.write_error_block(str(tmp_path / "run.log"), *values, normalize=normalize)
    text = open(tmp_path / "run.log").read()
    first = "Normalized consolidated" if normalize else "Consolidated"
    assert f"\n{first} Linf, L1, and L2 errors at final time \n" in text
    lines = [line[:8] for line in text.splitlines() if " = " in line]
    assert lines == ["#dofs = ", "t     = ", "Linf  = ", "L1    = ", "L2    = "]
    got = golden(str(tmp_path), "run.log")
    assert got[0] == values[0]
    for g, v in zip(got[1:], values[1:]):
        assert g == float(f"{v:.16g}") and abs(g - v) <= 5e-16 * abs(v)  # 16 significant digits, round-tripped
    # the same numbers the reference's own baseline holds are written the way it writes them
    assert "L2    = 0.3333333333333333\n" in text


def test_other_backends_refuse(oracle):
    off = offline.SyntheticOffline(offline.rectangle_2d(4))
    m = HyperbolicModule(off, equation=capi.EQ_EULER, backend=oracle.backend())
    shape, weights = error_norms.q1_tables(2)
    with pytest.raises(NotImplementedError):
        m.error_norms_configure(off.cells, shape, np.full(off.n_cells, off.cell_measure), weights)
    with pytest.raises(NotImplementedError):
        m.compute_error(m.new_state_vector(np.ones((off.n_relevant, 4))), 0.0)
    m.close()


def test_chain_length_follows_the_launch_shape():
    assert hen.chain_length([17], 3) == 3 + 1 + 6 + 4 + 1 + 6 + 1
    assert hen.chain_length([1200, 0, 300], 9) == 9 + 1 + 6 + 4 + 1 + 6 + 3
    assert hen.chain_length([2_500_000], 9) == 9 + 10 + 6 + 4 + 16 + 6 + 1
