"""The lattice generator with a prescribed widest row (tests/helpers_row_width.py) and the case table built on it
(tests/helpers_row_width_cases.py), on the CPU: the properties step() relies on, the round trip of every case's pattern
through the device layout (ryujin_hip_debug_layout: host code, no GPU), and the coverage condition of every case
evaluated on the oracle -- the GPU test (tests/test_gpu_row_widths.py) asserts it again on the same data."""
import numpy as np
import pytest

import helpers_row_width as rw
import helpers_row_width_cases as cases
from ryujin_amd import capi

MESHES = {}   # one mesh per (shape, width): the cases share them


def _mesh(name):
    case = cases.CASES[name]
    key = (case["n_points"], case["width"], name.split("_")[1])
    if key not in MESHES:
        MESHES[key] = case["mesh"]()
    return MESHES[key]


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_generated_offline_data_is_consistent(name):
    """c_ij = -c_ji, c_ii = 0, m_ij = m_ji > 0, m_i = sum_j m_ij, columns sorted behind the diagonal; the widest row
    has exactly the prescribed width and no row fewer than 3 entries; rows of the widest width in at least two slices,
    next to narrower rows; far columns weigh as much as near ones"""
    case = cases.CASES[name]
    off = _mesh(name)
    assert off.n_owned == case["n_points"] and off.max_row_len == case["width"]
    widths = rw.check_consistency(off, case["width"])
    assert (widths >= 3).all()
    rs = off.row_starts.astype(np.int64)
    diag = np.zeros(rs[-1], dtype=bool)
    diag[rs[:-1]] = True
    c_norm = np.linalg.norm(off.cij[~diag], axis=1)
    # (the same order of magnitude: |c0_ij| is one number; the correction that removes the row sums spreads it)
    assert c_norm.max() <= 10.0 * np.median(c_norm) and np.percentile(c_norm, 5) >= 0.1 * np.median(c_norm)
    assert off.mij[~diag].max() <= 1.5 * off.mij[~diag].min()


def test_half_space_offsets_are_a_half_space_ordered_by_length():
    for dim, count in ((1, 5), (2, 63), (2, 511), (3, 63)):
        d = rw.half_space_offsets(dim, count)
        both = np.concatenate([d, -d])
        assert len(np.unique(both, axis=0)) == 2 * count          # no vector with its negative, none twice
        assert (np.diff((d * d).sum(axis=1)) >= 0).all()
        # nothing shorter was left out
        R = int(np.ceil(np.sqrt((d * d).sum(axis=1).max())))
        axes = np.meshgrid(*([np.arange(-R, R + 1)] * dim), indexing="ij")
        every = np.stack([a.reshape(-1) for a in axes], axis=1)
        shorter = ((every * every).sum(axis=1) < (d[-1] * d[-1]).sum()) & (every != 0).any(axis=1)
        assert shorter.sum() <= 2 * count and shorter.sum() == 2 * ((d * d).sum(axis=1) < (d[-1] * d[-1]).sum()).sum()


def test_the_lattice_of_the_wide_ragged_parity_test():
    """test_wide_ragged_stencil_generic_kernels (tests/test_gpu_parity.py): 7 x 7 stencils on a lattice open in both
    directions"""
    off = rw.lattice_offline((24, 24), 49, open_axes=(0, 1), norm="max")
    widths = rw.check_consistency(off, 49)
    assert widths.max() == 49 and widths.min() == 16


@pytest.mark.parametrize("name", sorted(cases.CASES) + ["aeos_refused", "aeos_refused_1d", "aeos_refused_3d"])
def test_layout_round_trip(name):
    """ryujin_hip_debug_layout (CSR -> SELL-64 -> logical view): the pattern and a three-component matrix come back
    entry by entry, and `transposed` is the involution (i, j) <-> (j, i)"""
    if name == "aeos_refused":
        off = cases._lattice(cases.AEOS_REFUSED["shape"], cases.AEOS_REFUSED["width"])()
    elif name.startswith("aeos_refused_"):
        off = cases.AEOS_REFUSED_DIMENSIONS[name[-2:]]["mesh"]()
        assert off.max_row_len == 33
    else:
        off = _mesh(name)
    n, nnz = off.n_owned, len(off.columns)
    matrix = np.random.default_rng(7).uniform(-1.0, 1.0, size=(nnz, 3))
    ptr, col = np.zeros(n + 1, dtype=np.uint64), np.zeros(nnz, dtype=np.uint32)
    tr, out = np.zeros(nnz, dtype=np.uint64), np.zeros((nnz, 3))
    rc = capi.load_hip().ryujin_hip_debug_layout(off.c, capi.as_ptr(ptr, capi.c_u64_p), capi.as_ptr(col, capi.c_u32_p),
                                                 capi.as_ptr(tr, capi.c_u64_p), capi.as_ptr(matrix, capi.c_double_p), 3,
                                                 capi.as_ptr(out, capi.c_double_p))
    assert rc == 0, capi.load_hip().ryujin_hip_last_error()
    assert np.array_equal(ptr, off.row_starts) and np.array_equal(col, off.columns)
    assert np.array_equal(out, matrix)
    tr = tr.astype(np.int64)
    assert np.array_equal(tr, rw.transposed_entries(off))
    assert np.array_equal(tr[tr], np.arange(nnz))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_the_oracle_alone_covers_the_columns(oracle, name):
    """the coverage condition of the case (helpers_row_width_cases.coverage) on the oracle's first-pass l_ij: a
    condition on the inputs, checked before any GPU run"""
    case = cases.CASES[name]
    off, dirichlet, states, weights, tau = cases.develop(case, oracle)
    first_pass = cases.oracle_first_pass(case, oracle, off, dirichlet, states, weights, tau)
    covered = cases.coverage(off, first_pass, case["width"])
    assert min(covered.values()) > 0, {k: v for k, v in covered.items() if v == 0}


@pytest.mark.parametrize("name", ["euler_1d_65", "euler_1d_128", "sw_1d_65"])
def test_rings_of_more_than_64_entries(name):
    """the rings with two partners per widened node, all indices modulo n (tests/helpers_row_width_cases.py: _ring): the
    widest row has exactly the requested width -- not 64 --, and EVERY slice of 64 rows holds rows of at least three
    widths, the widest among them"""
    case = cases.CASES[name]
    off = _mesh(name)
    widths = rw.check_consistency(off, case["width"])
    assert widths.max() == case["width"] and case["n_points"] % 64 == 0
    for s in range(case["n_points"] // 64):
        in_slice = widths[64 * s: 64 * s + 64]
        assert len(np.unique(in_slice)) >= 3 and in_slice.max() == case["width"], (s, np.unique(in_slice))
