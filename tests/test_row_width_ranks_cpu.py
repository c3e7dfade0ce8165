"""The multi-rank row-width cases (tests/helpers_row_width_ranks.py: RANK_CASES) on the CPU, before any GPU run: the
per-rank views satisfy the exchange contract, the literals of the table are those of the partition (tests/test_step_plan.py
holds the plan and the launches against plan_step()), the partitioned oracle -- the yardstick of
tests/test_gpu_row_widths_ranks.py -- reproduces the single-rank oracle on these lattices, and the data covers what a
rank adds to a wide row: ghost columns in the last blocks of 63, l_ji read from long ghost rows."""
import numpy as np
import pytest

import helpers_row_width_ranks as ranks
from helpers_partitioned import exchange_lists

NAMES = sorted(ranks.RANK_CASES)


@pytest.mark.parametrize("name", NAMES)
def test_rank_views_satisfy_the_exchange_contract(oracle, name):
    """send and receive counts match pairwise, for the vectors and for the matrix ghost rows; a ghost row holds its
    diagonal and columns owned by this rank, nothing else; every rank's widest owned row is the case's width (and the
    lattice has no wider one); rows behind the export range have no ghost column"""
    b = ranks.built(name, oracle)
    views, width = b["views"], b["case"]["width"]
    lists = [exchange_lists(v) for v in views]
    assert sum(v.n_owned for v in views) == b["off"].n_owned
    for r, (v, x) in enumerate(zip(views, lists)):
        n, ptr = v.n_owned, x["ptr"]
        cols = np.asarray(v._keep["columns"]).astype(np.int64)
        lengths = np.diff(ptr)
        assert lengths[:n].max() == width and v.n_relevant > n, (r, lengths[:n].max())
        rows = np.repeat(np.arange(v.n_relevant), lengths)
        assert (cols[ptr[:-1]] == np.arange(v.n_relevant)).all(), "diagonal first"
        ghost_entries = rows >= n
        assert (cols[ghost_entries & (cols != rows)] < n).all(), "a ghost row holds the diagonal and owned columns only"
        assert (cols[(rows >= v.n_export) & ~ghost_entries] < n).all(), "only export rows couple to ghost columns"
        assert x["recv_off"][0] == n and x["recv_off"][-1] == v.n_relevant
        for q, p in enumerate(x["nbr"]):
            y = lists[p]
            qq = y["nbr"].index(r)
            assert x["send_off"][q + 1] - x["send_off"][q] == y["recv_off"][qq + 1] - y["recv_off"][qq], (r, p)
            sent = x["row_send_off"][q + 1] - x["row_send_off"][q]
            assert sent == y["ptr"][y["recv_off"][qq + 1]] - y["ptr"][y["recv_off"][qq]], (r, p, "ghost rows")
            # the global nodes sent are the ones the neighbour numbers as its ghosts, in that order
            mine = views[r].global_ids[x["send_idx"][x["send_off"][q]:x["send_off"][q + 1]]]
            assert np.array_equal(mine, views[p].global_ids[y["recv_off"][qq]:y["recv_off"][qq + 1]]), (r, p)


@pytest.mark.parametrize("name", NAMES)
def test_literals_of_the_table_are_those_of_the_partition(oracle, name):
    """n_owned, n_export and the slices of the two launches: ceil(n_export / 64) of ceil(n_owned / 64) slices, a rank
    whose owned rows are all exported has one launch"""
    b = ranks.built(name, oracle)
    assert len(b["views"]) == len(b["case"]["ranks"])
    for v, literal in zip(b["views"], b["case"]["ranks"]):
        assert (v.n_owned, v.n_export) == (literal["n_owned"], literal["n_export"])
        n_slices, n_export_slices = (v.n_owned + 63) // 64, (v.n_export + 63) // 64
        sizes = [s for s, _, _ in literal["launches"]]
        assert sizes == ([n_export_slices, n_slices - n_export_slices] if n_slices > n_export_slices else [n_slices])
    # the table holds what it was built for: a rank of nothing but export rows, their number no multiple of 64 ...
    if b["case"]["owner"] is ranks.uneven:
        first = b["case"]["ranks"][0]
        assert first["n_owned"] == first["n_export"] and first["n_export"] % 64 != 0 and len(first["launches"]) == 1
    # ... and three neighbours per rank
    if b["case"]["owner"] is ranks.quadrants:
        assert all(v.c.contents.n_nbr == 3 for v in b["views"])


def test_the_table_has_every_kind_of_launch():
    """one launch (every row exported), two launches, a last export slice that mixes exported and interior rows, an
    export range of exactly one slice; wide cases with one, two and three neighbours"""
    every = [r for case in ranks.RANK_CASES.values() for r in case["ranks"]]
    assert any(len(r["launches"]) == 1 for r in every) and any(len(r["launches"]) == 2 for r in every)
    assert any(r["n_export"] % 64 and r["n_export"] < r["n_owned"] for r in every)
    assert any(r["n_export"] == 64 for r in every)
    wide = {len(c["ranks"]) for c in ranks.RANK_CASES.values() if c["width"] > 64}
    assert wide == {2, 3, 4}


@pytest.mark.parametrize("name", NAMES)
def test_partitioned_oracle_reproduces_the_single_rank_oracle(oracle, name):
    """the update of the owned rows to 1e-12 of the component's scale (the bound of
    test_partitioned_oracle_helper_reproduces_the_single_rank_oracle; measured: 5e-15 at the most), tau to 1e-13"""
    b = ranks.built(name, oracle)
    scale = np.abs(b["U_single"]).max(axis=0)
    for r, (v, x) in enumerate(zip(b["views"], b["ref"])):
        assert x["status"] == 0
        assert abs(x["tau"] - b["tau_single"]) <= 1e-13 * b["tau_single"]
        assert (np.abs(x["U"] - b["U_single"][v.global_ids[: v.n_owned]]) / scale).max() < 1e-12, r


@pytest.mark.parametrize("name", NAMES)
def test_the_partitioned_oracle_alone_covers_the_ghost_columns_and_rows(oracle, name):
    """helpers_row_width_ranks.ghost_coverage on every rank, and the single-rank condition of the case
    (helpers_row_width_cases.coverage) on the union of the owned rows: conditions on the inputs"""
    b = ranks.built(name, oracle)
    counts = ranks.assert_coverage(name, b, b["ref"])
    if b["case"]["width"] == 1023:
        # the leading blocks of a very wide row hold owned columns only: the condition is stated for the blocks that
        # have a ghost column, and the last block is among them
        for c in counts:
            assert not any(k.startswith("ghost columns in block 1..") for k in c)
            assert any(k.startswith("ghost columns in block 1009..1022") for k in c)
