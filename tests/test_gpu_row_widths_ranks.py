"""The kernel variants that the WIDEST STENCIL ROW selects, ON SEVERAL RANKS, against the partitioned oracle
(tests/helpers_row_width_ranks.py: the lattices cut into slabs, ragged uneven slabs and quadrants, the case table and the
coverage conditions; tests/test_row_width_ranks_cpu.py checks partition, literals, yardstick and coverage on the CPU,
tests/test_step_plan.py pins the plan and the launches of every rank against plan_step()).

What a rank adds to a wide row: its ghost columns fill the LAST blocks of 63 columns -- the blocks the wide kernels treat
specially --, l_ji of a ghost column is read through idx_t from a ghost row that the pack kernels and the transport
filled (up to 494 entries long here), and every sweep is an export launch of ceil(n_export / 64) slices and an interior
launch -- or one launch where every owned row is exported.

One process, the in-process transport, one thread per rank (at most four contexts). Per case: the flow is developed on the
SINGLE-RANK oracle, every rank gets its share, ONE update runs on both backends with every intermediate array fetched,
helpers_partitioned.compare_rank holds each rank to the contract of helpers_parity.py over its whole locally relevant
range, compare_ghost_rows holds the received ghost rows of l_ij bit for bit to what the neighbour holds, the coverage
conditions are asserted on the oracle ranks' arrays, and last_plan() of every rank must report the plan and both launches
of steps 5 and 6 of the table. No slack is claimed for any array: the tolerances are those of compare_rank. Each case
prints what it measured (profiles/row_width_ranks_pytest_gpu.txt).

Kernels of steps 2 / 3 / 5 / 6 per case (step 7 is k_high_order<E, true, false> throughout):
  euler_2d_10, 28, 33, 64             k_dij_alpha_records | k_dij_alpha (33, 64), k_dij_diag, k_pij_lij_recompute<2, 4>,
                                      at 64 once more <2, 1> (debug_no_small_mesh_split), k_high_order
  euler_2d_65 (quadrants), 127 (uneven), 128 (slabs; all rows exported), 1023, euler_1d_65
                                      k_dij_alpha, k_dij_diag, k_pij_lij<Euler<dim>, false, true>, k_high_order<.., true>
  euler_2d_checked_65                 the same with k_check_limiter / k_check_admissible behind them
  euler_3d_33, 128                    k_pij_lij<Euler<3>, false, false | true>
  sw_2d_10, 33 (friction), 65         the two walks of k_low_order_sw, k_pij_lij<ShallowWater<2>, false, W > 64>
  scalar_2d_65, aeos_2d_32            k_dij_alpha_sc / k_alpha_aeos + k_dij_aeos, k_pij_lij<.., false, W > 64>
  aeos_3d_28 (two slabs), aeos_1d_31 (two halves of the ring, cut through the widened run)
                                      k_ghost_records_aeos<3 | 1>, k_pij_lij<EulerAeos<3 | 1> >, four bounds in the ghost range"""
import numpy as np
import pytest

import helpers_row_width_ranks as ranks
from helpers_partitioned import compare_ghost_rows, compare_rank, global_scales, run_hip_ranks

pytestmark = pytest.mark.gpu


def _assert_plan(got, case, expected, label):
    for key, value in case["plan"].items():
        assert got[key] == value, (label, key, got[key], value)
    launches = expected["launches"]
    assert got["step5_launches"] == [dict(n_slices=s, grid_y=y) for s, y, _ in launches], (label, got["step5_launches"])
    assert got["step6_launches"] == [dict(n_slices=s, grid_y=1, shares_slices=b) for s, _, b in launches], \
        (label, got["step6_launches"])


@pytest.mark.parametrize("name", sorted(ranks.RANK_CASES))
def test_row_width_on_ranks_against_the_partitioned_oracle(oracle, name):
    b = ranks.built(name, oracle)
    case, views, ref, k = b["case"], b["views"], b["ref"], b["k"]
    assert len(views) <= 4
    hip = run_hip_ranks(views, ranks.make_params(name, oracle, b["off"].dim), ranks.hip_body(b["U_local"]))
    scales = global_scales(views, ref, k)
    for r, view in enumerate(views):   # the figures first, then the assertions
        figures = ranks.measured(view, hip[r], ref[r], k, scales)
        print(f"\nrow_width_ranks {name} rank {r}: n_owned={view.n_owned} n_export={view.n_export} "
              f"ghosts={view.n_relevant - view.n_owned} step5={hip[r]['plan']['step5']} wide={hip[r]['plan']['wide']} "
              f"step5_launches={hip[r]['plan']['step5_launches']} step6_launches={hip[r]['plan']['step6_launches']} | " +
              " ".join(f"{key}={value:.2e}" for key, value in figures.items()) + " slack_asked=False")
    accepted = []
    for r, view in enumerate(views):
        assert hip[r]["status"] == 0
        accepted.append(compare_rank(view, hip[r], ref[r], k, label=f"{name} rank {r}", scales=scales))
    n_ghost_row_entries = compare_ghost_rows(views, hip, ref, accepted)
    print(f"row_width_ranks {name}: ghost-row entries compared bit for bit: {n_ghost_row_entries}, "
          f"l_ij entries accepted by their effect: {sum(len(a[q]) for a in accepted for q in a)}")
    assert n_ghost_row_entries > 0
    ranks.assert_coverage(name, b, ref)
    for r, expected in enumerate(case["ranks"]):
        assert (views[r].n_owned, views[r].n_export) == (expected["n_owned"], expected["n_export"])
        _assert_plan(hip[r]["plan"], case, expected, f"{name} rank {r}")


def test_single_rank_reference_of_the_rank_cases_is_the_partitioned_one(oracle):
    """the GPU ranks are compared with the partitioned oracle; that run itself agrees with the single-rank oracle on the
    owned rows (asserted per case in tests/test_row_width_ranks_cpu.py) -- here once more for the widest case, next to
    the GPU result: U_new of the GPU ranks against the SINGLE-RANK oracle to the 1e-11 of compare_rank"""
    name = "euler_2d_1023"
    b = ranks.built(name, oracle)
    hip = run_hip_ranks(b["views"], ranks.make_params(name, oracle, 2), ranks.hip_body(b["U_local"]))
    scale = np.maximum(np.abs(b["U_single"]).max(axis=0), 1e-3 * np.abs(b["U_single"]).max())
    for view, g in zip(b["views"], hip):
        assert abs(g["tau"] - b["tau_single"]) <= 1e-12 * b["tau_single"]
        assert (np.abs(g["U"] - b["U_single"][view.global_ids[: view.n_owned]]) / scale).max() <= 1e-11
