"""The discontinuous-ansatz kernels against the oracle: three dimensions, rows of more than 64 entries, stage vectors, the
checked build, slip and Dirichlet boundaries, fractional incidence values, several ranks (tests/helpers_dg_cases.py: the
case table, the data and what a case must show on the oracle before it counts; tests/test_dg_cases_cpu.py checks the
meshes, the coverage and the partitioned yardstick on the CPU, tests/test_step_plan.py pins the plans).

Per single-rank case: the flow is developed ON THE ORACLE, both backends get that state, ONE update goes through
helpers_parity.compare_step -- every intermediate array to the stated contract -- TWICE: as the first update of a fresh
HIP context and as its second, after one update of that context from the same state (step() swaps the bounds buffer with
the combined one once per update: both parities are compared, behind k_check_limiter / k_check_admissible too).
HyperbolicModule.last_plan() must report the plan and the launches of the table, field by field. U_new of rows wider
than 64 entries may exceed its bound by the summation-order slack of the row's limited update
(helpers_row_width_cases.summation_slack) and by nothing else; each case prints what it measured and whether the slack
was asked for (profiles/dg_variants_pytest_gpu.txt).

Kernels per case (step 6 is k_high_order<E, false, W > 64>, step 7 k_high_order<E, true, false> throughout):
  euler_q1_3d                        k_dij_alpha, k_low_order<3, false, true, true>, k_pij_lij<Euler<3>, true, false>
  euler_q1_3d_erk33_step1 | 2        k_low_order<3, true, true, true>
  euler | sw | aeos_q1_2d_erk33_step2  k_low_order<2, true, true, true>, k_low_order_sw<2, true, true>,
                                     k_low_order_aeos<2, true, true, true>
  euler | sw | aeos_q1_2d_checked    k_check_limiter / k_check_admissible on the combined bounds
  euler_q1_2d_slip | dirichlet       boundary rows of a dG stencil
  euler_q2_1d, euler | sw_q2_2d      rows of 9 / 45 entries, graded meshes: fractional incidence, (M^-1)_ij per cell
  aeos_q1_1d, aeos_q2_1d, aeos_q1_1d_erk33_step2
                                     k_low_order_aeos<1, false | true, true, true>, k_pij_lij<EulerAeos<1>, true, false>
  euler_q2_3d                        rows of 189 entries: k_pij_lij<Euler<3>, true, true>, k_high_order<.., false, true>
  synthetic_*                        k_pij_lij<E, true, W > 64> on lattices with the widest row at 64 | 65, 127 | 128
  EulerAEOS dG-Q1 3-D, dG-Q2 2-D     refused by step() on the host
  ranks                              euler_q2_3d on two, aeos_q1_2d on three, synthetic_euler_2d_128 on two"""
import numpy as np
import pytest

import helpers_dg_cases as cases
import helpers_row_width_cases as width_cases
from helpers_parity import compare_step
from ryujin_amd import HyperbolicModule, capi

pytestmark = pytest.mark.gpu


def _assert_plan(got, expected_plan, launches, label):
    for key, value in expected_plan.items():
        assert got[key] == value, (label, key, got[key], value)
    assert got["step5_launches"] == launches["step5_launches"], (label, got["step5_launches"])
    assert got["step6_launches"] == launches["step6_launches"], (label, got["step6_launches"])


def _assert_inputs(name, case, off, first_pass_lij, alpha):
    covered = cases.coverage(off, first_pass_lij, case["width"])
    assert min(covered.values()) > 0, (name, {k: v for k, v in covered.items() if v == 0})
    if case["incidence"]:
        assert min(cases.incidence_arms(off, alpha)) > 0, (name, cases.incidence_arms(off, alpha))


def _run_case(oracle, name):
    case = cases.CASES[name]
    (off, dirichlet, states, weights, tau), alone = cases.developed(name, oracle)
    assert off.n_owned == case["n_points"] and off.max_row_len == case["width"]
    assert alone["status"] == 0 and alone["warnings"] == 0
    _assert_inputs(name, case, off, alone["lij_next"], alone["alpha"])
    slack = cases.summation_slack(off, case["equation"]) if case["width"] > 64 else None
    for update in ("first", "second"):
        label = f"{name} ({update} update of the context)"
        mods, stage_vectors, params = width_cases.modules(case, oracle, off, states)
        for (m, old, new), vectors in zip(mods, stage_vectors):
            for v in vectors:   # stage vectors are prepared state vectors (hyperbolic_module.h:207-213)
                m.prepare_state_vector(v, 0.0, dirichlet)
            if update == "second":   # one update from the same state first: the bounds buffers have been swapped once
                m.prepare_state_vector(old, 0.0, dirichlet)
                m.step(old, list(vectors), list(weights), new, tau)
        g, c = compare_step(off, mods, dirichlet, tau, oracle=oracle, params=params, label=label,
                            stage_vectors=stage_vectors if case["stages"] else None, stage_weights=weights,
                            row_slack=slack)
        print(f"\ndg_variants {label}: " + " ".join(f"{k}={v:.2e}" for k, v in g["measured"].items()) +
              f" slack_used={g['slack_used']} flips={g['n_flips']}")
        assert g["status"] == 0 and mods[0][0].n_warnings() == 0 and mods[1][0].n_warnings() == 0
        _assert_inputs(label, case, off, c["lij_next"], c["alpha"])
        if name in ("euler_q1_2d_slip", "euler_q1_2d_dirichlet"):   # the update has moved the boundary rows
            moved = np.abs(c["U"] - c["U_old"])[off.dg_info["is_bdry"]].max(axis=0)
            assert (moved > 1e-3 * np.abs(c["U"]).max(axis=0))[[0, -1]].all(), (label, moved)
        _assert_plan(mods[0][0].last_plan(), case["plan"], case, label)
        for m, _, _ in mods:
            m.close()


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_dg_variant_against_the_oracle(oracle, name):
    _run_case(oracle, name)


def test_euler_aeos_refuses_wide_dg_stencils_and_runs_on(oracle):
    """EulerAEOS on dG-Q1 in 3-D (56 entries) and dG-Q2 in 2-D (45): step() returns RYUJIN_ERR_UNSUPPORTED with the
    message of plan_step() -- on the host, before any launch, again on the next call --, the state vectors are
    untouched, and the library then runs the EulerAEOS dG-Q1 2-D case as ever."""
    refused = cases.AEOS_REFUSED
    for key, (mesh, width) in sorted(refused["meshes"].items()):
        off = mesh()
        assert off.max_row_len == width > 32
        p = oracle.default_params(capi.EQ_EULER_AEOS, off.dim)
        refused["edit"](p)
        m = HyperbolicModule(off, p, backend="hip")
        U0 = cases._aeos_blast()(off)["U0"]
        old, new = m.new_state_vector(U0), m.new_state_vector(np.zeros_like(U0))
        m.prepare_state_vector(old, 0.0, None)
        for _ in range(2):
            with pytest.raises(RuntimeError, match=f"status {capi.RYUJIN_ERR_UNSUPPORTED}: {refused['message']}"):
                m.step(old, [], [], new)
        assert np.array_equal(old.download(), U0) and not new.download().any(), key
        m.close()
    _run_case(oracle, refused["accepted"])


# ------------------------------------------------------------------ several ranks

@pytest.mark.parametrize("name", sorted(cases.RANK_CASES))
def test_dg_variant_on_ranks_against_the_partitioned_oracle(oracle, name):
    """one process, the in-process transport, one thread per rank: compare_rank holds every rank to the contract over
    its whole locally relevant range, compare_ghost_rows the received ghost rows of l_ij bit for bit to what the neighbour
    holds; no slack is claimed"""
    import helpers_row_width_ranks as ranks
    from helpers_partitioned import compare_ghost_rows, compare_rank, global_scales, run_hip_ranks
    b = cases.built_ranks(name, oracle)
    case, views, ref, k = b["case"], b["views"], b["ref"], b["k"]
    assert len(views) <= 4
    hip = run_hip_ranks(views, b["make_params"], ranks.hip_body(b["U_local"]))
    scales = global_scales(views, ref, k)
    for r, view in enumerate(views):   # the figures first, then the assertions
        figures = ranks.measured(view, hip[r], ref[r], k, scales)
        print(f"\ndg_variants ranks {name} rank {r}: n_owned={view.n_owned} n_export={view.n_export} "
              f"ghosts={view.n_relevant - view.n_owned} | " +
              " ".join(f"{key}={value:.2e}" for key, value in figures.items()) + " slack_asked=False")
    accepted = []
    for r, view in enumerate(views):
        assert hip[r]["status"] == 0 and ref[r]["status"] == 0
        accepted.append(compare_rank(view, hip[r], ref[r], k, label=f"{name} rank {r}", scales=scales))
    assert compare_ghost_rows(views, hip, ref, accepted) > 0
    cases.assert_rank_coverage(name, b, ref)
    for r, (n_owned, n_export, launches) in enumerate(b["entry"]["ranks"]):
        assert (views[r].n_owned, views[r].n_export) == (n_owned, n_export)
        _assert_plan(hip[r]["plan"], case["plan"],
                     dict(step5_launches=[dict(n_slices=s, grid_y=y) for s, y, _ in launches],
                          step6_launches=[dict(n_slices=s, grid_y=1, shares_slices=x) for s, _, x in launches]),
                     f"{name} rank {r}")
