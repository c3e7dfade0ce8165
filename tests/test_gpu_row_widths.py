"""Every kernel variant that the WIDEST STENCIL ROW selects, against the oracle, next to each threshold of
ryujin_amd/csrc/step_plan.hpp and of the kernels (tests/helpers_row_width_cases.py: the case table and what each width
changes; tests/helpers_row_width.py: the lattices with a prescribed widest row; tests/test_step_plan.py pins the table's
literals against plan_step() on the CPU, tests/test_row_width_generator.py checks the meshes and the coverage there).

Per case, as tests/test_gpu_plan_variants.py: the flow is developed ON THE ORACLE, both backends get that state, ONE
update goes through helpers_parity.compare_step -- every intermediate array to the stated contract, l_ij and l'_ij of
both passes included -- and HyperbolicModule.last_plan() must report the plan and the launches of the table, field by
field. A case counts only if the oracle's first-pass l_ij covers the columns (helpers_row_width_cases.coverage). The
tolerances are those of helpers_parity.py; U_new may exceed its bound by the summation-order slack of the row's limited
update (helpers_row_width_cases.summation_slack) and by nothing else -- each case prints what it measured and whether
the slack was asked for (profiles/row_width_pytest_gpu.txt).

Kernels of steps 2 / 3 / 5 / 6 per case (W the widest row; step 7 is k_high_order<E, true, false> throughout):
  euler_1d_4, 9 | 10                 k_dij_alpha_records, k_dij_diag_unrolled<9 | 27>, k_pij_lij_recompute<1, 4>, k_high_order
  euler_2d_10, 27 | 28, 32 | 33, 64  k_dij_alpha_records (W <= 32) | k_dij_alpha, k_dij_diag_unrolled<27> (W <= 27) |
                                     k_dij_diag, k_pij_lij_recompute<2, 4> and, second run, <2, 1>
  euler_2d_65, 127 | 128, 1023       k_dij_alpha, k_dij_diag, k_low_order storing P_ij, k_pij_lij<Euler<2>, false, true>,
                                     k_high_order<.., false, true>: two, two, three and seventeen blocks of 63 columns
  euler_3d_28, 33, 65, 128           k_pij_lij<Euler<3>, false, W > 64>
  euler_2d_newton_32 | 33            k_alpha + k_dij_records<.., true> | k_dij_alpha (Newton iterations in the Riemann solver)
  euler_2d_checked_65                the wide kernels with k_check_limiter / k_check_admissible behind them
  euler_2d_erk33_10, 128             step<2> of ERK33: k_low_order<2, true, true, false>, k_pij_lij<.., W > 64>
  sw_1d_4, sw_2d_10 ... 128          k_low_order_sw (two walks; friction at 33), k_pij_lij<ShallowWater<dim>, false, W > 64>
  scalar_2d_10, 28, 65, 128          k_dij_alpha_sc, k_low_order_sc, k_pij_lij<ScalarConservation<2>, false, W > 64>
  aeos_2d_10, 32                     k_alpha_aeos + k_dij_aeos, k_low_order_aeos storing P_ij, k_pij_lij<EulerAeos<2> >
  aeos_1d_4, 9 | 10, 31              k_dij_diag_unrolled<9 | 27> | k_dij_diag, k_low_order_aeos<1, false, true, false>,
                                     k_pij_lij<EulerAeos<1> >, k_high_order
  aeos_3d_28, 32                     k_low_order_aeos<3, false, true, false>, k_pij_lij<EulerAeos<3> >
  aeos_3d_erk33_28, aeos_2d_erk33_32 step<2> of ERK33: k_low_order_aeos<3 | 2, true, true, false>
  aeos_3d_checked_28                 k_check_limiter / k_check_admissible on four bounds
  EulerAEOS with 33 entries          refused by step() on the host, in one, two and three dimensions"""
import numpy as np
import pytest

import helpers_row_width_cases as cases
from helpers_parity import compare_step
from ryujin_amd import HyperbolicModule, capi

pytestmark = pytest.mark.gpu


def _assert_plan(m, expected_plan, launches, label):
    got = m.last_plan()
    for key, value in expected_plan.items():
        assert got[key] == value, (label, key, got[key], value)
    assert got["step5_launches"] == launches["step5_launches"], (label, got["step5_launches"])
    assert got["step6_launches"] == launches["step6_launches"], (label, got["step6_launches"])


def _run_case(oracle, name):
    case = cases.CASES[name]
    off, dirichlet, states, weights, tau = cases.develop(case, oracle)
    assert off.n_owned == case["n_points"] and off.max_row_len == case["width"]
    for run, launches in enumerate(case["runs"]):
        label = name + (" (debug_no_small_mesh_split)" if run == 1 else "")
        mods, stage_vectors, params = cases.modules(case, oracle, off, states, run)
        for m, vectors in zip((mods[0][0], mods[1][0]), stage_vectors):
            for v in vectors:   # stage vectors are prepared state vectors (hyperbolic_module.h:207-213)
                m.prepare_state_vector(v, 0.0, dirichlet)
        g, c = compare_step(off, mods, dirichlet, tau, oracle=oracle, params=params, label=label,
                            stage_vectors=stage_vectors if case["stages"] else None, stage_weights=weights,
                            row_slack=cases.summation_slack(off, case["equation"]))
        print(f"\nrow_width {label}: " + " ".join(f"{k}={v:.2e}" for k, v in g["measured"].items()) +
              f" slack_used={g['slack_used']} flips={g['n_flips']}")
        assert g["status"] == 0
        covered = cases.coverage(off, c["lij_next"], case["width"])
        assert min(covered.values()) > 0, (label, {k: v for k, v in covered.items() if v == 0})
        _assert_plan(mods[0][0], case["plan"], launches, label)
        for m, _, _ in mods:
            m.close()


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_row_width_against_the_oracle(oracle, name):
    _run_case(oracle, name)


def test_euler_aeos_refuses_33_entries_and_runs_on(oracle):
    """EulerAEOS with a row of 33 entries: step() returns RYUJIN_ERR_UNSUPPORTED with the message of plan_step() -- a
    refusal on the host before any launch, again on the next call --, the state vectors are untouched, and the library
    runs the 32-wide case afterwards as ever."""
    refused = cases.AEOS_REFUSED
    _refused_then_accepted(oracle, dict(refused["accepted"], mesh=cases._lattice(refused["shape"], refused["width"])),
                           refused["message"], "aeos_2d_32")


@pytest.mark.parametrize("key", sorted(cases.AEOS_REFUSED_DIMENSIONS))
def test_euler_aeos_refuses_33_entries_in_one_and_three_dimensions(oracle, key):
    """the same on a ring and on a 3-D lattice with a row of 33 entries; afterwards the widest accepted case of that
    dimension runs"""
    refused = cases.AEOS_REFUSED_DIMENSIONS[key]
    _refused_then_accepted(oracle, dict(cases.CASES[refused["accepted"]], mesh=refused["mesh"]), refused["message"],
                           refused["accepted"])


def _refused_then_accepted(oracle, case, message, accepted):
    import helpers_plan_cases as plan_cases
    off, U0, dirichlet, _ = plan_cases.build(case)
    assert off.max_row_len == 33
    m = HyperbolicModule(off, plan_cases.params_of(case, oracle, off.dim), backend="hip")
    old, new = m.new_state_vector(U0), m.new_state_vector(np.zeros_like(U0))
    m.prepare_state_vector(old, 0.0, dirichlet)
    for _ in range(2):
        with pytest.raises(RuntimeError, match=f"status {capi.RYUJIN_ERR_UNSUPPORTED}: {message}"):
            m.step(old, [], [], new)
    assert np.array_equal(old.download(), U0) and not new.download().any()
    m.close()
    _run_case(oracle, accepted)
