"""Every kernel variant that the launch-size splits of steps 5 and 6 select, against the oracle, at the slice counts where
the selection changes (tests/helpers_plan_cases.py: the case table; tests/test_step_plan.py pins its literals against
plan_step() on the CPU).

Per case: the flow is developed ON THE ORACLE, both backends get that state, ONE update goes through
helpers_parity.compare_step -- every intermediate array to the stated contract, every l_ij outlier classified -- and
then HyperbolicModule.last_plan() must report the plan and the launches of the table: which kernel was compared is
asserted, not assumed. A case counts only if the oracle's first-pass l_ij has entries below 1 in every off-diagonal
column position and in rows of every width (limiter_coverage): the waves of a split variant take different columns, and
narrow rows leave waves without one.

Kernels of step 5 / step 6 per case, as the fetch reports them (NY = gridDim.y of step 5, `shared`: the four waves of a
block share a slice in step 6):
  euler_1d_512 / 513 / 680 / 681 / 1024    k_lij_stage0<Euler<1>, 4 / 3 / 3 / 2 / 2>, shared
  euler_1d_1025                            k_lij_stage0<Euler<1>, 1, false, true> (P_ij per tile), not shared
  euler_2d_step_896                        k_lij_stage0<Euler<2>, 2>, shared
  euler_2d_step_1588, box_4096, box_4097   k_lij_stage0<Euler<2>, 1, false, true>, not shared; boundary conditions
                                           folded into the pre-pass up to 4096 slices, a launch of their own above
  aeos_2d_step_674 / 896                   k_lij_stage0<EulerAeos<2>, 3 / 2>, shared
  aeos_1d_512 / 513 / 680 / 681 / 1024     k_lij_stage0<EulerAeos<1>, 4 / 3 / 3 / 2 / 2>, shared
  aeos_1d_1025, aeos_2d_step_1588          k_lij_stage0<EulerAeos<1 | 2>, 1, false, true> (P_ij per tile), not shared
  aeos_3d_box_562 / 1000 / 1424            k_lij_stage0<EulerAeos<3>, 3 / 2 / 1>, 1000 with the Noble-Abel stiffened gas;
                                           1424, second update: <EulerAeos<3>, 1, true, false> and step 6 as light,
                                           repair, heavy
  euler_3d_box_562 / 1000 / 1424           k_lij_stage0<Euler<3>, 3 / 2 / 1>; 1424, second update: <Euler<3>, 1, true, false>
                                           (P_ij per slice) and step 6 as light, repair, heavy
  sw_2d_1001 / 1148, scalar_2d_1001 / 1148 k_pij_lij, P_ij everywhere; step 6 shared / not shared
  euler_q2_625 / 900 / 1225                k_pij_lij_recompute<2, 3 / 2 / 1>, k_high_order
  erk33 (896 slices)                       step<1>, step<2>: k_pij_lij, step 6 shared
  erk33_aeos_1d_681, erk33_aeos_3d_box_562 step<1>, step<2>: k_low_order_aeos<1 | 3, true, ...>, k_pij_lij<EulerAeos<1 | 3> >,
                                           step 6 shared in 1-D, not shared in 3-D
  erk33_sw_friction_1d_100 / 2d_13x7       stage 0: k_low_order_sw_single_walk<1 | 2, false, 3 | 9, true>; step<1>, step<2>:
                                           <1 | 2, true, 3 | 9, true> (Manning friction, uneven and partly dry bed)
  two ranks, shallow water                 step 6 shared in the export part, not shared in the interior part"""
import numpy as np
import pytest

import helpers_plan_cases as cases
from helpers_parity import compare_step
from ryujin_amd import HyperbolicModule, offline

pytestmark = pytest.mark.gpu


def _assert_coverage(off, first_pass_lij, label):
    per_position, per_width = cases.limiter_coverage(off, first_pass_lij)
    assert min(per_position.values()) > 0, (label, "column positions the limiter never acts in", per_position)
    assert min(per_width.values()) > 0, (label, "row widths the limiter never acts in", per_width)


def _assert_plan(m, expected_plan, step5_launches, step6_launches, label):
    got = m.last_plan()
    for key, value in expected_plan.items():
        assert got[key] == value, (label, key, got[key], value)
    assert got["step5_launches"] == step5_launches, (label, got["step5_launches"])
    assert got["step6_launches"] == step6_launches, (label, got["step6_launches"])


def _print_measured(label, g):
    """the largest difference of every compared array, in its bound's units (profiles/aeos_dimensions_pytest_gpu.txt)"""
    print(f"\nplan_variants {label}: " + " ".join(f"{k}={v:.2e}" for k, v in g["measured"].items()) +
          f" slack_used={g['slack_used']} flips={g['n_flips']}")


def _compare(off, mods, oracle, params, dirichlet, label, **kw):
    g, c = compare_step(off, mods, dirichlet, oracle=oracle, params=params, label=label, **kw)
    _print_measured(label, g)
    assert g["status"] == 0
    return g, c


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_variant_against_the_oracle(oracle, name):
    case = cases.CASES[name]
    off, U0, dirichlet, after_warm = cases.build(case)
    assert off.n_owned == case["n_points"]
    U_start = cases.warm_up(case, oracle, off, U0, dirichlet, after_warm)
    mods = cases.both_backends(case, oracle, off, U_start)
    params = cases.params_of(case, oracle, off.dim)
    g, c = _compare(off, mods, oracle, params, dirichlet, name)
    _assert_coverage(off, c["lij_next"], name)
    (mg, og, ng), (mc, oc, nc) = mods
    _assert_plan(mg, case["plan"], case["step5_launches"], case["step6_launches"], name)
    second = case["second_update"]
    if second:
        # the next update of the same context, from the ORACLE's result on both backends: the limited fraction of the
        # first one now decides how P_ij is stored
        ng.upload(nc.download())
        g, c = _compare(off, [(mg, ng, og), (mc, nc, oc)], oracle, params, dirichlet, name + " second update")
        _assert_coverage(off, c["lij_next"], name + " second update")
        _assert_plan(mg, second["plan"], second["step5_launches"], second["step6_launches"], name + " second update")
    for m, _, _ in mods:
        m.close()


def test_erk33_stages_with_stage_vectors_share_slices_in_step_6(oracle):
    """step<1> and step<2> of ERK33 (time_integrator.template.h:373-403) on the Mach-3 step at 896 slices: with stage
    vectors step 4 stores P_ij, step 5 is k_pij_lij and step 6 shares slices. Every stage on identical inputs (the
    oracle's stage result goes to both backends), as test_erk43_erk54_parity_with_the_oracle."""
    _erk33_stages(oracle, cases.ERK33_CASE, "erk33")


@pytest.mark.parametrize("name", sorted(set(cases.ERK33_CASES) - {"erk33"} - set(cases.ERK33_SW_FRICTION_CASES)))
def test_erk33_stages_with_stage_vectors_on_euler_aeos(oracle, name):
    """the same on EulerAEOS in 1-D (681 slices: step 6 shares slices) and 3-D (562 slices): k_low_order_aeos with stage
    vectors -- the stage vectors' precomputed pressures enter the fluxes --, step 5 is k_pij_lij"""
    _erk33_stages(oracle, cases.ERK33_CASES[name], name)


@pytest.mark.parametrize("name", sorted(cases.ERK33_SW_FRICTION_CASES))
def test_erk33_stages_on_shallow_water_with_friction(oracle, name):
    """the same on shallow water with a Manning coefficient over an uneven, partly dry bed, in 1-D and 2-D: the plain
    update of stage 0 is k_low_order_sw_single_walk<dim, false, 3 | 9, true>, step<1> and step<2> are
    <dim, true, 3 | 9, true> -- the row's and the neighbours' friction sources of the stage vectors enter F_iH and P_ij"""
    case = cases.ERK33_SW_FRICTION_CASES[name]
    _erk33_stages(oracle, case, name, stage0_plan=dict(case["plan"], step4_has_stages=False))


def _erk33_stages(oracle, case, name, stage0_plan=None):
    off, U0, dirichlet, after_warm = cases.build(case)
    assert off.n_owned == case["n_points"]
    U_start = cases.warm_up(case, oracle, off, U0, dirichlet, after_warm)
    mods = cases.both_backends(case, oracle, off, U_start)
    params = cases.params_of(case, oracle, off.dim)
    (mg, og, _), (mc, oc, _) = mods
    vec = {id(mg): [og], id(mc): [oc]}
    table = [((), ()), ((0,), (-1.0,)), ((0, 1), (0.75, -2.0))]
    tau = 0.0
    for stage, (idx, weights) in enumerate(table):
        for m in (mg, mc):
            vec[id(m)].append(m.new_state_vector())
            for q in idx:   # stage vectors are prepared state vectors (hyperbolic_module.h:207-213)
                m.prepare_state_vector(vec[id(m)][q], 0.0, dirichlet)
        step_mods = [(mg, vec[id(mg)][stage], vec[id(mg)][stage + 1]), (mc, vec[id(mc)][stage], vec[id(mc)][stage + 1])]
        g, c = compare_step(off, step_mods, dirichlet, tau, oracle=oracle, params=params, label=f"{name} stage {stage}",
                            stage_vectors=([vec[id(mg)][q] for q in idx], [vec[id(mc)][q] for q in idx]),
                            stage_weights=weights)
        _print_measured(f"{name} stage {stage}", g)
        assert g["status"] == 0
        tau = c["tau"]
        if stage == 0 and stage0_plan:
            _assert_plan(mg, stage0_plan, case["step5_launches"], case["step6_launches"], f"{name} stage 0")
        if stage > 0:
            _assert_coverage(off, c["lij_next"], f"{name} stage {stage}")
            _assert_plan(mg, case["plan"], case["step5_launches"], case["step6_launches"], f"{name} stage {stage}")
        vec[id(mg)][stage + 1].upload(vec[id(mc)][stage + 1].download())
    for m, _, _ in mods:
        m.close()


def test_two_ranks_take_different_step_6_kernels_in_export_and_interior(oracle):
    """Shallow water on two ranks of one GPU (in-process transport): the export part of a rank has a few slices, the
    interior part more than 1024 -- the two launches of step 6 decide differently, and the fetch says so. One update from
    a state developed on the single-rank oracle; the owned rows against the single-rank oracle's update to the contract
    of the partitioned tests (tau to 1e-13, U to 1e-11 per component)."""
    from helpers_partitioned import run_hip_ranks
    case = cases.TWO_RANK_CASE
    n, lower, upper = case["n"], case["lower"], case["upper"]
    single = dict(cases.CASES["sw_2d_1148"], mesh=lambda: offline.SyntheticOffline(offline.rectangle_2d(n, lower, upper)),
                  warm=case["warm"])
    off, U0, dirichlet, after_warm = cases.build(single)
    assert off.n_owned == case["n_points"]
    U_start = cases.warm_up(single, oracle, off, U0, dirichlet, after_warm)
    mc = HyperbolicModule(off, cases.params_of(single, oracle, 2), backend=oracle.backend())
    oc, nc = mc.new_state_vector(U_start), mc.new_state_vector()
    mc.prepare_state_vector(oc, 0.0, None)
    tau_ref = mc.step(oc, [], [], nc)
    assert mc.last_status == 0
    U_ref = nc.download()[: off.n_owned]
    first_pass = mc.debug_fetch("lij_next")
    _assert_coverage(off, first_pass, "two ranks")
    gid_ref = off.global_ids[: off.n_owned].astype(np.int64)
    by_gid = np.empty(int(gid_ref.max()) + 1, dtype=np.int64)
    by_gid[gid_ref] = np.arange(off.n_owned)

    parts = [offline.SyntheticOffline(offline.rectangle_2d(n, lower, upper, n_ranks=2, rank=r)) for r in range(2)]

    def body(m, part, r):
        local = by_gid[part.global_ids.astype(np.int64)]
        old, new = m.new_state_vector(U_start[local]), m.new_state_vector()
        m.prepare_state_vector(old, 0.0, None)
        tau = m.step(old, [], [], new)
        return dict(tau=tau, status=m.last_status, plan=m.last_plan(), U=new.download()[: part.n_owned],
                    rows=local[: part.n_owned])

    out = run_hip_ranks(parts, lambda: cases.params_of(single, oracle, 2), body)
    scale = np.maximum(np.abs(U_ref).max(axis=0), 1e-3 * np.abs(U_ref).max())
    for r, (part, res) in enumerate(zip(parts, out)):
        assert res["status"] == 0
        assert abs(res["tau"] - tau_ref) <= 1e-13 * tau_ref
        assert (np.abs(res["U"] - U_ref[res["rows"]]) / scale).max() <= 1e-11, r
        for key, value in case["plan"].items():
            assert res["plan"][key] == value, (r, key, res["plan"][key], value)
        assert part.n_owned == case["ranks"][r]["n_owned"]
        launches = case["ranks"][r]["launches"]
        assert res["plan"]["step5_launches"] == [dict(n_slices=s, grid_y=y) for s, y, _ in launches], res["plan"]
        assert res["plan"]["step6_launches"] == [dict(n_slices=s, grid_y=1, shares_slices=shares)
                                                 for s, _, shares in launches], res["plan"]
    mc.close()
