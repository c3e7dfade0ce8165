"""The update against the oracle on meshes at and below one 64-row slice (tests/helpers_small_meshes.py: the case table,
the data, the expected plans; tests/test_step_plan.py pins the plans against plan_step() on the CPU).

Every kernel of the update works on 64-row slices, one wave per slice and four waves per block, and small meshes get
launch shapes of their own. What runs here and nowhere else in the suite: a mesh that is one partial slice, exactly one
slice, or one slice and one row (row_context() with idle lanes, the clamp of padded rows in k_lij_stage0, blocks in which
three of four waves have no slice, the tau_max reduction over mostly idle lanes); rows of 2, 4, 8 and 18 entries under the
unrolled widths 3, 9 and 27 (with four waves per slice: waves whose first column lies beyond the row); ranks that export
every owned row, ranks without a boundary row, ranks with fewer than 64 rows; the block remaps with a band or chunk
larger than the launch.

Per case, as tests/test_gpu_plan_variants.py: two warm-up updates ON THE ORACLE, both backends get that state, the third
update is compared array by array with what the Description's step-parity test uses -- helpers_parity.compare_step for
Euler, EulerAEOS and shallow water, _scalar_compare of tests/test_gpu_parity.py for scalar conservation --, and
HyperbolicModule.last_plan() must report the plan and the launches of the table. Every case runs twice: as the mesh
selects its kernels, and with the kernels of large meshes. The oracle's arrays must show the limiter and the indicator
at work (helpers_small_meshes.assert_not_vacuous). Each test prints what it measured
(profiles/small_meshes_pytest_gpu.txt)."""
import math

import numpy as np
import pytest

import helpers_plan_cases as plan_cases
import helpers_small_meshes as sm
from helpers_parity import compare_step
from helpers_partitioned import (compare_ghost_rows, compare_rank, global_scales, one_update_with_intermediates, run_hip_ranks,
                                 run_oracle_ranks)
from ryujin_amd import HyperbolicModule, TimeIntegrator, capi

pytestmark = pytest.mark.gpu


def _assert_plan(m, expected_plan, launches, label):
    got = m.last_plan()
    for key, value in expected_plan.items():
        assert got[key] == value, (label, key, got[key], value)
    assert got["step5_launches"] == launches["step5_launches"], (label, got["step5_launches"])
    assert got["step6_launches"] == launches["step6_launches"], (label, got["step6_launches"])


def _report(label, g, c=None):
    if "measured" in g:
        measured = g["measured"]
    else:   # _scalar_compare returns the arrays of both backends
        measured = {k: float(np.abs(np.asarray(g[k]) - np.asarray(c[k])).max())
                    for k in ("alpha", "r", "pij", "lij", "lij_next", "U")}
        measured["tau"] = abs(g["tau"] - c["tau"]) / c["tau"]
    print(f"\nsmall_mesh {label}: " + " ".join(f"{k}={v:.2e}" for k, v in sorted(measured.items())))


def _compare(case, off, mods, oracle, params, dirichlet, label, **kw):
    """one update on both backends through the comparison of the Description's step-parity test"""
    if case["equation"] == "scalar":
        assert not kw
        from test_gpu_parity import _scalar_compare
        g, c = _scalar_compare(off, mods, dirichlet)
    else:
        g, c = compare_step(off, mods, dirichlet, oracle=oracle, params=params, label=label, **kw)
    assert g["status"] == 0 and c["status"] == 0
    _report(label, g, c)
    return g, c


def _close(mods):
    for m, _, _ in mods:
        m.close()


# ------------------------------------------------------------------ 1. the case table, both kernel selections

@pytest.mark.parametrize("run", range(2), ids=sm.RUNS)
@pytest.mark.parametrize("name", sorted(sm.CASES))
def test_small_mesh_against_the_oracle(oracle, name, run):
    case = sm.CASES[name]
    off, dirichlet, U_start = sm.developed(name, oracle)
    this = sm.for_run(case, run)
    mods = plan_cases.both_backends(this, oracle, off, U_start)
    label = f"{name} {sm.RUNS[run]}"
    g, c = _compare(case, off, mods, oracle, plan_cases.params_of(this, oracle, off.dim), dirichlet, label)
    sm.assert_not_vacuous(case, off, c)
    _assert_plan(mods[0][0], case["plans"][run], case["launches"][run], label)
    # step 6 hands the tile mask to step 7 where every launch of it has one wave per slice, up to two dimensions
    assert mods[0][0].next_tile_mask_info()["active"] == case["tile_mask"][run], label
    _close(mods)


@pytest.mark.parametrize("name", sm.SUBSET)
def test_small_mesh_erk33_stages_with_stage_vectors(oracle, name):
    """step<1> and step<2> of ERK33 with stage vectors (step 4 stores P_ij, step 5 is k_pij_lij), formed as
    test_erk33_stages_with_stage_vectors_share_slices_in_step_6: every stage on identical inputs, the oracle's stage
    result goes to both backends"""
    case = sm.CASES[name]
    off, dirichlet, U_start = sm.developed(name, oracle)
    mods = plan_cases.both_backends(case, oracle, off, U_start)
    params = plan_cases.params_of(case, oracle, off.dim)
    (mg, og, _), (mc, oc, _) = mods
    vec = {id(mg): [og], id(mc): [oc]}
    table = [((), ()), ((0,), (-1.0,)), ((0, 1), (0.75, -2.0))]
    plan, launches = sm.stage_plan(name)
    tau = 0.0
    for stage, (idx, weights) in enumerate(table):
        for m in (mg, mc):
            vec[id(m)].append(m.new_state_vector())
            for q in idx:   # stage vectors are prepared state vectors (hyperbolic_module.h:207-213)
                m.prepare_state_vector(vec[id(m)][q], 0.0, dirichlet)
        step_mods = [(mg, vec[id(mg)][stage], vec[id(mg)][stage + 1]), (mc, vec[id(mc)][stage], vec[id(mc)][stage + 1])]
        g, c = _compare(case, off, step_mods, oracle, params, dirichlet, f"{name} erk33 stage {stage}", tau=tau,
                        stage_vectors=([vec[id(mg)][q] for q in idx], [vec[id(mc)][q] for q in idx]),
                        stage_weights=weights)
        tau = c["tau"]
        if stage > 0:
            sm.assert_not_vacuous(case, off, c)
            _assert_plan(mg, plan, launches, f"{name} erk33 stage {stage}")
        vec[id(mg)][stage + 1].upload(vec[id(mc)][stage + 1].download())
    _close(mods)


@pytest.mark.parametrize("name", sm.SUBSET)
def test_small_mesh_with_the_expensive_bounds_check(oracle, name):
    """one update with debug_expensive_bounds_check = 1 on both backends (the checked kernels behind every sweep)"""
    case = sm.CASES[name]
    off, dirichlet, U_start = sm.developed(name, oracle)
    this = sm.for_run(case, 0, dict(debug_expensive_bounds_check=1))
    mods = plan_cases.both_backends(this, oracle, off, U_start)
    oracle.lib().ryujin_oracle_set_expensive_bounds_check(mods[1][0]._ctx, 1)
    g, c = _compare(case, off, mods, oracle, plan_cases.params_of(this, oracle, off.dim), dirichlet, name + " checked")
    sm.assert_not_vacuous(case, off, c)
    plan, launches = sm.checked_plan(name)
    _assert_plan(mods[0][0], plan, launches, name + " checked")
    _close(mods)


# ------------------------------------------------------------------ 2. the same bits under the layout switches

@pytest.mark.parametrize("run", range(2), ids=sm.RUNS)
@pytest.mark.parametrize("name", sm.LAYOUT_SWITCH_CASES)
def test_small_mesh_layout_switches_give_the_same_bits(oracle, name, run):
    """The assertion of test_tile_map_gives_the_same_bits_as_the_index_arrays at sizes where every remap meets its "does
    not fill a band or chunk" branch: three updates under each switch, U, alpha and tau bit for bit those of the
    default run. (Both kernel selections: the tile mask exists with one wave per slice only.)"""
    case = sm.CASES[name]
    off, U0, dirichlet, _ = plan_cases.build(case)
    results = []
    for switches in ({},) + sm.LAYOUT_SWITCHES:
        m = HyperbolicModule(off, plan_cases.params_of(sm.for_run(case, run, switches), oracle, off.dim), backend="hip")
        a, b = m.new_state_vector(U0), m.new_state_vector()
        taus = []
        for _ in range(3):
            m.prepare_state_vector(a, 0.0, dirichlet)
            taus.append(m.step(a, [], [], b))
            assert m.last_status == 0
            a, b = b, a
        results.append((a.download(), m.alpha().copy(), np.array(taus)))
        m.close()
    assert np.isfinite(results[0][0]).all()
    for switches, other in zip(sm.LAYOUT_SWITCHES, results[1:]):
        for what, x, y in zip(("U", "alpha", "tau"), results[0], other):
            assert np.array_equal(x, y), (name, switches, what)


# ------------------------------------------------------------------ 3. ranks smaller than a slice, ranks that export everything

def _oracle_develop(oracle, parts, make, U_init, n_warm):
    from test_partitioned_vs_oracle import _develop_on
    return _develop_on(lambda *a: run_oracle_ranks(oracle, *a), parts, make, U_init, n_warm, None)


@pytest.mark.parametrize("name, equation", [(n, e) for n in sm.RANK_CASES for e in sm.RANK_CASES[n][4]])
def test_small_ranks_rank_by_rank_against_the_oracle(oracle, name, equation):
    """As _compare_partitioned of tests/test_partitioned_vs_oracle.py, with the two warm-up updates on the ORACLE ranks:
    every rank of the HIP run against the same rank of the partitioned oracle, ghost ranges and received ghost rows
    included."""
    from test_partitioned_vs_oracle import _params
    dim, _, n_ranks, counts, _ = sm.RANK_CASES[name]
    specs, parts = sm.rank_parts(name)
    if counts is not None:
        assert [sm.rank_counts(p) for p in parts] == counts
    if name in sm.RANK_N_OWNED:
        assert tuple(p.n_owned for p in parts) == sm.RANK_N_OWNED[name]
    eq = sm.EQUATIONS[equation]
    k = {capi.EQ_EULER: dim + 2, capi.EQ_SHALLOW_WATER: dim + 1}[eq]
    make = _params(oracle, eq, dim, 0.9)
    states = _oracle_develop(oracle, parts, make, sm.rank_states(equation, specs, parts), 2)
    body = one_update_with_intermediates(states, None)
    hip = run_hip_ranks(parts, make, lambda m, part, r: dict(body(m, part, r), plan=m.last_plan()))
    ref = run_oracle_ranks(oracle, parts, make, body)
    for r, part in enumerate(parts):
        # the launches of a sweep (ryujin_hip_ctx::sweep): ceil(n_export / 64) export slices, then the interior slices
        # -- none on a rank of one slice, and on a rank that exports every row: the export launch is the whole sweep
        n_all = (part.n_owned + 63) // 64
        n_export = min(n_all, (part.n_export + 63) // 64)
        sizes = [n_export] + ([n_all - n_export] if n_all > n_export else [])
        assert [q["n_slices"] for q in hip[r]["plan"]["step5_launches"]] == sizes, (r, hip[r]["plan"])
        assert [q["n_slices"] for q in hip[r]["plan"]["step6_launches"]] == sizes, (r, hip[r]["plan"])
    scales = global_scales(parts, ref, k)
    accepted = [compare_rank(part, hip[r], ref[r], k, label=f"rank {r}", scales=scales) for r, part in enumerate(parts)]
    assert all(h["status"] == 0 for h in hip)
    assert compare_ghost_rows(parts, hip, ref, accepted) > 0
    for r, part in enumerate(parts):   # every rank received and compared its ghost range
        assert part.n_relevant > part.n_owned and hip[r]["U_old"].shape[0] == part.n_relevant
        assert np.abs(ref[r]["U_old"][part.n_owned:]).min(axis=0).max() > 0.0
        assert int(part.row_starts[part.n_relevant]) > int(part.row_starts[part.n_owned])
    if dim > 1:   # the comparison of the ghost rows of l_ij is not vacuous: some ghost-row entry was actually limited
        ghost_l = np.concatenate([ref[r]["lij_next"][int(parts[r].row_starts[parts[r].n_owned]):] for r in range(n_ranks)])
        assert ghost_l.size and ghost_l.min() < 1.0


# ------------------------------------------------------------------ 4. the device-resident driver and the reductions

@pytest.mark.parametrize("scheme", ["erk 33", "ssprk 33"])
@pytest.mark.parametrize("name", sm.DRIVER_CASES)
def test_small_mesh_device_resident_time_step_equals_stagewise_driver(oracle, name, scheme):
    """the assertion of test_device_resident_time_step_equals_stagewise_driver: five steps, the same t, the same bits"""
    case = sm.CASES[name]
    off, U0, dirichlet, _ = plan_cases.build(case)
    m = HyperbolicModule(off, equation=case["eq"], backend="hip")
    sv = m.new_state_vector(U0)
    ti = TimeIntegrator(m, scheme, cfl_min=0.9, cfl_max=0.9, cfl_recovery_strategy="none",
                        dirichlet_fn=(lambda t: dirichlet) if dirichlet is not None else None)
    t_a = 0.0
    for _ in range(5):
        sv, tau = ti.step(sv, t_a)
        t_a += tau
    ref = sv.download()
    assert np.isfinite(ref).all() and t_a > 0.0

    m2 = HyperbolicModule(off, equation=case["eq"], backend="hip")
    m2.cfl = 0.9
    state = m2.new_state_vector(U0)
    temps = [m2.new_state_vector() for _ in range(3)]
    t_b = 0.0
    for n in range(5):
        t_b += m2.time_step(scheme, state, temps, dirichlet if n == 0 else None)
    assert t_a == t_b
    np.testing.assert_array_equal(state.download()[: off.n_owned], ref[: off.n_owned])
    m.close()
    m2.close()


@pytest.mark.parametrize("name", sm.DRIVER_CASES)
def test_small_mesh_device_integrals(oracle, name):
    """integrals(state) = sum_i m_i U_i, formed here with math.fsum per component, to 1e-13 relative (the bound of
    test_device_integrals_conservation_monitor), and bitwise reproducible"""
    case = sm.CASES[name]
    off, U0, dirichlet, _ = plan_cases.build(case)
    m = HyperbolicModule(off, equation=case["eq"], backend="hip")
    state = m.new_state_vector(U0)
    got = m.integrals(state)
    mi = np.asarray(off.mi)[: off.n_owned]
    ref = np.array([math.fsum((mi * U0[: off.n_owned, q]).tolist()) for q in range(U0.shape[1])])
    assert ref[0] > 0.0 and ref[-1] > 0.0
    np.testing.assert_allclose(got, ref, rtol=1e-13)
    assert np.array_equal(got, m.integrals(state))
    m.close()
