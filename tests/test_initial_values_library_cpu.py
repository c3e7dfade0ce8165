"""CPU-side checks of the Riemann-data, shock-front, ramp-up and Noh states (no GPU needed): names, slots, defaults
and ids against the header; the yardsticks of tests/test_gpu_initial_values_library.py
(tests/helpers_initial_values_library.py) -- every point clear of every region boundary, the error arithmetic against
the restatement it bounds --; and the numpy restatements as data of the reference's two verification setups on the CPU
oracle, against the reference's recorded results."""
import subprocess

import numpy as np
import pytest

import helpers_initial_values_library as hl
import test_oracle_golden_verification as tv
from ryujin_amd import _build, capi
from ryujin_amd import initial_states as ist

# the table of the states: (family, name) -> ((parameter, first slot, default), ...)
TABLE = {
    ("euler", "contrast"): (("primitive state left", 0, (1.4, 0.0, 1.0)), ("primitive state right", 3, (1.4, 0.0, 1.0))),
    ("euler", "three state contrast"): (("primitive state left", 0, (1.0, 0.0, 1.0e3)), ("left region length", 3, 0.1),
                                        ("primitive state middle", 4, (1.0, 0.0, 1.0e-2)),
                                        ("middle region length", 7, 0.8),
                                        ("primitive state right", 8, (1.0, 0.0, 1.0e2))),
    ("euler", "four state contrast"): (("primitive state bottom left", 0, (1.4, 0.0, 0.0, 1.0)),
                                       ("primitive state bottom right", 4, (1.4, 0.0, 0.0, 1.0)),
                                       ("primitive state top left", 8, (1.4, 0.0, 0.0, 1.0)),
                                       ("primitive state top right", 12, (1.4, 0.0, 0.0, 1.0))),
    ("euler", "shock front"): (("primitive state", 0, (1.4, 0.0, 1.0)), ("mach number", 3, 2.0), ("gamma", 4, 1.4)),
    ("euler", "ramp up"): (("primitive state initial", 0, (1.4, 0.0, 1.0)), ("primitive state final", 3, (1.4, 3.0, 1.0)),
                           ("time initial", 6, 0.0), ("time final", 7, 1.0)),
    ("euler", "noh"): (("reference density", 0, 1.0), ("reference velocity magnitude", 1, 1.0),
                       ("reference pressure", 2, 1.0e-12), ("gamma", 3, 1.4)),
    ("euler", "smooth wave"): (("reference density", 0, 1.0), ("reference pressure", 1, 1.0), ("mach number", 2, 1.0)),
    ("euler", "astro jet"): (("jet width", 0, 0.05), ("primitive jet state", 1, (5.0, 30.0, 0.4127)),
                             ("primitive ambient right", 4, (5.0, 0.0, 0.4127)), ("gamma", 7, 5.0 / 3.0)),
    ("shallow water", "uniform"): (("primitive state", 0, (1.0, 1.0)),),
    ("shallow water", "contrast"): (("primitive state left", 0, (1.0, 0.0)), ("primitive state right", 2, (1.0, 0.0))),
}
HEADER_NAMES = {
    ("euler", "contrast"): "RYUJIN_IV_CONTRAST", ("euler", "three state contrast"): "RYUJIN_IV_THREE_STATE_CONTRAST",
    ("euler", "four state contrast"): "RYUJIN_IV_FOUR_STATE_CONTRAST", ("euler", "shock front"): "RYUJIN_IV_SHOCK_FRONT",
    ("euler", "ramp up"): "RYUJIN_IV_RAMP_UP", ("euler", "noh"): "RYUJIN_IV_NOH",
    ("euler", "smooth wave"): "RYUJIN_IV_SMOOTH_WAVE", ("euler", "astro jet"): "RYUJIN_IV_ASTRO_JET",
    ("shallow water", "uniform"): "RYUJIN_IV_SW_UNIFORM", ("shallow water", "contrast"): "RYUJIN_IV_SW_CONTRAST",
}


def test_names_slots_and_defaults_are_the_tables():
    assert set(capi.IV_LIBRARY_STATES) == set(TABLE)
    for key, spec in TABLE.items():
        assert capi.IV_LIBRARY_STATES[key][1] == spec, key
        # the slots of a state do not overlap and stay inside params[16]
        used = []
        for _, slot, default in spec:
            used += list(range(slot, slot + (len(default) if isinstance(default, tuple) else 1)))
        assert len(set(used)) == len(used) and max(used) < 16, key
    eq = {"euler": capi.EQ_EULER, "shallow water": capi.EQ_SHALLOW_WATER}
    for (family, name), spec in TABLE.items():
        iv = capi.initial_values_struct(name, 2, equation=eq[family])
        assert iv.state == capi.IV_LIBRARY_STATES[(family, name)][0]
        want = [0.0] * 16
        for _, slot, default in spec:
            for q, v in enumerate(default if isinstance(default, tuple) else (default,)):
                want[slot + q] = v
        assert list(iv.params) == want, (family, name)
    four = capi.initial_values_struct("four state contrast", 2, equation=capi.EQ_EULER_AEOS,
                                      primitive_state_top_right=(1.5, 0.25, -0.5, 2.0))
    assert list(four.params)[12:] == [1.5, 0.25, -0.5, 2.0]          # all 16 slots are in use
    jet = capi.initial_values_struct("astro jet", 3, equation=capi.EQ_EULER, jet_width=0.1)
    assert list(jet.params)[:8] == [0.1, 5.0, 30.0, 0.4127, 5.0, 0.0, 0.4127, 5.0 / 3.0]


def test_ids_are_distinct_from_eleven_on_and_the_headers(tmp_path):
    ids = {key: value[0] for key, value in capi.IV_LIBRARY_STATES.items()}
    assert len(set(ids.values())) == len(ids) and min(ids.values()) >= 11
    assert not set(ids.values()) & {v[0] for v in capi.IV_STATES.values()}
    keys = sorted(HEADER_NAMES)
    lines = ['printf("%%d\\n", %s);' % HEADER_NAMES[k] for k in keys]
    src, exe = tmp_path / "ids.c", tmp_path / "ids"
    src.write_text('#include <stdio.h>\n#include "ryujin_hip.h"\nint main(void) { ' + " ".join(lines)
                   + " return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", _build.INCLUDE, str(src),
                    "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [ids[k] for k in keys]


def test_the_equation_keyword_changes_nothing_for_the_ten_earlier_names():
    def same(a, b):
        return bytes(a) == bytes(b)

    for name, (state, shallow, _) in capi.IV_STATES.items():
        plain = capi.initial_values_struct(name, 2, direction=(1.0, 1.0), position=(0.5, -0.5))
        assert plain.state == state
        assert same(plain, capi.initial_values_struct(name, 2, direction=(1.0, 1.0), position=(0.5, -0.5),
                                                      equation=None))
        own = capi.EQ_SHALLOW_WATER if shallow else capi.EQ_EULER
        assert same(plain, capi.initial_values_struct(name, 2, direction=(1.0, 1.0), position=(0.5, -0.5),
                                                      equation=own))
    # the two names that exist twice
    assert capi.initial_values_struct("uniform", 1).state == capi.IV_UNIFORM
    assert capi.initial_values_struct("uniform", 1, equation=capi.EQ_EULER_AEOS).state == capi.IV_UNIFORM
    assert capi.initial_values_struct("uniform", 1, equation=capi.EQ_SHALLOW_WATER).state == capi.IV_SW_UNIFORM
    assert capi.initial_values_struct("contrast", 1, equation=capi.EQ_EULER).state == capi.IV_CONTRAST
    assert capi.initial_values_struct("contrast", 1, equation=capi.EQ_SHALLOW_WATER).state == capi.IV_SW_CONTRAST
    assert capi.IV_SW_UNIFORM != capi.IV_UNIFORM and capi.IV_SW_CONTRAST != capi.IV_CONTRAST
    # a scalar context gets the struct of the state, which the library then refuses; unknown names stay ValueError
    assert capi.initial_values_struct("uniform", 1, equation=capi.EQ_SCALAR_CONSERVATION).state == capi.IV_UNIFORM
    assert capi.initial_values_struct("noh", 1, equation=capi.EQ_SCALAR_CONSERVATION).state == capi.IV_NOH
    for equation in (None, capi.EQ_EULER, capi.EQ_SHALLOW_WATER):
        with pytest.raises(ValueError):
            capi.initial_values_struct("function", 1, equation=equation)
        with pytest.raises(ValueError):
            capi.initial_values_struct("no such state", 1, equation=equation)
    with pytest.raises(ValueError):
        capi.initial_values_struct("shock front", 1)            # without the equation: the ten earlier names only
    with pytest.raises(ValueError):
        capi.initial_values_struct("noh", 1, equation=capi.EQ_EULER, radius=1.0)


def test_restatements_against_hand_computed_values():
    """the constants the host forms, from the formulas of the reference's constructors evaluated by hand"""
    # a Mach-2 shock into (1.4, 0, 1), gamma 1.4: a_R = 1, S3 = 2, rho_L / rho_R = 2.4 * 4 / (0.4 * 4 + 2) = 8/3,
    # p_L / p_R = (2.8 * 4 - 0.4) / 2.4 = 4.5, u_L = (1 - 3/8) * 2 = 1.25
    (rho_L, u_L, p_L), S3 = ist.euler_shock_front_constants((1.4, 0.0, 1.0), 2.0, 1.4)
    np.testing.assert_allclose([rho_L, u_L, p_L, S3], [1.4 * 8.0 / 3.0, 1.25, 4.5, 2.0], rtol=4e-16)
    # Mach 10 into (1.4, 0, 1): the post-shock state of the double Mach reflection, (8, 8.25, 116.5)
    (rho_L, u_L, p_L), S3 = ist.euler_shock_front_constants((1.4, 0.0, 1.0), 10.0, 1.4)
    np.testing.assert_allclose([rho_L, u_L, p_L, S3], [8.0, 8.25, 116.5, 10.0], rtol=1e-15)
    # noh, gamma = 5/3: D = 1/3, interior density 4^dim, interior pressure 1/2 (8/3)^dim / (2/3)^(dim - 1)
    for dim, rho_in, p_in in ((1, 4.0, 4.0 / 3.0), (2, 16.0, 16.0 / 3.0), (3, 64.0, 64.0 / 3.0)):
        D, rho, p = ist.euler_noh_constants(dim, 1.0, 1.0, 5.0 / 3.0)
        np.testing.assert_allclose([D, rho, p], [1.0 / 3.0, rho_in, p_in], rtol=1e-14)
    # ... t == 0 is never interior, the velocity is radial with magnitude u0
    X = np.array([[0.0, 0.0], [3.0, 4.0], [1e-3, 0.0]])
    rho, vel, p = ist.euler_noh_primitive(X, 0.0, 1.0, 2.0, 1e-12, 5.0 / 3.0)
    np.testing.assert_array_equal(rho, 1.0)
    np.testing.assert_allclose(vel, [[0.0, 0.0], [-1.2, -1.6], [-2.0, 0.0]], rtol=1e-15)
    rho, vel, p = ist.euler_noh_primitive(X, 1.0, 1.0, 2.0, 1e-12, 5.0 / 3.0)       # D t = 2/3
    np.testing.assert_allclose(rho, [16.0, 1.0 + 1.0 / 5.0, 16.0], rtol=1e-15)
    np.testing.assert_array_equal(vel[[0, 2]], 0.0)
    # smooth wave: the polynomial is 1 at the middle of [0.1, 0.3] and 0 at its ends
    rho, vel, p = ist.euler_smooth_wave_primitive(np.array([[0.2 + 0.5], [0.1 + 0.5], [0.0]]), 0.5, 1.0, 1.0, 1.0)
    np.testing.assert_allclose(rho, [2.0, 1.0, 1.0], atol=1e-14)
    assert ist.fixed_power_3(2.0) == 8.0 and ist.fixed_power_6(2.0) == 64.0
    # ramp up: cos^2 weights
    assert ist.euler_ramp_up_weights(0.1, 0.1, 0.3) == (1.0, 0.0) and ist.euler_ramp_up_weights(0.3, 0.1, 0.3) == (0.0, 1.0)
    np.testing.assert_allclose(ist.euler_ramp_up_weights(0.2, 0.1, 0.3), (0.5, 0.5), atol=2e-16)
    # four state contrast and astro jet have no 1-D form
    for fn in (ist.euler_four_state_contrast_primitive, ist.euler_astro_jet_primitive):
        with pytest.raises(ValueError):
            fn(np.zeros((1, 1)))


CASES = hl.function_cases()


def test_every_new_state_is_covered_in_every_dimension_it_has():
    for eq, eos in ((capi.EQ_EULER, None), (capi.EQ_EULER_AEOS, capi.EOS_POLYTROPIC_GAS),
                    (capi.EQ_EULER_AEOS, capi.EOS_NOBLE_ABEL_STIFFENED_GAS)):
        have = {(c.name, c.dim) for c in CASES if c.equation == eq and c.edits.get("eos") == eos
                and not c.eos_function}
        assert have == {(n, d) for n in hl.EULER_STATES for d in (1, 2, 3) if d >= hl.MIN_DIM.get(n, 1)}
    assert any(c.eos_function for c in CASES)
    assert {(c.name, c.dim) for c in CASES if c.equation == capi.EQ_SHALLOW_WATER} == \
        {(n, d) for n in hl.SW_STATES for d in (1, 2)}
    assert {c.name for c in CASES if c.equation != capi.EQ_SHALLOW_WATER} == \
        {n for f, n in capi.IV_LIBRARY_STATES if f == "euler"}
    for c in CASES:
        assert c.times[0] == 0.0 and len(c.times) == 3 and min(c.times[1:]) > 0.0
        assert c.dim == 1 or c.direction == (1.0,) * c.dim
        if c.name == "ramp up":
            t_i, t_f = c.get("time initial"), c.get("time final")
            assert c.times[0] < t_i < c.times[1] < t_f < c.times[2]
    assert len({c.label for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.label for c in CASES])
def test_points_are_clear_of_the_jumps_and_the_error_arithmetic_follows_the_restatement(case):
    """What GPU test A relies on, checked without a GPU: ALL 1000 points of a case are further than 1e-9 (1 + |x|)
    from every region boundary at its three times (nothing is dropped); the formulas restated in the error arithmetic
    give the values of ryujin_amd.initial_states within their own bound; the bound is finite and at most
    1e-12 scale + 1e-12; the points see the regions of a piecewise state."""
    X = hl.points_for(case)
    assert X.shape == (1000, case.dim)
    regions, sides_of_noh = set(), set()
    for t in case.times:
        clearance = hl.jump_clearance(case, X, t)
        assert clearance.shape == (1000,) and (clearance > 0.0).all(), (case.label, t)
        ref = hl.reference(case, X, t)
        val, tol = hl.tolerance(case, X, t)
        assert ref.shape == val.shape == tol.shape == (1000, case.dim + (1 if case.equation == capi.EQ_SHALLOW_WATER
                                                                         else 2))
        assert np.isfinite(ref).all() and np.isfinite(tol).all() and (tol >= 0.0).all()
        assert (np.abs(val - ref) <= tol).all()
        scale = np.abs(ref).max(axis=0)
        assert (tol <= 1e-12 * np.maximum(scale, 1e-300) + 1e-12).all()
        ids = hl.region_ids(case, X, t)
        if case.name == "noh":
            if t > 0.0:
                assert set(ids.tolist()) == {0, 1}, (case.label, t)     # points on both sides of |x| / t = D
                sides_of_noh |= set(ids.tolist())
        else:
            regions |= set(ids.tolist())
    if hl.is_jump_state(case) and case.name != "noh":
        assert len(regions) >= hl.N_REGIONS.get(case.name, 2), (case.label, regions)
    if case.name == "noh":
        assert sides_of_noh == {0, 1}


# --------------------------------------------------------------------------- the oracle runs

def test_the_baseline_fixtures_start_with_the_401_dof_block(golden_dir):
    for name in (hl.SMOOTH_WAVE_GOLDEN, hl.SHOCK_FRONT_GOLDEN):
        dofs, t, linf, l1, l2 = tv.golden(golden_dir, name)
        assert dofs == 401 and t > 0.0 and linf > 0.0 and l1 > 0.0 and l2 > 0.0


@pytest.mark.parametrize("name", sorted(hl.VERIFICATION))
def test_verification_setups_on_the_oracle_with_the_restatements_as_data(oracle, golden_dir, name):
    """prm/verification/euler-{smooth_wave,shock_front}-erk33.prm at 401 DoFs on the CPU oracle: initial state,
    Dirichlet data at the stage times and the reference of the error norms are the numpy restatements. Against the
    reference's recorded results (written by another version of the reference: offsets of 1e-8 / 1e-6 in t and up to
    5.8e-4 in the norms were measured, at 801 DoFs the same) within rtol_t = 5e-6 and rtol_err = 1.5e-3 -- far below
    the O(1) change of L1 a wrong shock speed or wave position gives."""
    gold, _, _, cfl, relaxation, t_final = hl.VERIFICATION[name]
    res = tv.run_verification(oracle.backend(), hl.verification_mesh(), hl.verification_params(
        oracle.default_params, relaxation), hl.verification_exact(name), (0, 1, 2), cfl=cfl, t_final=t_final)
    g = tv.golden(golden_dir, gold)
    print(f"{name}: t {res['t']!r} Linf {res['linf']!r} L1 {res['l1']!r} L2 {res['l2']!r}; relative to the baseline "
          f"{[abs(a - b) / b for a, b in zip((res['t'], res['linf'], res['l1'], res['l2']), g[1:])]}")
    tv.check(res, g, **hl.VERIFICATION_TOL)
