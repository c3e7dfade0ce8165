"""CPU-side checks of the shallow-water states that bring their own bathymetry (no GPU needed): names, slots, defaults
and ids of capi.IV_BATHYMETRY_STATES against the header; the strings of the reference and their ValueErrors; the two
earlier tables untouched; properties of the numpy restatements (ryujin_amd.initial_states) that follow from the
formulas; and the yardsticks of tests/test_gpu_initial_values_bathymetry.py
(tests/helpers_initial_values_bathymetry.py): 1000 points per case, every one clear of every region boundary, every
region populated, finite bounds."""
import re
import subprocess

import numpy as np
import pytest

import helpers_initial_values_bathymetry as hb
from ryujin_amd import _build, capi
from ryujin_amd import initial_states as ist

SW = capi.EQ_SHALLOW_WATER
# (family, name) -> ((parameter, first slot, default[, choices in slot order]), ...)
TABLE = {
    ("shallow water", "flow over bump"): (("flow type", 0, "transcritical", ("transcritical", "subsonic")),),
    ("shallow water", "three bumps dam break"): (("well balancing validation", 0, False, (False, True)),
                                                 ("left water depth", 1, 1.875), ("right water depth", 2, 0.0),
                                                 ("cone magnitude", 3, 1.0)),
    ("shallow water", "hou test"): (("reservoir water depth", 0, 35.0),),
    ("shallow water", "transient experiments"): (("flow state left", 0, (1.0, 0.0)), ("flow state right", 2, (1.0, 0.0)),
                                                 ("experimental configuration", 4, "G1", ("G1", "G2", "G3", "none"))),
    ("shallow water", "soliton"): (("still water depth", 0, 1.0), ("amplitude", 1, 0.1)),
}
HEADER_NAMES = {
    ("shallow water", "flow over bump"): ("RYUJIN_IV_SW_FLOW_OVER_BUMP", 21),
    ("shallow water", "three bumps dam break"): ("RYUJIN_IV_SW_THREE_BUMPS_DAM_BREAK", 22),
    ("shallow water", "hou test"): ("RYUJIN_IV_SW_HOU_TEST", 23),
    ("shallow water", "transient experiments"): ("RYUJIN_IV_SW_TRANSIENT", 24),
    ("shallow water", "soliton"): ("RYUJIN_IV_SW_SOLITON", 25),
}


def test_names_slots_and_defaults_are_the_tables():
    assert set(capi.IV_BATHYMETRY_STATES) == set(TABLE)
    for key, spec in TABLE.items():
        got = capi.IV_BATHYMETRY_STATES[key][1]
        assert [p[:4] for p in got] == [p for p in spec], key
        used = []
        for _, slot, default, *_ in spec:
            used += list(range(slot, slot + (len(default) if isinstance(default, tuple) else 1)))
        assert len(set(used)) == len(used) and max(used) < 16, key
        iv = capi.initial_values_struct(key[1], 2, equation=SW)
        assert iv.state == capi.IV_BATHYMETRY_STATES[key][0] == HEADER_NAMES[key][1]
        want = [0.0] * 16
        for _, slot, default, *choices in spec:
            if choices:
                want[slot] = float(choices[0].index(default))
                continue
            for q, v in enumerate(default if isinstance(default, tuple) else (default,)):
                want[slot + q] = v
        assert list(iv.params) == want, key
    # every selector's default is the reference's and sits in slot value 0
    for key, (_, spec) in capi.IV_BATHYMETRY_STATES.items():
        for p in spec:
            if len(p) > 3:
                assert p[3][0] == p[2] and len(p) == 5 and isinstance(p[4], str), (key, p[0])


def test_ids_and_entry_points_are_in_the_header(tmp_path):
    keys = sorted(HEADER_NAMES)
    lines = ['printf("%%d\\n", %s);' % HEADER_NAMES[k][0] for k in keys]
    uses = ["(void)ryujin_hip_initial_values_interpolate_initial_precomputed;",
            "(void)ryujin_hip_initial_values_evaluate_initial_precomputed;", "(void)ryujin_hip_get_initial_precomputed;"]
    src, exe = tmp_path / "ids.c", tmp_path / "ids"
    src.write_text('#include <stdio.h>\n#include "ryujin_hip.h"\nint main(void) { ' + " ".join(lines + uses)
                   + " return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", _build.INCLUDE, str(src),
                    "-c", "-o", str(exe) + ".o"], check=True, capture_output=True)
    src.write_text('#include <stdio.h>\n#include "ryujin_hip.h"\nint main(void) { ' + " ".join(lines) + " return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", _build.INCLUDE, str(src),
                    "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [HEADER_NAMES[k][1] for k in keys]
    for symbol in ("ryujin_hip_initial_values_interpolate_initial_precomputed",
                   "ryujin_hip_initial_values_evaluate_initial_precomputed", "ryujin_hip_get_initial_precomputed"):
        assert symbol in capi.HIP_SYMBOLS


def test_the_header_no_longer_lists_the_five_states_as_not_offered():
    with open(_build.INCLUDE + "/ryujin_hip.h") as f:
        text = f.read()
    sentence = re.search(r"Not offered:(.*?)\n \*\n", text, re.S).group(1)
    for name in ("flow over bump", "three bumps dam break", "hou test", "transient", "soliton"):
        assert name not in sentence, name
    for name in ("geotiff", "icf like", "becker solution", "perturbation"):
        assert name in sentence, name
    # the parameter names and defaults of the table stand in the header's text
    flat = " ".join(text.split()).replace("* ", "")
    for spec in TABLE.values():
        for pname, *_ in spec:
            assert f'"{pname}"' in flat, pname


def test_the_reference_strings_map_to_the_slots():
    def slots(name, dim=2, **params):
        return list(capi.initial_values_struct(name, dim, equation=SW, **params).params)

    assert slots("flow over bump", flow_type="transcritical")[0] == 0.0
    assert slots("flow over bump", 1, flow_type="subsonic")[0] == 1.0
    for index, which in enumerate(("G1", "G2", "G3", "none")):
        got = slots("transient experiments", experimental_configuration=which, flow_state_left=(2.0, 0.5))
        assert got[:5] == [2.0, 0.5, 1.0, 0.0, float(index)]
    assert slots("three bumps dam break", well_balancing_validation=True, cone_magnitude=0.5)[:4] == \
        [1.0, 1.875, 0.0, 0.5]
    assert slots("three bumps dam break", well_balancing_validation=False)[0] == 0.0
    # a number is passed on as it is: the library refuses what is none of the indices
    assert slots("flow over bump", flow_type=0.5)[0] == 0.5
    assert slots("transient experiments", experimental_configuration=5)[4] == 5.0
    with pytest.raises(ValueError, match="Flow type must be 'transcritical' or 'subsonic'"):
        slots("flow over bump", flow_type="supersonic")
    with pytest.raises(ValueError, match="Case must be 'G1', 'G2', 'G3' or 'none'"):
        slots("transient experiments", experimental_configuration="G4")
    with pytest.raises(ValueError):
        slots("three bumps dam break", well_balancing_validation="yes")
    with pytest.raises(ValueError, match="has no parameter"):
        slots("soliton", depth=1.0)
    # the numpy restatements raise the same messages
    with pytest.raises(ValueError, match="Flow type must be"):
        ist.sw_flow_over_bump_constants(9.81, "supersonic")
    with pytest.raises(ValueError, match="Case must be"):
        ist.sw_transient_bathymetry(np.zeros((1, 2)), "G4")
    # without `equation` the names are not found, as before; on another Description the struct is built (and refused
    # by the library)
    with pytest.raises(ValueError, match="Could not find"):
        capi.initial_values_struct("soliton", 1)
    assert capi.initial_values_struct("hou test", 2, equation=capi.EQ_EULER).state == capi.IV_SW_HOU_TEST


def test_the_earlier_tables_keep_their_entries():
    assert len(capi.IV_STATES) == 10 and sorted(capi.IV_STATES) == sorted(
        ("uniform", "radial contrast", "isentropic vortex", "leblanc", "rarefaction", "circular dam break",
         "paraboloid", "ritter dam break", "smooth vortex", "sloping friction"))
    assert len(capi.IV_LIBRARY_STATES) == 10 and sorted(capi.IV_LIBRARY_STATES) == sorted(
        [("euler", n) for n in ("contrast", "three state contrast", "four state contrast", "shock front", "ramp up",
                                "noh", "smooth wave", "astro jet")] +
        [("shallow water", "uniform"), ("shallow water", "contrast")])
    ids = [v[0] for v in capi.IV_STATES.values()] + [v[0] for v in capi.IV_LIBRARY_STATES.values()] + \
        [v[0] for v in capi.IV_BATHYMETRY_STATES.values()]
    assert sorted(ids) == list(range(10)) + list(range(11, 26))


# --------------------------------------------------------------------------- the restatements

def test_flow_over_bump_bed_and_initial_surface():
    x = np.array([[7.0], [7.999], [8.0], [10.0], [12.0], [12.001], [15.0], [-3.0]])
    bed = ist.sw_flow_over_bump_bathymetry(x)
    assert bed.tolist() == [0.0, 0.0, 0.0, 0.2, 0.0, 0.0, 0.0, 0.0]
    xs = np.linspace(0.0, 25.0, 2001)[:, None]
    bed = ist.sw_flow_over_bump_bathymetry(xs)
    assert (bed[(xs[:, 0] < 8.0) | (xs[:, 0] > 12.0)] == 0.0).all() and (bed >= 0.0).all() and bed.max() == 0.2
    for flow_type in ist.FLOW_OVER_BUMP_TYPES:
        h_inflow, q_inflow, _, _ = ist.sw_flow_over_bump_constants(9.81, flow_type)
        for t in (0.0, 5.0e-13):
            U, Z = ist.sw_flow_over_bump(xs, t, 9.81, flow_type)
            np.testing.assert_array_equal(Z, bed)
            assert np.abs(U[:, 0] + Z - h_inflow).max() <= 2.0 * hb.EPS * h_inflow
            assert (U[:, 1] == q_inflow).all()
    # the steady solution: Bernoulli's constant holds wherever the flow is smooth (upstream of the jump)
    _, q, cBer, _ = ist.sw_flow_over_bump_constants(9.81, "transcritical")
    U, Z = ist.sw_flow_over_bump(xs, 1.0, 9.81, "transcritical")
    smooth = (xs[:, 0] < ist.FLOW_OVER_BUMP_XS) & (np.abs(xs[:, 0] - 10.0) > 0.05)
    bernoulli = q * q / (2.0 * 9.81 * U[:, 0] ** 2) + U[:, 0] + Z
    assert np.abs(bernoulli[smooth] - cBer).max() < 1e-12
    assert (U[xs[:, 0] > ist.FLOW_OVER_BUMP_XS, 0] == ist.FLOW_OVER_BUMP_H_OUTFLOW).all()
    # subcritical before the crest, supercritical behind it: x == xS keeps the first root's formula (no outflow depth)
    froude = q / (U[:, 0] * np.sqrt(9.81 * U[:, 0]))
    assert (froude[xs[:, 0] < 9.9] < 1.0).all() and (froude[(xs[:, 0] > 10.1) & (xs[:, 0] < 11.7)] > 1.0).all()
    at_xs = ist.sw_flow_over_bump(np.array([[ist.FLOW_OVER_BUMP_XS]]), 1.0, 9.81, "transcritical")[0][0, 0]
    assert at_xs != ist.FLOW_OVER_BUMP_H_OUTFLOW and at_xs > 0.3
    # the argument of acos is -1 at the crest of the transcritical flow and inside (-1, 1) away from it
    a = ist.sw_flow_over_bump_acos_argument(np.array([[10.0], [9.0], [2.0]]), 9.81, "transcritical")
    assert abs(a[0] + 1.0) < 1e-12 and (np.abs(a[1:]) < 1.0 - 1e-3).all()


def test_three_bumps_dam_break_cones_and_dam():
    for magnitude in (1.0, 0.5):
        peaks = ist.sw_three_bumps_dam_break_bathymetry(np.array([[30.0, 6.0], [30.0, 24.0], [47.5, 15.0]]), magnitude)
        assert peaks.tolist() == [magnitude, magnitude, 3.0 * magnitude]
        assert ist.sw_three_bumps_dam_break_bathymetry(np.array([[47.5]]), magnitude).tolist() == [3.0 * magnitude]
    far = ist.sw_three_bumps_dam_break_bathymetry(np.array([[0.0, 0.0], [75.0, 30.0], [16.0, 15.0]]))
    assert (far == 0.0).all() and not np.signbit(far).any()
    # one cone in 1-D, of radius 10
    bed1 = ist.sw_three_bumps_dam_break_bathymetry(np.array([[37.4], [37.6], [57.4], [57.6]]))
    assert bed1[0] == 0.0 and bed1[1] > 0.0 and bed1[2] > 0.0 and bed1[3] == 0.0
    X = np.array([[10.0, 15.0], [16.0, 15.0], [47.5, 15.0], [30.0, 6.0]])
    U, Z = ist.sw_three_bumps_dam_break(X, 0.0)
    assert U[:, 0].tolist() == [1.875, 0.0, 0.0, 0.0] and (U[:, 1] == 0.0).all()
    U, _ = ist.sw_three_bumps_dam_break(X, 1.0e-10)                       # t <= 1e-10: still the initial state
    assert U[:, 0].tolist() == [1.875, 0.0, 0.0, 0.0]
    U, _ = ist.sw_three_bumps_dam_break(X, 2.0e-10, gravity=9.81)
    assert (U[:, 0] == 1.875).all() and (U[:, 1] == 1.875 * float(np.sqrt(9.81 * 1.875))).all()
    U, _ = ist.sw_three_bumps_dam_break(X, 5.0, well_balancing_validation=True, right_depth=1.875, cone_magnitude=0.5)
    np.testing.assert_array_equal(U[:, 0] + Z * 0.5, [1.875] * 4)         # all wet: a lake at rest


# hand-computed: (x, y) -> bed; one point inside each bump indicator, one on each paraboloid's floor
HOU_PINS = [((-250.0, 0.0), 80.0), ((-250.0, 20.0), 72.0), ((200.0, -10.0), 10.0), ((380.0, 50.0), 20.0),
            ((250.0, 0.0), 0.0), ((0.0, 50.0), 0.0), ((0.0, 80.0), 4.0)]


def test_hou_test_bed():
    X = np.array([p for p, _ in HOU_PINS])
    assert ist.sw_hou_test_bathymetry(X).tolist() == [z for _, z in HOU_PINS]
    rng = np.random.default_rng(3)
    X = np.column_stack([rng.uniform(-400.0, 500.0, 5000), rng.uniform(-150.0, 150.0, 5000)])
    bed = ist.sw_hou_test_bathymetry(X)
    # max(base, bumps) with bumps >= max(bump2, bump3) >= 0: the -10 floor of base3 never shows
    assert (bed >= 0.0).all() and (bed == 0.0).any()
    base3 = (X[:, 0] - 250.0) ** 2 / 1225.0 + X[:, 1] ** 2 / 225.0 - 10.0
    assert (base3 >= -10.0).all() and (bed[base3 < 0.0] <= 20.0).all()
    U, Z = ist.sw_hou_test(X, 35.0)
    np.testing.assert_array_equal(Z, bed)
    west = X[:, 0] < -100.0
    assert (U[~west, 0] == 0.0).all() and (U[:, 1] == 0.0).all()
    wet = west & (bed < 35.0)
    assert wet.any() and np.abs(U[wet, 0] + bed[wet] - 35.0).max() <= 64.0 * hb.EPS and (U[west & ~wet, 0] == 0.0).all()
    with pytest.raises(ValueError):
        ist.sw_hou_test_bathymetry(np.zeros((1, 1)))


def test_transient_configurations_agree_outside_the_obstacles():
    rng = np.random.default_rng(4)
    X = np.column_stack([rng.uniform(-0.5, 4.5, 4000), rng.uniform(-0.3, 0.3, 4000)])
    beds = {w: ist.sw_transient_bathymetry(X, w) for w in ist.TRANSIENT_CONFIGURATIONS}
    outside = (X[:, 0] < 1.84) | (X[:, 0] > 2.6)
    for w in ("G1", "G2", "G3"):
        np.testing.assert_array_equal(beds[w][outside], beds["none"][outside])
        assert (beds[w][~outside] != beds["none"][~outside]).any()
        assert (beds[w] >= beds["none"]).all()
    x = X[:, 0]
    knee = 326.0 / 100.0
    assert (beds["none"][x < 0.0] == 0.0).all()
    np.testing.assert_array_equal(beds["none"][(x >= 0) & (x <= knee)], -0.00092 * x[(x >= 0) & (x <= knee)])
    # the obstacles' heights: the rectangle 0.07 (G2 and G3 overwrite with it last), the bump <= 0.073, the walls 0.21
    lift = {w: beds[w] - beds["none"] for w in ("G1", "G2", "G3")}
    assert np.isclose(lift["G1"].max(), 0.07) and np.isclose(lift["G3"].max(), 0.21)
    assert 0.07 < lift["G2"].max() <= 0.073 + 1e-15
    centre = np.array([[ist.TRANSIENT_CENTERS["rectangle"], 0.0]])
    for w in ("G2", "G3"):
        assert np.isclose(ist.sw_transient_bathymetry(centre, w) - ist.sw_transient_bathymetry(centre, "none"), 0.07)
    U, _ = ist.sw_transient(np.array([[0.0, 0.0], [1.0e-8, 0.0], [2.0e-8, 0.0]]), (2.0, 0.5), (1.0, -0.25))
    assert U.tolist() == [[2.0, 0.5], [2.0, 0.5], [1.0, -0.25]]


def test_soliton_profile():
    depth, amplitude = 1.5, 0.25
    U, Z = ist.sw_soliton(np.array([[0.0, 0.0], [200.0, 1.0], [-200.0, -1.0]]), 0.0, 9.81, depth, amplitude)
    assert U[0, 0] == depth + amplitude and (Z == 0.0).all()
    assert (np.abs(U[1:, 0] - depth) < 1e-12).all() and (np.abs(U[1:, 1]) < 1e-11).all()
    celerity, _ = ist.sw_soliton_constants(9.81, depth, amplitude)
    assert U[0, 1] == (depth + amplitude) * (celerity * ((depth + amplitude) - depth) / (depth + amplitude))
    # the wave travels with its celerity
    x = np.linspace(-5.0, 5.0, 101)[:, None]
    moved, _ = ist.sw_soliton(x + celerity * 0.5, 0.5, 9.81, depth, amplitude)
    np.testing.assert_allclose(moved, ist.sw_soliton(x, 0.0, 9.81, depth, amplitude)[0], rtol=1e-13, atol=1e-14)


def test_the_beds_of_paraboloid_and_sloping_friction_are_the_earlier_ones_bit_for_bit():
    x = np.random.default_rng(6).uniform(0.0, 10000.0, 500)[:, None]
    for t in (0.0, 300.0):
        np.testing.assert_array_equal(ist.sw_paraboloid_1d_bathymetry(x, 3000.0, 10.0, 10000.0),
                                      ist.sw_paraboloid_1d(x, t, 9.81, 0.002, 3000.0, 10.0, 10000.0, 2.0)[1])
    np.testing.assert_array_equal(ist.sw_sloping_friction_bathymetry(x, 1.0e-2),
                                  ist.sw_sloping_friction(x, 0.01, 1.0e-2, 0.1)[1])
    # ... and through the helper the GPU tests compare the device's beds with
    para = hb.Case("", SW, 1, "paraboloid", {"free surface radius": 3000.0, "water height": 10.0,
                                              "paraboloid length": 10000.0, "speed": 2.0}, position=(12.5,))
    np.testing.assert_array_equal(hb.reference_bed(para, x),
                                  ist.sw_paraboloid_1d(x - 12.5, 0.0, 9.81, 0.0, 3000.0, 10.0, 10000.0, 2.0)[1])
    ramp = hb.Case("", SW, 1, "sloping friction", {"ramp slope": 1.0e-2, "initial discharge": 0.1})
    np.testing.assert_array_equal(hb.reference_bed(ramp, x), ist.sw_sloping_friction(x, 0.01, 1.0e-2, 0.1)[1])
    assert (hb.reference_bed(hb.Case("", SW, 1, "ritter dam break"), x) == 0.0).all()


# --------------------------------------------------------------------------- the yardsticks of the GPU tests

CASES = hb.function_cases()


def test_the_cases_cover_every_state_dimension_and_a_transform_each():
    assert sorted(hb.NEW_STATES) == sorted(name for _, name in capi.IV_BATHYMETRY_STATES)
    for case in CASES:
        # every parameter a case sets is one of the state's table, and the struct builds from it
        assert set(case.params) <= {p[0] for p in capi.IV_BATHYMETRY_STATES[case.key()][1]}, case.label
        iv = capi.initial_values_struct(case.name, case.dim, case.direction, case.position, equation=SW,
                                        **{k.replace(" ", "_"): v for k, v in case.params.items()})
        assert iv.state == capi.IV_BATHYMETRY_STATES[case.key()][0]
    for name in hb.NEW_STATES:
        for dim in hb.DIMS[name]:
            mine = [c for c in CASES if c.name == name and c.dim == dim]
            assert mine and all(any(c.pos()) for c in mine), (name, dim)       # a non-zero position everywhere
            if dim == 2:
                assert any(c.direction == (1.0, 1.0) for c in mine), name      # ... and a rotated direction


@pytest.mark.parametrize("case", CASES, ids=[c.label for c in CASES])
def test_points_are_clear_of_every_boundary_and_every_region_is_populated(case):
    X = hb.points_for(case)
    assert X.shape == (1000, case.dim)
    hb.assert_clear_of_jumps(case, X)
    Xt = hb.affine_transform(case.dir(), case.pos(), X)
    x = Xt[:, 0]
    if case.name == "flow over bump":
        for lo, hi in ((-np.inf, 8.0), (8.0, 10.0), (10.0, 11.7), (11.7, 12.0), (12.0, np.inf)):
            assert ((lo < x) & (x < hi)).sum() >= 10, (lo, hi)
        if hb.is_transcritical(case):
            a = ist.sw_flow_over_bump_acos_argument(Xt, hb.G, "transcritical")
            assert (1.0 - np.abs(a) >= hb.ACOS_MARGIN).all() and (1.0 - np.abs(a)).min() < 0.05
    elif case.name == "three bumps dam break":
        bed = hb.reference_bed(case, X)
        assert (bed > 0.0).sum() >= 100 and (bed == 0.0).sum() >= 100 and (x < 16.0).sum() >= 100
    elif case.name == "hou test":
        y = Xt[:, 1]
        assert ((x - 200.0) ** 2 + (y + 10.0) ** 2 <= 1000.0).sum() >= 3
        assert ((np.abs(x - 380.0) <= 40.0) & (np.abs(y - 50.0) <= 40.0)).sum() >= 10
        assert (x < -100.0).sum() >= 100
    elif case.name == "transient experiments":
        which = case.get("experimental configuration")
        lift = hb.reference_bed(case, X) - ist.sw_transient_bathymetry(Xt, "none")
        if which != "none":
            assert np.isclose(lift, 0.07).sum() >= 3, which
        if which == "G3":
            assert np.isclose(lift, 0.21).sum() >= 5
        if which == "G2":
            assert ((lift > 0.0) & (lift < 0.0699)).sum() >= 5
        assert (x > 1.0e-8).sum() >= 100 and (x < 0.0).sum() >= 50
    for t in case.times:
        U, bed = hb.reference(case, X, t)
        tol_state, tol_bed = hb.tolerance(case, X, t)
        assert np.isfinite(U).all() and np.isfinite(bed).all()
        assert np.isfinite(tol_state).all() and np.isfinite(tol_bed).all()
        assert (tol_state >= 0.0).all() and tol_state.max() <= 1.0e-11 * max(1.0, np.abs(U).max())
        assert tol_bed.max() <= (1.0e-7 if case.name == "transient experiments" else 1.0e-10)
        # what both sides copy from a parameter, or select as the 0 of a max, is demanded bit for bit by the bound
        if case.name == "transient experiments" and hb.exact_transform(case):
            assert (tol_state[:, 0] == 0.0).all()
    mask = hb.bitwise_bed_mask(case, X)
    if mask is not None:
        assert mask.sum() >= 300, case.label
