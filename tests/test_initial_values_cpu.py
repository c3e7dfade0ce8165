"""CPU-side checks of the device-resident InitialValues (no GPU needed): the new entry points are exported and
mirrored, the ctypes struct has the header's layout, and the numpy yardsticks of tests/test_gpu_initial_values.py
(tests/helpers_initial_values.py) are themselves right -- the affine transform against hand-computed rotations, the
error arithmetic against the restatement it bounds, the points of the function-level test against the jumps."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import helpers_initial_values as hiv
from ryujin_amd import _build, capi
from ryujin_amd import initial_states as ist

NEW_SYMBOLS = ("ryujin_hip_initial_values_configure", "ryujin_hip_initial_values_evaluate",
               "ryujin_hip_initial_values_interpolate", "ryujin_hip_prepare_state_vector_iv",
               "ryujin_hip_time_step_iv")


def test_the_library_exports_the_new_entry_points():
    lib = capi.load_hip()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.HIP_SYMBOLS
        assert getattr(lib, name).argtypes is not None, name


def test_the_ctypes_struct_has_the_headers_layout(tmp_path):
    fields = [f[0] for f in capi.InitialValues._fields_]
    lines = ['printf("%zu\\n", sizeof(ryujin_hip_initial_values));']
    lines += ['printf("%%zu\\n", offsetof(ryujin_hip_initial_values, %s));' % f for f in fields]
    lines += ['printf("%d\\n", RYUJIN_IV_UNIFORM); printf("%d\\n", RYUJIN_IV_SLOPING_FRICTION);']
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ryujin_hip.h"\nint main(void) { '
                   + " ".join(lines) + " return 0; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", _build.INCLUDE, str(src),
                    "-o", str(exe)], check=True, capture_output=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(capi.InitialValues)
    assert out[1:-2] == [getattr(capi.InitialValues, f).offset for f in fields]
    assert out[-2:] == [capi.IV_UNIFORM, capi.IV_SLOPING_FRICTION]


def test_entries_refuse_a_null_context_without_touching_a_device():
    lib = capi.load_hip()
    iv = capi.initial_values_struct("uniform", 1)
    assert lib.ryujin_hip_initial_values_configure(None, C.byref(iv), None, None) == capi.RYUJIN_ERR_ARG
    assert lib.ryujin_hip_initial_values_evaluate(None, None, 0, 0.0, None) == capi.RYUJIN_ERR_ARG
    assert lib.ryujin_hip_initial_values_interpolate(None, 0, 0.0) == capi.RYUJIN_ERR_ARG
    assert lib.ryujin_hip_prepare_state_vector_iv(None, 0, 0.0) == capi.RYUJIN_ERR_ARG
    tau = C.c_double()
    assert lib.ryujin_hip_time_step_iv(None, capi.SCHEME_ERK_33, 0, 3, None, 0.0, 1.0, 0, 0.2, 0.2,
                                       C.byref(tau)) == capi.RYUJIN_ERR_ARG


def test_configuration_names_and_parameters_are_the_references():
    iv = capi.initial_values_struct("isentropic vortex", 2, direction=(1.0, 1.0), position=(-1.0, -1.0),
                                    mach_number=1.0)
    assert iv.state == capi.IV_ISENTROPIC_VORTEX
    assert list(iv.params)[:3] == [1.0, 5.0, 1.4]        # "mach number", "beta" [5], "gamma" [1.4]
    assert list(iv.direction) == [1.0, 1.0, 0.0] and list(iv.position) == [-1.0, -1.0, 0.0]
    iv = capi.initial_values_struct("radial contrast", 3, primitive_state_outer=(0.125, 0.0, 0.1), radius=0.25)
    assert list(iv.params)[:7] == [1.0, 0.0, 100.0, 0.125, 0.0, 0.1, 0.25] and list(iv.direction) == [1.0, 0.0, 0.0]
    iv = capi.initial_values_struct("ritter dam break", 1, **{"time initial": 1.0})
    assert list(iv.params)[:2] == [1.0, 0.005]
    assert sorted(capi.IV_STATES) == sorted(["uniform", "radial contrast", "isentropic vortex", "leblanc",
                                             "rarefaction", "circular dam break", "paraboloid", "ritter dam break",
                                             "smooth vortex", "sloping friction"])
    assert sorted(v[0] for v in capi.IV_STATES.values()) == list(range(10))
    with pytest.raises(ValueError):
        capi.initial_values_struct("function", 1)
    with pytest.raises(ValueError):
        capi.initial_values_struct("uniform", 1, radius=1.0)
    with pytest.raises(ValueError):
        capi.initial_values_struct("uniform", 2, direction=(1.0,))


def test_affine_transform_against_hand_computed_rotations():
    """initial_values.template.h:66-148 in 3-D. direction e_z: one roll about y by 90 degrees, x' = (z, y, -x);
    direction e_y: one roll about z, x' = (y, -x, z); direction (1, 1, 1): BOTH rolls are by 45 degrees (the second
    uses the original direction's x and y), so e_x goes to (1/2, -1/2, -1/sqrt 2) and a momentum along the profile
    comes back as (1/2, 1/sqrt 2, 1/2)."""
    s = np.sqrt(0.5)
    x = np.array([[1.0, 2.0, 3.0]])
    np.testing.assert_allclose(hiv.affine_transform((0, 0, 1), (0, 0, 0), x), [[3.0, 2.0, -1.0]], atol=1e-15)
    np.testing.assert_allclose(hiv.affine_transform((0, 2, 0), (0, 0, 0), x), [[2.0, -1.0, 3.0]], atol=1e-15)
    np.testing.assert_allclose(hiv.affine_transform((1, 0, 0), (0.5, 1.0, -1.0), x), [[0.5, 1.0, 4.0]], atol=0)
    np.testing.assert_allclose(hiv.affine_transform((1, 1, 0), (0, 0, 0), [[1.0, 1.0, 7.0]]),
                               [[np.sqrt(2.0), 0.0, 7.0]], atol=2e-16)
    e_x = np.array([[1.0, 0.0, 0.0]])
    np.testing.assert_allclose(hiv.affine_transform((1, 1, 1), (0, 0, 0), e_x), [[0.5, -0.5, -s]], atol=2e-16)
    np.testing.assert_allclose(hiv.affine_transform_vector((1, 1, 1), e_x), [[0.5, s, 0.5]], atol=2e-16)
    np.testing.assert_allclose(hiv.affine_transform_vector((0, 0, 1), e_x), [[0.0, 0.0, 1.0]], atol=1e-15)
    np.testing.assert_allclose(hiv.affine_transform_vector((0, 1, 0), e_x), [[0.0, 1.0, 0.0]], atol=1e-15)
    np.testing.assert_allclose(hiv.affine_transform_vector((3, 4), [[5.0, 0.0]]), [[3.0, 4.0]], atol=1e-15)
    # the momentum rotation undoes the point rotation, whatever the direction
    rng = np.random.default_rng(3)
    for dim in (2, 3):
        for _ in range(5):
            d, v = rng.normal(size=dim), rng.normal(size=(20, dim))
            back = hiv.affine_transform_vector(d, hiv.affine_transform(d, np.zeros(dim), v))
            np.testing.assert_allclose(back, v, atol=1e-14)
    # 1-D: the translation only
    np.testing.assert_array_equal(hiv.affine_transform((-1.0,), (0.25,), [[1.0]]), [[0.75]])
    # ... and the 2-D restatements of ryujin_amd.initial_states compose the same transform
    X = rng.uniform(-3, 3, size=(50, 2))
    Xt = hiv.affine_transform((1.0, 1.0), (-1.0, -1.0), X)
    rho, u, v, p, _ = ist.euler_isentropic_vortex_primitive(X, 0.0, direction=(1.0, 1.0), position=(-1.0, -1.0))
    rho2, u2, v2, p2, _ = ist.euler_isentropic_vortex_primitive(Xt, 0.0, direction=(1.0, 0.0), position=(0.0, 0.0))
    np.testing.assert_allclose(rho, rho2, rtol=1e-14)


CASES = hiv.function_cases()


def test_every_state_of_both_descriptions_is_covered():
    euler = {c.name for c in CASES if c.equation == capi.EQ_EULER}
    aeos = {(c.name, c.edits.get("eos")) for c in CASES if c.equation == capi.EQ_EULER_AEOS}
    sw = {c.name for c in CASES if c.equation == capi.EQ_SHALLOW_WATER}
    assert euler == set(hiv.EULER_STATES)
    assert aeos == {(n, e) for n in hiv.EULER_STATES
                    for e in (capi.EOS_POLYTROPIC_GAS, capi.EOS_NOBLE_ABEL_STIFFENED_GAS)}
    assert sw == {"circular dam break", "paraboloid", "ritter dam break", "smooth vortex", "sloping friction"}
    for name in ("leblanc", "uniform"):
        assert {(c.dim, c.direction) for c in CASES if c.name == name and c.equation == capi.EQ_EULER} == \
            {(1, None), (2, (1.0, 1.0)), (3, (1.0, 1.0, 1.0))}
    for c in CASES:
        assert c.times[0] == 0.0 and len(c.times) == 3 and min(c.times[1:]) > 0.0


@pytest.mark.parametrize("case", CASES, ids=[c.label for c in CASES])
def test_points_are_clear_of_the_jumps_and_the_error_arithmetic_follows_the_restatement(case):
    """What GPU test A relies on, checked without a GPU: all 1000 points of a case are further than 1e-9 (1 + |x|)
    from every region boundary at its three times; the formulas restated in the error arithmetic give the values of
    ryujin_amd.initial_states within their own bound (they ARE the same statements); the bound is finite, and a few
    1e-14 of the component's scale at most except where the value itself is ill-conditioned."""
    X = hiv.points_for(case)
    assert X.shape == (1000, case.dim)
    regions = set()
    for t in case.times:
        hiv.assert_clear_of_jumps(case, X, t)
        ref = hiv.reference(case, X, t)
        val, tol = hiv.tolerance(case, X, t)
        assert ref.shape == val.shape == tol.shape and np.isfinite(ref).all() and np.isfinite(tol).all()
        assert (np.abs(val - ref) <= tol).all()
        scale = np.abs(ref).max(axis=0)
        assert (tol <= 1e-12 * np.maximum(scale, 1e-300) + 1e-12).all()
        regions |= set(np.round(ref[:, 0], 12).tolist()) if case.name in hiv.JUMP_STATES else set()
    if case.name in hiv.JUMP_STATES:
        assert len(regions) >= 2                  # the points see both sides of a jump
