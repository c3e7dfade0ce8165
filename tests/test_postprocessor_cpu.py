"""CPU: the numpy restatement of Postprocessor::compute() (tests/helpers_postprocessor.py, the yardstick of
tests/test_gpu_postprocessor.py) on analytic fields, the properties of the normalisation, the name resolution of
HyperbolicModule.postprocess() and the C declarations of the new entry points."""
import subprocess

import numpy as np
import pytest

import helpers_postprocessor as hp
from ryujin_amd import _build, capi, offline


def _meshes():
    return [offline.SyntheticOffline(offline.mach3_step_2d(20)), offline.SyntheticOffline(offline.box_3d(12))]


@pytest.mark.parametrize("off", _meshes(), ids=["mach3_step_2d", "box_3d"])
def test_gradient_of_a_linear_field_is_exact_on_every_row(off):
    """q = a.x + b: sum_j c_ij q_j / m_i = a on EVERY owned row, boundary rows included (partition of unity and
    sum_j c_ij x_j = m_i Id hold for the generator's stencils), so the schlieren value is |a|."""
    dim = off.dim
    a = np.array([0.7, -1.3, 0.4])[:dim]
    x = off.positions
    U = np.zeros((off.n_relevant, dim + 2))
    U[:, 0] = x @ a + 2.5
    U[:, 1:] = 1.0
    rows, cols, c, mi, lens = hp.csr(off)
    assert lens.min() > 1  # neither mesh has a constrained row
    grad = np.stack([np.bincount(rows, weights=c[:, d] * U[cols, 0], minlength=off.n_owned) for d in range(dim)], 1)
    assert np.abs(grad / mi[:, None] - a).max() < 5e-14
    raw, scale = hp.raw_values(off, U, [(hp.SCHLIEREN, 0, 0)])
    assert np.abs(raw[0] - np.linalg.norm(a)).max() < 5e-14
    assert (hp.raw_tolerance(scale[0]) > 0).all() and hp.raw_tolerance(scale[0]).max() < 1e-9


def test_signed_curl_of_a_rigid_rotation_2d():
    """v = omega (-y, x), counter-clockwise: +2 omega on every row; the mirrored rotation gives -2 omega"""
    off = _meshes()[0]
    x = off.positions
    for omega in (0.8, -0.8):
        U = np.ones((off.n_relevant, 4))
        U[:, 1], U[:, 2] = -omega * x[:, 1], omega * x[:, 0]
        raw, _ = hp.raw_values(off, U, [(hp.VORTICITY, 0, 1)])
        assert np.abs(raw[0] - 2.0 * omega).max() < 1e-13
        # ... and of the primitive velocity of a state with rho = 2 (m = rho v)
        U[:, 0] = 2.0
        U[:, 1:3] *= 2.0
        U[:, 3] = 50.0
        p = capi.Params()
        p.gamma = 1.4
        raw, _ = hp.raw_values(off, U, [(hp.VORTICITY, 1, 1), (hp.VORTICITY, 0, 1)], capi.EQ_EULER, p)
        assert np.abs(raw[0] - 2.0 * omega).max() < 1e-13 and np.abs(raw[1] - 4.0 * omega).max() < 1e-13


def test_curl_norm_of_a_rigid_rotation_3d():
    off = _meshes()[1]
    x = off.positions
    w = np.array([0.3, -0.5, 0.9])
    U = np.ones((off.n_relevant, 5))
    U[:, 1:4] = np.cross(w, x)
    raw, _ = hp.raw_values(off, U, [(hp.VORTICITY, 0, 1)])
    assert np.abs(raw[0] - 2.0 * np.linalg.norm(w)).max() < 1e-13


def test_rows_of_length_one_get_zero():
    """a constrained DoF (row of length 1) is skipped: 0, whatever the field"""
    class One:
        dim, n_owned, n_relevant = 2, 2, 2
        row_starts = np.array([0, 1, 3], dtype=np.uint64)
        columns = np.array([0, 1, 0], dtype=np.uint32)
        cij = np.array([[1.0, 2.0], [0.5, 0.0], [-0.5, 0.0]])
        mi = np.array([1.0, 2.0])

        class c:
            class contents:
                simd_length, n_internal = 1, 0
    U = np.array([[3.0], [5.0]])
    raw, _ = hp.raw_values(One, U, [(hp.SCHLIEREN, 0, 0)], capi.EQ_SCALAR_CONSERVATION)
    assert raw[0, 0] == 0.0 and raw[0, 1] == abs(0.5 * 5.0 - 0.5 * 3.0) / 2.0


def test_normalisation_properties():
    rng = np.random.default_rng(7)
    beta = 10.0
    # schlieren: non-negative raw values -> [0, 1)
    raw = np.abs(rng.normal(size=1000)) * 3.0
    q_max, q_min = hp.bounds(raw)
    out = hp.normalise(raw, q_max, q_min, beta)
    assert (out >= 0.0).all() and (out < 1.0).all()
    # the row holding q_max: ratio = 1 - floor / (q_max - q_min)
    expected = 1.0 - np.exp(-beta * (1.0 - hp.FLOOR / (q_max - q_min)))
    assert abs(out[raw.argmax()] - expected) <= 4 * hp.EPS
    # the row holding q_min is clipped to exactly 0 by the floor
    assert out[raw.argmin()] == 0.0
    # 2-D vorticity: the sign of the raw value is kept, the magnitude is in [0, 1)
    raw = rng.normal(size=1000)
    q_max, q_min = hp.bounds(raw)
    out = hp.normalise(raw, q_max, q_min, beta)
    assert (np.signbit(out) == np.signbit(raw)).all() and (np.abs(out) < 1.0).all()
    # q_max starts from 0 and both bounds are bounds of |.|
    assert q_max == np.abs(raw).max() and q_min == np.abs(raw).min()
    # a constant field: every gradient is rounding noise below the floor -> exactly 0 everywhere
    off = _meshes()[0]
    U = np.full((off.n_relevant, 4), 1.4)
    raw, _ = hp.raw_values(off, U, [(hp.SCHLIEREN, 0, 0)])
    q_max, q_min = hp.bounds(raw[0])
    assert q_max < 1e-12
    assert (hp.normalise(raw[0], q_max, q_min, beta) == 0.0).all()
    # ... and exactly equal raw values (q_max == q_min) too
    assert (hp.normalise(np.full(10, 2.0), 2.0, 2.0, beta) == 0.0).all()


def test_primitive_states():
    p = capi.Params()
    p.gamma = 1.4
    U = np.array([[2.0, 4.0, -6.0, 30.0]])
    V = hp.primitive_state(capi.EQ_EULER, 2, U, p)
    assert np.allclose(V, [[2.0, 2.0, -3.0, 0.4 * (30.0 - 0.5 * 52.0 / 2.0)]], rtol=1e-15)
    V = hp.primitive_state(capi.EQ_EULER_AEOS, 2, U, p)
    assert np.allclose(V, [[2.0, 2.0, -3.0, (30.0 - 0.5 * 52.0 / 2.0) / 2.0]], rtol=1e-15)
    p.reference_water_depth, p.dry_state_relaxation_small = 1.0, 1.0e2
    U = np.array([[0.5, 1.0, -2.0], [0.0, 1e-20, 0.0]])
    V = hp.primitive_state(capi.EQ_SHALLOW_WATER, 2, U, p)
    assert np.allclose(V[0], [0.5, 2.0, -4.0], rtol=1e-15)
    assert V[1, 0] == 0.0 and V[1, 1] == 1e-20 / (1.0e2 * hp.EPS)  # a dry node: the sharp cut-off, no division by 0
    assert (hp.primitive_state(capi.EQ_SCALAR_CONSERVATION, 2, np.array([[3.0]])) == 3.0).all()


def test_name_resolution():
    """conserved names first, primitive names second (Postprocessor::prepare()); unknown names are refused"""
    assert capi.resolve_component(capi.EQ_EULER, 2, "rho") == (0, 0)   # in both lists: the conserved one
    assert capi.resolve_component(capi.EQ_EULER, 2, "m_1") == (0, 1)
    assert capi.resolve_component(capi.EQ_EULER, 2, "E") == (0, 3)
    assert capi.resolve_component(capi.EQ_EULER, 2, "v_1") == (1, 1)
    assert capi.resolve_component(capi.EQ_EULER, 2, "p") == (1, 3)
    assert capi.resolve_component(capi.EQ_EULER, 3, "p") == (1, 4)
    assert capi.resolve_component(capi.EQ_EULER, 1, "m") == (0, 1)
    assert capi.resolve_component(capi.EQ_EULER, 1, "v") == (1, 1)
    assert capi.resolve_component(capi.EQ_EULER_AEOS, 2, "e") == (1, 3)
    assert capi.resolve_component(capi.EQ_SHALLOW_WATER, 2, "h") == (0, 0)
    assert capi.resolve_component(capi.EQ_SHALLOW_WATER, 2, "v_2") == (1, 2)
    assert capi.resolve_component(capi.EQ_SCALAR_CONSERVATION, 2, "u") == (0, 0)
    for equation, dim, name in ((capi.EQ_EULER, 2, "v_3"), (capi.EQ_EULER, 2, "e"), (capi.EQ_EULER, 1, "m_1"),
                                (capi.EQ_SHALLOW_WATER, 2, "rho"), (capi.EQ_SCALAR_CONSERVATION, 1, "")):
        with pytest.raises(ValueError):
            capi.resolve_component(equation, dim, name)
    quantities, names = hp.resolve(capi.EQ_EULER, 2, ("rho", "p", "E"), ("m_1", "v_1"))
    assert names == ["schlieren_rho", "schlieren_p", "schlieren_E", "vorticity_m_1", "vorticity_v_1"]
    assert quantities == [(0, 0, 0), (0, 1, 3), (0, 0, 3), (1, 0, 1), (1, 1, 1)]


def test_postprocess_declarations_compile_as_c(tmp_path):
    """the new entry points are plain C99 (the way tests/test_capi_cpu.py checks the ABI), and the ctypes mirror of
    the quantity descriptor has the C compiler's layout"""
    import ctypes as C
    src = tmp_path / "pp.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "ryujin_hip.h"\n'
        'int main(void) {\n'
        '  ryujin_hip_postprocess_quantity q = {RYUJIN_PP_VORTICITY, 1, 1};\n'
        '  int (*configure)(ryujin_hip_ctx *, int, const ryujin_hip_postprocess_quantity *, double, int) =\n'
        '      ryujin_hip_postprocess_configure;\n'
        '  int (*compute)(ryujin_hip_ctx *, int) = ryujin_hip_postprocess_compute;\n'
        '  int (*download)(ryujin_hip_ctx *, int, double *, int) = ryujin_hip_postprocess_download;\n'
        '  int (*bounds)(ryujin_hip_ctx *, int, double *, double *) = ryujin_hip_postprocess_bounds;\n'
        '  (void)configure; (void)compute; (void)download; (void)bounds;\n'
        '  printf("%zu %zu %zu %zu %d %d %d %d\\n", sizeof q, offsetof(ryujin_hip_postprocess_quantity, kind),\n'
        '         offsetof(ryujin_hip_postprocess_quantity, is_primitive),\n'
        '         offsetof(ryujin_hip_postprocess_quantity, component), RYUJIN_PP_SCHLIEREN, RYUJIN_PP_VORTICITY,\n'
        '         RYUJIN_PP_MAX_QUANTITIES, q.kind);\n'
        '  return 0;\n}\n')
    obj = tmp_path / "pp.o"
    # (compiled, not linked: the definitions live in the device library)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", _build.INCLUDE, "-c",
                    str(src), "-o", str(obj)], check=True, capture_output=True)
    Q = capi.PostprocessQuantity
    assert C.sizeof(Q) == 12 and [getattr(Q, f[0]).offset for f in Q._fields_] == [0, 4, 8]
    header = open(_build.INCLUDE + "/ryujin_hip.h").read()
    assert "#define RYUJIN_PP_MAX_QUANTITIES %d" % capi.PP_MAX_QUANTITIES in header
    assert "RYUJIN_PP_SCHLIEREN = %d, RYUJIN_PP_VORTICITY = %d" % (capi.PP_SCHLIEREN, capi.PP_VORTICITY) in header
    for name in ("configure", "compute", "download", "bounds"):
        assert "ryujin_hip_postprocess_" + name in capi.HIP_SYMBOLS
