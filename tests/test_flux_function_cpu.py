"""The function flux of the scalar conservation equation on the CPU: the parser with the variable u and the component
split (flux_compile), the host interpreter behind ryujin_hip_flux_function_evaluate against numpy, and the condition on
the data of tests/test_gpu_flux_function.py, evaluated on the oracle alone. No GPU: the library is loaded for its host
entry points only."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import helpers_expression as hx
import helpers_flux_function as hf
from ryujin_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "flux_function_cases")


# --------------------------------------------------------------------------- the stand-alone program

@pytest.fixture(scope="module")
def checker():
    src = os.path.join(ROOT, "tests", "cpp", "flux_function_cases.cc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-I" + os.path.join(ROOT, "ryujin_amd", "csrc"), src, "-o", BIN], check=True)
    return BIN


@pytest.mark.parametrize("mode", ["grammar", "components", "limits", "values"])
def test_header_alone_without_hip(checker, mode):
    """flux_compile and flux_evaluate_points compile with g++ alone (no HIP, no library) and pass their cases"""
    out = subprocess.run([checker, mode], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


# --------------------------------------------------------------------------- through the library

def evaluate(expr, dim=1, u=(0.25,), delta=hf.DELTA, gradient=True):
    return capi.flux_function_evaluate(expr, dim, np.asarray(u, dtype=np.float64), delta, gradient)


def refusal(expr, dim, delta=hf.DELTA):
    lib = capi.load_hip()
    u, value = np.full(1, 0.25), np.full(3, 7.0)
    rc = lib.ryujin_hip_flux_function_evaluate(expr.encode(), dim, delta, capi.as_ptr(u, capi.c_double_p), 1,
                                               capi.as_ptr(value, capi.c_double_p), None)
    assert (value == 7.0).all(), "a refused call wrote something"
    return rc, lib.ryujin_hip_last_error().decode()


def test_symbols_are_exported_listed_and_typed():
    lib = capi.load_hip()
    for name in ("ryujin_hip_flux_configure_function", "ryujin_hip_flux_function_evaluate", "ryujin_hip_flux_info"):
        assert name in capi.HIP_SYMBOLS and getattr(lib, name).argtypes is not None
    assert capi.FLUX_FUNCTION == 3


def test_the_variable_is_u():
    value, gradient = evaluate("u", 1, [0.25, -1.5])
    assert (value[:, 0] == [0.25, -1.5]).all()
    assert gradient.shape == (2, 1)
    value, _ = evaluate("u; 2*u; u - 1", 3, [0.5])
    assert (value[0] == [0.5, 1.0, -0.5]).all()


@pytest.mark.parametrize("expr, dim, status, position", [
    ("x", 1, capi.RYUJIN_ERR_ARG, 0),
    ("u + t", 1, capi.RYUJIN_ERR_ARG, 4),
    ("u; u*y", 2, capi.RYUJIN_ERR_ARG, 5),
    ("pi*u", 1, capi.RYUJIN_ERR_ARG, 0),
    ("u; rand()", 2, capi.RYUJIN_ERR_UNSUPPORTED, 3),
    ("u = 3", 1, capi.RYUJIN_ERR_UNSUPPORTED, 2),
    ("u; u = 3", 2, capi.RYUJIN_ERR_UNSUPPORTED, 5),
    ("(u + 1", 1, capi.RYUJIN_ERR_ARG, 0),
    ("u; (u + 1", 2, capi.RYUJIN_ERR_ARG, 3),
    ("u + 1)", 1, capi.RYUJIN_ERR_ARG, 5),
    ("u; u 2", 2, capi.RYUJIN_ERR_ARG, 5),
    ("u 2; u", 2, capi.RYUJIN_ERR_ARG, 2),
])
def test_refusals_name_status_and_position(expr, dim, status, position):
    rc, message = refusal(expr, dim)
    assert rc == status, (rc, message)
    assert f"at character {position} " in message, message


@pytest.mark.parametrize("expr, accepted_in", [
    ("u", (1,)), ("u; u", (2,)), ("u; u; u", (3,)), ("u; u; u; u", ()),
    ("", ()), (";", ()), ("u;", ()), ("u; u;", ()), (";;", ()), ("u;;u", ()), (";u", ()),
])
def test_component_count_against_the_dimension(expr, accepted_in):
    for dim in (1, 2, 3):
        if dim in accepted_in:
            assert evaluate(expr, dim)[0].shape == (1, dim)
        else:
            rc, message = refusal(expr, dim)
            assert rc == capi.RYUJIN_ERR_ARG and "at character " in message, (dim, rc, message)


def test_an_empty_component_is_located_in_the_whole_string():
    assert "at character 3 " in refusal("u; ", 2)[1]
    assert "at character 2 " in refusal("u;;u", 3)[1]
    assert "at character 0 " in refusal(";;", 3)[1]


def left_sum(terms):
    """2 * terms instructions: the sign, `terms` operands, terms - 1 additions"""
    return "-u" + "+1" * (terms - 1)


def right_nested_sum(operands):
    return "1+(" * (operands - 1) + "1" + ")" * (operands - 1)


def test_limits_hold_per_component():
    longest = left_sum(capi.EXPR_MAX_INSTRUCTIONS // 2)
    full = capi.EXPR_MAX_INSTRUCTIONS // 2 - 1
    assert evaluate(longest)[0][0, 0] == -0.25 + full
    assert (evaluate("; ".join([longest] * 3), 3)[0][0] == -0.25 + full).all()
    for expr, dim in (("-" + longest, 1), ("u; -" + longest, 2), ("u; u; -" + longest, 3)):
        rc, message = refusal(expr, dim)
        assert rc == capi.RYUJIN_ERR_ARG and "instructions" in message, message
    deepest = right_nested_sum(capi.EXPR_MAX_STACK)
    assert (evaluate("u; " + deepest, 2)[0][0] == [0.25, capi.EXPR_MAX_STACK]).all()
    for expr, dim in ((right_nested_sum(capi.EXPR_MAX_STACK + 1), 1),
                      ("u; " + right_nested_sum(capi.EXPR_MAX_STACK + 1), 2)):
        rc, message = refusal(expr, dim)
        assert rc == capi.RYUJIN_ERR_ARG and "operands alive" in message, message


def test_delta_must_be_positive_and_finite():
    for delta in (0.0, -1e-10, float("inf"), float("nan")):
        rc, message = refusal("u", 1, delta)
        assert rc == capi.RYUJIN_ERR_ARG and "delta" in message, (delta, rc, message)


U_POINTS = np.concatenate([np.random.default_rng(7).uniform(-2.0, 2.0, size=997), [0.0, 0.5, 1.0]])


@pytest.mark.parametrize("coefficients", [hf.CUBIC, hf.BURGERS, hf.TRANSPORT], ids=["cubic", "burgers", "transport"])
def test_horner_polynomials_bit_for_bit(coefficients):
    """value and gradient at 1000 points: the operations of ScalarConservation::polynomial and of its difference
    quotient, in their order"""
    expr, fns = hf.polynomial_flux(coefficients, 3)
    value, gradient = evaluate(expr, 3, U_POINTS)
    for d, fn in enumerate(fns):
        assert (value[:, d] == fn(U_POINTS)).all()
        assert (gradient[:, d] == hf.numpy_gradient(fn, U_POINTS, hf.DELTA)).all()


@pytest.mark.parametrize("name", sorted(hf.ARITHMETIC_SETS))
def test_arithmetic_sets_bit_for_bit(name):
    """Buckley-Leverett, if / min / max, the multiplied-out cube: exactly rounded operations only"""
    expr, fns = hf.ARITHMETIC_SETS[name]
    value, gradient = evaluate(expr, len(fns), U_POINTS)
    for d, fn in enumerate(fns):
        assert (value[:, d] == fn(U_POINTS)).all()
        assert (gradient[:, d] == hf.numpy_gradient(fn, U_POINTS, hf.DELTA)).all()


def test_another_operation_order_may_differ_and_does_not_crash():
    a, _ = evaluate("0.5*u*u", 1, U_POINTS)
    b, _ = evaluate("u*0.5*u", 1, U_POINTS)
    assert (np.abs(a - b) <= hx.EPS * np.abs(a)).all()
    a, _ = evaluate("u*u*u/3", 1, U_POINTS)
    b, _ = evaluate("u*(u*(u/3))", 1, U_POINTS)
    assert (np.abs(a - b) <= 4.0 * hx.EPS * np.abs(a)).all()


@pytest.mark.parametrize("name", sorted(hf.LIBRARY_SETS))
def test_library_sets_within_the_function_caps(name):
    """host interpreter against numpy: the two C libraries' errors alone, B_f eps |f| per function; the gradient within
    (B_f eps |f| 2) / (2 delta), the bound of the device test"""
    expr, parts = hf.LIBRARY_SETS[name]
    value, gradient = evaluate(expr, len(parts), U_POINTS, hf.DELTA_LIBRARY)
    for d, (fn, b_f) in enumerate(parts):
        want = fn(U_POINTS)
        assert (np.abs(value[:, d] - want) <= hx.function_bound(want, b_f)).all()
        plus, minus = fn(U_POINTS + hf.DELTA_LIBRARY), fn(U_POINTS - hf.DELTA_LIBRARY)
        quotient = (plus - minus) / (2 * hf.DELTA_LIBRARY)
        bound = hf.library_gradient_bound(plus, minus, b_f, hf.DELTA_LIBRARY)
        assert (np.abs(gradient[:, d] - quotient) <= bound).all()


def test_gradient_at_a_kink():
    """if(u < 0.5, u, 1 - u) at u = 0.5: f(0.5 + d) = 0.5 - d and f(0.5 - d) = 0.5 - d, so the quotient vanishes; half
    a step to either side it is the one-sided slope to round-off"""
    delta = 2.0 ** -20   # exactly representable: 0.5 +- delta are exact
    _, gradient = evaluate("if(u < 0.5, u, 1 - u)", 1, [0.5, 0.5 - 4 * delta, 0.5 + 4 * delta], delta)
    assert gradient[0, 0] == 0.0 and gradient[1, 0] == 1.0 and gradient[2, 0] == -1.0


def test_empty_and_null_arguments():
    lib = capi.load_hip()
    f = lib.ryujin_hip_flux_function_evaluate
    guard = np.full(2, 7.0)
    assert f(b"u", 1, 1e-10, None, 0, None, None) == capi.RYUJIN_OK
    assert f(b"u", 1, 1e-10, capi.as_ptr(guard, capi.c_double_p), 0, capi.as_ptr(guard, capi.c_double_p),
             capi.as_ptr(guard, capi.c_double_p)) == capi.RYUJIN_OK
    assert (guard == 7.0).all()
    assert f(None, 1, 1e-10, None, 0, None, None) == capi.RYUJIN_ERR_ARG
    assert f(b"u", 1, 1e-10, None, 1, capi.as_ptr(guard, capi.c_double_p), None) == capi.RYUJIN_ERR_ARG
    assert f(b"u", 1, 1e-10, capi.as_ptr(guard, capi.c_double_p), 1, None, None) == capi.RYUJIN_ERR_ARG
    value, gradient = capi.flux_function_evaluate("u*u", 1, [3.0], gradient=False)
    assert value[0, 0] == 9.0 and gradient is None


def test_the_existing_entry_point_keeps_its_variables():
    """ryujin_hip_expression_evaluate: x y z t as before, u unknown"""
    assert capi.expression_evaluate("x + t", 1, [[0.5]], 2.0)[0] == 2.5
    with pytest.raises(RuntimeError) as refused:
        capi.expression_evaluate("u", 1, [[0.5]], 0.0)
    assert refused.value.status == capi.RYUJIN_ERR_ARG


# --------------------------------------------------------------------------- the data of the GPU comparisons

# (mesh, coefficients, greedy wavespeed): the averaged-entropy cases of the GPU comparison in which f(k) can show at all
CONDITIONED = [("plane", hf.BURGERS, True), ("plane", hf.CUBIC, False), ("plane", hf.CUBIC, True),
               ("box", hf.CUBIC, False)]


@pytest.mark.parametrize("mesh, coefficients, greedy", CONDITIONED,
                         ids=["burgers-greedy", "cubic", "cubic-greedy", "cubic-3d"])
def test_developed_data_lets_the_averaged_entropy_decide(oracle, mesh, coefficients, greedy):
    """The condition on the data of test_one_update_against_the_oracle, on the oracle alone: with averaged entropy
    lambda_left / lambda_right decide d_ij in interior pairs and in boundary pairs whose stored value is d_ji. The numpy
    restatement of the Riemann solver is held against the oracle's d_ij first. (A convex flux -- Burgers -- meets it with
    the greedy wavespeed only, the linear flux never: helpers_flux_function.CUBIC.)"""
    off = hf.mesh(mesh)
    p = hf.polynomial_params(oracle, off.dim, coefficients, averaged=True, greedy=greedy)
    U, dirichlet = hf.develop(off, p, oracle)
    expr, _ = hf.polynomial_flux(coefficients, off.dim)
    counts = hf.averaged_entropy_coverage(off, hf.oracle_arrays(off, p, oracle, U, dirichlet), expr, hf.DELTA, greedy)
    assert len(counts) == 2 and all(v > 0 for v in counts.values()), counts
