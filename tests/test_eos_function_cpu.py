"""The function equation of state of EulerAEOS on the CPU: the parser with the variable sets (rho, e) and (rho, p) and
the four programs (eos_compile), the host interpreter behind ryujin_hip_eos_function_evaluate against the oracle's
closed-form members and against numpy. No GPU: the library is loaded for its host entry points only."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import helpers_eos_function as he
from helpers_initial_values import EPS
from ryujin_amd import capi, initial_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "eos_function_cases")
SRC = os.path.join(ROOT, "tests", "cpp", "eos_function_cases.cc")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
         "-I" + os.path.join(ROOT, "ryujin_amd", "csrc")]


# --------------------------------------------------------------------------- the stand-alone program

@pytest.fixture(scope="module")
def checker():
    subprocess.run(["g++", "-O2", *FLAGS, SRC, "-o", BIN], check=True)
    return BIN


@pytest.mark.parametrize("mode", ["grammar", "limits", "defaults", "values"])
def test_header_alone_without_hip(checker, mode):
    """eos_compile and eos_evaluate_points compile with g++ alone (no HIP, no library) and pass their cases"""
    out = subprocess.run([checker, mode], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_header_alone_under_the_sanitizers():
    """the same program with its own main, once under -fsanitize=address,undefined as a plain host program"""
    binary = BIN + "_sanitized"
    subprocess.run(["g++", "-O1", "-g", *FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    SRC, "-o", binary], check=True)
    out = subprocess.run([binary, "all"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


# --------------------------------------------------------------------------- through the library

def refusal(which, expr):
    lib = capi.load_hip()
    rho, second, out = np.full(1, 1.5), np.full(1, 2.5), np.full(1, 7.0)
    rc = lib.ryujin_hip_eos_function_evaluate(which, expr.encode(), capi.as_ptr(rho, capi.c_double_p),
                                              capi.as_ptr(second, capi.c_double_p), 1,
                                              capi.as_ptr(out, capi.c_double_p))
    assert out[0] == 7.0, "a refused call wrote something"
    return rc, lib.ryujin_hip_last_error().decode()


NAMES = ("pressure", "specific internal energy", "temperature", "speed of sound")


def test_symbols_are_exported_listed_and_typed():
    lib = capi.load_hip()
    for name in ("ryujin_hip_eos_configure_function", "ryujin_hip_eos_function_evaluate",
                 "ryujin_hip_eos_function_evaluate_device", "ryujin_hip_eos_info"):
        assert name in capi.HIP_SYMBOLS and getattr(lib, name).argtypes is not None
    assert capi.EOS_FUNCTION == 4
    assert (capi.EOS_PRESSURE, capi.EOS_SPECIFIC_INTERNAL_ENERGY, capi.EOS_TEMPERATURE,
            capi.EOS_SPEED_OF_SOUND) == (0, 1, 2, 3)


def test_each_second_variable_in_its_own_programs_only():
    for which in (0, 2, 3):
        assert capi.eos_function_evaluate(which, "rho + 2*e", [1.5], [2.5])[0] == 6.5
        rc, message = refusal(which, "rho*p")
        assert rc == capi.RYUJIN_ERR_ARG and "at character 4 " in message and NAMES[which] in message, message
    assert capi.eos_function_evaluate(1, "rho + 2*p", [1.5], [2.5])[0] == 6.5
    rc, message = refusal(1, "rho*e")
    assert rc == capi.RYUJIN_ERR_ARG and "at character 4 " in message and NAMES[1] in message, message


@pytest.mark.parametrize("which", [0, 1, 2, 3])
@pytest.mark.parametrize("expr, status, position", [
    ("x", capi.RYUJIN_ERR_ARG, 0),
    ("rho + t", capi.RYUJIN_ERR_ARG, 6),
    ("rho*u", capi.RYUJIN_ERR_ARG, 4),
    ("rho*y", capi.RYUJIN_ERR_ARG, 4),
    ("pi*rho", capi.RYUJIN_ERR_ARG, 0),
    ("rho*rand()", capi.RYUJIN_ERR_UNSUPPORTED, 4),
    ("rho = 3", capi.RYUJIN_ERR_UNSUPPORTED, 4),
    ("(rho + 1", capi.RYUJIN_ERR_ARG, 0),
    ("rho + 1)", capi.RYUJIN_ERR_ARG, 7),
    ("", capi.RYUJIN_ERR_ARG, 0),
])
def test_refusals_name_status_parameter_and_position(which, expr, status, position):
    rc, message = refusal(which, expr)
    assert rc == status, (rc, message)
    assert f"at character {position} " in message and f"eos: {NAMES[which]}: " in message, message


def test_e_is_the_variable_and_underscore_e_the_constant():
    rho, e = np.array([1.75]), np.array([2.5])
    assert capi.eos_function_evaluate(0, "1e-3*e", rho, e)[0] == 1e-3 * 2.5
    assert capi.eos_function_evaluate(0, "2*e", rho, e)[0] == 5.0
    assert capi.eos_function_evaluate(0, "rho*e", rho, e)[0] == 1.75 * 2.5
    assert capi.eos_function_evaluate(0, "1.5e1*e", rho, e)[0] == 37.5
    assert capi.eos_function_evaluate(0, "_e", rho, e)[0] == np.e
    assert capi.eos_function_evaluate(0, "_e*e", rho, e)[0] == np.e * 2.5
    assert capi.eos_function_evaluate(1, "_e*p", rho, e)[0] == np.e * 2.5
    rc, message = refusal(1, "p*e")
    assert rc == capi.RYUJIN_ERR_ARG and "at character 2 " in message


def left_sum(terms):
    return "-rho" + "+1" * (terms - 1)


def right_nested_sum(operands):
    return "1+(" * (operands - 1) + "1" + ")" * (operands - 1)


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_limits_hold_per_expression(which):
    longest = left_sum(capi.EXPR_MAX_INSTRUCTIONS // 2)
    assert capi.eos_function_evaluate(which, longest, [0.25], [1.0])[0] == -0.25 + capi.EXPR_MAX_INSTRUCTIONS // 2 - 1
    rc, message = refusal(which, "-" + longest)
    assert rc == capi.RYUJIN_ERR_ARG and "instructions" in message and NAMES[which] in message, message
    assert capi.eos_function_evaluate(which, right_nested_sum(capi.EXPR_MAX_STACK), [1.0], [1.0])[0] \
        == capi.EXPR_MAX_STACK
    rc, message = refusal(which, right_nested_sum(capi.EXPR_MAX_STACK + 1))
    assert rc == capi.RYUJIN_ERR_ARG and "operands alive" in message and NAMES[which] in message, message


def test_null_gives_the_defaults():
    rho, e = he.admissible_points("polytropic", 100)
    assert (capi.eos_function_evaluate(0, None, rho, e) == (1.4 - 1.0) * rho * e).all()
    assert (capi.eos_function_evaluate(1, None, rho, e) == e / (rho * (1.4 - 1.0))).all()
    assert (capi.eos_function_evaluate(2, None, rho, e) == e / 718.).all()
    assert (capi.eos_function_evaluate(3, None, rho, e) == np.sqrt(1.4 * (1.4 - 1.0) * e)).all()


def test_empty_and_bad_arguments():
    lib = capi.load_hip()
    f = lib.ryujin_hip_eos_function_evaluate
    guard = np.full(1, 7.0)
    ptr = capi.as_ptr(guard, capi.c_double_p)
    assert f(0, b"rho", None, None, 0, None) == capi.RYUJIN_OK
    assert f(0, b"rho", ptr, ptr, 0, ptr) == capi.RYUJIN_OK and guard[0] == 7.0
    assert f(0, b"rho", None, ptr, 1, ptr) == capi.RYUJIN_ERR_ARG
    assert f(4, b"rho", ptr, ptr, 1, ptr) == capi.RYUJIN_ERR_ARG
    assert f(-1, b"rho", ptr, ptr, 1, ptr) == capi.RYUJIN_ERR_ARG
    assert guard[0] == 7.0


@pytest.mark.parametrize("name", ["polytropic", "nasg", "vdw"])
def test_closed_form_members_as_expressions_bit_for_bit(oracle, name):
    """all four functions at 1000 random admissible (rho, e) against the oracle: the same IEEE operations in the same
    order, -ffp-contract=off on both sides. The specific internal energy at the oracle's own p(rho, e)."""
    p = he.member_params(oracle.default_params(capi.EQ_EULER_AEOS, 1), name)
    expressions = he.member_expressions(p)
    rho, e = he.admissible_points(name)
    want = he.oracle_functions(oracle, p, rho, e)
    assert np.isfinite(want).all()
    for which in range(4):
        second = want[0] if which == 1 else e
        got = capi.eos_function_evaluate(which, he.expression_of(expressions, which), rho, second)
        assert (got == want[which]).all(), (name, he.FUNCTIONS[which], np.abs(got - want[which]).max())


def test_jones_wilkins_lee_as_expressions_within_one_exp_per_term(oracle):
    """helpers_eos_function.jwl_bound: the bound that follows from one exp per term. (Measured: the difference is 0 in
    all four functions -- interpreter and oracle call the same libm exp on the same operand.)"""
    p = he.member_params(oracle.default_params(capi.EQ_EULER_AEOS, 1), "jwl")
    expressions = he.member_expressions(p)
    rho, e = he.admissible_points("jwl")
    want = he.oracle_functions(oracle, p, rho, e)
    assert np.isfinite(want).all()
    for which in range(4):
        second = want[0] if which == 1 else e
        got = capi.eos_function_evaluate(which, he.expression_of(expressions, which), rho, second)
        bound = he.jwl_bound(p, which, rho, second)
        print(he.FUNCTIONS[which], "max |difference| / bound", (np.abs(got - want[which]) / bound).max())
        assert (np.abs(got - want[which]) <= bound).all(), he.FUNCTIONS[which]


@pytest.mark.parametrize("with_if", [False, True])
def test_an_equation_of_state_with_an_if_bit_for_bit_against_numpy(with_if):
    expressions = he.LINEARISED_IF if with_if else he.LINEARISED
    rho, e = he.admissible_points("polytropic")
    rho[:3] = 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)   # the kink and its neighbours
    pressure = capi.eos_function_evaluate(0, expressions["pressure"], rho, e)
    assert (pressure == he.linearised_pressure(rho, e, with_if)).all()
    sie = capi.eos_function_evaluate(1, expressions["specific_internal_energy"], rho, pressure)
    assert (sie == he.linearised_sie(rho, pressure, with_if)).all()
    # the round trip of THESE expressions (neither the reference nor the library checks consistency): e -> p -> e
    # through a subtraction of c^2 (rho - 1) <= 0.5 from p and well-conditioned products: a few roundings of
    # (|p| + 0.5) / (0.4 rho)
    assert (np.abs(sie - e) <= 16 * EPS * (np.abs(pressure) + 0.5) / (0.4 * rho)).all()


def test_numpy_restatement_takes_the_host_interpreter_for_a_function_parameter_set():
    lib = capi.load_hip()
    p = capi.Params()
    lib.ryujin_hip_default_params(p, capi.EQ_EULER_AEOS, 2)
    p.eos = capi.EOS_FUNCTION
    rho, pressure = np.array([[1.0, 2.0], [0.5, 3.0]]), np.array([[1.0, 0.25], [4.0, 2.0]])
    default = initial_states.aeos_specific_internal_energy(p, rho, pressure)
    assert default.shape == (2, 2) and (default == pressure / (rho * (1.4 - 1.0))).all()
    p.eos_function_sie = he.LINEARISED["specific_internal_energy"]
    assert (initial_states.aeos_specific_internal_energy(p, rho, pressure)
            == he.linearised_sie(rho, pressure)).all()
    U = initial_states.aeos_from_primitive(p, rho[0], np.zeros((2, 2)), pressure[0])
    assert (U[:, -1] == rho[0] * he.linearised_sie(rho[0], pressure[0])).all()
