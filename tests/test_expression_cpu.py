"""The expression-defined "function" state on the CPU: parser, program and host interpreter
(ryujin_amd/csrc/expression.hpp, ryujin_hip_expression_evaluate), the grammar table of include/ryujin_hip.h case by
case, every refusal with its status and position, and the plumbing of the new entry points. No GPU: the library is
loaded, no context is created."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers_expression as hx
from ryujin_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "expression_cases")


# --------------------------------------------------------------------------- the stand-alone program

@pytest.fixture(scope="module")
def checker():
    src = os.path.join(ROOT, "tests", "cpp", "expression_cases.cc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-I" + os.path.join(ROOT, "ryujin_amd", "csrc"), src, "-o", BIN], check=True)
    return BIN


@pytest.mark.parametrize("mode", ["grammar", "refusals", "limits"])
def test_header_alone_without_hip(checker, mode):
    """expression.hpp compiles with g++ alone (no HIP, no library) and passes its cases: the values of the grammar
    table against <cmath>, every refusal with the character position, the limits of program length, operand stack and
    nesting"""
    out = subprocess.run([checker, mode], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


# --------------------------------------------------------------------------- the grammar table

def value(expr, dim=1, point=None, t=0.0):
    point = np.zeros(dim) if point is None else np.asarray(point, dtype=np.float64)
    return float(capi.expression_evaluate(expr, dim, point.reshape(1, dim), t)[0])


GRAMMAR = [
    ("2+3*4", 14.0), ("2^3^2", 512.0), ("-2^2", -4.0), ("1 < 2 == 1", 1.0), ("0 || 2 && 0", 0.0),
    ("1 ? 2 : 3 ? 4 : 5", 2.0), ("0 ? 2 : 0 ? 4 : 5", 5.0), ("0 ? 2 : 1 ? 4 : 5", 4.0),
    ("if(0.4,1,2)", 2.0), ("if(0.5,1,2)", 1.0), ("if(-0.4,1,2)", 2.0), ("if(-0.5,1,2)", 1.0),
    ("0.4 ? 1 : 2", 1.0), ("0.4 && 1", 1.0), ("0.4 & 1", 0.0), ("0.4 || 0", 1.0), ("0.4 | 0", 0.0), ("0.5 | 0", 1.0),
    ("int(2.5)", 3.0), ("int(-2.5)", -3.0), ("int(2.4)", 2.0), ("min(3,1,2)", 1.0), ("max(1)", 1.0),
    ("max(3,1,2)", 3.0), ("min(2)", 2.0), ("_pi", np.pi), ("_e", np.e), ("1e-3", 1e-3), (".5", 0.5), ("1.5E+2", 150.0),
    ("2.", 2.0), ("  2 *\t( 3 + 4 )\n", 14.0), ("2*-3", -6.0), ("2^-1", 0.5), ("7 - 2 - 1", 4.0), ("8 / 4 / 2", 1.0),
    ("1 < 2 < 3", 1.0), ("3 > 2 > 1", 0.0), ("1 + 2 < 4 - 0.5", 1.0), ("1 | 0 & 0", 1.0), ("2 * 3 ^ 2", 18.0),
    ("-3 ^ 2 * 2", -18.0), ("sign(-3) + sign(0) + 2 * sign(7)", 1.0), ("rint(2.5)", 3.0), ("rint(-2.5)", -2.0),
    ("floor(-1.5)", -2.0), ("ceil(-1.5)", -1.0), ("abs(-1.5)", 1.5), ("log(_e)", 1.0), ("ln(_e)", 1.0),
    ("log2(8)", 3.0), ("log10(1000)", 3.0), ("sqrt(16)", 4.0), ("pow(2, 10)", 1024.0),
    ("if(1, 3, sqrt(-1))", 3.0), ("0 ? log(-1) : 7", 7.0),
]


@pytest.mark.parametrize("expr,expected", GRAMMAR, ids=[g[0].strip() for g in GRAMMAR])
def test_grammar_table(expr, expected):
    assert value(expr) == expected


def test_variables_by_dimension():
    p = [0.5, -2.0, 3.0]
    assert value("x", 1, p[:1], 7.0) == 0.5 and value("t", 1, p[:1], 7.0) == 7.0
    assert value("x + 10*y + 100*t", 2, p[:2], 7.0) == 0.5 - 20.0 + 700.0
    assert value("x + 10*y + 100*z + 1000*t", 3, p, 7.0) == 0.5 - 20.0 + 300.0 + 7000.0


def test_power_rewrite_bit_for_bit():
    """x^2, x^3, x^4 are multiplied out from the left; every other exponent, and pow, is the C library's pow"""
    X = np.random.default_rng(2).uniform(0.1, 3.0, size=(1000, 1))
    x = X[:, 0]
    ev = lambda e: capi.expression_evaluate(e, 1, X, 0.0)  # noqa: E731
    assert np.array_equal(ev("x^2"), x * x) and np.array_equal(ev("x^2"), ev("x*x"))
    assert np.array_equal(ev("x^3"), x * x * x) and np.array_equal(ev("x^4"), x * x * x * x)
    assert np.array_equal(ev("x^5"), ev("pow(x,5)")) and np.array_equal(ev("x^2.0"), ev("x*x"))
    assert np.array_equal(ev("pow(x,2)"), ev("x^(1+1)"))
    assert not np.array_equal(ev("x^5"), ev("x*x*x*x*x"))   # pow, not products: one rounding instead of four


# --------------------------------------------------------------------------- refusals

UNSUPPORTED, ARG = capi.RYUJIN_ERR_UNSUPPORTED, capi.RYUJIN_ERR_ARG
REFUSALS = [
    ("rand(1)", 1, UNSUPPORTED, 0), ("1 + rand_seed(1)", 1, UNSUPPORTED, 4), ("sum(1,2)", 1, UNSUPPORTED, 0),
    ("2*avg(1,2)", 1, UNSUPPORTED, 2), ('max("a", 1)', 1, UNSUPPORTED, 4), ("x = 3", 1, UNSUPPORTED, 2),
    ("x += 3", 1, UNSUPPORTED, 3), ("pi", 1, ARG, 0), ("2 * foo", 1, ARG, 4), ("foo(1)", 1, ARG, 0),
    ("x + y", 1, ARG, 4), ("x + z", 2, ARG, 4), ("(1 + 2", 1, ARG, 0), ("1 + 2)", 1, ARG, 5), ("sin(1, 2)", 1, ARG, 0),
    ("pow(1)", 1, ARG, 0), ("pow(1,2,3)", 1, ARG, 0), ("if(1, 2)", 1, ARG, 0), ("min()", 1, ARG, 0), ("", 1, ARG, 0),
    ("   ", 1, ARG, 3), ("1 2", 1, ARG, 2), ("1 +", 1, ARG, 3), ("1 ? 2", 1, ARG, 5), ("1e", 1, ARG, 1),
    ("2 $ 3", 1, ARG, 2), ("sin", 1, ARG, 0), ("sin x", 1, ARG, 0), ("x", 0, ARG, 0), ("x", 4, ARG, 0),
]


@pytest.mark.parametrize("expr,dim,status,position", REFUSALS, ids=[repr(r[0]) + f"-{r[1]}d" for r in REFUSALS])
def test_refusals_name_status_and_position(expr, dim, status, position):
    lib = capi.load_hip()
    point, out = np.zeros(3), np.full(1, 7.0)
    rc = lib.ryujin_hip_expression_evaluate(expr.encode(), dim, capi.as_ptr(point, capi.c_double_p), 1, 0.0,
                                            capi.as_ptr(out, capi.c_double_p))
    message = lib.ryujin_hip_last_error().decode()
    assert rc == status, (rc, message)
    assert re.search(rf"at character {position}\b", message), message
    assert out[0] == 7.0


def right_nested_sum(operands):
    return "1+(" * (operands - 1) + "1" + ")" * (operands - 1)


def test_limits_of_stack_and_program():
    assert value(right_nested_sum(capi.EXPR_MAX_STACK)) == capi.EXPR_MAX_STACK
    with pytest.raises(RuntimeError, match="operands alive") as refused:
        value(right_nested_sum(capi.EXPR_MAX_STACK + 1))
    assert refused.value.status == ARG and "at character" in str(refused.value)
    ones = capi.EXPR_MAX_INSTRUCTIONS // 2         # -1+1+...+1: `ones` constants, ones - 1 additions, one sign
    longest = "-1" + "+1" * (ones - 1)
    assert value(longest) == ones - 2
    with pytest.raises(RuntimeError, match="instructions") as refused:
        value("-" + longest)
    assert refused.value.status == ARG and "at character" in str(refused.value)
    header = open(os.path.join(ROOT, "include", "ryujin_hip.h")).read()
    assert f"#define RYUJIN_EXPR_MAX_INSTRUCTIONS {capi.EXPR_MAX_INSTRUCTIONS}\n" in header
    assert f"#define RYUJIN_EXPR_MAX_STACK {capi.EXPR_MAX_STACK}\n" in header


def test_empty_and_null_arguments():
    lib = capi.load_hip()
    f = lib.ryujin_hip_expression_evaluate
    guard = np.full(2, 7.0)
    point = np.zeros(1)
    out_p, point_p = capi.as_ptr(guard, capi.c_double_p), capi.as_ptr(point, capi.c_double_p)
    assert f(b"x", 1, None, 0, 0.0, out_p) == capi.RYUJIN_OK and (guard == 7.0).all()
    assert f(b"x", 1, None, 0, 0.0, None) == capi.RYUJIN_OK
    assert f(None, 1, point_p, 1, 0.0, out_p) == ARG
    assert f(b"x", 1, None, 1, 0.0, out_p) == ARG
    assert f(b"x", 1, point_p, 1, 0.0, None) == ARG
    assert (guard == 7.0).all()
    assert capi.expression_evaluate("x", 2, np.zeros((0, 2)), 0.0).shape == (0,)
    # no context: nothing to configure
    assert lib.ryujin_hip_initial_values_configure_function(None, 1, None, None, None, None, None) == ARG


# --------------------------------------------------------------------------- string against numpy

@pytest.mark.parametrize("expr,dim,fn", hx.ARITHMETIC, ids=[a[0] for a in hx.ARITHMETIC])
def test_arithmetic_bit_for_bit_against_numpy(expr, dim, fn):
    """1000 points per expression, among them the points where a comparison is decided by equality"""
    X = hx.arithmetic_points(dim)
    for t in (0.0, 0.375):
        got, want = capi.expression_evaluate(expr, dim, X, t), hx.evaluate_numpy(fn, X, t)
        assert np.array_equal(got, want), (expr, t, X[got != want][:3], got[got != want][:3], want[got != want][:3])


def test_kpp_state_on_the_unit_circle():
    X = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0], [0.6, 0.8], [0.0, 0.0], [0.999, 0.0]])
    got = capi.expression_evaluate(hx.KPP, 2, X, 0.0)
    inside = 0.78539816339 * 14.0
    assert got.tolist() == [0.78539816339] * 5 + [inside] * 2   # 0.36 + 0.64 rounds to 1: not < 1


@pytest.mark.parametrize("name,expr,lower,upper,fn,b_f", hx.FUNCTIONS, ids=[f[0] for f in hx.FUNCTIONS])
def test_library_functions_against_numpy(name, expr, lower, upper, fn, b_f):
    X = hx.function_points(lower, upper)
    got, want = capi.expression_evaluate(expr, 1, X, 0.0), fn(X[:, 0])
    excess = np.abs(got - want) - hx.function_bound(want, b_f)
    assert (excess <= 0.0).all(), (name, float(excess.max()))


@pytest.mark.parametrize("expr,fn,exponent", hx.POW, ids=[p[0] for p in hx.POW])
def test_pow_against_numpy(expr, fn, exponent):
    X = hx.pow_points()
    x = X[:, 0]
    got, want = capi.expression_evaluate(expr, 1, X, 0.0), fn(x)
    assert (np.abs(got - want) <= hx.pow_bound(x, exponent(x), want)).all()


@pytest.mark.parametrize("expr,dim,fn", hx.COMPOSITES, ids=[c[0] for c in hx.COMPOSITES])
def test_composites_within_the_error_arithmetic(expr, dim, fn):
    X = hx.arithmetic_points(dim)
    for t in (0.0, 0.375):
        want, bound = hx.evaluate_err(fn, X, t)
        got = capi.expression_evaluate(expr, dim, X, t)
        assert (np.abs(got - want) <= bound).all(), (expr, t, float((np.abs(got - want) - bound).max()))


# --------------------------------------------------------------------------- plumbing and ABI

def test_symbols_are_exported_listed_and_typed():
    lib = capi.load_hip()
    for name in ("ryujin_hip_initial_values_configure_function", "ryujin_hip_expression_evaluate"):
        assert name in capi.HIP_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert len(lib.ryujin_hip_initial_values_configure_function.argtypes) == 7
    assert len(lib.ryujin_hip_expression_evaluate.argtypes) == 6
    header = open(os.path.join(ROOT, "include", "ryujin_hip.h")).read()
    for name in ("ryujin_hip_initial_values_configure_function", "ryujin_hip_expression_evaluate"):
        assert re.search(rf"\bint {name}\(", header)


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "ryujin_hip.h"\n'
                   "int main(void) {\n"
                   "  const char *const e[1] = {\"0.25 * x\"};\n"
                   "  const double d[3] = {1., 0., 0.}, p[3] = {0., 0., 0.};\n"
                   "  double out[1];\n"
                   "  int (*f)(ryujin_hip_ctx *, int, const char *const *, const double[3], const double[3],\n"
                   "           const double *, const double *) = ryujin_hip_initial_values_configure_function;\n"
                   "  int (*g)(const char *, int, const double *, size_t, double, double *) = "
                   "ryujin_hip_expression_evaluate;\n"
                   "  (void)e; (void)d; (void)p; (void)out; (void)f; (void)g;\n"
                   "  return RYUJIN_EXPR_MAX_INSTRUCTIONS > RYUJIN_EXPR_MAX_STACK ? 0 : 1;\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-c",
                    "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "use.o")], check=True)


def test_expression_names_defaults_and_the_dict_form():
    f = capi.function_expressions
    assert f(capi.EQ_EULER, 1, {}) == ("1.4", "3.0", "1.0")
    assert f(capi.EQ_EULER, 3, {}) == ("1.4", "3.0", "0.0", "0.0", "1.0")
    assert f(capi.EQ_EULER_AEOS, 2, {"pressure expression": "2.5", "velocity_y_expression": "x*t"}) == \
        ("1.4", "3.0", "x*t", "2.5")
    assert f(capi.EQ_SHALLOW_WATER, 2, {"water depth expression": "1 + x"}) == ("1 + x", "3.0", "0.0")
    assert f(capi.EQ_SHALLOW_WATER, 1, {}) == ("1.4", "3.0")
    assert f(capi.EQ_SCALAR_CONSERVATION, 2, {}) == ("0.25 * x",)
    assert f(capi.EQ_SCALAR_CONSERVATION, 1, {"expression": "sin(x-t)"}) == ("sin(x-t)",)
    assert f(capi.EQ_SCALAR_CONSERVATION, 1, "sin(x-t)") == ("sin(x-t)",)
    assert f(capi.EQ_EULER, 1, ["1", "x", 2.5]) == ("1", "x", "2.5")
    assert [n for n, _ in capi.function_expression_names(capi.EQ_EULER, 3)] == \
        ["density expression", "velocity x expression", "velocity y expression", "velocity z expression",
         "pressure expression"]
    with pytest.raises(ValueError):
        f(capi.EQ_EULER, 2, ["1", "x", "2.5"])               # 2-D takes four
    with pytest.raises(ValueError):
        f(capi.EQ_EULER, 1, {"velocity y expression": "0"})  # no such parameter in 1-D
    with pytest.raises(ValueError):
        f(capi.EQ_SHALLOW_WATER, 1, {"density expression": "1"})


def test_module_method_forwards_primitive_order(monkeypatch):
    """HyperbolicModule.initial_values_configure_function hands the library the expressions in primitive order, the
    direction and position padded to three components, and the offline data's positions (no context: a recorder in
    place of the library function)"""
    from ryujin_amd.module import HyperbolicModule
    calls = []

    class Offline:
        positions = np.arange(8.0).reshape(4, 2)
        b_positions = np.arange(4.0).reshape(2, 2)
        n_bdry = 2

    class Params:
        equation = capi.EQ_SHALLOW_WATER

    m = object.__new__(HyperbolicModule)
    m.params, m.dim, m.offline, m.n_relevant, m._ctx = Params(), 2, Offline(), 4, None

    def record(ctx, n, texts, direction, position, pos, bpos):
        calls.append(([texts[q].decode() for q in range(n)], [direction[q] for q in range(3)],
                      [position[q] for q in range(3)], [pos[q] for q in range(8)], [bpos[q] for q in range(4)]))
        return capi.RYUJIN_OK

    monkeypatch.setattr(m, "_f", lambda name: record if name == "initial_values_configure_function" else None,
                        raising=False)
    monkeypatch.setattr(m, "close", lambda: None, raising=False)
    m.initial_values_configure_function({"velocity y expression": "x - t"}, direction=(1.0, 1.0), position=(0.5, -1.0))
    assert calls == [(["1.4", "3.0", "x - t"], [1.0, 1.0, 0.0], [0.5, -1.0, 0.0], list(np.arange(8.0)),
                      list(np.arange(4.0)))]
    with pytest.raises(ValueError):
        m.initial_values_configure_function({}, direction=(1.0,))
