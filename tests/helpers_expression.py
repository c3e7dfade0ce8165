"""Yardsticks of tests/test_expression_cpu.py and tests/test_gpu_initial_values_function.py: every expression of the
function state (ryujin_amd/csrc/expression.hpp, the grammar table of include/ryujin_hip.h) written twice -- as the
string the library parses and as a Python function over numpy arrays.

ARITHMETIC   + - * /, sqrt, comparisons, selection, rounding, the power rewrite: every operation is exactly rounded or
             exact, the numpy function performs the same operations in the same order, so the two agree BIT FOR BIT.
FUNCTIONS    one library function each. The argument is the same double on both sides, so the difference is the two
             implementations' errors alone: bound = B_f EPS |result| (tests/helpers_initial_values.py: exp 2, sin and
             cos 3, sqrt 1, pow 2.5 (1 + |y ln x|)). For the functions the project states no B_f for (tan, the inverse
             and hyperbolic functions, the logarithms, erf, erfc) the cap is B = 16: a condition that catches a wrong
             opcode or a wrong function, not an accuracy claim. Their arguments are drawn where the condition number
             |x f'(x) / f(x)| is at most 4 (the intervals below; e.g. acos on [-0.9, 0.8], log on [1.5, 10], erfc on
             [-2, 1]), so that the cap is not an artefact of cancellation inside the function.
COMPOSITES   expressions of several functions, through the error arithmetic `Err` of helpers_initial_values.
"""
from __future__ import annotations

import math

import numpy as np

import helpers_initial_values as hiv
from helpers_initial_values import EPS, Err

B_UNSTATED = 16.0


def rounded(v):
    """nearest integer, halves away from zero, as the table defines it"""
    v = np.asarray(v, dtype=np.float64)
    return np.trunc(v + np.where(v >= 0.0, 0.5, -0.5))


def truth(mask):
    return np.where(mask, 1.0, 0.0)


def if_(c, a, b):
    return np.where(rounded(c) != 0.0, a, b)


def select(c, a, b):
    return np.where(c != 0.0, a, b)


def min_(a, b):
    return np.where(b < a, b, a)


def max_(a, b):
    return np.where(a < b, b, a)


def _full(x, c):
    return np.full_like(x, c)


KPP = "0.78539816339 * if(x*x + y*y < 1, 14, 1)"

# (expression, dim, function of (x, y, z, t) -> [n]); y, z are None below their dimension
ARITHMETIC = [
    ("0.25 * x", 1, lambda x, y, z, t: 0.25 * x),
    ("x - t", 1, lambda x, y, z, t: x - t),
    ("1 + 0.5 * x * (x < 0.25) - t / (2 + x*x)", 1,
     lambda x, y, z, t: 1.0 + 0.5 * x * truth(x < 0.25) - t / (2.0 + x * x)),
    ("x^2 - x^3 + x^4", 1, lambda x, y, z, t: x * x - x * x * x + x * x * x * x),
    ("-x^2 + +x", 1, lambda x, y, z, t: -(x * x) + x),
    ("sqrt(abs(x)) * sign(x) + int(3*x) + rint(3*x) + floor(x) + ceil(x)", 1,
     lambda x, y, z, t: np.sqrt(np.abs(x)) * np.sign(x) + rounded(3.0 * x) + np.floor(3.0 * x + 0.5) + np.floor(x) +
     np.ceil(x)),
    (KPP, 2, lambda x, y, z, t: 0.78539816339 * if_(truth(x * x + y * y < 1.0), _full(x, 14.0), _full(x, 1.0))),
    ("x*x + y*y <= 1 ? sqrt(2 - x*x - y*y) : min(x, y, t) / max(2, x + y)", 2,
     lambda x, y, z, t: select(truth(x * x + y * y <= 1.0), np.sqrt(np.maximum(2.0 - x * x - y * y, 0.0)),
                               min_(min_(x, y), _full(x, t)) / max_(_full(x, 2.0), x + y))),
    ("(x > 0 && y > 0) + 2 * (x > 0 || y > 0) + 4 * (x & y) + 8 * (x | y) + 16 * (x != y) + 32 * (x >= y)", 2,
     lambda x, y, z, t: truth((x > 0.0) & (y > 0.0)) + 2.0 * truth((x > 0.0) | (y > 0.0)) +
     4.0 * truth((rounded(x) != 0.0) & (rounded(y) != 0.0)) + 8.0 * truth((rounded(x) != 0.0) | (rounded(y) != 0.0)) +
     16.0 * truth(x != y) + 32.0 * truth(x >= y)),
    ("if(x - y, x / (1 + y*y), -y) * (t + 1)", 2,
     lambda x, y, z, t: if_(x - y, x / (1.0 + y * y), -y) * (t + 1.0)),
    ("x * y - z / (1.5 + t) + (x < y) * (y < z) - x^2 * z", 3,
     lambda x, y, z, t: x * y - z / (1.5 + t) + truth(x < y) * truth(y < z) - x * x * z),
    ("sqrt(x*x + y*y + z*z) == 0 ? 1 : x / sqrt(x*x + y*y + z*z)", 3,
     lambda x, y, z, t: select(truth(np.sqrt(x * x + y * y + z * z) == 0.0), _full(x, 1.0),
                               x / np.where(np.sqrt(x * x + y * y + z * z) == 0.0, 1.0,
                                            np.sqrt(x * x + y * y + z * z)))),
]


def arithmetic_points(dim, n=1000, seed=11):
    """n random points of [-2, 2]^dim, the first ones replaced by the points where the comparisons above are decided
    by equality: (+-1, 0) and (0, +-1) on the unit circle of the KPP state, the origin, x = y"""
    rng = np.random.default_rng(seed + dim)
    X = rng.uniform(-2.0, 2.0, size=(n, dim))
    special = [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 0.0],
               [0.5, 0.5, 0.5], [0.25, -0.5, 1.5], [0.6, 0.8, 0.0], [-0.5, 0.5, 2.0], [1.5, -2.5 + 2.0, 0.5]]
    special = np.array(special)[:min(n, 10), :dim]
    X[:len(special)] = special
    return X


def evaluate_numpy(fn, X, t):
    cols = [X[:, d] if d < X.shape[1] else None for d in range(3)]
    with np.errstate(all="ignore"):
        return np.asarray(fn(cols[0], cols[1], cols[2], t), dtype=np.float64) + np.zeros(len(X))


_erf = np.vectorize(math.erf, otypes=[np.float64])
_erfc = np.vectorize(math.erfc, otypes=[np.float64])

# (name, expression in x, lower, upper, numpy function, B_f); the intervals: module docstring
FUNCTIONS = [
    ("exp", "exp(x)", -3.0, 3.0, np.exp, 2.0),
    ("sin", "sin(x)", -3.0, 3.0, np.sin, 3.0),
    ("cos", "cos(x)", -1.5, 1.5, np.cos, 3.0),
    ("sqrt", "sqrt(x)", 0.0, 4.0, np.sqrt, 1.0),
    ("tan", "tan(x)", -1.0, 1.0, np.tan, B_UNSTATED),
    ("asin", "asin(x)", -0.9, 0.9, np.arcsin, B_UNSTATED),
    ("acos", "acos(x)", -0.9, 0.8, np.arccos, B_UNSTATED),
    ("atan", "atan(x)", -3.0, 3.0, np.arctan, B_UNSTATED),
    ("sinh", "sinh(x)", -3.0, 3.0, np.sinh, B_UNSTATED),
    ("cosh", "cosh(x)", -3.0, 3.0, np.cosh, B_UNSTATED),
    ("tanh", "tanh(x)", -3.0, 3.0, np.tanh, B_UNSTATED),
    ("asinh", "asinh(x)", -3.0, 3.0, np.arcsinh, B_UNSTATED),
    ("acosh", "acosh(x)", 1.5, 4.0, np.arccosh, B_UNSTATED),
    ("atanh", "atanh(x)", -0.8, 0.8, np.arctanh, B_UNSTATED),
    ("log", "log(x)", 1.5, 10.0, np.log, B_UNSTATED),
    ("ln", "ln(x)", 1.5, 10.0, np.log, B_UNSTATED),
    ("log2", "log2(x)", 1.5, 10.0, np.log2, B_UNSTATED),
    ("log10", "log10(x)", 1.5, 10.0, np.log10, B_UNSTATED),
    ("erf", "erf(x)", -2.0, 2.0, _erf, B_UNSTATED),
    ("erfc", "erfc(x)", -2.0, 1.0, _erfc, B_UNSTATED),
    # 1 / f: the function's cap and one rounding of the division
    ("cot", "cot(x)", 0.2, 1.0, lambda x: 1.0 / np.tan(x), B_UNSTATED + 1.0),
    ("csc", "csc(x)", 0.2, 3.0, lambda x: 1.0 / np.sin(x), 3.0 + 1.0),
    ("sec", "sec(x)", -1.5, 1.5, lambda x: 1.0 / np.cos(x), 3.0 + 1.0),
]
UNSTATED = tuple(name for name, *_, b in FUNCTIONS if b == B_UNSTATED)


def function_points(lower, upper, n=1000, seed=3):
    return np.random.default_rng(seed).uniform(lower, upper, size=(n, 1))


def function_bound(values, b_f):
    return b_f * EPS * np.abs(values)


# pow: its own B_f, which depends on the arguments
POW = [
    ("x^5", lambda x: np.power(x, 5.0), lambda x: _full(x, 5.0)),
    ("pow(x, 5)", lambda x: np.power(x, 5.0), lambda x: _full(x, 5.0)),
    ("x^2.5", lambda x: np.power(x, 2.5), lambda x: _full(x, 2.5)),
    ("pow(x, -1.4)", lambda x: np.power(x, -1.4), lambda x: _full(x, -1.4)),
    ("x^x", lambda x: np.power(x, x), lambda x: x),
]


def pow_points(n=1000):
    return function_points(0.1, 4.0, n, seed=4)


def pow_bound(x, exponent, values):
    return 2.5 * (1.0 + np.abs(exponent * np.log(x))) * EPS * np.abs(values)


# (expression, dim, function of Err values (x, y, z, t) -> Err); the error arithmetic carries the bound
COMPOSITES = [
    ("exp(0.5 - 0.5*(x*x + y*y)) * sin(x - t) + cos(y)", 2,
     lambda x, y, z, t: hiv.e_exp(0.5 - 0.5 * (x * x + y * y)) * hiv.e_sin(x - t) + hiv.e_cos(y)),
    ("pow(1 + x*x, 0.3) / sqrt(6 + y)", 2,
     lambda x, y, z, t: hiv.e_pow(1.0 + x * x, 0.3) / hiv.e_sqrt(6.0 + y)),
    ("sin(x - t)", 1, lambda x, y, z, t: hiv.e_sin(x - t)),
    ("2 + sin(_pi * (x - t)) * exp(-t)", 1,
     lambda x, y, z, t: 2.0 + hiv.e_sin(Err(np.pi) * (x - t)) * hiv.e_exp(Err(np.asarray(-t)))),
]


def evaluate_err(fn, X, t):
    """(values [n], bound [n]) of a COMPOSITES function at the points X [n, dim]"""
    cols = [Err(X[:, d]) if d < X.shape[1] else None for d in range(3)]
    out = fn(cols[0], cols[1], cols[2], t)
    return out.v + np.zeros(len(X)), out.e + np.zeros(len(X))
