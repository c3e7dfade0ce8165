"""Yardsticks of tests/test_eos_function_cpu.py and tests/test_gpu_eos_function.py: the four closed-form members of the
EquationOfStateLibrary written as the four expressions of the "function" member (pressure and specific internal
energy, temperature, speed of sound), statement by statement in the operation order of oracle/euler_aeos.hpp:70-175,
the constants through repr() -- the shortest string that reads back as the same double. Polytropic gas, Noble-Abel
stiffened gas and van der Waals are exactly rounded operations only (+ - * / sqrt): the interpreter agrees with the
oracle BIT FOR BIT. Jones-Wilkins-Lee has one exp per term; its bound is jwl_bound() below.

Also an equation of state the library does not have (LINEARISED and its `if` variant), as string and numpy function."""
from __future__ import annotations

import ctypes as C

import numpy as np

from helpers_initial_values import EPS
from ryujin_amd import capi

B_EXP = 2.0   # tests/helpers_expression.py: the cap of exp, device or host against another implementation

# the parameter sets of tests/test_gpu_parity.py::test_aeos_step_parity_equations_of_state, and the polytropic gas
MEMBERS = {
    "polytropic": dict(eos=capi.EOS_POLYTROPIC_GAS),
    "nasg": dict(eos=capi.EOS_NOBLE_ABEL_STIFFENED_GAS, eos_covolume_b=0.05, eos_pinf=0.5, eos_q=0.1),
    "vdw": dict(eos=capi.EOS_VAN_DER_WAALS, eos_covolume_b=0.1, eos_vdw_a=0.01),
    "jwl": dict(eos=capi.EOS_JONES_WILKINS_LEE, jwl_A=1.0, jwl_B=-0.1, jwl_R1=4.0, jwl_R2=1.0, jwl_omega=0.4,
                jwl_rho_0=1.0, jwl_q_0=0.0, jwl_cv=1.0),
}
FUNCTIONS = ("pressure", "specific_internal_energy", "temperature", "speed_of_sound")


def c(value: float) -> str:
    """a constant as a parenthesised literal: repr() round-trips, the sign is an exact negation"""
    return "(" + repr(float(value)) + ")"


def member_params(p, name):
    """`p` (a capi.Params of EulerAEOS) with the member's parameters set"""
    for key, value in MEMBERS[name].items():
        setattr(p, key, value)
    return p


def member_expressions(p) -> dict:
    """The closed-form member selected by the capi.Params `p` as keyword arguments of
    HyperbolicModule.eos_configure_function: four expressions and the interpolation parameters of
    oracle/euler_aeos.hpp:55-72."""
    G, R = c(p.gamma), c(p.eos_gas_constant_R)
    cv = f"({R}/({G} - 1.))"
    if p.eos == capi.EOS_POLYTROPIC_GAS:
        return dict(pressure=f"({G} - 1.)*rho*e",
                    specific_internal_energy=f"p/(rho*({G} - 1.))",
                    temperature=f"e/{cv}",
                    speed_of_sound=f"sqrt({G}*({G} - 1.)*e)",
                    interpolation_b=0.0, interpolation_pinfty=0.0, interpolation_q=0.0)
    if p.eos == capi.EOS_NOBLE_ABEL_STIFFENED_GAS:
        B, Q, PINF = c(p.eos_covolume_b), c(p.eos_q), c(p.eos_pinf)
        cov = f"(1. - {B}*rho)"
        return dict(pressure=f"({G} - 1.)*rho*(e - {Q})/{cov} - {G}*{PINF}",
                    specific_internal_energy=f"{Q} + (p + {G}*{PINF})*{cov}/(rho*({G} - 1.))",
                    temperature=f"(e - {Q} - {PINF}*(1./rho - {B}))/{cv}",
                    speed_of_sound=f"sqrt((rho*(e - {Q}) - {PINF}*{cov})/rho*({G}*({G} - 1.)))/{cov}",
                    interpolation_b=p.eos_covolume_b, interpolation_pinfty=p.eos_pinf, interpolation_q=p.eos_q)
    if p.eos == capi.EOS_VAN_DER_WAALS:
        A, B = c(p.eos_vdw_a), c(p.eos_covolume_b)
        cov = f"(1. - {B}*rho)"
        b = p.eos_covolume_b
        return dict(pressure=f"({G} - 1.)*(rho*e + {A}*rho*rho)/{cov} - {A}*rho*rho",
                    specific_internal_energy=f"(p + {A}*rho*rho)*{cov}/(rho*({G} - 1.)) - {A}*rho",
                    temperature=f"(e + {A}*rho)/{cv}",
                    speed_of_sound=f"sqrt({G}*({G} - 1.)*(e + {A}*rho)/({cov}*{cov}) - 2.*{A}*rho)",
                    interpolation_b=b, interpolation_pinfty=p.eos_vdw_a / (b * b) if b > 0.0 else 0.0,
                    interpolation_q=0.0)
    assert p.eos == capi.EOS_JONES_WILKINS_LEE
    A, B, R1, R2 = c(p.jwl_A), c(p.jwl_B), c(p.jwl_R1), c(p.jwl_R2)
    W, RHO0, Q0, CV = c(p.jwl_omega), c(p.jwl_rho_0), c(p.jwl_q_0), c(p.jwl_cv)
    ratio = f"(rho/{RHO0})"
    first = f"{A}*(1. - {W}/{R1}*{ratio})*exp(-{R1}*1./{ratio})"
    second = f"{B}*(1. - {W}/{R2}*{ratio})*exp(-{R2}*1./{ratio})"
    t1, t2 = f"({W}*rho/({R1}*{RHO0}))", f"({W}*rho/({R2}*{RHO0}))"
    s1 = f"{A}/rho*({W}*(1. - {t1})*(1. + 1./{t1}) - {t1})*exp(-1./{t1}/{W})"
    s2 = f"{B}/rho*({W}*(1. - {t2})*(1. + 1./{t2}) - {t2})*exp(-1./{t2}/{W})"
    return dict(pressure=f"{first} + {second} + {W}*rho*(e + {Q0})",
                specific_internal_energy=f"(p - {first} - {second})/(rho*{W})",
                temperature=(f"(e + {Q0} - 1./{RHO0}*({A}/{R1}*exp(-{R1}*1./{ratio}) + "
                             f"{B}/{R2}*exp(-{R2}*1./{ratio})))/{CV}"),
                speed_of_sound=f"sqrt({s1} + {s2} + {W}*({W} + 1.)*e)",
                interpolation_b=0.0, interpolation_pinfty=0.0, interpolation_q=0.0)


def expression_of(expressions: dict, which: int) -> str:
    return expressions[FUNCTIONS[which]]


def oracle_functions(oracle, p, rho, e):
    """(p(rho, e), e(rho, p(rho, e)) -- the oracle's own round trip --, T(rho, e), c(rho, e)) [4][n] and the pressure
    handed to specific_internal_energy, through ryujin_oracle_aeos_eos, the entry tests/test_oracle_golden_aeos.py
    uses"""
    lib = oracle.lib()
    out = (C.c_double * 7)()
    result = np.zeros((4, len(rho)))
    for n, (r, ee) in enumerate(zip(rho, e)):
        assert lib.ryujin_oracle_aeos_eos(C.byref(p), float(r), float(ee), 0.0, out) == 0
        pressure = out[0]
        assert lib.ryujin_oracle_aeos_eos(C.byref(p), float(r), float(ee), pressure, out) == 0
        result[:, n] = out[0], out[1], out[2], out[3]
    return result


def admissible_points(name, n=1000, seed=5):
    """n random (rho, e) of [0.2, 3] x [3, 8]: for the parameter sets above the covolume 1 - b rho stays above 0.7 and
    every radicand positive (the smallest, NASG at rho = 0.2 and e = 3: 0.2 * 2.9 - 0.5 * 0.99 > 0)"""
    rng = np.random.default_rng(seed)
    rho = rng.uniform(0.2, 3.0, size=n)
    e = rng.uniform(3.0, 8.0, size=n)
    return rho, e


def jwl_bound(p, which, rho, second):
    """|interpreter - oracle| for the Jones-Wilkins-Lee member when the two exp differ by B_EXP ulp at most (they are
    the same libm function on the same operand on the CPU, where the difference is 0; the device's exp is another
    one). Every term that holds an exp, t = a * exp(.), then differs by (B_EXP + 1) EPS |t| -- the cap and one rounding
    of the product --, and each of the n - 1 additions of a sum of n terms may round to the other neighbour: EPS
    times the sum of the absolute terms. What is applied to the sum afterwards adds its own rounding and scales the
    difference: the division of sie and T by their condition-free denominators, the sqrt of c by 1 / (2 sqrt(s))."""
    A, B, R1, R2, w, rho0, q0 = p.jwl_A, p.jwl_B, p.jwl_R1, p.jwl_R2, p.jwl_omega, p.jwl_rho_0, p.jwl_q_0
    ratio = rho / rho0
    first = A * (1. - w / R1 * ratio) * np.exp(-R1 / ratio)
    second_term = B * (1. - w / R2 * ratio) * np.exp(-R2 / ratio)

    def sum_bound(with_exp, others):
        n_terms = len(with_exp) + len(others)
        total = sum(np.abs(t) for t in with_exp + others)
        return EPS * ((B_EXP + 1.) * sum(np.abs(t) for t in with_exp) + (n_terms - 1) * total)

    if which == 0:
        return sum_bound([first, second_term], [w * rho * (second + q0)])
    if which == 1:
        numerator = second - first - second_term
        return sum_bound([first, second_term], [second]) / np.abs(rho * w) + EPS * np.abs(numerator / (rho * w))
    if which == 2:
        f, s = A / R1 * np.exp(-R1 / ratio), B / R2 * np.exp(-R2 / ratio)
        inner = sum_bound([f, s], []) / rho0 + EPS * np.abs((f + s) / rho0)
        value = (second + q0 - (f + s) / rho0) / p.jwl_cv
        return (inner + EPS * (np.abs(second + q0) + np.abs((f + s) / rho0))) / abs(p.jwl_cv) + EPS * np.abs(value)
    t1, t2 = w * rho / (R1 * rho0), w * rho / (R2 * rho0)
    a = A / rho * (w * (1. - t1) * (1. + 1. / t1) - t1) * np.exp(-1. / t1 / w)
    b = B / rho * (w * (1. - t2) * (1. + 1. / t2) - t2) * np.exp(-1. / t2 / w)
    third = w * (w + 1.) * second
    radicand = a + b + third
    return sum_bound([a, b], [third]) / (2. * np.sqrt(radicand)) + EPS * np.sqrt(radicand)


# ---- an equation of state the library does not have: a polytropic gas with a linear elastic term,
#      p = (1.4 - 1) rho e + c^2 (rho - 1); the surrogate interpolates it with p_infty = c^2
SOUND = 0.5
LINEARISED = dict(pressure=f"(1.4-1)*rho*e + {SOUND}*{SOUND}*(rho - 1)",
                  specific_internal_energy=f"(p - {SOUND}*{SOUND}*(rho - 1))/((1.4-1)*rho)",
                  interpolation_b=0.0, interpolation_pinfty=SOUND * SOUND, interpolation_q=0.0)
# the elastic term only under compression
LINEARISED_IF = dict(pressure=f"if(rho < 1, (1.4-1)*rho*e, (1.4-1)*rho*e + {SOUND}*{SOUND}*(rho - 1))",
                     specific_internal_energy=(f"if(rho < 1, p/((1.4-1)*rho), "
                                               f"(p - {SOUND}*{SOUND}*(rho - 1))/((1.4-1)*rho))"),
                     interpolation_b=0.0, interpolation_pinfty=SOUND * SOUND, interpolation_q=0.0)


def linearised_pressure(rho, e, with_if=False):
    gas = (1.4 - 1) * rho * e
    full = gas + SOUND * SOUND * (rho - 1)
    return np.where(rho < 1, gas, full) if with_if else full


def linearised_sie(rho, p, with_if=False):
    full = (p - SOUND * SOUND * (rho - 1)) / ((1.4 - 1) * rho)
    return np.where(rho < 1, p / ((1.4 - 1) * rho), full) if with_if else full
