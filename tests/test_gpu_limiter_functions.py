"""The DEVICE limiters pair by pair: Euler<1|2|3>, EulerAeos<1|2|3>, ShallowWater<1|2> in the four (kinetic energy, square
velocity) combinations and ScalarConservation, as the sweeps compose them (limit_fast, then limit if undecided) and in
the EXPENSIVE_BOUNDS_CHECK control flow (limit_checked), through ryujin_hip_debug_function on the cases of
helpers_limiter_cases.py -- 4096 random admissible cases and the named edge rows per family.

  A  parity      |l_dev - l_oracle| <= the case's own tolerance 1e-13 + 4 spread (Y1: the oracle's response to last-bit
                 changes of the inputs; test_limiter_cases_cpu.py caps the cases beyond 1e-10 at 1 % per family),
                 success equal on every case, `undecided` never set for shallow water and scalar conservation
  B  acceptance  the device's l passes the reference's acceptance test of the limited state in exact arithmetic (Y2)
                 wherever success = 1
  C  checked     with debug_expensive_bounds_check the same l bit for bit, success as the oracle's checked flow
  D  the sweeps  run this function: on a developed flow per Description the stored l_ij of one limiter pass equals,
                 bit for bit, what the debug entry returns for (bounds_i, U_i, P_ij) as the device holds them

Every yardstick comes from the reference side (helpers_limiter_cases.py); one launch per family and flow.
"""
import ctypes as C

import numpy as np
import pytest

import helpers_limiter_cases as H
from ryujin_amd import HyperbolicModule, capi, offline

pytestmark = pytest.mark.gpu

ALL = H.FAMILIES + H.VARIANTS
CHECKED = [name for name in ALL if H.family(name).device_entry(checked=True) is not None]


def _launch(params, which, n_out, bounds, U, P):
    lib = capi.load_hip()
    items = np.ascontiguousarray(np.hstack([bounds, U, P]), dtype=np.float64)
    out = np.zeros((items.shape[0], n_out))
    rc = lib.ryujin_hip_debug_function(0, C.byref(params), which, capi.as_ptr(items, capi.c_double_p),
                                       capi.as_ptr(out, capi.c_double_p), items.shape[0])
    assert rc == 0, lib.ryujin_hip_last_error()
    return out


_results = {}


def _device(oracle, name, checked=False):
    """(l, success, undecided) of the device on the family, one launch, shared by the tests"""
    if (name, checked) not in _results:
        fam = H.family(name)
        which, n_out = fam.device_entry(checked)
        out = _launch(fam.params(oracle, checked), which, n_out, fam.bounds, fam.U, fam.P)
        for x in (out,):
            x.setflags(write=False)
        _results[name, checked] = out[:, 0], out[:, 1] != 0, out[:, 2] != 0
    return _results[name, checked]


@pytest.mark.parametrize("name", ALL)
def test_a_device_l_and_success_against_the_oracle(oracle, name):
    fam = H.family(name)
    assert fam.n <= 4200
    l_ref, success_ref, spread, tol = H.conditioning(oracle, fam)
    l, success, undecided = _device(oracle, name)
    err = np.abs(l - l_ref)
    contracted = tol <= H.L_TOL
    print(f"{name}: max |l_dev - l_oracle| = {np.nanmax(err):.3e} (contracted cases: {np.nanmax(err[contracted]):.3e}), "
          f"largest spread = {spread.max():.3e}, uncontracted = {int((~contracted).sum())}, "
          f"undecided = {int(undecided.sum())}")
    bad = np.nonzero(~(err <= tol))[0]
    assert bad.size == 0, [dict(fam.item(i), l_dev=float(l[i]), l_oracle=float(l_ref[i]), spread=float(spread[i]))
                           for i in bad[:3]]
    bad = np.nonzero(success != success_ref)[0]
    assert bad.size == 0, [dict(fam.item(i), success_dev=bool(success[i]), l_dev=float(l[i]),
                                l_oracle=float(l_ref[i]), spread=float(spread[i])) for i in bad[:3]]
    if fam.description in ("sw", "scalar"):
        assert not undecided.any()
    elif fam.n_random and fam.edits.get("limiter_newton_max_iterations", 2) > 0:
        assert undecided.mean() > 0.02       # the Newton tail was exercised
    for label, i in fam.rows.items():        # and every designed row does on the device what it was built for
        assert H.matches(fam.expect[label][0], l[i]), (name, label, l[i], fam.expect[label])


@pytest.mark.parametrize("name", ALL)
def test_b_device_l_passes_the_acceptance_test_in_exact_arithmetic(oracle, name):
    fam = H.family(name)
    l, success, _ = _device(oracle, name)
    ok = H.accepts(oracle, fam, l)
    bad = np.nonzero(success & ~ok)[0]
    assert bad.size == 0, [dict(fam.item(i), l_dev=float(l[i])) for i in bad[:3]]


@pytest.mark.parametrize("name", CHECKED)
def test_c_checked_flow_same_l_and_the_oracles_success(oracle, name):
    fam = H.family(name)
    l, _, _ = _device(oracle, name)
    l_checked, success_checked, undecided = _device(oracle, name, checked=True)
    assert not undecided.any()
    bad = np.nonzero(l_checked != l)[0]
    assert bad.size == 0, [dict(fam.item(i), l_production=float(l[i]), l_checked=float(l_checked[i])) for i in bad[:3]]
    _, success_ref = H.oracle_limit(oracle, fam, checked=True)
    bad = np.nonzero(success_checked != success_ref)[0]
    assert bad.size == 0, [dict(fam.item(i), success_dev=bool(success_checked[i])) for i in bad[:3]]
    assert {H.family(n).description for n in CHECKED} == {"euler", "aeos", "sw", "scalar"}


# ------------------------------------------------------------------------------------------------- D

def _flow(oracle, name):
    """(offline data, parameters, initial state, Dirichlet data, updates, debug function id, outputs per item)"""
    from ryujin_amd.initial_states import (aeos_from_primitive, euler_radial_contrast, euler_uniform,
                                           sw_circular_dam_break)
    if name == "euler_2d":
        off = offline.SyntheticOffline(offline.mach3_step_2d(60))
        return (off, oracle.default_params(capi.EQ_EULER, 2), euler_uniform(off.positions), euler_uniform(off.b_positions),
                40, capi.DEBUG_EULER_LIMIT_2D, 5)
    if name == "euler_3d":
        off = offline.SyntheticOffline(offline.box_3d(12))
        return (off, oracle.default_params(capi.EQ_EULER, 3), euler_radial_contrast(off.positions, radius=0.4), None,
                6, capi.DEBUG_EULER_LIMIT_3D, 5)
    if name == "shallow_water_2d":
        off = offline.SyntheticOffline(offline.rectangle_2d(40, (-5.0, -5.0), (5.0, 5.0)))
        return (off, oracle.default_params(capi.EQ_SHALLOW_WATER, 2), sw_circular_dam_break(off.positions), None,
                10, capi.DEBUG_SW_LIMIT_2D, 3)
    if name == "aeos_2d_nasg":
        off = offline.SyntheticOffline(offline.rectangle_2d(40, (-1.0, -1.0), (1.0, 1.0)))
        p = oracle.default_params(capi.EQ_EULER_AEOS, 2)
        p.eos, p.eos_covolume_b, p.eos_pinf, p.eos_q = capi.EOS_NOBLE_ABEL_STIFFENED_GAS, 0.05, 0.5, 0.1
        r = np.linalg.norm(off.positions, axis=1)
        U0 = aeos_from_primitive(p, np.where(r < 0.4, 2.0, 1.0), np.zeros((off.n_relevant, 2)), np.where(r < 0.4, 10.0, 1.0))
        return off, p, U0, None, 12, capi.DEBUG_AEOS_LIMIT_2D, 5
    off = offline.SyntheticOffline(offline.rectangle_2d(40, (-2.0, -2.5), (2.0, 1.5), bc=capi.BC_DIRICHLET))
    p = oracle.default_params(capi.EQ_SCALAR_CONSERVATION, 2)
    p.sc_flux = capi.FLUX_KPP
    r = np.linalg.norm(off.positions, axis=1)
    U0 = np.where(r < 1.0, 3.4 * np.pi, 0.3 * np.pi).reshape(-1, 1)    # (as test_gpu_parity.test_scalar_parity_2d)
    return off, p, U0, U0[off.b_i], 10, capi.DEBUG_SCALAR_LIMIT, 3


@pytest.mark.parametrize("name", ["euler_2d", "euler_3d", "shallow_water_2d", "aeos_2d_nasg", "scalar_2d_kpp"])
def test_d_the_sweeps_store_what_the_function_returns(oracle, name):
    """One limiter pass on a developed flow: l_ij as step 5 stored it against the debug entry on the device's own
    bounds_i, P_ij and the low-order update U_i (the same update with limiter_iterations = 0, as
    helpers_parity.EulerFlipClassifier._state_seen_by_limiter obtains it). The library is built with
    -ffp-contract=off and both sides inline the same function: bit for bit."""
    off, p, U0, dirichlet, n_updates, which, n_out = _flow(oracle, name)
    p.cfl = 0.9
    m = HyperbolicModule(off, p, backend="hip")
    a, b = m.new_state_vector(U0), m.new_state_vector()
    for _ in range(n_updates):
        m.prepare_state_vector(a, 0.0, dirichlet)
        m.step(a, [], [], b)
        a, b = b, a
    U_start = a.download()
    m.close()
    rng = np.random.default_rng(5)
    U_start *= 1.0 + 1e-3 * rng.uniform(-1.0, 1.0, size=U_start.shape)    # (as test_gpu_tail_visibility.py)

    def update(limiter_iterations, tau=0.0):
        q = capi.Params()
        C.memmove(C.byref(q), C.byref(p), C.sizeof(capi.Params))
        q.limiter_iterations = limiter_iterations
        q.debug_pij_storage = -1
        q.debug_no_small_mesh_split = 1
        mod = HyperbolicModule(off, q, backend="hip")
        old, new = mod.new_state_vector(U_start), mod.new_state_vector()
        mod.prepare_state_vector(old, 0.0, dirichlet)
        tau = mod.step(old, [], [], new, tau)
        got = dict(U=new.download(), tau=tau)
        if limiter_iterations:
            got.update({key: mod.debug_fetch(key).copy() for key in ("bounds", "pij", "lij")})
        mod.close()
        return got, q

    one, q = update(1)
    low, _ = update(0, one["tau"])
    assert low["tau"] == one["tau"]
    n = off.n_owned
    rs = off.row_starts[: n + 1].astype(np.int64)
    cols = off.columns[: rs[-1]].astype(np.int64)
    rows = np.repeat(np.arange(n), np.diff(rs))
    pairs = np.nonzero(cols != rows)[0]
    k = U_start.shape[1]
    bounds = one["bounds"].reshape(n, -1)[rows[pairs]]
    out = _launch(q, which, n_out, bounds, low["U"][rows[pairs]], one["pij"].reshape(-1, k)[pairs])
    stored = one["lij"][pairs]
    between = float(((stored > 0.0) & (stored < 1.0)).mean())
    differing = np.nonzero(out[:, 0] != stored)[0]
    print(f"{name}: {pairs.size} pairs, {between:.3f} strictly between 0 and 1, {differing.size} differ, "
          f"largest difference {np.abs(out[:, 0] - stored).max():.3e}")
    assert between > 0.02, between     # the Newton tail was exercised (the threshold of test_gpu_tail_visibility.py)
    assert differing.size == 0, [(int(rows[pairs[e]]), int(cols[pairs[e]]), float(out[e, 0]), float(stored[e]))
                                 for e in differing[:5]]
