"""State transfer between the caller's AoS arrays (K doubles per row) and the device vectors (KP = K padded to whole
pairs): ryujin_hip_state_upload / _download / _download_owned / _download_prepared, bit for bit, with K != KP (Euler 1-D,
shallow water 2-D) and K == KP (Euler 2-D), on one rank and on two (in-process transport: a ghost range). And: a
create() that is refused touches no device -- a valid one on the same device works afterwards."""
import ctypes as C

import numpy as np
import pytest

import helpers_partitioned as partitioned
from ryujin_amd import HyperbolicModule, capi, offline

pytestmark = pytest.mark.gpu

CASES = {
    "euler_1d": (capi.EQ_EULER, lambda **kw: offline.MeshSpec(1, (200,), (0.0,), (1.0,),
                                                             (capi.BC_DIRICHLET, capi.BC_DO_NOTHING))),
    "euler_2d": (capi.EQ_EULER, lambda **kw: offline.rectangle_2d(12)),
    "shallow_water_2d": (capi.EQ_SHALLOW_WATER, lambda **kw: offline.rectangle_2d(12)),
    "euler_2d_two_ranks": (capi.EQ_EULER, lambda **kw: offline.mach3_step_2d(20, **kw)),
}


def _random_states(rng, n, k):
    """admissible for Euler and shallow water alike: density / depth in (1, 2), small momenta, a large last component"""
    U = rng.uniform(-0.5, 0.5, (n, k))
    U[:, 0] = rng.uniform(1.0, 2.0, n)
    if k > 2:
        U[:, -1] = rng.uniform(5.0, 6.0, n)
    return U


def _round_trip(m, part, rank):
    rng = np.random.default_rng(11 + rank)
    U = _random_states(rng, part.n_relevant, m.k)
    dirichlet = _random_states(rng, part.n_bdry, m.k)
    sv = m.new_state_vector(U)
    assert np.array_equal(sv.download(), U)
    owned = np.full_like(U, np.nan)
    m._check(m._lib.ryujin_hip_state_download_owned(m._ctx, sv.handle, capi.as_ptr(owned, capi.c_double_p)))
    assert np.array_equal(owned[: part.n_owned], U[: part.n_owned]) and np.isnan(owned[part.n_owned:]).all()

    m.prepare_state_vector(sv, 0.0, dirichlet)
    prepared = U.copy()
    m._check(m._lib.ryujin_hip_state_download_prepared(m._ctx, sv.handle, capi.as_ptr(prepared, capi.c_double_p)))
    after = sv.download()
    b_i = capi.np_from_ptr(part.c.contents.b_i, part.n_bdry, np.uint32)
    b_id = capi.np_from_ptr(part.c.contents.b_id, part.n_bdry, np.uint8)
    touched = np.zeros(part.n_relevant, dtype=bool)
    touched[b_i] = True
    touched[part.n_owned:] = True
    # it differs from the upload in the boundary rows and the ghost range only, and equals download() there ...
    assert np.array_equal(prepared[~touched], U[~touched]) and np.array_equal(after[~touched], U[~touched])
    assert np.array_equal(prepared[touched], after[touched])
    # ... where the boundary conditions and the exchange did change the random data
    changed = (prepared != U).any(axis=1)
    rewritten = np.unique(b_i[np.isin(b_id, (capi.BC_DIRICHLET, capi.BC_SLIP))])
    assert len(rewritten) > 0 and changed[rewritten].all()
    assert changed[part.n_owned:].all()
    return dict(n_ghost=part.n_relevant - part.n_owned, n_changed=int(changed.sum()))


@pytest.mark.parametrize("case", ["euler_1d", "euler_2d", "shallow_water_2d"])
def test_round_trip(case):
    equation, spec = CASES[case]
    off = offline.SyntheticOffline(spec())
    m = HyperbolicModule(off, equation=equation)
    assert (m.k % 2 == 1) == (case != "euler_2d")   # K != KP but for Euler 2-D
    out = _round_trip(m, off, 0)
    m.close()
    assert out["n_ghost"] == 0


def test_round_trip_on_two_ranks():
    equation, spec = CASES["euler_2d_two_ranks"]
    parts = [offline.SyntheticOffline(spec(n_ranks=2, rank=r)) for r in range(2)]

    def params():
        p = capi.Params()
        capi.load_hip().ryujin_hip_default_params(C.byref(p), equation, 2)
        return p
    out = partitioned.run_hip_ranks(parts, params, _round_trip)
    assert all(o["n_ghost"] > 0 for o in out)


def test_a_refused_create_leaves_the_device_usable():
    lib = capi.load_hip()
    off = offline.SyntheticOffline(CASES["euler_2d"][1]())
    p = capi.Params()
    lib.ryujin_hip_default_params(C.byref(p), capi.EQ_EULER, 2)
    p.limiter_iterations = 5
    ctx = C.c_void_p()
    rc = lib.ryujin_hip_create(C.byref(ctx), off.c, C.byref(p), None, 0)
    if rc >= 0:
        lib.ryujin_hip_destroy(ctx)
    assert rc == capi.RYUJIN_ERR_ARG and b"limiter iterations" in lib.ryujin_hip_last_error()
    m = HyperbolicModule(off, equation=capi.EQ_EULER)
    assert _round_trip(m, off, 0)["n_changed"] > 0
    m.close()
