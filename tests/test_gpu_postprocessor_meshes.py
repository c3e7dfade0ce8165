"""The postprocessor sweep on every mesh family the update is tested on (tests/helpers_postprocessor_cases.py: the case
table; tests/test_postprocessor_cases_cpu.py pins its literals and that no case is vacuous). Every case runs the whole
call -- postprocess, postprocess_download(raw=True), postprocess_bounds -- and is compared by _compare of
tests/test_gpu_postprocessor.py with the derived tolerances of tests/helpers_postprocessor.py: raw values row by row on
100 % of the owned rows, both bounds, the normalised values, isfinite everywhere, |normalised| < 1.

What runs here and nowhere else in the postprocessor's suite: meshes of one partial slice, exactly one slice, one slice
and one row; rows narrower than their slice (c < r.len against r.width) up to 1023 entries; irregular tiles under a
compiled-in tile map; the band and chunk renumberings with a partial last band; ranks with up to four neighbours, ranks
of 16 rows that export all of them; rows of length 1.

Each test prints the largest ratio of error to tolerance it measured (`pp_mesh <family> <case>: raw bounds normalised`)
before it asserts."""
import numpy as np
import pytest

import helpers_postprocessor as hp
import helpers_postprocessor_cases as pc
import helpers_small_meshes as sm
from helpers_partitioned import run_hip_ranks
from ryujin_amd import HyperbolicModule
from test_gpu_postprocessor import _compare

pytestmark = pytest.mark.gpu

BETA = 10.0


def _measure(label, off, U, names, quantities, eq, params, dev_raw, dev_bounds, dev_norm, reference=None):
    """the largest error / tolerance of raw values, bounds and normalised values: the figures _compare asserts on"""
    raw, scale = hp.raw_values(off, U, quantities, eq, params)
    ref_raw, ref_scale = (raw, scale) if reference is None else reference
    worst = [0.0, 0.0, 0.0]
    for k, name in enumerate(names):
        tol = hp.raw_tolerance(scale[k])
        err = np.abs(dev_raw[name] - raw[k])
        worst[0] = max(worst[0], float(np.where(err > 0.0, err / np.maximum(tol, 1e-300), 0.0).max()))
        q_max, q_min = hp.bounds(ref_raw[k])
        d_max, d_min = hp.bounds_tolerance(ref_raw[k], ref_scale[k])
        for got, want, d in ((dev_bounds[name][0], q_max, d_max), (dev_bounds[name][1], q_min, d_min)):
            if got != want:
                worst[1] = max(worst[1], abs(got - want) / max(d, 1e-300))
        ntol = hp.normalised_tolerance(scale[k], max(d_max, d_min), q_max, q_min, BETA)
        worst[2] = max(worst[2], float((np.abs(dev_norm[name] - hp.normalise(raw[k], q_max, q_min, BETA)) / ntol).max()))
    print(f"\npp_mesh {label}: raw {worst[0]:.3e} bounds {worst[1]:.3e} normalised {worst[2]:.3e}")


def _sweep(off, equation, U, params, schlieren=None, vorticity=None):
    """the whole call on one context: (normalised, raw, bounds, the state as the device holds it)"""
    if schlieren is None:
        schlieren, vorticity = pc.quantities(equation, off.dim)
    m = HyperbolicModule(off, params, backend="hip")
    state = m.new_state_vector(U)
    norm = m.postprocess(state, schlieren=schlieren, vorticity=vorticity, beta=BETA)
    out = norm, m.postprocess_download(raw=True), m.postprocess_bounds(), state.download()
    m.close()
    return out


def _run_case(name, **switches):
    case, off = pc.CASES[name], pc.mesh(name)
    equation, eq = case["equation"], pc.EQUATIONS[case["equation"]]
    params = pc.params(equation, off.dim, **switches)
    U = pc.case_state(name, params)
    quantities, names = hp.resolve(eq, off.dim, *pc.quantities(equation, off.dim))
    norm, raw, bounds, U_dev = _sweep(off, equation, U, params)
    assert list(norm) == names and np.array_equal(U_dev[: off.n_owned], U[: off.n_owned])
    label = f"{case['family']} {name}"
    _measure(label, off, U, names, quantities, eq, params, raw, bounds, norm)
    _compare(label, off, U, names, quantities, eq, params, raw, bounds, norm, BETA)
    return off, names, raw, bounds, norm


def _family(letter):
    return sorted(n for n, c in pc.CASES.items() if c["family"] == letter)


# ------------------------------------------------------------------ A, C, D, E: one context, against numpy

@pytest.mark.parametrize("name", _family("A"))
def test_at_and_below_one_slice(name):
    """one partial slice, exactly one slice, one slice and one row, two slices; rows of 2, 4, 8 and 18 entries. The
    single-cell meshes: q_max == q_min to round-off, the normalisation divides by max(q_max - q_min, eps) -- what
    numpy gives, whatever it is"""
    _run_case(name)


@pytest.mark.parametrize("name", _family("C"))
def test_row_widths(name):
    """narrow rows padded next to full ones in every slice, on both sides of every width threshold of the update and
    at 1023 entries, where the tolerance is the forward bound of the summation"""
    _run_case(name)


@pytest.mark.parametrize("name", _family("D"))
def test_q2_lattices(name):
    _run_case(name)


@pytest.mark.parametrize("name", _family("E"))
def test_unstructured_p1(name):
    """ragged rows, irregular tiles under the compiled-in tile map (2-D), m_i over orders of magnitude; shallow water
    with dry nodes, with and without a residual momentum"""
    _run_case(name)


@pytest.mark.parametrize("which", ["disk", "ball"])
def test_unstructured_p1_identities_on_the_device(which):
    """rho = a . x + b and a rigid rotation: schlieren(rho) = |a|, vorticity(v) = 2 omega (signed, 2-D) or 2 |omega|
    (3-D) -- the device values against the identity itself. numpy meets it to the per-row tolerance
    (tests/test_postprocessor_cases_cpu.py) and the device meets numpy to the same: twice that here."""
    from test_postprocessor_cases_cpu import A2, A3, OMEGA2, OMEGA3
    off, info = pc.p1(which)
    a, omega = (A2, OMEGA2) if off.dim == 2 else (A3, OMEGA3)
    params = pc.params("euler", off.dim)
    U = pc.linear_density_rigid_rotation(off.positions, a, 3.0, omega)
    quantities, names = hp.resolve(pc.EQUATIONS["euler"], off.dim, ("rho",), ("v_1",))
    norm, raw, bounds, _ = _sweep(off, "euler", U, params, ("rho",), ("v_1",))
    _, scale = hp.raw_values(off, U, quantities, pc.EQUATIONS["euler"], params)
    rows = pc.interior_rows(info)
    expected = (np.linalg.norm(a), 2.0 * omega if off.dim == 2 else 2.0 * np.linalg.norm(omega))
    for k, name in enumerate(names):
        err, tol = np.abs(raw[name] - expected[k])[rows], 2.0 * hp.raw_tolerance(scale[k])[rows]
        print(f"\npp_mesh E identity {which} {name}: max err / tol {(err / tol).max():.3e}")
        assert (err <= tol).all(), (name, float((err / tol).max()))


# ------------------------------------------------------------------ B: the layout switches

@pytest.mark.parametrize("name", pc.LAYOUT_SWITCH_CASES)
def test_layout_switches_give_the_same_bits(name):
    """The sweep adds the terms of a row in column order whichever wave takes the slice, and the bounds are exact
    maxima and minima: raw values, normalised values and both bounds under every switch the postprocessor reads are
    those of the default parameters, bit for bit. (Two runs of the same code: a sweep that is wrong in the same way
    under every layout passes here; families A and C - G are what catches it.)"""
    if name in pc.CASES:
        off, equation = pc.mesh(name), pc.CASES[name]["equation"]
    else:
        off, equation = sm.CASES[name]["mesh"](), sm.CASES[name]["equation"]
    results = []
    for switches in ({},) + pc.LAYOUT_SWITCHES:
        params = pc.params(equation, off.dim, **switches)
        U = pc.state(equation, pc.box_of(off), off.positions, params)
        results.append(_sweep(off, equation, U, params)[:3])
    assert all(np.isfinite(v).all() for v in results[0][1].values())
    for switches, (norm, raw, bounds) in zip(pc.LAYOUT_SWITCHES, results[1:]):
        for q in results[0][0]:
            assert np.array_equal(raw[q], results[0][1][q]), (name, switches, q, "raw")
            assert np.array_equal(norm[q], results[0][0][q]), (name, switches, q, "normalised")
            assert bounds[q] == results[0][2][q], (name, switches, q, "bounds")


# ------------------------------------------------------------------ F: arbitrary partitions, stale ghosts

@pytest.mark.parametrize("name", sorted(pc.RANK_CASES))
def test_partitioned_with_stale_ghosts(name):
    """sectors of the P1 disk (up to four neighbours per rank, nodes exported to several of them) and x-slabs of 16
    rows (the middle ranks export every row), over the in-process transport. Every rank gets a state whose ghost range
    is NOT current. Per rank: raw values against the numpy field of the single-rank mesh at the rank's rows, the same
    bounds on all ranks, bit by bit, within tolerance of the single-rank bounds, and the normalised values against the
    single-rank normalisation."""
    single, parts, box = pc.rank_case(name)
    eq = pc.EQUATIONS["euler"]
    params = pc.params("euler", single.dim)
    schlieren, vorticity = pc.quantities("euler", single.dim)
    quantities, names = hp.resolve(eq, single.dim, schlieren, vorticity)
    reference = hp.raw_values(single, pc.state("euler", box, single.positions, params), quantities, eq, params)

    def body(m, part, r):
        stale = pc.state("euler", box, part.positions, params)
        stale[part.n_owned:] = 0.0   # compute() has to exchange the ghost range
        state = m.new_state_vector(stale)
        norm = m.postprocess(state, schlieren=schlieren, vorticity=vorticity, beta=BETA)
        return norm, m.postprocess_download(raw=True), m.postprocess_bounds(), state.download()

    ranks = run_hip_ranks(parts, lambda: pc.params("euler", single.dim), body)
    for r, (norm, raw, bounds, U_after) in enumerate(ranks):
        part = parts[r]
        U = pc.state("euler", box, part.positions, params)
        np.testing.assert_allclose(U_after, U, rtol=1e-14, atol=0.0)   # the exchange filled the ghost range
        assert bounds == ranks[0][2]
        rows = pc.global_rows(single, part)
        label = f"F {name} rank {r}"
        _measure(label, part, U, names, quantities, eq, params, raw, bounds, norm, reference)
        _compare(label, part, U, names, quantities, eq, params, raw, bounds, norm, BETA, reference_rows=rows,
                 reference=reference)
    # the bounds are those of ALL ranks: no single rank's rows give both
    own = [hp.bounds(ranks[r][1][names[0]]) for r in range(len(parts))]
    assert len(set(own)) > 1


# ------------------------------------------------------------------ G: rows of length 1

@pytest.mark.parametrize("name", _family("G"))
def test_rows_of_length_one(name):
    """a handful of rows cut down to their diagonal: raw value 0 exactly, q_min = 0 exactly, everything else as numpy
    gives it. One cut row is the last lane of a slice that is otherwise full, one the last row of the mesh."""
    off, names, raw, bounds, norm = _run_case(name)
    cut = list(pc.CASES[name]["cut"])
    for q in names:
        assert (raw[q][cut] == 0.0).all() and (norm[q][cut] == 0.0).all()
        assert bounds[q][1] == 0.0 and bounds[q][0] > 0.0
        assert (np.delete(raw[q], cut) != 0.0).any()


def test_the_one_sided_cut_is_refused():
    """the layout wants a structurally symmetric pattern: a mesh whose cut rows stay in their neighbours' columns is
    refused at create(), before anything is launched -- why family G cuts both sides"""
    off = pc.cut_rows(pc.p1("disk")[0], pc.CUT_DISK, one_sided=True)
    with pytest.raises(RuntimeError, match="not structurally symmetric"):
        HyperbolicModule(off, pc.params("euler", 2), backend="hip")
