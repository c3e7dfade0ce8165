"""The HIP-free selection logic of VTUOutput (ryujin_amd/csrc/output_selection.hpp) on the CPU: the name tables and the
resolver against the reference's arrays (source/<eq>/hyperbolic_system.h, source/selected_components_extractor.h,
source/postprocessor.template.h), restated here by hand; the cell rule of vtu_output.template.h:171-187 on hand-made
vertex values; the order-preserving compaction plan against numpy.flatnonzero. The checker
(tests/cpp/output_selection_cases.cc) is a stand-alone program built with the address and undefined-behaviour
sanitizers; it prints what the header computes, the expectations are formed here."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from ryujin_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "output_selection_cases")
EPS = np.finfo(np.float64).eps
CONSERVED, PRIMITIVE, PRECOMPUTED, INITIAL, ALPHA, POSTPROCESSED = range(6)
BLOCK = 256   # kOutputBlock

# the reference's arrays, written out (View::component_names, primitive_component_names, precomputed_names,
# initial_precomputed_names); shallow water has them up to dim = 3 although the library runs it up to 2-D
REFERENCE = {
    (capi.EQ_EULER, 1): (["rho", "m", "E"], ["rho", "v", "p"], ["s", "eta_h"], []),
    (capi.EQ_EULER, 2): (["rho", "m_1", "m_2", "E"], ["rho", "v_1", "v_2", "p"], ["s", "eta_h"], []),
    (capi.EQ_EULER, 3): (["rho", "m_1", "m_2", "m_3", "E"], ["rho", "v_1", "v_2", "v_3", "p"], ["s", "eta_h"], []),
    (capi.EQ_EULER_AEOS, 1): (["rho", "m", "E"], ["rho", "v", "e"],
                              ["p", "surrogate_gamma", "surrogate_specific_entropy", "surrogate_harten_entropy"], []),
    (capi.EQ_EULER_AEOS, 2): (["rho", "m_1", "m_2", "E"], ["rho", "v_1", "v_2", "e"],
                              ["p", "surrogate_gamma", "surrogate_specific_entropy", "surrogate_harten_entropy"], []),
    (capi.EQ_EULER_AEOS, 3): (["rho", "m_1", "m_2", "m_3", "E"], ["rho", "v_1", "v_2", "v_3", "e"],
                              ["p", "surrogate_gamma", "surrogate_specific_entropy", "surrogate_harten_entropy"], []),
    (capi.EQ_SHALLOW_WATER, 1): (["h", "m"], ["h", "v"], ["eta_m", "h_star"], ["bathymetry"]),
    (capi.EQ_SHALLOW_WATER, 2): (["h", "m_1", "m_2"], ["h", "v_1", "v_2"], ["eta_m", "h_star"], ["bathymetry"]),
    (capi.EQ_SHALLOW_WATER, 3): (["h", "m_1", "m_2", "m_3"], ["h", "v_1", "v_2", "v_3"], ["eta_m", "h_star"],
                                 ["bathymetry"]),
    (capi.EQ_SCALAR_CONSERVATION, 1): (["u"], ["u"], ["f", "df"], []),
    (capi.EQ_SCALAR_CONSERVATION, 2): (["u"], ["u"], ["f_1", "f_2", "df_1", "df_2"], []),
    (capi.EQ_SCALAR_CONSERVATION, 3): (["u"], ["u"], ["f_1", "f_2", "f_3", "df_1", "df_2", "df_3"], []),
}


@pytest.fixture(scope="module")
def checker():
    src = os.path.join(ROOT, "tests", "cpp", "output_selection_cases.cc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ryujin_amd", "csrc"), src,
                    "-o", BIN], check=True)
    return BIN


def _run(checker, *args):
    out = subprocess.run([checker, *map(str, args)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    return json.loads(out.stdout)


def _expected(equation, dim, name, postprocess_names=()):
    """SelectedComponentsExtractor::extract (:77-88), then the postprocessed names"""
    tables = REFERENCE[equation, dim]
    for kind, names in enumerate(tables):
        if name in names:
            return kind, names.index(name)
    if name == "alpha":
        return ALPHA, 0
    if name in postprocess_names:
        return POSTPROCESSED, list(postprocess_names).index(name)
    return None


# ------------------------------------------------------------------------------------------------ names

@pytest.mark.parametrize("equation,dim", sorted(REFERENCE))
def test_name_tables_are_the_references(checker, equation, dim):
    got = _run(checker, "names", equation, dim)
    conserved, primitive, precomputed, initial = REFERENCE[equation, dim]
    assert got == dict(conserved=conserved, primitive=primitive, precomputed=precomputed, initial_precomputed=initial)
    if (equation, dim) != (capi.EQ_SHALLOW_WATER, 3):
        # the Python twin of the tables (capi.output_names) and the component names the package already had
        assert {k: list(v) for k, v in capi.output_names(equation, dim).items()} == got
        assert capi.component_names(equation, dim) == (tuple(conserved), tuple(primitive))


@pytest.mark.parametrize("equation,dim", sorted(REFERENCE))
def test_every_name_resolves_to_kind_and_index(checker, equation, dim):
    seen = []
    for names in REFERENCE[equation, dim]:
        seen += [n for n in names if n not in seen]
    for name in seen + ["alpha"]:
        got = _run(checker, "resolve", equation, dim, "-", name)
        assert got["ok"] and (got["kind"], got["index"]) == _expected(equation, dim, name), (name, got)


def test_duplicates_between_conserved_and_primitive_go_to_conserved(checker):
    for equation, dim, name in ((capi.EQ_EULER, 2, "rho"), (capi.EQ_EULER_AEOS, 3, "rho"),
                                (capi.EQ_SHALLOW_WATER, 2, "h"), (capi.EQ_SCALAR_CONSERVATION, 1, "u")):
        assert name in REFERENCE[equation, dim][0] and name in REFERENCE[equation, dim][1]
        got = _run(checker, "resolve", equation, dim, "-", name)
        assert got["ok"] and (got["kind"], got["index"]) == (CONSERVED, 0)
    # "p" is primitive for Euler and precomputed for EulerAEOS; "e" primitive for EulerAEOS only
    assert _run(checker, "resolve", capi.EQ_EULER, 2, "-", "p")["kind"] == PRIMITIVE
    assert _run(checker, "resolve", capi.EQ_EULER_AEOS, 2, "-", "p")["kind"] == PRECOMPUTED
    assert _run(checker, "resolve", capi.EQ_EULER_AEOS, 2, "-", "e")["kind"] == PRIMITIVE
    assert not _run(checker, "resolve", capi.EQ_EULER, 2, "-", "e")["ok"]


@pytest.mark.parametrize("name", ["pressure", "Rho", "m_3", "", "alpha ", "schlieren_rho", "t"])
def test_unknown_names_are_refused_with_the_references_message(checker, name):
    got = _run(checker, "resolve", capi.EQ_EULER, 2, "-", name)
    assert not got["ok"]
    assert got["error"] == ("Invalid component name: \"" + name + "\" is not a valid "
                            "conserved/primitive/precomputed/initial component name.")


def test_alpha_and_bathymetry(checker):
    for equation, dim in sorted(REFERENCE):
        got = _run(checker, "resolve", equation, dim, "-", "alpha")
        assert got["ok"] and (got["kind"], got["index"]) == (ALPHA, 0)
        got = _run(checker, "resolve", equation, dim, "-", "bathymetry")
        if equation == capi.EQ_SHALLOW_WATER:
            assert got["ok"] and (got["kind"], got["index"]) == (INITIAL, 0)
        else:
            assert not got["ok"] and "bathymetry" in got["error"]


def test_postprocessed_names_are_formed_as_the_postprocessor_forms_them(checker):
    # (kind, is_primitive, component): schlieren of rho, vorticity of v_1, schlieren of the pressure, of E
    pp = "0:0:0,1:1:1,0:1:3,0:0:3"
    names = ["schlieren_rho", "vorticity_v_1", "schlieren_p", "schlieren_E"]
    got = _run(checker, "resolve", capi.EQ_EULER, 2, pp, "vorticity_v_1")
    assert got["postprocess_names"] == names
    assert got["ok"] and (got["kind"], got["index"]) == (POSTPROCESSED, 1)
    # the names of Python's postprocess_configure are the same rule
    for q, (kind, is_primitive, component) in enumerate(((0, 0, 0), (1, 1, 1), (0, 1, 3), (0, 0, 3))):
        base = capi.component_names(capi.EQ_EULER, 2)[is_primitive][component]
        assert names[q] == ("schlieren_" if kind == 0 else "vorticity_") + base
    # a state name wins over a postprocessed one; a name that is not configured is unknown
    assert _run(checker, "resolve", capi.EQ_EULER, 2, pp, "rho")["kind"] == CONSERVED
    assert not _run(checker, "resolve", capi.EQ_EULER, 2, pp, "schlieren_m_1")["ok"]
    assert _run(checker, "resolve", capi.EQ_EULER, 2, pp, "schlieren_E")["index"] == 3
    # a quantity outside the state has no name
    assert _run(checker, "resolve", capi.EQ_EULER, 2, "0:0:7", "alpha")["postprocess_names"] == [""]


# ------------------------------------------------------------------------------------------------ the cell rule

def _bits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def _cell(checker, *manifolds):
    values = [v for m in manifolds for v in m]
    return _run(checker, "cell", len(manifolds), len(manifolds[0]), *map(_bits, values))["selected"]


def _rule(*manifolds):
    """vtu_output.template.h:171-187, restated with numpy"""
    for f in manifolds:
        f = np.asarray(f, dtype=np.float64)
        if (f >= 0.0 - 100.0 * EPS).any() and (f <= 0.0 + 100.0 * EPS).any():
            return True
    return False


CELLS = {
    "all above": ([1.0, 2.0, 3.0, 0.5], False),
    "all below": ([-1.0, -2.0, -3.0, -0.5], False),
    "straddling": ([-1.0, 2.0, 3.0, 0.5], True),
    "straddling, last vertex": ([1.0, 2.0, 3.0, -0.5], True),
    "one vertex on the level set": ([0.0, 2.0, 3.0, 0.5], True),   # both counters rise on the same vertex
    "+100 eps counts as below": ([100.0 * EPS, 1.0], True),
    "+101 eps does not": ([101.0 * EPS, 1.0], False),
    "-100 eps counts as above": ([-100.0 * EPS, -1.0], True),
    "-101 eps does not": ([-101.0 * EPS, -1.0], False),
    "next after +100 eps": ([np.nextafter(100.0 * EPS, 1.0), 1.0], False),
    "next after -100 eps": ([np.nextafter(-100.0 * EPS, -1.0), -1.0], False),
    "+0.0": ([0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], True),
    "-0.0": ([-0.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0], True),
    "NaN everywhere": ([np.nan, np.nan, np.nan, np.nan], False),
    "NaN next to one side": ([np.nan, 1.0, 2.0, np.nan], False),
    "NaN next to both sides": ([np.nan, 1.0, -2.0, np.nan], True),
    "infinities": ([np.inf, -np.inf], True),
}


@pytest.mark.parametrize("case", sorted(CELLS))
def test_cell_rule_on_hand_made_vertex_values(checker, case):
    values, expected = CELLS[case]
    assert _rule(values) == expected, "the restatement and the table agree"
    assert _cell(checker, values) == expected


def test_cell_rule_with_two_manifolds(checker):
    above, cut, nan = [1.0, 2.0, 3.0, 4.0], [1.0, -2.0, 3.0, 4.0], [np.nan] * 4
    assert _cell(checker, above, cut) is True          # only the second cuts
    assert _cell(checker, cut, above) is True
    assert _cell(checker, above, above) is False
    assert _cell(checker, nan, cut) is True
    # above of one manifold and below of ANOTHER do not combine
    assert _cell(checker, above, [-v for v in above]) is False
    assert _rule(above, [-v for v in above]) is False
    rng = np.random.default_rng(5)
    for _ in range(40):
        f = rng.normal(size=(3, 8)) + rng.choice([-1.5, 0.0, 1.5], size=(3, 1))
        assert _cell(checker, *f.tolist()) == _rule(*f)


# ------------------------------------------------------------------------------------------------ the compaction plan

def _compact(checker, flags, tmp_path, block=BLOCK):
    path = tmp_path / "flags.txt"
    path.write_text("".join("1" if f else "0" for f in flags))
    return _run(checker, "compact", block, "@" + str(path))


def _check_compaction(got, flags, block):
    flags = np.asarray(flags, dtype=bool)
    n = len(flags)
    n_blocks = (n + block - 1) // block
    expected = np.flatnonzero(flags)
    counts = [int(flags[b * block:(b + 1) * block].sum()) for b in range(n_blocks)]
    assert got["n"] == n and got["n_blocks"] == n_blocks
    assert got["counts"] == counts
    assert got["offsets"] == [int(x) for x in np.concatenate(([0], np.cumsum(counts)))]
    assert got["total"] == got["length"] == len(expected)
    assert np.array_equal(np.array(got["list"], dtype=np.int64), expected)
    position = np.full(n, 0xffffffff, dtype=np.int64)
    position[expected] = np.arange(len(expected))
    assert np.array_equal(np.array(got["map"], dtype=np.int64), position)


LENGTHS = [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, BLOCK * BLOCK + BLOCK + 7]


@pytest.mark.parametrize("n", LENGTHS)
def test_compaction_plan_against_flatnonzero(checker, tmp_path, n):
    rng = np.random.default_rng(n)
    for flags in (rng.random(n) < 0.3, np.ones(n, dtype=bool), np.zeros(n, dtype=bool)):
        _check_compaction(_compact(checker, flags, tmp_path), flags, BLOCK)


def test_compaction_plan_with_a_small_block(checker, tmp_path):
    """more than (block size)^2 items at a block of 4: every boundary case of the offsets in a short list"""
    rng = np.random.default_rng(11)
    for n in (0, 1, 3, 4, 5, 17, 23):
        flags = rng.random(n) < 0.5
        _check_compaction(_compact(checker, flags, tmp_path, block=4), flags, 4)


def test_symbols_and_limits_are_declared():
    for name in ("configure", "info", "selection", "levelset_values", "extract"):
        assert "ryujin_hip_output_" + name in capi.HIP_SYMBOLS
    header = open(os.path.join(ROOT, "include", "ryujin_hip.h")).read()
    assert f"#define RYUJIN_OUT_MAX_QUANTITIES {capi.OUT_MAX_QUANTITIES}" in header
    assert f"#define RYUJIN_OUT_MAX_MANIFOLDS {capi.OUT_MAX_MANIFOLDS}" in header
