"""CPU: the host side of the species block of the run monitors -- unpack_species on a synthetic block, combine() on synthetic parts, the
functions{} reader's acceptance and refusal of species names, the two species writers, and the agreement of header, binding and library
on the three new entries."""
import os
import re

import numpy as np
import pytest

from qgdsolver_amd import _lib as L
from qgdsolver_amd import foamfile as ff
from qgdsolver_amd import monitor as mon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def synthetic_block(nS, n_probes, n_patches, seed):
    """a species block in the layout of include/qgd_amd.h and its parts"""
    rng = np.random.default_rng(seed)
    off = [0, 8, 8 + nS, 8 + 5 * nS, 8 + 5 * nS + nS * n_probes]
    mass, ex = rng.standard_normal(nS), rng.standard_normal((nS, 4))
    ex[:, 1], ex[:, 3] = rng.integers(0, 1000, nS), rng.integers(0, 1000, nS)
    probes, patches = rng.standard_normal((n_probes, nS)), rng.standard_normal((n_patches, nS))
    raw = np.concatenate([[nS, 1, 2, 3, 17, 2.5e-16, n_probes, n_patches], mass, ex.reshape(-1), probes.reshape(-1), patches.reshape(-1)])
    return raw, off, mass, ex, probes, patches


@pytest.mark.parametrize("nS,n_probes,n_patches", [(2, 0, 0), (5, 3, 2), (32, 1, 6)])
def test_unpack_of_a_synthetic_species_block(nS, n_probes, n_patches):
    raw, off, mass, ex, probes, patches = synthetic_block(nS, n_probes, n_patches, 3)
    s = mon.unpack_species(raw, off)
    assert s["nSpecies"] == nS and s["speciesInert"] == 1 and s["speciesFluxState"] == 2
    assert s["speciesNonFinite"] == 3 and s["speciesFirstNonFinite"] == 17 and s["speciesSumDefect"] == 2.5e-16
    assert np.array_equal(s["speciesMass"], mass)
    assert np.array_equal(s["speciesMin"], ex[:, 0]) and np.array_equal(s["speciesMinCell"], ex[:, 1].astype(np.int64))
    assert np.array_equal(s["speciesMax"], ex[:, 2]) and np.array_equal(s["speciesMaxCell"], ex[:, 3].astype(np.int64))
    assert s["speciesMinCell"].dtype == np.int64
    assert s["speciesProbes"].shape == (n_probes, nS) and np.array_equal(s["speciesProbes"], probes)
    assert s["speciesPatchFlux"].shape == (n_patches, nS) and np.array_equal(s["speciesPatchFlux"], patches)
    raw[:] = 0.0                                   # the named arrays are copies
    assert np.array_equal(s["speciesMass"], mass) and s["speciesRaw"] is raw


def _flow_part(seed, n_probes):
    rng = np.random.default_rng(100 + seed)
    integ = rng.standard_normal(8)
    return dict(time=0.0, step=1, nonFinite=0, firstNonFinite=-1, integrals=integ, momentum=integ[2:5], volume=0, mass=0, totalEnergy=0,
                internalEnergy=0, kineticEnergy=0, ownedCells=10 + seed, fluxState=1,
                min=rng.standard_normal(5), minCell=rng.integers(0, 24, 5), max=rng.standard_normal(5), maxCell=rng.integers(0, 24, 5),
                probes=rng.standard_normal((n_probes, 7)), patchArea=rng.random(2), patchFlux=rng.standard_normal((2, 5)),
                patchPressureForce=rng.standard_normal((2, 3)))


def test_combine_merges_the_species_block_like_the_flow_block():
    nS = 5
    parts = []
    for seed in (1, 2, 3):
        raw, off, *_ = synthetic_block(nS, 3, 2, seed)
        parts.append(dict(_flow_part(seed, 3), **mon.unpack_species(raw, off)))
    a, b, c = parts
    a["speciesNonFinite"], a["speciesFirstNonFinite"] = 0, -1
    b["speciesNonFinite"], b["speciesFirstNonFinite"] = 2, 40
    c["speciesNonFinite"], c["speciesFirstNonFinite"] = 1, 12
    a["speciesSumDefect"], b["speciesSumDefect"], c["speciesSumDefect"] = 1e-16, float("nan"), 3e-16
    # probe 0 on rank 0, probe 1 on rank 2, probe 2 on no rank
    a["speciesProbes"][1:] = np.nan
    b["speciesProbes"][:] = np.nan
    c["speciesProbes"][[0, 2]] = np.nan
    # species 0: a tie of the minimum goes to the lowest label; species 1: rank 0 saw no finite value; species 2: the maximum on rank 1
    for p, cell in ((a, 70), (b, 30), (c, 50)):
        p["speciesMin"][0], p["speciesMinCell"][0] = -9.0, cell
    a["speciesMax"][1], a["speciesMaxCell"][1] = np.nan, -1
    b["speciesMax"][2] = 99.0
    want_probe = [a["speciesProbes"][0].copy(), c["speciesProbes"][1].copy()]
    tot = mon.combine(parts)
    assert np.array_equal(tot["speciesMass"], a["speciesMass"] + b["speciesMass"] + c["speciesMass"])
    assert np.array_equal(tot["speciesPatchFlux"], a["speciesPatchFlux"] + b["speciesPatchFlux"] + c["speciesPatchFlux"])
    assert tot["speciesNonFinite"] == 3 and tot["speciesFirstNonFinite"] == 12 and tot["speciesSumDefect"] == 3e-16
    assert tot["speciesMin"][0] == -9.0 and tot["speciesMinCell"][0] == 30
    assert tot["speciesMax"][1] == max(b["speciesMax"][1], c["speciesMax"][1]) and tot["speciesMaxCell"][1] >= 0
    assert tot["speciesMax"][2] == 99.0 and tot["speciesMaxCell"][2] == b["speciesMaxCell"][2]
    for k in range(nS):
        assert tot["speciesMin"][k] == min(p["speciesMin"][k] for p in parts)
    assert np.array_equal(tot["speciesProbes"][0], want_probe[0]) and np.array_equal(tot["speciesProbes"][1], want_probe[1])
    assert np.isnan(tot["speciesProbes"][2]).all()
    assert "speciesRaw" not in tot and tot["nSpecies"] == nS and tot["speciesFluxState"] == 2
    # the flow block next to it is merged as before
    assert np.array_equal(tot["integrals"], a["integrals"] + b["integrals"] + c["integrals"]) and tot["ownedCells"] == 36
    # parts without a species block: nothing of it appears
    flow_only = mon.combine([_flow_part(1, 3), _flow_part(2, 3)])
    assert not any(k.startswith("species") for k in flow_only)
    # one part: returned as it is
    assert mon.combine([a])["speciesMass"] is a["speciesMass"]


FUNCTIONS = """
application QGDFoam; deltaT 1e-3;
functions
{
    wake      { type probes; fields (p O2 U CO2); probeLocations ((0.1 0.2 0.3)); writeInterval 5; }
    extremes  { type fieldMinMax; fields (N2 Mach H2O); }
    budget    { type qgdSpeciesIntegrals; writeInterval 2; }
    ends      { type qgdSpeciesPatchFluxes; patches (outlet inlet); writeInterval 3; }
    nowhere   { type qgdSpeciesPatchFluxes; }
    flow      { type qgdIntegrals; }
}
"""


def test_functions_reader_takes_species_names_in_a_case_with_species():
    warnings = []
    specs = ff.read_functions(ff.parse_foam_text(FUNCTIONS), warn=warnings.append, species=["N2", "O2", "H2O"])
    assert [s["name"] for s in specs] == ["wake", "extremes", "budget", "ends", "flow"]
    wake, extremes, budget, ends, flow = specs
    assert wake["fields"] == ["p", "O2", "U"] and extremes["fields"] == ["N2", "Mach", "H2O"]
    assert budget == dict(name="budget", type="qgdSpeciesIntegrals", interval=2)
    assert ends == dict(name="ends", type="qgdSpeciesPatchFluxes", interval=3, patches=["outlet", "inlet"])
    assert flow == dict(name="flow", type="qgdIntegrals", interval=1)
    assert len(warnings) == 2
    assert any("'wake'" in w and "'CO2'" in w and "O2" in w.split("served:")[1] for w in warnings)      # the served list names the species
    assert any("'nowhere'" in w and "no patches" in w for w in warnings)


def test_functions_reader_refuses_species_in_a_case_without_species_by_name():
    cd = ff.parse_foam_text(FUNCTIONS)
    for typ in ("budget", "ends"):
        one = dict(cd, functions={typ: cd["functions"][typ]})
        with pytest.raises(ff.FoamFileError, match="needs a case with species") as ei:
            ff.read_functions(one, warn=lambda w: None)
        assert f"'{typ}'" in str(ei.value) and one["functions"][typ]["type"] in str(ei.value)
    # a species name among the fields is a field that is not served: named in a warning and left out, as any unknown field is
    warnings = []
    specs = ff.read_functions(dict(cd, functions={k: cd["functions"][k] for k in ("wake", "extremes", "flow")}), warn=warnings.append)
    assert [(s["name"], s.get("fields")) for s in specs] == [("wake", ["p", "U"]), ("extremes", ["Mach"]), ("flow", None)]
    assert sorted(w.split("field '")[1].split("'")[0] for w in warnings) == ["CO2", "H2O", "N2", "O2"]
    # what the reader gives for a case without species is what it gave before there were species to name
    flow_text = "functions { a { type probes; fields (p k); probeLocations ((0 0 0)); } b { type fieldMinMax; fields (T); } }"
    w1, w2 = [], []
    assert str(ff.read_functions(ff.parse_foam_text(flow_text), warn=w1.append)) == str(ff.read_functions(ff.parse_foam_text(flow_text), warn=w2.append, species=[]))
    assert w1 == w2 == ["functions: 'a': field 'k' is not served by type probes (served: rho, U, p, T, e): left out"]


class _Mesh:
    """what FunctionObjects asks of the file mesh before it creates the monitor"""
    patch_names = ["inlet", "outlet"]

    def find_cells(self, pts):
        return np.zeros(len(pts), dtype=np.int64)


def test_function_objects_refuse_a_species_name_the_case_does_not_carry():
    spec = [dict(name="wake", type="probes", interval=1, fields=["p", "O2"], probeLocations=np.zeros((1, 3)))]
    with pytest.raises(ValueError, match="'wake'.*'O2'.*neither a flow field nor a species"):
        mon.FunctionObjects(None, spec, _Mesh(), "/nonexistent", "0", lambda c: c, np.arange(4), species=["N2"])
    with pytest.raises(ValueError, match="'budget'.*qgdSpeciesIntegrals needs a case with species"):
        mon.FunctionObjects(None, [dict(name="budget", type="qgdSpeciesIntegrals", interval=1)], _Mesh(), "/nonexistent", "0", lambda c: c, np.arange(4))


def test_species_writers_files_parse_back_to_the_numbers(tmp_path):
    names = ["N2", "O2", "H2O"]
    file_label = np.arange(1000)[::-1]
    centres = np.random.default_rng(0).random((1000, 3))
    samples = []
    for k in range(3):
        raw, off, *_ = synthetic_block(3, 2, 2, 10 + k)
        s = mon.unpack_species(raw, off)
        s.update(probes=np.full((2, 7), 1.5 + k), min=np.arange(5.0), minCell=np.arange(5), max=np.arange(5.0) + 1, maxCell=np.arange(5) + 5)
        samples.append((1e-3 * (k + 1), s))
    d = str(tmp_path)
    locs = np.array([[0.1, 0.2, 0.3], [0.5, 0.5, 0.5]])
    pw = mon.ProbesWriter(d, dict(fields=["O2", "p"], probeLocations=locs), [True, True], names)
    mw = mon.FieldMinMaxWriter(d, dict(fields=["H2O", "p"]), centres, file_label, names)
    iw = mon.SpeciesIntegralsWriter(d, {}, file_label, names)
    fw = mon.SpeciesPatchFluxWriter(d, dict(patches=["outlet", "inlet"]), [1, 0], names)
    for t, s in samples:
        for w in (pw, mw, iw, fw):
            w.write(t, s)

    def table(name):
        return np.atleast_2d(np.loadtxt(os.path.join(d, name), comments="#"))

    rows = table("O2")
    assert open(os.path.join(d, "O2")).read().splitlines()[3] == "# Time"          # the probes layout, as for a flow scalar
    for r, (t, s) in zip(rows, samples):
        assert r[0] == t and np.array_equal(r[1:], s["speciesProbes"][:, 1])
    assert np.array_equal(table("p")[:, 1:], [[1.5, 1.5], [2.5, 2.5], [3.5, 3.5]])
    rows = table("fieldMinMax.dat")
    assert rows.shape == (3, 21)
    assert open(os.path.join(d, "fieldMinMax.dat")).read().splitlines()[1].split("\t")[1:3] == ["min(H2O)", "cell(min)"]
    for r, (t, s) in zip(rows, samples):
        lo, hi = s["speciesMinCell"][2], s["speciesMaxCell"][2]
        assert r[1] == s["speciesMin"][2] and r[2] == file_label[lo] and np.array_equal(r[3:6], centres[lo])
        assert r[6] == s["speciesMax"][2] and r[7] == file_label[hi] and np.array_equal(r[8:11], centres[hi])
        assert r[11] == 1.0 and r[12] == file_label[1]                              # p: row 1 of the flow block's extrema
    rows = table("speciesIntegrals.dat")
    assert rows.shape == (3, 7)
    for r, (t, s) in zip(rows, samples):
        assert r[0] == t and np.array_equal(r[1:4], s["speciesMass"]) and r[4] == 2.5e-16 and r[5] == 3 and r[6] == file_label[17]
    head = open(os.path.join(d, "speciesPatchFluxes.dat")).read().splitlines()[1].split("\t")
    assert head == ["# Time", "outlet:N2", "outlet:O2", "outlet:H2O", "inlet:N2", "inlet:O2", "inlet:H2O"]
    for r, (t, s) in zip(table("speciesPatchFluxes.dat"), samples):
        assert r[0] == t and np.array_equal(r[1:4], s["speciesPatchFlux"][1]) and np.array_equal(r[4:7], s["speciesPatchFlux"][0])


def test_header_binding_and_library_agree_on_the_new_entries():
    text = open(os.path.join(ROOT, "include", "qgd_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("qgd_monitor_enable_species", 1), ("qgd_monitor_species_layout", 3), ("qgd_monitor_species_read", 4)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, f"{name} is not declared in include/qgd_amd.h"
        assert len(m.group(1).split(",")) == n_args == len(L.SIGNATURES[name][1])
        assert hasattr(L.lib, name), f"libqgd_amd.so does not export {name}"
    assert L.ABI_VERSION == 9 and "#define QGD_MONITOR_SECTIONS 5" in text
    assert "monitors of species" not in text                   # the header no longer lists them as not served
