"""CPU: the host side of the QHD run monitor -- foamfile.read_qhd_functions, the writers of the QHD applications, monitor.unpack_qhd on a
synthetic block and monitor.combine of QHD parts; read_functions keeps serving QGDFoam as before."""
import os

import numpy as np

import qgdsolver_amd as q
from qgdsolver_amd import foamfile as ff
from qgdsolver_amd import monitor as mon

from test_monitor_host import FUNCTIONS

QHD_FUNCTIONS = """
application QHDFoam; deltaT 1e-3;
functions
{
    points     { type probes; fields (p U T rho); probeLocations ((0.1 0.2 0.3) (0.5 0.5 0.5)); writeControl timeStep; writeInterval 5; }
    extremes   { type fieldMinMax; fields (U T p contErr Mach); }
    budget     { type qhdIntegrals; writeInterval 2; }
    walls      { type qhdPatchFluxes; patches (hot cold); writeInterval 3; }
    nowhere    { type qhdPatchFluxes; writeInterval 3; }
    continuity { type qhdContinuityErrors; }
    mass       { type qgdIntegrals; }
    drag       { type forces; patches (hot); }
    later      { type qhdIntegrals; writeControl runTime; writeInterval 0.5; }
    off        { type qhdContinuityErrors; enabled false; }
}
"""


def test_qhd_functions_text_parses_to_the_specifications():
    warnings = []
    specs = ff.read_qhd_functions(ff.parse_foam_text(QHD_FUNCTIONS), warn=warnings.append)
    assert [s["name"] for s in specs] == ["points", "extremes", "budget", "walls", "continuity"]
    points, extremes, budget, walls, continuity = specs
    assert points["type"] == "probes" and points["interval"] == 5 and points["fields"] == ["p", "U", "T"]
    assert np.array_equal(points["probeLocations"], [[0.1, 0.2, 0.3], [0.5, 0.5, 0.5]])
    assert extremes == dict(name="extremes", type="fieldMinMax", interval=1, fields=["U", "T", "p", "contErr"])
    assert budget == dict(name="budget", type="qhdIntegrals", interval=2)
    assert walls == dict(name="walls", type="qhdPatchFluxes", interval=3, patches=["hot", "cold"])
    assert continuity == dict(name="continuity", type="qhdContinuityErrors", interval=1)
    # one line each, naming what is skipped: rho at the probes, Mach, the missing patches, QGDFoam's type, the unknown type, runTime
    assert len(warnings) == 6, warnings
    assert any("'points'" in w and "'rho'" in w for w in warnings) and any("'extremes'" in w and "'Mach'" in w for w in warnings)
    assert any("'nowhere'" in w and "no patches" in w for w in warnings)
    assert any("'mass'" in w and "'qgdIntegrals'" in w and "skipped" in w for w in warnings)
    assert any("'drag'" in w and "'forces'" in w and "skipped" in w for w in warnings)
    assert any("'later'" in w and "runTime" in w for w in warnings)
    assert ff.read_qhd_functions(ff.parse_foam_text("deltaT 1;")) == []


def test_read_functions_gives_what_it_gave():
    warnings = []
    specs = ff.read_functions(ff.parse_foam_text(FUNCTIONS), warn=warnings.append)
    assert [s["name"] for s in specs] == ["wake", "extremes", "budget", "outlet"]
    wake, extremes, budget, outlet = specs
    assert wake["type"] == "probes" and wake["interval"] == 5 and wake["fields"] == ["p", "U", "T", "rho", "e"]
    assert np.array_equal(wake["probeLocations"], [[0.1, 0.2, 0.3], [0.5, 0.5, 0.5]]) and set(wake) == {"name", "type", "interval", "fields", "probeLocations"}
    assert extremes == dict(name="extremes", type="fieldMinMax", interval=1, fields=["p", "U", "Mach"])
    assert budget == dict(name="budget", type="qgdIntegrals", interval=2)
    assert outlet == dict(name="outlet", type="qgdPatchFluxes", interval=3, patches=["outlet", "inlet"])
    assert len(warnings) == 3 and any("served: probes, fieldMinMax, qgdIntegrals, qgdPatchFluxes, qgdSpeciesIntegrals, qgdSpeciesPatchFluxes" in w for w in warnings)
    # a QHD type is not one of QGDFoam's
    w2 = []
    assert ff.read_functions(ff.parse_foam_text("functions { c { type qhdContinuityErrors; } }"), warn=w2.append) == [] and len(w2) == 1


def _block(seed, n_probes=3, n_patches=2, state=1, flags=0, owned=10, bad=0):
    """a synthetic result block of the QHD layout and its offsets"""
    rng = np.random.default_rng(seed)
    off = [0, 8, 20, 36, 36 + 5 * n_probes]
    raw = rng.standard_normal(off[4] + 9 * n_patches)
    raw[0:8] = [owned, state, n_probes, n_patches, bad, 4 if bad else -1, 2e-3, flags]
    raw[8] = 1.0 + rng.random()                                   # the volume
    raw[off[2]:off[3]].reshape(4, 4)[:, [1, 3]] = rng.integers(0, 24, (4, 2))
    return raw, off


def test_unpack_qhd_names_the_sections_of_a_block():
    raw, off = _block(7, flags=3, bad=2)
    s = mon.unpack_qhd(raw, off, 0.25, 12)
    assert s["kind"] == "qhd" and s["time"] == 0.25 and s["step"] == 12 and s["deltaT"] == 2e-3 and s["ownedCells"] == 10 and s["fluxState"] == 1
    assert s["nonFinite"] == 2 and s["firstNonFinite"] == 4 and s["rotating"] and s["frozenT"]
    assert np.array_equal(s["integrals"], raw[8:20]) and len(mon.QHD_INTEGRALS) == 12
    assert s["volume"] == raw[8] and np.array_equal(s["momentum"], raw[9:12]) and np.array_equal(s["bodyForce"], raw[15:18])
    assert s["continuityGlobal"] == raw[18] and s["continuityLocal"] == raw[19]
    ex = raw[20:36].reshape(4, 4)
    assert np.array_equal(s["min"], ex[:, 0]) and np.array_equal(s["minCell"], ex[:, 1]) and np.array_equal(s["max"], ex[:, 2]) and np.array_equal(s["maxCell"], ex[:, 3])
    assert s["minCell"].dtype == np.int64 and len(mon.QHD_EXTREMA_FIELDS) == 4
    assert np.array_equal(s["probes"], raw[36:51].reshape(3, 5)) and len(mon.QHD_PROBE_COLUMNS) == 5
    pa = raw[51:69].reshape(2, 9)
    assert np.array_equal(s["patchArea"], pa[:, 0]) and np.array_equal(s["patchFlux"], pa[:, 1:6]) and np.array_equal(s["patchPressureForce"], pa[:, 6:9])
    assert len(mon.QHD_PATCH_COLUMNS) == 9
    s0 = mon.unpack_qhd(_block(8, flags=1)[0], off, 0.0, 0)
    assert s0["rotating"] and not s0["frozenT"]
    local, glob = mon.continuity_errors(s)
    assert local == (2e-3 / raw[8]) * raw[19] and glob == (2e-3 / raw[8]) * raw[18]


def test_combine_three_qhd_parts():
    parts = []
    for k in range(3):
        raw, off = _block(20 + k, owned=10 + k, bad=1 if k == 1 else 0)
        s = mon.unpack_qhd(raw, off, 0.5, 3)
        s.pop("raw")
        parts.append(s)
    a, b, c = parts
    a["probes"][1:] = np.nan          # every part holds one of the three probes
    b["probes"][[0, 2]] = np.nan
    c["probes"][:2] = np.nan
    a["min"][0], a["minCell"][0], b["min"][0], b["minCell"][0], c["min"][0], c["minCell"][0] = 1.0, 7, 1.0, 3, 1.5, 1      # a tie: the lowest label
    a["max"][3], a["maxCell"][3] = np.nan, -1                                                                          # part 0 saw no finite value
    keep = [{k: np.copy(v) for k, v in p.items()} for p in parts]
    t = mon.combine(parts)
    assert t["kind"] == "qhd" and t["ownedCells"] == 33 and t["nonFinite"] == 1 and t["firstNonFinite"] == 4 and t["fluxState"] == 1 and "raw" not in t
    for key in ("integrals", "momentum", "patchArea", "patchFlux", "patchPressureForce"):
        assert np.array_equal(t[key], (keep[0][key] + keep[1][key]) + keep[2][key]), key
    assert t["volume"] == t["integrals"][0] and np.array_equal(t["momentum"], t["integrals"][1:4]) and np.array_equal(t["bodyForce"], t["integrals"][7:10])
    assert t["continuityGlobal"] == t["integrals"][10] and t["continuityLocal"] == t["integrals"][11]
    assert t["minCell"][0] == 3 and t["min"][0] == 1.0
    assert t["max"][3] == max(keep[1]["max"][3], keep[2]["max"][3])
    for k in range(1, 4):
        assert t["min"][k] == min(p["min"][k] for p in keep)
    assert np.array_equal(t["probes"][0], keep[0]["probes"][0]) and np.array_equal(t["probes"][1], keep[1]["probes"][1]) and np.array_equal(t["probes"][2], keep[2]["probes"][2])
    for p, k in zip(parts, keep):                                  # the parts are left as they were
        assert all(np.array_equal(p[key], k[key], equal_nan=True) for key in p if isinstance(p[key], np.ndarray))
    one = mon.combine(parts[:1])
    assert one["ownedCells"] == 10 and np.array_equal(one["integrals"], keep[0]["integrals"])


def _table(path):
    return np.atleast_2d(np.loadtxt(path, comments="#"))


def test_qhd_writers_files_parse_back_to_the_numbers(tmp_path):
    mesh = q.PolyMesh.box(4, 3, 2)
    centres = mesh.array("C").reshape(-1, 3)
    file_label = np.arange(mesh.nCells)[::-1]        # device label c is cell 23 - c of the case files
    samples = []
    for k in range(3):
        raw, off = _block(40 + k, bad=k % 2, flags=2 if k == 2 else 0)
        s = mon.unpack_qhd(raw, off, 0.0, k)
        if k == 2:
            s["patchFlux"][:, 4] = np.nan          # a frozen T has no flux
        samples.append((0.001 * (k + 1), s))
    locs = np.array([[0.1, 0.2, 0.3], [0.5, 0.5, 0.5], [7.0, 7.0, 7.0]])
    d = str(tmp_path)
    pw = mon.QHDProbesWriter(d, dict(fields=["p", "U", "T"], probeLocations=locs), found=[True, True, False])
    mw = mon.QHDFieldMinMaxWriter(d, dict(fields=["T", "U", "contErr", "p"]), centres, file_label)
    iw = mon.QHDIntegralsWriter(d, {}, file_label)
    fw = mon.QHDPatchFluxWriter(d, dict(patches=["cold", "hot"]), rows=[1, 0])
    cw = mon.ContinuityErrorsWriter(d, {}, file_label)
    for t, s in samples:
        for w in (pw, mw, iw, fw, cw):
            w.write(t, s)

    text = open(os.path.join(d, "U")).read().splitlines()
    assert text[0].startswith("# Probe 0 (0.1") and text[2].endswith("# Not Found") and text[3] == "# Probe 0 1 2" and text[4] == "# Time"
    for name, cols in (("p", [4]), ("T", [3]), ("U", [0, 1, 2])):
        rows = np.array([[float(x) for x in line.replace("(", " ").replace(")", " ").split()]
                         for line in open(os.path.join(d, name)).read().splitlines() if not line.startswith("#")])
        assert rows.shape == (3, 1 + 3 * len(cols))
        for r, (t, s) in zip(rows, samples):
            assert r[0] == t and np.array_equal(r[1:], s["probes"][:, cols].reshape(-1))

    rows = _table(os.path.join(d, "fieldMinMax.dat"))
    assert rows.shape == (3, 1 + 4 * 10)
    head = open(os.path.join(d, "fieldMinMax.dat")).read().splitlines()[1].split("\t")
    assert head[1] == "min(T)" and head[11] == "min(mag(U))" and head[21] == "min(contErr)"
    for r, (t, s) in zip(rows, samples):
        assert r[0] == t
        for j, k in enumerate((1, 0, 3, 2)):               # T, mag(U), contErr, p of QHD_EXTREMA_FIELDS
            blk = r[1 + 10 * j:11 + 10 * j]
            assert blk[0] == s["min"][k] and blk[1] == file_label[s["minCell"][k]] and np.array_equal(blk[2:5], centres[s["minCell"][k]])
            assert blk[5] == s["max"][k] and blk[6] == file_label[s["maxCell"][k]] and np.array_equal(blk[7:10], centres[s["maxCell"][k]])

    rows = _table(os.path.join(d, "volIntegrals.dat"))
    assert rows.shape == (3, 15)
    head = open(os.path.join(d, "volIntegrals.dat")).read().splitlines()[1].split("\t")
    assert head[1:13] == list(mon.QHD_INTEGRALS) and head[11] == "continuityGlobal"
    for r, (t, s) in zip(rows, samples):
        assert r[0] == t and np.array_equal(r[1:13], s["integrals"]) and r[13] == s["nonFinite"]
        assert r[14] == (file_label[4] if s["nonFinite"] else -1)

    rows = _table(os.path.join(d, "patchFluxes.dat"))
    assert rows.shape == (3, 19)
    head = open(os.path.join(d, "patchFluxes.dat")).read().splitlines()[1].split("\t")
    assert head[1] == "cold:area" and head[10] == "hot:area" and head[2] == "cold:volumetricFlux" and head[6] == "cold:TFlux"
    for r, (t, s) in zip(rows, samples):
        assert r[0] == t
        for j, p in enumerate((1, 0)):
            blk = r[1 + 9 * j:10 + 9 * j]
            assert blk[0] == s["patchArea"][p] and np.array_equal(blk[1:6], s["patchFlux"][p], equal_nan=True) and np.array_equal(blk[6:9], s["patchPressureForce"][p])
    assert np.isnan(rows[2, 6]) and not np.isnan(rows[1, 6])            # cold:TFlux

    rows = _table(os.path.join(d, "continuityErrors.dat"))
    assert rows.shape == (3, 6)
    cumulative = 0.0
    for r, (t, s) in zip(rows, samples):
        local, glob = s["deltaT"] / s["volume"] * s["continuityLocal"], s["deltaT"] / s["volume"] * s["continuityGlobal"]
        cumulative += glob
        assert r[0] == t and r[1] == local and r[2] == glob and r[3] == cumulative and r[4] == s["max"][3] and r[5] == file_label[s["maxCell"][3]]
