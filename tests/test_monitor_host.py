"""CPU: the host side of the run monitors -- PolyMesh.find_cells, the functions{} reader and the four writers."""
import os

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import foamfile as ff
from qgdsolver_amd import monitor as mon
from util import make_mesh


def _mesh(kind):
    return q.PolyMesh.box(4, 3, 2) if kind == "box432" else make_mesh(kind)


@pytest.mark.parametrize("kind", ["box432", "box654_jitter", "box654_poly", "plane2d_jitter"])
def test_find_cells_centres_map_to_their_own_cell(kind):
    mesh = _mesh(kind)
    C = mesh.array("C").reshape(-1, 3)
    assert np.array_equal(mesh.find_cells(C), np.arange(mesh.nCells))


@pytest.mark.parametrize("kind", ["box432", "box654_poly", "plane2d_jitter"])
def test_find_cells_outside_is_minus_one(kind):
    mesh = _mesh(kind)
    pts = mesh.array("points").reshape(-1, 3)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    mid = 0.5 * (lo + hi)
    outside = [mid + (hi - lo) * np.array(d) for d in ((0.6, 0, 0), (-0.6, 0, 0), (0, 0.6, 0), (0, 0, -0.6), (0, 0, 0.51), (5, 5, 5))]
    assert np.array_equal(mesh.find_cells(outside), -np.ones(len(outside), dtype=np.int64))
    assert mesh.find_cells([mid])[0] >= 0


def test_find_cells_shared_face_edge_and_vertex_go_to_the_lowest_label():
    mesh = q.PolyMesh.box(4, 3, 2)   # cell (i, j, k) has label i + 4 j + 12 k; dx = 1/4, dy = 1/3, dz = 1/2
    # the face between cells 1 and 2; the edge shared by cells 5, 6, 9, 10; the vertex shared by 5, 6, 9, 10, 17, 18, 21, 22
    pts = [(0.5, 1 / 6, 0.25), (0.5, 2 / 3, 0.25), (0.5, 2 / 3, 0.5)]
    assert list(mesh.find_cells(pts)) == [1, 5, 5]
    # a face of the boundary belongs to the mesh
    assert mesh.find_cells([(0.0, 0.1, 0.1)])[0] == 0 and mesh.find_cells([(1.0, 0.9, 0.9)])[0] == 23
    # the face of a jittered mesh: its centre is on the plane both neighbours are tested against
    jm = make_mesh("box654_jitter")
    own, nei, Cf = jm.array("owner"), jm.array("neighbour"), jm.array("Cf").reshape(-1, 3)
    f = nei.size // 2
    assert jm.find_cells([Cf[f]])[0] == min(own[f], nei[f])


FUNCTIONS = """
application QGDFoam; deltaT 1e-3;
functions
{
    wake      { type probes; libs ("libsampling.so"); fields (p U T rho e k); probeLocations ((0.1 0.2 0.3) (0.5 0.5 0.5));
                writeControl timeStep; writeInterval 5; }
    extremes  { type fieldMinMax; fields (p U Mach); }
    budget    { type qgdIntegrals; writeInterval 2; }
    outlet    { type qgdPatchFluxes; patches (outlet inlet); writeControl timeStep; writeInterval 3; }
    drag      { type forces; patches (wall); }
    later     { type qgdIntegrals; writeControl runTime; writeInterval 0.5; }
    off       { type qgdIntegrals; enabled false; }
}
"""


def test_functions_text_parses_to_the_specifications():
    warnings = []
    specs = ff.read_functions(ff.parse_foam_text(FUNCTIONS), warn=warnings.append)
    assert [s["name"] for s in specs] == ["wake", "extremes", "budget", "outlet"]
    wake, extremes, budget, outlet = specs
    assert wake["type"] == "probes" and wake["interval"] == 5 and wake["fields"] == ["p", "U", "T", "rho", "e"]
    assert np.array_equal(wake["probeLocations"], [[0.1, 0.2, 0.3], [0.5, 0.5, 0.5]])
    assert extremes == dict(name="extremes", type="fieldMinMax", interval=1, fields=["p", "U", "Mach"])
    assert budget == dict(name="budget", type="qgdIntegrals", interval=2)
    assert outlet == dict(name="outlet", type="qgdPatchFluxes", interval=3, patches=["outlet", "inlet"])
    # one line each: the unknown type, the field probes does not serve, the writeControl that is not timeStep
    assert len(warnings) == 3
    assert any("'drag'" in w and "'forces'" in w and "skipped" in w for w in warnings)
    assert any("'wake'" in w and "'k'" in w for w in warnings)
    assert any("'later'" in w and "runTime" in w for w in warnings)
    assert ff.read_functions(ff.parse_foam_text("deltaT 1;")) == []


def _sample(seed, n_probes=3, n_patches=2):
    rng = np.random.default_rng(seed)
    integ = rng.standard_normal(8)
    return dict(time=0.0, step=seed, nonFinite=seed % 2, firstNonFinite=4 if seed % 2 else -1, integrals=integ,
                min=rng.standard_normal(5), minCell=rng.integers(0, 24, 5), max=rng.standard_normal(5), maxCell=rng.integers(0, 24, 5),
                probes=rng.standard_normal((n_probes, 7)), patchArea=rng.random(n_patches), patchFlux=rng.standard_normal((n_patches, 5)),
                patchPressureForce=rng.standard_normal((n_patches, 3)))


def _table(path):
    return np.atleast_2d(np.loadtxt(path, comments="#"))


def test_writers_files_parse_back_to_the_numbers(tmp_path):
    mesh = q.PolyMesh.box(4, 3, 2)
    centres = mesh.array("C").reshape(-1, 3)
    file_label = np.arange(mesh.nCells)[::-1]        # a relabelled run: device label c is cell 23 - c of the case files
    samples = [(0.001 * (k + 1), _sample(k)) for k in range(3)]
    locs = np.array([[0.1, 0.2, 0.3], [0.5, 0.5, 0.5], [7.0, 7.0, 7.0]])
    d = str(tmp_path)
    pw = mon.ProbesWriter(d, dict(fields=["p", "U", "rho", "T", "e"], probeLocations=locs), found=[True, True, False])
    mw = mon.FieldMinMaxWriter(d, dict(fields=["rho", "U", "Mach"]), centres, file_label)
    iw = mon.IntegralsWriter(d, {}, file_label)
    fw = mon.PatchFluxWriter(d, dict(patches=["outlet", "inlet"]), rows=[1, 0])
    for t, s in samples:
        for w in (pw, mw, iw, fw):
            w.write(t, s)

    # probes: OpenFOAM's header, then time + one value per probe (a vector in parentheses)
    text = open(os.path.join(d, "U")).read().splitlines()
    assert text[0].startswith("# Probe 0 (0.1") and text[2].endswith("# Not Found") and text[3] == "# Probe 0 1 2" and text[4] == "# Time"
    for name, cols in (("p", [4]), ("rho", [0]), ("T", [5]), ("e", [6]), ("U", [1, 2, 3])):
        rows = np.array([[float(x) for x in line.replace("(", " ").replace(")", " ").split()]
                         for line in open(os.path.join(d, name)).read().splitlines() if not line.startswith("#")])
        assert rows.shape == (3, 1 + 3 * len(cols))
        for r, (t, s) in zip(rows, samples):
            assert r[0] == t and np.array_equal(r[1:], s["probes"][:, cols].reshape(-1))

    rows = _table(os.path.join(d, "fieldMinMax.dat"))
    assert rows.shape == (3, 1 + 3 * 10)
    for r, (t, s) in zip(rows, samples):
        assert r[0] == t
        for j, k in enumerate((0, 3, 4)):                  # rho, mag(U), Mach of EXTREMA_FIELDS
            blk = r[1 + 10 * j:11 + 10 * j]
            assert blk[0] == s["min"][k] and blk[1] == file_label[s["minCell"][k]] and np.array_equal(blk[2:5], centres[s["minCell"][k]])
            assert blk[5] == s["max"][k] and blk[6] == file_label[s["maxCell"][k]] and np.array_equal(blk[7:10], centres[s["maxCell"][k]])

    rows = _table(os.path.join(d, "volIntegrals.dat"))
    assert rows.shape == (3, 11)
    for r, (t, s) in zip(rows, samples):
        assert r[0] == t and np.array_equal(r[1:9], s["integrals"]) and r[9] == s["nonFinite"]
        assert r[10] == (file_label[4] if s["nonFinite"] else -1)

    rows = _table(os.path.join(d, "patchFluxes.dat"))
    assert rows.shape == (3, 19)
    head = open(os.path.join(d, "patchFluxes.dat")).read().splitlines()[1].split("\t")
    assert head[1] == "outlet:area" and head[10] == "inlet:area" and head[2] == "outlet:massFlux"
    for r, (t, s) in zip(rows, samples):
        assert r[0] == t
        for j, p in enumerate((1, 0)):
            blk = r[1 + 9 * j:10 + 9 * j]
            assert blk[0] == s["patchArea"][p] and np.array_equal(blk[1:6], s["patchFlux"][p]) and np.array_equal(blk[6:9], s["patchPressureForce"][p])


def test_combine_ranks():
    a, b = _sample(1), _sample(2)
    a.update(ownedCells=10, volume=0, mass=0, momentum=a["integrals"][2:5], totalEnergy=0, internalEnergy=0, kineticEnergy=0)
    b.update(ownedCells=14, volume=0, mass=0, momentum=b["integrals"][2:5], totalEnergy=0, internalEnergy=0, kineticEnergy=0)
    a["probes"][1] = np.nan          # rank 0 does not hold probe 1, rank 1 does not hold probes 0 and 2
    b["probes"][[0, 2]] = np.nan
    a["min"][0], a["minCell"][0], b["min"][0], b["minCell"][0] = 1.0, 7, 1.0, 3      # a tie: the lowest label
    a["max"][1], a["maxCell"][1] = np.nan, -1                                        # rank 0 saw no finite value
    c = mon.combine([a, b])
    assert c["ownedCells"] == 24 and c["nonFinite"] == 1 and c["firstNonFinite"] == 4
    assert np.array_equal(c["integrals"], a["integrals"] + b["integrals"]) and c["mass"] == c["integrals"][1]
    assert np.array_equal(c["patchFlux"], a["patchFlux"] + b["patchFlux"])
    assert c["minCell"][0] == 3 and c["max"][1] == b["max"][1] and c["maxCell"][1] == b["maxCell"][1]
    for k in range(5):
        assert c["min"][k] == min(a["min"][k], b["min"][k])
    assert np.array_equal(c["probes"][[0, 2]], a["probes"][[0, 2]]) and np.array_equal(c["probes"][1], b["probes"][1])
