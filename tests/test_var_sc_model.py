"""CPU: the varScModel7 closure [varScModel7.C L166-300] -- the numpy restatement of its pressure-jump sensor (var_sc_ref.py, the
reference of the device tests) pinned by cases with known answers, and the case reader's side of the model."""
import os
import re

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L
from qgdsolver_amd import foamfile as ff

from test_foamfile import write_step_case
from util import make_mesh
from var_sc_ref import SensorGeometry, sensor

G, E = L.PATCH_GENERIC, L.PATCH_EMPTY


def zero_gradient_patch_values(mesh, p):
    return p[mesh.array("owner")[mesh.nInternalFaces:]]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["box654", "box654_jitter", "box654_poly", "plane2d_jitter", "step2d"])
def test_uniform_pressure_gives_zero(kind):
    mesh = make_mesh(kind)
    p = np.full(mesh.nCells, 1.7)
    sc, scb = sensor(SensorGeometry(mesh), p, zero_gradient_patch_values(mesh, p), ScQGD=0.3)
    assert np.abs(sc).max() == 0.0 and np.all(scb == 0.3)


def test_linear_pressure_on_a_uniform_box_gives_zero_inside():
    mesh = q.PolyMesh.box(6, 5, 4)
    C = mesh.array("C").reshape(-1, 3)
    p = 2.0 + 0.3 * C[:, 0] - 0.2 * C[:, 1] + 0.5 * C[:, 2]
    sc, _ = sensor(SensorGeometry(mesh), p, zero_gradient_patch_values(mesh, p), ScQGD=0.3)
    touches = np.zeros(mesh.nCells, dtype=bool)
    touches[mesh.array("owner")[mesh.nInternalFaces:]] = True
    assert (~touches).sum() == 4 * 3 * 2
    assert np.abs(sc[~touches]).max() <= 1e-14
    assert sc[touches].min() > 1e-3          # a zero-gradient patch value breaks the balance of the cell next to it


def jump_fields(mesh, x_cut, pL, pR):
    C = mesh.array("C").reshape(-1, 3)
    return np.where(C[:, 0] < x_cut, pL, pR), C


def test_single_jump_on_a_uniform_box():
    pL, pR = 1.0, 0.4
    mesh = q.PolyMesh.box(6, 5, 4)
    p, C = jump_fields(mesh, 0.5, pL, pR)
    sc, _ = sensor(SensorGeometry(mesh), p, zero_gradient_patch_values(mesh, p), ScQGD=0.3)
    dx = 1.0 / 6
    left = np.abs(C[:, 0] - (0.5 - dx / 2)) < 1e-12
    right = np.abs(C[:, 0] - (0.5 + dx / 2)) < 1e-12
    assert left.sum() == 20 and right.sum() == 20
    assert np.abs(sc[left] - abs(pR - pL) / ((5 * pL + (pL + pR) / 2) / 6)).max() <= 1e-15
    assert np.abs(sc[right] - abs(pR - pL) / ((5 * pR + (pL + pR) / 2) / 6)).max() <= 1e-15
    assert np.abs(sc[~(left | right)]).max() == 0.0


def test_empty_faces_are_not_counted():
    pL, pR = 1.0, 0.4
    mesh = q.PolyMesh.box(8, 7, 1, hi=(1.0, 0.875, 0.1), patch_types=[G, G, G, G, E, E])
    p, C = jump_fields(mesh, 0.5, pL, pR)
    sc, _ = sensor(SensorGeometry(mesh), p, zero_gradient_patch_values(mesh, p), ScQGD=0.3)
    left = np.abs(C[:, 0] - (0.5 - 1.0 / 16)) < 1e-12
    assert left.sum() == 7
    assert np.abs(sc[left] - abs(pR - pL) / ((3 * pL + (pL + pR) / 2) / 4)).max() <= 1e-15


def test_patch_faces_enter_with_their_own_pressure():
    mesh = q.PolyMesh.box(3, 1, 1, patch_types=[G, G, E, E, E, E])      # a line of three cells; x-min is patch 0
    p = np.array([1.0, 1.0, 1.0])
    pb = zero_gradient_patch_values(mesh, p).copy()
    first = int(mesh.array("patchStart")[0]) - mesh.nInternalFaces
    pb[first] = 1.6
    sc, _ = sensor(SensorGeometry(mesh), p, pb, ScQGD=0.3, cSc1=2.0)
    assert abs(sc[0] - 2.0 * 0.6 / ((1.6 + 1.0) / 2)) <= 1e-15 and sc[1] == 0.0 and sc[2] == 0.0


def test_clipping_and_the_cell_set():
    mesh = q.PolyMesh.box(6, 5, 4)
    p, C = jump_fields(mesh, 0.5, 1.0, 0.4)
    geo, pb = SensorGeometry(mesh), None
    pb = zero_gradient_patch_values(mesh, p)
    raw, _ = sensor(geo, p, pb, ScQGD=0.2)
    sc, scb = sensor(geo, p, pb, ScQGD=0.2, minSc=0.05, maxSc=0.5)
    assert np.array_equal(sc, np.clip(raw, 0.05, 0.5)) and sc.min() == 0.05 and sc.max() == 0.5 and np.all(scb == 0.2)
    _, scb = sensor(geo, p, pb, ScQGD=0.7, minSc=0.05, maxSc=0.5)
    assert np.all(scb == 0.5)                 # the clips are field operations: the patch values take them too
    _, scb = sensor(geo, p, pb, ScQGD=0.01, minSc=0.05, maxSc=-1.0)
    assert np.all(scb == 0.05)
    only_min, _ = sensor(geo, p, pb, ScQGD=0.2, minSc=0.05)
    assert np.array_equal(only_min, np.maximum(raw, 0.05))
    cells = np.array([0, 17, 119])
    sc, _ = sensor(geo, p, pb, ScQGD=0.2, minSc=0.05, maxSc=0.5, const_cells=cells)
    assert np.all(sc[cells] == 0.2)
    rest = np.setdiff1d(np.arange(mesh.nCells), cells)
    assert np.array_equal(sc[rest], np.clip(raw, 0.05, 0.5)[rest])


def test_nonorthogonal_ratio_differs_from_one_on_a_jittered_mesh():
    geo = SensorGeometry(make_mesh("box654_jitter"))
    assert np.abs(geo.r_i - 1.0).max() > 1e-3 and np.abs(geo.r_b[geo.keep] - 1.0).max() > 1e-3 and geo.r_i.min() >= 1.0 - 1e-15


# ---- the reader -----------------------------------------------------------------------------------------------------------------------
def write_var_sc_case(case_dir, body="QGDCoeffs varScModel7;\n varScModel7Dict { ScQGD 0.2; PrQGD 0.9; cSc1 1.5; minSc 0.05; maxSc 1; }", **kw):
    """write_step_case with the QGD dictionary's closure entries replaced by `body`"""
    mesh = write_step_case(case_dir, **kw)
    path = os.path.join(case_dir, "constant", "thermophysicalProperties")
    text = open(path).read()
    new, n = re.subn(r"QGDCoeffs constScPrModel1;\s*constScPrModel1Dict \{[^}]*\}", lambda m: body, text)
    assert n == 1
    open(path, "w").write(new)
    return mesh


def write_cell_set(case_dir, name, labels):
    d = os.path.join(case_dir, "constant", "polyMesh", "sets")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, name), "w") as f:
        f.write(f"FoamFile\n{{\n    version 2.0;\n    format ascii;\n    class cellSet;\n    location \"constant/polyMesh/sets\";\n    object {name};\n}}\n\n")
        f.write(f"{len(labels)}\n(\n" + "\n".join(str(int(x)) for x in labels) + "\n)\n")


def test_reader_takes_the_model_and_its_keys(tmp_path):
    write_var_sc_case(str(tmp_path / "a"))
    _, opt, fields, _ = ff.read_case_setup(str(tmp_path / "a"))
    assert opt["ScQGD"] == 0.2 and opt["PrQGD"] == 0.9
    assert opt["varSc"] == dict(model="varScModel7", ScQGD=0.2, cSc1=1.5, minSc=0.05, maxSc=1.0, const_cells=None)
    o = q.default_options(**opt)               # the model's entries pass the options struct by
    assert o.ScQGD == 0.2 and o.PrQGD == 0.9


def test_reader_defaults_and_keys_in_the_qgd_dictionary_itself(tmp_path):
    write_var_sc_case(str(tmp_path / "a"), body="QGDCoeffs varScModel7;\n ScQGD 0.3; PrQGD 1;")
    _, opt, _, _ = ff.read_case_setup(str(tmp_path / "a"))
    assert opt["varSc"] == dict(model="varScModel7", ScQGD=0.3, cSc1=1.0, minSc=-1.0, maxSc=-1.0, const_cells=None)


def test_reader_accepts_and_ignores_the_unused_keys_and_the_field_file(tmp_path):
    case_dir = str(tmp_path / "a")
    mesh = write_var_sc_case(case_dir, body="QGDCoeffs varScModel7;\n varScModel7Dict { ScQGD 0.2; PrQGD 1; smoothCoeff 0.1; rC 0.5; "
                                            "badQualitySc 0.05; maxAspectRatio 5; }")
    _, opt, _, bcs = ff.read_case_setup(case_dir)
    assert opt["varSc"]["ScQGD"] == 0.2 and set(opt["varSc"]) == {"model", "ScQGD", "cSc1", "minSc", "maxSc", "const_cells"}
    # a ScQGD file in the time directory (the application writes one) is the constructor's to overwrite: not read for this model
    from qgdsolver_amd import QGDFoam as app
    data = {"ScQGD": np.linspace(0.0, 1.0, mesh.nCells)}
    app._write_cell_fields(case_dir, "0", data, bcs, ff.read_polymesh(os.path.join(case_dir, "constant", "polyMesh")), opt["varSc"])
    text = open(os.path.join(case_dir, "0", "ScQGD")).read()
    assert "type            calculated;" in text and "value           uniform 0.2;" in text.split("inlet")[1].split("}")[0]
    _, opt2, fields2, _ = ff.read_case_setup(case_dir)
    assert "ScQGD" not in fields2 and opt2["ScQGD"] == 0.2


def test_reader_reads_the_cell_set(tmp_path):
    case_dir = str(tmp_path / "a")
    write_var_sc_case(case_dir, body="QGDCoeffs varScModel7;\n varScModel7Dict { ScQGD 0.2; PrQGD 1; constScCellSet nearStep; }")
    with pytest.raises(ff.FoamFileError, match=r"constScCellSet 'nearStep'.*is missing"):
        ff.read_case_setup(case_dir)
    write_cell_set(case_dir, "nearStep", [3, 5, 8, 13])
    _, opt, _, _ = ff.read_case_setup(case_dir)
    assert opt["varSc"]["const_cells"].dtype == np.int32 and list(opt["varSc"]["const_cells"]) == [3, 5, 8, 13]
    write_cell_set(case_dir, "nearStep", [3, 10 ** 6])
    with pytest.raises(ff.FoamFileError, match=r"sets/nearStep: cell label out of range"):
        ff.read_case_setup(case_dir)


def test_reader_refusals_by_name(tmp_path):
    write_var_sc_case(str(tmp_path / "a"), body="QGDCoeffs varScModel7;\n varScModel7Dict { PrQGD 1; }")
    with pytest.raises(ff.FoamFileError, match=r"QGD\.varScModel7: entry 'ScQGD' is missing"):
        ff.read_case_setup(str(tmp_path / "a"))
    write_var_sc_case(str(tmp_path / "b"), body="QGDCoeffs varScModel7;\n varScModel7Dict { ScQGD 1; }")
    with pytest.raises(ff.FoamFileError, match=r"QGD\.varScModel7: entry 'PrQGD' is missing"):
        ff.read_case_setup(str(tmp_path / "b"))
    for k, word in enumerate(("varScModel5", "varScModel6", "constScPrModel2")):
        write_var_sc_case(str(tmp_path / f"c{k}"), body=f"QGDCoeffs {word};\n {word}Dict {{ ScQGD 1; PrQGD 1; }}")
        with pytest.raises(ff.FoamFileError, match=rf"QGDCoeffs '{word}' is not supported \(served: constScPrModel1, varScModel7\)"):
            ff.read_case_setup(str(tmp_path / f"c{k}"))


def test_reader_refuses_the_model_on_a_case_with_cyclic_patches(tmp_path):
    from test_cyclic_patches import write_periodic_case
    case_dir = str(tmp_path / "a")
    write_periodic_case(case_dir)
    path = os.path.join(case_dir, "constant", "thermophysicalProperties")
    text = open(path).read()
    new, n = re.subn(r"QGDCoeffs\s+constScPrModel1;", "QGDCoeffs varScModel7; ScQGD 0.2; PrQGD 1;", text)
    assert n == 1
    open(path, "w").write(new)
    with pytest.raises(ff.FoamFileError, match=r"cyclic patches.*varScModel7 is not served"):
        ff.read_case_setup(case_dir)
