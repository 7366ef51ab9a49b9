"""adjustTimeStep of QHDFoam and SRFQHDFoam on the host: the time controls of system/controlDict as read_qhd_case_setup and
read_srf_case_setup return them on request [readTimeControls.H; setDeltaT-QGDQHD.H L45], the two C-ABI entries in the library and in
_lib.SIGNATURES, and the numpy restatement of hQGDf that the device tests use against the listing's updateQGDLength (fixture
ref_expr_qgdlength)."""
import os

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L, foamfile as ff

import ref_expr_cases as rc
from qhd_time_step_ref import h_qgd_f
from srf_ref import write_srf_case
from test_qhdfoam_case import write_cavity_case

GREAT = 1e300


def add_control(case_dir, text):
    with open(os.path.join(case_dir, "system", "controlDict"), "a") as f:
        f.write(text)


def test_qhd_reader_returns_the_time_controls_on_request(tmp_path):
    d = str(tmp_path / "full")
    write_cavity_case(d)
    assert len(ff.read_qhd_case_setup(d)) == 4                                   # as before
    tc = ff.read_qhd_case_setup(d, time_control=True)[4]
    assert tc == dict(adjustTimeStep=False, maxCo=1.0, maxDeltaT=GREAT, cTau=0.75)
    add_control(d, "adjustTimeStep yes; maxCo 0.2; maxDeltaT 0.5; cTau 0.6;\n")
    with pytest.raises(ff.FoamFileError, match="adjustTimeStep"):                # the default keeps the refusal
        ff.read_qhd_case_setup(d)
    mesh, opt, fields, bcs, tc = ff.read_qhd_case_setup(d, time_control=True)
    assert tc == dict(adjustTimeStep=True, maxCo=0.2, maxDeltaT=0.5, cTau=0.6)
    assert opt["deltaT"] == 1e-3 and not set(tc) & set(opt)                     # the options go into qgd_qhd_options as they are
    d2 = str(tmp_path / "defaults")
    write_cavity_case(d2)
    add_control(d2, "adjustTimeStep yes;\n")
    assert ff.read_qhd_case_setup(d2, time_control=True)[4] == dict(adjustTimeStep=True, maxCo=1.0, maxDeltaT=GREAT, cTau=0.75)


def test_srf_reader_passes_the_keyword_through(tmp_path):
    d = str(tmp_path / "srf")
    write_srf_case(d)
    assert len(ff.read_srf_case_setup(d)) == 5
    add_control(d, "adjustTimeStep yes; maxCo 0.2; maxDeltaT 0.5; cTau 0.6;\n")
    with pytest.raises(ff.FoamFileError, match="adjustTimeStep"):
        ff.read_srf_case_setup(d)
    out = ff.read_srf_case_setup(d, time_control=True)
    assert len(out) == 6 and out[5] == dict(adjustTimeStep=True, maxCo=0.2, maxDeltaT=0.5, cTau=0.6) and "omega" in out[4]
    d2 = str(tmp_path / "srf_defaults")
    write_srf_case(d2)
    add_control(d2, "adjustTimeStep yes;\n")
    assert ff.read_srf_case_setup(d2, time_control=True)[5] == dict(adjustTimeStep=True, maxCo=1.0, maxDeltaT=GREAT, cTau=0.75)


def test_both_entries_are_declared_and_exported():
    for name in ("qgd_qhd_case_set_time_control", "qgd_qhd_case_time_info"):
        assert name in L.SIGNATURES, name
        assert getattr(L.lib, name) is not None
    assert len(L.SIGNATURES["qgd_qhd_case_set_time_control"][1]) == 5 and len(L.SIGNATURES["qgd_qhd_case_time_info"][1]) == 2


def test_the_restated_hQGDf_is_the_listings():
    """h_qgd_f (2 min(|C_O - Cf|, |C_N - Cf|) inside, 2/|deltaCoeffs| on patch faces, nothing on empty ones) against
    QGDCoeffs::updateQGDLength executed from the listing text over three whole meshes"""
    g = rc.load("qgdlength")
    for mi in range(int(g["nMeshes"])):
        a = {k: g[f"m{mi}_{k}"] for k in ("points", "faceOffsets", "facePoints", "owner", "neighbour", "patchStart", "patchSize", "patchType")}
        mesh = q.PolyMesh.from_arrays(a["points"], a["faceOffsets"], a["facePoints"], a["owner"], a["neighbour"], int(g[f"m{mi}_nCells"]),
                                      a["patchStart"], a["patchSize"], a["patchType"])
        hf, live = h_qgd_f(mesh)
        want = g[f"m{mi}_hQGDf"]
        assert np.abs(hf[live] - want[live]).max() <= 1e-14 * np.abs(want).max(), mi
        assert live.sum() == mesh.nFaces - sum(int(z) for z, t in zip(a["patchSize"], a["patchType"]) if t == L.PATCH_EMPTY)
