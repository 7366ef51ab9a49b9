"""CPU: the SRFQHDFoam case reader (foamfile.read_srf_case_setup) -- omega from SRFProperties, SRFVelocity patches, what it refuses --
the three C-ABI entries of the rotating-frame case in the ctypes table, and the superposition of srf_ref.py against a direct run of
the oracle."""
import os

import numpy as np
import pytest

from qgdsolver_amd import _lib as L, foamfile as ff

import srf_ref as R
from util import make_mesh


def test_omega_from_rpm_and_a_non_unit_axis(tmp_path):
    R.write_srf_case(str(tmp_path), rpm=90.0, axis=(0, 3, 4), origin=(0.5, 0.25, 0.0))
    mesh, opt, fields, bcs, srf = ff.read_srf_case_setup(str(tmp_path))
    assert np.allclose(srf["omega"], np.array([0.0, 0.6, 0.8]) * 90.0 * 2.0 * np.pi / 60.0, rtol=1e-15, atol=0)
    assert np.allclose(srf["axis"], (0.0, 0.6, 0.8)) and np.array_equal(srf["origin"], (0.5, 0.25, 0.0)) and srf["rpm"] == 90.0
    assert opt["stencil"] == "GaussVolPoint" and opt["implicitDiffusion"] == 0 and opt["beta"] == 0.0 and opt["pRefCell"] == 17
    assert fields["U"].shape == (mesh.nCells, 3) and np.all(fields["T"] == 300.0)


def test_srfvelocity_patches(tmp_path):
    inlet = np.array([0.1, -0.2, 0.05])
    R.write_srf_case(str(tmp_path), rpm=45.0, axis=(1, 1, 0), origin=(0.1, 0.2, 0.3), urel_entries={
        "casing": "type SRFVelocity; relative no; inletValue uniform (0.1 -0.2 0.05); value uniform (0 0 0);",
        "rotor": "type SRFVelocity; relative yes; inletValue uniform (0.1 -0.2 0.05); value uniform (0 0 0);",
        "floor": "type zeroGradient;"})
    mesh, opt, fields, bcs, srf = ff.read_srf_case_setup(str(tmp_path))
    by = dict(zip(mesh.patch_names, bcs))
    i = mesh.patch_names.index("casing")
    ps, pz = int(mesh.array("patchStart")[i]), int(mesh.array("patchSize")[i])
    Cf = mesh.array("Cf").reshape(-1, 3)[ps:ps + pz]
    kind, vals = by["casing"]["U"]
    assert kind == "fixedValue" and vals.shape == (pz, 3)
    assert np.array_equal(vals, -np.cross(srf["omega"], Cf - srf["origin"]) + inlet)
    assert np.abs(vals - inlet).max() > 0.1                           # the wall does move in the frame
    kind, val = by["rotor"]["U"]
    assert kind == "fixedValue" and np.shape(val) == (3,) and np.array_equal(val, inlet)      # relative yes: one value
    assert by["floor"]["U"] == ("zeroGradient", None) and by["ceiling"]["U"][0] == "fixedValue" and np.shape(by["ceiling"]["U"][1]) == (3,)
    assert by["casing"]["p"] == ("fixedGradient", 0.0) and by["casing"]["T"] == ("zeroGradient", None)


def test_reader_refusals(tmp_path):
    d = str(tmp_path / "model")
    os.makedirs(d)
    R.write_srf_case(d, srf_text="SRFModel omegaTable;\norigin (0 0 0);\naxis (0 0 1);\n")
    with pytest.raises(ff.FoamFileError, match="SRFModel 'omegaTable'"):
        ff.read_srf_case_setup(d)
    d = str(tmp_path / "free")
    os.makedirs(d)
    R.write_srf_case(d, urel_entries={"rotor": "type SRFFreestreamVelocity; UInf (1 0 0); value uniform (0 0 0);"})
    with pytest.raises(ff.FoamFileError, match="SRFFreestreamVelocity"):
        ff.read_srf_case_setup(d)
    d = str(tmp_path / "inlet")
    os.makedirs(d)
    n = 5 * 4
    lst = "nonuniform List<vector> %d (%s)" % (n, " ".join("(%g 0 0)" % (0.01 * k) for k in range(n)))
    R.write_srf_case(d, urel_entries={"casing": f"type SRFVelocity; relative no; inletValue {lst}; value uniform (0 0 0);"})
    with pytest.raises(ff.FoamFileError, match="uniform inletValue"):
        ff.read_srf_case_setup(d)
    # Urel is required: a case that only has U is refused, and told why
    d = str(tmp_path / "nourel")
    os.makedirs(d)
    R.write_srf_case(d, velocity_file="U")
    with pytest.raises(ff.FoamFileError, match="Urel"):
        ff.read_srf_case_setup(d)
    d = str(tmp_path / "noprops")
    os.makedirs(d)
    R.write_srf_case(d)
    os.remove(os.path.join(d, "constant", "SRFProperties"))
    with pytest.raises(ff.FoamFileError, match="SRFProperties"):
        ff.read_srf_case_setup(d)


def test_ctypes_table_carries_the_new_entries():
    for name in ("qgd_qhd_case_set_srf", "qgd_qhd_case_srf_info", "qgd_qhd_case_set_bc_values"):
        assert name in L.SIGNATURES and hasattr(L.lib, name), name
    assert L.SRF_SOLVE_T == 1
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qgd_amd.h")).read()
    assert "#define QGD_SRF_SOLVE_T 1" in text and "#define QGD_ABI_VERSION 9" in text


@pytest.mark.parametrize("implicit", [0, 1])
@pytest.mark.parametrize("kind", ["box654_jitter", "box654_tri"])
def test_superposition_reproduces_a_direct_oracle_run(kind, implicit):
    """U = s(x) d with one direction d: -2 omega ^ U = (-2 s) (omega ^ d), which the oracle takes directly as beta = 1, g = omega ^ d,
    T = -2 s.  The superposition of srf_ref.py (three runs with T = U_k, beta*T*g off) gives the same step: to rounding in the explicit
    branch, to the solves' tolerance (implicitTol = 1e-12) in the implicit one."""
    from oracle import OracleQhdCase
    from util import oracle_mesh_of

    mesh = make_mesh(kind)
    d = np.array([0.6, -0.3, 0.2])
    omega = R.OMEGA_3D
    C = mesh.array("C").reshape(-1, 3)
    rng = np.random.default_rng(2)
    s = 0.5 + 0.2 * rng.standard_normal(mesh.nCells)
    U, p = s[:, None] * d[None, :], 0.1 * rng.standard_normal(mesh.nCells)
    opt = R.options("GaussVolPoint", implicit, beta=0.0)
    bcs = R.patch_bcs(mesh)
    bcs[0]["U"] = ("fixedValue", tuple(0.4 * d))
    ref = R.SrfReference(mesh, opt, bcs, omega)
    want, plain = ref.step(U, np.full(mesh.nCells, 300.0), p)
    direct = OracleQhdCase(oracle_mesh_of(mesh), R.copy_options(opt, beta=1.0, g=np.cross(omega, d)))
    for ip, bc in enumerate(bcs):
        tb = ("fixedValue", -2.0 * 0.4) if ip == 0 else (("zeroGradient", None) if bc["U"][0] == "zeroGradient" else ("fixedValue", 0.0))
        direct.set_bc(ip, U=bc["U"], T=tb, p=bc["p"])
    direct.set_fields(U, -2.0 * s, p)
    direct.step(1)
    assert R.rel(want["U"], plain["U"]) >= 1e-3
    for f in R.FIELDS:
        err = R.rel(want[f], direct.field(f))
        assert err <= (1e-10 if implicit else 1e-13), (f, err)
    direct.close(); ref.close()
