"""CPU: foamfile.read_case_setup on a case whose thermophysicalProperties carries a `species` list (the species block of
reactingLagrangianQGDFoam, passive: one thermo for every species)."""
import os
import textwrap

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import foamfile as ff

from test_foamfile import write_step_case

HDR = "FoamFile {{ version 2.0; format ascii; class {cls}; object {obj}; }}\n"
MIX = f"specie {{ molWeight {ff.RR * 1.4!r}; }} thermodynamics {{ Cv {1.0 / 1.4 / 0.4!r}; Hf 0; }} transport {{ mu 1e-3; Pr 1; }}"
QGD = "QGD { implicitDiffusion false; QGDCoeffs constScPrModel1; constScPrModel1Dict { ScQGD 1; PrQGD 1; } }\n"
SPECIES = dict(names=["N2", "O2", "H2O"], inert="N2", ScNumbers=[1.0, 0.8, 1.25])


def species_field_text(name, internal, inlet_value):
    return (HDR.format(cls="volScalarField", obj=name) + f"dimensions [0 0 0 0 0 0 0];\ninternalField {internal};\nboundaryField\n{{\n"
            f"    xMin {{ type fixedValue; value uniform {inlet_value}; }}\n    \"(xMax|yMin|yMax|zMin|zMax)\" {{ type zeroGradient; }}\n}}\n")


def write_species_case(case_dir, end_time=6e-3, write_interval=3e-3, n=(6, 5, 4), thermo=None, files=("N2", "O2", "H2O")):
    """a small box: inlet xMin (fixedValue flow and composition), zero-gradient walls elsewhere; GaussVolPoint, fixed deltaT 1e-3.
    thermo: the text of thermophysicalProperties after thermoType (default: mixture{} + the entries species_entries_text writes)"""
    case_dir = str(case_dir)
    mesh = q.PolyMesh.box(*n).jitter(0.1, seed=5)
    mesh.patch_names = ["xMin", "xMax", "yMin", "yMax", "zMin", "zMax"]
    ff.write_polymesh(mesh, os.path.join(case_dir, "constant", "polyMesh"))
    os.makedirs(os.path.join(case_dir, "0"))
    os.makedirs(os.path.join(case_dir, "system"))
    C = mesh.array("C").reshape(-1, 3)
    zg = {pn: ("zeroGradient", None) for pn in mesh.patch_names}
    ff.write_field(os.path.join(case_dir, "0", "U"), mesh, "U", np.tile([0.3, 0.05, 0.0], (mesh.nCells, 1)),
                   dict(zg, xMin=("fixedValue", np.array([0.3, 0.0, 0.0]))), "[0 1 -1 0 0 0 0]")
    ff.write_field(os.path.join(case_dir, "0", "T"), mesh, "T", np.ones(mesh.nCells), dict(zg, xMin=("fixedValue", np.float64(1.0))), "[0 0 0 1 0 0 0]")
    ff.write_field(os.path.join(case_dir, "0", "p"), mesh, "p", 1.0 + 0.1 * np.exp(-((C[:, 0] - 0.5) ** 2 + (C[:, 1] - 0.4) ** 2) / 0.02), zg,
                   "[1 -1 -2 0 0 0 0]")
    o2 = 0.2 + 0.1 * np.sin(2 * np.pi * C[:, 0]) * np.cos(np.pi * C[:, 1])
    h2o = 0.2 + 0.1 * np.cos(3.0 * C[:, 0] + 2.0 * C[:, 1])
    values = {"N2": 1.0 - o2 - h2o, "O2": o2, "H2O": h2o}
    inlet = {"N2": 0.5, "O2": 0.3, "H2O": 0.2}
    for name in files:
        ff.write_field(os.path.join(case_dir, "0", name), mesh, name, values[name], dict(zg, xMin=("fixedValue", np.float64(inlet[name]))))
    with open(os.path.join(case_dir, "0", "Ydefault"), "w") as f:
        f.write(species_field_text("Ydefault", "uniform 0.25", 0.125))
    with open(os.path.join(case_dir, "constant", "thermophysicalProperties"), "w") as f:
        f.write(HDR.format(cls="dictionary", obj="thermophysicalProperties") +
                "thermoType { type hePsiQGDThermo; mixture reactingMixture; transport const; thermo eConst; equationOfState perfectGas; "
                "specie specie; energy sensibleInternalEnergy; }\n" +
                (thermo if thermo is not None else f"mixture {{ {MIX} }}\n" + ff.species_entries_text(SPECIES)) + QGD)
    with open(os.path.join(case_dir, "system", "fvSchemes"), "w") as f:
        f.write(HDR.format(cls="dictionary", obj="fvSchemes") + textwrap.dedent('''
            ddtSchemes { default Euler; }
            gradSchemes { default Gauss linear; }
            divSchemes { default none; }
            laplacianSchemes { default Gauss linear corrected; }
            interpolationSchemes { default linear; }
            snGradSchemes { default corrected; }
            fvsc { default GaussVolPoint; }
            '''))
    with open(os.path.join(case_dir, "system", "controlDict"), "w") as f:
        f.write(HDR.format(cls="dictionary", obj="controlDict") +
                f"application QGDFoam;\nstartFrom startTime;\nstartTime 0;\nendTime {end_time!r};\ndeltaT 1e-3;\nwriteControl runTime;\n"
                f"writeInterval {write_interval!r};\nadjustTimeStep no;\ntimePrecision 8;\n")
    return mesh, values, inlet


def test_round_trip_of_a_written_species_case(tmp_path):
    mesh, values, inlet = write_species_case(tmp_path)
    m2, opt, fields, bcs = ff.read_case_setup(str(tmp_path))
    sp = opt["species"]
    assert sp["names"] == SPECIES["names"] and sp["inert"] == "N2" and sp["ScNumbers"] == SPECIES["ScNumbers"]
    assert opt["implicitDiffusion"] == 0 and opt["mu"] == 1e-3
    for n in sp["names"]:
        assert np.array_equal(sp["fields"][n], values[n])
        assert sp["bcs"][n][0] == ("fixedValue", inlet[n]) and all(e == ("zeroGradient", None) for e in sp["bcs"][n][1:])
    # the entries travel past the options struct, like varSc
    o = q.default_options(**opt)
    assert o.implicitDiffusion == 0
    # ... and back: what the writer leaves is what the reader takes
    ff.write_species_fields(str(tmp_path), "0.5", m2, sp, {n: sp["fields"][n] * 0.5 for n in sp["names"]})
    for name in ("U", "T", "p"):
        os.link(os.path.join(str(tmp_path), "0", name), os.path.join(str(tmp_path), "0.5", name))
    sp2 = ff.read_case_setup(str(tmp_path), "0.5")[1]["species"]
    assert sp2["bcs"] == sp["bcs"] and sp2["ScNumbers"] == sp["ScNumbers"]
    for n in sp["names"]:
        assert np.array_equal(sp2["fields"][n], sp["fields"][n] * 0.5)


def test_ydefault_serves_a_species_without_a_file(tmp_path):
    write_species_case(tmp_path, files=("N2", "O2"))
    sp = ff.read_case_setup(str(tmp_path))[1]["species"]
    assert np.all(sp["fields"]["H2O"] == 0.25) and sp["bcs"]["H2O"][0] == ("fixedValue", 0.125) and sp["bcs"]["H2O"][3] == ("zeroGradient", None)
    assert not np.all(sp["fields"]["O2"] == 0.25)
    os.remove(os.path.join(str(tmp_path), "0", "Ydefault"))
    with pytest.raises(ff.FoamFileError, match="Ydefault"):
        ff.read_case_setup(str(tmp_path))


def test_sc_numbers_default_to_one_and_unknown_names_are_ignored(tmp_path):
    write_species_case(tmp_path, thermo=f"mixture {{ {MIX} }}\nspecies (N2 O2 H2O);\ninertSpecie O2;\nScNumbers ((H2O 0.6) (CO2 2.0));\n")
    sp = ff.read_case_setup(str(tmp_path))[1]["species"]
    assert sp["inert"] == "O2" and sp["ScNumbers"] == [1.0, 1.0, 0.6]
    write_species_case(tmp_path / "b", thermo=f"mixture {{ {MIX} }}\nspecies (N2 O2 H2O);\ninertSpecie O2;\n")
    assert ff.read_case_setup(str(tmp_path / "b"))[1]["species"]["ScNumbers"] == [1.0, 1.0, 1.0]


def test_inert_specie_is_required_and_must_be_a_species(tmp_path):
    write_species_case(tmp_path / "a", thermo=f"mixture {{ {MIX} }}\nspecies (N2 O2 H2O);\n")
    with pytest.raises(ff.FoamFileError, match="inertSpecie"):
        ff.read_case_setup(str(tmp_path / "a"))
    write_species_case(tmp_path / "b", thermo=f"mixture {{ {MIX} }}\nspecies (N2 O2 H2O);\ninertSpecie AR;\n")
    with pytest.raises(ff.FoamFileError, match="'AR' is not in the species list"):
        ff.read_case_setup(str(tmp_path / "b"))


def test_per_species_dictionaries_must_be_equal(tmp_path):
    same = "".join(f"{n} {{ {MIX} }}\n" for n in SPECIES["names"])
    write_species_case(tmp_path / "a", thermo=same + ff.species_entries_text(SPECIES))
    opt = ff.read_case_setup(str(tmp_path / "a"))[1]
    assert opt["mu"] == 1e-3 and abs(opt["R"] - 1 / 1.4) < 1e-15 and opt["species"]["names"] == SPECIES["names"]
    other = same.replace("H2O { specie { molWeight " + repr(ff.RR * 1.4), "H2O { specie { molWeight 18.0")
    assert other != same
    write_species_case(tmp_path / "b", thermo=other + ff.species_entries_text(SPECIES))
    with pytest.raises(ff.FoamFileError, match="species with different thermophysical properties are not served: the composition is passive"):
        ff.read_case_setup(str(tmp_path / "b"))


def test_implicit_diffusion_default_is_refused(tmp_path):
    write_species_case(tmp_path)
    tp = os.path.join(str(tmp_path), "constant", "thermophysicalProperties")
    text = open(tp).read().replace("implicitDiffusion false;", "")
    open(tp, "w").write(text)
    with pytest.raises(ff.FoamFileError, match="implicitDiffusion false"):
        ff.read_case_setup(str(tmp_path))


def test_unsupported_species_boundary_condition_is_refused_by_name(tmp_path):
    write_species_case(tmp_path)
    path = os.path.join(str(tmp_path), "0", "O2")
    text = open(path).read().replace("type            zeroGradient;", "type            inletOutlet;", 1)
    open(path, "w").write(text)
    with pytest.raises(ff.FoamFileError, match="inletOutlet"):
        ff.read_case_setup(str(tmp_path))


def test_a_case_without_species_reads_as_before(tmp_path):
    write_step_case(str(tmp_path))
    _, opt, fields, bcs = ff.read_case_setup(str(tmp_path))
    assert "species" not in opt and sorted(fields) == ["T", "U", "p"]
    assert sorted(opt) == sorted(["R", "Cv", "mu", "Pr", "implicitDiffusion", "ScQGD", "PrQGD", "alphaQGD", "stencil", "fluxSchemeU", "fluxSchemeH",
                                  "deltaT", "adjustTimeStep", "maxCo", "maxDeltaT", "cTau"])
    # stray species files in the time directory change nothing without the list
    open(os.path.join(str(tmp_path), "0", "Ydefault"), "w").write("not even a field")
    assert "species" not in ff.read_case_setup(str(tmp_path))[1]
