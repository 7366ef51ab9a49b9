"""CPU: foamfile.read_case_setup on a species case that runs the implicitDiffusion branch -- the reference's default when the QGD dictionary
has no entry [QGDThermo.C L70-82] -- and the controls of the species' solves, fvSolution.solvers.<species name> [QGDYEqn.H L62]."""
import os

import numpy as np

from qgdsolver_amd import foamfile as ff

from test_species_reader import MIX, SPECIES, write_species_case

HDR = "FoamFile { version 2.0; format ascii; class dictionary; object fvSolution; }\n"


def uncorrected_laplacian(case_dir):
    """the mesh is jittered: the implicit branch's fvm::laplacian is read with `Gauss linear uncorrected` there (the reader refuses the explicit
    non-orthogonal correction by name)"""
    fs = os.path.join(str(case_dir), "system", "fvSchemes")
    text = open(fs).read()
    assert "laplacianSchemes { default Gauss linear corrected; }" in text
    open(fs, "w").write(text.replace("laplacianSchemes { default Gauss linear corrected; }", "laplacianSchemes { default Gauss linear uncorrected; }"))


def write_default_branch_case(case_dir, solvers=None):
    """write_species_case without its `implicitDiffusion false;`; solvers: the body of fvSolution.solvers (None: no fvSolution)"""
    mesh, values, inlet = write_species_case(case_dir)
    tp = os.path.join(str(case_dir), "constant", "thermophysicalProperties")
    text = open(tp).read()
    assert "implicitDiffusion false;" in text
    open(tp, "w").write(text.replace("implicitDiffusion false;", ""))
    uncorrected_laplacian(case_dir)
    if solvers is not None:
        open(os.path.join(str(case_dir), "system", "fvSolution"), "w").write(HDR + "solvers\n{\n" + solvers + "}\n")
    return mesh, values, inlet


def test_a_species_case_without_the_entry_reads_as_the_implicit_branch(tmp_path):
    mesh, values, inlet = write_default_branch_case(tmp_path)
    _, opt, fields, bcs = ff.read_case_setup(str(tmp_path))
    assert opt["implicitDiffusion"] == 1
    sp = opt["species"]
    assert sp["names"] == SPECIES["names"] and sp["inert"] == "N2" and sp["ScNumbers"] == SPECIES["ScNumbers"]
    for n in sp["names"]:
        assert np.array_equal(sp["fields"][n], values[n])
        assert sp["bcs"][n][0] == ("fixedValue", inlet[n])
    # no fvSolution: OpenFOAM's defaults, as for U and e
    assert sp["tolerance"] == 1e-6 and sp["maxIter"] == 1000


def test_the_explicit_branch_carries_no_solver_controls(tmp_path):
    write_species_case(tmp_path)
    opt = ff.read_case_setup(str(tmp_path))[1]
    assert opt["implicitDiffusion"] == 0 and "tolerance" not in opt["species"] and "maxIter" not in opt["species"]


def test_solver_entries_by_name_by_regular_expression_and_absent(tmp_path):
    # O2 by name, H2O by a quoted regular expression; N2 is the inert species: its entry is never looked up
    write_default_branch_case(tmp_path / "a", '    O2 { solver PBiCGStab; tolerance 1e-9; maxIter 300; }\n'
                                              '    "H2.*" { solver PBiCGStab; tolerance 1e-7; maxIter 700; }\n'
                                              '    N2 { solver PBiCGStab; tolerance 1e-15; maxIter 9000; }\n'
                                              '    "(U|e)" { solver PBiCGStab; tolerance 1e-8; maxIter 50; }\n')
    opt = ff.read_case_setup(str(tmp_path / "a"))[1]
    assert (opt["species"]["tolerance"], opt["species"]["maxIter"]) == (1e-9, 700)       # the tightest, the largest
    assert (opt["implicitTol"], opt["implicitMaxIter"]) == (1e-8, 50)                    # U and e keep their own
    # H2O absent: OpenFOAM's defaults 1e-6 and 1000 take part in the choice
    write_default_branch_case(tmp_path / "b", '    O2 { solver PBiCGStab; tolerance 1e-9; maxIter 300; }\n')
    sp = ff.read_case_setup(str(tmp_path / "b"))[1]["species"]
    assert (sp["tolerance"], sp["maxIter"]) == (1e-9, 1000)
    # an entry of the name wins over an expression that matches it too; an expression must match the whole name
    write_default_branch_case(tmp_path / "c", '    ".*" { solver PBiCGStab; tolerance 1e-11; maxIter 40; }\n'
                                              '    O2 { solver PBiCGStab; tolerance 1e-5; maxIter 30; }\n'
                                              '    "H2" { solver PBiCGStab; tolerance 1e-13; maxIter 5000; }\n')
    sp = ff.read_case_setup(str(tmp_path / "c"))[1]["species"]
    assert (sp["tolerance"], sp["maxIter"]) == (1e-11, 40)                               # O2: (1e-5, 30); H2O: ".*" (1e-11, 40); "H2" matches neither
    # entries without the two controls: the defaults
    write_default_branch_case(tmp_path / "d", '    "(O2|H2O)" { solver PBiCGStab; preconditioner DILU; }\n')
    sp = ff.read_case_setup(str(tmp_path / "d"))[1]["species"]
    assert (sp["tolerance"], sp["maxIter"]) == (1e-6, 1000)


def test_round_trip_through_species_entries_text(tmp_path):
    write_default_branch_case(tmp_path / "a", '    "(O2|H2O)" { solver PBiCGStab; tolerance 1e-10; maxIter 400; }\n')
    m, opt, _, _ = ff.read_case_setup(str(tmp_path / "a"))
    sp = opt["species"]
    # what the reader returned, written back (species_entries_text ignores the solver controls: they live in fvSolution), reads the same
    thermo = "mixture { " + MIX + " }\n" + ff.species_entries_text(sp)
    write_species_case(tmp_path / "b", thermo=thermo)
    tp = os.path.join(str(tmp_path / "b"), "constant", "thermophysicalProperties")
    text = open(tp).read()
    open(tp, "w").write(text.replace("implicitDiffusion false;", ""))
    uncorrected_laplacian(tmp_path / "b")
    open(os.path.join(str(tmp_path / "b"), "system", "fvSolution"), "w").write(
        HDR + 'solvers\n{\n    "(O2|H2O)" { solver PBiCGStab; tolerance 1e-10; maxIter 400; }\n}\n')
    sp2 = ff.read_case_setup(str(tmp_path / "b"))[1]["species"]
    assert sp2["names"] == sp["names"] and sp2["inert"] == sp["inert"] and sp2["ScNumbers"] == sp["ScNumbers"] and sp2["bcs"] == sp["bcs"]
    assert (sp2["tolerance"], sp2["maxIter"]) == (sp["tolerance"], sp["maxIter"]) == (1e-10, 400)
    for n in sp["names"]:
        assert np.array_equal(sp2["fields"][n], sp["fields"][n])


class RecordingCase:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a, **k: self.calls.append((name, a, k))


def test_apply_species_passes_the_controls_on(tmp_path):
    write_default_branch_case(tmp_path / "a", '    "(O2|H2O)" { solver PBiCGStab; tolerance 1e-10; maxIter 400; }\n')
    case = RecordingCase()
    ff.apply_species(case, ff.read_case_setup(str(tmp_path / "a"))[1]["species"])
    names = [c[0] for c in case.calls]
    assert names[0] == "set_species" and ("set_species_solver", (1e-10, 400), {}) in case.calls
    assert case.calls[0][2].get("implicit") is True           # the implicit branch is asked for by name (QGD_SPECIES_IMPLICIT)
    write_species_case(tmp_path / "b")
    case = RecordingCase()
    ff.apply_species(case, ff.read_case_setup(str(tmp_path / "b"))[1]["species"])
    assert "set_species_solver" not in [c[0] for c in case.calls] and "implicit" not in case.calls[0][2]


def test_the_written_case_itself_names_both_ways_out(tmp_path):
    """write_species_case asks for `Gauss linear corrected` on a jittered mesh: without its `implicitDiffusion false;` the implicit branch
    would read that scheme, and the refusal names the uncorrected scheme and the explicit branch"""
    import pytest
    write_species_case(tmp_path)
    tp = os.path.join(str(tmp_path), "constant", "thermophysicalProperties")
    text = open(tp).read()
    open(tp, "w").write(text.replace("implicitDiffusion false;", ""))
    with pytest.raises(ff.FoamFileError, match="Gauss linear uncorrected.*implicitDiffusion false"):
        ff.read_case_setup(str(tmp_path))
