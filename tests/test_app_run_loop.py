"""The host logic the case-directory applications share (qgdsolver_amd.apprun and the writers / reader helpers of foamfile), driven by
stub cases: the write cadence, the -nSteps cut, the end of an adjustTimeStep run, the hand-over to the function objects, the patch
entries of the written fields and the thermo block the QHD family reads alike.  No device is opened."""
import os
import types

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L, apprun, foamfile as ff

from test_qhdfoam_case import write_cavity_case
from test_scalar_transport_case import write_scalar_case


# ---- 1. the run loop --------------------------------------------------------------------------------------------------------------------
class StubCase:
    """steps of a fixed deltaT, or of the deltaTs given; counts in whole steps so that the times are the multiples of deltaT"""

    def __init__(self, dt=0.1, dts=None):
        self.dt, self.dts, self.calls, self.steps, self.time = dt, dts, [], 0, 0.0

    def step(self, n):
        self.calls.append(n)
        for _ in range(n):
            self.time = self.time + self.dts[self.steps] if self.dts else (self.steps + 1) * self.dt
            self.steps += 1

    def info(self):
        return {"time": self.time, "deltaT": self.dts[self.steps - 1] if self.dts and self.steps else self.dt}


def control(**entries):
    return dict({"deltaT": 0.1, "endTime": 1.0}, **entries)


def loop(cd, n_steps=None, adjust=False, case=None, functions=None, **kw):
    case = case or StubCase()
    dt, end_time, chunk, precision, total = apprun.run_control(cd, 0.0, n_steps, adjust, **kw)
    seen, written = [], []
    names = apprun.step_chunks(case, apprun.stepping(case.step, functions, 0.0), 0.0, chunk, total, precision,
                               lambda done, t, info: seen.append((done, t, info["time"])), written.append, end_time)
    assert names == written and all(t == time for _, t, time in seen)
    return case, seen, written


def test_write_cadence_and_the_last_short_chunk():
    case, seen, written = loop(control(writeControl="timeStep", writeInterval=3))
    assert case.calls == [3, 3, 3, 1] and written == ["0.3", "0.6", "0.9", "1"]
    assert [done for done, _, _ in seen] == [3, 6, 9, 10]


def test_nsteps_cuts_the_run():
    case, _, written = loop(control(writeControl="timeStep", writeInterval=3), n_steps=4)
    assert case.calls == [3, 1] and written == ["0.3", "0.4"]


def test_no_writer_writes_nothing():
    case = StubCase()
    assert apprun.step_chunks(case, case.step, 0.0, 3, 4, 6, lambda *a: None) == [] and case.calls == [3, 1]


def test_run_time_control_is_the_rounded_number_of_steps():
    for word in ("runTime", "adjustableRunTime"):
        assert apprun.run_control(control(writeControl=word, writeInterval=0.25), 0.0) == (0.1, 1.0, 2, 6, 10)    # round(2.5) = 2
    assert apprun.run_control(control(writeControl="runTime", writeInterval=0.01, timePrecision=9), 0.5) == (0.1, 1.0, 1, 9, 5)
    assert apprun.run_control(control(), 0.0)[2] == 1                                                             # writeControl timeStep; writeInterval 1


def test_unknown_write_control_is_refused_in_the_callers_words():
    with pytest.raises(ff.FoamFileError) as ei:
        apprun.run_control(control(writeControl="clockTime"), 0.0)
    assert str(ei.value) == "writeControl 'clockTime' is not supported (timeStep, runTime, adjustableRunTime)"
    with pytest.raises(ff.FoamFileError) as ei:        # QGDFoam under adjustTimeStep
        apprun.run_control(control(writeControl="runTime"), 0.0, None, True, apprun.ADJUST_REFUSAL, run_time=False)
    assert str(ei.value) == "writeControl 'runTime' with adjustTimeStep is not supported (use writeControl timeStep)"
    assert apprun.run_control(control(writeInterval=4), 0.0, None, True, apprun.ADJUST_REFUSAL, run_time=False) == (0.1, 1.0, 4, 6, None)


class StubFunctions:
    def __init__(self, every):
        self.every, self.seen = every, []

    def next_due(self, taken):
        return self.every - taken % self.every

    def after_step(self, taken, t0):
        self.seen.append((taken, t0))


def test_steps_are_cut_where_a_function_is_due():
    fo = StubFunctions(2)
    case, _, written = loop(control(writeControl="timeStep", writeInterval=3), functions=fo)
    assert [taken for taken, _ in fo.seen] == [2, 3, 4, 6, 8, 9, 10] and all(t0 == 0.0 for _, t0 in fo.seen)
    assert case.calls == [2, 1, 1, 2, 2, 1, 1] and written == ["0.3", "0.6", "0.9", "1"]
    case = StubCase()
    assert apprun.stepping(case.step, None, 0.0) == case.step      # without functions: the step itself


def test_adjustable_run_ends_with_the_first_step_at_end_time_and_writes_it():
    case, seen, written = loop(control(writeControl="timeStep", writeInterval=3), adjust=True, case=StubCase(dts=[0.3, 0.3, 0.3, 0.25, 0.25]))
    assert case.calls == [1, 1, 1, 1] and written == ["0.9", "1.15"] and [done for done, _, _ in seen] == [3, 4]
    # endTime to 1e-12 of its size [the run loop's test of runTime.run()]
    case, _, written = loop(control(writeInterval=5), adjust=True, case=StubCase(dts=[0.5, 0.5 - 1e-13, 0.5]))
    assert case.calls == [1, 1] and written == ["1"]
    case, _, _ = loop(control(writeInterval=5), adjust=True, case=StubCase(dts=[0.5, 0.5 - 1e-11, 0.5]))
    assert case.calls == [1, 1, 1]
    # -nSteps under adjustTimeStep: the count decides, whatever the time
    case, _, written = loop(control(writeInterval=2), n_steps=3, adjust=True, case=StubCase(dts=[0.6, 0.6, 0.6]))
    assert case.calls == [2, 1] and written == ["1.2", "1.8"]


def test_qhd_run_logs_and_writes_around_the_loop(tmp_path):
    """apprun.run_qhd with a stub case: the banner, the per-chunk report with the implicit solves that worked, End"""
    os.makedirs(tmp_path / "system")
    os.makedirs(tmp_path / "0.2")
    (tmp_path / "system" / "controlDict").write_text("startFrom latestTime;\nendTime 0.5;\ndeltaT 0.1;\nwriteInterval 2;\n")
    case = StubCase()
    case.mesh = types.SimpleNamespace(nCells=12)
    case.options = types.SimpleNamespace(implicitTol=1e-9, implicitMaxIter=50)
    info = case.info
    case.info = lambda: dict(info(), pInitialResidual=0.5, pFinalResidual=1e-7, pIterations=4)
    case.implicit_info = lambda: {"solves": {"Ux": dict(initial=0.25, final=1e-10, iterations=3), "Uz": dict(initial=0.0, final=0.0, iterations=0)},
                                  "unconverged_steps": 2 if case.steps > 2 else 0, "stalled_steps": 0}
    opt = {"implicitDiffusion": 1, "stencil": "GaussVolPoint", "tauModel": "constTau"}
    written, lines = [], []

    def assemble(t0_name):
        assert t0_name == "0.2"
        return "dev", case, opt, ("  a line of its own",), written.append

    def summary(c):
        return "T", np.array([c.time]), f"time is {c.time:g}"

    dev, got, names = apprun.run_qhd("QHDFoam", "U / T", str(tmp_path), None, True, lines.append, assemble, summary)
    assert (dev, got) == ("dev", case) and names == written == ["0.4", "0.5"] and case.calls == [2, 1]
    assert lines[0] == "QHDFoam (qgdsolver_amd, implicitDiffusion true): 12 cells, fvsc GaussVolPoint, QGDCoeffs constTau, deltaT 0.1, start 0.2"
    assert lines[1] == "  a line of its own" and lines[-1] == "End"
    body = [x for x in lines[2:-1] if not x.startswith("  NOTE: the pressure solve")]
    assert [x.split("  ClockTime")[0] for x in body] == [
        "Time = 0.4  steps 2", "  p: Initial residual = 0.5, Final residual = 1e-07, No Iterations 4", "  Ux: 0.25 -> 1e-10 in 3", "  time is 0.2",
        "Time = 0.5  steps 3", "  p: Initial residual = 0.5, Final residual = 1e-07, No Iterations 4", "  Ux: 0.25 -> 1e-10 in 3",
        "  WARNING: 2 step(s) so far in which an implicit solve stopped above its tolerance (implicitTol 1e-09, maxIter 50)", "  time is 0.3"]
    # a field that is not finite ends the run, after its report
    lines.clear()
    with pytest.raises(FloatingPointError, match="T is not finite at time 0.6"):
        apprun.run_qhd("QHDFoam", "U / T", str(tmp_path), 1, False, lines.append, lambda name: ("dev", case, opt, (), None), lambda c: ("T", np.array([np.nan]), "x"))
    assert lines[-1].startswith("  x  ClockTime")


# ---- 2. the patch entries of the written fields -------------------------------------------------------------------------------------------
class FieldCase:
    """a case that holds known fields: cell values and the values on the boundary faces"""

    def __init__(self, mesh):
        rng = np.random.default_rng(5)
        self.mesh = mesh
        self.fields = {}
        for name, shape in (("U", (3,)), ("T", ()), ("p", ())):
            self.fields[name] = rng.standard_normal((mesh.nCells,) + shape)
            self.fields[name + ".boundary"] = rng.standard_normal((mesh.nBoundaryFaces,) + shape)

    def field(self, name):
        return self.fields[name]


def small_mesh():
    G, E, S = L.PATCH_GENERIC, L.PATCH_EMPTY, L.PATCH_SYMMETRYPLANE
    mesh = q.PolyMesh.box(2, 2, 1, hi=(1.0, 1.0, 0.1), patch_types=[G, G, S, G, E, E])
    mesh.patch_names = ["left", "right", "mirror", "lid", "front", "back"]
    bcs = [{"U": ("fixedValue", np.zeros(3)), "T": ("fixedValue", 310.0), "p": ("fixedGradient", 0.02)},
           {"U": ("zeroGradient", None), "T": ("zeroGradient", None), "p": ("fixedValue", 0.0)},
           {"U": ("slip", None), "T": ("zeroGradient", None), "p": ("none", None)},
           {"U": ("fixedValue", np.ones(3)), "T": ("zeroGradient", None), "p": ("fixedGradient", None)}] + [{"U": ("none", None), "T": ("none", None), "p": ("none", None)}] * 2
    return mesh, bcs


def patch_slices(mesh):
    ps, pz = mesh.array("patchStart"), mesh.array("patchSize")
    return {n: slice(int(ps[i]) - mesh.nInternalFaces, int(ps[i]) - mesh.nInternalFaces + int(pz[i])) for i, n in enumerate(mesh.patch_names)}


def test_write_qhd_time_reads_back_bit_for_bit(tmp_path):
    mesh, bcs = small_mesh()
    case = FieldCase(mesh)
    ff.write_qhd_time(case, str(tmp_path), "0.5", bcs)
    assert sorted(os.listdir(tmp_path / "0.5")) == ["T", "U", "p"]
    sl = patch_slices(mesh)
    for name in ("U", "T", "p"):
        vals, patches = ff.read_field(str(tmp_path / "0.5" / name), mesh)
        assert np.array_equal(vals.reshape(case.field(name).shape), case.field(name)), name
        for pn in ("left", "right", "lid"):
            want = case.field(name + ".boundary")[sl[pn]]
            assert np.array_equal(patches[pn]["value"].reshape(want.shape), want), (name, pn)
        # constraint patches: their own word, no value
        assert patches["mirror"]["type"] == "symmetryPlane" and patches["mirror"]["value"] is None and "gradient" not in patches["mirror"]
        assert patches["front"]["type"] == "empty" and patches["front"]["value"] is None
        text = (tmp_path / "0.5" / name).read_text()
        assert "    mirror\n    {\n        type            symmetryPlane;\n    }\n" in text
    _, pp = ff.read_field(str(tmp_path / "0.5" / "p"), mesh)
    assert pp["left"]["type"] == "fixedGradient" and np.all(pp["left"]["gradient"] == 0.02) and pp["left"]["gradient"].shape == (2, 1)
    assert pp["lid"]["type"] == "fixedGradient" and np.all(pp["lid"]["gradient"] == 0.0)       # a gradient of None is written as 0
    assert pp["right"]["type"] == "fixedValue" and "gradient" not in pp["right"]
    assert "dimensions      [0 2 -2 0 0 0 0];" in (tmp_path / "0.5" / "p").read_text()        # kinematic pressure
    _, pu = ff.read_field(str(tmp_path / "0.5" / "U"), mesh)
    assert (pu["left"]["type"], pu["right"]["type"]) == ("fixedValue", "zeroGradient")
    # without boundary conditions every patch value is `calculated`
    ff.write_qhd_time(case, str(tmp_path), "0.6")
    _, pt = ff.read_field(str(tmp_path / "0.6" / "T"), mesh)
    assert pt["left"]["type"] == "calculated" and pt["mirror"]["type"] == "symmetryPlane"
    assert np.array_equal(pt["left"]["value"][:, 0], case.field("T.boundary")[sl["left"]])


def test_write_srf_time_writes_urel_and_the_absolute_velocity(tmp_path):
    mesh, bcs = small_mesh()
    case = FieldCase(mesh)
    omega, origin = np.array([0.0, 0.0, 2.0]), np.array([0.5, 0.25, 0.0])
    ff.write_srf_time(case, str(tmp_path), "1", {"omega": omega, "origin": origin}, bcs)
    assert sorted(os.listdir(tmp_path / "1")) == ["T", "Uabs", "Urel", "p"]
    urel, _ = ff.read_field(str(tmp_path / "1" / "Urel"), mesh)
    assert np.array_equal(urel, case.field("U")) and "object      Urel;" in (tmp_path / "1" / "Urel").read_text()
    uabs, patches = ff.read_field(str(tmp_path / "1" / "Uabs"), mesh)
    C, Cf = mesh.array("C").reshape(-1, 3), mesh.array("Cf").reshape(-1, 3)[mesh.nInternalFaces:]
    assert np.array_equal(uabs, case.field("U") + np.cross(omega, C - origin))
    want = case.field("U.boundary") + np.cross(omega, Cf - origin)
    for pn, sl in patch_slices(mesh).items():
        if pn in ("left", "right", "lid"):
            assert patches[pn]["type"] == "calculated" and np.array_equal(patches[pn]["value"], want[sl]), pn
        else:
            assert patches[pn]["type"] in ("symmetryPlane", "empty") and patches[pn]["value"] is None


def test_cell_field_writer_stays_where_the_application_had_it(tmp_path):
    from qgdsolver_amd import QGDFoam
    assert QGDFoam._write_cell_fields is ff.write_cell_fields and QGDFoam.time_name is apprun.time_name
    assert QGDFoam.find_start_time is apprun.find_start_time
    mesh, bcs = small_mesh()
    data = {"T": np.arange(4.0), "rho": np.ones(4), "ScQGD": np.full(4, 0.5)}
    ff.write_cell_fields(str(tmp_path), "2", data, bcs, mesh, {"ScQGD": 0.5, "minSc": 0.75, "maxSc": -1.0})
    _, pt = ff.read_field(str(tmp_path / "2" / "T"), mesh)
    assert pt["left"]["type"] == "fixedValue" and np.all(pt["left"]["value"] == 310.0) and pt["right"]["value"] is None
    _, pr = ff.read_field(str(tmp_path / "2" / "rho"), mesh)
    assert pr["left"]["type"] == "calculated" and pr["left"]["value"] is None and pr["mirror"]["type"] == "symmetryPlane"
    _, psc = ff.read_field(str(tmp_path / "2" / "ScQGD"), mesh)
    assert psc["lid"]["type"] == "calculated" and np.all(psc["lid"]["value"] == 0.75)            # clipped like the field


# ---- 3. the thermo block of the QHD family ------------------------------------------------------------------------------------------------
def test_qhd_and_scalar_readers_share_the_thermo_block(tmp_path):
    qhd, scalar = str(tmp_path / "qhd"), str(tmp_path / "scalar")
    os.makedirs(scalar)
    mesh = write_cavity_case(qhd, implicit_line="implicitDiffusion off;", closure="T0byGr")
    smesh, _, _ = write_scalar_case(scalar)
    tp = os.path.join("constant", "thermophysicalProperties")
    text = open(os.path.join(qhd, tp)).read()
    open(os.path.join(scalar, tp), "w").write(text)
    ff.write_field(os.path.join(qhd, "0", "alphaQGD"), mesh, "alphaQGD", np.full(mesh.nCells, 0.3), {pn: ("calculated", None) for pn in mesh.patch_names})
    ff.write_field(os.path.join(scalar, "0", "alphaQGD"), smesh, "alphaQGD", np.full(smesh.nCells, 0.3), {pn: ("calculated", None) for pn in smesh.patch_names})
    oq, os_ = ff.read_qhd_case_setup(qhd)[1], ff.read_scalar_case_setup(scalar)[1]
    shared = ("rho0", "mu", "Pr", "implicitDiffusion", "tauModel", "aQGD", "T0", "Gr")
    assert [oq[k] for k in shared] == [os_[k] for k in shared] == [1.2, 1.8e-2, 0.71, 0, "T0byGr", 0.3, 1.5, 400.0]
    assert oq["beta"] == 3.4e-3 and oq["pRefCell"] == 17 and "beta" not in os_ and "pRefCell" not in os_
    # refusals name the application
    for case_dir, read, app in ((qhd, ff.read_qhd_case_setup, "QHDFoam"), (scalar, ff.read_scalar_case_setup, "scalarTransportQHDFoam")):
        path = os.path.join(case_dir, tp)
        open(path, "w").write(text.replace("QGDCoeffs T0byGr;", "QGDCoeffs constScPrModel1;"))
        with pytest.raises(ff.FoamFileError) as ei:
            read(case_dir)
        assert str(ei.value) == f"QGDCoeffs 'constScPrModel1' is not a closure of the {app} path (constTau, HbyUQHD, T0byGr, H2bynuQHD)"
        open(path, "w").write(text.replace("equationOfState rhoConst;", "equationOfState perfectGas;"))
        with pytest.raises(ff.FoamFileError) as ei:
            read(case_dir)
        assert str(ei.value) == f"thermoType.equationOfState 'perfectGas' is not supported by the {app} path (only rhoConst)"
        open(path, "w").write(text.replace("Gr 400;", ""))
        with pytest.raises(ff.FoamFileError, match="QGD.T0byGr: entry 'Gr' is missing"):
            read(case_dir)
        open(path, "w").write(text)
        a = np.full(mesh.nCells, 0.3)
        a[1] = 0.4
        m = mesh if case_dir == qhd else smesh
        ff.write_field(os.path.join(case_dir, "0", "alphaQGD"), m, "alphaQGD", a[:m.nCells], {pn: ("calculated", None) for pn in m.patch_names})
        with pytest.raises(ff.FoamFileError, match=f"a non-uniform alphaQGD is not supported by the {app} path"):
            read(case_dir)


def test_solver_entries_keep_each_readers_rule():
    solvers = {"p": {"tolerance": 1e-8, "relTol": 0.01}, "(U|e)": {"tolerance": 1e-7, "maxIter": 20}, "U.air": {"tolerance": 1e-9}, "T": {"maxIter": 7},
               "(T|k)": {"tolerance": 1e-5}, "Ux": "PCG", "pFinal": {"tolerance": 1e-3}}
    names = lambda fields, **kw: [ff._tol_iter(e) for e in ff._solver_entries(solvers, fields, **kw)]      # noqa: E731
    assert names(("U", "e", "Ux", "Uy", "Uz"), prefixes=("U.", "e.")) == [(1e-7, 20), (1e-9, 1000)]         # QGDFoam
    assert names(("U", "T", "Ux", "Uy", "Uz")) == [(1e-7, 20), (1e-6, 7), (1e-5, 1000)]                     # QHDFoam's U and T
    assert names(("p",)) == [(1e-8, 1000)] and names(("T",))[-1] == (1e-5, 1000)                            # QHDFoam's p; the scalar's last T entry
    assert ff._solver_entries("none", ("p",)) == [] and ff._solver_entries({}, ("p",)) == []
