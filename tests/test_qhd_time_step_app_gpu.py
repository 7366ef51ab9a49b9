"""QHDFoam and SRFQHDFoam from a written case with ``adjustTimeStep yes`` [QHDFoam.C L104-106, SRFQHDFoam.C L114-116]: the time
directories carry the accumulated times, the last one is a QHDFoamCase driven by hand with the same control (bit for bit), every step
prints the listing's three lines, -nSteps cuts by count, writeControl runTime is refused with apprun.ADJUST_REFUSAL."""
import os
import re

import numpy as np
import pytest

from qgdsolver_amd import QHDFoam, SRFQHDFoam, apprun, foamfile as ff

from srf_ref import write_srf_case
from test_qhdfoam_case import write_cavity_case

pytestmark = pytest.mark.gpu

MAX_CO, MAX_DT, END = 4e-4, 5e-3, 0.012


def edit(path, pairs):
    text = open(path).read()
    for a, b in pairs:
        assert text.count(a) == 1, a
        text = text.replace(a, b)
    open(path, "w").write(text)


def adjusted_cavity(case_dir, write_control="timeStep"):
    """the written cavity without buoyancy, stirred at the start (the flow decays), deltaT ten times what maxCo allows"""
    mesh = write_cavity_case(case_dir, implicit_line="implicitDiffusion false;")
    edit(os.path.join(case_dir, "constant", "thermophysicalProperties"), [("beta 3.4e-3;", "beta 0;")])
    U = 5e-2 * np.random.default_rng(4).standard_normal((mesh.nCells, 3))
    rows = "\n".join(f"({float(u[0])!r} {float(u[1])!r} {float(u[2])!r})" for u in U)
    edit(os.path.join(case_dir, "0", "U"), [("internalField uniform (0 0 0);", f"internalField nonuniform List<vector>\n{mesh.nCells}\n(\n{rows}\n)\n;")])
    edit(os.path.join(case_dir, "system", "controlDict"),
         [("deltaT 1e-3;", "deltaT 1e-2;"), ("writeControl timeStep;\nwriteInterval 6;", f"writeControl {write_control};\nwriteInterval 4;"),
          ("timePrecision 8;", f"timePrecision 8;\nadjustTimeStep yes;\nmaxCo {MAX_CO};\nmaxDeltaT {MAX_DT};\n")])
    return mesh


def by_hand(load, end=END, n_steps=None):
    """(case, the time after every step) of a case stepped one step at a time to the first time at or beyond `end`, or n_steps steps"""
    dev, case, tc = load()
    case.set_time_control(True, tc["maxCo"], tc["maxDeltaT"], tc["cTau"])
    times = []
    while (n_steps is None and (not times or times[-1] < end - 1e-12 * max(1.0, abs(end)))) or (n_steps is not None and len(times) < n_steps):
        case.step(1)
        times.append(case.info()["time"])
    return dev, case, times


def time_dirs(case_dir):
    return sorted((d for d in os.listdir(case_dir) if re.fullmatch(r"[0-9.e+-]+", d)), key=float)


def test_qhdfoam_runs_an_adjusted_case(tmp_path, capsys):
    case_dir = str(tmp_path)
    adjusted_cavity(case_dir)

    def load():
        mesh, opt, fields, bcs, tc = ff.read_qhd_case_setup(case_dir, "0", time_control=True)
        assert tc == dict(adjustTimeStep=True, maxCo=MAX_CO, maxDeltaT=MAX_DT, cTau=0.75)
        return ff.assemble_qhd_case(mesh, opt, fields, bcs, fused_tables=False) + (tc,)

    dev, gc, times = by_hand(load)
    assert len(times) > 8 and times[-2] < END <= times[-1] + 1e-14
    assert QHDFoam.main(["-case", case_dir]) == 0
    out = capsys.readouterr().out
    # the time directories: every fourth step and the last one, at the accumulated times
    want = [apprun.time_name(t, 8) for i, t in enumerate(times) if (i + 1) % 4 == 0 or i + 1 == len(times)]
    assert time_dirs(case_dir) == ["0"] + want, (time_dirs(case_dir), want)
    assert out.rstrip().endswith("End") and f"steps {len(times)}" in out
    for name in ("U", "T", "p"):
        vals, _ = ff.read_field(os.path.join(case_dir, want[-1], name), gc.mesh)
        ref = gc.field(name)
        assert np.abs(ref).max() > 0 and np.array_equal(vals.reshape(ref.shape), ref), name
    # the listing's three lines, once per step; the Courant number at most maxCo once the too-large deltaT has been cut
    co = [float(x) for x in re.findall(r"^Courant Number = (\S+)$", out, flags=re.M)]
    dts = [float(x) for x in re.findall(r"^deltaT = (\S+)$", out, flags=re.M)]
    m1 = [float(x) for x in re.findall(r"^maxDeltaT1 = (\S+)$", out, flags=re.M)]
    print("Courant numbers", co, "deltaT", dts)
    assert len(co) == len(dts) == len(m1) == len(times)
    assert co[0] > 5 * MAX_CO and all(c <= MAX_CO * (1 + 1e-5) for c in co[3:]), co     # (printed with six digits)
    assert all(abs(d - (b - a)) <= 1e-5 * d for d, a, b in zip(dts, [0.0] + times, times)) and set(m1) == {MAX_DT}
    gc.close(); dev.close()
    # -nSteps cuts by count
    for d in want:
        for f in os.listdir(os.path.join(case_dir, d)):
            os.remove(os.path.join(case_dir, d, f))
        os.rmdir(os.path.join(case_dir, d))
    assert QHDFoam.main(["-case", case_dir, "-nSteps", "5"]) == 0
    out = capsys.readouterr().out
    assert time_dirs(case_dir) == ["0"] + [apprun.time_name(times[i], 8) for i in (3, 4)] and "steps 5" in out and "steps 6" not in out
    assert len(re.findall(r"^Courant Number = ", out, flags=re.M)) == 5


def test_run_time_write_control_is_refused_under_adjust_time_step(tmp_path):
    case_dir = str(tmp_path)
    adjusted_cavity(case_dir, write_control="runTime")
    with pytest.raises(ff.FoamFileError) as e:
        QHDFoam.main(["-case", case_dir, "-noWrite"])
    assert apprun.ADJUST_REFUSAL in str(e.value)


def test_srfqhdfoam_runs_an_adjusted_case(tmp_path, capsys):
    case_dir = str(tmp_path)
    write_srf_case(case_dir)
    edit(os.path.join(case_dir, "system", "controlDict"), [("timePrecision 8;", "timePrecision 8;\nadjustTimeStep yes;\nmaxCo 0.05;\nmaxDeltaT 2e-3;\n")])

    def load():
        mesh, opt, fields, bcs, srf, tc = ff.read_srf_case_setup(case_dir, "0", time_control=True)
        assert tc == dict(adjustTimeStep=True, maxCo=0.05, maxDeltaT=2e-3, cTau=0.75)
        return ff.assemble_qhd_case(mesh, opt, fields, bcs, fused_tables=False, omega=srf["omega"]) + (tc,)

    dev, gc, times = by_hand(load, end=0.006)
    assert gc.srf_info()["rotating"] and len(times) >= 3
    assert SRFQHDFoam.main(["-case", case_dir]) == 0
    out = capsys.readouterr().out
    want = [apprun.time_name(t, 8) for i, t in enumerate(times) if (i + 1) % 3 == 0 or i + 1 == len(times)]
    assert time_dirs(case_dir) == ["0"] + want, (time_dirs(case_dir), want)
    for name, field in (("Urel", "U"), ("p", "p")):
        vals, _ = ff.read_field(os.path.join(case_dir, want[-1], name), gc.mesh)
        ref = gc.field(field)
        assert np.abs(ref).max() > 0 and np.array_equal(vals.reshape(ref.shape), ref), name
    assert len(re.findall(r"^Courant Number = ", out, flags=re.M)) == len(times) and len(set(np.diff([0.0] + times).round(12))) > 1
    gc.close(); dev.close()
