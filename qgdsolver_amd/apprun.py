"""What the case-directory applications (QGDFoam, QHDFoam, SRFQHDFoam, scalarTransportQHDFoam) share on the host: the name of a time
directory and the start time, the run control of system/controlDict (``run_control``), the report of the implicit solves
(``log_implicit_solves``), the stepping that stops where a function object is due (``stepping``), the loop "advance a chunk, report,
write" (``step_chunks``), the QHD family's run around it (``run_qhd``) and the command line (``main``).  Nothing in here opens a
device: the cases and the function objects come in from the caller.
"""
import argparse
import os
import time as _time

import numpy as np

from . import foamfile as ff


def time_name(t, precision=6):
    """Time::timeName(): general format with timePrecision significant digits (L0)"""
    s = f"{t:.{precision}g}"
    if "e" in s:
        m, e = s.split("e")
        s = f"{m}e{int(e):+03d}"
    return s


def find_start_time(case_dir, cd):
    start_from = str(cd.get("startFrom", "startTime"))
    times = []
    for d in os.listdir(case_dir):
        try:
            times.append((float(d), d))
        except ValueError:
            pass
    if not times:
        raise ff.FoamFileError(f"{case_dir}: no time directory")
    if start_from == "latestTime":
        return max(times)
    if start_from == "firstTime":
        return min(times)
    want = float(cd.get("startTime", 0))
    for t, d in times:
        if abs(t - want) <= 1e-12 * max(1.0, abs(want)):
            return t, d
    raise ff.FoamFileError(f"{case_dir}: no time directory for startTime {want}")


RUN_TIME_REFUSAL = "is not supported (timeStep, runTime, adjustableRunTime)"
ADJUST_REFUSAL = "with adjustTimeStep is not supported (use writeControl timeStep)"


def run_control(cd, t0, n_steps=None, adjust=False, refusal=RUN_TIME_REFUSAL, run_time=True):
    """(deltaT, endTime, chunk, timePrecision, total) of a run from t0: chunk is the number of steps between two writes (writeControl
    timeStep: writeInterval; runTime / adjustableRunTime, where ``run_time`` serves them: writeInterval / deltaT), total the number of
    steps to take (n_steps, else up to endTime; None under adjustTimeStep, where the time decides).  Any other writeControl is refused
    with the caller's words."""
    rc = ff.read_run_control(cd)
    dt = float(cd["deltaT"])
    if rc["writeControl"] == "timeStep":
        chunk = max(1, int(round(rc["writeInterval"])))
    elif rc["writeControl"] in ("runTime", "adjustableRunTime") and run_time:
        chunk = max(1, int(round(rc["writeInterval"] / dt)))
    else:
        raise ff.FoamFileError(f"writeControl '{rc['writeControl']}' {refusal}")
    total = n_steps if n_steps is not None else (None if adjust else int(round((rc["endTime"] - t0) / dt)))
    return dt, rc["endTime"], chunk, rc["timePrecision"], total


def log_implicit_solves(log, ii, options, worked_only=False):
    """the residuals of the implicit solves of the last step (``implicit_info()``), and how many steps so far ended unconverged or
    stalled.  worked_only (the QHD family): a solve that did not run (no iterations, no residual) is left out."""
    log("  " + "  ".join(f"{k}: {v['initial']:.3g} -> {v['final']:.3g} in {v['iterations']}" for k, v in ii["solves"].items()
                          if not worked_only or v["iterations"] or v["initial"]))
    if ii["unconverged_steps"]:
        log(f"  WARNING: {ii['unconverged_steps']} step(s) so far in which an implicit solve stopped above its tolerance "
            f"(implicitTol {options.implicitTol:g}, maxIter {options.implicitMaxIter})")
    if ii["stalled_steps"]:
        log(f"  NOTE: {ii['stalled_steps']} step(s) so far in which a Chebyshev solve ended at the rounding floor of its residual, above "
            f"implicitTol {options.implicitTol:g} (OpenFOAM would have iterated on to maxIter)")


def stepping(step, functions, t0):
    """advance(n) for a run with function objects (monitor.FunctionObjects / QHDFunctionObjects): n steps of ``step``, cut at the steps
    at which a function is due, each cut followed by one sample of the device monitor (read two samples late, flushed by
    functions.finish()).  Without functions advance is ``step`` itself."""
    if functions is None:
        return step
    taken = [0]

    def advance(n):
        while n > 0:
            k = min(n, functions.next_due(taken[0]))
            step(k)
            taken[0] += k
            n -= k
            functions.after_step(taken[0], t0)
    return advance


def step_chunks(case, advance, t0, chunk, total, precision, report, write_time=None, end_time=None):
    """The time loop: advance ``chunk`` steps (the last chunk what is left of ``total``), report(done, t, info) -- the caller's log lines
    and checks; info is case.info(), t = t0 + info["time"] -- and write_time(name) where there is one; returns the names written.
    total None (adjustTimeStep): the time is asked after every step [QGDFoam.C L90], the run ends with the first step at or beyond
    ``end_time``, and that last state is written whatever the cadence."""
    ended = None if total is not None else end_time - 1e-12 * max(1.0, abs(end_time))
    done, written = 0, []
    while total is None or done < total:
        if total is None:
            n = 0
            while n < chunk:
                advance(1)
                n += 1
                if t0 + case.info()["time"] >= ended:
                    break
        else:
            n = min(chunk, total - done)
            advance(n)
        done += n
        info = case.info()
        t = t0 + info["time"]
        report(done, t, info)
        if write_time is not None:
            name = time_name(t, precision)
            write_time(name)
            written.append(name)
        if total is None and t >= ended:
            break
    return written


def run_qhd(app, solves, case_dir, n_steps, write, log, assemble, summary):
    """The run of QHDFoam and SRFQHDFoam.  assemble(t0_name) -> (dev, case, opt, banner lines of its own, write_time(name)[, the time
    controls of foamfile.read_qhd_case_setup: without them the run has a fixed deltaT]); summary(case) -> (name, values, text): the closing line of a step's report and the field
    whose finiteness the run depends on; ``solves`` names the implicit solves in the note on their start values.
    adjustTimeStep yes [QHDFoam.C L104-106]: the case sets deltaT every step (QHDFoamCase.set_time_control), every step prints the
    listing's three lines, the run ends with the first step at or beyond endTime, and writeControl must be timeStep."""
    cd = ff.read_dict(os.path.join(case_dir, "system", "controlDict"))
    t0, t0_name = find_start_time(case_dir, cd)
    dev, case, opt, banner, write_time, *tc = assemble(t0_name)
    mesh = case.mesh
    tc = tc[0] if tc else {"adjustTimeStep": False}
    adjust = bool(tc["adjustTimeStep"])
    dt, end_time, chunk, precision, total = run_control(cd, t0, n_steps, adjust, ADJUST_REFUSAL, run_time=not adjust)
    if adjust:
        case.set_time_control(True, tc["maxCo"], tc["maxDeltaT"], tc["cTau"])
    branch = "implicitDiffusion true" if opt["implicitDiffusion"] else "implicitDiffusion false"
    log(f"{app} (qgdsolver_amd, {branch}): {mesh.nCells} cells, fvsc {opt['stencil']}, QGDCoeffs {opt['tauModel']}, deltaT {dt:g}, "
        f"start {t0_name}")
    for line in banner:
        log(line)
    px, xx = os.environ.get("QGD_QHD_PEXTRAP", "4"), os.environ.get("QGD_IMPL_XEXTRAP", "3")
    if px != "0" or (opt.get("implicitDiffusion") and xx != "0"):
        log(f"  NOTE: the pressure solve starts from p extrapolated in time over the last steps (QGD_QHD_PEXTRAP={px}, limited per value)"
            + (f", the {solves} solves from the extrapolated fields (QGD_IMPL_XEXTRAP={xx})" if opt.get("implicitDiffusion") else "")
            + ", not from the old field as OpenFOAM does [QHDpEqn.H L45]: same systems, same tolerances, same answer to those tolerances -- but "
            f"'Initial residual' and 'No Iterations' below are NOT comparable with a reference {app} log.  QGD_QHD_PEXTRAP=0 "
            "QGD_IMPL_XEXTRAP=0 restore OpenFOAM's start values.")
    # functions{} of system/controlDict (foamfile.read_qhd_functions) through the device monitor
    functions = None
    specs = ff.read_qhd_functions(cd, warn=log)
    if specs:
        from .monitor import QHDFunctionObjects
        functions = QHDFunctionObjects(case, specs, mesh, case_dir, t0_name, lambda g: g, np.arange(mesh.nCells), log=log)
    wall0 = _time.perf_counter()

    def report(done, t, info):
        name, values, text = summary(case)
        log(f"Time = {time_name(t, precision)}  steps {done}")
        log(f"  p: Initial residual = {info['pInitialResidual']:.3g}, Final residual = {info['pFinalResidual']:.3g}, No Iterations {info['pIterations']}")
        if opt["implicitDiffusion"]:
            log_implicit_solves(log, case.implicit_info(), case.options, worked_only=True)
        log(f"  {text}  ClockTime {_time.perf_counter() - wall0:.2f} s")
        if not np.isfinite(values).all():
            raise FloatingPointError(f"{name} is not finite at time {t:g}")

    def step_adjusted(n):
        for _ in range(n):
            case.step(1)
            ti = case.time_info()
            log(f"Courant Number = {ti['CoNum']:.6g}")                                      # QHDCourantNo.H L56
            log(f"maxDeltaT1 = {min(tc['maxDeltaT'], tc['cTau'] * ti['minTau']):.6g}")       # setDeltaT-QGDQHD.H L46-49
            log(f"deltaT = {ti['deltaT']:.6g}")                                             # L61

    written = step_chunks(case, stepping(step_adjusted if adjust else case.step, functions, t0), t0, chunk, total, precision, report,
                          write_time if write else None, end_time)
    if functions is not None:
        functions.finish()
    log("End")
    return dev, case, written


def main(prog, doc, run, extra_args=None, argv=None):
    """the command line of an application: -case, -nSteps, -device, -noWrite and the application's own ``extra_args`` ((flag, keywords
    of add_argument) pairs, handed to ``run`` by their dest)"""
    ap = argparse.ArgumentParser(prog=prog, description=doc.split("\n\n")[0])
    ap.add_argument("-case", dest="case", default=".")
    ap.add_argument("-nSteps", dest="n_steps", type=int, default=None, help="run this many steps instead of up to endTime")
    ap.add_argument("-device", dest="device", type=int, default=0)
    ap.add_argument("-noWrite", dest="no_write", action="store_true")
    for flag, kw in extra_args or ():
        ap.add_argument(flag, **kw)
    a = ap.parse_args(argv)
    dev, case, _ = run(a.case, a.n_steps, a.device, not a.no_write, **{kw["dest"]: getattr(a, kw["dest"]) for _, kw in extra_args or ()})
    case.close()
    dev.close()
    return 0
