"""``python -m qgdsolver_amd.scalarTransportQHDFoam -case <dir>``: the scalarTransportQHDFoam application (scalarTransportQHDFoam.C
L60-135) run from an OpenFOAM case directory on one MI355X.

What the reference's ``main`` does -- thermo.correct() and updateFluxes.H once, then per step the Courant number and setDeltaT-QGDQHD.H
(adjustTimeStep), updateFields.H, the T equation, runTime.write() -- is ``ScalarTransportQHDCase.set_fields`` / ``step`` plus
``foamfile.write_scalar_time`` here (the case is put together by ``foamfile.assemble_scalar_case``; the loop is this module's own: it logs
every step and writes on a counter).  Read from system/controlDict (apprun.run_control): startFrom/startTime, endTime, deltaT, writeControl timeStep,
writeInterval, timePrecision, adjustTimeStep, maxCo, maxDeltaT, cTau.  The run restarts from the latest time directory (startFrom
latestTime) or from startTime.
"""
import os
import sys
import time as _time

import numpy as np

from . import apprun
from . import foamfile as ff
from .apprun import time_name


def run(case_dir, n_steps=None, device_id=0, write=True, log=print):
    cd = ff.read_dict(os.path.join(case_dir, "system", "controlDict"))
    t0, t0_name = apprun.find_start_time(case_dir, cd)
    mesh, opt, fields, bcs, _ = ff.read_scalar_case_setup(case_dir, t0_name)
    adjust = bool(opt["adjustTimeStep"])
    _, end_time, chunk, precision, total = apprun.run_control(cd, t0, n_steps, adjust, "is not supported (timeStep)", run_time=False)
    dev, case = ff.assemble_scalar_case(mesh, opt, fields, bcs, device_id)
    log(f"scalarTransportQHDFoam (qgdsolver_amd, implicitDiffusion {'true' if opt['implicitDiffusion'] else 'false'}): {mesh.nCells} cells, "
        f"fvsc {opt['stencil']}, QGDCoeffs {opt['tauModel']}, deltaT {opt['deltaT']:g}{' (adjustTimeStep)' if adjust else ''}, start {t0_name}")
    if not opt["implicitDiffusion"]:
        log("  WARNING: implicitDiffusion false: scalarTransportQHDFoam.C L113 solves the T equation only under implicitDiffusion and has no "
            "else branch -- T stays as it is and only time advances (reproduced as listed)")
    done, since_write = 0, 0
    wall0 = _time.perf_counter()
    written = []
    while (done < total) if total is not None else (t0 + case.info()["time"] < end_time - 1e-12 * max(abs(end_time), 1.0)):
        case.step(1)
        done += 1
        since_write += 1
        info = case.info()
        t = t0 + info["time"]
        T = case.field("T")
        log(f"Courant Number max: {info['CoNum']:.9g}")                              # .C L92
        log(f"deltaT = {info['deltaT']:.9g}")                                        # setDeltaT-QGDQHD.H L63
        log(f"Time = {time_name(t, precision)}")
        if opt["implicitDiffusion"]:
            log(f"Solving for T, Initial residual = {info['initialResidual']:.3g}, Final residual = {info['finalResidual']:.3g}, "
                f"No Iterations {info['iterations']}")
            if info["unconverged_steps"]:
                log(f"  WARNING: {info['unconverged_steps']} step(s) so far in which the T solve stopped above its tolerance "
                    f"(implicitTol {case.options.implicitTol:g}, maxIter {case.options.implicitMaxIter})")
        log(f"max/min of T: {T.max():.9g}/{T.min():.9g}  ClockTime {_time.perf_counter() - wall0:.2f} s")
        if not np.isfinite(T).all():
            raise FloatingPointError(f"T is not finite at time {t:g}")
        last = (done == total) if total is not None else not (t < end_time - 1e-12 * max(abs(end_time), 1.0))
        if write and (since_write == chunk or last):
            name = time_name(t, precision)
            ff.write_scalar_time(case, case_dir, name, fields["U"], bcs)
            written.append(name)
            since_write = 0
    log("End")
    return dev, case, written


def main(argv=None):
    return apprun.main("scalarTransportQHDFoam", __doc__, run, argv=argv)


if __name__ == "__main__":
    sys.exit(main())
