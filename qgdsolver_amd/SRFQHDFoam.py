"""``python -m qgdsolver_amd.SRFQHDFoam -case <dir>``: the SRFQHDFoam application (SRFQHDFoam.C L70-154) run from an OpenFOAM case
directory on one MI355X: incompressible QHD flow in a single rotating frame.

What the reference's ``main`` does per step -- updateFields.H with BdFrc = beta*T*g - 2 (omega ^ Urel) [L73-74], updateFluxes.H,
QHDpEqn.H, QHDUEqn.H (either branch of implicitDiffusion), the reference level of p, runTime.write() -- is ``QHDFoamCase.step`` after
``set_srf`` plus ``foamfile.write_srf_time`` here, inside ``apprun.run_qhd``.  The loop has no QHDTEqn.H: T stays as read.  There is no
centrifugal term, as in the reference: p is the reduced pressure.  Read from constant/SRFProperties: SRFModel rpm, origin, axis,
rpmCoeffs.rpm; the velocity file is Urel; walls at rest in the inertial frame are SRFVelocity patches with ``relative no``.
system/controlDict as for QHDFoam: startFrom/startTime, endTime, deltaT, writeControl (timeStep, or runTime/adjustableRunTime),
writeInterval, timePrecision, ``functions{}`` as QHDFoam serves it, adjustTimeStep / maxCo / maxDeltaT / cTau [SRFQHDFoam.C
L114-116] as QHDFoam serves them.  Written per time: Urel, T, p and
Uabs = Urel + omega ^ (C - origin).  One rank.
"""
import sys

import numpy as np

from . import apprun
from . import foamfile as ff


def run(case_dir, n_steps=None, device_id=0, write=True, log=print):
    def assemble(t0_name):
        mesh, opt, fields, bcs, srf, tc = ff.read_srf_case_setup(case_dir, t0_name, time_control=True)
        dev, case = ff.assemble_qhd_case(mesh, opt, fields, bcs, device_id, fused_tables=False, omega=srf["omega"])
        w = srf["omega"]
        banner = (f"  SRFModel rpm: omega ({w[0]:.9g} {w[1]:.9g} {w[2]:.9g}) rad/s about origin ({' '.join(f'{x:g}' for x in srf['origin'])}), "
                  f"T frozen (the loop has no T equation), p is the reduced pressure (no centrifugal term)",)
        return dev, case, opt, banner, lambda name: ff.write_srf_time(case, case_dir, name, srf, bcs), tc

    def summary(case):
        U = case.field("U")
        return "Urel", U, f"max |Urel|: {np.sqrt((U * U).sum(axis=1)).max():.9g}"

    return apprun.run_qhd("SRFQHDFoam", "U", case_dir, n_steps, write, log, assemble, summary)


def main(argv=None):
    return apprun.main("SRFQHDFoam", __doc__, run, argv=argv)


if __name__ == "__main__":
    sys.exit(main())
