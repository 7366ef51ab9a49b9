"""``python -m qgdsolver_amd.QHDFoam -case <dir>``: the QHDFoam application (QHDFoam.C L63-139) run from an OpenFOAM case
directory on one MI355X.

What the reference's ``main`` does per step -- updateFields.H, updateFluxes.H, QHDpEqn.H, QHDUEqn.H, QHDTEqn.H (either branch of
implicitDiffusion; the reference's default is true), the reference level of p, runTime.write() -- is ``QHDFoamCase.step`` plus
``foamfile.write_qhd_time`` here, inside ``apprun.run_qhd``.  Read from system/controlDict (apprun.run_control): startFrom/startTime,
endTime, deltaT, writeControl (timeStep, or runTime/adjustableRunTime), writeInterval, timePrecision, and of ``functions{}`` the types
probes, fieldMinMax, qhdIntegrals, qhdPatchFluxes and qhdContinuityErrors (foamfile.read_qhd_functions; files under postProcessing/);
adjustTimeStep, maxCo, maxDeltaT, cTau [QHDFoam.C L104-106: readTimeControls.H, QHDCourantNo.H, setDeltaT-QGDQHD.H] -- with
``adjustTimeStep yes`` the case sets deltaT on every step (QHDFoamCase.set_time_control), the run ends with the first step at or
beyond endTime, writeControl must be timeStep, and a restart begins from controlDict's deltaT.  One rank; a decomposed run goes through
``bench.py --workload qhd --gpus N`` / ``qgd_qhd_case_step_sharded``.
"""
import os
import sys

from . import apprun
from . import foamfile as ff


def run(case_dir, n_steps=None, device_id=0, write=True, log=print):
    def assemble(t0_name):
        mesh, opt, fields, bcs, tc = ff.read_qhd_case_setup(case_dir, t0_name, time_control=True)
        # QGD_QHD_FUSED=1: the cell blocks of QGDFoam's one-launch step carry QHDFoam's explicit U and T equations on 3-D GaussVolPoint cases (off
        # by default: no gain measured); otherwise QHDFoam has no use for their tables
        blocks = (os.environ.get("QGD_QHD_FUSED", "0") == "1" and opt["stencil"] == "GaussVolPoint" and not opt.get("implicitDiffusion")
                  and mesh.nGeometricD == 3)
        dev, case = ff.assemble_qhd_case(mesh, opt, fields, bcs, device_id, fused_tables=blocks)
        return dev, case, opt, (), lambda name: ff.write_qhd_time(case, case_dir, name, bcs), tc

    def summary(case):
        T = case.field("T")
        return "T", T, f"max/min of T: {T.max():.9g}/{T.min():.9g}"   # QHDTEqn.H L94

    return apprun.run_qhd("QHDFoam", "U / T", case_dir, n_steps, write, log, assemble, summary)


def main(argv=None):
    return apprun.main("QHDFoam", __doc__, run, argv=argv)


if __name__ == "__main__":
    sys.exit(main())
