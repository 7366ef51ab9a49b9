"""time of the resident scalarTransportQHDFoam step on an n^3 box, next to the only way the tree could do that step before: the flux pieces
through host pointers every step (qhdfoam.updateFluxes, what config 1's GPU arm does):  scalar_step_timing.py [n] [steps] [warmup] [out]

Writes `out` (default profiles/scalar_n<n>_step.txt).  The step time is wall clock around ONE qgd_scalar_case_step(steps) call, which queues
every launch of the steps and ends in a single stream synchronisation; the per-kernel split is not measured here (rocprofv3 --kernel-trace
--stats on this script gives it).  The byte count is DESIGN.md's ("scalarTransportQHDFoam: the static / per-step split").
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import qgdsolver_amd as q
from qgdsolver_amd import qhdfoam, scalarfoam

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 10
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", f"scalar_n{n}_step.txt")
BYTES_FIXED, BYTES_PER_ITER = 696.0, 112.0      # per cell and step / per cell and solver iteration
PEAK, ACHIEVABLE = 8.0e12, 6.3e12               # HBM3E of the MI355X: peak, and what a streaming copy achieves on it

mesh = q.PolyMesh.box(n, n, n)
C = mesh.array("C").reshape(-1, 3)
U = np.stack([1.0 + 0.3 * np.sin(2.0 * C[:, 0] + C[:, 1]), 0.2 * np.cos(3.0 * C[:, 1] + C[:, 0]), 0.1 + 0.15 * C[:, 0] * C[:, 2]], axis=1)
T = 1.0 + 0.5 * np.sin(3.0 * C[:, 0]) * np.cos(2.0 * C[:, 1]) + 0.2 * C[:, 2]
dev = q.Device(mesh, fused_tables=False)
lines = [f"scalarTransportQHDFoam resident step, {n}^3 box ({mesh.nCells} cells), GaussVolPoint, mu > 0, {steps} steps after {warm}; one box, one run"]
case = scalarfoam.ScalarTransportQHDCase(dev, scalarfoam.scalar_options(stencil="GaussVolPoint", tauModel="constTau", Tau=1e-4, mu=1e-3, Pr=0.7,
                                                                         deltaT=0.1 / n, implicitTol=1e-10))
case.set_bc(0, U=("fixedValue", (1.0, 0.0, 0.0)), T=("fixedValue", 1.3))
case.set_fields(U, T)
case.step(warm)
t0 = time.perf_counter(); case.step(steps); ms = (time.perf_counter() - t0) / steps * 1e3
info = case.info()
it = info["iterations"]
byt = (BYTES_FIXED + BYTES_PER_ITER * it) * mesh.nCells
lines.append(f"resident: {ms:.3f} ms/step (wall clock around one call of {steps} steps, one synchronisation at its end)")
lines.append(f"  solver: {info['solver']}, {it} iterations in the last step, final residual {info['finalResidual']:.3g}, unconverged steps {info['unconverged_steps']}")
lines.append(f"  bytes per cell-step by DESIGN.md: {BYTES_FIXED:.0f} + {BYTES_PER_ITER:.0f} x {it} iterations = {byt / mesh.nCells:.0f} -> {byt / (ms * 1e-3) / 1e12:.3f} TB/s "
             f"= {byt / (ms * 1e-3) / PEAK:.1%} of 8 TB/s, {byt / (ms * 1e-3) / ACHIEVABLE:.1%} of the ~6.3 TB/s a streaming copy achieves")
assert np.isfinite(case.field("T")).all()
case.close()
# the per-step pieces through host pointers (the flux part of config 1's GPU arm at this size; its host solve is not comparable and not run)
nb = mesh.nBoundaryFaces
Ub = np.tile([1.0, 0.0, 0.0], (nb, 1)); Tb = np.ones(nb)
rho = (np.ones(mesh.nCells), np.ones(nb)); tau = np.full(mesh.nFaces, 1e-4)
reps = 3
qhdfoam.updateFluxes(dev, "GaussVolPoint", (U, Ub), (T, Tb), rho, tau, 0.0, (0, 0, 0))
t0 = time.perf_counter()
for _ in range(reps):
    qhdfoam.updateFluxes(dev, "GaussVolPoint", (U, Ub), (T, Tb), rho, tau, 0.0, (0, 0, 0))
ms_host = (time.perf_counter() - t0) / reps * 1e3
lines.append(f"host-pointer flux pieces (qhdfoam.updateFluxes per step, {reps} calls): {ms_host:.1f} ms/call -> resident step is {ms_host / ms:.0f}x below it")
dev.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
open(out_path, "w").write("\n".join(lines) + "\n")
print("\n".join(lines), flush=True)
