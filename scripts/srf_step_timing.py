"""wall time of the resident step on an n^3 box, plain QHDFoam case against the rotating-frame one (qgd_qhd_case_set_srf: Coriolis force,
T frozen), both branches of implicitDiffusion, alternated in one process after a warm-up; every timed run ends in a synchronise
(qgd_qhd_case_step waits for the stream).  The workload is bench.py's `--workload qhd` (secondary.qhd_n200: buoyant cavity, 200^3
cells), the rotating case the same cavity turning about an oblique axis.  usage  srf_step_timing.py [n = 200] [steps = 20] [rounds = 3]
The two cases run different flows, so their pressure solves take different numbers of iterations: the line gives the whole step, the
pressure solve of the last step and the rest (flux assembly, U / T equations), which is what the rotating-frame kernels change."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qgdsolver_amd as q
from qgdsolver_amd import qhdfoam
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
OMEGA = (3.0, -4.0, 4.4)
mesh = q.PolyMesh.box(n, n, n)
h = 1.0 / n
dev = q.Device(mesh, fused_tables=False)
C = mesh.array("C").reshape(-1, 3)
U = np.zeros((mesh.nCells, 3))
U[:, 0] = 0.1 * np.sin(np.pi * C[:, 0]) * np.cos(np.pi * C[:, 1])
U[:, 1] = -0.1 * np.cos(np.pi * C[:, 0]) * np.sin(np.pi * C[:, 1])
T = 300.0 + 10.0 * (0.5 - C[:, 0]) + 0.1 * np.random.default_rng(5).standard_normal(mesh.nCells)
p = np.zeros(mesh.nCells)
WALL = dict(U=("fixedValue", (0.0, 0.0, 0.0)), p=("qhdFluxCoupled", None))
for implicit in (0, 1):
    cases = {}
    for name in ("plain", "srf"):
        opt = qhdfoam.qhd_options(stencil="GaussVolPoint", tauModel="HbyUQHD", aQGD=0.5, UQHD=0.1, rho0=1.0, mu=1e-3, Pr=0.71, beta=3.4e-3,
                                  g=(0.0, -9.81, 0.0), deltaT=0.02 * h / 0.1, pTol=1e-8, pMaxIter=300, pRefCell=0, implicitDiffusion=implicit,
                                  implicitTol=1e-10, implicitMaxIter=1000)
        c = qhdfoam.QHDFoamCase(dev, opt)
        if name == "srf":
            c.set_srf(OMEGA)
        for ip in range(mesh.nPatches):
            c.set_bc(ip, T=("fixedValue", 310.0) if ip == 0 else (("fixedValue", 290.0) if ip == 1 else ("zeroGradient", None)), **WALL)
        c.set_fields(U, T, p)
        c.step(10)   # warm-up
        cases[name] = c
    for r in range(rounds):
        for name, c in cases.items():
            t0 = time.perf_counter(); c.step(steps); ms = (time.perf_counter() - t0) / steps * 1e3
            i = c.info()
            extra = ""
            if implicit:
                s = c.implicit_info()["solves"]
                extra = "  U/T iterations " + "/".join(str(s[k]["iterations"]) for k in ("Ux", "Uy", "Uz", "T"))
            print(f"{n}^3 implicitDiffusion={implicit} round {r} {name:5s}: {ms:8.2f} ms/step  p solve {i['pSolveMs']:7.2f} ms ({i['pIterations']} it)  "
                  f"rest {ms - i['pSolveMs']:7.2f} ms{extra}", flush=True)
    for name, c in cases.items():
        Un = c.field("U")
        assert np.isfinite(Un).all() and np.abs(Un).max() < 10.0, name
        print(f"{n}^3 implicitDiffusion={implicit} {name:5s}: max |U| {np.abs(Un).max():.4f} after {10 + rounds * steps} steps", flush=True)
        c.close()
dev.close()
