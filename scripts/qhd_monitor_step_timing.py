"""What the QHD run monitor costs on an n^3 box (bench.py's buoyant cavity: GaussVolPoint, HbyUQHD, pressure equation to 1e-8): ms per
step without a monitor, sampling after every step and after every 10th step, alternating inside one call, for the explicit branch and for
implicitDiffusion; and the time of one sample (cell pass + patch pass + fold + the copy).  The QHD step waits for its pressure solve on the
host, so a step is timed by the host clock around ``case.step(1)``; the samples are read two behind, as the applications do.  One sample is
timed as a burst: 50 samples enqueued back to back on an idle stream, the last one read, the span divided by 50 (the enqueue of a sample
takes the host less than the device takes to run it at this size, so the span is the device's).  Writes
profiles/qhd_monitor_step_cost.txt.
    python scripts/qhd_monitor_step_timing.py [n=200] [steps=30] [warmup=10]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qgdsolver_amd as q  # noqa: E402
from qgdsolver_amd import _lib as L  # noqa: E402
from qgdsolver_amd import qhdfoam  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 10
BURST = 50
# per owned cell: the {U,T} record 32 + p 8 + V 8 + the face count 1 (the issue's "about 50 B of records"), six face items 24 and six
# gathers of phi 48 on a hexahedron (every face's phi is gathered by both of its cells)
ESTIMATE = 32 + 8 + 8 + 1 + 6 * 4 + 6 * 8

if q.device_count() < 1:
    raise SystemExit("qhd_monitor_step_timing.py: no HIP device (a timing needs the GPU)")

mesh = q.PolyMesh.box(n, n, n)
h = 1.0 / n
C = mesh.array("C").reshape(-1, 3)
rng = np.random.default_rng(5)
U = np.zeros((mesh.nCells, 3))
U[:, 0] = 0.1 * np.sin(np.pi * C[:, 0]) * np.cos(np.pi * C[:, 1])
U[:, 1] = -0.1 * np.cos(np.pi * C[:, 0]) * np.sin(np.pi * C[:, 1])
T = 300.0 + 10.0 * (0.5 - C[:, 0]) + 0.1 * rng.standard_normal(mesh.nCells)
p = np.zeros(mesh.nCells)
del C
dev = q.Device(mesh, fused_tables=False)
WALL = dict(U=("fixedValue", (0.0, 0.0, 0.0)), T=("zeroGradient", None), p=("qhdFluxCoupled", None))
probes = [0, mesh.nCells // 3, mesh.nCells // 2, mesh.nCells - 1]


def open_case(implicit):
    opt = qhdfoam.qhd_options(stencil="GaussVolPoint", tauModel="HbyUQHD", aQGD=0.5, UQHD=0.1, rho0=1.0, mu=1e-3, Pr=0.71, beta=3.4e-3,
                              g=(0.0, -9.81, 0.0), deltaT=0.02 * h / 0.1, pTol=1e-8, pMaxIter=300, pRefCell=0,
                              implicitDiffusion=implicit, implicitTol=1e-10, implicitMaxIter=1000)
    case = qhdfoam.QHDFoamCase(dev, opt)
    for ip in range(mesh.nPatches):
        case.set_bc(ip, U=WALL["U"], T=("fixedValue", 310.0) if ip == 0 else (("fixedValue", 290.0) if ip == 1 else WALL["T"]), p=WALL["p"])
    case.set_fields(U, T, p)
    return case


lines = [f"QHD run monitor on a {n}^3 box ({mesh.nCells} cells), bench.py's buoyant cavity, GaussVolPoint, pressure equation to 1e-8; "
         f"{steps} steps after {warmup}; probes 4, patches 6; {L.lib.qgd_version().decode()}"]
modes = (("no monitor", 0), ("every step", 1), ("every 10th", 10))
for implicit, branch in ((0, "explicit branch"), (1, "implicitDiffusion")):
    ms = {m[0]: [] for m in modes}
    sample_ms = []
    lines.append(f"{branch}:")
    for rep in range(3):
        for name, every in modes:
            case = open_case(implicit)
            mon = case.monitor(probes=probes, patches=range(6)) if every else None
            case.step(warmup)
            if mon:
                mon.sample()
                mon.read()
            case.sync()
            t0 = time.perf_counter()
            for k in range(1, steps + 1):
                case.step(1)
                if mon and k % every == 0:
                    mon.sample()
                    if len(mon._pending) > 2:
                        mon.read()
            case.sync()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
            if mon:
                while mon._pending:
                    last = mon.read()
                assert last["nonFinite"] == 0 and last["step"] == warmup + steps and last["fluxState"] == (2 if implicit else 1), last
                if every == 1:
                    case.sync()
                    t0 = time.perf_counter()
                    for _ in range(BURST):
                        slot = mon.sample()
                    mon.read(slot)
                    sample_ms.append((time.perf_counter() - t0) / BURST * 1e3)
            info = case.info()
            lines.append(f"  run {rep} {name:<11} {ms[name][-1]:8.4f} ms/step  (pressure iterations of the last step {info['pIterations']})")
            case.close()
    best = {k: min(v) for k, v in ms.items()}
    s = min(sample_ms)
    base = best["no monitor"]
    lines.append(f"  ms per step (best of 3): no monitor {base:.4f}, every step {best['every step']:.4f} ({(best['every step'] / base - 1) * 100:+.1f} %), "
                 f"every 10th {best['every 10th']:.4f} ({(best['every 10th'] / base - 1) * 100:+.1f} %)")
    lines.append(f"  one sample (three launches + the copy; a burst of {BURST} back to back, best of 3 runs): {s:.4f} ms = {s / base * 100:.1f} % of a step")
    lines.append(f"  estimate {ESTIMATE} B per owned cell: {ESTIMATE * mesh.nCells / s / 1e6:.0f} GB/s if the cell pass moved exactly that")
dev.close()
lines.append("(hardware byte counters were not collected: they want a counter run of their own)")
out = os.path.join(ROOT, "profiles", "qhd_monitor_step_cost.txt")
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
