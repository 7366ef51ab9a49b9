"""What the varScModel7 closure costs per step on an n^3 box (GaussVolPoint, explicit branch, fixed deltaT): ms per step with the model and
with constScPrModel1 on the same tree, alternating; the sensor kernel's own time by HIP events (qgd_case_timing, QGD_K_VARSC); the bytes
per cell that time corresponds to against the estimate.  Writes profiles/var_sc_model7_step.txt.
    python scripts/var_sc_step_timing.py [n=200] [steps=100] [warmup=20]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qgdsolver_amd as q  # noqa: E402
from qgdsolver_amd import _lib as L  # noqa: E402
from qgdsolver_amd.synthetic import box_initial_fields  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 20
# per cell: 6 faces x (cfItem 4 + cfNbr 4 + w 8 + r_f 8) + the neighbours' record lines (about 64 once shared) + 8 written
ESTIMATE = 6 * (4 + 4 + 8 + 8) + 64 + 8
STEP_BYTES = 700   # what the fused step moves per cell

if q.device_count() < 1:
    raise SystemExit("var_sc_step_timing.py: no HIP device (a timing needs the GPU)")
mesh = q.PolyMesh.box(n, n, n)
U, T, p = box_initial_fields(mesh.array("C").reshape(-1, 3))
dev = q.Device(mesh)
lines = [f"varScModel7 on a {n}^3 box ({mesh.nCells} cells), GaussVolPoint, explicit, deltaT fixed; {steps} steps after {warmup}; {L.lib.qgd_version().decode()}"]
ms = {"constScPrModel1": [], "varScModel7": []}
sensor_ms = []
for rep in range(3):
    for model in ("constScPrModel1", "varScModel7"):
        case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=0.05 / n / 1.3, mu=1e-3, ScQGD=0.2))
        if model == "varScModel7":
            case.set_var_sc(ScQGD=0.2, cSc1=1.0, minSc=0.05, maxSc=1.0)
        case.set_fields(U, T, p)
        fused = case.fused_info()["fused"]
        case.step(warmup)
        t0 = time.perf_counter()
        case.step(steps)          # returns after the device has finished
        ms[model].append((time.perf_counter() - t0) / steps * 1e3)
        if model == "varScModel7":
            case.timing(True)
            case.timing_reset()
            case.step(steps)
            total, launches = case.kernel_time(L.K_VARSC)
            case.timing(False)
            assert launches == steps, (launches, steps)
            sensor_ms.append(total / launches)
            hi, lo = case.sc_range()
        info = case.info()
        assert info["minRho"] > 0, info
        lines.append(f"  run {rep} {model:<16} {ms[model][-1]:8.4f} ms/step  ({'fused step' if fused else 'separate kernels'})")
        case.close()
dev.close()
best = {k: min(v) for k, v in ms.items()}
s = min(sensor_ms)
lines.append(f"ms per step (best of 3): constScPrModel1 {best['constScPrModel1']:.4f}, varScModel7 {best['varScModel7']:.4f} "
             f"(+{(best['varScModel7'] / best['constScPrModel1'] - 1) * 100:.1f} %)")
lines.append(f"sensor kernel (HIP events, mean of {steps} launches, best of 3 runs): {s:.4f} ms; max/min ScQGD after the run {hi:.4g}/{lo:.4g}")
lines.append(f"estimate {ESTIMATE} B per cell (step: about {STEP_BYTES}): {ESTIMATE * mesh.nCells / s / 1e6:.0f} GB/s if the kernel moved exactly that; "
             f"at the step's own rate ({STEP_BYTES * mesh.nCells / best['constScPrModel1'] / 1e6:.0f} GB/s) the kernel's time is "
             f"{s * STEP_BYTES / best['constScPrModel1']:.0f} B per cell")
lines.append("(hardware byte counters were not collected: they want a counter run of their own)")
lines.append("note: the timing box's pressure pulse is smooth -- every cell sits on minSc after the run; the kernel's work does not depend on the values")
out = os.path.join(ROOT, "profiles", "var_sc_model7_step.txt")
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
