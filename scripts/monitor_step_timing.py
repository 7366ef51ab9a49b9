"""What a run monitor costs per step on an n^3 box (GaussVolPoint, explicit branch, fixed deltaT, the fused one-launch step): ms per step
without a monitor, sampling after every step and sampling after every 10th step, alternating inside one call; per-launch times of the
three launches of a sample (cell pass + patch pass + fold) from HIP events around them.  The steps go out as stream-ordered phases and the
samples are read two behind, as the application does, so the host never waits inside the timed span.  Writes profiles/monitor_step_cost.txt.
    python scripts/monitor_step_timing.py [n=200] [steps=100] [warmup=20]"""
import ctypes as C
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
ESTIMATE = 48 + 32 + 8 + 8   # per owned cell: RecA + RecB + rE + V (the issue's 80-100 B)

if q.device_count() < 1:
    raise SystemExit("monitor_step_timing.py: no HIP device (a timing needs the GPU)")
try:   # the runtime the library itself links: events on the case's stream
    hip = C.CDLL("libamdhip64.so")
except OSError:
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]


def hip_ok(rc, what):
    if rc != 0:
        raise SystemExit(f"monitor_step_timing.py: {what} failed with HIP status {rc}")


mesh = q.PolyMesh.box(n, n, n)
U, T, p = box_initial_fields(mesh.array("C").reshape(-1, 3))
dev = q.Device(mesh)
stream = C.c_void_p()
hip_ok(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
events = []
for _ in range(2 * steps):
    e = C.c_void_p()
    hip_ok(hip.hipEventCreate(C.byref(e)), "hipEventCreate")
    events.append(e)
lines = [f"run monitor on a {n}^3 box ({mesh.nCells} cells), GaussVolPoint, explicit, deltaT fixed; {steps} steps after {warmup}; "
         f"probes 4, patches 6; {L.lib.qgd_version().decode()}"]
modes = (("no monitor", 0), ("every step", 1), ("every 10th", 10))
ms = {m[0]: [] for m in modes}
sample_ms = []
for rep in range(3):
    for name, every in modes:
        case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=0.05 / n / 1.3, mu=1e-3))
        case.set_fields(U, T, p)
        case.set_stream(stream.value)
        fused = case.fused_info()["fused"]
        mon = case.monitor(probes=[0, mesh.nCells // 3, mesh.nCells // 2, mesh.nCells - 1], patches=range(6)) if every else None
        for _ in range(warmup):
            case.step_phase(3)
        if mon:
            mon.sample()
            mon.read()
        case.sync()
        used = 0
        t0 = time.perf_counter()
        for k in range(1, steps + 1):
            case.step_phase(3)               # one whole step, stream-ordered, no host wait
            if mon and k % every == 0:
                hip_ok(hip.hipEventRecord(events[used], stream), "hipEventRecord")
                mon.sample()
                hip_ok(hip.hipEventRecord(events[used + 1], stream), "hipEventRecord")
                used += 2
                if len(mon._pending) > 2:
                    mon.read()
        case.sync()
        ms[name].append((time.perf_counter() - t0) / steps * 1e3)
        if mon:
            while mon._pending:
                last = mon.read()
            per = []
            for i in range(0, used, 2):
                t = C.c_float()
                hip_ok(hip.hipEventElapsedTime(C.byref(t), events[i], events[i + 1]), "hipEventElapsedTime")
                per.append(t.value)
            if every == 1:
                sample_ms.append(sorted(per)[len(per) // 2])
            assert last["nonFinite"] == 0 and last["step"] == warmup + steps, last
        info = case.info()
        assert info["minRho"] > 0, info
        lines.append(f"  run {rep} {name:<11} {ms[name][-1]:8.4f} ms/step  ({'fused step' if fused else 'separate kernels'})")
        case.close()
dev.close()
best = {k: min(v) for k, v in ms.items()}
s = min(sample_ms)
base = best["no monitor"]
lines.append(f"ms per step (best of 3): no monitor {base:.4f}, every step {best['every step']:.4f} (+{(best['every step'] / base - 1) * 100:.1f} %), "
             f"every 10th {best['every 10th']:.4f} (+{(best['every 10th'] / base - 1) * 100:.1f} %)")
lines.append(f"one sample (three launches + the copy; HIP events, median of {steps}, best of 3 runs): {s:.4f} ms = {s / base * 100:.1f} % of a step")
lines.append(f"estimate {ESTIMATE} B per owned cell: {ESTIMATE * mesh.nCells / s / 1e6:.0f} GB/s if the cell pass moved exactly that")
lines.append("(hardware byte counters were not collected: they want a counter run of their own)")
out = os.path.join(ROOT, "profiles", "monitor_step_cost.txt")
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
