"""What the species block of a run monitor costs per sample on an n^3 box (GaussVolPoint, explicit branch, fixed deltaT, the separate
kernels a case with species steps with) for nS = 2, 5 and 9 species: ms per step of the case, ms per sample of a monitor without and with
the species block (HIP events around qgd_monitor_sample on the idle stream: three launches + the copy, and six launches + the copy), their
difference -- the species block -- and the rate that difference means against the block's own traffic, nS planes of 8 B per owned
cell plus rho and V once.  A case with species steps through qgd_case_step, which waits for the device, so every sample starts on an idle
stream.  Writes profiles/species_monitor_cost.txt.
    python scripts/species_monitor_step_timing.py [n=200] [steps=30] [warmup=5]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qgdsolver_amd as q  # noqa: E402
from qgdsolver_amd import _lib as L  # noqa: E402
from qgdsolver_amd.synthetic import box_initial_fields  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 5
FLOW_BLOCK_MS = 0.22   # profiles/monitor_step_cost.txt: one sample of the flow block at 8 M cells

if q.device_count() < 1:
    raise SystemExit("species_monitor_step_timing.py: no HIP device (a timing needs the GPU)")
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
        raise SystemExit(f"species_monitor_step_timing.py: {what} failed with HIP status {rc}")


mesh = q.PolyMesh.box(n, n, n)
Cc = mesh.array("C").reshape(-1, 3)
U, T, p = box_initial_fields(Cc)
dev = q.Device(mesh, fused_tables=False)
stream = C.c_void_p()
hip_ok(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
ev = [C.c_void_p(), C.c_void_p()]
for e in ev:
    hip_ok(hip.hipEventCreate(C.byref(e)), "hipEventCreate")
lines = [f"species block of the run monitor on a {n}^3 box ({mesh.nCells} cells), GaussVolPoint, explicit, deltaT fixed, separate kernels; "
         f"{steps} steps after {warmup}, a sample after every step; probes 4, patches 6; {L.lib.qgd_version().decode()}"]
probes = [0, mesh.nCells // 3, mesh.nCells // 2, mesh.nCells - 1]
for nS in (2, 5, 9):
    inert = nS - 1
    amp = 0.5 / (nS - 1)
    Y = [amp * (1.0 + 0.4 * np.sin((1.0 + 0.5 * i) * np.pi * Cc[:, 0] + 0.7 * i) * np.cos((0.5 + 0.3 * i) * np.pi * Cc[:, 1])) for i in range(nS - 1)]
    Y.append(1.0 - sum(Y))
    res = {}
    for mode in ("flow block", "flow + species"):
        case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=0.05 / n / 1.3, mu=1e-3))
        case.set_species([f"S{i}" for i in range(nS)], inert)
        for i in range(nS):
            case.set_species_field(i, Y[i])
        case.set_fields(U, T, p)
        case.set_stream(stream.value)
        mon = case.monitor(probes=probes, patches=range(6), species=mode != "flow block")
        case.step(warmup)
        mon.sample()
        mon.read()
        per, t_step = [], 0.0
        for k in range(steps):
            t0 = time.perf_counter()
            case.step(1)
            t_step += time.perf_counter() - t0
            hip_ok(hip.hipEventRecord(ev[0], stream), "hipEventRecord")
            mon.sample()
            hip_ok(hip.hipEventRecord(ev[1], stream), "hipEventRecord")
            last = mon.read()
            hip_ok(hip.hipEventSynchronize(ev[1]), "hipEventSynchronize")   # (read() waited for the slot's own event, recorded just before)
            t = C.c_float()
            hip_ok(hip.hipEventElapsedTime(C.byref(t), ev[0], ev[1]), "hipEventElapsedTime")
            per.append(t.value)
        assert last["nonFinite"] == 0 and last["step"] == warmup + steps, last
        if mode != "flow block":
            assert last["speciesNonFinite"] == 0 and last["speciesFluxState"] == 1 and last["speciesMin"].min() > 0, last
        res[mode] = (sorted(per)[len(per) // 2], min(per), t_step / steps * 1e3)
        case.close()
    flow, both = res["flow block"], res["flow + species"]
    block = both[0] - flow[0]
    traffic = (nS + 2) * 8 * mesh.nCells
    lines.append(f"nS {nS}: step {both[2]:.4f} ms (host clock around qgd_case_step); one sample, median of {steps} (best): flow block {flow[0]:.4f} ({flow[1]:.4f}) ms, "
                 f"flow + species {both[0]:.4f} ({both[1]:.4f}) ms")
    lines.append(f"       species block {block:.4f} ms = {block / both[2] * 100:.1f} % of a step, {block / FLOW_BLOCK_MS:.2f} x the flow block's {FLOW_BLOCK_MS} ms; "
                 f"traffic {nS} planes + rho + V = {traffic / 1e6:.0f} MB once: {traffic / block / 1e6:.0f} GB/s if the pass moved exactly that")
dev.close()
lines.append("(the difference of two medians on an idle stream: launch gaps of the three extra launches are in it; hardware byte counters were not "
             "collected: they want a counter run of their own)")
out = os.path.join(ROOT, "profiles", "species_monitor_cost.txt")
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
