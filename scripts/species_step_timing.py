"""What carrying species costs per step on an n^3 box (GaussVolPoint, explicit branch, fixed deltaT, the three-kernel step), with 1, 4 and 8
transported species (+ the inert one):
  a) the step without species (the `kernels` arm);
  b) the resident species case (qgd_case_set_species: vertex, face, cell and patch kernels of qgd_species.hip inside qgd_case_step);
  c) the way without the resident block: the same three-kernel step, the face fields phiJm / phi / tauQGDf / muf staged ONCE to device arrays
     (a real run would stage them every step: this arm is timed in its favour), then qgd_species_flux_dev + qgd_species_step_dev per species
     and step, all stream-ordered, one wait at the end.
Writes profiles/species_resident_step.txt.
    python scripts/species_step_timing.py [n=200] [steps=20] [warmup=5]"""
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
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 5
# DESIGN.md 1, "species resident in the case": algorithmic bytes per species on a hexahedral box (3 internal faces and 1 vertex per cell):
# per face 8 B net flux written + 8 B read back; per cell Y read by the face walk, read and written by the cell kernel, read by the vertex
# walk (4 x 8 B); per vertex 8 B written + 8 B read
BYTES_PER_CELL_PER_SPECIES = 3 * 16 + 4 * 8 + 16

if q.device_count() < 1:
    raise SystemExit("species_step_timing.py: no HIP device (a timing needs the GPU)")

mesh = q.PolyMesh.box(n, n, n)
C3 = mesh.array("C").reshape(-1, 3)
U, T, p = box_initial_fields(C3)
dev = q.Device(mesh, fused_tables=False)
opt = dict(stencil="GaussVolPoint", deltaT=0.05 / n / 1.3, mu=1e-3)
vp = lambda ptr: C.c_void_p(ptr)  # noqa: E731


def composition(n_active):
    Y = [(0.5 / n_active) * (1.0 + 0.3 * np.sin((1 + i) * np.pi * C3[:, 0]) * np.cos((1 + 0.5 * i) * np.pi * C3[:, 1])) for i in range(n_active)]
    return Y + [1.0 - sum(Y)]


def timed(fn, sync):
    fn(warmup)
    sync()
    t0 = time.perf_counter()
    fn(steps)
    sync()
    return (time.perf_counter() - t0) / steps * 1e3


def plain():
    case = q.QGDFoamCase(dev, q.default_options(**opt))
    assert not case.fused_info()["fused"]
    case.set_fields(U, T, p)
    ms = timed(case.step, case.sync)
    assert case.info()["minRho"] > 0
    case.close()
    return ms


batch = [0]   # register batch of the face and cell kernels, as the library reports it


def resident(n_active):
    case = q.QGDFoamCase(dev, q.default_options(**opt))
    Y = composition(n_active)
    case.set_species([f"S{i}" for i in range(n_active + 1)], n_active, ScNumbers=[0.7 + 0.1 * i for i in range(n_active + 1)])
    for i, y in enumerate(Y):
        case.set_species_field(i, y)
    case.set_fields(U, T, p)
    batch[0] = case.species_info()["batchWidth"]
    ms = timed(case.step, case.sync)
    total = sum(case.species_field(i) for i in range(n_active + 1))
    assert case.info()["minRho"] > 0 and np.abs(total - 1.0).max() < 1e-12
    case.close()
    return ms


def stateless(n_active):
    case = q.QGDFoamCase(dev, q.default_options(**opt))
    case.set_fields(U, T, p)
    case.updateFluxes()
    nif = mesh.nInternalFaces
    own, nei, w = mesh.array("owner"), mesh.array("neighbour"), mesh.array("weights")[:nif]
    mu = case.field("mu") + case.field("muQGD")
    mub = case.field("mu.boundary") + case.field("muQGD.boundary")
    muf = np.concatenate([w * mu[own[:nif]] + (1 - w) * mu[nei], mub])
    d = {k: dev.to_device(case.field(k)) for k in ("phiJm", "phi", "tauQGDf")}
    d["muf"] = dev.to_device(muf)
    d["U"], d["Ub"] = dev.to_device(case.field("U")), dev.to_device(case.field("U.boundary"))
    d["rho"] = dev.to_device(case.field("rho"))
    Y = composition(n_active)[:n_active]
    own_b = own[nif:]
    dY = [dev.to_device(y) for y in Y]
    dYb = [dev.to_device(y[own_b]) for y in Y]
    dNew = [dev.alloc(8 * mesh.nCells) for _ in Y]
    work = {k: dev.alloc(8 * mesh.nFaces) for k in ("phiJmY", "df")}
    work["grad"] = dev.alloc(24 * mesh.nFaces)
    dt = float(case.options.deltaT)

    def run(k):
        for _ in range(k):
            case.step_phase(3)
            for i in range(n_active):
                L.check(L.lib.qgd_species_flux_dev(dev._h, L.FVSC_GAUSSVOLPOINT, vp(dY[i]), vp(dYb[i]), vp(d["U"]), vp(d["Ub"]), vp(d["phiJm"]), vp(d["phi"]),
                                                   vp(d["tauQGDf"]), vp(work["phiJmY"]), vp(work["df"]), vp(work["grad"])), "qgd_species_flux_dev")
                L.check(L.lib.qgd_species_step_dev(dev._h, vp(dY[i]), vp(dYb[i]), vp(d["rho"]), vp(d["rho"]), vp(work["phiJmY"]), vp(d["muf"]),
                                                   0.7 + 0.1 * i, dt, None, vp(work["df"]), vp(dNew[i])), "qgd_species_step_dev")
                dY[i], dNew[i] = dNew[i], dY[i]

    def sync():
        case.sync()
        dev.sync()

    ms = timed(run, sync)
    for ptr in list(d.values()) + dY + dYb + dNew + list(work.values()):
        dev.release(ptr)
    case.close()
    return ms


lines = [f"species resident in the case, {n}^3 box ({mesh.nCells} cells, {mesh.nFaces} faces), GaussVolPoint, explicit, deltaT fixed, separate kernels; "
         f"{steps} steps after {warmup}, best of 2; {L.lib.qgd_version().decode()}",
         f"command: python scripts/species_step_timing.py {n} {steps} {warmup}"]
base = min(plain() for _ in range(2))
lines.append(f"  step without species                       {base:8.4f} ms/step")
res, sl = {}, {}
for k in (1, 4, 8):
    res[k] = min(resident(k) for _ in range(2))
    sl[k] = min(stateless(k) for _ in range(2))
    lines.append(f"  {k} transported species: resident {res[k]:8.4f} ms/step (+{res[k] - base:7.4f}), stateless pair per species {sl[k]:8.4f} ms/step (+{sl[k] - base:7.4f})")
inc_res, inc_sl = (res[8] - res[1]) / 7, (sl[8] - sl[1]) / 7
gb = BYTES_PER_CELL_PER_SPECIES * mesh.nCells / 1e9
W = batch[0]
lines.append(f"resident, inside a batch of {W} (from 1 to 4 species): {(res[4] - res[1]) / 3:.4f} ms per species; from 4 to 8 species: "
             f"{(res[8] - res[4]) / 4:.4f} ms per species; the first species (one walk of every kernel): {res[1] - base:.4f} ms")
lines.append(f"increment per extra species (from 1 to 8): resident {inc_res:.4f} ms, stateless pair {inc_sl:.4f} ms (ratio {inc_sl / inc_res:.2f})")
lines.append(f"DESIGN's algorithmic bytes: {BYTES_PER_CELL_PER_SPECIES} B per cell per species = {gb:.3f} GB per species and step: "
             f"{gb / (inc_res * 1e-3):.0f} GB/s if the increment moved exactly that")
lines.append("(the stateless arm's face fields are staged once, not every step, and its rho is not advanced: it is timed in its favour; "
             "hardware byte counters were not collected)")
dev.close()
with open(os.path.join(ROOT, "profiles", "species_resident_step.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
