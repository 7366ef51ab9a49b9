"""What species cost per step on the implicitDiffusion branch, on an n^3 box (GaussVolPoint, fixed deltaT), one GPU: ms per step of the
implicit case without species -- on the default path (block-fused assembly of the U systems) and on the separate implicit kernels, the path a
case with species takes --, with 4 and 8 transported species (+ the inert one) and their iteration counts, and for scale the explicit
branch's step with the same species.  The runs alternate, best of `reps`.  Writes profiles/species_implicit_step.txt.
    python scripts/species_implicit_step_timing.py [n=200] [steps=40] [warmup=10] [reps=2]"""
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
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 40
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 10
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 2

if q.device_count() < 1:
    raise SystemExit("species_implicit_step_timing.py: no HIP device (a timing needs the GPU)")
mesh = q.PolyMesh.box(n, n, n)
C = mesh.array("C").reshape(-1, 3)
U, T, p = box_initial_fields(C)
dev = q.Device(mesh)


def composition(n_active):
    """n_active transported species with different wavelengths and the inert one last; every value in (0, 1)"""
    Y = [(0.5 / n_active) * (1.0 + 0.4 * np.sin((1.0 + 0.5 * i) * np.pi * C[:, 0] + 0.7 * i) * np.cos((0.5 + 0.3 * i) * np.pi * C[:, 1]))
         for i in range(n_active)]
    return Y + [1.0 - sum(Y)]


def run(implicit, n_active, fused_assembly=True):
    if fused_assembly:
        os.environ.pop("QGD_IMPL_FUSED", None)
    else:
        os.environ["QGD_IMPL_FUSED"] = "0"
    case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=0.05 / n / 1.3, mu=1e-3, implicitDiffusion=1 if implicit else 0))
    os.environ.pop("QGD_IMPL_FUSED", None)
    if n_active:
        names = [f"S{i}" for i in range(n_active + 1)]
        case.set_species(names, n_active, ScNumbers=[0.6 + 0.1 * i for i in range(n_active + 1)], implicit=bool(implicit))
        for name, y in zip(names, composition(n_active)):
            case.set_species_field(name, y)
    case.set_fields(U, T, p)
    fi = case.fused_info()
    path = "fused step" if fi["fused"] else ("block-fused U assembly" if fi["fusedImplicit"] else "separate kernels")
    case.step(warmup)
    t0 = time.perf_counter()
    case.step(steps)          # returns after the device has finished
    ms = (time.perf_counter() - t0) / steps * 1e3
    assert case.info()["minRho"] > 0
    note = ""
    if implicit:
        ii = case.implicit_info()
        note = "U " + "/".join(str(ii["solves"][k]["iterations"]) for k in ("Ux", "Uy", "Uz")) + f" e {ii['solves']['e']['iterations']}"
        if n_active:
            si = case.species_implicit_info()
            note += "; species " + "/".join(str(s["iterations"]) for s in si["species"].values())
            note += f"; unconverged {si['unconvergedSteps']} stalled {si['stalledSteps']}"
            s = sum(case.species_field(i) for i in range(n_active + 1))
            assert np.abs(s - 1.0).max() < 1e-12
    case.close()
    return ms, path, note


CASES = [("implicit, no species, default path", True, 0, True), ("implicit, no species, separate kernels", True, 0, False),
         ("implicit, 4 + 1 species", True, 4, True), ("implicit, 8 + 1 species", True, 8, True),
         ("explicit, no species", False, 0, True), ("explicit, 4 + 1 species", False, 4, True), ("explicit, 8 + 1 species", False, 8, True)]
lines = [f"species on the implicitDiffusion branch, {n}^3 box ({mesh.nCells} cells), GaussVolPoint, deltaT fixed, implicitTol "
         f"{q.default_options().implicitTol:g}; {steps} steps after {warmup}, best of {reps} alternating runs; {L.lib.qgd_version().decode()}",
         "iterations: those of the last step"]
best = {}
for rep in range(reps):
    for name, implicit, n_active, fused in CASES:
        ms, path, note = run(implicit, n_active, fused)
        lines.append(f"  run {rep} {name:<40} {ms:8.3f} ms/step  ({path}{'; ' + note if note else ''})")
        best[name] = min(best.get(name, 1e300), ms)
dev.close()
sep = best["implicit, no species, separate kernels"]
lines.append("ms per step, best: " + "; ".join(f"{k} {v:.3f}" for k, v in best.items()))
for k in (4, 8):
    d = best[f"implicit, {k} + 1 species"] - sep
    e = best[f"explicit, {k} + 1 species"] - best["explicit, no species"]
    lines.append(f"{k} transported species: +{d:.3f} ms over the implicit step on the same kernels ({d / k:.3f} ms per species); "
                 f"explicit branch for scale: +{e:.3f} ms over its fused step without species ({e / k:.3f} ms per species, the three-kernel step included)")
lines.append(f"the default path without species is {sep - best['implicit, no species, default path']:.3f} ms faster than the separate kernels: "
             "what a case pays for carrying species at all, before the first one")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "species_implicit_step.txt"), "w") as f:
    f.write(text)
