"""What species cost a shard's step and its state message, timed on ONE GPU: one k-slab of the n^3 box as rank `r` of `world` would hold it
(scripts/shard_slab_step.py's slab), with four species and QGD_SPECIES_HALO, exchanging with ITSELF through the library's own transport
(halo.NativeComm: qgd_case_step_sharded, plain and overlapped), against the UNCUT box with the same number of cells and the same species
stepped by qgd_case_step.

    python scripts/species_halo_step.py slab [n=400] [world=8] [rank=3] [steps=50]
    python scripts/species_halo_step.py box  [n=400] [world=8] [rank=3] [steps=50]

`box` needs nothing this script's tree added to the library, so QGD_AMD_LIB=<an older build> measures that build.  Prints one JSON line
per case: ms per step, and for the slab the state message with and without the species tail, in bytes per slot and in ms per exchange."""
import json
import sys
import time

import os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import qgdsolver_amd as q  # noqa: E402
from qgdsolver_amd.halo import NativeComm, slab_range  # noqa: E402
from qgdsolver_amd.synthetic import box_initial_fields  # noqa: E402

SC = [0.7, 1.0, 1.0, 1.3]


def composition(C):
    y0 = 0.2 + 0.1 * np.sin(2 * np.pi * C[:, 0]) * np.cos(np.pi * C[:, 1])
    y1 = 0.2 + 0.05 * np.cos(2 * np.pi * C[:, 2])
    y3 = 0.2 + 0.1 * np.cos(3.0 * C[:, 0] + 2.0 * C[:, 1])
    return [y0, y1, 1.0 - y0 - y1 - y3, y3]


def make(mesh, deltaT, species, halo):
    dev = q.Device(mesh, fused_tables=False)     # (a case with species steps with the separate kernels: the cases without species do too)
    case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=deltaT))
    C = mesh.array("C").reshape(-1, 3)
    if species:
        case.set_species(["A", "B", "C", "D"], 2, ScNumbers=SC, **({"halo": True} if halo else {}))
        for i, y in enumerate(composition(C)):
            case.set_species_field(i, y)
    case.set_fields(*box_initial_fields(C))
    return dev, case


def timed(fn, sync, steps, warmup=10):
    for _ in range(warmup):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    return round((time.perf_counter() - t0) / steps * 1e3, 4)


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "slab"
    n, world, rank, steps = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((2, 400), (3, 8), (4, 3), (5, 50)))
    lib = os.environ.get("QGD_AMD_LIB", "this tree's")
    if what == "box":
        m = round((n ** 3 / world) ** (1.0 / 3.0))
        mesh = q.PolyMesh.box(m, m, m)
        for species in (True, False):
            dev, case = make(mesh, 0.1 / m / 1.3, species, False)
            ms = timed(lambda: case.step(1), case.sync, steps)
            print(json.dumps({"case": f"uncut box {m}^3", "library": lib, "species": 4 if species else 0, "cells_owned": m ** 3, "ms_per_step": ms,
                              "min_rho": case.info()["minRho"]}), flush=True)
            case.close(); dev.close()
        return
    lo, hi, k_lo, k_hi = slab_range(n, rank, world)
    mesh = q.PolyMesh.box(n, n, n, k_range=(k_lo, k_hi))
    comm = NativeComm(0)
    peers = [0, 0]
    for species in (True, False):
        dev, case = make(mesh, 0.1 / n / 1.3, species, True)
        out = {"case": f"slab {n}x{n}x{hi - lo} (+{(k_hi - k_lo) - (hi - lo)} ghost planes), self-exchange through RCCL", "library": lib,
               "species": 4 if species else 0, "cells_owned": n * n * (hi - lo),
               "state_message_bytes_per_slot": [8 * case.halo_count(k) for k in range(2)],
               "ms_per_exchange": timed(lambda: comm.exchange(case, peers), case.sync, steps), "ms_per_step": {}}
        for name, ov in (("plain", False), ("overlapped", True)):
            out["ms_per_step"][name] = timed(lambda: comm.step(case, peers, overlapped=ov), case.sync, steps)
        out["min_rho"] = case.info()["minRho"]
        if species:
            out["min_Y"] = min(float(case.species_field(i).min()) for i in range(4))
        print(json.dumps(out), flush=True)
        case.close(); dev.close()
    comm.close()


if __name__ == "__main__":
    main()
