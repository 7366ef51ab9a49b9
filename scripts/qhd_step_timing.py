"""wall time of the resident QHDFoam step (qgd_qhd_case_step) on an n^3 box: usage  qhd_step_timing.py n [steps] [adjust [arms] | weights]

adjust: the step with the Courant-number control (qgd_qhd_case_set_time_control) against the step without it, same process, alternating
blocks of `steps` single steps, per arm (arms: a comma list out of explicit, implicit, explicit-rotating, implicit-rotating; default all).
Both kinds of block run at the SAME deltaT (the "on" blocks under a large maxCo and maxDeltaT = the options' deltaT: the rule returns it),
so the solves do the same work and the difference is the control's own; reported per kind: the median / min / max of the step's time
outside the pressure solve (host clock around the step minus the solve's own, as scripts/srf_step_timing.py does) and of the whole step,
and the iteration counts.

weights: the start values of the solves while deltaT moves.  implicitDiffusion, `steps` steps per arm after six of warm-up, fresh case per
arm: deltaT alternating every step between 0.85 and 1.0 of deltaT0 (it never stops moving, its level does not drift) with the Lagrange
weights (QGD_QHD_LAGRANGE=1, the default) and with the equal-step ones (=0), and a fixed deltaT = 0.925 deltaT0 as the floor either could
reach: pressure and U / T iteration counts, first residuals of the pressure solve, ms per step."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import qgdsolver_amd as q
from qgdsolver_amd import qhdfoam
from test_qhd_case import cavity_bcs, options, initial
n = int(sys.argv[1]); steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
mesh = q.PolyMesh.box(n, n, n)
dev = q.Device(mesh)
dt0 = 0.1 / n   # (with mu = 1e-3, the benchmark's: nu deltaT / h^2 = 0.02 at n = 200 -- the explicit branch is stable)
if len(sys.argv) > 3 and sys.argv[3] == "adjust":
    arms = sys.argv[4].split(",") if len(sys.argv) > 4 else ["explicit", "implicit", "explicit-rotating", "implicit-rotating"]
    for arm in arms:
        implicit, rotating = arm.startswith("implicit"), arm.endswith("rotating")
        c = qhdfoam.QHDFoamCase(dev, options(deltaT=dt0, mu=1e-3, pTol=1e-8, pMaxIter=400, implicitDiffusion=int(implicit), implicitTol=1e-10))
        if rotating:
            c.set_srf((0.3, -0.5, 0.8))
        cavity_bcs(c, mesh)
        c.set_fields(*initial(mesh))
        c.step(6)
        ms, rest, pit, xit = {0: [], 1: []}, {0: [], 1: []}, {0: [], 1: []}, {0: [], 1: []}
        for block in range(6):
            on = block % 2
            c.set_time_control(bool(on), 1e30, dt0, 0.75)
            for _ in range(steps):
                t0 = time.perf_counter(); c.step(1); t = (time.perf_counter() - t0) * 1e3
                info = c.info()
                assert info["deltaT"] == dt0
                ms[on].append(t); rest[on].append(t - info["pSolveMs"]); pit[on].append(info["pIterations"])
                if implicit:
                    xit[on].append(max(s["iterations"] for s in c.implicit_info()["solves"].values()))
        for on in (0, 1):
            a, r = np.array(ms[on]), np.array(rest[on])
            print(f"QHD {n}^3 {arm} control {'on ' if on else 'off'}: outside the pressure solve median {np.median(r):.3f} min {r.min():.3f} max {r.max():.3f} ms; "
                  f"whole step median {np.median(a):.3f} min {a.min():.3f} max {a.max():.3f} ms over {a.size} steps; p iterations mean {np.mean(pit[on]):.2f}"
                  + (f"; U/T iterations mean {np.mean(xit[on]):.2f}" if implicit else ""), flush=True)
        U = c.field("U")
        print(f"QHD {n}^3 {arm}: on - off outside the pressure solve, medians {np.median(rest[1]) - np.median(rest[0]):+.3f} ms, minima "
              f"{min(rest[1]) - min(rest[0]):+.3f} ms; CoNum {c.time_info()['CoNum']:.4g}; U finite {bool(np.isfinite(U).all())}", flush=True)
        c.close()
    dev.close()
    sys.exit(0)
if len(sys.argv) > 3 and sys.argv[3] == "weights":
    for tag, lagrange, moving in (("deltaT moving, Lagrange weights  ", "1", True), ("deltaT moving, equal-step weights", "0", True),
                                  ("deltaT fixed at 0.925 deltaT0    ", "1", False)):
        os.environ["QGD_QHD_LAGRANGE"] = lagrange
        c = qhdfoam.QHDFoamCase(dev, options(deltaT=dt0 if moving else 0.925 * dt0, mu=1e-3, pTol=1e-8, pMaxIter=400, implicitDiffusion=1, implicitTol=1e-10))
        cavity_bcs(c, mesh)
        c.set_fields(*initial(mesh))
        ms, pit, xit, r0, x0 = [], [], [], [], []
        for step in range(6 + steps):
            if moving:
                c.set_time_control(True, 1e30, dt0 * (1.0 if step % 2 else 0.85), 0.75)
            t0 = time.perf_counter(); c.step(1); t = (time.perf_counter() - t0) * 1e3
            if step < 6:
                continue
            info, ii = c.info(), c.implicit_info()
            ms.append(t); pit.append(info["pIterations"]); r0.append(info["pInitialResidual"])
            xit.append(max(s["iterations"] for s in ii["solves"].values())); x0.append(max(s["initial"] for s in ii["solves"].values()))
        ii = c.implicit_info()
        print(f"QHD {n}^3 implicit, {tag}: p iterations mean {np.mean(pit):.2f} (first residual, geometric mean {np.exp(np.mean(np.log(r0))):.3g}); "
              f"U/T iterations mean {np.mean(xit):.2f} (first residual {np.exp(np.mean(np.log(x0))):.3g}); median {np.median(ms):.3f} ms/step over {len(ms)} steps; "
              f"unconverged {ii['unconverged_steps']}, stalled {ii['stalled_steps']}", flush=True)
        c.close()
    dev.close()
    sys.exit(0)
c = qhdfoam.QHDFoamCase(dev, options(deltaT=0.2 / n, pTol=1e-8, pMaxIter=400))
cavity_bcs(c, mesh)
c.set_fields(*initial(mesh))
c.step(2)
t0 = time.perf_counter(); c.step(steps); c.field("p")[:1]; dt = (time.perf_counter() - t0) / steps
info = c.info()
print(f"QHD {n}^3: {dt * 1e3:.2f} ms/step, {info}", flush=True)
