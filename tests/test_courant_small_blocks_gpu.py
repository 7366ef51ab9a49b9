"""Courant-number control on meshes whose cell blocks are small.

Under adjustTimeStep every kernel that computes faces leaves max Cof / min tauQGDf of its workgroup in a slot of one table
(CaseView::blkFace): the internal-face kernels in slots [0, faceBlocks), faceBlocks = ceil(nInternalFaces / 64), the patch kernel behind them,
and -- on the block path, fusedFaceCellKernel<..., ADJ> -- every cell block in a slot too.  The blocks once used slot `block`: fine while a
mesh has fewer blocks than 64-face tiles (about 384 internal faces per block on every mesh the parity matrix steps), wrong on a chain of
cells, where a block holds 50 to 60 cells and as many internal faces: blocks faceBlocks .. nBlocks-1 then overwrote the partials of the
first patch workgroups, and the faces of an inlet on xMin dropped out of deltaT.  The blocks have slots of their own behind the patch
kernel's now.  tests/cpp/fused_blocks_test.cpp asserts the premise on the host for the very meshes below (more blocks than face tiles;
patch 0 wholly inside the patch faces whose slots the blocks used to take); here the case itself says so (fused_info), and the oracle
alone shows that the inlet decides deltaT where it is meant to.

Three arms per mesh, one step at a time, 12 steps: the blocks ("fusedAdjust", asserted), the three kernels, the oracle.  deltaT, CoNum
and time against the oracle at the 1e-11 of test_adjust_time_step, the states at STATE_TOL; blocks against kernels at the 1e-13 of
test_fused_step_under_courant_number_control."""
import numpy as np
import pytest

import qgdsolver_amd as q

import cases
from oracle import OracleCase
from util import assert_path, oracle_mesh_of, rel_err

STATE_TOL = 1e-10      # tests/test_case_parity_gpu.py
STEPS = 12
INLET_U = (2.0, 0.0, 0.0)


def inlet_bcs(u):
    """a fixedValue inlet on xMin (as mixed_box_bcs has one), everything else left at zeroGradient"""
    def fn(case):
        case.set_bc(0, U=("fixedValue", u), T=("fixedValue", 1.0), p=("zeroGradient", None))
    return fn


# tag -> (mesh, deltaT0, whether an inlet on xMin, faster than anything inside, is to set the step)
MESHES = {
    "1024x1x1": (lambda: q.PolyMesh.box(1024, 1, 1), 2e-5, True),
    "700x1x1": (lambda: q.PolyMesh.box(700, 1, 1, lo=(0.0, 0.45, 0.45), hi=(7.0, 0.55, 0.55)), 1e-4, True),
    "1x1x700": (lambda: q.PolyMesh.box(1, 1, 700), 2e-5, False),      # the pressure pulse in the middle of the chain decides: an interior face
}


def options(dt0):
    return q.default_options(stencil="GaussVolPoint", deltaT=dt0, adjustTimeStep=1, maxCo=0.3, maxDeltaT=1.0, cTau=0.75, mu=1e-3)


def history(case, steps=STEPS):
    h = []
    for _ in range(steps):
        case.step(1)
        i = case.info()
        h.append((i["deltaT"], i["time"], i["CoNum"]))
    return np.array(h)


def oracle_run(mesh, dt0, bc_fn):
    oc = OracleCase(oracle_mesh_of(mesh), options(dt0))
    if bc_fn:
        bc_fn(oc)
    oc.set_fields(*cases.box_initial_fields(mesh.array("C").reshape(-1, 3)))
    return oc, history(oc)


def inlet_decides(mesh, dt0, hist):
    """the oracle alone: with the inlet as slow as the fluid behind it the deltaT / CoNum history is another one, by far more than any
    tolerance below -- so a device that lost the inlet faces' partials could not pass"""
    _, slow = oracle_run(mesh, dt0, inlet_bcs((0.0, 0.0, 0.0)))
    return float(np.abs(hist[:, [0, 2]] - slow[:, [0, 2]]).max() / np.abs(hist[:, [0, 2]]).max())


@pytest.mark.parametrize("tag", [t for t in MESHES if MESHES[t][2]])
def test_the_inlet_sets_the_step_in_the_oracle(tag):
    make, dt0, _ = MESHES[tag]
    mesh = make()
    _, hist = oracle_run(mesh, dt0, inlet_bcs(INLET_U))
    assert np.isfinite(hist).all() and inlet_decides(mesh, dt0, hist) > 1e-3, tag


def device_run(mesh, dt0, bc_fn, arm):
    dev = q.Device(mesh, fused_tables="any" if arm == "fusedAdjust" else False)
    gc = q.QGDFoamCase(dev, options(dt0))
    assert_path(gc, arm, arm)
    if arm == "fusedAdjust":
        fi = gc.fused_info()
        # the premise, for the library that runs: more blocks than 64-face tiles of internal faces
        assert fi["blocks"] > (mesh.nInternalFaces + 63) // 64, (fi, mesh.nInternalFaces)
    if bc_fn:
        bc_fn(gc)
    gc.set_fields(*cases.box_initial_fields(mesh.array("C").reshape(-1, 3)))
    return dev, gc


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(MESHES))
def test_courant_control_on_small_blocks(tag):
    make, dt0, inlet = MESHES[tag]
    mesh = make()
    assert mesh.nGeometricD == 3
    bc_fn = inlet_bcs(INLET_U) if inlet else None
    oc, ho = oracle_run(mesh, dt0, bc_fn)
    assert np.isfinite(ho).all()
    if inlet:
        d = inlet_decides(mesh, dt0, ho)
        print(f"{tag}: the oracle's deltaT / CoNum history moves by {d:.3e} (relative) with the inlet")
        assert d > 1e-3, (tag, d)
    out, hist = {}, {}
    for arm in ("fusedAdjust", "kernels"):
        dev, gc = device_run(mesh, dt0, bc_fn, arm)
        h = []
        for k in range(STEPS):
            gc.step(1)
            i = gc.info()
            h.append((i["deltaT"], i["time"], i["CoNum"]))
            err = [abs(h[-1][j] - ho[k, j]) / max(ho[k, j], 1e-30) for j in range(3)]
            print(f"{tag} {arm} step {k + 1}: deltaT {h[-1][0]:.15e} rel err deltaT {err[0]:.2e} time {err[1]:.2e} CoNum {err[2]:.2e}")
            assert abs(i["deltaT"] - ho[k, 0]) <= 1e-11 * ho[k, 0], (tag, arm, k, i, ho[k])
            assert abs(i["CoNum"] - ho[k, 2]) <= 1e-11 * max(ho[k, 2], 1e-30), (tag, arm, k, i, ho[k])
            assert abs(i["time"] - ho[k, 1]) <= 1e-11 * ho[k, 1], (tag, arm, k, i, ho[k])
        hist[arm] = np.array(h)
        out[arm] = {n: gc.field(n).copy() for n in ("rho", "U", "p", "e", "rhoE", "p.boundary", "U.boundary")}
        for n in ("rho", "U", "p", "e"):
            e = rel_err(out[arm][n], oc.field(n))
            print(f"{tag} {arm} {n}: {e:.3e}")
            assert e <= STATE_TOL, (tag, arm, n, e)
        gc.close(); dev.close()
    ha, hb = hist["kernels"], hist["fusedAdjust"]
    assert np.abs(ha - hb).max() <= 1e-13 * np.abs(ha).max(), (tag, ha[-1], hb[-1])
    a, b = out["kernels"], out["fusedAdjust"]
    for k in a:
        assert np.isfinite(b[k]).all() and np.abs(a[k] - b[k]).max() <= 1e-13 * np.abs(a[k]).max(), (tag, k, np.abs(a[k] - b[k]).max())
