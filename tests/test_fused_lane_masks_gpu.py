"""The lane masks of the fused step's loads (fusedFaceCellKernel): a lane loads only what it keeps -- the own-cell data under tid < 128, a
record piece under the condition of its LDS store, a vertex's weights and positions under tid < nUv, a face's streams under lf < nFc -- and a
wavefront whose whole slot range is empty skips the instruction.  A mask cannot change a result, so every case here asks for the states of the
three-kernel step BIT FOR BIT (np.array_equal after 5 steps), one small mesh per mask path:

    box(8,4,4)      one full block: 360 staged cells, 288 own + across-a-face, 225 vertices (a partly filled last piece round of each kind)
    box(3,2,2)      nOwn below a wavefront: waves 1-3 carry no cell and no vertex
    box(1,1,40)     almost every vertex is a patch point; fewer than 64 faces: three waves skip the face loads
    box(9,5,5)      a full brick surrounded by partial ones
    box(16,8,8)     464 faces per block: the second face round is partly filled
    c5_mesh(...)    vertices with more than eight cells, cells with more than six faces: the unpredicated tail loops

each in the plain arm, with `Gauss upwind` fluxes (UPW) and under Courant-number control (ADJ); the implicitDiffusion assembly (IMPL) on
box(9,5,5), compared the way tests/test_implicit_diffusion.py compares it with the separate kernels (to rounding, same iteration counts).
Every fused arm asserts that the fused kernel is what ran: a fall-back to the three kernels must not pass silently."""
import numpy as np
import pytest

import qgdsolver_amd as q

import cases
from test_config5_gpu import c5_mesh

pytestmark = pytest.mark.gpu

FIELDS = ("rho", "U", "p", "e", "rhoE", "p.boundary", "U.boundary")
STEPS = 5

MESHES = {
    "box8x4x4": lambda: q.PolyMesh.box(8, 4, 4),
    "box3x2x2": lambda: q.PolyMesh.box(3, 2, 2),
    "box1x1x40": lambda: q.PolyMesh.box(1, 1, 40),
    "box9x5x5": lambda: q.PolyMesh.box(9, 5, 5),
    "box16x8x8": lambda: q.PolyMesh.box(16, 8, 8),
    "c5poly": lambda: c5_mesh(16, 8 ** 3, poly=True),
}

# which entry of fused_info() says that the arm's instantiation of the fused kernel runs the step
ARMS = {
    "plain": (dict(deltaT=2e-4, mu=1e-3), "fused"),
    "upwind": (dict(deltaT=2e-4, mu=1e-3, fluxSchemeU=1, fluxSchemeH=1), "fused"),
    "adjust": (dict(deltaT=1e-4, mu=1e-3, adjustTimeStep=1, maxCo=0.3, maxDeltaT=1.0), "fusedAdjust"),
}


def run(mesh, fused, key, fields=FIELDS, **opt):
    dev = q.Device(mesh, fused_tables="any" if fused else False)
    case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", **opt))
    info = case.fused_info()
    assert bool(info[key]) == fused, (key, fused, info)
    U, T, p = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    case.set_fields(U, T, p)
    case.step(STEPS)
    out = {n: case.field(n).copy() for n in fields}
    i = case.info()
    out["mins"] = np.array([i["minRho"], i["minE"], i["steps"], i["time"], i["deltaT"]])
    impl = case.implicit_info()
    case.close(); dev.close()
    return out, info, impl


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("name", list(MESHES))
def test_masked_loads_leave_the_step_bit_identical(name, arm):
    mesh = MESHES[name]()
    opt, key = ARMS[arm]
    a, _, _ = run(mesh, False, key, **opt)
    b, ib, _ = run(mesh, True, key, **opt)
    assert ib["blocks"] >= (mesh.nCells + 127) // 128, ib
    if key == "fused":      # (the count is the one-launch step's; the ADJ arm reports its blocks only)
        assert ib["facesComputed"] >= mesh.nInternalFaces, ib
    worst = {k: float(np.abs(a[k] - b[k]).max()) for k in a}
    print(f"{name} {arm}: blocks {ib['blocks']}, max |fused - three kernels| {worst}")
    for k in a:
        assert np.isfinite(b[k]).all(), (name, arm, k)
        assert np.array_equal(a[k], b[k]), (name, arm, k, worst[k])


def test_masked_loads_in_the_implicit_assembly():
    mesh = MESHES["box9x5x5"]()
    fields = FIELDS + ("phiTauMC", "phiSigmaDotU")
    opt = dict(deltaT=1e-3, mu=1e-2, implicitDiffusion=1)
    a, _, ia = run(mesh, False, "fusedImplicit", fields=fields, **opt)
    b, ib, ii = run(mesh, True, "fusedImplicit", fields=fields, **opt)
    assert ib["blocks"] >= (mesh.nCells + 127) // 128, ib
    worst = {k: float(np.abs(a[k] - b[k]).max()) for k in a}
    print(f"box9x5x5 implicit: blocks {ib['blocks']}, max |fused - separate kernels| {worst}")
    for k in a:
        assert np.isfinite(b[k]).all(), k
        assert worst[k] <= 1e-13 * max(np.abs(a[k]).max(), 1e-300), (k, worst[k])
    assert ia["solves"] == ii["solves"], (ia, ii)
