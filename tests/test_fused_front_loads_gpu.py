"""The issue order of the fused step's loads (fusedFaceCellKernel): the block header (counts and template id) comes through the scalar path,
and what needs the header but no label -- the template's face positions, the own cells' face entries, a vertex's cell positions and weights --
goes out in round 0 behind the lists and stays in flight across the counted wait that ends the round.  The masks of these loads are those of
tests/test_fused_lane_masks_gpu.py; the cases here are the ones the new order can break, each against the three-kernel step BIT FOR BIT
(np.array_equal after 5 steps):

    many blocks     box(17,9,9): full bricks beside partial rim blocks; box(40,20,20): 125 full bricks, a block count that is no multiple of
                    the XCD run (the tail of xcdTile), headers of neighbouring blocks in one cache line -- plain, upwind, Courant control
    one template    QGD_FUSED_TEMPLATES=0 while the device is built: every block has its own template, so the template offset
    per block       tpl x capF x 12 grows with the block index and is formed from a scalar
    firstBlock != 0 a shard steps its boundary-layer blocks in a launch of their own and the rest in a second one
    small blocks    box(3,2,2), box(1,1,40): with no wavefront-level skip in the front-loaded group, three of four waves issue it under an
                    empty mask
    IMPL            box(9,5,5): the implicit assembly requests its face streams later in the kernel, behind the same waits (to rounding,
                    same iteration counts, as tests/test_implicit_diffusion.py compares it)

Every fused arm asserts that the fused kernel is what ran."""
import numpy as np
import pytest

import qgdsolver_amd as q

import cases
from test_config5_gpu import c5_mesh
from test_fused_step_gpu import equal, shard_run

pytestmark = pytest.mark.gpu

FIELDS = ("rho", "U", "p", "e", "rhoE", "p.boundary", "U.boundary")
STEPS = 5

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
    if fused:
        info["templates"] = dev.fused_blocks()["templates"]
    U, T, p = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    case.set_fields(U, T, p)
    case.step(STEPS)
    out = {n: case.field(n).copy() for n in fields}
    i = case.info()
    out["mins"] = np.array([i["minRho"], i["minE"], i["steps"], i["time"], i["deltaT"]])
    impl = case.implicit_info()
    case.close(); dev.close()
    return out, info, impl


def bit_identical(mesh, arm, tag):
    opt, key = ARMS[arm]
    a, _, _ = run(mesh, False, key, **opt)
    b, ib, _ = run(mesh, True, key, **opt)
    assert ib["blocks"] >= (mesh.nCells + 127) // 128, ib
    worst = {k: float(np.abs(a[k] - b[k]).max()) for k in a}
    print(f"{tag} {arm}: blocks {ib['blocks']}, max |fused - three kernels| {worst}")
    for k in a:
        assert np.isfinite(b[k]).all(), (tag, arm, k)
        assert np.array_equal(a[k], b[k]), (tag, arm, k, worst[k])
    return ib


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("shape", [(17, 9, 9), (40, 20, 20)])
def test_many_blocks_and_several_templates(shape, arm):
    ib = bit_identical(q.PolyMesh.box(*shape), arm, f"box{shape}")
    assert ib["blocks"] > 8, ib
    if shape == (40, 20, 20):
        assert ib["blocks"] == 125, ib


@pytest.mark.parametrize("name", ["box17x9x9", "c5poly"])
def test_one_template_per_block(name, monkeypatch):
    monkeypatch.setenv("QGD_FUSED_TEMPLATES", "0")   # read when the device builds its tables
    mesh = q.PolyMesh.box(17, 9, 9) if name == "box17x9x9" else c5_mesh(16, 8 ** 3, poly=True)
    ib = bit_identical(mesh, "plain", name + ", own templates")
    assert ib["templates"] == ib["blocks"] > 8, ib   # the variable took effect: no two blocks share a template


@pytest.mark.parametrize("which", [0, 1])
def test_first_block_is_not_zero_on_a_shard(which):
    shard = q.PolyMesh.box(16, 8, 12).shard(2, which)
    dev = q.Device(shard, fused_tables="any")
    case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3, mu=1e-3))
    info = case.fused_info()
    case.close(); dev.close()
    assert info["fused"] and 0 < info["layerBlocks"] < info["blocks"], info   # the second launch starts at block layerBlocks
    ref = shard_run(shard, False, (0, 1), steps=STEPS)
    got = shard_run(shard, True, (0, 10, 11), steps=STEPS)   # (asserts that the fused kernel steps the shard)
    equal(ref, got, ("box16x8x12", 2, which))


@pytest.mark.parametrize("shape", [(3, 2, 2), (1, 1, 40)])
def test_blocks_below_a_wavefront_and_of_patch_points_only(shape):
    bit_identical(q.PolyMesh.box(*shape), "plain", f"box{shape}")


def test_front_loads_in_the_implicit_assembly():
    mesh = q.PolyMesh.box(9, 5, 5)
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
