"""The geometry of the fused step block-major and packed (fusedFaceCellKernel<..., PACKW = 3>; qgd_setup.hpp FusedBlocks::gCode / gOwn / gDict):
on a mesh whose face streams pack and whose blocks see at most 16 reference patterns per axis among their cell centres and among their vertex
coordinates -- every uniform box -- a coordinate is a 16-bit code (dictionary entry << 12 | offset) in the block's own LDS slot order, V and hQGD
of an own cell are two 16-bit offsets, all read in the list round without a label; the doubles are formed behind the staging barrier:
dictionary entry + offset, integer arithmetic, the stored double exactly.  So every case here is BIT FOR BIT (np.array_equal after 5 steps, the
fields of tests/test_fused_front_loads_gpu.py)

    against the three-kernel step, and
    against the same device built with QGD_FUSED_PACKED_G=0 (centres, coordinates, V, hQGD gathered by label: level 2, the kernel as it was),

and every arm asserts that `packedGeometry` is what it expects and that the fused kernel ran.

    box(17,9,9), box(40,20,20)   plain, upwind and Courant-control arms; full bricks beside rim blocks
    box(16,8,12)                 three axis spacings
    box(3,2,2), box(1,1,40)      three of four waves issue the front-loaded group under an empty mask.  box(1,1,40) does not pack at level 1
                                 (no interior vertex), so nothing above packs either, and the kernel that runs is level 0
    box(16,8,12).shard(2, .)     firstBlock != 0: the boundary-layer blocks in a launch of their own
    QGD_FUSED_TEMPLATES=0        the template offset grows with the block; the geometry tables are per block either way
    IMPL on box(9,5,5)           to 1e-13 relative and with equal iteration counts, as tests/test_implicit_diffusion.py compares the assembly
    graded box                   20x8x8, the last cell twice as long as the first along x: V spans far more than 65 535 patterns -- not packed
    c5_mesh(16, 8**3, poly), prism543, ref533   bit-identical whichever way the rule decides; the decision is printed (ref533: one level of
                                 2:1 refinement, cells of 6 to 24 face entries -- the template tail beyond the six entries kept in LDS)
    the wide recipes             tests/packed_geometry_recipes.py: codes that use the high offset bits and several dictionary entries
"""
import contextlib
import os

import numpy as np
import pytest

import qgdsolver_amd as q

import packed_geometry_recipes as recipes
from test_config5_gpu import c5_mesh
from test_fused_front_loads_gpu import ARMS, FIELDS, STEPS, run
from test_fused_step_gpu import equal, shard_run
from util import make_mesh

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def packed_g(on):
    """QGD_FUSED_PACKED_G while a device builds its tables: unset (the default: pack where the mesh allows it) or 0"""
    old = os.environ.pop("QGD_FUSED_PACKED_G", None)
    if not on:
        os.environ["QGD_FUSED_PACKED_G"] = "0"
    try:
        yield
    finally:
        os.environ.pop("QGD_FUSED_PACKED_G", None)
        if old is not None:
            os.environ["QGD_FUSED_PACKED_G"] = old


def blocks_of(mesh):
    """what a device of this mesh reports (the run's info comes from the case: the device's own figure says which tables it holds)"""
    dev = q.Device(mesh, fused_tables="any")
    b = dev.fused_blocks()
    dev.close()
    return b


def graded_box():
    """scripts/probes/setup_harness.cpp's `graded`: box(20, 8, 8) with the last cell twice as long as the first along x, geometric"""
    n = 20
    p = q.PolyMesh.box(n, 8, 8).primitives()
    pts = p["points"].reshape(-1, 3).copy()
    r = 2.0 ** (1.0 / (n - 1))
    pts[:, 0] = (r ** (pts[:, 0] * n) - 1.0) / (r ** float(n) - 1.0)
    return q.PolyMesh.from_arrays(pts, p["faceOffsets"], p["facePoints"], p["owner"], p["neighbour"], p["nCells"], p["patchStart"],
                                  p["patchSize"], p["patchType"])


def three_arms(mesh, arm, tag, packs):
    """three kernels / fused at level 2 (geometry gathered by label) / fused with whatever the mesh allows: all three bit-identical.
    packs = None: whichever way the rule decides"""
    opt, key = ARMS[arm]
    ref, _, _ = run(mesh, False, key, **opt)
    with packed_g(False):
        full, i_full, _ = run(mesh, True, key, **opt)
    with packed_g(True):
        got, i_got, _ = run(mesh, True, key, **opt)
    assert i_full["packedGeometry"] is False, (tag, i_full)
    if packs is not None:
        assert i_got["packedGeometry"] is packs, (tag, i_got)
    assert not i_got["packedGeometry"] or (i_got["packedFaces"] and i_got["packedWeights"]), (tag, i_got)   # only where levels 1 and 2 apply
    assert (i_full["packedWeights"], i_full["packedFaces"]) == (i_got["packedWeights"], i_got["packedFaces"]), (tag, i_full, i_got)   # the switch touches the geometry alone
    assert i_got["blocks"] == i_full["blocks"] >= (mesh.nCells + 127) // 128, (i_got, i_full)
    worst = {k: (float(np.abs(ref[k] - got[k]).max()), float(np.abs(full[k] - got[k]).max())) for k in ref}
    print(f"{tag} {arm}: blocks {i_got['blocks']}, packed geometry {i_got['packedGeometry']}, faces {i_got['packedFaces']}, weights {i_got['packedWeights']}, "
          f"max |packed - three kernels|, |packed - by label| {worst}")
    for k in ref:
        assert np.isfinite(got[k]).all(), (tag, arm, k)
        assert np.array_equal(ref[k], got[k]), (tag, arm, k, "three kernels", worst[k])
        assert np.array_equal(full[k], got[k]), (tag, arm, k, "by label", worst[k])
    return i_got


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("shape", [(17, 9, 9), (40, 20, 20)])
def test_packed_geometry_on_many_blocks(shape, arm):
    ib = three_arms(q.PolyMesh.box(*shape), arm, f"box{shape}", True)
    assert ib["blocks"] > 8, ib
    if shape == (40, 20, 20):
        assert ib["blocks"] == 125, ib


def test_packed_geometry_with_three_axis_spacings():
    three_arms(q.PolyMesh.box(16, 8, 12), "plain", "box(16, 8, 12)", True)


@pytest.mark.parametrize("shape,packs", [((3, 2, 2), True), ((1, 1, 40), False)])
def test_packed_geometry_on_blocks_below_a_wavefront(shape, packs):
    ib = three_arms(q.PolyMesh.box(*shape), "plain", f"box{shape}", packs)
    if not packs:
        assert not ib["packedWeights"] and not ib["packedFaces"], ib   # level 0


@pytest.mark.parametrize("which", [0, 1])
def test_packed_geometry_on_a_shard(which):
    shard = q.PolyMesh.box(16, 8, 12).shard(2, which)
    for on in (False, True):
        with packed_g(on):
            dev = q.Device(shard, fused_tables="any")
            case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3, mu=1e-3))
            info, blocks = case.fused_info(), dev.fused_blocks()
            case.close(); dev.close()
        assert info["fused"] and 0 < info["layerBlocks"] < info["blocks"], info   # the second launch starts at block layerBlocks
        assert info["packedGeometry"] is on and blocks["packedGeometry"] is on, (on, info, blocks)
        assert info["packedFaces"] and blocks["packedFaces"], (on, info, blocks)
    ref = shard_run(shard, False, (0, 1), steps=STEPS)
    with packed_g(False):
        full = shard_run(shard, True, (0, 10, 11), steps=STEPS)   # (asserts that the fused kernel steps the shard)
    with packed_g(True):
        got = shard_run(shard, True, (0, 10, 11), steps=STEPS)
    equal(ref, got, ("box16x8x12", 2, which, "three kernels"))
    equal(full, got, ("box16x8x12", 2, which, "by label"))


def test_packed_geometry_with_one_template_per_block(monkeypatch):
    monkeypatch.setenv("QGD_FUSED_TEMPLATES", "0")   # read when the device builds its tables
    ib = three_arms(q.PolyMesh.box(17, 9, 9), "plain", "box17x9x9, own templates", True)
    assert ib["templates"] == ib["blocks"] > 8, ib   # the variable took effect: no two blocks share a template


def implicit_arms(mesh, tag, packs):
    fields = FIELDS + ("phiTauMC", "phiSigmaDotU")
    opt = dict(deltaT=1e-3, mu=1e-2, implicitDiffusion=1)
    ref, _, i_ref = run(mesh, False, "fusedImplicit", fields=fields, **opt)
    with packed_g(False):
        full, b_full, i_full = run(mesh, True, "fusedImplicit", fields=fields, **opt)
    with packed_g(True):
        got, b_got, i_got = run(mesh, True, "fusedImplicit", fields=fields, **opt)
    assert b_full["packedGeometry"] is False and b_got["packedGeometry"] is packs, (b_full, b_got)
    assert b_got["blocks"] >= (mesh.nCells + 127) // 128, b_got
    for other, impl, what in ((ref, i_ref, "separate kernels"), (full, i_full, "by label")):
        worst = {k: float(np.abs(other[k] - got[k]).max()) for k in got}
        print(f"{tag} implicit: blocks {b_got['blocks']}, max |packed - {what}| {worst}")
        for k in got:
            assert np.isfinite(got[k]).all(), k
            assert worst[k] <= 1e-13 * max(np.abs(other[k]).max(), 1e-300), (what, k, worst[k])
        assert impl["solves"] == i_got["solves"], (what, impl, i_got)


def test_packed_geometry_in_the_implicit_assembly():
    implicit_arms(q.PolyMesh.box(9, 5, 5), "box9x5x5", True)


def test_a_graded_box_does_not_pack():
    three_arms(graded_box(), "plain", "graded 20x8x8", False)


def test_a_jittered_polyhedral_mesh_whichever_way_the_rule_decides():
    mesh = c5_mesh(16, 8 ** 3, poly=True)
    b = blocks_of(mesh)
    print(f"c5poly: the rule decides packed geometry {b['packedGeometry']}, faces {b['packedFaces']}, weights {b['packedWeights']}")
    ib = three_arms(mesh, "plain", "c5poly", None)
    assert ib["packedGeometry"] is b["packedGeometry"], (ib, b)


def test_uniform_prisms_whichever_way_the_rule_decides():
    mesh = make_mesh("prism543")
    b = blocks_of(mesh)
    print(f"prism543: the rule decides packed geometry {b['packedGeometry']}, faces {b['packedFaces']}, weights {b['packedWeights']}")
    ib = three_arms(mesh, "plain", "prism543", None)
    assert ib["packedGeometry"] is b["packedGeometry"], (ib, b)


def test_refined_cells_whichever_way_the_rule_decides():
    mesh = make_mesh("ref533")
    b = blocks_of(mesh)
    print(f"ref533: the rule decides packed geometry {b['packedGeometry']}, faces {b['packedFaces']}, weights {b['packedWeights']}")
    ib = three_arms(mesh, "plain", "ref533", None)
    assert ib["packedGeometry"] is b["packedGeometry"], (ib, b)


# ---- codes that use the high offset bits and several dictionary entries (a uniform box keeps every offset below 16) ----
@pytest.mark.parametrize("arm", list(ARMS))
def test_wide_codes_on_many_blocks(arm):
    r = recipes.RECIPES["many blocks"]
    mesh = recipes.mesh_of(r)
    recipes.check(r, blocks_of(mesh))
    ib = three_arms(mesh, arm, r.tag, True)
    assert ib["blocks"] > 8, ib


def test_wide_codes_in_the_implicit_assembly():
    r = recipes.RECIPES["implicit"]
    mesh = recipes.mesh_of(r)
    recipes.check(r, blocks_of(mesh))
    implicit_arms(mesh, r.tag, True)
