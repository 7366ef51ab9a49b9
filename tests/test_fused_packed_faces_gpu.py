"""The per-face streams of the fused step block-major and packed (fusedFaceCellKernel<..., PACKW = 2>; qgd_setup.hpp FusedBlocks::fW16 / fKC):
on a mesh whose vertex weights pack and whose linear weights w lie within 65 535 bit patterns of each other, with hQGDf in at most four such
classes -- every uniform box -- w, hQGDf and the kind of a block's face slots are one word and one byte per slot in the block's own order, read in
the list round without the face label, and the doubles are formed in the face loop: reference + offset, integer arithmetic, the stored double
exactly.  So every case here is BIT FOR BIT (np.array_equal after 5 steps, the fields of tests/test_fused_front_loads_gpu.py)

    against the three-kernel step, and
    against the same device built with QGD_FUSED_PACKED_F=0 (w / hQGDf / kind gathered by label, the kernel as it was),

and every arm asserts that `packedFaces` is what it expects and that the fused kernel ran.

    box(17,9,9), box(40,20,20)   plain, upwind and Courant-control arms; two classes of hQGDf; full bricks beside rim blocks
    box(16,8,12)                 three classes of hQGDf
    box(3,2,2), box(1,1,40)      three of four waves issue the front-loaded group under an empty mask.  box(1,1,40) has no interior vertex: its
                                 weights do not pack, so its faces do not either, and the kernel that runs is level 0
    box(16,8,12).shard(2, .)     firstBlock != 0: the boundary-layer blocks in a launch of their own
    QGD_FUSED_TEMPLATES=0        the template offset grows with the block; the face tables are per block either way
    IMPL on box(9,5,5)           to 1e-13 relative and with equal iteration counts, as tests/test_implicit_diffusion.py compares the assembly
    c5_mesh(16, 8**3, poly)      jittered polyhedra: not packed, still bit-identical
    prism543                     uniform prisms (triangles among the faces): bit-identical whichever way the rule decides; the decision is printed
"""
import contextlib
import os

import numpy as np
import pytest

import qgdsolver_amd as q

from test_config5_gpu import c5_mesh
from test_fused_front_loads_gpu import ARMS, FIELDS, STEPS, run
from test_fused_step_gpu import equal, shard_run
from util import make_mesh

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def packed_f(on):
    """QGD_FUSED_PACKED_F while a device builds its tables: unset (the default: pack where the mesh allows it) or 0"""
    old = os.environ.pop("QGD_FUSED_PACKED_F", None)
    if not on:
        os.environ["QGD_FUSED_PACKED_F"] = "0"
    try:
        yield
    finally:
        os.environ.pop("QGD_FUSED_PACKED_F", None)
        if old is not None:
            os.environ["QGD_FUSED_PACKED_F"] = old


def packed_faces_of(mesh):
    """what a device of this mesh reports (the run's info comes from the case: the device's own figure says which tables it holds)"""
    dev = q.Device(mesh, fused_tables="any")
    b = dev.fused_blocks()
    dev.close()
    return b["packedFaces"], b["packedWeights"]


def three_arms(mesh, arm, tag, packs):
    """three kernels / fused with the streams gathered by label / fused with whatever the mesh allows: all three bit-identical.
    packs = None: whichever way the rule decides"""
    opt, key = ARMS[arm]
    ref, _, _ = run(mesh, False, key, **opt)
    with packed_f(False):
        full, i_full, _ = run(mesh, True, key, **opt)
    with packed_f(True):
        got, i_got, _ = run(mesh, True, key, **opt)
    assert i_full["packedFaces"] is False, (tag, i_full)
    if packs is not None:
        assert i_got["packedFaces"] is packs, (tag, i_got)
    assert not i_got["packedFaces"] or i_got["packedWeights"], (tag, i_got)   # faces pack only where the weights do
    assert i_full["packedWeights"] == i_got["packedWeights"], (tag, i_full, i_got)   # the switch touches the face streams alone
    assert i_got["blocks"] == i_full["blocks"] >= (mesh.nCells + 127) // 128, (i_got, i_full)
    worst = {k: (float(np.abs(ref[k] - got[k]).max()), float(np.abs(full[k] - got[k]).max())) for k in ref}
    print(f"{tag} {arm}: blocks {i_got['blocks']}, packed faces {i_got['packedFaces']}, weights {i_got['packedWeights']}, "
          f"max |packed - three kernels|, |packed - by label| {worst}")
    for k in ref:
        assert np.isfinite(got[k]).all(), (tag, arm, k)
        assert np.array_equal(ref[k], got[k]), (tag, arm, k, "three kernels", worst[k])
        assert np.array_equal(full[k], got[k]), (tag, arm, k, "by label", worst[k])
    return i_got


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("shape", [(17, 9, 9), (40, 20, 20)])
def test_packed_faces_on_many_blocks(shape, arm):
    ib = three_arms(q.PolyMesh.box(*shape), arm, f"box{shape}", True)
    assert ib["blocks"] > 8, ib
    if shape == (40, 20, 20):
        assert ib["blocks"] == 125, ib


def test_packed_faces_with_three_classes_of_hqgdf():
    three_arms(q.PolyMesh.box(16, 8, 12), "plain", "box(16, 8, 12)", True)


@pytest.mark.parametrize("shape,packs", [((3, 2, 2), True), ((1, 1, 40), False)])
def test_packed_faces_on_blocks_below_a_wavefront(shape, packs):
    three_arms(q.PolyMesh.box(*shape), "plain", f"box{shape}", packs)


@pytest.mark.parametrize("which", [0, 1])
def test_packed_faces_on_a_shard(which):
    shard = q.PolyMesh.box(16, 8, 12).shard(2, which)
    for on in (False, True):
        with packed_f(on):
            dev = q.Device(shard, fused_tables="any")
            case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3, mu=1e-3))
            info, blocks = case.fused_info(), dev.fused_blocks()
            case.close(); dev.close()
        assert info["fused"] and 0 < info["layerBlocks"] < info["blocks"], info   # the second launch starts at block layerBlocks
        assert info["packedFaces"] is on and blocks["packedFaces"] is on, (on, info, blocks)
        assert info["packedWeights"] and blocks["packedWeights"], (on, info, blocks)
    ref = shard_run(shard, False, (0, 1), steps=STEPS)
    with packed_f(False):
        full = shard_run(shard, True, (0, 10, 11), steps=STEPS)   # (asserts that the fused kernel steps the shard)
    with packed_f(True):
        got = shard_run(shard, True, (0, 10, 11), steps=STEPS)
    equal(ref, got, ("box16x8x12", 2, which, "three kernels"))
    equal(full, got, ("box16x8x12", 2, which, "by label"))


def test_packed_faces_with_one_template_per_block(monkeypatch):
    monkeypatch.setenv("QGD_FUSED_TEMPLATES", "0")   # read when the device builds its tables
    ib = three_arms(q.PolyMesh.box(17, 9, 9), "plain", "box17x9x9, own templates", True)
    assert ib["templates"] == ib["blocks"] > 8, ib   # the variable took effect: no two blocks share a template


def test_packed_faces_in_the_implicit_assembly():
    mesh = q.PolyMesh.box(9, 5, 5)
    fields = FIELDS + ("phiTauMC", "phiSigmaDotU")
    opt = dict(deltaT=1e-3, mu=1e-2, implicitDiffusion=1)
    ref, _, i_ref = run(mesh, False, "fusedImplicit", fields=fields, **opt)
    with packed_f(False):
        full, b_full, i_full = run(mesh, True, "fusedImplicit", fields=fields, **opt)
    with packed_f(True):
        got, b_got, i_got = run(mesh, True, "fusedImplicit", fields=fields, **opt)
    assert b_full["packedFaces"] is False and b_got["packedFaces"] is True, (b_full, b_got)
    assert b_got["blocks"] >= (mesh.nCells + 127) // 128, b_got
    for other, impl, what in ((ref, i_ref, "separate kernels"), (full, i_full, "by label")):
        worst = {k: float(np.abs(other[k] - got[k]).max()) for k in got}
        print(f"box9x5x5 implicit: blocks {b_got['blocks']}, max |packed - {what}| {worst}")
        for k in got:
            assert np.isfinite(got[k]).all(), k
            assert worst[k] <= 1e-13 * max(np.abs(other[k]).max(), 1e-300), (what, k, worst[k])
        assert impl["solves"] == i_got["solves"], (what, impl, i_got)


def test_a_jittered_polyhedral_mesh_does_not_pack():
    three_arms(c5_mesh(16, 8 ** 3, poly=True), "plain", "c5poly", False)


def test_uniform_prisms_whichever_way_the_rule_decides():
    mesh = make_mesh("prism543")
    faces, weights = packed_faces_of(mesh)
    print(f"prism543: the rule decides packed faces {faces}, packed weights {weights}")
    ib = three_arms(mesh, "plain", "prism543", None)
    assert ib["packedFaces"] is faces, (ib, faces)
