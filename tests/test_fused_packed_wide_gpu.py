"""The device decode of the packed tables of the fused step at offsets that use all 16 bits (fusedFaceCellKernel<..., PACKW = 1 | 2>: (1b) and the
face loop of qgd_kernels.hip, fuWeightFromOffset / fuVertexWeight of qgd_device.hpp; qhdFusedAdvanceKernel, the packed vertex weights' other
reader).  Every mesh that reached the GPU in a packed state before was a uniform box, whose offsets stay below 128: a decode that takes the low
byte alone, a register read before its load arrived (reference + 0), or the fourth class of hQGDf read as another would have passed there
(tests/test_fused_packed_wide_host.py counts exactly that on the host).  The meshes here are the recipes of tests/packed_wide_recipes.py: boxes
whose interior points are moved by ~1e-12 of the cell size, which still pack and whose offsets fill the half words -- an offset left out is an
error of 1e-12 relative or more in a weight, ten times the tolerance of the loosest comparison below.

Every case first asserts the recipe's expectation on what the device reports (Device.fused_blocks(): packedWeights, packedFaces, hfClasses,
maxWeightOffset, maxFaceOffset), so the kernel is known to have decoded wide offsets, and every fused arm asserts that the fused kernel ran.

    main kernel        BIT FOR BIT after 5 steps between the three-kernel step, the fused step with QGD_FUSED_PACKED_W=0 (level 0), with
                       QGD_FUSED_PACKED_F=0 (level 1: weights packed, faces by label) and as the mesh allows (level 2): the two-class,
                       three-classes-by-split and FOUR-class 17x9x9 recipes under every arm of ARMS, the 16x8x12 recipe plain
    level boundaries   a recipe whose weights pack and faces do not (level 1), one where nothing packs (level 0)
    below a wavefront  box(3,2,2) and box(5,4,3)
    shards             both halves of the two-class recipe (every block touches the cut) and of the 16x8x12 recipe (firstBlock != 0 in the
                       second launch); each shard decides for itself whether it packs, and what it decided is printed
    own templates      QGD_FUSED_TEMPLATES=0 on the four-class recipe
    IMPL               box(9,5,5): to 1e-13 relative against the separate kernels with equal solve counts; packed against unpacked bit for bit
    QHD                qhdFusedAdvanceKernel on uniform box(17,9,9) and the two-class recipe: packed against QGD_FUSED_PACKED_W=0
"""
import numpy as np
import pytest

import qgdsolver_amd as q

import packed_wide_recipes as recipes
from packed_wide_recipes import RECIPES, WIDE
from test_fused_front_loads_gpu import ARMS, FIELDS, STEPS, run
from test_fused_packed_faces_gpu import packed_f
from test_fused_packed_weights_gpu import packed_w, three_arms
from test_fused_step_gpu import equal, shard_run

pytestmark = pytest.mark.gpu


def blocks_of(mesh):
    """what a device of this mesh reports about its tables, under the switches in force"""
    dev = q.Device(mesh, fused_tables="any")
    b = dev.fused_blocks()
    dev.close()
    return b


def expected(r, mesh):
    return recipes.check(r, blocks_of(mesh))


def all_levels(r, arm):
    """three kernels / level 0 / level 1 / whatever the mesh allows: bit-identical.  Returns what the device reports."""
    mesh = recipes.mesh_of(r)
    got_blocks = expected(r, mesh)
    opt, key = ARMS[arm]
    ref, _, _ = run(mesh, False, key, **opt)
    with packed_w(False):
        lvl0, i0, _ = run(mesh, True, key, **opt)
    with packed_f(False):
        lvl1, i1, _ = run(mesh, True, key, **opt)
    got, i2, _ = run(mesh, True, key, **opt)
    assert not i0["packedWeights"] and not i0["packedFaces"], (r.tag, i0)
    assert i1["packedWeights"] is r.packedWeights and not i1["packedFaces"], (r.tag, i1)
    assert i2["packedWeights"] is r.packedWeights and i2["packedFaces"] is r.packedFaces, (r.tag, i2)
    assert i0["blocks"] == i1["blocks"] == i2["blocks"] >= (mesh.nCells + 127) // 128, (i0, i1, i2)
    others = (("three kernels", ref), ("level 0", lvl0), ("level 1", lvl1))
    worst = {k: [float(np.abs(o[k] - got[k]).max()) for _, o in others] for k in ref}
    print(f"{r.tag} {arm}: blocks {i2['blocks']}, max |as the mesh allows - three kernels, level 0, level 1| {worst}")
    for k in ref:
        assert np.isfinite(got[k]).all(), (r.tag, arm, k)
        for (what, o), d in zip(others, worst[k]):
            assert np.array_equal(o[k], got[k]), (r.tag, arm, k, what, d)
    return got_blocks


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("tag", ["two classes", "three classes by split", "four classes"])
def test_wide_offsets_on_many_blocks(tag, arm):
    b = all_levels(RECIPES[tag], arm)
    if tag == "four classes":
        assert b["hfClasses"] == 4 and b["maxFaceOffset"] >= WIDE, b   # fv[6], cls == 3, runs on the device
    if tag != "two classes":
        assert b["maxWeightOffset"] >= 28000, b                      # all but the last 4768 patterns of the half word


def test_wide_offsets_with_three_spacings():
    all_levels(RECIPES["three spacings"], "plain")


@pytest.mark.parametrize("tag", ["weights only", "nothing packs"])
def test_wide_offsets_at_the_level_boundaries(tag):
    r = RECIPES[tag]
    mesh = recipes.mesh_of(r)
    expected(r, mesh)
    i_got = three_arms(mesh, "plain", r.tag, r.packedWeights)   # three kernels / QGD_FUSED_PACKED_W=0 / as the mesh allows
    assert i_got["packedFaces"] is False, i_got                 # level 1, or level 0: never level 2


@pytest.mark.parametrize("tag", ["12 cells", "60 cells"])
def test_wide_offsets_on_blocks_below_a_wavefront(tag):
    all_levels(RECIPES[tag], "plain")


@pytest.mark.parametrize("tag", ["two classes", "three spacings"])
def test_wide_offsets_on_shards(tag):
    """17x9x9 cut in two: every block of a half touches the cut (layerBlocks == blocks, one launch does it all); 16x8x12: the boundary-layer
    blocks in a launch of their own and the second launch starting at block layerBlocks, as on the uniform box of the tests before"""
    r = RECIPES[tag]
    mesh = recipes.mesh_of(r)
    decided = []
    for which in (0, 1):
        shard = mesh.shard(2, which)
        b = blocks_of(shard)
        decided.append(b)
        print(f"{r.tag}, shard {which} of 2: " + str({k: b[k] for k in ("blocks", "layerBlocks", "packedWeights", "packedFaces", "hfClasses", "maxWeightOffset", "maxFaceOffset")}))
        assert 0 < b["layerBlocks"] <= b["blocks"], b
        if tag == "three spacings":
            assert b["layerBlocks"] < b["blocks"], b   # the second launch starts at block layerBlocks
        ref = shard_run(shard, False, (0, 1), steps=STEPS)
        with packed_w(False):
            assert not blocks_of(shard)["packedWeights"]
            lvl0 = shard_run(shard, True, (0, 10, 11), steps=STEPS)   # (asserts that the fused kernel steps the shard)
        with packed_f(False):
            assert not blocks_of(shard)["packedFaces"]
            lvl1 = shard_run(shard, True, (0, 10, 11), steps=STEPS)
        got = shard_run(shard, True, (0, 10, 11), steps=STEPS)
        equal(ref, got, (r.tag, 2, which, "three kernels"))
        equal(lvl0, got, (r.tag, 2, which, "level 0"))
        equal(lvl1, got, (r.tag, 2, which, "level 1"))
    assert any(b["packedWeights"] and b["maxWeightOffset"] >= WIDE for b in decided), decided


def test_wide_offsets_with_one_template_per_block(monkeypatch):
    monkeypatch.setenv("QGD_FUSED_TEMPLATES", "0")   # read when the device builds its tables
    b = all_levels(RECIPES["four classes"], "plain")
    assert b["templates"] == b["blocks"] > 8, b      # the variable took effect: no two blocks share a template
    assert b["hfClasses"] == 4, b


def test_wide_offsets_in_the_implicit_assembly():
    """Against the separate kernels: 1e-13 relative and equal solve counts, the bound the assembly has always been compared at -- which an offset
    left out (1e-12 or more in a weight on this mesh) no longer fits under.  Packed against QGD_FUSED_PACKED_W=0 and against
    QGD_FUSED_PACKED_F=0: measured on the MI355X, the largest difference is 0 in every field, so those two arms are held to np.array_equal."""
    r = RECIPES["implicit"]
    mesh = recipes.mesh_of(r)
    expected(r, mesh)
    fields = FIELDS + ("phiTauMC", "phiSigmaDotU")
    opt = dict(deltaT=1e-3, mu=1e-2, implicitDiffusion=1)
    ref, _, i_ref = run(mesh, False, "fusedImplicit", fields=fields, **opt)
    with packed_w(False):
        lvl0, b0, i_0 = run(mesh, True, "fusedImplicit", fields=fields, **opt)
    with packed_f(False):
        lvl1, b1, i_1 = run(mesh, True, "fusedImplicit", fields=fields, **opt)
    got, b2, i_got = run(mesh, True, "fusedImplicit", fields=fields, **opt)
    assert not b0["packedWeights"] and not b0["packedFaces"] and b1["packedWeights"] and not b1["packedFaces"], (b0, b1)
    assert b2["packedWeights"] and b2["packedFaces"] and b2["blocks"] >= (mesh.nCells + 127) // 128, b2
    for other, impl, what, exact in ((ref, i_ref, "separate kernels", False), (lvl0, i_0, "QGD_FUSED_PACKED_W=0", True), (lvl1, i_1, "QGD_FUSED_PACKED_F=0", True)):
        worst = {k: float(np.abs(other[k] - got[k]).max()) for k in got}
        print(f"{r.tag}: blocks {b2['blocks']}, max |packed - {what}| {worst}")
        for k in got:
            assert np.isfinite(got[k]).all(), k
            assert worst[k] <= 1e-13 * max(np.abs(other[k]).max(), 1e-300), (what, k, worst[k])
            if exact:
                assert np.array_equal(other[k], got[k]), (what, k, worst[k])
        assert impl["solves"] == i_got["solves"], (what, impl, i_got)


@pytest.mark.parametrize("tag", ["uniform box(17,9,9)", "two classes"])
def test_wide_offsets_in_the_qhd_advance(tag, monkeypatch):
    """qhdFusedAdvanceKernel reads the packed table through fuVertexWeight: one instantiation, a branch on the table that is there, so packed
    and unpacked are expected bit-identical -- provided the unpacked arm repeats itself, which is measured first."""
    from test_qhd_fused_gpu import FIELDS as QHD_FIELDS, _run
    monkeypatch.setenv("QGD_QHD_FUSED", "1")
    if tag == "two classes":
        mesh = recipes.mesh_of(RECIPES[tag])
        b = expected(RECIPES[tag], mesh)
        assert b["maxWeightOffset"] >= WIDE, b
    else:
        mesh = q.PolyMesh.box(17, 9, 9)
        assert blocks_of(mesh)["packedWeights"]
    with packed_w(False):
        assert not blocks_of(mesh)["packedWeights"]
        full_a, fa, _ = _run(mesh, "any", 6)
        full_b, fb, _ = _run(mesh, "any", 6)
    assert blocks_of(mesh)["packedWeights"]
    got, fg, info = _run(mesh, "any", 6)
    assert fa["fusedAdvance"] and fb["fusedAdvance"] and fg["fusedAdvance"] and fg["blocks"] > 0, (fa, fb, fg)
    assert info["steps"] == 6
    noise = {k: float(np.abs(full_a[k] - full_b[k]).max()) for k in QHD_FIELDS}
    diff = {k: float(np.abs(full_a[k] - got[k]).max()) for k in QHD_FIELDS}
    reproducible = all(np.array_equal(full_a[k], full_b[k]) for k in QHD_FIELDS)
    print(f"QHD {tag}: unpacked arm run to run {noise} (reproducible: {reproducible}); packed - unpacked {diff}")
    for k in QHD_FIELDS:
        assert np.isfinite(got[k]).all(), (tag, k)
        if reproducible:
            assert np.array_equal(full_a[k], got[k]), (tag, k, diff[k])
        else:
            assert diff[k] <= 4 * noise[k], (tag, k, diff[k], noise[k])
    if tag == "two classes":   # and the comparison this kernel had before, on the mesh with wide offsets
        sep, fs, _ = _run(mesh, False, 6)
        assert not fs["fusedAdvance"], fs
        for k in QHD_FIELDS:
            scale = max(np.abs(sep[k]).max(), 1e-300)
            assert k == "U.boundary" or np.abs(sep[k]).max() > 0
            assert np.abs(got[k] - sep[k]).max() <= 1e-11 * scale, (tag, k, np.abs(got[k] - sep[k]).max() / scale)
