"""The vertex weights of the fused step as 16-bit offsets (fusedFaceCellKernel<..., PACKW>; qgd_setup.hpp FusedBlocks::vW16): on a mesh whose
weights all lie within 65 535 bit patterns of each other -- every uniform box -- a vertex's eight weights are one 16-byte load of offsets from
one reference pattern, and the doubles are formed behind the staging barrier: reference + offset, integer arithmetic, the stored double exactly.
So every case here is BIT FOR BIT (np.array_equal after 5 steps, the fields of tests/test_fused_front_loads_gpu.py)

    against the three-kernel step, and
    against the same device built with QGD_FUSED_PACKED_W=0 (the full table of doubles, the kernel as it was),

and every arm asserts that `packedWeights` is what it expects and that the fused kernel ran.

    box(17,9,9), box(40,20,20)   plain, upwind and Courant-control arms; full bricks beside rim blocks; a block count that is no multiple of the
                                 XCD run
    box(3,2,2), box(1,1,40)      three of four waves issue the front-loaded group under an empty mask.  box(1,1,40) has no interior vertex, so
                                 no vertex has cells (capPE is not 8): by the rule it does NOT pack, and the kernel that runs is the unpacked one
    box(16,8,12).shard(2, .)     firstBlock != 0: the boundary-layer blocks in a launch of their own
    QGD_FUSED_TEMPLATES=0        the template offset grows with the block, the weights' offset does too (they are per block either way)
    IMPL on box(9,5,5)           to rounding and with equal iteration counts, as tests/test_implicit_diffusion.py compares the assembly
    c5_mesh(16, 8**3, poly)      jittered polyhedra: not packed, still bit-identical
"""
import contextlib
import os

import numpy as np
import pytest

import qgdsolver_amd as q

from test_config5_gpu import c5_mesh
from test_fused_front_loads_gpu import ARMS, FIELDS, STEPS, run
from test_fused_step_gpu import equal, shard_run

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def packed_w(on):
    """QGD_FUSED_PACKED_W while a device builds its tables: unset (the default: pack where the mesh allows it) or 0"""
    old = os.environ.pop("QGD_FUSED_PACKED_W", None)
    if not on:
        os.environ["QGD_FUSED_PACKED_W"] = "0"
    try:
        yield
    finally:
        os.environ.pop("QGD_FUSED_PACKED_W", None)
        if old is not None:
            os.environ["QGD_FUSED_PACKED_W"] = old


def three_arms(mesh, arm, tag, packs):
    """three kernels / fused with the full table / fused with whatever the mesh allows: all three bit-identical"""
    opt, key = ARMS[arm]
    ref, _, _ = run(mesh, False, key, **opt)
    with packed_w(False):
        full, i_full, _ = run(mesh, True, key, **opt)
    with packed_w(True):
        got, i_got, _ = run(mesh, True, key, **opt)
    assert i_full["packedWeights"] is False, (tag, i_full)
    assert i_got["packedWeights"] is packs, (tag, i_got)
    assert i_got["blocks"] == i_full["blocks"] >= (mesh.nCells + 127) // 128, (i_got, i_full)
    worst = {k: (float(np.abs(ref[k] - got[k]).max()), float(np.abs(full[k] - got[k]).max())) for k in ref}
    print(f"{tag} {arm}: blocks {i_got['blocks']}, packed {i_got['packedWeights']}, max |packed - three kernels|, |packed - full table| {worst}")
    for k in ref:
        assert np.isfinite(got[k]).all(), (tag, arm, k)
        assert np.array_equal(ref[k], got[k]), (tag, arm, k, "three kernels", worst[k])
        assert np.array_equal(full[k], got[k]), (tag, arm, k, "full table", worst[k])
    return i_got


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("shape", [(17, 9, 9), (40, 20, 20)])
def test_packed_weights_on_many_blocks(shape, arm):
    ib = three_arms(q.PolyMesh.box(*shape), arm, f"box{shape}", True)
    assert ib["blocks"] > 8, ib
    if shape == (40, 20, 20):
        assert ib["blocks"] == 125, ib


@pytest.mark.parametrize("shape,packs", [((3, 2, 2), True), ((1, 1, 40), False)])
def test_packed_weights_on_blocks_below_a_wavefront(shape, packs):
    three_arms(q.PolyMesh.box(*shape), "plain", f"box{shape}", packs)


@pytest.mark.parametrize("which", [0, 1])
def test_packed_weights_on_a_shard(which):
    shard = q.PolyMesh.box(16, 8, 12).shard(2, which)
    for on in (False, True):
        with packed_w(on):
            dev = q.Device(shard, fused_tables="any")
            case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3, mu=1e-3))
            info, blocks = case.fused_info(), dev.fused_blocks()
            case.close(); dev.close()
        assert info["fused"] and 0 < info["layerBlocks"] < info["blocks"], info   # the second launch starts at block layerBlocks
        assert info["packedWeights"] is on and blocks["packedWeights"] is on, (on, info, blocks)
    ref = shard_run(shard, False, (0, 1), steps=STEPS)
    with packed_w(False):
        full = shard_run(shard, True, (0, 10, 11), steps=STEPS)   # (asserts that the fused kernel steps the shard)
    with packed_w(True):
        got = shard_run(shard, True, (0, 10, 11), steps=STEPS)
    equal(ref, got, ("box16x8x12", 2, which, "three kernels"))
    equal(full, got, ("box16x8x12", 2, which, "full table"))


def test_packed_weights_with_one_template_per_block(monkeypatch):
    monkeypatch.setenv("QGD_FUSED_TEMPLATES", "0")   # read when the device builds its tables
    ib = three_arms(q.PolyMesh.box(17, 9, 9), "plain", "box17x9x9, own templates", True)
    assert ib["templates"] == ib["blocks"] > 8, ib   # the variable took effect: no two blocks share a template


def test_packed_weights_in_the_implicit_assembly():
    mesh = q.PolyMesh.box(9, 5, 5)
    fields = FIELDS + ("phiTauMC", "phiSigmaDotU")
    opt = dict(deltaT=1e-3, mu=1e-2, implicitDiffusion=1)
    ref, _, i_ref = run(mesh, False, "fusedImplicit", fields=fields, **opt)
    with packed_w(False):
        full, b_full, i_full = run(mesh, True, "fusedImplicit", fields=fields, **opt)
    with packed_w(True):
        got, b_got, i_got = run(mesh, True, "fusedImplicit", fields=fields, **opt)
    assert b_full["packedWeights"] is False and b_got["packedWeights"] is True, (b_full, b_got)
    assert b_got["blocks"] >= (mesh.nCells + 127) // 128, b_got
    for other, impl, what in ((ref, i_ref, "separate kernels"), (full, i_full, "full table")):
        worst = {k: float(np.abs(other[k] - got[k]).max()) for k in got}
        print(f"box9x5x5 implicit: blocks {b_got['blocks']}, max |packed - {what}| {worst}")
        for k in got:
            assert np.isfinite(got[k]).all(), k
            assert worst[k] <= 1e-13 * max(np.abs(other[k]).max(), 1e-300), (what, k, worst[k])
        assert impl["solves"] == i_got["solves"], (what, impl, i_got)


def test_a_jittered_polyhedral_mesh_does_not_pack():
    three_arms(c5_mesh(16, 8 ** 3, poly=True), "plain", "c5poly", False)
