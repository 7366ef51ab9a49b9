"""The two ends of a block of the fused step (fusedFaceCellKernel).

The head: the launcher divides for the XCD order of the blocks once per launch (the blocks inside whole spans of eight runs, the run's
logarithm), so a run that is a power of two costs the kernel two shifts and a mask; any other run keeps xcdTile's divisions.

The end: the block's slot of the positivity monitor (max -rho, min e since the last query) is read in round 1, in front of the records, and
parked in LDS; waves 0 and 1 fold their rows of sixteen lanes in the vector unit, and thread 0 folds the eight row pairs into the parked
value and stores it -- no load behind the last barrier.

Each fused arm against the three-kernel step BIT FOR BIT (np.array_equal after 5 steps, the monitor's minima included), and every fused
arm asserts that the fused kernel is what ran:

    monitor         box(17,9,9) with a dip of density and energy that fills in: the first step's minimum is the lowest, so a slot that lost
                    its history, or kept a stale one across the reset of a query, shows
    block index     box(40,20,20), 125 blocks, no multiple of a span: QGD_FU_XCD_RUN 64 (no whole span), 4 (three spans and a tail), 3 (the
                    division path); shards of box(16,8,12) and box(16,8,40), whose second launch starts at firstBlock != 0 (runs 64, 1, 3)
    block shapes    box(3,2,2), box(1,1,40): wave 1 carries no cell at all; box(17,9,9); triangles and polygons -- plain, upwind,
                    Courant control (whose blocks leave Courant partials instead, by the reduction all kernels share)
    IMPL            box(9,5,5): the implicit assembly has no monitor slot but the same head (to rounding, same iteration counts)"""
import numpy as np
import pytest

import qgdsolver_amd as q

import cases
from test_config5_gpu import c5_mesh
from test_fused_front_loads_gpu import ARMS, FIELDS, STEPS, bit_identical, run

pytestmark = pytest.mark.gpu


# ---- the monitor across steps ---------------------------------------------------------------------------------------------------------
def dip_case(mesh, fused):
    dev = q.Device(mesh, fused_tables="any" if fused else False)
    case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=2e-4, mu=1e-3))
    assert case.fused_info()["fused"] == fused
    C = mesh.array("C").reshape(-1, 3)
    U, T, p = cases.box_initial_fields(C)
    g = np.exp(-((C - np.array([0.25, 0.5, 0.5])) ** 2).sum(axis=1) / 0.02)
    T = T * (1.0 - 0.2 * g)            # e = cv T dips by 20 %, rho = p / (R T) by 12.5 %
    p = p * (1.0 - 0.3 * g)
    case.set_fields(U, T, p)
    return dev, case


def mins(case):
    i = case.info()
    return np.array([i["minRho"], i["minE"]])


def monitor_history(fused):
    """(minima over six steps in one query, the six single-step minima of a second run, a seventh step's own minima after the query)"""
    mesh = q.PolyMesh.box(17, 9, 9)
    dev, case = dip_case(mesh, fused)
    case.step(6)
    six = mins(case)
    case.step(1)
    seventh = mins(case)
    case.close(); dev.close()
    dev, case = dip_case(mesh, fused)
    single = []
    for _ in range(7):
        case.step(1)
        single.append(mins(case))
    case.close(); dev.close()
    return six, np.array(single), seventh


def test_monitor_keeps_the_lowest_value_across_steps_and_forgets_it_with_a_query():
    six, single, seventh = monitor_history(True)
    six3, single3, seventh3 = monitor_history(False)
    print(f"fused: six steps {six}, single steps {single.tolist()}, seventh {seventh}")
    # the case is what it claims: the dip fills in, so the first step's minima are the lowest and a slot that forgot them would show
    assert (single[0] < single[1:6].min(axis=0)).all(), single
    assert np.array_equal(six, single[:6].min(axis=0)), (six, single)
    assert np.array_equal(six, single[0]), (six, single)
    # after the query the slot starts again: the seventh step reports its own minima, not the first step's
    assert np.array_equal(seventh, single[6]), (seventh, single)
    assert (seventh > six).all(), (seventh, six)
    # and all of it is what the three kernels report
    assert np.array_equal(six, six3) and np.array_equal(single, single3) and np.array_equal(seventh, seventh3), (six, six3, seventh, seventh3)


# ---- the block index ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three_kernels_40_20_20():
    """the three-kernel step of box(40,20,20) per arm, computed once: the run of the fused blocks does not touch it"""
    mesh = q.PolyMesh.box(40, 20, 20)
    return mesh, {arm: run(mesh, False, ARMS[arm][1], **ARMS[arm][0])[0] for arm in ("plain", "adjust")}


@pytest.mark.parametrize("arm", ["plain", "adjust"])
@pytest.mark.parametrize("xcd_run", [64, 4, 3])
def test_block_index_with_and_without_the_division(xcd_run, arm, three_kernels_40_20_20, monkeypatch):
    monkeypatch.setenv("QGD_FU_XCD_RUN", str(xcd_run))   # read when the device is built
    mesh, ref = three_kernels_40_20_20
    opt, key = ARMS[arm]
    b, ib, _ = run(mesh, True, key, **opt)
    assert ib["blocks"] == 125, ib                       # run 64: no whole span; 4: 96 blocks in spans, 29 behind; 3: 120 and 5
    for k in ref[arm]:
        assert np.isfinite(b[k]).all(), (xcd_run, arm, k)
        assert np.array_equal(ref[arm][k], b[k]), (xcd_run, arm, k, float(np.abs(ref[arm][k] - b[k]).max()))


def shard_steps(shard, fused, order):
    dev = q.Device(shard, fused_tables="any" if fused else False)
    case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3, mu=1e-3))
    U, T, p = cases.box_initial_fields(shard.array("C").reshape(-1, 3))
    case.set_fields(U, T, p)
    info = case.fused_info()
    assert info["fused"] == fused, info
    for _ in range(STEPS):              # no exchange: the ghost cells keep their values, in both runs
        for ph in order:
            case.step_phase(ph)
    case.sync()
    out = {n: case.field(n).copy() for n in FIELDS}
    out["mins"] = mins(case)
    case.close(); dev.close()
    return out, info


@pytest.mark.parametrize("shape,xcd_run", [((16, 8, 12), 64), ((16, 8, 40), 1), ((16, 8, 40), 3)])
@pytest.mark.parametrize("which", [0, 1])
def test_block_index_of_a_launch_that_starts_behind_block_zero(which, shape, xcd_run, monkeypatch):
    monkeypatch.setenv("QGD_FU_XCD_RUN", str(xcd_run))   # run 1: spans of eight blocks, so the second launch holds whole spans and a tail
    shard = q.PolyMesh.box(*shape).shard(2, which)
    ref, _ = shard_steps(shard, False, (0, 1))
    got, info = shard_steps(shard, True, (0, 10, 11))
    print(f"box{shape} shard {which} of 2, run {xcd_run}: blocks {info['blocks']}, of them boundary layer {info['layerBlocks']}")
    assert 0 < info["layerBlocks"] < info["blocks"], info   # the second launch starts at block layerBlocks, with a `full` of its own
    if xcd_run == 1:
        assert info["blocks"] - info["layerBlocks"] > 8, info
    for k in ref:
        assert np.isfinite(got[k]).all(), (which, shape, xcd_run, k)
        assert np.array_equal(ref[k], got[k]), (which, shape, xcd_run, k, float(np.abs(ref[k] - got[k]).max()))


# ---- block shapes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("name", ["box3x2x2", "box1x1x40", "box17x9x9", "c5poly"])
def test_block_ends_on_small_partial_and_polyhedral_blocks(name, arm):
    mesh = {"box3x2x2": lambda: q.PolyMesh.box(3, 2, 2), "box1x1x40": lambda: q.PolyMesh.box(1, 1, 40),
            "box17x9x9": lambda: q.PolyMesh.box(17, 9, 9), "c5poly": lambda: c5_mesh(16, 8 ** 3, poly=True)}[name]()
    bit_identical(mesh, arm, name)


def test_block_head_in_the_implicit_assembly():
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
