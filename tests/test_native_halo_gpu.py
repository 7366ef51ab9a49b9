"""The library's own RCCL halo transport (qgd_comm_*, qgd_case_halo_exchange, qgd_case_step_sharded) on the one GPU of the
test box: a one-rank communicator, a no-op on an unsharded case, and the pack -> ncclSend/ncclRecv to self -> unpack loop on
the middle slab of a three-slab cut (its two halo slots talk to rank 0 = itself, so the ghost planes receive the case's own
boundary layers: not a physical set-up, but every byte goes through the packed message, RCCL and the unpack kernel).
N > 1 ranks over xGMI cannot run here (one GPU per box): that leg is covered by the driver's scaling run only.

The same loop carries every other message kind of the two case types (the implicitDiffusion branch's, the mid-assembly one, the
QHD case's): each is pinned here against the same case driven phase by phase from Python with a loopback world in the
transport's place, bit for bit -- both arms launch the same kernels in the same order."""
import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import qhdfoam
from qgdsolver_amd.halo import (IMPL_MID, IMPL_STATE, QHD_PRESSURE, QHD_STATE, ImplicitShard, ImplicitStepper, LocalWorld, NativeComm,
                                QhdStepper)

import cases
from test_partition import mixed_bcs
from test_qhd_case import WALL, cavity_bcs, initial, options

pytestmark = pytest.mark.gpu


def test_one_rank_communicator_and_unsharded_noop():
    comm = NativeComm(0)
    mesh = q.PolyMesh.box(8, 7, 6)
    dev = q.Device(mesh)
    case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3, mu=1e-3))
    U, T, p = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    case.set_fields(U, T, p)
    ref = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3, mu=1e-3))
    ref.set_fields(U, T, p)
    ref.step(4)
    for _ in range(4):
        comm.step(case, [], overlapped=False)     # unsharded: assemble + advance, nothing to exchange
    case.sync()
    comm.allreduce_max(case)                      # one rank: no-op
    for f in ("rho", "U", "p"):
        assert np.array_equal(case.field(f), ref.field(f)), f
    case.close(); ref.close(); dev.close(); comm.close()


@pytest.mark.parametrize("overlapped", [False, True])
def test_self_exchange_moves_the_boundary_layers_through_rccl(overlapped):
    nx, ny, n = 9, 8, 12
    plane = nx * ny
    comm = NativeComm(0)
    mesh = q.PolyMesh.box(nx, ny, n, k_range=(3, 9))          # planes 3..8: ghost 3, owned 4..7, ghost 8
    dev = q.Device(mesh)
    case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3, mu=1e-3))
    U, T, p = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    case.set_fields(U, T, p)
    assert case.halo_count(0) == case.halo_recv_count(0) == case.halo_count(1) == case.halo_recv_count(1) > 8 * plane
    comm.exchange(case, [0, 0])
    case.sync()
    rho, Uf = case.field("rho").reshape(6, plane), case.field("U").reshape(6, plane, 3)
    # sends to self are matched with receives in issue order: slot 0's message (lowest owned plane) lands in slot 0's ghost plane
    assert np.array_equal(rho[0], rho[1]) and np.array_equal(Uf[0], Uf[1])
    assert np.array_equal(rho[5], rho[4]) and np.array_equal(Uf[5], Uf[4])
    # steps through the library's own choreography stay finite and keep moving the layers
    for _ in range(3):
        comm.step(case, [0, 0], overlapped=overlapped)
    case.sync()
    rho = case.field("rho").reshape(6, plane)
    assert np.isfinite(rho).all() and np.array_equal(rho[0], rho[1]) and np.array_equal(rho[5], rho[4])
    assert case.info()["minRho"] > 0
    case.close(); dev.close(); comm.close()


def test_two_slots_towards_one_other_rank_are_refused():
    """RCCL matches the messages of a peer in issue order: two halo slots with the same (other) peer rank would land in each
    other's ghost lists, so the exchange refuses them; so does a peer outside the communicator"""
    comm = NativeComm(0)
    mesh = q.PolyMesh.box(9, 8, 12, k_range=(3, 9))
    dev = q.Device(mesh)
    case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3))
    U, T, p = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    case.set_fields(U, T, p)
    for peers in ([1, 1], [0, 5]):
        with pytest.raises(q.QgdError) as ei:
            comm.exchange(case, peers)
        assert ei.value.code == q._lib.ERR_INVALID
    comm.exchange(case, [0, 0])     # the communicator is still usable: no group was left open
    case.sync()
    case.close(); dev.close(); comm.close()


# ---- every other message kind: the library's transport against a loopback world ------------------------------------------
SLAB = dict(nx=9, ny=8, n=12, k_range=(3, 9))     # the middle slab of a three-slab cut: 432 cells, two halo slots
SELF = [0, 0]                                     # both slots talk to rank 0 = this rank


class Loopback(LocalWorld):
    """One case whose halo slots all face the case itself: slot s receives what slot s packed, which is how RCCL matches a rank's
    sends to itself (issue order).  Stock LocalWorld would look the peer's slot up by rank and route slot 1 into slot 0."""

    def exchange(self, kind):
        case = self.cases[0]
        for (_, slot), buf in self.buf.items():
            case.halo_pack(slot, kind, buf)
        case.sync()
        for (_, slot), buf in self.buf.items():
            case.halo_unpack(slot, kind, buf)
        case.sync()


def slab_mesh():
    return q.PolyMesh.box(SLAB["nx"], SLAB["ny"], SLAB["n"], k_range=SLAB["k_range"])


def assert_identical(got, want, what):
    diff = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
    print(f"{what}: largest relative difference {diff:.3e}")
    assert np.array_equal(got, want), (what, diff)


def qgd_pair(dev, mesh, bc_fn=None, **opt):
    """(the case the library's transport drives, its twin for the loopback world): same device, options and fields"""
    U, T, p = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    pair = []
    for _ in range(2):
        c = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3, mu=1e-3, **opt))
        if bc_fn:
            bc_fn(c)
        c.set_fields(U, T, p)
        pair.append(c)
    return pair


def test_implicit_branch_messages_through_rccl():
    """message kinds 1..4 of the implicitDiffusion branch (and the state message behind them): qgd_case_step_sharded against
    ImplicitStepper over the loopback world"""
    comm, mesh = NativeComm(0), slab_mesh()
    dev = q.Device(mesh)
    case, twin = qgd_pair(dev, mesh, implicitDiffusion=1)
    comm.exchange(case, SELF)                    # the ghost planes start from the boundary layers, as ImplicitStepper starts
    for _ in range(2):
        comm.step(case, SELF)
    case.sync()
    ImplicitStepper(Loopback([ImplicitShard(twin)], [SELF], kinds=range(5))).step(2)
    twin.sync()
    for f in ("rho", "U", "p"):
        assert_identical(case.field(f), twin.field(f), f)
    got, want = case.implicit_info(), twin.implicit_info()
    print("iterations:", {k: (v["iterations"], want["solves"][k]["iterations"]) for k, v in got["solves"].items()})
    assert all(v["iterations"] > 0 for v in want["solves"].values()), want
    assert {k: v["iterations"] for k, v in got["solves"].items()} == {k: v["iterations"] for k, v in want["solves"].items()}
    assert case.info()["steps"] == twin.info()["steps"] == 2
    case.close(); twin.close(); dev.close(); comm.close()


def test_mid_assembly_message_through_rccl():
    """the message between step phases 5 and 6 (a GaussVolPoint shard that meets a qgdFlux wall): qgd_case_step_sharded against
    phases 5 | mid | 6 | 1 | state | 2 over the loopback world"""
    comm, mesh = NativeComm(0), slab_mesh()
    dev = q.Device(mesh)
    case, twin = qgd_pair(dev, mesh, bc_fn=mixed_bcs)
    assert case.needs_mid_exchange() and case.mid_halo_count(0)[0] > 0 and case.mid_halo_count(1)[1] > 0
    comm.exchange(case, SELF)
    for _ in range(3):
        comm.step(case, SELF)
    case.sync()
    world = Loopback([ImplicitShard(twin)], [SELF], kinds=(IMPL_STATE,))
    assert world.needs_mid()
    world.exchange(IMPL_STATE)
    for _ in range(3):
        world.phase(5)
        world.exchange(IMPL_MID)
        world.phase(6)
        world.phase(1)
        world.exchange(IMPL_STATE)
        world.phase(2)
    twin.sync()
    for f in ("rho", "U", "p"):
        assert_identical(case.field(f), twin.field(f), f)
    assert np.isfinite(case.field("rho")).all() and case.info()["steps"] == twin.info()["steps"] == 3
    case.close(); twin.close(); dev.close(); comm.close()


def qhd_pair(dev, mesh, fixed_p_patch=None):
    U, T, p = initial(mesh)
    rng = np.random.default_rng(3)
    U = U + 1e-2 * rng.standard_normal(U.shape)
    p = p + 1e-2 * rng.standard_normal(p.shape)
    pair = []
    for _ in range(2):
        c = qhdfoam.QHDFoamCase(dev, options("GaussVolPoint", deltaT=1e-3))
        cavity_bcs(c, mesh)
        if fixed_p_patch is not None:
            c.set_bc(fixed_p_patch, U=WALL["U"], T=WALL["T"], p=("fixedValue", 0.0))
        c.set_fields(U, T, p)
        pair.append(c)
    return pair


QHD_FIELDS = ("U", "T", "p", "U.boundary", "T.boundary", "p.boundary")


def test_qhd_messages_through_rccl_without_a_solve():
    """message kinds 0 (state) and 1 (pressure) of the QHD case: qgd_qhd_case_halo_exchange against pack -> buffer -> unpack"""
    comm, mesh = NativeComm(0), slab_mesh()
    plane = SLAB["nx"] * SLAB["ny"]
    dev = q.Device(mesh)
    case, twin = qhd_pair(dev, mesh)
    world = Loopback([twin], [SELF])
    for kind, moved in ((QHD_STATE, "U"), (QHD_PRESSURE, "p")):
        before = case.field(moved)
        comm.qhd_exchange(case, SELF, kind)
        case.sync()
        world.exchange(kind)
        ghosts = np.r_[0:plane, 5 * plane:6 * plane]
        assert not np.array_equal(case.field(moved)[ghosts], before[ghosts]), (kind, "the message did not reach the ghost planes")
        owned = np.r_[plane:5 * plane]
        assert np.array_equal(case.field(moved)[owned], before[owned]), (kind, "the message wrote owned cells")
        for f in QHD_FIELDS:
            assert_identical(case.field(f), twin.field(f), f"kind {kind}, {f}")
    case.close(); twin.close(); dev.close(); comm.close()


def test_qhd_step_through_rccl():
    """qgd_qhd_case_step_sharded (state, pressure, search-direction and multigrid messages over RCCL) against QhdStepper over the
    loopback world.  The self-fed ghost planes make each cut a zero-gradient wall; a fixedValue pressure patch on a side wall
    (yMax) keeps the pressure system non-singular."""
    comm, mesh = NativeComm(0), slab_mesh()
    dev = q.Device(mesh)
    case, twin = qhd_pair(dev, mesh, fixed_p_patch=3)
    QhdStepper(Loopback([twin], [SELF])).step(2)
    twin.sync()
    want = twin.info()
    print("reference arm:", want)
    assert want["steps"] == 2 and want["pIterations"] > 0 and want["pFinalResidual"] < 1e-12, want
    comm.qhd_exchange(case, SELF, QHD_STATE)     # QhdStepper.start
    comm.qhd_step(case, SELF, 2)
    got = case.info()
    print("library's transport:", got)
    for f in QHD_FIELDS + ("phi",):
        assert_identical(case.field(f), twin.field(f), f)
    assert got["pIterations"] == want["pIterations"] and got["steps"] == 2
    case.close(); twin.close(); dev.close(); comm.close()
