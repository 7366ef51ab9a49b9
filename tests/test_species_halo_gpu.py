"""GPU: species on cell-range shards and on cyclic patches (qgd_case_set_species with QGD_SPECIES_HALO): the state message carries the
composition, the species' cell and patch kernels follow the cell roles of the flow's.

The reference is never the code under test: it is the UNSHARDED, NON-PERIODIC device case with species on the `kernels` arm, itself anchored
once per case against the host replay of tests/species_ref.py (rel_err <= 1e-12, min Y > 0 so that the clip hides nothing).
Bars: shards against the unsharded case and the periodic box against the long box 1e-12 relative (test_partition_gpu.py,
test_cyclic_patches.py); conservation 1e-13 of the total mass (test_cyclic_patches.py); ghost cells bit-equal to their originals."""
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L
from qgdsolver_amd.halo import NativeComm

import cases
from oracle import OracleCase
from species_ref import SpeciesReplay
from test_cyclic_patches import periodic_box, smooth_fields, tiled_fields, wall_bcs
from test_partition import random_perm
from test_species_case import flow_fields, smooth_composition
from util import assert_path, make_mesh, oracle_mesh_of, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-12
STEPS = 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOW = ("rho", "U", "p", "e")


def inlet_bcs(mesh):
    """flow: one fixedValue inlet (patch 0), zero-gradient walls elsewhere, nothing on the patches of an empty direction (the patches of
    the UNCUT mesh: a shard keeps their labels)"""
    types = [int(t) for t in mesh.array("patchType")]

    def apply(case):
        case.set_bc(0, U=("fixedValue", (0.3, 0.0, 0.0)), T=("fixedValue", 1.0), p=("zeroGradient", None))
        for patch, t in enumerate(types):
            if t != 0:
                case.set_bc(patch, U=("none", None), T=("none", None), p=("none", None))
    return apply


def step_fields(C):
    U = np.zeros((C.shape[0], 3))
    U[:, 0] = 3.0
    return U, 1.0 + 0.05 * np.sin(2.0 * C[:, 0]) * np.cos(3.0 * C[:, 1]), 1.0 + 0.05 * np.cos(1.5 * C[:, 0] + C[:, 1])


def six_species(C):
    """six species, the inert one (index 2) included; five transported ones: two register batches"""
    Y = [0.12 * (1.0 + 0.4 * np.sin((1.0 + 0.5 * i) * np.pi * C[:, 0] + 0.7 * i) * np.cos((0.5 + 0.3 * i) * np.pi * C[:, 1])) for i in range(5)]
    Y.insert(2, 1.0 - sum(Y))
    return Y


COMPOSITIONS = {
    4: (smooth_composition, [0.7, 1.0, 1.0, 1.3], [0.3, 0.25, 0.3, 0.15]),
    6: (six_species, [0.7, 1.0, 1.0, 1.3, 0.9, 1.1], [0.15, 0.1, 0.45, 0.1, 0.1, 0.1]),
}
INERT = 2


def put_species(case, Y0, Sc, inlet, cells=None, inlet_patch=0, **kw):
    names = [f"S{i}" for i in range(len(Y0))]
    case.set_species(names, INERT, ScNumbers=Sc, **kw)
    for i, n in enumerate(names):
        if inlet is not None:
            case.set_species_bc(i, inlet_patch, ("fixedValue", inlet[i]))
        case.set_species_field(n, Y0[i] if cells is None else Y0[i][cells])
    return names


# kind -> (flow boundary conditions (None: inlet_bcs), initial flow, options)
SETUPS = {
    "box654_poly": (None, lambda C: flow_fields(C), dict(deltaT=1e-3, mu=1e-3)),
    "box654_jitter": (None, lambda C: flow_fields(C), dict(deltaT=1e-3, mu=1e-3)),
    "step2d": (cases.forward_step_bcs, step_fields, dict(deltaT=5e-4, mu=1e-3)),
}


def mesh_of(kind):
    g = make_mesh(kind)
    if kind == "box654_poly":
        g.renumber(random_perm(g.nCells, 21))
    return g


@functools.lru_cache(maxsize=None)
def reference(kind, stencil, nS):
    """the unsharded device case with species after STEPS steps, anchored against the host replay: computed once per case, never changed"""
    g = mesh_of(kind)
    bc_fn, init_fn, opt = SETUPS[kind]
    bc_fn = bc_fn or inlet_bcs(g)
    Y_fn, Sc, inlet = COMPOSITIONS[nS]
    C = g.array("C").reshape(-1, 3)
    options = q.default_options(stencil=stencil, **opt)
    om = oracle_mesh_of(g)
    dev = q.Device(g, fused_tables=False)
    gc = q.QGDFoamCase(dev, options)
    oc = OracleCase(om, options)
    for case in (gc, oc):
        bc_fn(case)
    Y0 = Y_fn(C)
    put_species(gc, Y0, Sc, inlet)

    def fresh():
        o2 = OracleCase(om, options)
        bc_fn(o2)
        o2.set_fields(*init_fn(C))
        return o2
    rep = SpeciesReplay(g, om, oc, stencil, Y0, INERT, ScNumbers=Sc, bcs=[{0: ("fixedValue", inlet[i])} for i in range(nS)], fresh=fresh)
    U, T, p = init_fn(C)
    gc.set_fields(U, T, p)
    oc.set_fields(U, T, p)
    assert_path(gc, "kernels", (kind, stencil))
    gc.step(STEPS)
    rep.step(STEPS)
    out = {f: gc.field(f) for f in FLOW}
    out["Y"] = [gc.species_field(i) for i in range(nS)]
    out["Yb"] = [gc.species_field(i, "Y.boundary") for i in range(nS)]
    for i in range(nS):
        e = rel_err(out["Y"][i], rep.Y[i])
        print("anchor", kind, stencil, nS, i, f"{e:.3e}")
        assert e <= TOL, (kind, stencil, i, e)
    assert min(float(y.min()) for y in rep.Y) > 0.0 and min(float(y.min()) for y in out["Y"]) > 0.0
    gc.close(); dev.close()
    for v in out.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    return out


class Shards:
    """W shards of g on one GPU in this process, driven phase by phase as tests/test_partition_gpu.py::run_sharded_device drives them, each
    with the species of COMPOSITIONS[nS] and QGD_SPECIES_HALO"""

    def __init__(self, g, world, stencil, bc_fn, init_fn, opt, nS):
        self.g, self.world = g, world
        Y_fn, Sc, inlet = COMPOSITIONS[nS]
        C = g.array("C").reshape(-1, 3)
        U, T, p = init_fn(C)
        Y0 = Y_fn(C)
        self.nS = nS
        self.shards = [g.shard(world, r) for r in range(world)]
        self.devs, self.cs, self.plain_counts = [], [], []
        for s in self.shards:
            d = q.Device(s, fused_tables=False)
            cg = s.array("cellGlobal")
            plain = q.QGDFoamCase(d, q.default_options(stencil=stencil, **opt))      # the same shard without species: today's message
            self.plain_counts.append([plain.halo_count(k) for k in range(s.halo_slots)])
            plain.close()
            c = q.QGDFoamCase(d, q.default_options(stencil=stencil, **opt))
            bc_fn(c)
            put_species(c, Y0, Sc, inlet, cells=cg, halo=True)
            c.set_fields(U[cg], T[cg], p[cg])
            assert_path(c, "kernels")
            self.devs.append(d); self.cs.append(c)
        self.peers = [[int(x) for x in s.array("haloPeer")] for s in self.shards]
        self.bufs = {}
        for r, (c, d) in enumerate(zip(self.cs, self.devs)):
            for k, peer in enumerate(self.peers[r]):
                self.bufs[(r, peer)] = d.alloc(8 * max(1, c.halo_count(k)))
        self.mid = {}
        if self.cs[0].needs_mid_exchange():
            for r, (c, d) in enumerate(zip(self.cs, self.devs)):
                for k, peer in enumerate(self.peers[r]):
                    self.mid[(r, peer)] = d.alloc(8 * max(1, c.mid_halo_count(k)[0]))

    def check_counts(self):
        for r, (s, c) in enumerate(zip(self.shards, self.cs)):
            for k in range(s.halo_slots):
                n_send = s.array(f"haloSend{k}").size
                today = self.plain_counts[r][k]
                n_bf, rem = divmod(today - 8 * n_send, 12)
                assert rem == 0 and n_bf >= 0, (r, k, today, n_send)                  # today's number: 8 nSend + 12 nSendBF
                assert c.halo_count(k) == (8 + self.nS) * n_send + 12 * n_bf, (r, k)
                peer = self.peers[r][k]
                assert c.halo_recv_count(k) == self.cs[peer].halo_count(self.peers[peer].index(r))

    def exchange(self):
        for r, c in enumerate(self.cs):
            for k, peer in enumerate(self.peers[r]):
                c.halo_pack(k, self.bufs[(r, peer)])
            c.sync()
        for r, c in enumerate(self.cs):
            for k, peer in enumerate(self.peers[r]):
                c.halo_unpack(k, self.bufs[(peer, r)])
            c.step_phase(2)
            c.sync()

    def exchange_mid(self):
        for r, c in enumerate(self.cs):
            for k, peer in enumerate(self.peers[r]):
                c.mid_halo_pack(k, self.mid[(r, peer)])
            c.sync()
        for r, c in enumerate(self.cs):
            for k, peer in enumerate(self.peers[r]):
                c.mid_halo_unpack(k, self.mid[(peer, r)])
            c.sync()

    def run(self, steps, layer_first):
        self.exchange()
        for _ in range(steps):
            if self.mid:
                for c in self.cs:
                    c.step_phase(5)
                self.exchange_mid()
                for c in self.cs:
                    c.step_phase(6)
            else:
                for c in self.cs:
                    c.step_phase(0)
            if layer_first:
                for c in self.cs:
                    c.step_phase(10)
                self.exchange()
                for c in self.cs:
                    c.step_phase(11)
                    c.sync()
            else:
                for c in self.cs:
                    c.step_phase(1)
                self.exchange()

    def owned(self, r):
        cg = self.shards[r].array("cellGlobal")
        n = self.g.nCells
        return (cg >= (n * r) // self.world) & (cg < (n * (r + 1)) // self.world)

    def gathered(self):
        g = self.g
        out = {f: np.full((g.nCells, 3) if f == "U" else g.nCells, np.nan) for f in FLOW}
        out["Y"] = [np.full(g.nCells, np.nan) for _ in range(self.nS)]
        out["Yb"] = [np.full(g.nBoundaryFaces, np.nan) for _ in range(self.nS)]
        for r, (s, c) in enumerate(zip(self.shards, self.cs)):
            cg, own = s.array("cellGlobal"), self.owned(r)
            for f in FLOW:
                out[f][cg[own]] = c.field(f)[own]
            # the shard's real patch faces whose owner cell it owns, by their labels in the uncut mesh
            fg = s.array("faceGlobal")[s.nInternalFaces:]
            o = s.array("owner")[s.nInternalFaces:]
            pick = (fg >= g.nInternalFaces) & own[o]
            for i in range(self.nS):
                out["Y"][i][cg[own]] = c.species_field(i)[own]
                out["Yb"][i][fg[pick] - g.nInternalFaces] = c.species_field(i, "Y.boundary")[pick]
        return out

    def close(self):
        for c, d in zip(self.cs, self.devs):
            c.close(); d.close()


@pytest.mark.parametrize("kind,stencil,world,layer_first,nS", [
    ("box654_poly", "GaussVolPoint", 3, False, 4),
    ("box654_poly", "GaussVolPoint", 3, True, 4),
    ("box654_jitter", "reduced", 2, False, 4),
    ("step2d", "leastSquares", 4, True, 4),
    ("step2d", "GaussVolPoint", 3, False, 4),          # qgdFlux walls: the mid-assembly message, phases 5 and 6
    ("box654_poly", "GaussVolPoint", 3, True, 6),      # five transported species: two register batches, the tail's stride past one batch
])
def test_shards_match_the_unsharded_case(kind, stencil, world, layer_first, nS):
    ref = reference(kind, stencil, nS)
    g = mesh_of(kind)
    bc_fn, init_fn, opt = SETUPS[kind]
    sh = Shards(g, world, stencil, bc_fn or inlet_bcs(g), init_fn, opt, nS)
    assert bool(sh.mid) == (kind == "step2d" and stencil == "GaussVolPoint")
    sh.check_counts()
    sh.run(STEPS, layer_first)
    got = sh.gathered()
    tag = (kind, stencil, world, layer_first, nS)
    for f in FLOW:
        e = np.abs(got[f] - ref[f]).max() / np.abs(ref[f]).max()
        print(tag, f, f"{e:.3e}")
        assert e <= TOL, (tag, f, e)
    for i in range(nS):
        e, eb = rel_err(got["Y"][i], ref["Y"][i]), rel_err(got["Yb"][i], ref["Yb"][i])
        print(tag, "Y", i, f"{e:.3e}", "Y.boundary", f"{eb:.3e}")
        assert e <= TOL and eb <= TOL, (tag, i, e, eb)       # (NaN where no shard owned a cell or face: fails)
    # after the last exchange every ghost cell holds, bit for bit, its original's composition
    for r, (s, c) in enumerate(zip(sh.shards, sh.cs)):
        cg, own = s.array("cellGlobal"), sh.owned(r)
        assert (~own).any()
        for i in range(nS):
            assert np.array_equal(c.species_field(i)[~own], got["Y"][i][cg[~own]]), (tag, r, i)
    sh.close()


# ---- the library's own transport ---------------------------------------------------------------------------------------------------------
def slab_case(nS=4):
    nx, ny, n = 9, 8, 12
    mesh = q.PolyMesh.box(nx, ny, n, k_range=(3, 9))          # planes 3..8: ghost 3, owned 4..7, ghost 8
    dev = q.Device(mesh, fused_tables=False)
    case = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3, mu=1e-3))
    C = mesh.array("C").reshape(-1, 3)
    Y_fn, Sc, inlet = COMPOSITIONS[nS]
    put_species(case, Y_fn(C), Sc, inlet, halo=True)
    case.set_fields(*cases.box_initial_fields(C))
    return mesh, dev, case, nx * ny


@functools.lru_cache(maxsize=None)
def slab_by_phases(layer_first):
    """the slab whose two slots face the slab itself, driven by phases from Python: slot s unpacks what slot s packed (how RCCL matches a
    rank's sends to itself)"""
    mesh, dev, case, plane = slab_case()
    bufs = [dev.alloc(8 * case.halo_count(k)) for k in range(2)]

    def exchange():
        for k in range(2):
            case.halo_pack(k, bufs[k])
        case.sync()
        for k in range(2):
            case.halo_unpack(k, bufs[k])
        case.step_phase(2)
        case.sync()
    exchange()
    for _ in range(3):
        case.step_phase(0)
        if layer_first:
            case.step_phase(10); exchange(); case.step_phase(11); case.sync()
        else:
            case.step_phase(1); exchange()
    out = {f: case.field(f) for f in FLOW}
    out["Y"] = [case.species_field(i) for i in range(4)]
    out["Yb"] = [case.species_field(i, "Y.boundary") for i in range(4)]
    case.close(); dev.close()
    return out


@pytest.mark.parametrize("overlapped", [False, True])
def test_self_exchange_moves_the_composition_through_rccl(overlapped):
    want = slab_by_phases(overlapped)
    comm = NativeComm(0)
    mesh, dev, case, plane = slab_case()
    assert case.halo_count(0) == case.halo_recv_count(0) == case.halo_count(1) == case.halo_recv_count(1) >= (8 + 4) * plane
    comm.exchange(case, [0, 0])
    case.sync()
    for i in range(4):
        y = case.species_field(i).reshape(6, plane)
        assert np.array_equal(y[0], y[1]) and np.array_equal(y[5], y[4]), i
    for _ in range(3):
        comm.step(case, [0, 0], overlapped=overlapped)
    case.sync()
    for f in FLOW:
        assert np.array_equal(case.field(f), want[f]), (overlapped, f)
    for i in range(4):
        assert np.array_equal(case.species_field(i), want["Y"][i]), (overlapped, i)
        assert np.array_equal(case.species_field(i, "Y.boundary"), want["Yb"][i]), (overlapped, i)
        y = case.species_field(i).reshape(6, plane)
        assert np.array_equal(y[0], y[1]) and np.array_equal(y[5], y[4])
    assert min(float(case.species_field(i).min()) for i in range(4)) > 0
    case.close(); dev.close(); comm.close()


# ---- cyclic patches ----------------------------------------------------------------------------------------------------------------------
def periodic_composition(C):
    """four species as functions of x mod 1 (smooth across the seam), the inert one (index 2) included; every value in [0.1, 0.6]"""
    x, y, z = np.mod(C[:, 0], 1.0), C[:, 1], C[:, 2]
    y0 = 0.2 + 0.1 * np.sin(2 * np.pi * x) * np.cos(np.pi * y)
    y1 = 0.2 + 0.05 * np.cos(2 * np.pi * x + 0.4) * np.cos(np.pi * z)
    y3 = 0.2 + 0.1 * np.cos(4 * np.pi * x + 2.0 * y)
    Y = [y0, y1, 1.0 - y0 - y1 - y3, y3]
    assert all(v.min() >= 0.1 and v.max() <= 0.6 for v in Y)
    return Y


PER_SC = [0.7, 1.0, 1.0, 1.3]
WALL_VALUE = [0.25, 0.2, 0.35, 0.2]       # fixedValue on the yMin wall (patch 2): a patch the copies behind the halves have faces on


@pytest.mark.parametrize("stencil,bc_fn", [("GaussVolPoint", None), ("GaussVolPoint", wall_bcs), ("reduced", None)])
def test_periodic_box_is_the_middle_of_a_three_times_longer_box(stencil, bc_fn):
    nx, ny, nz, steps = 8, 5, 4, 3
    options = q.default_options(stencil=stencil, deltaT=2e-3, mu=1e-3)
    # the reference: the same case on [-1, 2) x [0, 1)^2 with ordinary patches at its far ends, on the device, anchored against the replay
    long = q.PolyMesh.box(3 * nx, ny, nz, lo=(-1.0, 0.0, 0.0), hi=(2.0, 1.0, 1.0))
    Cl = long.array("C").reshape(-1, 3)
    om = oracle_mesh_of(long)
    ldev = q.Device(long, fused_tables=False)
    lc = q.QGDFoamCase(ldev, options)
    oc = OracleCase(om, options)
    for case in (lc, oc):
        if bc_fn:
            bc_fn(case)
    Yl = periodic_composition(Cl)
    put_species(lc, Yl, PER_SC, WALL_VALUE, inlet_patch=2)

    def fresh():
        o2 = OracleCase(om, options)
        if bc_fn:
            bc_fn(o2)
        o2.set_fields(*tiled_fields(smooth_fields, Cl, 1.0))
        return o2
    rep = SpeciesReplay(long, om, oc, stencil, Yl, INERT, ScNumbers=PER_SC, bcs=[{2: ("fixedValue", WALL_VALUE[i])} for i in range(4)], fresh=fresh)
    for case in (lc, oc):
        case.set_fields(*tiled_fields(smooth_fields, Cl, 1.0))
    lc.step(steps)
    rep.step(steps)
    ref = [lc.species_field(i) for i in range(4)]
    for i in range(4):
        assert rel_err(ref[i], rep.Y[i]) <= TOL, (stencil, i)
    assert min(float(y.min()) for y in rep.Y) > 0.0
    lc.close(); ldev.close()
    # the periodic case: plain qgd_case_step, the library refreshes the copies -- records and composition -- itself
    g = periodic_box((nx, ny, nz), (True, False, False))
    ext = g.unroll_cyclic()
    cg = ext.array("cellGlobal")
    dev = q.Device(ext, fused_tables=False)
    gc = q.QGDFoamCase(dev, options)
    if bc_fn:
        bc_fn(gc)
    Cg = g.array("C").reshape(-1, 3)
    Y0 = [y[cg].copy() for y in periodic_composition(Cg)]
    for y in Y0:
        y[g.nCells:] = np.nan                                 # (the copies belong to the library, whatever the caller put there)
    put_species(gc, Y0, PER_SC, WALL_VALUE, inlet_patch=2, halo=True)
    U, T, p = smooth_fields(Cg)
    gc.set_fields(U[cg], T[cg], p[cg])
    gc.step(steps)
    idx = np.arange(long.nCells).reshape(nz, ny, 3 * nx)[:, :, nx: 2 * nx].reshape(-1)
    for i in range(4):
        a, b = gc.species_field(i)[:g.nCells], ref[i][idx]
        e = np.abs(a - b).max() / np.abs(b).max()
        print(stencil, bool(bc_fn), "Y", i, f"{e:.3e}")
        assert e <= TOL, (stencil, i, e)
        assert np.array_equal(gc.species_field(i)[g.nCells:], gc.species_field(i)[cg[g.nCells:]])     # the copies ARE their originals
    gc.close(); dev.close()


def all_moving_composition(C):
    """four species, none uniform (a uniform species stays uniform: nothing to conserve against), triply periodic, in [0.1, 0.5]"""
    x, y, z = C[:, 0], C[:, 1], C[:, 2]
    y0 = 0.2 + 0.08 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y)
    y1 = 0.2 + 0.06 * np.cos(2 * np.pi * y) * np.sin(2 * np.pi * z)
    y3 = 0.2 + 0.08 * np.cos(2 * np.pi * (x + z))
    return [y0, y1, 1.0 - y0 - y1 - y3, y3]


@pytest.mark.parametrize("adjust", [0, 1])
def test_triply_periodic_box_conserves_every_species(adjust):
    """sum rho Y_i V over the real cells, the inert species included, to 1e-13 of the total mass over 12 steps.  The amplitudes keep every
    Y in [0.1, 0.5] at the start, and min Y > 0 is asserted on the device after EVERY step (where the clip Yi.max(0) acted, it would add
    mass): there is no host replay of a periodic species case to choose them with, so the property itself is watched throughout."""
    g = periodic_box((6, 5, 4), (True, True, True))
    ext = g.unroll_cyclic()
    assert ext.halo_slots == 26
    n, cg = g.nCells, ext.array("cellGlobal")
    opt = dict(stencil="GaussVolPoint", deltaT=2e-3, mu=1e-3)
    if adjust:
        opt.update(adjustTimeStep=1, maxCo=0.3)
    dev = q.Device(ext, fused_tables=False)
    gc = q.QGDFoamCase(dev, q.default_options(**opt))
    C = g.array("C").reshape(-1, 3)
    Y0 = all_moving_composition(C)
    put_species(gc, [y[cg] for y in Y0], PER_SC, None, halo=True)
    U, T, p = smooth_fields(C)
    U[:, 2] += 0.04 * np.sin(2 * np.pi * C[:, 1])
    T = T + 0.03 * np.sin(2 * np.pi * C[:, 2])
    gc.set_fields(U[cg], T[cg], p[cg])
    V = g.array("V")

    def masses():
        rho = gc.field("rho")[:n]
        return np.array([(rho * gc.species_field(i)[:n] * V).sum() for i in range(4)]), float((rho * V).sum())
    before, total = masses()
    for _ in range(12):
        gc.step(1)
        assert min(float(gc.species_field(i)[:n].min()) for i in range(4)) > 0.0
    after, total_after = masses()
    defect = (after - before) / total
    print("adjust", adjust, "species mass defect / total mass:", defect, "mass:", (total_after - total) / total)
    assert (np.abs(defect) <= 1e-13).all(), defect
    assert abs(after.sum() - total_after) <= 1e-13 * total            # the composition still sums to one, cell by cell
    for i in range(4):
        assert np.abs(gc.species_field(i)[:n] - Y0[i]).max() >= 100 * 1e-13, i     # (every species moved, by far more than the bar)
        assert np.abs(gc.species_field(i)[:n] - Y0[i]).max() > 1e-4, i
    gc.close(); dev.close()


# ---- the flag itself ---------------------------------------------------------------------------------------------------------------------
def refusal(fn, code, *words):
    with pytest.raises(q.QgdError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    for w in words:
        assert w in str(ei.value), (w, str(ei.value))


def test_the_flag_changes_nothing_on_an_ordinary_device():
    g = mesh_of("box654_poly")
    bc_fn, init_fn, opt = SETUPS["box654_poly"]
    C = g.array("C").reshape(-1, 3)
    Y_fn, Sc, inlet = COMPOSITIONS[4]
    out = []
    for halo in (False, True):
        dev = q.Device(g, fused_tables=False)
        gc = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", **opt))
        inlet_bcs(g)(gc)
        put_species(gc, Y_fn(C), Sc, inlet, halo=halo)
        gc.set_fields(*init_fn(C))
        gc.step(3)
        out.append([gc.field(f) for f in FLOW + ("rhoE",)] + [gc.species_field(i, w) for i in range(4) for w in ("Y", "Y.boundary")])
        if halo:   # phases belong to shards: an unsharded case with species keeps today's refusal, flag or not
            refusal(lambda: gc.step_phase(10), L.ERR_NOT_IMPLEMENTED, "species")
            refusal(lambda: gc.step_phase(0), L.ERR_NOT_IMPLEMENTED, "species")
        gc.close(); dev.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_refusals_with_the_flag():
    assert L.SPECIES_HALO == 4
    sh = q.PolyMesh.box(8, 6, 4).shard(2, 0)
    sdev = q.Device(sh, fused_tables=False)
    G = L.PATCH_GENERIC
    ext = q.PolyMesh.box(6, 5, 4, patch_types=[L.PATCH_CYCLIC, L.PATCH_CYCLIC, G, G, G, G]).unroll_cyclic()
    pdev = q.Device(ext, fused_tables=False)
    for dev, word in ((sdev, "sharded"), (pdev, "periodic")):
        c = q.QGDFoamCase(dev, q.default_options(implicitDiffusion=1))
        refusal(lambda: c.set_species(["A", "B"], 1, implicit=True, halo=True), L.ERR_NOT_IMPLEMENTED, "implicitDiffusion", "not distributed")
        c.close()
        c = q.QGDFoamCase(dev, q.default_options())
        refusal(lambda: c.set_species(["A", "B"], 1), L.ERR_NOT_IMPLEMENTED, word)                    # without the flag: as before
        assert L.lib.qgd_case_set_species(c._h, 2, 1, None, 4 | 8) == L.ERR_INVALID and b"unknown flags" in L.lib.qgd_last_error()
        assert L.lib.qgd_case_set_species(c._h, 2, 1, None, 4 | 16) == L.ERR_INVALID and b"unknown flags" in L.lib.qgd_last_error()
        c.set_species(["A", "B"], 1, halo=True)                                                       # the explicit branch: accepted
        c.close()
    c = q.QGDFoamCase(sdev, q.default_options(stencil="GaussVolPoint", termStencils={"grad(p)": "reduced"}))
    refusal(lambda: c.set_species(["A", "B"], 1, halo=True), L.ERR_NOT_IMPLEMENTED, "per-term stencils")
    c.close()
    # a periodic device is stepped with qgd_case_step; on a shard a phase that begins a step asks for every species' field
    c = q.QGDFoamCase(sdev, q.default_options())
    c.set_species(["A", "B"], 1, halo=True)
    c.set_species_field("A", np.full(sh.nCells, 0.3))
    c.set_fields(*cases.box_initial_fields(sh.array("C").reshape(-1, 3)))
    refusal(lambda: c.step_phase(0), L.ERR_INVALID, "never set")
    refusal(lambda: c.step_phase(3), L.ERR_NOT_IMPLEMENTED, "species")
    c.close()
    cg = ext.array("cellGlobal")
    c = q.QGDFoamCase(pdev, q.default_options())
    c.set_species(["A", "B"], 1, halo=True)
    for n, v in (("A", 0.3), ("B", 0.7)):
        c.set_species_field(n, np.full(ext.nCells, v))
    c.set_fields(*cases.box_initial_fields(ext.array("C").reshape(-1, 3)[cg]))
    refusal(lambda: c.step_phase(0), L.ERR_NOT_IMPLEMENTED, "species")
    c.step(1)
    assert np.abs(c.species_field("A") - 0.3).max() <= 1e-13
    c.close()
    sdev.close(); pdev.close()


# ---- the application ---------------------------------------------------------------------------------------------------------------------
def run_app(args, timeout=300):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), MASTER_ADDR="127.0.0.1")
    return subprocess.run([sys.executable] + args, capture_output=True, text=True, cwd=ROOT, env=env, timeout=timeout)


def launch(world, case_dir, port):
    return ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1", "--master-port", str(port),
            "-m", "qgdsolver_amd.QGDFoam", "-case", case_dir, "-backend", "gloo"]


def test_application_on_two_ranks_writes_the_one_rank_species(tmp_path):
    from qgdsolver_amd import foamfile as ff
    from test_species_reader import write_species_case

    one, many = str(tmp_path / "one"), str(tmp_path / "many")
    write_species_case(one, end_time=6e-3, write_interval=6e-3)
    shutil.copytree(one, many)
    r = run_app(["-m", "qgdsolver_amd.QGDFoam", "-case", one])
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    r = run_app(launch(2, many, 29561), timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "on 2 rank(s)" in r.stdout and "species N2 O2 H2O (inert N2)" in r.stdout
    mesh = ff.read_polymesh(os.path.join(one, "constant", "polyMesh"))
    Y0 = ff.read_case_setup(one, "0")[1]["species"]["fields"]
    for n in ("N2", "O2", "H2O", "rho", "U", "T", "p"):
        a, _ = ff.read_field(os.path.join(one, "0.006", n), mesh)
        b, _ = ff.read_field(os.path.join(many, "0.006", n), mesh)
        e = np.abs(a - b).max() / np.abs(a).max()
        print("2 ranks vs 1", n, f"{e:.3e}")
        assert e <= TOL, (n, e)
        if n in Y0:
            assert np.abs(a[:, 0] - Y0[n]).max() > 1e-6
    # the species' implicit branch is not distributed: refused by name before any device exists
    from test_species_implicit_reader import write_default_branch_case
    impl = str(tmp_path / "implicit")
    write_default_branch_case(impl)
    r = run_app(launch(2, impl, 29562), timeout=600)
    assert r.returncode != 0
    assert "FoamFileError" in r.stderr and "species with implicitDiffusion true run on one rank" in r.stderr and "cyclic patches" in r.stderr, r.stderr[-3000:]


def test_application_runs_a_periodic_species_case(tmp_path):
    """a written x-periodic channel with three species on one rank: the written Y_i are those of the library on the unrolled mesh in this
    process (same calls, bit for bit), only the real cells are written, and the composition moved and still sums to one"""
    from qgdsolver_amd import QGDFoam, foamfile as ff
    from test_cyclic_patches import write_periodic_case

    case_dir = str(tmp_path)
    mesh, (U, T, p) = write_periodic_case(case_dir)
    cd = os.path.join(case_dir, "system", "controlDict")
    text = open(cd).read()
    assert "endTime 1;" in text
    open(cd, "w").write(text.replace("endTime 1;", "endTime 0.005;") + "writeControl timeStep;\nwriteInterval 10;\n")
    names, Sc = ["N2", "O2", "H2O"], [1.0, 0.8, 1.25]
    tp = os.path.join(case_dir, "constant", "thermophysicalProperties")
    bcs = [("none", None), ("none", None), ("fixedValue", 0.3), ("zeroGradient", None), ("zeroGradient", None), ("zeroGradient", None)]
    species = dict(names=names, inert="N2", ScNumbers=Sc, bcs={n: bcs for n in names})
    open(tp, "a").write(ff.species_entries_text(species))
    C = mesh.array("C").reshape(-1, 3)
    o2 = 0.2 + 0.1 * np.sin(2 * np.pi * C[:, 0]) * np.cos(np.pi * C[:, 1])
    h2o = 0.2 + 0.1 * np.cos(4 * np.pi * C[:, 0] + 2.0 * C[:, 1])
    Y0 = {"N2": 1.0 - o2 - h2o, "O2": o2, "H2O": h2o}
    ff.write_species_fields(case_dir, "0", mesh, species, Y0)
    dev, case, written = QGDFoam.run(case_dir, n_steps=10, log=lambda *a, **k: None)
    assert written == ["0.005"]
    ext = case.mesh
    assert ext.nCells > mesh.nCells
    got = {n: ff.read_field(os.path.join(case_dir, "0.005", n), mesh)[0][:, 0] for n in names}
    for n in names:
        assert got[n].shape == (mesh.nCells,) and np.array_equal(got[n], case.species_field(n)[:mesh.nCells]), n
        assert np.abs(got[n] - Y0[n]).max() > 1e-6 and got[n].min() > 0
        assert ff.read_field(os.path.join(case_dir, "0.005", n), mesh)[1]["left"]["type"] == "cyclic"
    assert np.abs(sum(got.values()) - 1.0).max() <= 1e-14
    case.close(); dev.close()
    # the same case through foamfile.load_case: the loader asks for the flag too
    dev, case = ff.load_case(case_dir, "0")
    case.step(10)
    for n in names:
        assert np.array_equal(case.species_field(n)[:mesh.nCells], got[n]), n
    case.close(); dev.close()
