"""GPU: per-face values of fixedValue entries on U, T and p of a resident QGDFoam case (qgd_case_set_bc_values).

The independent check is the split patch: a patch of N faces with a value list is, by construction, the same case as N consecutive
one-face patches with one value each -- face labels do not move, so the arithmetic is the same -- and that second form is what the
device and the oracle both served before.  Case L carries the lists, case S the split patches; L and S agree bit for bit, S agrees with
the oracle to the project's bars (1e-12 explicit, 1e-10 implicit).

(A device serves at most 64 patches, and the box's inlet, outlet and wall have 20 + 20 + 24 faces: the wall's temperature is linear over
its first 20 faces and constant over the last 4, which S declares as one patch -- a run of equal values is one uniform patch.)"""
import os

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L
from qgdsolver_amd import foamfile as ff
from qgdsolver_amd.halo import ImplicitShard, ImplicitStepper, LocalWorld

import cases
from oracle import OracleCase
from util import assert_path, oracle_mesh_of

pytestmark = pytest.mark.gpu

G, E = L.PATCH_GENERIC, L.PATCH_EMPTY
STEPS = 5
FIELDS = ("rho", "U", "p", "e")
EXPL = dict(deltaT=1e-3, mu=1e-3)
IMPL = dict(deltaT=5e-4, mu=2e-2, implicitDiffusion=1, implicitTol=1e-14, implicitMaxIter=2000)
ADJ = dict(deltaT=1e-3, mu=1e-3, adjustTimeStep=1, maxCo=0.3, maxDeltaT=1.0, cTau=0.75)
# (tag, options, fused_tables of the Device, the path asserted)
CONFIGS = [("gvp-fused", dict(stencil="GaussVolPoint", **EXPL), "any", "fused"),
           ("gvp-kernels", dict(stencil="GaussVolPoint", **EXPL), False, "kernels"),
           ("reduced", dict(stencil="reduced", **EXPL), False, "kernels"),
           ("gvp-implicit", dict(stencil="GaussVolPoint", **IMPL), False, "kernels"),
           ("gvp-adjust-blocks", dict(stencil="GaussVolPoint", **ADJ), "any", "fusedAdjust"),
           ("gvp-adjust-kernels", dict(stencil="GaussVolPoint", **ADJ), False, "kernels")]
PLANE_CONFIGS = [("lsq", dict(stencil="leastSquares", **EXPL), False, "kernels"),
                 ("lsq-implicit", dict(stencil="leastSquares", **IMPL), False, "kernels")]


def box():
    return q.PolyMesh.box(6, 5, 4).jitter(0.2, seed=2024)


def plane():
    return q.PolyMesh.box(8, 6, 1, hi=(1.0, 0.75, 0.1), patch_types=[G, G, G, G, E, E])


def lists_of(mesh):
    """inlet (patch 0) velocities: a parabola over the faces; wall (patch 2) temperatures: linear, the faces beyond the 20th share one
    value; outlet (patch 1) pressures: varying"""
    pz = mesh.array("patchSize")
    n0, n1, n2 = int(pz[0]), int(pz[1]), int(pz[2])
    s = (np.arange(n0) + 0.5) / n0
    U = np.zeros((n0, 3))
    U[:, 0] = 0.1 * (0.4 + 2.4 * s * (1.0 - s))
    U[:, 1] = 0.002 * np.cos(3.0 * s)
    T = 1.0 + 0.004 * np.minimum(np.arange(n2), 20)
    p = 1.0 + 0.01 * np.sin(1.0 + 0.7 * np.arange(n1))
    return U, T, p


UNIFORM = dict(U=np.array([0.08, 0.002, 0.0]), T=1.03, p=0.99)


def set_bcs(case, mesh, U=None, T=None, p=None):
    """x-min inlet (U, T fixedValue), x-max outlet (p fixedValue), walls elsewhere (no-slip, qgdFlux; the y-min wall with a fixed
    temperature); U / T / p: the value or the value list of the three entries under test"""
    U = UNIFORM["U"] if U is None else U
    T = UNIFORM["T"] if T is None else T
    p = UNIFORM["p"] if p is None else p
    pt = mesh.array("patchType")
    case.set_bc(0, U=("fixedValue", U), T=("fixedValue", 1.02), p=("zeroGradient", None))
    case.set_bc(1, U=("zeroGradient", None), T=("zeroGradient", None), p=("fixedValue", p))
    case.set_bc(2, U=("fixedValue", (0.0, 0.0, 0.0)), T=("fixedValue", T), p=("qgdFlux", None))
    for i in range(3, mesh.nPatches):
        if int(pt[i]) == E:
            case.set_bc(i, U=("none", None), T=("none", None), p=("none", None))
        elif int(pt[i]) == G:
            case.set_bc(i, U=("fixedValue", (0.0, 0.0, 0.0)), T=("zeroGradient", None), p=("qgdFlux", None))


def fields_of(mesh):
    f = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    if mesh.nGeometricD == 2:
        f[0][:, 2] = 0.0
    return f


def run_device(mesh, opt, tables, arm, setup, steps=STEPS, tag=None, fields=None):
    dev = q.Device(mesh, fused_tables=tables)
    c = q.QGDFoamCase(dev, q.default_options(**opt))
    setup(c)
    assert_path(c, arm, tag)
    assert not c.fused_info()["fusedImplicit"]
    c.set_fields(*(fields if fields is not None else fields_of(mesh)))
    c.step(steps)
    out = {f: c.field(f).copy() for f in FIELDS}
    out.update({f + ".boundary": c.field(f + ".boundary").copy() for f in ("U", "T", "p", "rho")})
    info = c.info()
    assert np.all(np.isfinite(out["rho"])) and info["minRho"] > 0, (tag, info)
    c.close(); dev.close()
    return out


def split_mesh(mesh, runs):
    """the same mesh with patches 0, 1, 2 re-declared as consecutive patches of runs[i][k] faces; returns (mesh, first new patch of every
    old one)"""
    ps, pz, pt = mesh.array("patchStart"), mesh.array("patchSize"), mesh.array("patchType")
    nps, npz, npt, first = [], [], [], []
    for i in range(mesh.nPatches):
        first.append(len(nps))
        sizes = runs[i] if i < 3 else [int(pz[i])]
        assert sum(sizes) == int(pz[i])
        at = int(ps[i])
        for n in sizes:
            nps.append(at); npz.append(n); npt.append(int(pt[i]))
            at += n
    assert len(nps) <= 64
    m = q.PolyMesh.from_arrays(mesh.array("points"), mesh.array("faceOffsets"), mesh.array("facePoints"), mesh.array("owner"),
                               mesh.array("neighbour"), mesh.nCells, nps, npz, npt)
    for name in ("C", "V", "Sf"):
        assert np.array_equal(m.array(name), mesh.array(name)), name
    return m, first


def runs_of(values):
    """lengths of the runs of equal consecutive entries"""
    v = np.asarray(values).reshape(len(values), -1)
    cut = np.nonzero(np.any(v[1:] != v[:-1], axis=1))[0] + 1
    return [int(x) for x in np.diff(np.concatenate([[0], cut, [len(v)]]))]


def set_split_bcs(case, smesh, first, runs, U, T, p):
    pt = smesh.array("patchType")
    at = 0
    for k, n in enumerate(runs[0]):
        case.set_bc(first[0] + k, U=("fixedValue", U[at]), T=("fixedValue", 1.02), p=("zeroGradient", None)); at += n
    at = 0
    for k, n in enumerate(runs[1]):
        case.set_bc(first[1] + k, U=("zeroGradient", None), T=("zeroGradient", None), p=("fixedValue", float(p[at]))); at += n
    at = 0
    for k, n in enumerate(runs[2]):
        case.set_bc(first[2] + k, U=("fixedValue", (0.0, 0.0, 0.0)), T=("fixedValue", float(T[at])), p=("qgdFlux", None)); at += n
    for i in range(first[3], smesh.nPatches):
        if int(pt[i]) == E:
            case.set_bc(i, U=("none", None), T=("none", None), p=("none", None))
        else:
            case.set_bc(i, U=("fixedValue", (0.0, 0.0, 0.0)), T=("zeroGradient", None), p=("qgdFlux", None))


# ---- 4: a list of equal entries is the uniform patch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,opt,tables,arm", CONFIGS)
def test_equal_valued_lists_are_the_uniform_patch_bit_for_bit(tag, opt, tables, arm):
    mesh = box()
    pz = mesh.array("patchSize")
    uni = run_device(mesh, opt, tables, arm, lambda c: set_bcs(c, mesh), tag=tag)
    eq = dict(U=np.tile(UNIFORM["U"], (int(pz[0]), 1)), T=np.full(int(pz[2]), UNIFORM["T"]), p=np.full(int(pz[1]), UNIFORM["p"]))
    lst = run_device(mesh, opt, tables, arm, lambda c: set_bcs(c, mesh, **eq), tag=tag)
    for f in uni:
        assert np.array_equal(uni[f], lst[f]), (tag, f, np.abs(uni[f] - lst[f]).max())


# ---- 5: split-patch equivalence, and the split case against the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("make,tag,opt,tables,arm", [(box,) + c for c in CONFIGS] + [(plane,) + c for c in PLANE_CONFIGS])
def test_list_patch_is_its_one_face_patches(make, tag, opt, tables, arm):
    mesh = make()
    U, T, p = lists_of(mesh)
    runs = [runs_of(U), runs_of(p), runs_of(T)]
    assert runs[0] == [1] * len(U) and runs[1] == [1] * len(p) and runs[2][:min(len(T), 20)] == [1] * min(len(T), 20)
    smesh, first = split_mesh(mesh, runs)
    fields = fields_of(mesh)
    Lr = run_device(mesh, opt, tables, arm, lambda c: set_bcs(c, mesh, U=U, T=T, p=p), tag=tag, fields=fields)
    Sr = run_device(smesh, opt, tables, arm, lambda c: set_split_bcs(c, smesh, first, runs, U, T, p), tag=tag, fields=fields)
    oc = OracleCase(oracle_mesh_of(smesh), q.default_options(**opt))
    set_split_bcs(oc, smesh, first, runs, U, T, p)
    oc.set_fields(*fields)
    oc.step(STEPS)
    bar = 1e-10 if opt.get("implicitDiffusion") else 1e-12
    for f in FIELDS:
        ref = oc.field(f)
        err = np.abs(Sr[f] - ref).max() / np.abs(ref).max()
        print(f"{make.__name__} {tag} {f}: S vs oracle {err:.3e}, L vs S {np.abs(Lr[f] - Sr[f]).max():.3e}")
        assert err <= bar, (tag, f, err)
    for f in Lr:
        assert np.array_equal(Lr[f], Sr[f]), (tag, f, np.abs(Lr[f] - Sr[f]).max())
    # and the lists matter: the uniform case is another case
    uni = run_device(mesh, opt, tables, arm, lambda c: set_bcs(c, mesh), tag=tag, fields=fields)
    assert np.abs(uni["U"] - Lr["U"]).max() > 1e-6


# ---- 6: the lists are read, returned and dropped ---------------------------------------------------------------------------------------
def test_lists_are_read_returned_and_dropped():
    mesh = box()
    U, T, p = lists_of(mesh)
    opt = dict(stencil="GaussVolPoint", **EXPL)
    fields = fields_of(mesh)
    dev = q.Device(mesh, fused_tables="any")
    c = q.QGDFoamCase(dev, q.default_options(**opt))

    def one_step():
        c.set_fields(*fields)
        c.step(1)
        return {f: c.field(f).copy() for f in FIELDS}

    set_bcs(c, mesh)
    uni = one_step()
    set_bcs(c, mesh, U=U, T=T, p=p)
    for field, want in (("U", U), ("T", T), ("p", p)):
        got, is_list = c.get_bc_values({"U": 0, "p": 1, "T": 2}[field], field)
        assert is_list and np.array_equal(got, want), field
    got, is_list = c.get_bc_values(0, "T")
    assert not is_list and np.array_equal(got, np.full(len(U), 1.02))
    with pytest.raises(q.QgdError):
        c.step(1)                                  # like set_bc: the fields are set again first
    base = one_step()
    own = mesh.array("owner")
    ps = mesh.array("patchStart")
    for field, patch, values, j in (("U", 0, U, 7), ("T", 2, T, 3), ("p", 1, p, 11)):
        changed = np.array(values, copy=True)
        changed[j] = changed[j] * 1.05 + 0.01
        c.set_bc_values(patch, field, changed)
        got = one_step()
        cell = int(own[int(ps[patch]) + j])
        assert any(np.any(got[f][cell] != base[f][cell]) for f in FIELDS), (field, cell)
        c.set_bc_values(patch, field, values)
    again = one_step()
    for f in FIELDS:
        assert np.array_equal(again[f], base[f]), f
    # dropping the lists: the uniform values of the entries are back (set_bcs gave the list entries 0 as their uniform value)
    set_bcs(c, mesh)
    pz = mesh.array("patchSize")
    c.set_bc_values(0, "U", np.tile(UNIFORM["U"] * 2.0, (int(pz[0]), 1)))
    c.set_bc_values(2, "T", np.full(int(pz[2]), 1.5))
    c.set_bc_values(1, "p", np.full(int(pz[1]), 1.5))
    for patch, field in ((0, "U"), (2, "T"), (1, "p")):
        c.set_bc_values(patch, field, None)
        assert not c.get_bc_values(patch, field)[1]
    dropped = one_step()
    for f in FIELDS:
        assert np.array_equal(dropped[f], uni[f]), f
    c.close(); dev.close()


def test_implicit_case_with_velocity_lists_assembles_with_the_separate_kernels():
    """the block-fused assembly of the U systems reads a patch's one velocity: a case with per-face velocities says it does not use it"""
    mesh = box()
    U, T, p = lists_of(mesh)
    dev = q.Device(mesh, fused_tables="any")
    c = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", **IMPL))
    set_bcs(c, mesh, T=T, p=p)
    assert c.fused_info()["fusedImplicit"]           # temperature and pressure lists reach the blocks through the patch records
    set_bcs(c, mesh, U=U, T=T, p=p)
    assert not c.fused_info()["fusedImplicit"] and c.fused_info()["blocks"] == 0
    c.set_fields(*fields_of(mesh))
    c.step(STEPS)
    want = run_device(mesh, dict(stencil="GaussVolPoint", **IMPL), False, "kernels", lambda k: set_bcs(k, mesh, U=U, T=T, p=p))
    for f in FIELDS:
        assert np.array_equal(c.field(f), want[f]), f
    c.set_bc_values(0, "U", None)
    assert c.fused_info()["fusedImplicit"]
    c.close(); dev.close()


# ---- 7: shards -----------------------------------------------------------------------------------------------------------------------------
def step_explicit_shards(devs, cs, shards, steps):
    peers = [[int(x) for x in s.array("haloPeer")] for s in shards]
    bufs = {}
    for r, c in enumerate(cs):
        for k, peer in enumerate(peers[r]):
            bufs[(r, peer)] = c.halo_buffer(max(c.halo_count(k), 1))
            bufs[("mid", r, peer)] = c.halo_buffer(max(c.mid_halo_count(k)[0], 1))

    def exchange(mid=False):
        for r, c in enumerate(cs):
            for k, peer in enumerate(peers[r]):
                (c.mid_halo_pack(k, bufs[("mid", r, peer)]) if mid else c.halo_pack(k, bufs[(r, peer)]))
        for c in cs:
            c.sync()
        for r, c in enumerate(cs):
            for k, peer in enumerate(peers[r]):
                (c.mid_halo_unpack(k, bufs[("mid", peer, r)]) if mid else c.halo_unpack(k, bufs[(peer, r)]))
        for c in cs:
            c.sync()

    exchange()
    for _ in range(steps):
        if cs[0].needs_mid_exchange():
            for c in cs:
                c.step_phase(5)
            exchange(mid=True)
            for c in cs:
                c.step_phase(6)
        else:
            for c in cs:
                c.step_phase(0)
        for c in cs:
            c.step_phase(1)
        exchange()


@pytest.mark.parametrize("tag,opt", [("explicit", dict(stencil="GaussVolPoint", **EXPL)), ("implicit", dict(stencil="GaussVolPoint", **IMPL))])
def test_cut_across_the_inlet_patch_matches_the_uncut_run(tag, opt):
    mesh = box()
    U, T, p = lists_of(mesh)
    fields = fields_of(mesh)
    bcs = [{"U": ("fixedValue", U), "T": ("fixedValue", 1.02), "p": ("zeroGradient", None)},
           {"U": ("zeroGradient", None), "T": ("zeroGradient", None), "p": ("fixedValue", p)},
           {"U": ("fixedValue", (0.0, 0.0, 0.0)), "T": ("fixedValue", T), "p": ("qgdFlux", None)}] + \
          [{"U": ("fixedValue", (0.0, 0.0, 0.0)), "T": ("zeroGradient", None), "p": ("qgdFlux", None)} for _ in range(3)]
    whole = run_device(mesh, opt, False, "kernels", lambda c: [c.set_bc(i, **b) for i, b in enumerate(bcs)], fields=fields)
    shards = [mesh.shard(2, r) for r in range(2)]
    devs, cs = [], []
    for s in shards:
        assert 0 < int(s.array("patchSize")[0]) < len(U)          # the cut crosses the inlet
        d = q.Device(s)
        c = q.QGDFoamCase(d, q.default_options(**opt))
        for i, b in enumerate(ff.device_bcs(mesh, s, bcs)):
            c.set_bc(i, **b)
        cg = s.array("cellGlobal")
        c.set_fields(fields[0][cg], fields[1][cg], fields[2][cg])
        devs.append(d); cs.append(c)
    if opt.get("implicitDiffusion"):
        ImplicitStepper(LocalWorld([ImplicitShard(c) for c in cs], [[int(x) for x in s.array("haloPeer")] for s in shards], kinds=range(5))).step(STEPS)
        for c in cs:
            c.sync()
    else:
        step_explicit_shards(devs, cs, shards, STEPS)
    for r, (s, c) in enumerate(zip(shards, cs)):
        cg = s.array("cellGlobal")
        lo, hi = (mesh.nCells * r) // 2, (mesh.nCells * (r + 1)) // 2
        own = (cg >= lo) & (cg < hi)
        for f in FIELDS:
            err = np.abs(c.field(f)[own] - whole[f][cg[own]]).max() / np.abs(whole[f]).max()
            print(f"shards {tag} rank {r} {f}: {err:.3e}")
            assert err <= 1e-12, (tag, r, f, err)
    for d, c in zip(devs, cs):
        c.close(); d.close()


# ---- 8: a mesh unrolled from a cyclic pair -------------------------------------------------------------------------------------------------
def test_copies_behind_cyclic_halves_take_their_originals_records():
    CY = L.PATCH_CYCLIC
    pm = q.PolyMesh.box(6, 5, 4, patch_types=[G, G, CY, CY, G, G])
    um = pm.unroll_cyclic([(2, 3)])
    n = int(pm.array("patchSize")[0])
    s = (np.arange(n) + 0.5) / n
    U = np.zeros((n, 3)); U[:, 0] = 0.1 * (0.4 + 2.4 * s * (1.0 - s))
    cg = um.array("cellGlobal")
    f0 = cases.box_initial_fields(pm.array("C").reshape(-1, 3))
    fields = tuple(a[cg] for a in f0)
    opt = dict(stencil="GaussVolPoint", **EXPL)

    def run(inlet):
        bcs = [{"U": ("fixedValue", inlet), "T": ("fixedValue", 1.02), "p": ("zeroGradient", None)},
               {"U": ("zeroGradient", None), "T": ("zeroGradient", None), "p": ("fixedValue", 1.0)}] + \
              [{"U": ("none", None), "T": ("none", None), "p": ("none", None)}] * 2 + \
              [{"U": ("fixedValue", (0.0, 0.0, 0.0)), "T": ("zeroGradient", None), "p": ("qgdFlux", None)}] * 2 + \
              [{"U": ("none", None), "T": ("none", None), "p": ("none", None)}]
        dev = q.Device(um)
        c = q.QGDFoamCase(dev, q.default_options(**opt))
        for i, b in enumerate(ff.device_bcs(pm, um, bcs)):
            c.set_bc(i, **b)
        c.set_fields(*fields)
        c.step(STEPS)          # (the library refreshes the copies after every step)
        out ={f: c.field(f).copy() for f in FIELDS}
        out.update({f + ".boundary": c.field(f + ".boundary").copy() for f in ("U", "T", "p", "rho")})
        c.close(); dev.close()
        return out

    got = run(U)
    assert np.all(np.isfinite(got["rho"][:pm.nCells]))
    fg = um.array("faceGlobal")
    nif = um.nInternalFaces
    ps, pz = um.array("patchStart"), um.array("patchSize")
    local_of = {int(g): f for f, g in enumerate(fg) if g >= 0}
    checked = 0
    for patch in (0, 1, 4, 5):
        for f in range(int(ps[patch]), int(ps[patch]) + int(pz[patch])):
            if fg[f] < 0:
                o = local_of[-1 - int(fg[f])]
                assert o >= nif
                for name in ("U.boundary", "T.boundary", "p.boundary", "rho.boundary"):
                    assert np.array_equal(got[name][f - nif], got[name][o - nif]), (patch, f, name)
                checked += 1
    assert checked > 0 and int(pz[0]) > n
    assert np.abs(got["U.boundary"][int(ps[0]) - nif: int(ps[0]) - nif + n] - U).max() == 0.0
    # the trivial configuration: a list of equal values is the uniform inlet
    uni = run(np.array([0.08, 0.0, 0.0]))
    eq = run(np.tile(np.array([0.08, 0.0, 0.0]), (n, 1)))
    for f in uni:
        assert np.array_equal(uni[f], eq[f]), f


# ---- 9: refusals by name -------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi():
    mesh = q.PolyMesh.box(6, 5, 1, hi=(1.0, 1.0, 0.1), patch_types=[G, G, L.PATCH_SYMMETRYPLANE, G, E, E])
    dev = q.Device(mesh)
    c = q.QGDFoamCase(dev, q.default_options(stencil="leastSquares", **EXPL))
    c.set_bc(0, U=("fixedValue", (0.1, 0.0, 0.0)), T=("fixedValue", 1.0), p=("qgdFlux", None))
    n = int(mesh.array("patchSize")[0])
    with pytest.raises(q.QgdError, match=r"has 5 faces on this device's mesh, nFaces = 6"):
        c.set_bc_values(0, "T", np.ones(n + 1))
    with pytest.raises(q.QgdError, match=r"the p entry of patch '.*' is not fixedValue"):
        c.set_bc_values(0, "p", np.ones(n))
    with pytest.raises(q.QgdError, match=r"is a constraint patch"):
        c.set_bc_values(2, "U", np.zeros((int(mesh.array("patchSize")[2]), 3)))
    with pytest.raises(q.QgdError, match=r"patch out of range"):
        c.set_bc_values(9, "T", np.ones(n))
    with pytest.raises(ValueError, match="fixedValue"):
        c.set_bc(3, T=("zeroGradient", np.ones(6)))
    c.set_bc_values(0, "T", np.ones(n))             # and what is allowed passes
    c.close(); dev.close()
    sh = q.PolyMesh.box(6, 5, 4).shard(2, 0)
    assert int(sh.array("patchType")[-1]) == L.PATCH_HALO
    d2 = q.Device(sh)
    c2 = q.QGDFoamCase(d2, q.default_options(stencil="GaussVolPoint", **EXPL))
    halo = sh.nPatches - 1
    with pytest.raises(q.QgdError, match=r"is a halo patch"):
        c2.set_bc_values(halo, "T", np.ones(int(sh.array("patchSize")[halo])))
    c2.close(); d2.close()


# ---- 10 (and the round trip through write_time): the application ---------------------------------------------------------------------------
def test_application_runs_a_case_with_value_lists(tmp_path):
    from qgdsolver_amd import QGDFoam as app
    from test_bc_value_lists import write_list_case
    case_dir = str(tmp_path / "c")
    mesh, U, T = write_list_case(case_dir)
    dev, case, written = app.run(case_dir, n_steps=3, log=lambda *a, **k: None)
    assert len(written) == 3
    m2, opt, fields, bcs = ff.read_case_setup(case_dir, written[-1])
    by = dict(zip(m2.patch_names, bcs))
    assert np.array_equal(by["inlet"]["U"][1], U) and np.array_equal(by["bottom"]["T"][1], T)
    assert by["inlet"]["T"] == ("fixedValue", 1.0)
    case.close(); dev.close()
    # QGDFoamCase driven directly
    m0, opt0, fields0, bcs0 = ff.read_case_setup(case_dir, "0")
    d = q.Device(m0, fv_schemes={"fvsc": {"default": opt0["stencil"]}})
    c = q.QGDFoamCase(d, q.default_options(**opt0))
    for i, b in enumerate(bcs0):
        c.set_bc(i, U=b["U"], T=b["T"], p=b["p"])
    c.set_fields(fields0["U"], fields0["T"], fields0["p"])
    c.step(3)
    for f in ("U", "T", "p"):
        assert np.array_equal(np.asarray(fields[f]).reshape(c.field(f).shape), c.field(f)), f
    # write_time after load_case: the lists come back exactly, uniform entries stay uniform
    c.close(); d.close()
    d3, c3 = ff.load_case(case_dir, "0")
    ff.write_time(c3, case_dir, "7", bcs0)
    text = open(os.path.join(case_dir, "7", "T")).read()
    assert "uniform 1.0;" in text.split("inlet")[1].split("}")[0] and "nonuniform List<scalar>" in text.split("bottom")[1].split("}")[0]
    m7, opt7, fields7, bcs7 = ff.read_case_setup(case_dir, "7")
    for a, b in zip(bcs0, bcs7):
        for f in ("U", "T", "p"):
            assert a[f][0] == b[f][0] and np.shape(a[f][1]) == np.shape(b[f][1]) and (a[f][1] is None or np.array_equal(a[f][1], b[f][1])), (f, a[f], b[f])
    c3.close(); d3.close()
