"""The case entries of the C-ABI that the three resident cases (QGDFoam, QHDFoam, scalarTransportQHDFoam) serve from one core: set_bc,
the per-face value lists, the implicit-solve accessors, the public halo entries, the monitor's sample.  Every refusal is pinned with its
code and its complete message; the served paths with what they return.  Meshes of a dozen cells: nothing here depends on size."""
import ctypes as C

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L
from qgdsolver_amd import qhdfoam, scalarfoam

pytestmark = pytest.mark.gpu
G, E = L.PATCH_GENERIC, L.PATCH_EMPTY
INV = L.ERR_INVALID
KINDS = ("qgd", "qhd", "scalar")


def dp(a):
    return a.ctypes.data_as(L.c_double_p)


def refused(rc, message, code=INV):
    """rc is the status an entry returned just now: the QgdError made of it carries `code` and exactly `message`"""
    with pytest.raises(q.QgdError) as ei:
        L.check(rc, "entry")
    assert ei.value.code == code
    assert str(ei.value) == f"entry: status {code}: {message}"


def make_case(kind, dev, implicit=0):
    if kind == "qgd":
        return q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3, mu=1e-2, implicitDiffusion=implicit))
    if kind == "qhd":
        return qhdfoam.QHDFoamCase(dev, qhdfoam.qhd_options(stencil="GaussVolPoint", tauModel="HbyUQHD", aQGD=0.5, UQHD=1.0, rho0=1.0, mu=1e-2,
                                                            Pr=0.71, beta=3e-3, g=(0.0, -9.81, 0.0), deltaT=1e-3, pTol=1e-10, pMaxIter=200,
                                                            pRefCell=0, pRefValue=0.0, implicitDiffusion=implicit))
    return scalarfoam.ScalarTransportQHDCase(dev, scalarfoam.scalar_options(stencil="GaussVolPoint", deltaT=1e-3, mu=1e-2, implicitDiffusion=implicit))


def fields(mesh, seed=3):
    rng = np.random.default_rng(seed)
    n = mesh.nCells
    return 0.05 * rng.standard_normal((n, 3)), 1.0 + 0.02 * rng.standard_normal(n), 1.0 + 0.02 * rng.standard_normal(n)


def set_fields(kind, c, mesh):
    U, T, p = fields(mesh)
    if kind == "scalar":
        c.set_fields(U, T)
    else:
        c.set_fields(U, T, p)


SET_BC = {"qgd": L.lib.qgd_case_set_bc, "qhd": L.lib.qgd_qhd_case_set_bc, "scalar": L.lib.qgd_scalar_case_set_bc}
SET_BC_NAME = {"qgd": "qgd_case_set_bc", "qhd": "qgd_qhd_case_set_bc", "scalar": "qgd_scalar_case_set_bc"}


def raw_set_bc(kind, h, patch, bcU, bcT, bcP=L.BC_ZEROGRADIENT):
    vu = np.zeros(3)
    if kind == "scalar":
        return SET_BC[kind](h, patch, bcU, dp(vu), bcT, 1.0)
    return SET_BC[kind](h, patch, bcU, dp(vu), bcT, 1.0, bcP, 1.0)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_set_bc_refusals(kind):
    mesh = q.PolyMesh.box(3, 2, 2)
    dev = q.Device(mesh)
    c = make_case(kind, dev)
    w = SET_BC_NAME[kind]
    Z, F = L.BC_ZEROGRADIENT, L.BC_FIXEDVALUE
    refused(raw_set_bc(kind, None, 0, Z, Z), "null case")
    refused(raw_set_bc(kind, c._h, -1, Z, Z), f"{w}: patch out of range")
    refused(raw_set_bc(kind, c._h, 6, Z, Z), f"{w}: patch out of range")
    refused(raw_set_bc(kind, c._h, 0, 17, Z), f"{w}: unsupported boundary-condition kind")
    refused(raw_set_bc(kind, c._h, 0, Z, L.BC_SLIP), f"{w}: unsupported boundary-condition kind")
    refused(raw_set_bc(kind, c._h, 0, L.BC_QHDFLUX, Z), f"{w}: unsupported boundary-condition kind")
    if kind == "qgd":
        refused(raw_set_bc(kind, c._h, 0, Z, Z, L.BC_QHDFLUX), f"{w}: unsupported boundary-condition kind")
    if kind == "qhd":
        assert raw_set_bc(kind, c._h, 0, Z, Z, L.BC_QHDFLUX) == L.QGD_OK      # the p kind only the QHD case admits
    if kind != "scalar":
        refused(raw_set_bc(kind, c._h, 0, Z, Z, L.BC_SLIP), f"{w}: unsupported boundary-condition kind")
    assert raw_set_bc(kind, c._h, 1, F, F) == L.QGD_OK
    set_fields(kind, c, mesh)
    c.step(1)
    c.close(); dev.close()


def with_empty_cyclic_patch(mesh):
    """the same mesh with a seventh patch, cyclic and without faces (what a decomposed case leaves on a rank the pair does not touch): the
    only cyclic patch a resident case is created with"""
    pr = mesh.primitives()
    return q.PolyMesh.from_arrays(pr["points"], pr["faceOffsets"], pr["facePoints"], pr["owner"], pr["neighbour"], pr["nCells"],
                                  np.append(pr["patchStart"], mesh.nFaces), np.append(pr["patchSize"], 0), np.append(pr["patchType"], L.PATCH_CYCLIC))


def raw_set_values(kind, h, patch, field, values, n):
    ptr = dp(values) if values is not None else None
    if kind == "qgd":
        return L.lib.qgd_case_set_bc_values(h, patch, field, ptr, n)
    assert field == 0
    return L.lib.qgd_qhd_case_set_bc_values(h, patch, ptr, n)


@pytest.mark.parametrize("kind", ["qgd", "qhd"])
def test_set_bc_values_refusals(kind):
    w = "qgd_case_set_bc_values" if kind == "qgd" else "qgd_qhd_case_set_bc_values"
    one = kind == "qhd"   # the QHD entry has one text for the three kinds of patch without entries
    no_entry = "' is a halo, cyclic or constraint patch: its faces carry no fixedValue entry"
    # a constraint patch, and the rows of an ordinary one
    mesh = q.PolyMesh.box(4, 3, 1, patch_types=[G, G, G, G, E, E])
    dev = q.Device(mesh)
    c = make_case(kind, dev)
    c.set_bc(0, U=("fixedValue", (0.1, 0.0, 0.0)), T=("fixedValue", 1.0))
    n = int(mesh.array("patchSize")[0])
    assert n == 3
    good = np.tile(np.array([0.1, 0.02, 0.0]), (n, 1))
    refused(raw_set_values(kind, None, 0, 0, good, n), f"{w}: null case")
    refused(raw_set_values(kind, c._h, 6, 0, good, n), f"{w}: patch out of range")
    refused(raw_set_values(kind, c._h, -1, 0, good, n), f"{w}: patch out of range")
    refused(raw_set_values(kind, c._h, 0, 0, np.zeros((n + 1, 3)), n + 1), f"{w}: patch 'xMin' has 3 faces on this device's mesh, nFaces = 4")
    refused(raw_set_values(kind, c._h, 0, 0, good, n - 1), f"{w}: patch 'xMin' has 3 faces on this device's mesh, nFaces = 2")
    refused(raw_set_values(kind, c._h, 1, 0, good, n), f"{w}: the U entry of patch 'xMax' is not fixedValue (per-face values belong to fixedValue entries only)")
    refused(raw_set_values(kind, c._h, 4, 0, np.zeros((12, 3)), 12),
            f"{w}: patch 'zMin{no_entry}" if one else f"{w}: patch 'zMin' is a constraint patch (empty / symmetryPlane / symmetry / wedge): it keeps its own field type")
    if kind == "qgd":
        refused(raw_set_values(kind, c._h, 0, 3, good, n), f"{w}: field must be 0 (U), 1 (T) or 2 (p)")
        refused(raw_set_values(kind, c._h, 0, 2, np.ones(n), n), f"{w}: the p entry of patch 'xMin' is not fixedValue (per-face values belong to fixedValue entries only)")
        out, flag = np.zeros((n, 3)), C.c_int32(7)
        refused(L.lib.qgd_case_get_bc_values(c._h, 0, 0, dp(out), n + 1, C.byref(flag)),
                "qgd_case_get_bc_values: patch 'xMin' has 3 faces on this device's mesh, nFaces = 4")
        refused(L.lib.qgd_case_get_bc_values(c._h, 0, 0, None, n, C.byref(flag)), "qgd_case_get_bc_values: null argument")
        refused(L.lib.qgd_case_get_bc_values(c._h, 1, 1, dp(out), n, C.byref(flag)),
                "qgd_case_get_bc_values: the T entry of patch 'xMax' is not fixedValue (per-face values belong to fixedValue entries only)")
    else:
        bad = good.copy(); bad[1, 2] = np.nan
        refused(raw_set_values(kind, c._h, 0, 0, bad, n), f"{w}: non-finite value")
        bad[1, 2] = np.inf
        refused(raw_set_values(kind, c._h, 0, 0, bad, n), f"{w}: non-finite value")
    # a list arrives, and a null list clears the flag again whatever nFaces says
    assert raw_set_values(kind, c._h, 0, 0, good, n) == L.QGD_OK
    if kind == "qgd":
        got, is_list = c.get_bc_values(0, "U")
        assert is_list and np.array_equal(got, good)
    assert raw_set_values(kind, c._h, 0, 0, None, 99) == L.QGD_OK
    if kind == "qgd":
        got, is_list = c.get_bc_values(0, "U")
        assert not is_list and np.array_equal(got, np.tile(np.array([0.1, 0.0, 0.0]), (n, 1)))
    U, T, p = fields(mesh)
    U[:, 2] = 0.0
    c.set_fields(U, T, p)
    first = int(mesh.array("patchStart")[0]) - mesh.nInternalFaces
    assert np.array_equal(c.field("U.boundary")[first:first + n], np.tile(np.array([0.1, 0.0, 0.0]), (n, 1)))   # the uniform value again
    c.close(); dev.close()
    # a halo patch
    sh = q.PolyMesh.box(3, 2, 4).shard(2, 0)
    halo = sh.nPatches - 1
    assert int(sh.array("patchType")[halo]) == L.PATCH_HALO
    nh = int(sh.array("patchSize")[halo])
    d2 = q.Device(sh)
    c2 = make_case(kind, d2)
    refused(raw_set_values(kind, c2._h, halo, 0, np.zeros((nh, 3)), nh),
            f"{w}: patch 'halo{no_entry}" if one else f"{w}: patch 'halo' is a halo patch (its faces carry no boundary condition)")
    c2.close(); d2.close()
    # a cyclic patch
    cm = with_empty_cyclic_patch(q.PolyMesh.box(3, 2, 2))
    d3 = q.Device(cm)
    c3 = make_case(kind, d3)
    refused(raw_set_values(kind, c3._h, 6, 0, np.zeros((1, 3)), 0),
            f"{w}: patch 'patch6{no_entry}" if one else f"{w}: patch 'patch6' is a cyclic patch (its faces carry no boundary condition)")
    c3.close(); d3.close()


@pytest.mark.parametrize("kind", ["qgd", "qhd"])
def test_implicit_accessors_without_the_branch(kind):
    mesh = q.PolyMesh.box(3, 2, 2)
    dev = q.Device(mesh)
    c = make_case(kind, dev, implicit=0)
    pre = "qgd_case_implicit" if kind == "qgd" else "qgd_qhd_case_implicit"
    ctl, ptr, st = np.zeros(68), C.c_void_p(), np.zeros(2)
    text = {"qgd": lambda e: "bad argument", "qhd": lambda e: f"{pre}_{e}: an implicitDiffusion case is needed"}[kind]
    for set_ in (0, 1):
        refused(getattr(L.lib, pre + "_control")(c._h, dp(ctl), set_), text("control"))
    refused(getattr(L.lib, pre + "_control")(None, dp(ctl), 0), text("control"))
    refused(getattr(L.lib, pre + "_control_ptr")(c._h, C.byref(ptr)), text("control_ptr"))
    refused(getattr(L.lib, pre + "_control_ptr")(None, C.byref(ptr)), text("control_ptr"))
    refused(getattr(L.lib, pre + "_solve_status")(c._h, dp(st)), text("solve_status"))
    refused(getattr(L.lib, pre + "_solve_status")(None, dp(st)), text("solve_status"))
    refused(getattr(L.lib, pre + "_info")(None, dp(np.zeros(16))), "null argument" if kind == "qgd" else "bad argument")
    info = np.full(16, 7.0)
    assert getattr(L.lib, pre + "_info")(c._h, dp(info)) == L.QGD_OK and not info.any()     # no branch: sixteen zeros
    c.close(); dev.close()


def slab():
    """the lower of the two cell-range shards of box(3, 2, 4): one halo slot towards the upper one, a halo patch behind the box's six;
    (mesh, (cells it sends, real-patch boundary faces of those cells), the same two of its ghost cells)"""
    sh = q.PolyMesh.box(3, 2, 4).shard(2, 0)
    assert sh.halo_slots == 1
    ps, pz, pt = sh.array("patchStart"), sh.array("patchSize"), sh.array("patchType")
    owner = sh.array("owner")

    def sizes(cells):
        return int(cells.size), sum(int(np.isin(owner[s:s + z], cells).sum()) for s, z, t in zip(ps, pz, pt) if t != L.PATCH_HALO)

    send, ghost = sizes(sh.array("haloSend0")), sizes(sh.array("haloGhost0"))
    assert send == (6, 10) and ghost[0] == 6      # one plane of 3 x 2 cells and its rim
    return sh, send, ghost


def test_qgd_halo_entries():
    sh, (n_send, n_bf), (n_ghost, n_gbf) = slab()
    dev = q.Device(sh)
    c = make_case("qgd", dev, implicit=0)
    ci = make_case("qgd", dev, implicit=1)
    n, m = C.c_int64(-5), C.c_int64(-5)
    buf = dev.alloc(8 * (9 * n_send + 12 * n_bf))
    for fn in (L.lib.qgd_case_halo_count, L.lib.qgd_case_halo_recv_count):
        refused(fn(c._h, -1, C.byref(n)), "bad argument")
        refused(fn(None, 0, C.byref(n)), "bad argument")
        refused(fn(c._h, 0, None), "bad argument")
    refused(L.lib.qgd_case_mid_halo_count(c._h, -1, C.byref(n), C.byref(m)), "bad argument")
    refused(L.lib.qgd_case_mid_halo_count(c._h, 0, None, C.byref(m)), "bad argument")
    for fn in (L.lib.qgd_case_halo_pack, L.lib.qgd_case_halo_unpack, L.lib.qgd_case_mid_halo_pack, L.lib.qgd_case_mid_halo_unpack):
        refused(fn(c._h, -1, buf), "bad argument")
        refused(fn(None, 0, buf), "bad argument")
        refused(fn(c._h, 0, None), "null buffer")
        assert fn(c._h, 1, None) == L.QGD_OK                    # a slot beyond the device's: nothing to move
    for kind in (0, 5, -1):
        refused(L.lib.qgd_case_implicit_halo_count(ci._h, 0, kind, C.byref(n), C.byref(m)), "bad argument")
        refused(L.lib.qgd_case_implicit_halo_pack(ci._h, 0, kind, buf), "bad argument")
        refused(L.lib.qgd_case_implicit_halo_unpack(ci._h, 0, kind, buf), "bad argument")
    refused(L.lib.qgd_case_implicit_halo_count(ci._h, -1, 1, C.byref(n), C.byref(m)), "bad argument")
    for kind in (1, 2, 3, 4):                                   # without the branch
        refused(L.lib.qgd_case_implicit_halo_count(c._h, 0, kind, C.byref(n), C.byref(m)), "qgd_case_implicit_halo_count: not an implicitDiffusion case")
        assert (n.value, m.value) == (0, 0)
        refused(L.lib.qgd_case_implicit_halo_pack(c._h, 0, kind, buf), "bad argument")
        refused(L.lib.qgd_case_implicit_halo_unpack(c._h, 0, kind, buf), "bad argument")
    refused(L.lib.qgd_case_implicit_halo_pack(ci._h, 0, 1, None), "null buffer")
    # the counts: perCell * nSend + perFace * nSendBF, received the same of the ghost cells (kind 0: 8 and 12, kind 5: 0 and 2, kinds 1..4:
    # 9, 3, 3, 3 and no faces)
    assert c.halo_count(0) == 8 * n_send + 12 * n_bf and c.halo_recv_count(0) == 8 * n_ghost + 12 * n_gbf
    assert c.mid_halo_count(0) == (2 * n_bf, 2 * n_gbf)
    assert c.halo_count(1) == 0 and c.halo_recv_count(1) == 0 and c.mid_halo_count(1) == (0, 0)
    for kind, per_cell in ((1, 9), (2, 3), (3, 3), (4, 3)):
        assert ci.implicit_halo_count(0, kind) == (per_cell * n_send, per_cell * n_ghost)
        assert tuple(ci.implicit_halo_count(1, kind)) == (0, 0)
    # and a message goes out and comes back
    U, T, p = fields(sh)
    c.set_fields(U, T, p)
    c.halo_pack(0, buf)
    c.sync()
    dev.release(buf)
    c.close(); ci.close(); dev.close()


def test_qhd_halo_entries():
    sh, (n_send, n_bf), (n_ghost, n_gbf) = slab()
    dev = q.Device(sh)
    c = make_case("qhd", dev, implicit=0)
    n, m = C.c_int64(-5), C.c_int64(-5)
    buf = dev.alloc(8 * (10 * n_send + 4 * n_bf))
    for slot, kind in ((-1, 0), (0, -1), (0, 5)):
        refused(L.lib.qgd_qhd_case_halo_count(c._h, slot, kind, C.byref(n), C.byref(m)), "bad argument")
        refused(L.lib.qgd_qhd_case_halo_pack(c._h, slot, kind, buf), "bad argument")
        refused(L.lib.qgd_qhd_case_halo_unpack(c._h, slot, kind, buf), "bad argument")
    refused(L.lib.qgd_qhd_case_halo_count(None, 0, 0, C.byref(n), C.byref(m)), "bad argument")
    refused(L.lib.qgd_qhd_case_halo_count(c._h, 0, 0, None, C.byref(m)), "bad argument")
    for fn in (L.lib.qgd_qhd_case_halo_pack, L.lib.qgd_qhd_case_halo_unpack):
        refused(fn(None, 0, 0, buf), "bad argument")
        refused(fn(c._h, 0, 0, None), "null buffer")
        assert fn(c._h, 1, 0, None) == L.QGD_OK                 # a slot beyond the device's
        refused(fn(c._h, 0, 2, buf), "no solve in flight")      # before set_fields
    per = {0: (4, 4), 1: (10, 2), 2: (1, 0), 3: (1, 0), 4: (4, 0)}
    for kind, (per_cell, per_face) in per.items():
        assert tuple(c.halo_count(0, kind)) == (per_cell * n_send + per_face * n_bf, per_cell * n_ghost + per_face * n_gbf)
        assert tuple(c.halo_count(1, kind)) == (0, 0)
    U, T, p = fields(sh)
    c.set_fields(U, T, p)
    for fn in (L.lib.qgd_qhd_case_halo_pack, L.lib.qgd_qhd_case_halo_unpack):
        refused(fn(c._h, 0, 4, buf), "message kind 4 belongs to the implicitDiffusion branch")
        refused(fn(c._h, 0, 3, buf), "message kind 3: no multigrid iterate is waiting for its ghost entries (qgd_qhd_case_pending)")
    c.halo_pack(0, 0, buf)
    c.sync()
    dev.release(buf)
    c.close(); dev.close()


@pytest.mark.parametrize("kind", ["qgd", "qhd"])
def test_monitor_sample_is_refused_after_set_bc(kind):
    mesh = q.PolyMesh.box(3, 2, 2)
    dev = q.Device(mesh)
    c = make_case(kind, dev)
    set_fields(kind, c, mesh)
    mon = c.monitor(probes=[0], patches=[0])
    mon.sample(0)
    mon.read_raw(0)
    c.set_bc(0, U=("fixedValue", (0.1, 0.0, 0.0)))
    refused(L.lib.qgd_monitor_sample(mon._h, 1),
            "qgd_monitor_sample: the case's boundary conditions or coefficients changed: call qgd_case_set_fields first" if kind == "qgd"
            else "qgd_monitor_sample: the case's boundary conditions changed: call qgd_qhd_case_set_fields first")
    refused(L.lib.qgd_monitor_sample(mon._h, 4), "qgd_monitor_sample: slot must be 0..3")
    set_fields(kind, c, mesh)
    assert mon.sample(1) == 1
    out, t, step = mon.read_raw(1)
    assert out.size == mon.n_doubles and (t, step) == (0.0, 0)
    stale = mon._h
    mon.close()
    for handle in (stale, None):       # a freed monitor's handle is known by its value alone: nothing behind it is read
        refused(L.lib.qgd_monitor_sample(handle, 0), "qgd_monitor_sample: not an open monitor (a monitor is freed with its case)")
    c.close(); dev.close()


# ---- the served paths -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("implicit", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_entries_in_order(kind, implicit):
    """set_bc -> set_bc_values where served -> set_fields -> 2 steps, then what the accessors give"""
    mesh = q.PolyMesh.box(3, 2, 2)
    dev = q.Device(mesh)
    c = make_case(kind, dev, implicit=implicit)
    n = int(mesh.array("patchSize")[0])
    first = int(mesh.array("patchStart")[0]) - mesh.nInternalFaces
    c.set_bc(0, U=("fixedValue", (0.1, 0.0, 0.0)), T=("fixedValue", 1.0))
    rng = np.random.default_rng(11)
    Ub = np.array([0.1, 0.0, 0.0]) + 0.01 * rng.standard_normal((n, 3))
    Tb = 1.0 + 0.01 * rng.standard_normal(n)
    if kind == "qgd":
        c.set_bc_values(0, "U", Ub)
        c.set_bc_values(0, "T", Tb)
        for field, want in (("U", Ub), ("T", Tb)):
            got, is_list = c.get_bc_values(0, field)
            assert is_list and np.array_equal(got, want)
    elif kind == "qhd":
        c.set_bc_values(0, Ub)
    set_fields(kind, c, mesh)
    if kind != "scalar":
        assert np.array_equal(c.field("U.boundary")[first:first + n], Ub)
    c.step(2)
    c.sync()
    names = {"qgd": ("rho", "U", "p", "e"), "qhd": ("U", "T", "p"), "scalar": ("T",)}[kind]
    for name in names:
        assert np.isfinite(c.field(name)).all(), name
    if kind == "scalar":
        i = c.info()
        assert i["steps"] == 2 and (i["solver"] is None) == (not implicit)
        assert (i["iterations"] > 0) == bool(implicit) and i["unconverged_steps"] == 0
        c.close(); dev.close()
        return
    pre = "qgd_case_implicit" if kind == "qgd" else "qgd_qhd_case_implicit"
    info = np.full(16, 7.0)
    assert getattr(L.lib, pre + "_info")(c._h, dp(info)) == L.QGD_OK
    if not implicit:
        assert not info.any()
    else:
        assert np.isfinite(info).all() and info[13] in (1.0, 2.0) and info[15] == 0.0
        assert (info[0:4] > 0).all()                            # Ux, Uy, Uz and e (QGD) / T (QHD): every system was solved
        assert (info[4:8] > 0).all() and (info[8:12] >= 0).all() and (info[8:12] < info[4:8]).all()
        assert info[12] == 0.0                                  # no step stopped above its tolerance
        ctl = np.full(68, np.nan)
        assert getattr(L.lib, pre + "_control")(c._h, dp(ctl), 0) == L.QGD_OK and np.isfinite(ctl).all()
        back = np.full(68, np.nan)
        assert getattr(L.lib, pre + "_control")(c._h, dp(ctl), 1) == L.QGD_OK
        assert getattr(L.lib, pre + "_control")(c._h, dp(back), 0) == L.QGD_OK and np.array_equal(back, ctl)
        ptr = C.c_void_p()
        assert getattr(L.lib, pre + "_control_ptr")(c._h, C.byref(ptr)) == L.QGD_OK and ptr.value
        st = np.full(2, np.nan)
        assert getattr(L.lib, pre + "_solve_status")(c._h, dp(st)) == L.QGD_OK
        assert st[0] in (0.0, 1.0) and st[1] == (1.0 if kind == "qgd" else 4.0)     # the last solve of a QGD step is e's one system, a QHD step has one of four
    c.close(); dev.close()
