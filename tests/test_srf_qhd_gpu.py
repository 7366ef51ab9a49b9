"""SRFQHDFoam on the device: the QHD case in a single rotating frame (qgd_qhd_case_set_srf), per-face fixedValue velocities
(qgd_qhd_case_set_bc_values), the reader's refusals at the C-ABI and the application.

The Coriolis force is checked against the CPU oracle by superposition (srf_ref.py): the oracle knows beta*T*g only, a QHD step is
affine in the body force.  Bar: 1e-9 of each field's scale, the bar test_qhd_case.py uses for device against oracle; the
superposition itself reproduces a direct oracle run to 4e-16 (explicit) and, with implicitTol = 1e-12, well below 2.4e-11
(implicit), both measured on the CPU."""
import os

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L, foamfile as ff, qhdfoam

import srf_ref as R
from util import make_mesh

pytestmark = pytest.mark.gpu

ARMS = [("box654_jitter", "GaussVolPoint", False), ("box654_tri", "GaussVolPoint", False), ("tet433", "GaussVolPoint", False),
        ("box654", "GaussVolPoint", True), ("plane2d_jitter", "leastSquares", False), ("plane2d", "GaussVolPoint", False)]


def srf_case(dev, opt, bcs, omega, solve_T, fields):
    c = qhdfoam.QHDFoamCase(dev, opt)
    c.set_srf(omega, solve_T=solve_T)
    R.apply_bcs(c, bcs)
    c.set_fields(*fields)
    return c


@pytest.mark.parametrize("implicit", [0, 1])
@pytest.mark.parametrize("kind,stencil,slip", ARMS)
def test_coriolis_step_matches_the_superposed_oracle(kind, stencil, slip, implicit):
    mesh = make_mesh(kind)
    omega = R.OMEGA_3D if mesh.nGeometricD == 3 else R.OMEGA_2D
    opt = R.options(stencil, implicit)
    bcs = R.patch_bcs(mesh, slip)
    ref = R.SrfReference(mesh, opt, bcs, omega)
    dev = q.Device(mesh)
    fields = R.initial(mesh)
    cases = {solve_T: srf_case(dev, opt, bcs, omega, solve_T, fields) for solve_T in (False, True)}
    for c in cases.values():
        assert c.srf_info()["rotating"] and not c.fused_info()["fusedAdvance"]
    first = {}
    for solve_T, c in cases.items():
        assert c.srf_info()["frozenT"] == (not solve_T)
        for step in range(5):
            U, T, p = c.field("U"), c.field("T"), c.field("p")
            want, plain = ref.step(U, T, p)
            c.step(1)
            got = {f: c.field(f) for f in R.FIELDS}
            share = R.rel(want["U"], plain["U"])
            errs = {f: R.rel(got[f], want[f]) for f in R.FIELDS}
            print(f"{kind} {stencil} implicit={implicit} solve_T={solve_T} step {step}: Coriolis share of U {share:.3e}, errors {errs}")
            assert share >= 1e-3, share     # the test would pass on a kernel without the force otherwise
            for f in R.FIELDS:
                assert errs[f] <= 1e-9, (kind, stencil, implicit, solve_T, step, f, errs[f])
            if step == 0:
                first[solve_T] = got
    # the first step starts from the same state in both T modes: the same U, p, phi
    for f in R.FIELDS:
        if implicit:
            assert R.rel(first[False][f], first[True][f]) <= 1e-9, f    # (two solves to implicitTol)
        else:
            assert np.array_equal(first[False][f], first[True][f]), f
    for c in cases.values():
        c.close()
    ref.close()
    dev.close()


def cavity_state(mesh, seed=9):
    C = mesh.array("C").reshape(-1, 3)
    rng = np.random.default_rng(seed)
    return 1e-2 * rng.standard_normal((mesh.nCells, 3)), 300.0 + 10.0 * (0.5 - C[:, 0]) + 0.1 * rng.standard_normal(mesh.nCells), np.zeros(mesh.nCells)


def cavity_bcs(case, mesh):
    wall = dict(U=("fixedValue", (0.0, 0.0, 0.0)), p=("qhdFluxCoupled", None))
    for ip in range(mesh.nPatches):
        case.set_bc(ip, T=("fixedValue", 310.0) if ip == 0 else (("fixedValue", 290.0) if ip == 1 else ("zeroGradient", None)), **wall)


@pytest.mark.parametrize("implicit", [0, 1])
def test_zero_omega_with_solve_T_is_the_plain_case_bit_for_bit(implicit):
    mesh = make_mesh("box654_jitter")
    dev = q.Device(mesh)
    opt = R.options("GaussVolPoint", implicit, deltaT=1e-3)
    res = []
    for srf in (False, True):
        c = qhdfoam.QHDFoamCase(dev, opt)
        if srf:
            c.set_srf((0.0, 0.0, 0.0), solve_T=True)
            si = c.srf_info()
            assert not si["rotating"] and not si["frozenT"] and np.all(si["omega"] == 0.0)
        cavity_bcs(c, mesh)
        c.set_fields(*cavity_state(mesh))
        c.step(10)
        res.append({f: c.field(f) for f in ("U", "T", "p", "phi")})
        c.close()
    for f in res[0]:
        assert np.isfinite(res[0][f]).all() and np.abs(res[0][f]).max() > 0
        assert np.array_equal(res[0][f], res[1][f]), f
    dev.close()


@pytest.mark.parametrize("implicit", [0, 1])
def test_frozen_T_is_never_written_and_leaves_the_flow_alone_without_buoyancy(implicit):
    mesh = make_mesh("box654_jitter")
    dev = q.Device(mesh)
    opt = R.options("GaussVolPoint", implicit, deltaT=1e-3, beta=0.0)
    U, T, p = cavity_state(mesh)
    U = U + 0.05
    plain = qhdfoam.QHDFoamCase(dev, opt)
    cavity_bcs(plain, mesh)
    plain.set_fields(U, T, p)
    frozen = qhdfoam.QHDFoamCase(dev, opt)
    frozen.set_srf((0.0, 0.0, 0.0))
    assert frozen.srf_info()["frozenT"] and not frozen.srf_info()["rotating"]
    cavity_bcs(frozen, mesh)
    frozen.set_fields(U, T, p)
    T0, Tb0 = frozen.field("T"), frozen.field("T.boundary")
    assert np.array_equal(T0, T)
    plain.step(10); frozen.step(10)
    assert np.array_equal(frozen.field("T"), T0) and np.array_equal(frozen.field("T.boundary"), Tb0)
    assert np.abs(plain.field("T") - T0).max() > 1e-6      # the plain case does advance T
    for f in ("U", "p", "phi"):
        ref = plain.field(f)
        assert np.abs(ref).max() > 0 and R.rel(frozen.field(f), ref) <= 1e-12, (f, R.rel(frozen.field(f), ref))
    if implicit:
        it = frozen.implicit_info()["solves"]
        assert it["T"]["iterations"] == 0 and it["Ux"]["iterations"] > 0, it
        assert plain.implicit_info()["solves"]["T"]["iterations"] > 0
    plain.close(); frozen.close(); dev.close()


@pytest.mark.parametrize("rotating", [False, True])
@pytest.mark.parametrize("implicit", [0, 1])
def test_per_face_velocity_list(rotating, implicit):
    mesh = make_mesh("box654_jitter")
    dev = q.Device(mesh)
    opt = R.options("GaussVolPoint", implicit)
    bcs = R.patch_bcs(mesh)
    fields = R.initial(mesh)
    ps, pz = mesh.array("patchStart"), mesh.array("patchSize")
    n0, b0 = int(pz[0]), int(ps[0]) - mesh.nInternalFaces

    def make():
        c = qhdfoam.QHDFoamCase(dev, opt)
        if rotating:
            c.set_srf(R.OMEGA_3D)
        R.apply_bcs(c, bcs)
        return c

    uni, lst = make(), make()
    lst.set_bc_values(0, np.tile(np.asarray(bcs[0]["U"][1]), (n0, 1)))
    for c in (uni, lst):
        c.set_fields(*fields)
        c.step(5)
    for f in ("U", "T", "p", "phi", "U.boundary"):
        assert np.array_equal(uni.field(f), lst.field(f)), f
    # one value per face: read back exactly after five steps; the flow differs from the uniform patch's
    vals = np.asarray(bcs[0]["U"][1]) + 0.05 * np.random.default_rng(1).standard_normal((n0, 3))
    lst.set_bc_values(0, vals)
    lst.set_fields(*fields)
    lst.step(5)
    assert np.array_equal(lst.field("U.boundary")[b0:b0 + n0], vals)
    assert np.isfinite(lst.field("U")).all() and R.rel(lst.field("U"), uni.field("U")) > 1e-6
    # set_bc returns the patch to its one value
    lst.set_bc(0, **bcs[0])
    lst.set_fields(*fields)
    lst.step(5)
    for f in ("U", "p", "phi", "U.boundary"):
        assert np.array_equal(uni.field(f), lst.field(f)), f
    # refused by name
    with pytest.raises(q.QgdError, match="nFaces") as ei:
        lst.set_bc_values(0, vals[:-1])
    assert ei.value.code == L.ERR_INVALID
    with pytest.raises(q.QgdError, match="not fixedValue") as ei:
        lst.set_bc_values(1, np.zeros((int(pz[1]), 3)))
    assert ei.value.code == L.ERR_INVALID
    uni.close(); lst.close(); dev.close()


def test_set_srf_refusals():
    mesh = make_mesh("box654")
    dev = q.Device(mesh)
    c = qhdfoam.QHDFoamCase(dev, R.options())
    with pytest.raises(q.QgdError, match="non-finite") as ei:
        c.set_srf((0.0, np.nan, 1.0))
    assert ei.value.code == L.ERR_INVALID
    c.set_srf((0.0, 0.0, 1.0))
    R.apply_bcs(c, R.patch_bcs(mesh))
    c.set_fields(*R.initial(mesh))
    with pytest.raises(q.QgdError, match="before qgd_qhd_case_set_fields") as ei:
        c.set_srf((0.0, 0.0, 2.0))
    assert ei.value.code == L.ERR_INVALID
    c.close(); dev.close()
    # one empty direction: omega must be parallel to it
    mesh = make_mesh("plane2d")
    dev = q.Device(mesh)
    c = qhdfoam.QHDFoamCase(dev, R.options())
    with pytest.raises(q.QgdError, match="empty direction") as ei:
        c.set_srf((0.0, 1.0, 5.0))
    assert ei.value.code == L.ERR_INVALID
    c.set_srf((0.0, 0.0, 5.0))
    c.close(); dev.close()
    # 1-D
    mesh = make_mesh("line1d")
    dev = q.Device(mesh)
    c = qhdfoam.QHDFoamCase(dev, R.options("reduced"))
    with pytest.raises(q.QgdError, match="1-D") as ei:
        c.set_srf((0.0, 0.0, 5.0))
    assert ei.value.code == L.ERR_INVALID
    c.close(); dev.close()
    # a sharded device
    shard = q.PolyMesh.box(6, 5, 4).shard(2, 0)
    dev = q.Device(shard)
    c = qhdfoam.QHDFoamCase(dev, R.options())
    with pytest.raises(q.QgdError, match="sharded") as ei:
        c.set_srf((0.0, 0.0, 5.0))
    assert ei.value.code == L.ERR_NOT_IMPLEMENTED
    c.close(); dev.close()


def test_rotating_case_keeps_the_separate_kernels_under_QGD_QHD_FUSED(monkeypatch):
    mesh = q.PolyMesh.box(12, 10, 8).jitter(0.1, seed=3)
    opt = R.options("GaussVolPoint", 0)
    bcs = R.patch_bcs(mesh)
    fields = R.initial(mesh)
    res = {}
    for fused in ("0", "1"):
        monkeypatch.setenv("QGD_QHD_FUSED", fused)
        dev = q.Device(mesh, fused_tables=True)
        if fused == "1":
            plain = qhdfoam.QHDFoamCase(dev, opt)
            assert plain.fused_info()["fusedAdvance"]       # the variable does act on this mesh: a plain case takes the block kernel
            plain.close()
        c = qhdfoam.QHDFoamCase(dev, opt)
        c.set_srf(R.OMEGA_3D)
        assert not c.fused_info()["fusedAdvance"]
        R.apply_bcs(c, bcs)
        c.set_fields(*fields)
        c.step(5)
        res[fused] = {f: c.field(f) for f in ("U", "T", "p", "phi")}
        c.close(); dev.close()
    for f in res["0"]:
        assert np.isfinite(res["0"][f]).all() and np.array_equal(res["0"][f], res["1"][f]), f


def test_srfqhdfoam_application_restart_and_absolute_velocity(tmp_path, monkeypatch):
    """(OpenFOAM's start value of the pressure solve, QGD_QHD_PEXTRAP=0: the default start value extrapolates p over the steps before,
    which a restart does not have -- same answer to pTol, not the same bits)"""
    from qgdsolver_amd import SRFQHDFoam

    monkeypatch.setenv("QGD_QHD_PEXTRAP", "0")
    monkeypatch.setenv("QGD_IMPL_XEXTRAP", "0")

    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for d in (a, b):
        os.makedirs(d)
        mesh = R.write_srf_case(d)
    log = []
    dev, case, written = SRFQHDFoam.run(a, log=log.append)
    text = "\n".join(log)
    assert written == ["0.003", "0.006"] and "SRFQHDFoam" in text and "omega (0 0 6.28318531)" in text and "T frozen" in text and text.endswith("End")
    si = case.srf_info()
    assert si["rotating"] and si["frozenT"] and np.allclose(si["omega"], (0.0, 0.0, 2.0 * np.pi))
    assert np.abs(case.field("U")).max() > 1e-4          # the casing drags the fluid
    state = {f: case.field(f) for f in ("U", "T", "p")}
    case.close(); dev.close()
    # the same run stopped after 3 steps and started again from the latest time
    dev, case, written = SRFQHDFoam.run(b, n_steps=3, log=lambda s: None)
    assert written == ["0.003"]
    case.close(); dev.close()
    dev, case, written = SRFQHDFoam.run(b, log=lambda s: None)
    assert written == ["0.006"]
    case.close(); dev.close()
    m2 = ff.read_polymesh(os.path.join(a, "constant", "polyMesh"))
    C = m2.array("C").reshape(-1, 3)
    omega, origin = np.array([0.0, 0.0, 2.0 * np.pi]), np.array([0.5, 0.5, 0.0])
    for name, key in (("Urel", "U"), ("T", "T"), ("p", "p")):
        va, _ = ff.read_field(os.path.join(a, "0.006", name), m2)
        vb, _ = ff.read_field(os.path.join(b, "0.006", name), m2)
        assert np.array_equal(va.reshape(state[key].shape), state[key]), name      # written at full precision
        assert np.array_equal(va, vb), name                                        # restart = uninterrupted run, bit for bit
    assert np.all(state["T"] == 300.0)
    uabs, _ = ff.read_field(os.path.join(a, "0.006", "Uabs"), m2)
    want = np.cross(omega, C - origin)
    assert np.abs((uabs - state["U"]) - want).max() <= 4e-16 * max(np.abs(want).max(), np.abs(uabs).max())
