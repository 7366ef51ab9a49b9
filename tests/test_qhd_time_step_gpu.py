"""Courant-number time step control of the resident QHDFoam / SRFQHDFoam case (qgd_qhd_case_set_time_control)
[QHDFoam.C L104-106: QHDCourantNo.H L37-57, setDeltaT-QGDQHD.H L41-61].

The rule is checked step by step against numpy (qhd_time_step_ref.py: phiu from the CPU oracle's qhd_fluxes on the device's state before
the step, |Sf| from the mesh, hQGDf restated from the mesh; bars 1e-14 on deltaT and 1e-13 on CoNum, those of
test_adjust_time_step_follows_the_listing in the scalar suite), the step itself against one step of a fresh oracle case created with
that step's deltaT (bar 1e-9 of each field's scale: test_qhd_case.py / test_qhd_implicit.py; the implicit arm exercises the rebuilt
diagonals), the rotating arm through srf_ref.py's superposition at that file's bar.

Where the maximum sits: box(7, 5, 3) has 386 faces (6 x 64 + 2: neither a multiple of the wavefront nor of the 256-thread workgroup);
the reduction's grid is capped at 2048 workgroups = 524 288 lanes, so box(60, 60, 50) with 549 600 faces makes the first 25 312 lanes take
two faces, and the last cell's boundary faces (labels above 524 288) are reached in a lane's second pass only; box(90, 90, 90) with
2 211 300 faces (more than 4 x 524 288) sends the first lanes round the grid-stride loop a second time, where the last cell's faces lie.

Start values: with unequal steps the pressure and the U / T solves start from Lagrange weights handed over by value (QGD_QHD_LAGRANGE,
default 1); they change iteration counts, never the answer beyond the tolerances, and not a bit at a fixed deltaT."""
import ctypes as C

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L, qhdfoam

import srf_ref as R
from oracle import OracleQhdCase
from qhd_time_step_ref import CourantRef
from test_qhd_case import cavity_bcs, initial, options
from test_qhd_implicit import TIGHT
from util import make_mesh, oracle_mesh_of

pytestmark = pytest.mark.gpu

FIELDS = ("U", "T", "p")


def stirred(mesh, amp=5e-2, seed=3):
    U, T, p = initial(mesh)
    U = U + amp * np.random.default_rng(seed).standard_normal(U.shape)
    if mesh.nGeometricD == 2:
        U[:, 2] = 0.0
    return U, T, p


def device_case(dev, mesh, opt, fields, bcs=cavity_bcs):
    c = qhdfoam.QHDFoamCase(dev, opt)
    bcs(c, mesh)
    c.set_fields(*fields)
    return c


def oracle_step(om, mesh, opt, dt, state, bcs=cavity_bcs):
    """one step of a fresh oracle case whose deltaT is dt, from the state (U, T, p)"""
    oc = OracleQhdCase(om, R.copy_options(opt, deltaT=dt))
    bcs(oc, mesh)
    oc.set_fields(*state)
    oc.step(1)
    out = {f: oc.field(f) for f in FIELDS}
    oc.close()
    return out


def follow_the_rule(case, ref, dt0, steps, max_co, max_dt, c_tau, replay=None):
    """`steps` single steps: CoNum and deltaT against the numpy rule, time against the sum; replay(dt, state) -> the fields one step on"""
    dt, dts = dt0, []
    for step in range(steps):
        state = tuple(case.field(f) for f in FIELDS)
        max_ubyh = ref.max_unf_by_h(case)
        co, dt_new = ref.rule(dt, max_ubyh, max_co, max_dt, c_tau)
        case.step(1)
        ti = case.time_info()
        print("step", step, "deltaT", ti["deltaT"], dt_new, "CoNum", ti["CoNum"], co, "max", ti["maxUnfByH"], max_ubyh)
        assert abs(ti["deltaT"] - dt_new) <= 1e-14 * dt_new
        assert abs(ti["CoNum"] - co) <= 1e-13 * co
        assert ti["adjustTimeStep"] and ti["steps"] == step + 1 and case.info()["deltaT"] == ti["deltaT"]
        if replay is not None:
            want = replay(ti["deltaT"], state)
            for f, w in want.items():
                err = np.abs(case.field(f) - w).max() / max(np.abs(w).max(), 1e-300)
                print("   ", f, err)
                assert err <= 1e-9, (step, f, err)
        dt = ti["deltaT"]
        dts.append(dt)
    assert abs(case.time_info()["time"] - sum(dts)) <= 1e-13 * sum(dts) and case.info()["time"] == case.time_info()["time"]
    return dts


ARMS = [("box654_jitter", "GaussVolPoint", 0), ("plane2d_jitter", "leastSquares", 1), ("tet433", "GaussVolPoint", 0)]


@pytest.mark.parametrize("dt0", [1e-2, 1e-4], ids=["too-large", "too-small"])
@pytest.mark.parametrize("kind,stencil,implicit", ARMS)
def test_time_step_follows_the_listing_and_each_step_the_oracle(kind, stencil, implicit, dt0):
    mesh = make_mesh(kind)
    om = oracle_mesh_of(mesh)
    opt = options(stencil, deltaT=dt0, pTol=1e-13, mu=2e-2 if implicit else 1e-2, **(TIGHT if implicit else {}))
    fields = stirred(mesh)
    dev = q.Device(mesh)
    c = device_case(dev, mesh, opt, fields)
    ref = CourantRef(mesh, om, stencil, opt.rho0, c.field("tauQGDf"))
    hf = c.field("hQGDf")
    assert (np.abs(hf[ref.live] - ref.h[ref.live]) <= 1e-14 * ref.h[ref.live]).all()      # face by face
    assert c.time_info()["minTau"] == ref.min_tau and c.time_info()["CoNum"] == 0.0
    # the Courant number of the start state at deltaT = 1e-3 is maxCo: 1e-2 is an order of magnitude too large for it, 1e-4 too small
    max_co, max_dt, c_tau = 1e-3 * ref.max_unf_by_h(c), 1.0, 0.75
    c.set_time_control(True, max_co, max_dt, c_tau)
    dts = follow_the_rule(c, ref, dt0, 12, max_co, max_dt, c_tau, replay=lambda dt, state: oracle_step(om, mesh, opt, dt, state))
    assert (dts[-1] < 0.5 * dt0) if dt0 > 1e-3 else (dts[-1] > 2.0 * dt0)      # the control did act, in the direction the start value asks for
    assert len(set(dts)) > 6                                                   # ... and kept moving deltaT
    if implicit:
        ii = c.implicit_info()
        assert ii["implicit"] and ii["unconverged_steps"] == 0 and ii["stalled_steps"] == 0, ii
    c.close(); dev.close(); om.close()


@pytest.mark.parametrize("bound", ["cTau-minTau", "maxDeltaT"])
def test_the_other_two_bounds_bind(bound):
    mesh = make_mesh("box654_jitter")
    om = oracle_mesh_of(mesh)
    dt0 = 1e-4
    if bound == "cTau-minTau":
        opt, max_dt, c_tau = options(deltaT=dt0, pTol=1e-13, tauModel="constTau", Tau=2e-4), 1.0, 0.75
        want = 0.75 * 2e-4
    else:
        opt, max_dt, c_tau = options(deltaT=dt0, pTol=1e-13), 1.3e-4, 0.75
        want = 1.3e-4
    dev = q.Device(mesh)
    c = device_case(dev, mesh, opt, stirred(mesh))
    ref = CourantRef(mesh, om, "GaussVolPoint", opt.rho0, c.field("tauQGDf"))
    assert (c_tau * ref.min_tau < max_dt) == (bound == "cTau-minTau")
    c.set_time_control(True, 1e6, max_dt, c_tau)
    dts = follow_the_rule(c, ref, dt0, 6, 1e6, max_dt, c_tau, replay=lambda dt, state: oracle_step(om, mesh, opt, dt, state))
    assert dts[0] == 1.2 * dt0 and dts[-1] == dts[-2] == want, dts
    c.close(); dev.close(); om.close()


def one_cell_case(mesh, stencil, cell, wall_face=None):
    """a case whose velocity vanishes except in `cell`; wall_face: one face of patch 0 carries a large fixedValue velocity"""
    n = mesh.nCells
    U = np.zeros((n, 3))
    U[cell] = (0.3, -0.2, 0.0 if mesh.nGeometricD == 2 else 0.25)
    dev = q.Device(mesh)
    c = qhdfoam.QHDFoamCase(dev, options(stencil, deltaT=1e-4, pTol=1e-10))
    cavity_bcs(c, mesh)
    if wall_face is not None:
        vals = np.zeros((int(mesh.array("patchSize")[0]), 3))
        vals[wall_face] = (7.0, 1.0, 0.0)
        c.set_bc_values(0, vals)
    c.set_fields(U, np.full(n, 300.0), np.zeros(n))
    return dev, c


@pytest.mark.parametrize("where", ["first-cell", "last-cell", "wall-face", "beside-empty-2d", "last-cell-second-pass", "last-cell-second-round"])
def test_where_the_maximum_sits(where):
    if where == "beside-empty-2d":
        mesh, stencil = make_mesh("plane2d_jitter"), "leastSquares"
    elif where == "last-cell-second-pass":
        mesh, stencil = q.PolyMesh.box(60, 60, 50), "reduced"
        assert mesh.nFaces == 549600 and mesh.nFaces > 2048 * 256
    elif where == "last-cell-second-round":
        mesh, stencil = q.PolyMesh.box(90, 90, 90), "reduced"
        assert mesh.nFaces == 2211300 and mesh.nFaces > 4 * 2048 * 256
    else:
        mesh, stencil = q.PolyMesh.box(7, 5, 3).jitter(0.1, seed=12), "GaussVolPoint"
        assert mesh.nFaces == 386
    own, nei, nif = mesh.array("owner"), mesh.array("neighbour"), mesh.nInternalFaces
    cell = {"first-cell": 0, "wall-face": 0, "beside-empty-2d": 17}.get(where, mesh.nCells - 1)
    wall_face = None
    if where == "wall-face":      # a face of patch 0 (xMin) that belongs to another cell than the one that moves
        b0 = int(mesh.array("patchStart")[0])
        wall_face = int(mesh.array("patchSize")[0]) - 1
        assert own[b0 + wall_face] != cell
    dev, c = one_cell_case(mesh, stencil, cell, wall_face)
    om = oracle_mesh_of(mesh)
    ref = CourantRef(mesh, om, stencil, 1.0, c.field("tauQGDf"))
    cof = ref.per_face(c.field("U"), c.field("U.boundary"), c.field("T"), c.field("T.boundary"))
    f_max = int(np.argmax(cof))
    of_cell = set(np.nonzero(own == cell)[0]) | set(np.nonzero(nei[:nif] == cell)[0])
    if where == "wall-face":
        assert f_max == b0 + wall_face
    else:
        assert f_max in of_cell
    if where == "last-cell-second-pass":
        assert max(of_cell) >= 2048 * 256       # reached in a lane's second pass only
    if where == "last-cell-second-round":
        assert f_max >= 4 * 2048 * 256          # reached in the second round of the grid-stride loop only
    if where == "beside-empty-2d":
        empty = ~ref.live
        assert empty.sum() == 2 * mesh.nCells and (c.field("tauQGDf")[empty] == 0.0).all()     # a reduction over ALL faces would give min tau = 0
        assert c.time_info()["minTau"] == ref.min_tau > 0
    dt0 = c.info()["deltaT"]
    c.set_time_control(True, 1e6, 1.0, 0.75)
    c.step(1)
    ti = c.time_info()
    print(where, "face", f_max, "of", mesh.nFaces, "max", ti["maxUnfByH"], cof[f_max])
    assert cof[f_max] > 0 and abs(ti["maxUnfByH"] - cof[f_max]) <= 1e-13 * cof[f_max]
    assert abs(ti["CoNum"] - dt0 * cof[f_max]) <= 1e-13 * dt0 * cof[f_max]
    # and with the control off the same number is reported, from the fluxes of the last step
    c.set_time_control(False)
    again = ref.max_unf_by_h(c)
    c.step(1)
    t2 = c.time_info()
    assert not t2["adjustTimeStep"] and t2["deltaT"] == dt0 and t2["steps"] == 2
    assert again > 0 and abs(t2["maxUnfByH"] - again) <= 1e-13 * again and abs(t2["CoNum"] - dt0 * again) <= 1e-13 * dt0 * again
    c.close(); dev.close(); om.close()


@pytest.mark.parametrize("implicit", [0, 1])
def test_nothing_else_moves(implicit):
    """never asked, asked with adjust = 0, and adjust = 1 under bounds that return the options' deltaT exactly: the same bits"""
    mesh = make_mesh("box654_jitter")
    dev = q.Device(mesh)
    dt = 1e-3
    opt = options(deltaT=dt, mu=2e-2 if implicit else 1e-2, **(TIGHT if implicit else {}))
    res = []
    for arm in ("never", "off", "on"):
        c = device_case(dev, mesh, opt, stirred(mesh))
        if arm == "off":
            c.set_time_control(False)
        elif arm == "on":
            assert 0.75 * c.time_info()["minTau"] > dt
            c.set_time_control(True, 1e30, dt, 0.75)      # deltaTFact = 1.2, min(1.2 deltaT, min(deltaT, cTau min tau)) = deltaT
        for _ in range(5):
            c.step(1)
            assert c.time_info()["deltaT"] == dt and c.info()["deltaT"] == dt
        assert c.time_info()["adjustTimeStep"] == (arm == "on")
        res.append(({f: c.field(f) for f in FIELDS}, c.info()["time"]))
        c.close()
    assert res[0][1] == res[1][1] == res[2][1] > 0
    for f in FIELDS:
        assert np.isfinite(res[0][0][f]).all() and np.abs(res[0][0][f]).max() > 0
        assert np.array_equal(res[0][0][f], res[1][0][f]) and np.array_equal(res[0][0][f], res[2][0][f]), f
    dev.close()


@pytest.mark.parametrize("implicit", [0, 1])
def test_control_switched_off_returns_to_the_options_step(implicit):
    """adjusted steps, then adjust = 0: deltaT is the options' again, and the step after it is the oracle's step at that deltaT (under
    implicitDiffusion: the diagonals were rebuilt for it)"""
    mesh = make_mesh("box654_jitter")
    om = oracle_mesh_of(mesh)
    dt = 1e-3
    opt = options(deltaT=dt, pTol=1e-13, mu=2e-2 if implicit else 1e-2, **(TIGHT if implicit else {}))
    dev = q.Device(mesh)
    c = device_case(dev, mesh, opt, stirred(mesh))
    c.set_time_control(True, 1e6, 4e-4, 0.75)
    c.step(3)
    assert c.time_info()["deltaT"] == 4e-4
    c.set_time_control(False)
    assert c.info()["deltaT"] == dt
    state = tuple(c.field(f) for f in FIELDS)
    c.step(1)
    want = oracle_step(om, mesh, opt, dt, state)
    for f in FIELDS:
        assert np.abs(c.field(f) - want[f]).max() <= 1e-9 * np.abs(want[f]).max(), f
    assert abs(c.info()["time"] - (3 * 4e-4 + dt)) <= 1e-13
    c.close(); dev.close(); om.close()


@pytest.mark.parametrize("implicit", [0, 1])
def test_srf_zero_omega_with_the_control_is_the_plain_case_bit_for_bit(implicit):
    mesh = make_mesh("box654_jitter")
    dev = q.Device(mesh)
    opt = options(deltaT=1e-2, mu=2e-2 if implicit else 1e-2, **(TIGHT if implicit else {}))
    res = []
    for srf in (False, True):
        c = qhdfoam.QHDFoamCase(dev, opt)
        if srf:
            c.set_srf((0.0, 0.0, 0.0), solve_T=True)
        cavity_bcs(c, mesh)
        c.set_fields(*stirred(mesh))
        c.set_time_control(True, 1e-3, 1.0, 0.75)
        dts = []
        for _ in range(8):
            c.step(1)
            dts.append(c.time_info()["deltaT"])
        res.append(({f: c.field(f) for f in FIELDS}, dts))
        c.close()
    assert res[0][1] == res[1][1] and len(set(res[0][1])) > 4 and res[0][1][-1] < 5e-3
    for f in FIELDS:
        assert np.abs(res[0][0][f]).max() > 0 and np.array_equal(res[0][0][f], res[1][0][f]), f
    dev.close()


@pytest.mark.parametrize("implicit", [0, 1])
def test_rotating_case_follows_the_rule_and_the_superposed_oracle(implicit):
    mesh = make_mesh("tet433")
    om = oracle_mesh_of(mesh)
    dt0 = 1e-4
    opt = R.options("GaussVolPoint", implicit, deltaT=dt0)
    bcs = R.patch_bcs(mesh)
    dev = q.Device(mesh)
    c = qhdfoam.QHDFoamCase(dev, opt)
    c.set_srf(R.OMEGA_3D)
    R.apply_bcs(c, bcs)
    c.set_fields(*R.initial(mesh))
    assert c.srf_info()["rotating"] and c.srf_info()["frozenT"]
    ref = CourantRef(mesh, om, "GaussVolPoint", opt.rho0, c.field("tauQGDf"))
    max_co, max_dt, c_tau = 1e-3 * ref.max_unf_by_h(c), 1.0, 0.75
    c.set_time_control(True, max_co, max_dt, c_tau)

    def replay(dt, state):
        sr = R.SrfReference(mesh, R.copy_options(opt, deltaT=dt), bcs, R.OMEGA_3D)
        want, _ = sr.step(*state)
        sr.close()
        return {f: want[f] for f in ("U", "p")}     # (T is frozen: never written)

    T0 = c.field("T")
    dts = follow_the_rule(c, ref, dt0, 6, max_co, max_dt, c_tau, replay=replay)
    assert dts[-1] > 2.0 * dt0 and np.array_equal(c.field("T"), T0)
    if implicit:
        ii = c.implicit_info()
        assert ii["unconverged_steps"] == 0 and ii["stalled_steps"] == 0 and ii["solves"]["T"]["iterations"] == 0, ii
    c.close(); dev.close(); om.close()


def test_monitor_reports_the_step_in_force():
    mesh = make_mesh("box654_jitter")
    dev = q.Device(mesh)
    c = device_case(dev, mesh, options(deltaT=1e-2), stirred(mesh))
    mon = c.monitor()
    c.set_time_control(True, 1e-3, 1.0, 0.75)
    seen = []
    for _ in range(3):
        c.step(1)
        mon.sample()
        s = mon.read()
        assert s["deltaT"] == c.time_info()["deltaT"] != 1e-2, s["deltaT"]
        seen.append(s["deltaT"])
    assert len(set(seen)) == 3
    c.set_time_control(False)
    mon.sample()
    assert mon.read()["deltaT"] == 1e-2
    mon.close(); c.close(); dev.close()


def test_refusals():
    mesh = make_mesh("box654")
    dev = q.Device(mesh)
    c = device_case(dev, mesh, options(), initial(mesh))
    f = L.lib.qgd_qhd_case_set_time_control
    nan, inf = float("nan"), float("inf")
    for bad in ((0.0, 1.0, 0.75), (-1.0, 1.0, 0.75), (nan, 1.0, 0.75), (inf, 1.0, 0.75), (1.0, 0.0, 0.75), (1.0, nan, 0.75), (1.0, inf, 0.75),
                (1.0, 1.0, 0.0), (1.0, 1.0, -0.75), (1.0, 1.0, nan), (1.0, 1.0, inf)):
        for adjust in (0, 1):
            assert f(c._h, adjust, *bad) == L.ERR_INVALID, bad
    assert f(None, 1, 1.0, 1.0, 0.75) == L.ERR_INVALID
    assert L.lib.qgd_qhd_case_time_info(c._h, None) == L.ERR_INVALID and L.lib.qgd_qhd_case_time_info(None, (C.c_double * 8)()) == L.ERR_INVALID
    assert not c.time_info()["adjustTimeStep"]          # none of them took effect
    assert f(c._h, 1, 1.0, 1e300, 0.75) == L.QGD_OK      # the listing's defaults (maxDeltaT GREAT)
    assert L.lib.qgd_qhd_case_step_phase(c._h, 0) == L.ERR_NOT_IMPLEMENTED
    assert "qgd_qhd_case_set_time_control" in L.lib.qgd_last_error().decode() or "adjustTimeStep" in L.lib.qgd_last_error().decode()
    assert L.lib.qgd_qhd_case_step_sharded(c._h, None, None, 0, 1) == L.ERR_NOT_IMPLEMENTED
    assert f(c._h, 0, 1.0, 1.0, 0.75) == L.QGD_OK
    c.step(1)                                                        # the fixed step again
    assert c.time_info()["deltaT"] == c.options.deltaT
    c.close(); dev.close()
    # a sharded device
    sh = q.PolyMesh.box(3, 2, 4).shard(2, 0)
    d2 = q.Device(sh)
    c2 = qhdfoam.QHDFoamCase(d2, options())
    for adjust in (0, 1):
        assert f(c2._h, adjust, 1.0, 1.0, 0.75) == L.ERR_NOT_IMPLEMENTED
        assert "qgd_qhd_case_set_time_control" in L.lib.qgd_last_error().decode() and "sharded" in L.lib.qgd_last_error().decode()
    c2.close(); d2.close()


def test_fused_advance_takes_the_adjusted_step(monkeypatch):
    """QGD_QHD_FUSED=1: the block-fused U and T equations take deltaT by value -- the rule and every step's oracle replay as above"""
    monkeypatch.setenv("QGD_QHD_FUSED", "1")
    mesh = q.PolyMesh.box(12, 10, 8).jitter(0.1, seed=6)
    om = oracle_mesh_of(mesh)
    dt0 = 1e-4
    opt = options(deltaT=dt0, pTol=1e-13)
    dev = q.Device(mesh, fused_tables="any")
    c = device_case(dev, mesh, opt, stirred(mesh))
    assert c.fused_info()["fusedAdvance"]
    ref = CourantRef(mesh, om, "GaussVolPoint", opt.rho0, c.field("tauQGDf"))
    max_co, max_dt, c_tau = 1e-3 * ref.max_unf_by_h(c), 1.0, 0.75
    c.set_time_control(True, max_co, max_dt, c_tau)
    dts = follow_the_rule(c, ref, dt0, 6, max_co, max_dt, c_tau, replay=lambda dt, state: oracle_step(om, mesh, opt, dt, state))
    assert dts[-1] > 2.0 * dt0
    c.close(); dev.close(); om.close()


@pytest.mark.parametrize("implicit", [0, 1])
def test_start_weights_move_iteration_counts_only(implicit, monkeypatch):
    """deltaT alternating between two values: the Lagrange start values (default) and the equal-step ones (QGD_QHD_LAGRANGE=0) lead to the
    same fields to the solver tolerances -- bound: 1e-9 of each field's scale, the bar of device against oracle -- and, at a fixed deltaT,
    to the same bits"""
    mesh = make_mesh("box654_jitter")
    dev = q.Device(mesh)
    dt = 1e-3
    opt = options(deltaT=dt, pTol=1e-13, mu=2e-2 if implicit else 1e-2, **(TIGHT if implicit else {}))
    res = {}
    for moving in (True, False):
        for lagrange in ("1", "0"):
            monkeypatch.setenv("QGD_QHD_LAGRANGE", lagrange)
            c = device_case(dev, mesh, opt, stirred(mesh))
            its = []
            for step in range(10):
                if moving:
                    c.set_time_control(True, 1e30, dt * (1.0 if step % 2 else 0.85), 0.75)      # (up by 1.18: inside the rule's 1.2)
                c.step(1)
                its.append(c.info()["pIterations"])
            if moving:
                assert abs(c.info()["time"] - 5 * 1.85 * dt) <= 1e-12
            res[moving, lagrange] = ({f: c.field(f) for f in FIELDS}, its)
            if implicit:
                ii = c.implicit_info()
                assert ii["unconverged_steps"] == 0 and ii["stalled_steps"] == 0, ii
            c.close()
    print("pressure iterations, deltaT moving: Lagrange", res[True, "1"][1], "equal-step", res[True, "0"][1])
    for f in FIELDS:
        a, b = res[True, "1"][0][f], res[True, "0"][0][f]
        assert np.abs(a).max() > 0 and np.abs(a - b).max() <= 1e-9 * np.abs(b).max(), f
        assert np.array_equal(res[False, "1"][0][f], res[False, "0"][0][f]), f
    assert res[False, "1"][1] == res[False, "0"][1]
    # the two start values are not the same thing: somewhere the fields differ in their last bits, or the counts do
    assert res[True, "1"][1] != res[True, "0"][1] or any(not np.array_equal(res[True, "1"][0][f], res[True, "0"][0][f]) for f in FIELDS)
    dev.close()
