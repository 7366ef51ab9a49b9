"""The implicitDiffusion branch of QGDFoam (the reference's default, QGDThermo.C L70-82): tauMC / phiTauMC
[updateFluxes.H L107-111], the implicit U solve and phiSigmaDotU [QGDUEqn.H L54-75], the implicit e solve [QGDEEqn.H L53-64].

CPU (oracle): with no viscosity at all (mu = 0, ScQGD = 0) the implicit branch is the explicit one with the consistent
energy update, to rounding; a shear wave decays at the analytic rate in both branches (the two discretise the same
operator: laplacian + div(mu dev2(T(grad U))) against the face-gradient form); vector components along empty directions are
not solved (validComponents).  GPU: device against oracle after N steps, several meshes / stencils / patch kinds."""
import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L

import cases
from oracle import OracleCase
from test_partition import mixed_bcs
from util import make_mesh, oracle_mesh_of

G, E = L.PATCH_GENERIC, L.PATCH_EMPTY


def run_oracle(mesh, bc_fn, fields, steps, **opt):
    oc = OracleCase(oracle_mesh_of(mesh), q.default_options(**opt))
    if bc_fn:
        bc_fn(oc)
    oc.set_fields(*fields)
    oc.step(steps)
    return {f: oc.field(f) for f in ("rho", "U", "p", "e")}


def test_without_viscosity_the_implicit_branch_is_the_consistent_explicit_one():
    mesh = make_mesh("box654_jitter")
    fields = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    base = dict(stencil="GaussVolPoint", deltaT=1e-3, mu=0.0, ScQGD=0.0, implicitTol=1e-15)
    ex = run_oracle(mesh, mixed_bcs, fields, 10, implicitDiffusion=0, consistentEnergy=1, **base)
    im = run_oracle(mesh, mixed_bcs, fields, 10, implicitDiffusion=1, **base)
    for f in ex:
        assert np.abs(ex[f] - im[f]).max() <= 1e-13 * np.abs(ex[f]).max(), f


@pytest.mark.parametrize("implicit", [0, 1])
def test_shear_wave_decays_at_the_analytic_rate(implicit):
    """U_y = A sin(pi x) between two walls, rho = p = 1, no regularisation: rho dU_y/dt = mu d2U_y/dx2"""
    rates = []
    for n in (20, 40):
        mesh = q.PolyMesh.box(n, 4, 1, hi=(1.0, 0.2, 0.05), patch_types=[G, G, G, G, E, E])
        x = mesh.array("C").reshape(-1, 3)[:, 0]
        mu, dt = 0.05, 2e-4 * (20 / n) ** 2
        oc = OracleCase(oracle_mesh_of(mesh), q.default_options(stencil="reduced", deltaT=dt, mu=mu, alphaQGD=1e-12, ScQGD=0.0,
                                                                implicitDiffusion=implicit, implicitTol=1e-14, consistentEnergy=1))
        for patch in (0, 1):
            oc.set_bc(patch, U=("fixedValue", (0.0, 0.0, 0.0)))
        for patch in (4, 5):
            oc.set_bc(patch, U=("none", None), T=("none", None), p=("none", None))
        U = np.zeros((mesh.nCells, 3))
        U[:, 1] = 1e-3 * np.sin(np.pi * x)
        oc.set_fields(U, np.ones(mesh.nCells), np.ones(mesh.nCells))
        oc.step(int(round(0.2 / dt)))
        rho = oc.field("rho")[0]
        i = n // 2
        rates.append(abs(oc.field("U")[i, 1] / U[i, 1] - np.exp(-mu / rho * np.pi ** 2 * 0.2)))
    assert rates[0] < 2e-4 and rates[1] < rates[0] / 3      # second order in h


def test_components_along_empty_directions_are_not_solved():
    mesh = q.PolyMesh.box(20, 1, 1, hi=(1.0, 0.05, 0.05), patch_types=[G, G, E, E, E, E])
    x = mesh.array("C").reshape(-1, 3)[:, 0]
    oc = OracleCase(oracle_mesh_of(mesh), q.default_options(stencil="reduced", deltaT=2e-4, mu=0.05, alphaQGD=1e-12, ScQGD=0.0,
                                                            implicitDiffusion=1, implicitTol=1e-14))
    for patch in (0, 1):
        oc.set_bc(patch, U=("fixedValue", (0.0, 0.0, 0.0)))
    for patch in (2, 3, 4, 5):
        oc.set_bc(patch, U=("none", None), T=("none", None), p=("none", None))
    U = np.zeros((mesh.nCells, 3))
    U[:, 1] = 1e-3 * np.sin(np.pi * x)
    oc.set_fields(U, np.ones(mesh.nCells), np.ones(mesh.nCells))
    oc.step(200)
    assert np.abs(oc.field("U")[:, 1] / U[:, 1] - 1.0).max() < 1e-8   # fvMatrix<vector>::solve skips invalid components (L0)


GPU_CASES = [("box654_jitter", "GaussVolPoint", mixed_bcs), ("box654_tri", "GaussVolPoint", mixed_bcs), ("box654", "reduced", None),
             ("step2d", "leastSquares", cases.forward_step_bcs), ("step2d", "GaussVolPoint", cases.forward_step_bcs),
             ("plane2d_jitter", "leastSquares", None)]


# tetrahedra and prisms (tests/unstructured.py): vertices of 24 / 12 cells -- the vertex walk of the IMPL instantiation beyond its eight register
# slots -- and matrix rows of four and five off-diagonal entries under the Chebyshev iteration's eight-at-a-time row walk
UNSTRUCTURED_CASES = [("tet433", "GaussVolPoint", mixed_bcs), ("prism543", "GaussVolPoint", mixed_bcs), ("tet866", "GaussVolPoint", mixed_bcs)]
# one level of 2:1 refinement: matrix rows of 6 to 24 off-diagonal entries in one slice of the ELL matrix, three passes of the cell kernels' walks
UNSTRUCTURED_CASES += [("ref533", "GaussVolPoint", mixed_bcs)]
DELTA_T = {"tet433": 2e-4, "prism543": 2e-4, "tet866": 2e-4, "ref533": 2e-4}


def _implicit_arms(kind, stencil):
    """3-D GaussVolPoint cases run twice: through the block-fused assembly of the U systems (fusedFaceCellKernel<..., IMPL>: vertex values, QGD
    fluxes, tauMC and the rows of the three systems in one launch) and through the separate kernels; everything else the second way only"""
    mesh = make_mesh(kind)
    three_d = mesh.nGeometricD == 3
    mesh.close()
    return ["fused", "kernels"] if (stencil == "GaussVolPoint" and three_d) else ["kernels"]


IMPLICIT_ARMS = [c + (a,) for c in GPU_CASES + UNSTRUCTURED_CASES for a in _implicit_arms(c[0], c[1])]


def test_the_implicit_matrix_covers_the_block_fused_assembly():
    assert [c[0] for c in IMPLICIT_ARMS if c[3] == "fused"] == ["box654_jitter", "box654_tri", "tet433", "prism543", "tet866", "ref533"]
    assert sum(1 for c in IMPLICIT_ARMS if c[3] == "kernels") == len(GPU_CASES) + len(UNSTRUCTURED_CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,stencil,bc_fn,arm", IMPLICIT_ARMS)
def test_device_implicit_branch_matches_oracle(kind, stencil, bc_fn, arm):
    mesh = make_mesh(kind)
    C = mesh.array("C").reshape(-1, 3)
    if kind == "step2d":
        U = np.zeros((mesh.nCells, 3)); U[:, 0] = 3.0
        fields = (U, 1.0 + 0.05 * np.sin(2.0 * C[:, 0]) * np.cos(3.0 * C[:, 1]), 1.0 + 0.05 * np.cos(1.5 * C[:, 0] + C[:, 1]))
    else:
        fields = cases.box_initial_fields(C)
        if mesh.nGeometricD == 2:
            fields[0][:, 2] = 0.0
    opt = dict(stencil=stencil, deltaT=DELTA_T.get(kind, 5e-4), mu=2e-2, implicitDiffusion=1, implicitTol=1e-14, implicitMaxIter=2000)

    def empty_patches(case):
        for ip, t in enumerate(mesh.array("patchType")):
            if t == E:
                case.set_bc(ip, U=("none", None), T=("none", None), p=("none", None))

    setup = bc_fn if bc_fn else empty_patches
    ref = run_oracle(mesh, setup, fields, 12, **opt)
    dev = q.Device(mesh, fused_tables="any" if arm == "fused" else False)
    gc = q.QGDFoamCase(dev, q.default_options(**opt))
    fi = gc.fused_info()
    assert fi["fusedImplicit"] == (arm == "fused") and not fi["fused"], (arm, fi)    # the arm under test is the path that runs
    setup(gc)
    gc.set_fields(*fields)
    gc.step(12)
    worst = {}
    for f in ref:
        err = np.abs(gc.field(f) - ref[f]).max() / np.abs(ref[f]).max()
        worst[f] = float(err)
        assert err <= 1e-10, (kind, stencil, f, err)
    assert gc.info()["minRho"] > 0
    ii = gc.implicit_info()
    assert ii["unconverged_steps"] == 0, ii
    print(f"implicitDiffusion {kind} {stencil} {arm}: worst {max(worst.values()):.3e}; iterations of the last step "
          f"{ {n: s['iterations'] for n, s in ii['solves'].items()} }")
    # and it is not the explicit branch in disguise
    ex = run_oracle(mesh, setup, fields, 12, **dict(opt, implicitDiffusion=0))
    assert np.abs(ex["U"] - ref["U"]).max() > 1e-6 * np.abs(ref["U"]).max()
    gc.close(); dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,stencil,bc_fn", GPU_CASES)
def test_gradient_of_the_new_velocity_is_reused_by_the_next_step(kind, stencil, bc_fn, monkeypatch):
    """fvc::grad(U) is formed twice per step in the listing (QGDUEqn.H: of the state before the step for tauMC, of the new velocity for
    sigmaDotU).  Unsharded, the first of step n+1 IS the second of step n -- same cell values, same patch values -- and is skipped
    (QGD_IMPL_REUSE_GRADU, default 1).  Bit for bit the same states as with both gradients formed, on every mesh / patch kind of this module,
    also across a re-upload of the fields in mid-run (which invalidates the stored gradient)."""
    mesh = make_mesh(kind)
    C = mesh.array("C").reshape(-1, 3)
    if kind == "step2d":
        U = np.zeros((mesh.nCells, 3)); U[:, 0] = 3.0
        fields = (U, 1.0 + 0.05 * np.sin(2.0 * C[:, 0]) * np.cos(3.0 * C[:, 1]), 1.0 + 0.05 * np.cos(1.5 * C[:, 0] + C[:, 1]))
    else:
        fields = cases.box_initial_fields(C)
        if mesh.nGeometricD == 2:
            fields[0][:, 2] = 0.0
    opt = dict(stencil=stencil, deltaT=5e-4, mu=2e-2, implicitDiffusion=1, implicitTol=1e-12, implicitMaxIter=2000)

    def empty_patches(case):
        for ip, t in enumerate(mesh.array("patchType")):
            if t == E:
                case.set_bc(ip, U=("none", None), T=("none", None), p=("none", None))

    setup = bc_fn if bc_fn else empty_patches
    dev = q.Device(mesh)
    res = {}
    for reuse in ("0", "1"):
        monkeypatch.setenv("QGD_IMPL_REUSE_GRADU", reuse)
        gc = q.QGDFoamCase(dev, q.default_options(**opt))
        setup(gc)
        gc.set_fields(*fields)
        gc.step(5)
        U5, T5, p5 = gc.field("U").copy(), gc.field("T").copy(), gc.field("p").copy()
        gc.set_fields(U5 * 1.01, T5, p5)       # a fresh state: the stored gradient must not survive it
        gc.step(4)
        res[reuse] = {f: gc.field(f).copy() for f in ("rho", "U", "p", "e")}
        gc.close()
    for f in res["0"]:
        assert np.isfinite(res["0"][f]).all() and np.array_equal(res["0"][f], res["1"][f]), (kind, stencil, f, np.abs(res["0"][f] - res["1"][f]).max())
    dev.close()


@pytest.mark.gpu
def test_staged_face_kernel_of_the_implicit_branch_is_the_generic_walk_bit_for_bit(monkeypatch):
    """implFaceTileKernel (the internal faces of a 128-face tile: velocity, muQGD and fvc::grad(U) of its distinct cells out of LDS;
    QGD_IMPL_TILES default 1) against the generic implFaceKernel (QGD_IMPL_TILES=0): the same states after 6 steps, bit for bit, on hexahedra
    with a ragged last tile and row ends beyond the caps, on a jittered mesh with triangles and polygon faces and mixed patch kinds, and on a
    scrambled numbering (most tiles left to the generic kernel)."""
    from test_config5_gpu import c5_mesh
    scr = q.PolyMesh.box(12, 10, 8)
    scr.renumber(np.random.default_rng(5).permutation(scr.nCells).astype(np.int32))
    for tag, mesh, bc_fn in (("hex 37x11x5", q.PolyMesh.box(37, 11, 5), None), ("box654_tri", make_mesh("box654_tri"), mixed_bcs),
                             ("triangles + polygons, Morton order", c5_mesh(16, 8 ** 3, poly=True), None), ("scrambled labels", scr, None)):
        fields = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
        opt = dict(stencil="GaussVolPoint", deltaT=5e-4, mu=2e-2, implicitDiffusion=1, implicitTol=1e-12, implicitMaxIter=2000)
        res = {}
        for tiles in ("0", "1"):
            monkeypatch.setenv("QGD_IMPL_TILES", tiles)
            dev = q.Device(mesh)
            ft = dev.face_tiles()
            gc = q.QGDFoamCase(dev, q.default_options(**opt))
            if bc_fn:
                bc_fn(gc)
            gc.set_fields(*fields)
            gc.step(6)
            res[tiles] = {f: gc.field(f).copy() for f in ("rho", "U", "p", "e")}
            gc.close(); dev.close()
        if not tag.startswith("scrambled"):
            assert ft["facesPerTile"] == 128 and ft["gatherTiles"] < ft["tiles"], (tag, ft)
        for f in res["0"]:
            assert np.isfinite(res["0"][f]).all() and np.array_equal(res["0"][f], res["1"][f]), (tag, f, np.abs(res["0"][f] - res["1"][f]).max())


@pytest.mark.gpu
def test_step_phases_of_the_implicit_branch():
    """phases 0 + 1 are qgd_case_step; the split advance (10 / 11) does not exist for the implicit branch -- it used to run
    the whole advance twice -- and is refused"""
    mesh = make_mesh("box654_jitter")
    fields = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    opt = q.default_options(stencil="GaussVolPoint", deltaT=5e-4, mu=2e-2, implicitDiffusion=1, implicitTol=1e-13, implicitMaxIter=2000)
    dev = q.Device(mesh)
    a, b = q.QGDFoamCase(dev, opt), q.QGDFoamCase(dev, opt)
    for c in (a, b):
        mixed_bcs(c)
        c.set_fields(*fields)
    a.step(5)
    for _ in range(5):
        b.step_phase(0)
        b.step_phase(1)
    b.sync()
    for f in ("rho", "U", "p", "e"):
        assert np.array_equal(a.field(f), b.field(f)), f
    assert a.info()["steps"] == b.info()["steps"] == 5
    for phase in (10, 11):
        with pytest.raises(q.QgdError) as ei:
            b.step_phase(phase)
        assert ei.value.code == L.ERR_NOT_IMPLEMENTED
    a.close(); b.close(); dev.close()


@pytest.mark.gpu
def test_implicit_solves_report_their_convergence():
    mesh = make_mesh("box654_jitter")
    fields = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    dev = q.Device(mesh)
    good = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=5e-4, mu=2e-2, implicitDiffusion=1, implicitTol=1e-12,
                                                implicitMaxIter=500))
    good.set_fields(*fields)
    good.step(3)
    ii = good.implicit_info()
    assert ii["implicit"] and ii["unconverged_steps"] == 0
    for name, s in ii["solves"].items():
        assert 0 < s["iterations"] < 500 and s["final"] < 1e-12 <= s["initial"], (name, s)
    # an iteration limit that cannot be met is counted, step by step, and the step still completes
    starved = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=5e-4, mu=2e-2, implicitDiffusion=1, implicitTol=1e-14,
                                                   implicitMaxIter=1))
    starved.set_fields(*fields)
    starved.step(3)
    ii = starved.implicit_info()
    assert ii["unconverged_steps"] == 3 and all(s["iterations"] == 1 for s in ii["solves"].values())
    assert np.isfinite(starved.field("rho")).all()
    # the explicit branch has nothing to report
    ex = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=5e-4, mu=2e-2))
    ex.set_fields(*fields)
    ex.step(1)
    assert not ex.implicit_info()["implicit"] and ex.implicit_info()["unconverged_steps"] == 0
    good.close(); starved.close(); ex.close(); dev.close()


@pytest.mark.gpu
def test_conjugate_gradient_solver_is_still_selectable(monkeypatch):
    """round 4's default for the U and e systems is the Chebyshev iteration (no dot products: one kernel + one fold per iteration);
    QGD_IMPL_SOLVER=pcg keeps round 3's Jacobi-preconditioned conjugate gradients.  Same answer to the solver tolerance, and an
    unknown word is refused"""
    mesh = make_mesh("box654_jitter")
    fields = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    opt = dict(stencil="GaussVolPoint", deltaT=5e-4, mu=2e-2, implicitDiffusion=1, implicitTol=1e-14, implicitMaxIter=2000)
    ref = run_oracle(mesh, mixed_bcs, fields, 8, **opt)
    dev = q.Device(mesh)
    its = {}
    for solver in ("cheb", "pcg"):
        monkeypatch.setenv("QGD_IMPL_SOLVER", solver)
        gc = q.QGDFoamCase(dev, q.default_options(**opt))
        mixed_bcs(gc)
        gc.set_fields(*fields)
        gc.step(8)
        for f in ref:
            err = np.abs(gc.field(f) - ref[f]).max() / np.abs(ref[f]).max()
            assert err <= 1e-10, (solver, f, err)
        ii = gc.implicit_info()
        assert ii["unconverged_steps"] == 0
        its[solver] = max(s["iterations"] for s in ii["solves"].values())
        gc.close()
    assert 0 < its["cheb"] <= 2 * its["pcg"] + 4, its       # the Chebyshev bound is the conjugate-gradient bound
    monkeypatch.setenv("QGD_IMPL_SOLVER", "sor")
    with pytest.raises(q.QgdError):
        q.QGDFoamCase(dev, q.default_options(**opt))
    dev.close()


@pytest.mark.gpu
def test_chebyshev_solver_on_a_weakly_dominant_system():
    """a viscosity large enough that the laplacian carries most of the diagonal (Gershgorin radius of D^-1 A around 0.9 instead of the 0.1
    of the other cases): the Chebyshev interval is wide, the iteration count goes up, the answer stays the oracle's"""
    mesh = make_mesh("box654_jitter")
    fields = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    opt = dict(stencil="GaussVolPoint", deltaT=2e-3, mu=30.0, implicitDiffusion=1, implicitTol=1e-13, implicitMaxIter=3000)   # nu deltaT / h^2 ~ 1
    ref = run_oracle(mesh, mixed_bcs, fields, 6, **opt)
    dev = q.Device(mesh)
    gc = q.QGDFoamCase(dev, q.default_options(**opt))
    mixed_bcs(gc)
    gc.set_fields(*fields)
    gc.step(6)
    for f in ref:
        err = np.abs(gc.field(f) - ref[f]).max() / np.abs(ref[f]).max()
        assert err <= 1e-10, (f, err)
    ii = gc.implicit_info()
    its = max(s["iterations"] for s in ii["solves"].values())
    assert ii["unconverged_steps"] == 0 and 20 < its < 400, ii
    # implicitTol = 1e-13 lies below the rounding floor of the true residual here: the solves end at the floor (done = 4).  That is no
    # failure of the iteration, but it is not "solved to implicitTol" either, and the count says so (OpenFOAM would have run on to maxIter)
    worst = max(s["final"] for s in ii["solves"].values())
    if worst >= 1e-13:
        assert ii["stalled_steps"] > 0, ii
    assert 0 <= ii["stalled_steps"] <= 6, ii
    gc.close(); dev.close()


@pytest.mark.gpu
def test_block_fused_assembly_of_the_u_systems_is_the_separate_kernels_to_rounding():
    """fusedFaceCellKernel<..., IMPL> against pointInterpRecKernel + faceFluxGvp3TileKernel + implFaceTileKernel + implCellUKernel: the same
    inlined expressions (qgd_implicit_dev.hpp; the implicit ones compiled without contraction), the same summation orders -- states, phiTauMC
    and phiSigmaDotU agree TO ROUNDING after several steps (<= 1e-13 of each field's scale, same iteration counts; measured: 1e-16 .. 1e-15 --
    hipcc contracts the multiply-adds of the QGD flux algebra per template instantiation, and this instantiation is not the explicit step's,
    which is bit-identical to the face kernel), on hexahedra (several blocks), a jittered mesh with triangles and polygons in Morton order,
    walls of every kind, upwind fluxes; cases the fused assembly does not serve (shards, Courant-number control, other stencils) say so and
    run the separate kernels"""
    from test_config5_gpu import c5_mesh
    from test_case_parity_gpu import mixed_box_bcs

    def run(mesh, fused, bc_fn, steps, **opt):
        dev = q.Device(mesh, fused_tables="any" if fused else False)
        gc = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", implicitDiffusion=1, **opt))
        assert gc.fused_info()["fusedImplicit"] == fused
        if bc_fn:
            bc_fn(gc)
        gc.set_fields(*cases.box_initial_fields(mesh.array("C").reshape(-1, 3)))
        gc.step(steps)
        out = {n: gc.field(n).copy() for n in ("rho", "U", "p", "e", "rhoE", "phiTauMC", "phiSigmaDotU", "U.boundary", "p.boundary")}
        info = gc.implicit_info()
        gc.close(); dev.close()
        return out, info

    jit = q.PolyMesh.box(14, 9, 6).jitter(0.1, seed=11)
    for tag, mesh, bc_fn, opt in (("hex 20^3", q.PolyMesh.box(20, 20, 20), None, dict(deltaT=2e-3, mu=1e-2)),
                                  ("hex 37x11x5 + walls", q.PolyMesh.box(37, 11, 5), mixed_box_bcs, dict(deltaT=1e-3, mu=2e-2)),
                                  ("jitter + walls", jit, mixed_box_bcs, dict(deltaT=5e-4, mu=2e-2)),
                                  ("triangles + polygons, Morton order", c5_mesh(16, 8 ** 3, poly=True), None, dict(deltaT=1e-3, mu=1e-2)),
                                  ("upwind fluxes", q.PolyMesh.box(12, 10, 8), mixed_box_bcs, dict(deltaT=1e-3, mu=1e-2, fluxSchemeU=1, fluxSchemeH=1))):
        a, ia = run(mesh, False, bc_fn, 6, **opt)
        b, ib = run(mesh, True, bc_fn, 6, **opt)
        bad = {k: (float(np.abs(a[k] - b[k]).max()), int((a[k] != b[k]).sum())) for k in a
               if not (np.isfinite(b[k]).all() and np.abs(a[k] - b[k]).max() <= 1e-13 * max(np.abs(a[k]).max(), 1e-300))}
        assert not bad, (tag, bad)
        assert ia["solves"] == ib["solves"], (tag, ia, ib)
    # not served: a shard, Courant-number control, another stencil
    dev = q.Device(q.PolyMesh.box(12, 10, 8), fused_tables="any")
    for opt in (dict(adjustTimeStep=1, maxCo=0.2), dict(stencil="reduced")):
        gc = q.QGDFoamCase(dev, q.default_options(**dict(dict(stencil="GaussVolPoint", deltaT=1e-3, mu=1e-2, implicitDiffusion=1), **opt)))
        assert not gc.fused_info()["fusedImplicit"], opt
        gc.close()
    dev.close()
    sh = q.PolyMesh.box(24, 12, 12).shard(2, 0)
    dev = q.Device(sh, fused_tables="any")
    gc = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", deltaT=1e-3, mu=1e-2, implicitDiffusion=1))
    assert not gc.fused_info()["fusedImplicit"]
    gc.close(); dev.close()
