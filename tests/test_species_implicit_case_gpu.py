"""GPU: species mass fractions of a resident QGDFoam case on the implicitDiffusion branch [QGDYEqn.H L47-66] (qgd_species_implicit.hip: one
batched solve per register batch of species) against the host replay of tests/species_implicit_ref.py.

Bar: util.rel_err <= 1e-10, the bar tests/test_implicit_diffusion.py holds the device's implicit branch to against the oracle (two
different iterative solvers meet at their common tolerance, 1e-14 here, not at rounding); the error against the 1e-12 small-mesh bar is
printed next to it."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L

from oracle import OracleCase
from species_implicit_ref import SpeciesImplicitReplay
from test_species_case import flow_bcs, flow_fields, smooth_composition
from test_species_case_gpu import MESHES, front_composition, inlet_bcs, refusal
from util import assert_path, make_mesh, oracle_mesh_of, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-10
SOLVER = dict(implicitTol=1e-14, implicitMaxIter=2000)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_separate_kernels(case, tag=None):
    """a case with species assembles the U systems with the separate implicit kernels, not block-fused"""
    assert_path(case, "kernels", tag)
    assert not case.fused_info()["fusedImplicit"], (tag, case.fused_info())


def build(mesh, scheme, bc_fn, init_fn, opt, Y_fn, inert, Sc, inlet_values, keep=False, species=True, solver=(1e-14, 2000), replay=True):
    """a device case on the implicitDiffusion branch and its replay; species i is fixedValue inlet_values[i] on patch 0 (None: nowhere),
    zero-gradient elsewhere; solver: (tolerance, maxIter) of the species' solves on both sides"""
    if isinstance(mesh, str):
        mesh = make_mesh(mesh)
    om = oracle_mesh_of(mesh)
    options = q.default_options(stencil=scheme, implicitDiffusion=1, **dict(SOLVER, **opt))
    dev = q.Device(mesh, fused_tables=False)
    gc = q.QGDFoamCase(dev, options)
    oc = OracleCase(om, options)
    apply_bcs = bc_fn or inlet_bcs(mesh)
    for case in (gc, oc):
        apply_bcs(case)
    C = mesh.array("C").reshape(-1, 3)

    def fresh():
        o2 = OracleCase(om, options)
        apply_bcs(o2)
        o2.set_fields(*init_fn(C))
        return o2
    Y0 = Y_fn(C)
    rep = None
    if species:
        names = [f"S{i}" for i in range(len(Y0))]
        gc.set_species(names, inert, ScNumbers=Sc, keep_fluxes=keep, implicit=True)
        if solver is not None:
            gc.set_species_solver(*solver)
        bcs = [({0: ("fixedValue", inlet_values[i])} if inlet_values is not None and inlet_values[i] is not None else None) for i in range(len(Y0))]
        for i in range(len(Y0)):
            if bcs[i]:
                gc.set_species_bc(i, 0, bcs[i][0])
            gc.set_species_field(names[i], Y0[i])
        if replay:
            tol, it = solver if solver is not None else (options.implicitTol, options.implicitMaxIter)
            rep = SpeciesImplicitReplay(mesh, om, oc, scheme, Y0, inert, ScNumbers=Sc, bcs=bcs, fresh=fresh, tolerance=tol, maxIter=it)
    U, T, p = init_fn(C)
    gc.set_fields(U, T, p)
    oc.set_fields(U, T, p)
    assert_separate_kernels(gc, scheme)
    return mesh, dev, gc, oc, rep


def compare_species(gc, rep, what, tag, common_scale=False):
    """common_scale: the error of every species against the largest of all species' fields -- for the fluxes of a case with a UNIFORM species,
    whose own diffusiveFlux is zero up to rounding (1e-18) and no scale for itself"""
    ref = {"Y": rep.Y, "phiJmY": rep.phiJmY, "diffusiveFlux": rep.diffusiveFlux, "Y.boundary": rep.Yb}[what]
    scale = max(float(np.abs(r).max()) for r in ref)
    for i in range(rep.n):
        got = gc.species_field(i, what)
        e = float(np.abs(got - ref[i]).max()) / scale if common_scale else rel_err(got, ref[i])
        print(tag, what, i, f"{e:.3e}", "(under the 1e-12 small-mesh bar)" if e <= 1e-12 else "")
        assert e <= TOL, (tag, what, i, e)


def compare_flow(gc, oc, tag):
    for name in ("rho", "U", "T"):
        e = rel_err(gc.field(name), oc.field(name))
        print(tag, name, f"{e:.3e}")
        assert e <= TOL, (tag, name, e)


@pytest.mark.parametrize("adjust", [0, 1])
@pytest.mark.parametrize("kind,scheme,bc_fn,init_fn,opt", MESHES)
def test_parity_with_the_replay(kind, scheme, bc_fn, init_fn, opt, adjust):
    o = dict(opt, mu=2e-2)
    if adjust:
        o.update(adjustTimeStep=1, maxCo=0.3)
    mesh, dev, gc, oc, rep = build(kind, scheme, bc_fn, init_fn, o, smooth_composition, 2, [0.7, 1.0, 1.0, 1.3], [0.3, 0.25, 0.3, 0.15], keep=True)
    tag = (kind, scheme, adjust)
    gc.step(1)
    rep.step(1)
    compare_species(gc, rep, "phiJmY", tag)
    compare_species(gc, rep, "diffusiveFlux", tag)
    compare_species(gc, rep, "Y", tag)
    gc.step(2)
    rep.step(2)
    compare_species(gc, rep, "Y", tag + ("3 steps",))
    compare_species(gc, rep, "Y.boundary", tag + ("3 steps",))
    assert min(float(y.min()) for y in rep.Y) > 0.0     # the parity above does not hide behind the clip
    ig, io = gc.info(), oc.info()
    assert ig["steps"] == io["steps"] == 3 and abs(ig["deltaT"] - io["deltaT"]) <= TOL * io["deltaT"]
    compare_flow(gc, oc, tag)
    assert_separate_kernels(gc, tag)
    info = gc.species_implicit_info()
    print(tag, info)
    gc.close(); dev.close()


def batch_width():
    mesh = q.PolyMesh.box(2, 2, 2)
    dev = q.Device(mesh, fused_tables=False)
    probe = q.QGDFoamCase(dev, q.default_options())
    W = probe.species_info()["batchWidth"]
    probe.close(); dev.close()
    return W


def many_species(n_active, inert, uniform):
    """n_active transported species around the inert one; species `uniform` (None: none) is constant"""
    def make(C):
        n = n_active + 1
        Y = []
        for i in range(n):
            if i == inert:
                Y.append(None)
            elif i == uniform:
                Y.append(np.full(C.shape[0], 0.45 / n_active))
            else:
                Y.append((0.45 / n_active) * (1.0 + 0.4 * np.sin((1.0 + 0.5 * i) * np.pi * C[:, 0] + 0.7 * i) * np.cos((0.5 + 0.3 * i) * np.pi * C[:, 1])))
        Y[inert] = 1.0 - sum(y for y in Y if y is not None)
        return Y
    return make


@pytest.mark.parametrize("n_active", ["W-1", "W", "W+1", "1"])
def test_batch_edges(n_active):
    """W - 1, W, W + 1 and one transported species (W: the register batch = the right-hand sides of one solve), the inert one in the middle,
    all Schmidt numbers distinct (a gam taken from the wrong slot shows); the last species is uniform with an inlet value equal to its
    field: its solve has nothing to do while its batch mates iterate on (the per-component `done` flags)"""
    W = batch_width()
    assert 2 <= W <= 4
    n_active = {"W-1": W - 1, "W": W, "W+1": W + 1, "1": 1}[n_active]
    inert = 1 if n_active > 1 else 0
    uniform = n_active if n_active > 1 else None
    Sc = [0.5 + 0.25 * i for i in range(n_active + 1)]
    inlet = [0.4 / n_active] * (n_active + 1)
    inlet[inert] = 0.6
    if uniform is not None:
        inlet[uniform] = 0.45 / n_active
    kind, scheme, bc_fn, init_fn, opt = MESHES[0]
    mesh, dev, gc, oc, rep = build(kind, scheme, bc_fn, init_fn, dict(opt, mu=2e-2), many_species(n_active, inert, uniform), inert, Sc, inlet, keep=True)
    assert gc.species_info()["nSpecies"] == n_active + 1
    gc.step(1)
    rep.step(1)
    compare_species(gc, rep, "diffusiveFlux", ("batch", n_active), common_scale=True)
    compare_species(gc, rep, "Y", ("batch", n_active))
    info = gc.species_implicit_info()
    print(("batch", n_active), info)
    assert sorted(info["species"]) == sorted(f"S{i}" for i in range(n_active + 1) if i != inert)
    gc.step(2)
    rep.step(2)
    compare_species(gc, rep, "Y", ("batch", n_active, "3 steps"))
    assert min(float(y.min()) for y in rep.Y) > 0.0
    gc.close(); dev.close()


def test_more_than_one_solver_block():
    """315 cells: one full block of 256 rows and a ragged second one, so that the folds of the partial sums see two blocks"""
    mesh = q.PolyMesh.box(9, 7, 5).jitter(0.1, seed=4)
    assert mesh.nCells == 315
    mesh, dev, gc, oc, rep = build(mesh, "GaussVolPoint", None, flow_fields, dict(deltaT=1e-3, mu=2e-2), smooth_composition, 2, [0.7, 1.0, 1.0, 1.3],
                                   [0.3, 0.25, 0.3, 0.15], keep=True)
    gc.step(1)
    rep.step(1)
    compare_species(gc, rep, "diffusiveFlux", "315 cells")
    gc.step(2)
    rep.step(2)
    compare_species(gc, rep, "Y", "315 cells")
    compare_flow(gc, oc, "315 cells")
    assert min(float(y.min()) for y in rep.Y) > 0.0
    gc.close(); dev.close()


def test_sign_of_the_matrix_flux():
    """a case at rest with one fixedValue inlet of the composition: diffusiveFlux_i minus its explicit part is YEqn.flux() of the NEW Y_i,
    -(a_f / Sc_i)(Y_N - Y_O) inside and -(a_b / Sc_i)(Y_b - Y_P) on the fixedValue faces -- the listing's sign [L64], opposite to the explicit
    branch's --, restated here from muf, magSf and the delta coefficients; the inert species' is minus the sum of the others'"""
    kind, scheme = "box654_jitter", "reduced"
    Sc, inlet = [0.7, 1.0, 1.0, 1.3], [0.3, 0.25, 0.3, 0.15]
    mesh = make_mesh(kind)
    mesh, dev, gc, oc, rep = build(mesh, scheme, lambda case: flow_bcs(mesh, case), lambda C: flow_fields(C, moving=False), dict(deltaT=1e-3, mu=2e-2),
                                   smooth_composition, 2, Sc, inlet, keep=True)
    gc.step(1)
    rep.step(1)
    nif = mesh.nInternalFaces
    own, nei = mesh.array("owner"), mesh.array("neighbour")
    delta = np.where(np.arange(mesh.nFaces) < nif, mesh.array("nonOrthDeltaCoeffs"), mesh.array("deltaCoeffs"))
    a = rep.muf * mesh.array("magSf") * delta
    start, size = int(mesh.array("patchStart")[0]), int(mesh.array("patchSize")[0])
    total = np.zeros(mesh.nFaces)
    for i in (0, 1, 3):
        Y = gc.species_field(i, "Y")
        want = np.zeros(mesh.nFaces)
        want[:nif] = -(a[:nif] / Sc[i]) * (Y[nei[:nif]] - Y[own[:nif]])
        want[start:start + size] = -(a[start:start + size] / Sc[i]) * (inlet[i] - Y[own[start:start + size]])
        assert np.abs(want[:nif]).max() > 1e-8 and np.abs(want[start:start + size]).max() > 1e-8
        got = gc.species_field(i, "diffusiveFlux")
        e = rel_err(got - rep.explicitFlux[i], want)
        print("YEqn.flux()", i, f"{e:.3e}")
        assert e <= TOL, (i, e)
        assert rel_err(got - rep.explicitFlux[i], -want) > 1.0          # (the other sign is far away)
        total += got
    e = rel_err(gc.species_field(2, "diffusiveFlux"), -total)
    print("inert diffusiveFlux", f"{e:.3e}")
    assert e <= 1e-13
    assert np.all(gc.species_field(2, "phiJmY") == 0.0)
    gc.close(); dev.close()


CLIP_EPS = 1e-11


def test_clip():
    """a front (test_species_case_gpu.front_composition) with a weak QGD regularisation and a long step, so that the solution of species 0
    undershoots ahead of the front: Yi.max(0) acts on the device where it acts in the replay.

    Where is decided by the SIGN of the solve's result.  These parameters were chosen on the host replay so that the sign is decided: the
    smallest value the replay leaves positive is 1.4e-13 here (ahead of the front the solution decays, with the default regularisation down
    to 1e-17), a hundred times what the two solvers, both run to a normalised residual of 1e-14, differ by on this case (1e-15).  The zero
    pattern is compared exactly; next to it, what holds whatever the margin: a clipped cell holds at most CLIP_EPS on the other side (1e-11:
    three decades above the solves' tolerance, under the 1e-10 bar on a field of order 0.5)."""
    kind, scheme, bc_fn, init_fn, opt = MESHES[0]
    o = dict(opt, deltaT=8e-3, mu=1e-3, alphaQGD=0.08, ScQGD=0.3)
    mesh, dev, gc, oc, rep = build(kind, scheme, bc_fn, init_fn, o, front_composition, 2, [0.7, 1.0, 1.0], None)
    zeros_seen = 0
    for step in range(3):
        gc.step(1)
        rep.step(1)
        for i in range(3):
            got, ref = gc.species_field(i, "Y"), rep.Y[i]
            e = rel_err(got, ref)
            gz, rz = got == 0.0, ref == 0.0
            print("clip", step, i, f"{e:.3e}", "zeros", int(gz.sum()), int(rz.sum()), "common", int((gz & rz).sum()))
            assert e <= TOL, (step, i, e)
            assert got.min() >= 0.0 and np.all(got[rz] <= CLIP_EPS) and np.all(ref[gz] <= CLIP_EPS), (step, i)
            assert np.array_equal(gz, rz), (step, i)
        zeros_seen += int((rep.Y[0] == 0.0).sum())
    assert zeros_seen >= 3
    gc.close(); dev.close()


def test_flow_untouched():
    """rho, U, T, p, rhoE of an implicit case with species are, bit for bit, those of the same case without.  Species turn the block-fused
    assembly of the U systems off; both cases here run the SEPARATE implicit kernels (a device without block tables), the path a case with
    species takes"""
    kind, scheme, bc_fn, init_fn, opt = MESHES[0]
    for adjust in (0, 1):
        o = dict(opt, mu=2e-2, adjustTimeStep=adjust, maxCo=0.3)
        _, dev_a, a, _, _ = build(kind, scheme, bc_fn, init_fn, o, smooth_composition, 2, None, [0.3, 0.25, 0.3, 0.15], replay=False)
        _, dev_b, b, _, _ = build(kind, scheme, bc_fn, init_fn, o, smooth_composition, 2, None, None, species=False)
        assert_separate_kernels(a, "with species")
        assert_separate_kernels(b, "without species")
        a.step(3)
        b.step(3)
        for name in ("rho", "U", "T", "p", "rhoE"):
            assert np.array_equal(a.field(name), b.field(name)), ("separate implicit kernels", adjust, name)
        assert a.info() == b.info() and a.implicit_info() == b.implicit_info()
        a.close(); b.close(); dev_a.close(); dev_b.close()


def test_species_turn_the_block_fused_assembly_off():
    mesh = q.PolyMesh.box(8, 8, 8)
    dev = q.Device(mesh, fused_tables="any")
    gc = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", implicitDiffusion=1))
    before = gc.fused_info()
    gc.set_species(["A", "B"], "B", implicit=True)
    after = gc.fused_info()
    assert not after["fusedImplicit"] and not after["fused"] and after["blocks"] == 0, (before, after)
    gc.close(); dev.close()


def test_controls_and_statistics(monkeypatch):
    kind, scheme, bc_fn, init_fn, opt = MESHES[0]
    args = (kind, scheme, bc_fn, init_fn, dict(opt, mu=2e-2), smooth_composition, 2, [0.7, 1.0, 1.0, 1.3], [0.3, 0.25, 0.3, 0.15])
    _, dev, gc, _, _ = build(*args, solver=(1e-12, 2000), replay=False)
    gc.step(2)
    info = gc.species_implicit_info()
    print(info)
    assert sorted(info["species"]) == ["S0", "S1", "S3"] and info["unconvergedSteps"] == 0
    for name, s in info["species"].items():
        assert 0 < s["iterations"] < 500 and s["final"] < 1e-12 <= s["initial"], (name, s)
    Y = [gc.species_field(i) for i in range(4)]
    gc.close(); dev.close()
    # without set_species_solver: the case's implicitTol / implicitMaxIter
    _, dev, gc, _, _ = build(*args, solver=None, replay=False)
    gc.step(2)
    for i in range(4):
        assert rel_err(gc.species_field(i), Y[i]) <= TOL
    assert gc.species_implicit_info()["unconvergedSteps"] == 0
    gc.close(); dev.close()
    # an iteration limit that cannot be met: counted, and the step still succeeds
    _, dev, gc, _, _ = build(*args, solver=(1e-12, 2), replay=False)
    gc.step(1)
    assert gc.species_implicit_info()["unconvergedSteps"] == 1
    gc.step(1)
    info = gc.species_implicit_info()
    assert info["unconvergedSteps"] == 2 and all(s["iterations"] <= 2 for s in info["species"].values()), info
    gc.close(); dev.close()
    # conjugate gradients instead of the Chebyshev iteration
    monkeypatch.setenv("QGD_IMPL_SOLVER", "pcg")
    _, dev, gc, _, _ = build(*args, solver=(1e-12, 2000), replay=False)
    assert gc.implicit_info()["solver"] == "pcg"
    gc.step(2)
    for i in range(4):
        e = rel_err(gc.species_field(i), Y[i])
        print("pcg against chebyshev", i, f"{e:.3e}")
        assert e <= TOL, (i, e)
    gc.close(); dev.close()
    # the controls belong to the implicit branch of a case with species
    mesh = make_mesh(kind)
    dev = q.Device(mesh, fused_tables=False)
    gc = q.QGDFoamCase(dev, q.default_options(implicitDiffusion=1))
    refusal(lambda: gc.set_species_solver(1e-8, 100), L.ERR_INVALID, "no species")
    gc.set_species(["A", "B"], "B", implicit=True)
    refusal(lambda: gc.set_species_solver(0.0, 100), L.ERR_INVALID, "tolerance")
    refusal(lambda: gc.set_species_solver(1e-8, 0), L.ERR_INVALID, "maxIter")
    gc.close()
    gc = q.QGDFoamCase(dev, q.default_options())
    gc.set_species(["A", "B"], "B", implicit=True)          # (the flag is ignored on the explicit branch)
    refusal(lambda: gc.set_species_solver(1e-8, 100), L.ERR_INVALID, "explicit branch")
    refusal(lambda: gc.species_implicit_info(), L.ERR_INVALID, "implicitDiffusion")
    gc.close(); dev.close()


def test_refusals_kept():
    mesh = q.PolyMesh.box(6, 5, 4)
    dev = q.Device(mesh, fused_tables=False)
    gc = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", termStencils={"grad(p)": "reduced"}))
    refusal(lambda: gc.set_species(["A", "B"], 1), L.ERR_NOT_IMPLEMENTED, "per-term stencils")
    gc.close()
    gc = q.QGDFoamCase(dev, q.default_options(implicitDiffusion=1))
    # the implicit branch is asked for by name (QGD_SPECIES_IMPLICIT): without the flag such a case answers as it always did
    refusal(lambda: gc.set_species(["A", "B"], "B"), L.ERR_NOT_IMPLEMENTED, "implicitDiffusion", "QGD_SPECIES_IMPLICIT")
    gc.set_species(["A", "B"], "B", implicit=True)
    C = mesh.array("C").reshape(-1, 3)
    for n, v in (("A", 0.3), ("B", 0.7)):
        gc.set_species_field(n, np.full(mesh.nCells, v))
    gc.set_fields(*flow_fields(C))
    refusal(lambda: gc.step_phase(3), L.ERR_NOT_IMPLEMENTED, "species")
    refusal(lambda: gc.step_phase(20), L.ERR_NOT_IMPLEMENTED, "species")
    gc.step(1)
    assert np.abs(gc.species_field("A") - 0.3).max() <= 1e-13
    gc.close(); dev.close()
    sh = q.PolyMesh.box(8, 6, 4).shard(2, 0)
    sdev = q.Device(sh, fused_tables=False)
    sc = q.QGDFoamCase(sdev, q.default_options(implicitDiffusion=1))
    refusal(lambda: sc.set_species(["A", "B"], 1, implicit=True), L.ERR_NOT_IMPLEMENTED, "sharded")
    sc.close(); sdev.close()
    G = L.PATCH_GENERIC
    ext = q.PolyMesh.box(6, 5, 4, patch_types=[L.PATCH_CYCLIC, L.PATCH_CYCLIC, G, G, G, G]).unroll_cyclic()
    pdev = q.Device(ext, fused_tables=False)
    pc = q.QGDFoamCase(pdev, q.default_options(implicitDiffusion=1))
    refusal(lambda: pc.set_species(["A", "B"], 1, implicit=True), L.ERR_NOT_IMPLEMENTED, "periodic")
    pc.close(); pdev.close()


def test_the_new_entries_resolve():
    lib = ctypes.CDLL(L.lib._name)
    for name in ("qgd_case_set_species_solver", "qgd_case_species_implicit_info"):
        assert getattr(lib, name) is not None and hasattr(L.lib, name), name


def test_the_other_step_entry_serves_an_implicit_species_case_too():
    """qgd_case_step_sharded steps an unsharded device like qgd_case_step: the same species, bit for bit"""
    kind, scheme, bc_fn, init_fn, opt = MESHES[0]
    args = (kind, scheme, bc_fn, init_fn, dict(opt, mu=2e-2), smooth_composition, 2, [0.7, 1.0, 1.0, 1.3], [0.3, 0.25, 0.3, 0.15])
    _, dev_a, a, _, _ = build(*args, keep=True, replay=False)
    _, dev_b, b, _, _ = build(*args, keep=True, replay=False)
    a.step(2)
    for _ in range(2):
        L.check(L.lib.qgd_case_step_sharded(b._h, None, None, 0, 0), "qgd_case_step_sharded")
    b.sync()
    for i in range(4):
        for what in ("Y", "Y.boundary", "phiJmY", "diffusiveFlux"):
            assert np.array_equal(a.species_field(i, what), b.species_field(i, what)), (i, what)
    a.close(); b.close(); dev_a.close(); dev_b.close()


FV_SOLUTION = ('FoamFile { version 2.0; format ascii; class dictionary; object fvSolution; }\n'
               'solvers\n{\n    "(U|e)" { solver PBiCGStab; preconditioner DILU; tolerance 1e-12; relTol 0; maxIter 2000; }\n'
               '    "(N2|O2|H2O)" { solver PBiCGStab; preconditioner DILU; tolerance 1e-12; relTol 0; maxIter 2000; }\n}\n')


def test_application_runs_an_implicit_species_case_and_restarts(tmp_path):
    """python -m qgdsolver_amd.QGDFoam on a written species case WITHOUT an implicitDiffusion entry (the reference's default: true), in child
    processes: six steps in one run; three steps, a restart from the written time and three more in another.  Whole against restarted: the
    bar tests/test_species_case_gpu.py documents for the restart's one-step-behind patch densities, 1e-6 (measured there: 1.1e-7); printed."""
    from qgdsolver_amd import foamfile as ff
    from test_species_implicit_reader import uncorrected_laplacian
    from test_species_reader import write_species_case

    def run(case_dir):
        r = subprocess.run([sys.executable, "-m", "qgdsolver_amd.QGDFoam", "-case", str(case_dir)], capture_output=True, text=True, cwd=ROOT,
                           env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")), timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    whole, split = str(tmp_path / "whole"), str(tmp_path / "split")
    for d, end in ((whole, 6e-3), (split, 3e-3)):
        write_species_case(d, end_time=end, write_interval=3e-3)
        tp = os.path.join(d, "constant", "thermophysicalProperties")
        text = open(tp).read()
        assert "implicitDiffusion false;" in text
        open(tp, "w").write(text.replace("implicitDiffusion false;", ""))
        uncorrected_laplacian(d)
        open(os.path.join(d, "system", "fvSolution"), "w").write(FV_SOLUTION)
    out = run(whole)
    assert "implicitDiffusion true" in out and "species N2 O2 H2O (inert N2)" in out
    assert "O2: " in out and "H2O: " in out and " in " in out            # the species' solve lines, as those of U and e
    run(split)
    cd = os.path.join(split, "system", "controlDict")
    text = open(cd).read().replace("endTime 0.003;", "endTime 0.006;").replace("startFrom startTime;", "startFrom latestTime;")
    assert "latestTime" in text and "endTime 0.006;" in text
    open(cd, "w").write(text)
    assert "start 0.003" in run(split)
    m = ff.read_polymesh(os.path.join(whole, "constant", "polyMesh"))
    names = ("N2", "O2", "H2O")
    setup = ff.read_case_setup(whole, "0")[1]
    assert setup["implicitDiffusion"] == 1 and setup["species"]["tolerance"] == 1e-12 and setup["species"]["maxIter"] == 2000
    Y0 = setup["species"]["fields"]
    read = lambda d, t, n: ff.read_field(os.path.join(d, t, n), m)[0]   # noqa: E731
    for n in names:
        a, b = read(whole, "0.003", n)[:, 0], read(split, "0.003", n)[:, 0]
        assert np.array_equal(a, b), n
        assert np.abs(a - Y0[n]).max() > 1e-6          # (the species did move)
    for d in (whole, split):
        assert np.abs(sum(read(d, "0.006", n)[:, 0] for n in names) - 1.0).max() <= 1e-14
    for n in names:
        e = rel_err(read(split, "0.006", n), read(whole, "0.006", n))
        print("restarted vs uninterrupted", n, f"{e:.3e}")
        assert e <= 1e-6, (n, e)
