"""The step kernels on tetrahedra, prisms and prisms + hexahedra (tests/unstructured.py) against the CPU oracle.

Every other mesh of the suite is a box of hexahedra, jittered or with faces / edges split: no vertex has more than eight cells and no cell
fewer than six faces.  On these meshes a vertex has up to 24 (tetrahedra) or 12 (prisms, mix) cells, so the vertex walks of
fusedFaceCellKernel (explicit, IMPL, ADJ) and qhdFusedAdvanceKernel leave their eight register slots and read positions and weights from
memory, the ELL rows of the vertex kernel and the ghost layers of a shard are long, and the per-cell walks (face entries, matrix rows of
the pressure multigrid and the Chebyshev iteration) meet rows of four and five entries, padded to their stride, in wavefronts that are not
all hexahedra.  The host side of the block tables is checked entry by entry in tests/test_fused_blocks_host.py (capPE = 24 / 12 there);
the implicitDiffusion branch on these meshes is in tests/test_implicit_diffusion.py.

Tolerances are those of the files whose patterns are reused: 1e-12 for the fvsc operators (test_fvsc_parity_gpu), 1e-13 / 1e-11 / 1e-10 for
initial state / face fields / states (test_case_parity_gpu), 1e-11 for deltaT and the Courant number, 1e-9 and pFinalResidual < 1e-12 for
QHDFoam (test_qhd_case), 1e-12 against the unsharded device and 1e-10 against the oracle for shards (test_partition_gpu), 1e-13 for the
mass balance (test_cyclic_patches).  Each test prints its worst error (pytest -s).

The other families on these meshes: species (explicit, implicitDiffusion, range shards), varScModel7, QHDFoam with implicitDiffusion true,
QHDFoam and QGDFoam-implicit on range cuts, symmetry and cyclic patches in tests/test_unstructured_families_gpu.py; the run monitors
(tests/test_monitor_gpu.py, test_species_monitor_gpu.py, test_qhd_monitor_gpu.py) and scalarTransportQHDFoam
(tests/test_scalar_transport_case.py) as rows of their own files; SRFQHDFoam on tet433 in tests/test_srf_qhd_gpu.py.  The table of all of them
is tests/test_unstructured_meshes.py::test_every_family_has_an_unstructured_row.  Not on these meshes yet: SRFQHDFoam beyond that one arm,
species on cyclic patches, varScModel7 on shards, the applications on a written case.

One level of 2:1 refinement with hanging nodes (unstructured.REFINED: ref533, ref866, the quadtree ref2d87) runs as rows of the tests here and
of the families' files, and in tests/test_refined_cells_gpu.py, whose docstring says which row reaches which per-cell face loop with a cell
of 24 faces.  There the vertices stay within eight cells; it is the cells that are long (6 to 24 faces in one wavefront) and the faces that
have collinear points."""
import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import fvsc, qhdfoam

import cases
import unstructured
from oracle import OracleQhdCase
from test_case_parity_gpu import CELL_FIELDS, FACE_FIELDS, FLUX_TOL, STATE_TOL, build_pair, compare_fields, mixed_box_bcs
from test_fvsc_parity_gpu import OPS, TOL as FVSC_TOL
from test_partition import mixed_bcs, run_oracle
from test_partition_gpu import run_device, run_sharded_device
from test_qhd_case import cavity_bcs, initial, options as qhd_options
from util import assert_path, expects_fused, expects_fused_adjust, make_mesh, oracle_mesh_of, rel_err

pytestmark = pytest.mark.gpu

VALENCE = {"tet433": 24, "tet866": 24, "prism543": 12, "mix643": 12}
MOST_FACES = {"ref533": 24, "ref866": 24, "ref2d87": 10}
EXPLICIT = dict(deltaT=2e-4, mu=2e-3)


def report(family, tag, worst):
    print(f"unstructured {family} {tag}: worst {max(worst.values()):.3e} ({max(worst, key=worst.get)})")


def long_vertex_rows(kind, dev=None):
    """the mesh is one whose vertices have more cells than the fused kernels keep in registers (the vertex stride capPE of the block tables is
    the longest row: tests/test_fused_blocks_host.py), and the device has block tables.  The refined kinds: the mesh is one whose cells have
    more faces than a per-cell loop takes in one pass of eight, up to 24 (the entry stride capE of the block tables)"""
    if kind in unstructured.REFINED:
        prim = unstructured.refined_primitives(kind)
        per_cell = unstructured.faces_per_cell(prim)
        assert int(per_cell.max()) == MOST_FACES[kind] > 8 and int(per_cell.min()) == 6 and int(np.diff(prim["faceOffsets"]).max()) >= 7
    else:
        assert int(unstructured.point_valence(unstructured.primitives(kind)).max()) == VALENCE[kind] > 8
    if dev is not None:
        fb = dev.fused_blocks()
        assert fb["blocks"] >= (2 if kind.startswith("tet") else 1) and fb["templates"] >= 1 and 0 < fb["ldsBytes"] <= 64 * 1024, fb


# ---- fvsc operators -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("scheme", ["GaussVolPoint", "reduced"])
@pytest.mark.parametrize("kind", ["tet433", "prism543", "mix643", "ref533"])
def test_fvsc_operators_match_oracle(kind, scheme, entry):
    mesh = make_mesh(kind)
    om = oracle_mesh_of(mesh)
    dev = q.Device(mesh, fv_schemes={"fvsc": {"default": scheme}})
    worst = {}
    for op, nc in OPS:
        cell, bnd = cases.random_fields(mesh.nCells, mesh.nBoundaryFaces, nc, seed=sum(map(ord, kind + op)))
        rc, ref = om.fvsc(scheme, op, cell, bnd)
        assert rc == 0
        if entry == "host":
            vf = q.volField("f", cell, bnd)
            got = fvsc.grad(dev, vf) if op.startswith("grad") else fvsc.div(dev, vf)
        else:
            nco = 3 * nc if op.startswith("grad") else nc // 3
            vf = q.deviceVolField("f", dev.to_device(cell), dev.to_device(bnd), nc)
            out = dev.alloc(8 * mesh.nFaces * nco)
            ret = fvsc.grad(dev, vf, out=out) if op.startswith("grad") else fvsc.div(dev, vf, out=out)
            assert ret == out
            dev.sync()
            got = dev.to_host(out, ref.shape)
            for ptr in (vf.internal, vf.boundary, out):
                dev.release(ptr)
        assert got.shape == ref.shape and np.abs(ref).max() > 0
        worst[op] = rel_err(got, ref)
        assert worst[op] <= FVSC_TOL, (kind, scheme, entry, op, worst[op])
    report("fvsc", (kind, scheme, entry), worst)
    dev.close()


# ---- explicit QGDFoam step -----------------------------------------------------------------------------------------------------------
EXPLICIT_CASES = [(kind, "GaussVolPoint", bc_fn, arm) for kind in ("tet433", "prism543", "mix643", "tet866") for bc_fn in (None, mixed_box_bcs)
                  for arm in ("fused", "kernels")] + [("tet433", "reduced", None, "kernels")]
# one level of 2:1 refinement: cells of 6 to 24 face entries in one block, faces with hanging nodes (GaussVolPoint's FK_OTHER fallback)
EXPLICIT_CASES += [(kind, "GaussVolPoint", bc_fn, arm) for kind in ("ref533", "ref866") for bc_fn in (None, mixed_box_bcs) for arm in ("fused", "kernels")]


def test_the_explicit_matrix_covers_both_arms():
    assert sum(1 for c in EXPLICIT_CASES if c[3] == "fused") == 12 and sum(1 for c in EXPLICIT_CASES if c[3] == "kernels") == 13
    for kind in ("ref533", "ref866"):
        assert {(c[2], c[3]) for c in EXPLICIT_CASES if c[0] == kind} == {(bc, arm) for bc in (None, mixed_box_bcs) for arm in ("fused", "kernels")}


@pytest.mark.parametrize("kind,scheme,bc_fn,arm", EXPLICIT_CASES)
def test_update_fluxes_and_steps(kind, scheme, bc_fn, arm, init_fn=None):
    """test_case_parity_gpu.test_update_fluxes_and_steps on these meshes: initial state, face fields after updateFluxes, states after
    1 + 4 + 20 steps; default patches (zeroGradient) and the mixed ones, whose qgdFlux walls bring the mid-assembly refresh"""
    mesh, dev, gc, oc = build_pair(kind, scheme, bc_fn, init_fn, arm=arm, **EXPLICIT)    # (asserts the arm that runs)
    assert expects_fused(mesh, q.default_options(stencil=scheme, **EXPLICIT)) == (scheme == "GaussVolPoint" and mesh.nGeometricD == 3)
    long_vertex_rows(kind, dev if arm == "fused" else None)
    tag = (kind, scheme, "mixed" if bc_fn is mixed_box_bcs else bc_fn.__name__ if bc_fn else "default", arm)
    rho0 = oc.field("rho").copy()
    worst = {}
    worst.update({"init " + k: v for k, v in compare_fields(gc, oc, CELL_FIELDS, 1e-13, tag + ("init",)).items()})
    compare_fields(gc, oc, [n + ".boundary" for n in ("rho", "U", "p", "e", "c", "H", "muQGD")], 1e-13, tag + ("init.bnd",))
    gc.updateFluxes()
    oc.updateFluxes()
    flux = compare_fields(gc, oc, FACE_FIELDS, FLUX_TOL, tag + ("fluxes",))
    state = {}
    for chunk in (1, 4, 20):
        gc.step(chunk)
        oc.step(chunk)
        state.update({f"{k} +{chunk}": v for k, v in compare_fields(gc, oc, ["rho", "U", "p", "e", "rhoU", "rhoE"], STATE_TOL, tag + (f"step+{chunk}",)).items()})
    gc.updateFluxes()
    oc.updateFluxes()
    compare_fields(gc, oc, CELL_FIELDS, STATE_TOL, tag + ("final",))
    compare_fields(gc, oc, FACE_FIELDS, STATE_TOL, tag + ("final fluxes",))
    gc.info()
    gc.step(1)
    oc.step(1)
    ig, io = gc.info(), oc.info()
    assert ig["steps"] == io["steps"] == 26
    assert abs(ig["minRho"] - io["minRho"]) <= 1e-9 and abs(ig["minE"] - io["minE"]) <= 1e-9 and ig["minRho"] > 0 and ig["minE"] > 0
    assert np.abs(oc.field("rho") - rho0).max() > 1e-4 * np.abs(rho0).max()       # (something happened: 1e-3 of it, against a bar of 1e-10)
    report("explicit init", tag, worst)
    report("explicit fluxes", tag, flux)
    report("explicit states", tag, state)
    gc.close(); dev.close()


# ---- adjustTimeStep -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["fusedAdjust", "kernels"])
@pytest.mark.parametrize("kind", ["tet433", "mix643", "ref533"])
def test_adjust_time_step(kind, arm):
    """Courant number, deltaT and time follow the oracle step by step (1e-11), the states after ten steps (1e-10)"""
    opt = dict(deltaT=1e-4, mu=2e-3, adjustTimeStep=1, maxCo=0.3, maxDeltaT=1.0, cTau=0.75)
    mesh, dev, gc, oc = build_pair(kind, "GaussVolPoint", mixed_box_bcs, None, arm=arm, **opt)
    assert expects_fused_adjust(mesh, q.default_options(stencil="GaussVolPoint", **opt))
    long_vertex_rows(kind, dev if arm == "fusedAdjust" else None)
    worst = {"deltaT": 0.0, "CoNum": 0.0}
    for _ in range(10):
        gc.step(1)
        oc.step(1)
        ig, io = gc.info(), oc.info()
        worst["deltaT"] = max(worst["deltaT"], abs(ig["deltaT"] - io["deltaT"]) / io["deltaT"])
        worst["CoNum"] = max(worst["CoNum"], abs(ig["CoNum"] - io["CoNum"]) / max(io["CoNum"], 1e-30))
        assert abs(ig["deltaT"] - io["deltaT"]) <= 1e-11 * io["deltaT"], (ig, io)
        assert abs(ig["CoNum"] - io["CoNum"]) <= 1e-11 * max(io["CoNum"], 1e-30), (ig, io)
        assert abs(ig["time"] - io["time"]) <= 1e-11 * io["time"]
    assert oc.info()["deltaT"] > 2e-4                       # (the step grew: deltaT is the controller's, not the initial one)
    worst.update(compare_fields(gc, oc, ["rho", "U", "p", "e"], STATE_TOL, (kind, arm, "adjust")))
    report("adjustTimeStep", (kind, arm), worst)
    gc.close(); dev.close()


# ---- QHDFoam ---------------------------------------------------------------------------------------------------------------------------
QHD_FIELDS = ("U", "T", "p", "phi", "U.boundary", "T.boundary", "p.boundary")


QHD_VARIANTS = {"kernels": {}, "blocks": {"QGD_QHD_FUSED": "1"}, "deep": {"QGD_MG_DENSE_MAX": "64"}, "deep plain": {"QGD_MG_DENSE_MAX": "64", "QGD_MG_SA": "0"}}


@pytest.mark.parametrize("kind,variant", [("tet433", "kernels"), ("mix643", "kernels"), ("tet866", "kernels"), ("tet433", "blocks"),
                                          ("tet866", "deep"), ("tet866", "deep plain"),
                                          ("ref533", "kernels"), ("ref533", "blocks"), ("ref533", "deep"), ("ref533", "deep plain"), ("ref866", "kernels"),
                                          ("ref866", "deep plain")])
def test_qhd_case_matches_oracle(kind, variant, monkeypatch):
    """the buoyant cavity of test_qhd_case (15 steps, 1e-9, pFinalResidual < 1e-12).  "blocks": the U and T equations on the cell blocks
    (QGD_QHD_FUSED=1, qhdFusedAdvanceKernel: the second kernel whose vertex walk leaves its registers), asserted to be what runs.  By default
    a pressure matrix of up to 2048 rows is not coarsened -- every mesh here, the 1728 tetrahedra included: one level, its smoothing sweeps
    over rows of four or five entries and nothing else of the multigrid; "deep" (QGD_MG_DENSE_MAX=64, the knob of test_mg_cycle_gpu, whose
    'tetrahedra' rows check the cycle itself as an operator) makes the hierarchy aggregate the tetrahedral graph, smoothed and plain,
    asserted by its level count.  (The plain aggregation coarsens a matrix of more than 600 rows only, whatever QGD_MG_DENSE_MAX says: the
    143 rows of ref533 stay one level under "deep plain" -- asserted as well -- and ref866 has the plain hierarchy over rows of 6 to 24
    entries.)  The pressure iteration counts of the device and of the oracle are printed, not asserted."""
    for k, v in QHD_VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    fused = variant == "blocks"
    mesh = make_mesh(kind)
    om = oracle_mesh_of(mesh)
    opt = qhd_options("GaussVolPoint", deltaT=1e-3)
    dev = q.Device(mesh, fused_tables="any" if fused else True)
    gc, oc = qhdfoam.QHDFoamCase(dev, opt), OracleQhdCase(om, opt)
    fi = gc.fused_info()
    assert fi["fusedAdvance"] == fused and (not fused or (fi["blocks"] >= 2 and 0 < fi["ldsAdvance"] <= 65536)), fi
    long_vertex_rows(kind, dev if fused else None)
    U, T, p = initial(mesh)
    U = U + 1e-2 * np.random.default_rng(3).standard_normal(U.shape)
    for c in (gc, oc):
        cavity_bcs(c, mesh)
        c.set_fields(U, T, p)
    its = []
    for _ in range(15):
        gc.step(1); oc.step(1)
        its.append((gc.info()["pIterations"], oc.info()["pIterations"]))
    worst = {}
    for f in QHD_FIELDS:
        ref = oc.field(f)
        scale = max(np.abs(ref).max(), 1e-300)
        worst[f] = float(np.abs(gc.field(f) - ref).max() / scale)
        assert worst[f] <= 1e-9, (kind, fused, f, worst[f])
    assert np.abs(oc.field("U")).max() > 1e-3
    gi = gc.info()
    assert gi["pFinalResidual"] < 1e-12 and gi["steps"] == 15, gi
    assert (gi["mgLevels"] >= 2) == (variant == "deep" or (variant == "deep plain" and mesh.nCells > 600)), gi
    report("QHDFoam", (kind, variant), worst)
    print(f"unstructured QHDFoam {kind} {variant}: pressure iterations per step (device, oracle) {its}; multigrid levels {gi.get('mgLevels')}")
    gc.close(); dev.close()


# ---- shards ---------------------------------------------------------------------------------------------------------------------------
_SHARD_REF = {}


def _shard_reference(kind, fused):
    """the Morton-renumbered mesh, its fields, the oracle's run and the unsharded device's: formed once per (mesh, arm), read by both phase orders"""
    if (kind, None) not in _SHARD_REF:
        g = make_mesh(kind)
        g.renumber(g.morton_order())
        U, T, p = cases.box_initial_fields(g.array("C").reshape(-1, 3))
        _SHARD_REF[(kind, None)] = (g, U, T, p, run_oracle(g, "GaussVolPoint", mixed_bcs, U, T, p, 10, **EXPLICIT))
    g, U, T, p, ref = _SHARD_REF[(kind, None)]
    if (kind, fused) not in _SHARD_REF:
        _SHARD_REF[(kind, fused)] = run_device(g, "GaussVolPoint", mixed_bcs, U, T, p, 10, fused_tables=fused, **EXPLICIT)
    return g, U, T, p, ref, _SHARD_REF[(kind, fused)]


@pytest.mark.parametrize("overlapped", [False, True])
@pytest.mark.parametrize("fused", ["any", False])
@pytest.mark.parametrize("kind,world", [("tet433", 3), ("tet866", 2), ("ref866", 3)])
def test_sharded_device_matches_unsharded_and_oracle(kind, world, fused, overlapped):
    """cell ranges of the Morton-ordered mesh, one vertex-connected ghost layer each (on tetrahedra more ghost cells than owned ones): the
    fused step and the separate kernels, plain phase order (0, 1) and boundary layer first (0, 10, 11), qgdFlux walls (mid-step exchange)"""
    g, U, T, p, ref, one = _shard_reference(kind, fused)
    got = run_sharded_device(g, world, "GaussVolPoint", mixed_bcs, U, T, p, 10, overlapped=overlapped, fused_tables=fused, **EXPLICIT)
    worst = {}
    for f in ref:
        scale = np.abs(ref[f]).max()
        worst[f + " vs unsharded"] = float(np.abs(got[f] - one[f]).max() / scale)
        worst[f + " vs oracle"] = float(np.abs(got[f] - ref[f]).max() / scale)
        assert worst[f + " vs unsharded"] <= 1e-12, (kind, world, fused, overlapped, f, "sharded vs unsharded device", worst)
        assert worst[f + " vs oracle"] <= 1e-10, (kind, world, fused, overlapped, f, "sharded device vs oracle", worst)
    report("shards", (kind, world, "fused" if fused else "kernels", "layer first" if overlapped else "plain"), worst)


# ---- a property the oracle and the device cannot get wrong together ----------------------------------------------------------------------
def _closed_box(kind, scheme, arm):
    mesh = make_mesh(kind)
    dev = q.Device(mesh, fused_tables="any" if arm == "fused" else False)
    gc = q.QGDFoamCase(dev, q.default_options(stencil=scheme, **EXPLICIT))
    assert_path(gc, arm, (kind, scheme))
    for patch in range(6):
        gc.set_bc(patch, U=("slip", None), T=("zeroGradient", None), p=("qgdFlux", None))
    gc.set_fields(*cases.box_initial_fields(mesh.array("C").reshape(-1, 3)))
    return mesh, dev, gc, gc.field("rho").copy()


def test_mass_balance_of_a_box_closed_by_slip_walls_on_the_fused_step():
    """tet433 closed by slip walls (qgdFlux pressure), 20 fused steps: the mass changes by what the step's own mass flux carries through
    the walls and by nothing else, to 1e-13 of the mass -- every internal face gives one cell what it takes from the other, whichever block
    computes it and however a cell's face entries are padded.  (Under GaussVolPoint the wall flux itself does not vanish where the
    cell centre does not lie on the wall face's normal: the patch-face gradient of p is not nf * snGrad, so qgdFlux cancels phiw only
    approximately.  The ORACLE's mass drifts by 7.1e-7 over these 20 steps, by 8.9e-9 on the jittered hexahedra of box654_jitter and by
    3e-16 on the uniform box: a bare "mass is constant to 1e-13" is not a property of the scheme on these meshes with this stencil.  With
    the wall flux accounted for the balance is exact, which is the same statement where the flux vanishes: the test below.)"""
    mass_balance_through_the_walls("tet433")


def mass_balance_through_the_walls(kind):
    mesh, dev, gc, rho0 = _closed_box(kind, "GaussVolPoint", "fused")
    long_vertex_rows(kind, dev)
    V, nif = mesh.array("V"), mesh.nInternalFaces
    m0 = mass = float((V * gc.field("rho")).sum())
    through_walls, worst = 0.0, 0.0
    for _ in range(20):
        gc.updateFluxes()
        out = float(gc.field("phiJm")[nif:].sum())
        gc.step(1)
        new = float((V * gc.field("rho")).sum())
        worst = max(worst, abs(new - mass + EXPLICIT["deltaT"] * out) / m0)
        through_walls += EXPLICIT["deltaT"] * out
        mass = new
    total = abs(mass - m0 + through_walls) / m0
    print(f"unstructured mass balance {kind} fused: per step {worst:.3e}, over 20 steps {total:.3e}; through the walls {through_walls / m0:.3e} of the mass")
    assert worst <= 1e-13 and total <= 1e-13, (worst, total)
    assert np.abs(gc.field("rho") - rho0).max() > 1e-4 * np.abs(rho0).max()       # (the density moved ten orders above the bar)
    gc.close(); dev.close()


def test_mass_is_conserved_in_a_closed_box_where_the_wall_flux_vanishes():
    """... and with the `reduced` stencil, whose patch-face gradients are nf * snGrad, the walls are tight: the mass of tet433 is constant to
    1e-13 over 20 steps (separate kernels: the fused step serves GaussVolPoint only)"""
    mass_is_constant_with_the_reduced_stencil("tet433")


def mass_is_constant_with_the_reduced_stencil(kind):
    mesh, dev, gc, rho0 = _closed_box(kind, "reduced", "kernels")
    V = mesh.array("V")
    m0 = float((V * gc.field("rho")).sum())
    gc.step(20)
    m1 = float((V * gc.field("rho")).sum())
    print(f"unstructured mass conservation {kind} reduced: {abs(m1 - m0) / m0:.3e}")
    assert abs(m1 - m0) <= 1e-13 * m0, (m1 - m0) / m0
    assert np.abs(gc.field("rho") - rho0).max() > 1e-4 * np.abs(rho0).max()       # (the density moved ten orders above the bar)
    gc.close(); dev.close()
