"""The kernel families beside the step kernels on tetrahedra, prisms and prisms + hexahedra (tests/unstructured.py).

tests/test_unstructured_gpu.py holds the fvsc operators, the explicit step, adjustTimeStep, explicit QHDFoam and explicit shards to the oracle
on these meshes.  Here: the species (explicit, implicitDiffusion, on shards), varScModel7, QHDFoam's default branch (implicitDiffusion true),
QHDFoam and QGDFoam-implicit on shards, symmetry patches and cyclic patches.  The run monitors and scalarTransportQHDFoam have their rows in
their own files (tests/test_unstructured_meshes.py::test_every_family_has_an_unstructured_row lists them all).  Every one of these walks
per-cell face tables or per-point cell rows that a (split) hexahedron does not exercise: rows of 4 and 5 entries padded to their stride,
both lengths in one wavefront (mix643), point rows of 24 (tetrahedra) and 12 (prisms) cells, ghost layers longer than the owned range.

Nothing is restated: builders, references, bars and conditions are those of the hexahedral files, imported.  Where a hexahedral test's body
is a function of its mesh name alone it is CALLED on these meshes (hexahedral_body), so that no condition of it can drift; the error figures
it prints are collected for this file's one line per family, mesh and arm (pytest -s):

    unstructured <family> <tag>: worst <error> (<which>) bar <bar>

Bars: species 1e-12 (test_species_case_gpu), species implicit 1e-10 (test_species_implicit_case_gpu), sensor 1e-12 cSc1 and the muQGD
identity 1e-14, states 1e-10 (test_var_sc_model_gpu), QHDFoam implicit 1e-9 with solves below 1e-13 (test_qhd_implicit), QHD shards 1e-8
(test_qhd_sharded), implicit shards 1e-10 (test_implicit_sharded), symmetry and cyclic 1e-10 against the oracle, conservation 1e-13.

The 2:1 refined boxes (unstructured.REFINED) have rows here too -- species, the varScModel7 sensor, QHDFoam with implicitDiffusion true, the
range cuts of the iterative branches: what they bring is the other end of the per-cell walks, cells of 9 to 24 faces beside cells of 6
(tests/test_refined_cells_gpu.py has the table of loops and rows)."""
import functools
import re

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L, qhdfoam
from qgdsolver_amd.halo import ImplicitShard, ImplicitStepper, LocalWorld, QhdStepper

import cases
import unstructured
import test_implicit_sharded as ish
import test_qhd_sharded as qsh
import test_species_case_gpu as sp
import test_species_halo_gpu as shalo
import test_species_implicit_case_gpu as si
import test_symmetry_patches as sym
import test_var_sc_model_gpu as tv
from oracle import OracleCase, OracleQhdCase
from qhd_shards import gather, range_shards
from species_ref import SpeciesReplay
from test_cyclic_patches import OraclePeriodic, conserved
from test_partition import mixed_bcs
from test_qhd_case import cavity_bcs, initial, options as qhd_options
from test_qhd_implicit import TIGHT, run_oracle as run_qhd_oracle
from test_species_case import flow_fields, smooth_composition
from test_unstructured_gpu import EXPLICIT, MOST_FACES, VALENCE
from test_unstructured_meshes import PERIODIC_KINDS, PERIODIC_OPT, conservation_defect, periodic_fields, periodic_mesh
from util import assert_path, make_mesh, oracle_mesh_of, param_rows, rel_err

pytestmark = pytest.mark.gpu

G, SP, SY = L.PATCH_GENERIC, L.PATCH_SYMMETRYPLANE, L.PATCH_SYMMETRY


def report(family, tag, worst, bar):
    print(f"unstructured {family} {tag}: worst {max(worst.values()):.3e} ({max(worst, key=worst.get)}) bar {bar:g}")


def mesh_property(kind):
    """what makes the mesh worth running: vertices of 24 / 12 cells, cells of 4 / 5 / 5 + 6 faces, and on mix643 both face counts within
    one slice of 64 cells -- prisms and hexahedra share the wavefronts of every one-lane-per-cell walk.  The refined kinds: cells of 24
    faces (three full passes of a loop that takes eight faces per pass), and at least three face counts within one slice of 64 cells"""
    if kind in unstructured.REFINED:
        per_cell = unstructured.faces_per_cell(unstructured.refined_primitives(kind))
        assert int(per_cell.max()) == MOST_FACES[kind] == 24 and int(per_cell.min()) == 6
        assert any(len(set(per_cell[i:i + 64])) >= 3 for i in range(0, per_cell.size, 64))
        return
    prim = unstructured.primitives(kind)
    assert int(unstructured.point_valence(prim).max()) == VALENCE[kind] > 8
    per_cell = unstructured.faces_per_cell(prim)
    assert sorted(set(per_cell)) == {"tet": [4], "prism": [5], "mix": [5, 6]}[kind.rstrip("0123456789")]
    if kind == "mix643":
        assert any({5, 6} <= set(per_cell[i:i + 64]) for i in range(0, per_cell.size, 64))


def morton(kind):
    g = make_mesh(kind)
    g.renumber(g.morton_order())
    return g


def ghosts_outnumber_owned(g, world):
    """on at least one rank of the range cut the vertex-connected ghost layer is longer than the owned range"""
    counts = []
    for r in range(world):
        cg = g.shard(world, r).array("cellGlobal")
        own = (cg >= (g.nCells * r) // world) & (cg < (g.nCells * (r + 1)) // world)
        counts.append((int(own.sum()), int((~own).sum())))
    return any(ghost > owned for owned, ghost in counts), counts


_FIGURE = re.compile(r"(?<![\w.+-])(\d\.\d{3}e[-+]\d{2})(?![\w.])")


def hexahedral_body(capsys, test_fn, *args):
    """the body of a hexahedral file's test run on one of these meshes: its own builders, conditions and bars.  Returns the error figures
    it printed ('%.3e'), each keyed by the text in front of it; the text itself goes on to the terminal"""
    capsys.readouterr()
    try:
        test_fn(*args)
    finally:
        text = capsys.readouterr().out
        print(text, end="")
    worst = {}
    for line in text.splitlines():
        at = 0
        for m in _FIGURE.finditer(line):
            worst[line[at:m.start()].strip(" ,:|")] = float(m.group(1))
            at = m.end()
    assert worst, (test_fn.__name__, args, "printed no error figure")
    return worst


# ---- 1. species, explicit ----------------------------------------------------------------------------------------------------------------
SPECIES_ROWS = [("tet433", "GaussVolPoint"), ("mix643", "GaussVolPoint"), ("prism543", "reduced"), ("ref533", "GaussVolPoint")]
SPECIES_OPT = dict(deltaT=1e-3, mu=1e-3)


@pytest.mark.parametrize("adjust", [0, 1])
@pytest.mark.parametrize("kind,scheme", SPECIES_ROWS)
def test_species_explicit_match_the_replay(kind, scheme, adjust, capsys):
    """test_species_case_gpu.test_parity_with_the_replay: phiJmY, diffusiveFlux, Y and Y.boundary after one step, Y after three (1e-12), min Y > 0,
    the flow's rho at 1e-10; caseSpeciesPointKernel on point rows of 24 / 12 cells, caseSpeciesCellKernel on cells of 4 / 5 / 5 + 6 faces"""
    mesh_property(kind)
    worst = hexahedral_body(capsys, sp.test_parity_with_the_replay, kind, scheme, None, flow_fields, SPECIES_OPT, adjust)
    report("species explicit", (kind, scheme, "adjust", adjust, "kernels"), worst, sp.TOL)


def species_batch_edge(kind):
    """test_species_case_gpu.test_batch_edges with batchWidth + 1 transported species: the second register batch holds one species and walks
    the same rows"""
    mesh_property(kind)
    probe_dev = q.Device(q.PolyMesh.box(2, 2, 2), fused_tables=False)
    probe = q.QGDFoamCase(probe_dev, q.default_options())
    W = probe.species_info()["batchWidth"]
    probe.close(); probe_dev.close()
    assert W >= 2
    n_active, inert = W + 1, 1
    Sc = [0.5 + 0.25 * i for i in range(n_active + 1)]
    inlet = [0.4 / n_active] * (n_active + 1)
    inlet[inert] = 0.6
    mesh, dev, gc, oc, rep = sp.build(kind, "GaussVolPoint", None, flow_fields, SPECIES_OPT, sp.many_species(n_active, inert), inert, Sc, inlet, keep=True)
    assert gc.species_info()["nSpecies"] == n_active + 1
    gc.step(1)
    rep.step(1)
    sp.compare_species(gc, rep, "diffusiveFlux", ("batch", n_active))
    worst = {f"diffusiveFlux {i}": rel_err(gc.species_field(i, "diffusiveFlux"), rep.diffusiveFlux[i]) for i in range(rep.n)}
    gc.step(2)
    rep.step(2)
    sp.compare_species(gc, rep, "Y", ("batch", n_active))
    worst.update({f"Y {i}": rel_err(gc.species_field(i, "Y"), rep.Y[i]) for i in range(rep.n)})
    assert min(float(y.min()) for y in rep.Y) > 0.0
    assert_path(gc, "kernels", "batch edge")
    report("species explicit", (kind, "GaussVolPoint", f"{n_active} transported species", "kernels"), worst, sp.TOL)
    gc.close(); dev.close()


def test_species_batch_edge_on_tetrahedra():
    """... on tet433: point rows of 24 cells"""
    species_batch_edge("tet433")


SPECIES_SHARDS = ("tet433", "GaussVolPoint", 3, 6)          # mesh, stencil, world, species (five transported: two register batches)


@functools.lru_cache(maxsize=None)
def species_shard_reference():
    """test_species_halo_gpu.reference on the Morton-ordered tetrahedra: the unsharded device case with species after its STEPS steps, anchored
    against the host replay (1e-12, min Y > 0); formed once, read by both phase orders, never changed"""
    kind, stencil, _, nS = SPECIES_SHARDS
    g = morton(kind)
    bc_fn = shalo.inlet_bcs(g)
    Y_fn, Sc, inlet = shalo.COMPOSITIONS[nS]
    C = g.array("C").reshape(-1, 3)
    options = q.default_options(stencil=stencil, **SPECIES_OPT)
    om = oracle_mesh_of(g)
    dev = q.Device(g, fused_tables=False)
    gc, oc = q.QGDFoamCase(dev, options), OracleCase(om, options)
    for case in (gc, oc):
        bc_fn(case)
    Y0 = Y_fn(C)
    shalo.put_species(gc, Y0, Sc, inlet)

    def fresh():
        o2 = OracleCase(om, options)
        bc_fn(o2)
        o2.set_fields(*flow_fields(C))
        return o2
    rep = SpeciesReplay(g, om, oc, stencil, Y0, shalo.INERT, ScNumbers=Sc, bcs=[{0: ("fixedValue", inlet[i])} for i in range(nS)], fresh=fresh)
    for case in (gc, oc):
        case.set_fields(*flow_fields(C))
    assert_path(gc, "kernels", SPECIES_SHARDS)
    gc.step(shalo.STEPS)
    rep.step(shalo.STEPS)
    out = {f: gc.field(f) for f in shalo.FLOW}
    out["Y"] = [gc.species_field(i) for i in range(nS)]
    out["Yb"] = [gc.species_field(i, "Y.boundary") for i in range(nS)]
    anchor = {f"Y {i}": rel_err(out["Y"][i], rep.Y[i]) for i in range(nS)}
    report("species shards", SPECIES_SHARDS + ("unsharded device vs replay",), anchor, shalo.TOL)
    assert max(anchor.values()) <= shalo.TOL, anchor
    assert min(float(y.min()) for y in rep.Y) > 0.0 and min(float(y.min()) for y in out["Y"]) > 0.0
    gc.close(); dev.close()
    for v in out.values():
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
    return g, out


@pytest.mark.parametrize("layer_first", [False, True])
def test_species_on_range_shards_of_tetrahedra(layer_first):
    """test_species_halo_gpu.test_shards_match_the_unsharded_case on a range cut of the Morton-ordered tet433, world 3, plain phase order and
    boundary layer first: caseSpeciesHaloKernel and the species' cell roles where a shard has more ghost cells than owned ones"""
    kind, stencil, world, nS = SPECIES_SHARDS
    mesh_property(kind)
    g, ref = species_shard_reference()
    more, counts = ghosts_outnumber_owned(g, world)
    assert more, counts
    sh = shalo.Shards(g, world, stencil, shalo.inlet_bcs(g), flow_fields, SPECIES_OPT, nS)
    assert not sh.mid
    sh.check_counts()
    sh.run(shalo.STEPS, layer_first)
    got = sh.gathered()
    worst = {}
    for f in shalo.FLOW:
        worst[f] = float(np.abs(got[f] - ref[f]).max() / np.abs(ref[f]).max())
    for i in range(nS):
        worst[f"Y {i}"], worst[f"Y.boundary {i}"] = rel_err(got["Y"][i], ref["Y"][i]), rel_err(got["Yb"][i], ref["Yb"][i])
    report("species shards", SPECIES_SHARDS + ("layer first" if layer_first else "plain", "(owned, ghost)", counts), worst, shalo.TOL)
    assert all(v <= shalo.TOL for v in worst.values()), worst       # (NaN where no shard owned a cell or face: fails)
    for r, (s, c) in enumerate(zip(sh.shards, sh.cs)):             # every ghost cell holds, bit for bit, its original's composition
        cg, own = s.array("cellGlobal"), sh.owned(r)
        assert (~own).any()
        for i in range(nS):
            assert np.array_equal(c.species_field(i)[~own], got["Y"][i][cg[~own]]), (r, i)
    sh.close()


# ---- 2. species, implicitDiffusion ------------------------------------------------------------------------------------------------------------
SPECIES_IMPLICIT_ROWS = ["tet433", "mix643"]


@pytest.mark.parametrize("kind", SPECIES_IMPLICIT_ROWS)
def test_species_implicit_match_the_replay(kind):
    """the body of test_species_implicit_case_gpu.test_parity_with_the_replay (GaussVolPoint, fixed deltaT; 1e-10): the batched Chebyshev
    solves on matrix rows of 4 and of 5 + 6 entries -- and every solve of every step converged (test_controls_and_statistics there)"""
    mesh_property(kind)
    tag = (kind, "GaussVolPoint", 0)
    mesh, dev, gc, oc, rep = si.build(kind, "GaussVolPoint", None, flow_fields, dict(SPECIES_OPT, mu=2e-2), smooth_composition, 2, [0.7, 1.0, 1.0, 1.3],
                                      [0.3, 0.25, 0.3, 0.15], keep=True)                # (asserts the separate implicit kernels)
    worst = {}

    def compare(what, when):
        si.compare_species(gc, rep, what, tag + (when,))
        ref = {"Y": rep.Y, "phiJmY": rep.phiJmY, "diffusiveFlux": rep.diffusiveFlux, "Y.boundary": rep.Yb}[what]
        worst.update({f"{what} {i} {when}": rel_err(gc.species_field(i, what), ref[i]) for i in range(rep.n)})
    gc.step(1)
    rep.step(1)
    for what in ("phiJmY", "diffusiveFlux", "Y"):
        compare(what, "1 step")
    gc.step(2)
    rep.step(2)
    for what in ("Y", "Y.boundary"):
        compare(what, "3 steps")
    assert min(float(y.min()) for y in rep.Y) > 0.0     # the parity above does not hide behind the clip
    ig, io = gc.info(), oc.info()
    assert ig["steps"] == io["steps"] == 3 and abs(ig["deltaT"] - io["deltaT"]) <= si.TOL * io["deltaT"]
    si.compare_flow(gc, oc, tag)
    si.assert_separate_kernels(gc, tag)
    info = gc.species_implicit_info()
    assert sorted(info["species"]) == ["S0", "S1", "S3"] and info["unconvergedSteps"] == 0, info
    for name, s in info["species"].items():
        assert 0 < s["iterations"] < si.SOLVER["implicitMaxIter"] and s["final"] < 1e-13, (name, s)
    report("species implicitDiffusion", (kind, "GaussVolPoint", "kernels"), worst, si.TOL)
    print(f"unstructured species implicitDiffusion {kind}: Chebyshev iterations of the last step "
          f"{ {n: s['iterations'] for n, s in info['species'].items()} }, final residuals { {n: s['final'] for n, s in info['species'].items()} }")
    gc.close(); dev.close()


# ---- 3. varScModel7 ---------------------------------------------------------------------------------------------------------------------------
SENSOR_KINDS = ["tet433", "prism543", "mix643", "ref533"]
SENSOR_PARAMS = param_rows(tv.test_sensor_matches_the_restatement_after_set_fields, "params")
VAR_SC_RUNS = [(kind, arm) for kind in ("tet433", "mix643") for arm in ("fused", "kernels", "fusedAdjust", "implicitDiffusion")]


@pytest.mark.parametrize("params", SENSOR_PARAMS, ids=["unclipped", "clipped", "max-only+cellSet"])
@pytest.mark.parametrize("kind", SENSOR_KINDS)
def test_var_sc_sensor_matches_the_restatement(kind, params, capsys):
    """test_var_sc_model_gpu.test_sensor_matches_the_restatement_after_set_fields: varSc7Kernel, one lane per cell, eight face slots per pass
    masked by cfCount = 4 / 5 / 6 and sumP / cnt with cnt = 4 or 5 -- on ref533 up to three passes, cnt up to 24 -- (1e-12 cSc1; muQGD = p ScQGD tauQGD to 1e-14; sc_range() the extrema)"""
    assert len(SENSOR_PARAMS) == 3
    mesh_property(kind)
    worst = hexahedral_body(capsys, tv.test_sensor_matches_the_restatement_after_set_fields, kind, "GaussVolPoint", params)
    report("varScModel7 sensor", (kind, sorted(params.items())), worst, 1e-12 * params["cSc1"])


@pytest.mark.parametrize("kind,arm", VAR_SC_RUNS)
def test_var_sc_first_step_matches_the_oracle_fed_by_the_restatement(kind, arm, capsys):
    mesh_property(kind)
    worst = hexahedral_body(capsys, tv.test_first_step_matches_the_oracle_fed_by_the_restatement, kind, "GaussVolPoint", arm)
    report("varScModel7 first step", (kind, arm), worst, tv.STATE_TOL)


@pytest.mark.parametrize("kind,arm", VAR_SC_RUNS)
def test_var_sc_every_step_takes_the_restatement_of_its_pressures(kind, arm, capsys):
    """ten steps; the conditions of the hexahedral test as they are: a share of cells between the clips > 0.05, min rho > 0.3, pressures
    moved, the walls' patch pressures moved by the assembly (GaussVolPoint)"""
    mesh_property(kind)
    worst = hexahedral_body(capsys, tv.test_every_step_takes_the_restatement_of_the_pressures_it_starts_with, kind, "GaussVolPoint", arm)
    worst = {k: v for k, v in worst.items() if "ScQGD - ref" in k or "muQGD identity" in k}
    assert len(worst) == 2
    report("varScModel7 every step", (kind, arm), worst, 1e-12 * tv.PARAMS["cSc1"])


# ---- 6. QHDFoam, implicitDiffusion true: the reference's default ----------------------------------------------------------------------------------
QHD_IMPLICIT_ROWS = ["tet433", "mix643", "ref533"]
QHD_FIELDS = ("U", "T", "p", "phi", "U.boundary", "T.boundary", "p.boundary")


@pytest.mark.parametrize("kind", QHD_IMPLICIT_ROWS)
def test_qhd_implicit_branch_matches_oracle(kind):
    """the body of test_qhd_implicit.test_device_implicit_branch_matches_oracle (15 steps, 1e-9): four right-hand sides {Ux, Uy, Uz, T} of one
    matrix walk over rows of 4 and 5 + 6 entries, every solve below 1e-13, no unconverged step, and not the explicit branch in disguise"""
    mesh_property(kind)
    mesh = make_mesh(kind)
    opt = qhd_options("GaussVolPoint", deltaT=1e-3, mu=2e-2, pTol=1e-13, **TIGHT)
    U, T, p = initial(mesh)
    U = U + 1e-2 * np.random.default_rng(3).standard_normal(U.shape)
    oc = run_qhd_oracle(mesh, opt, 15, fields=(U, T, p))
    dev = q.Device(mesh)
    gc = qhdfoam.QHDFoamCase(dev, opt)
    cavity_bcs(gc, mesh)
    gc.set_fields(U, T, p)
    assert gc.implicit_info()["implicit"] and not gc.fused_info()["fusedAdvance"], (gc.implicit_info(), gc.fused_info())
    gc.step(15)
    worst = {}
    for f in QHD_FIELDS:
        ref = oc.field(f)
        worst[f] = float(np.abs(gc.field(f) - ref).max() / max(np.abs(ref).max(), 1e-300))
    report("QHDFoam implicitDiffusion", (kind, "GaussVolPoint", "kernels"), worst, 1e-9)
    assert all(v <= 1e-9 for v in worst.values()), (kind, worst)
    ii = gc.implicit_info()
    assert ii["implicit"] and ii["solver"] == "chebyshev" and ii["unconverged_steps"] == 0, ii
    solved = [n for n, s in ii["solves"].items() if s["iterations"] > 0]
    assert "T" in solved and len(solved) == 4, ii
    for n in solved:
        assert ii["solves"][n]["final"] < 1e-13, ii
    print(f"unstructured QHDFoam implicitDiffusion {kind}: Chebyshev iterations of the last step { {n: ii['solves'][n]['iterations'] for n in solved} }, "
          f"pressure iterations (device, oracle) {gc.info()['pIterations'], oc.info()['pIterations']}")
    ex = run_qhd_oracle(mesh, qhd_options("GaussVolPoint", deltaT=1e-3, mu=2e-2), 15, fields=(U, T, p))
    assert np.abs(ex.field("U") - oc.field("U")).max() > 1e-7 * np.abs(oc.field("U")).max()
    gc.close(); dev.close()


# ---- 7. shards of the iterative branches ----------------------------------------------------------------------------------------------------------
SHARD_CUTS = [("tet433", 3), ("tet866", 2), ("ref866", 2)]


@pytest.mark.parametrize("kind,world", SHARD_CUTS)
def test_qhd_shards_match_unsharded_device_and_oracle(kind, world, monkeypatch):
    """test_qhd_sharded.test_device_shards_match_unsharded_device_and_oracle on a range cut of the Morton-ordered tetrahedra (six steps, 1e-8
    against the unsharded device and the oracle, pFinalResidual < 1e-12).  QGD_MG_DENSE_MAX=64 (the knob of test_mg_cycle_gpu) makes the
    pressure matrix a hierarchy, which on shards is the one that spans the ranks: level 0 stays distributed, on rows whose ghost layer is
    longer than the owned range.  The pressure iteration counts are printed, not asserted."""
    monkeypatch.setenv("QGD_MG_DENSE_MAX", "64")
    mesh_property(kind)
    g = morton(kind)
    if kind == "tet433":
        more, counts = ghosts_outnumber_owned(g, world)
        assert more, counts
    shards = range_shards(g, world)
    ref_cell = g.nCells // 2
    opt = qhd_options("GaussVolPoint", deltaT=1e-3, precond=1, pRefCell=ref_cell, pRefValue=0.25, pTol=1e-12)
    fields = qsh.perturbed(g)
    steps = 6
    ref = qsh.run_unsharded_oracle(g, qhd_options("GaussVolPoint", deltaT=1e-3, precond=0, pRefCell=ref_cell, pRefValue=0.25, pTol=1e-13), cavity_bcs, fields, steps)
    gdev = q.Device(g)
    whole = qhdfoam.QHDFoamCase(gdev, opt)
    cavity_bcs(whole, g)
    whole.set_fields(*fields)
    whole.step(steps)
    assert whole.info()["mgLevels"] >= 2, whole.info()
    pairs = [qsh.make_device_shard_case(sh, opt, cavity_bcs, fields) for sh in shards]
    cs = [c for _, c in pairs]
    QhdStepper(LocalWorld(cs, [sh["peers"] for sh in shards])).step(steps)
    worst = {}
    for f, nc in qsh.FIELDS:
        got = gather(shards, cs, f, g.nCells, nc)
        for tag, want in (("unsharded device", whole.field(f)), ("oracle", ref.field(f))):
            worst[f"{f} vs {tag}"] = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
    report("QHDFoam shards", (kind, world, "distributed multigrid"), worst, 1e-8)
    assert all(v <= 1e-8 for v in worst.values()), (kind, world, worst)
    infos = [c.info() for c in cs]
    assert all(i["steps"] == steps and i["pFinalResidual"] < 1e-12 for i in infos), infos
    print(f"unstructured QHDFoam shards {kind} world {world}: pressure iterations of the last step: shards {[i['pIterations'] for i in infos]}, "
          f"unsharded device {whole.info()['pIterations']}, oracle {ref.info()['pIterations']}; multigrid levels: shards {[i['mgLevels'] for i in infos]}, "
          f"unsharded {whole.info()['mgLevels']}")
    for d, c in pairs:
        c.close(); d.close()
    whole.close(); gdev.close()


@pytest.mark.parametrize("kind,world", SHARD_CUTS)
def test_implicit_shards_match_unsharded_device_and_oracle(kind, world):
    """test_implicit_sharded.test_device_shards_match_unsharded_device_and_oracle on the same cuts (six steps, qgdFlux walls and their
    mid-assembly message, 1e-10 against the unsharded device and the oracle, solves below 5e-14)"""
    mesh_property(kind)
    g = morton(kind)
    shards = range_shards(g, world)
    fields = cases.box_initial_fields(g.array("C").reshape(-1, 3))
    steps = 6
    ref = ish.run_unsharded_oracle(g, mixed_bcs, fields, steps)
    gdev = q.Device(g)
    whole = q.QGDFoamCase(gdev, q.default_options(**ish.OPT))
    mixed_bcs(whole)
    whole.set_fields(*fields)
    whole.step(steps)
    assert whole.implicit_info()["implicit"], whole.implicit_info()
    pairs = []
    for sh in shards:
        dev = q.Device(sh["mesh"])
        c = q.QGDFoamCase(dev, q.default_options(**ish.OPT))
        mixed_bcs(c)
        cg = sh["cell_global"]
        c.set_fields(fields[0][cg], fields[1][cg], fields[2][cg])
        pairs.append((dev, c))
    cs = [c for _, c in pairs]
    ImplicitStepper(LocalWorld([ImplicitShard(c) for c in cs], [sh["peers"] for sh in shards], kinds=ish.KINDS)).step(steps)
    worst = {}
    for f, nc in ish.FIELDS:
        got = gather(shards, cs, f, g.nCells, nc)
        for tag, want in (("unsharded device", whole.field(f)), ("oracle", ref.field(f))):
            worst[f"{f} vs {tag}"] = float(np.abs(got - want).max() / np.abs(want).max())
    report("QGDFoam implicitDiffusion shards", (kind, world), worst, 1e-10)
    assert all(v <= 1e-10 for v in worst.values()), (kind, world, worst)
    for c in cs:
        ii = c.implicit_info()
        assert ii["unconverged_steps"] == 0 and all(s["final"] < 5e-14 for s in ii["solves"].values()), ii
    print(f"unstructured QGDFoam implicitDiffusion shards {kind} world {world}: Chebyshev iterations of the last step: shards "
          f"{[{n: s['iterations'] for n, s in c.implicit_info()['solves'].items()} for c in cs]}, unsharded "
          f"{ {n: s['iterations'] for n, s in whole.implicit_info()['solves'].items()} }")
    for d, c in pairs:
        c.close(); d.close()
    whole.close(); gdev.close()


# ---- 8. symmetry patches ------------------------------------------------------------------------------------------------------------------------
SYMMETRY_KINDS = ["tet433", "prism543"]
SYMMETRY_ARMS = {"fused": (EXPLICIT, "any"), "kernels": (EXPLICIT, False),
                 "implicitDiffusion": (dict(EXPLICIT, implicitDiffusion=1, implicitTol=1e-14, implicitMaxIter=2000), False)}


def symmetry_mesh(kind):
    """yMin a symmetryPlane, zMax a symmetry patch, the rest ordinary: buildPointConstraints meets patch points shared by up to 12 cells"""
    return make_mesh(kind, [G, G, SP, G, G, SY])


def normal_velocity(case, mesh):
    faces = sym.patch_faces(mesh, (SP, SY))
    Sf = mesh.array("Sf").reshape(-1, 3)
    n = Sf[faces] / np.linalg.norm(Sf[faces], axis=1)[:, None]
    return float(np.abs((case.field("U.boundary").reshape(-1, 3)[faces - mesh.nInternalFaces] * n).sum(axis=1)).max())


@pytest.mark.parametrize("arm", sorted(SYMMETRY_ARMS))
@pytest.mark.parametrize("kind", SYMMETRY_KINDS)
def test_symmetry_patches_match_the_oracle(kind, arm):
    """QGDFoam, ten steps under test_symmetry_patches.hostile_bcs ("none" and contradicting fixedValue requests: the patch type wins on the
    constraint patches), 1e-10 against the oracle; the device's patch velocity has no normal component (1e-15, as on hexahedra).
    Impermeability (boundary phiJm = 0) is NOT asserted here: under GaussVolPoint the patch-face gradient of p is not nf * snGrad where the
    cell centre does not lie on the face's normal, and the ORACLE's own boundary phiJm on a box closed by such patches is 3.9e-3 (tet433) and
    2.9e-3 (prism543) of max |phiJm|, its mass drifting by 2.2e-8 / 1.8e-7 over 20 steps -- the effect test_unstructured_gpu.py documents for
    slip walls.  On these meshes both are properties of the `reduced` stencil: the closed box below."""
    mesh_property(kind)
    opt, tables = SYMMETRY_ARMS[arm]
    mesh = symmetry_mesh(kind)
    assert sorted(int(t) for t in mesh.array("patchType")) == sorted([G, G, SP, G, G, SY])
    options = q.default_options(stencil="GaussVolPoint", **opt)
    dev = q.Device(mesh, fused_tables=tables)
    gc, oc = q.QGDFoamCase(dev, options), OracleCase(oracle_mesh_of(mesh), options)
    assert_path(gc, "fused" if arm == "fused" else "kernels", (kind, arm))
    U, T, p = sym.initial_state(mesh)
    for case in (gc, oc):
        sym.hostile_bcs(case)
        case.set_fields(U, T, p)
    rho0 = oc.field("rho").copy()
    gc.step(10)
    oc.step(10)
    worst = {name: rel_err(gc.field(name), oc.field(name)) for name in ("rho", "U", "p", "e", "U.boundary", "p.boundary")}
    report("symmetry QGDFoam", (kind, arm), worst, 1e-10)
    assert all(v <= 1e-10 for v in worst.values()), (kind, arm, worst)
    un = normal_velocity(gc, mesh)
    assert un <= 1e-15 and normal_velocity(oc, mesh) <= 1e-15, (kind, arm, un)
    assert np.abs(oc.field("rho") - rho0).max() > 1e-3 and np.isfinite(oc.field("rho")).all()
    if arm == "implicitDiffusion":
        assert gc.implicit_info()["implicit"] and gc.implicit_info()["unconverged_steps"] == 0, gc.implicit_info()
    gc.close(); dev.close()


@pytest.mark.parametrize("kind", SYMMETRY_KINDS)
def test_qhd_case_on_symmetry_patches(kind):
    """QHDFoam (the state and options of test_symmetry_patches.test_qhd_case_on_symmetry_planes), ten steps under hostile_bcs, 1e-10
    against the oracle; U_b . n = 0 on the device (1e-16, as on hexahedra)"""
    mesh_property(kind)
    mesh = symmetry_mesh(kind)
    opt = qhdfoam.qhd_options(stencil="GaussVolPoint", deltaT=2e-3, mu=1e-2, Pr=0.7, beta=3e-3, g=(-9.81, 0.0, 0.0), tauModel="constTau", Tau=1e-3,
                              implicitDiffusion=0, implicitTol=1e-13, pTol=1e-13)
    dev = q.Device(mesh)
    gc, oc = qhdfoam.QHDFoamCase(dev, opt), OracleQhdCase(oracle_mesh_of(mesh), opt)
    assert not gc.implicit_info()["implicit"]
    C = mesh.array("C").reshape(-1, 3)
    U = 0.05 * np.stack([np.sin(2 * np.pi * C[:, 0]) * np.cos(np.pi * C[:, 1]), 0.5 + 0 * C[:, 0], 0.3 * np.cos(np.pi * C[:, 2])], axis=1)
    for case in (gc, oc):
        sym.hostile_bcs(case)
        case.set_fields(U, 300.0 + 5.0 * C[:, 0], np.zeros(mesh.nCells))
    gc.step(10)
    oc.step(10)
    worst = {name: rel_err(gc.field(name), oc.field(name)) for name in ("U", "T", "p", "phi")}
    report("symmetry QHDFoam", (kind, "kernels"), worst, 1e-10)
    print(f"unstructured symmetry QHDFoam {kind}: pressure iterations of the last step (device, oracle) {gc.info()['pIterations'], oc.info()['pIterations']}")
    assert all(v <= 1e-10 for v in worst.values()), (kind, worst)
    assert normal_velocity(gc, mesh) <= 1e-16
    assert np.isfinite(oc.field("U")).all() and np.abs(oc.field("U") - U).max() > 1e-3
    gc.close(); dev.close()


def test_closed_box_of_symmetry_patches_is_tight_with_the_reduced_stencil():
    """tet433 closed by [SP, SP, SP, SP, SY, SY], `reduced` (separate kernels), 20 steps: no mass flux through any patch face (exactly) and
    the mass constant to 1e-13 (the oracle alone: 1.6e-16)"""
    mesh_property("tet433")
    mesh = make_mesh("tet433", [SP, SP, SP, SP, SY, SY])
    dev = q.Device(mesh, fused_tables=False)
    gc = q.QGDFoamCase(dev, q.default_options(stencil="reduced", **EXPLICIT))
    assert_path(gc, "kernels", "closed box")
    gc.set_fields(*sym.initial_state(mesh))
    V, nif = mesh.array("V"), mesh.nInternalFaces
    rho0 = gc.field("rho").copy()
    m0 = float((V * rho0).sum())
    through = 0.0
    for _ in range(4):
        gc.updateFluxes()
        through = max(through, float(np.abs(gc.field("phiJm")[nif:]).max()))
        assert np.abs(gc.field("phiJm")[:nif]).max() > 0
        gc.step(5)
    m1 = float((V * gc.field("rho")).sum())
    print(f"unstructured symmetry closed box tet433 reduced: mass drift {abs(m1 - m0) / m0:.3e} bar 1e-13, boundary |phiJm| max {through:.3e}, "
          f"U_b . n {normal_velocity(gc, mesh):.3e}")
    assert through == 0.0 and abs(m1 - m0) <= 1e-13 * m0, (through, (m1 - m0) / m0)
    assert normal_velocity(gc, mesh) <= 1e-15
    assert np.abs(gc.field("rho") - rho0).max() > 1e-4 * np.abs(rho0).max()
    gc.close(); dev.close()


# ---- 9. cyclic patches --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["fused", "kernels"])
@pytest.mark.parametrize("kind", sorted(PERIODIC_KINDS))
def test_triply_periodic_case_matches_the_oracle_and_conserves(kind, arm):
    """all six sides cyclic (tests/test_unstructured_meshes.py: 26 slots, copies of tetrahedra / prisms behind sides, edges and corners):
    qgd_case_step, the library refreshing the copies itself, against OraclePeriodic after 1 + 9 steps (1e-10); mass, momentum and energy
    of the real cells constant to 1e-13; the copies bit-equal to their originals"""
    mesh_property(kind)
    g, ext = periodic_mesh(kind)
    assert ext.halo_slots == 26 and ext.nCells == PERIODIC_KINDS[kind]
    opt = q.default_options(stencil="GaussVolPoint", **PERIODIC_OPT)
    U, T, p = periodic_fields(g.array("C").reshape(-1, 3))
    per = OraclePeriodic(ext, opt)
    per.set_fields(U, T, p)
    dev = q.Device(ext, fused_tables="any" if arm == "fused" else False)
    gc = q.QGDFoamCase(dev, opt)
    fi = gc.fused_info()          # (util.assert_path counts the internal faces of the device's mesh, copies among themselves included)
    assert fi["fused"] == (arm == "fused") and not fi["fusedAdjust"], (kind, arm, fi)
    assert arm != "fused" or (fi["blocks"] >= 1 and fi["facesComputed"] >= g.nFaces), (kind, fi)      # every face of a real cell is computed
    cg, n, V = ext.array("cellGlobal"), g.nCells, g.array("V")
    gc.set_fields(U[cg], T[cg], p[cg])
    before, rho0 = conserved(gc, V, n), gc.field("rho")[:n].copy()
    worst = {}
    for chunk in (1, 9):
        gc.step(chunk)
        per.step(chunk)
        for f in ("rho", "U", "p", "e"):
            a, b = gc.field(f)[:n], per.field(f, n)
            worst[f"{f} +{chunk}"] = float(np.abs(a - b).max() / np.abs(b).max())
        assert np.array_equal(gc.field("rho")[n:], gc.field("rho")[cg[n:]])
    defect = conservation_defect(before, conserved(gc, V, n))
    report("cyclic", (kind, arm), worst, 1e-10)
    print(f"unstructured cyclic {kind} {arm}: change of mass, momentum x y z, energy over 10 steps {defect} bar 1e-13")
    assert all(v <= 1e-10 for v in worst.values()), (kind, arm, worst)
    assert (defect <= 1e-13).all(), (kind, arm, defect)
    assert np.abs(gc.field("rho")[:n] - rho0).max() > 1e-3
    gc.close(); dev.close()


def test_mixed_halves_are_refused_by_name_on_the_device_path():
    """mix643 periodic in x: the library's unroll, which every periodic device goes through, refuses it by name"""
    with pytest.raises(q.QgdError, match="do not match point by point"):
        make_mesh("mix643", [L.PATCH_CYCLIC, L.PATCH_CYCLIC, G, G, G, G]).unroll_cyclic()
