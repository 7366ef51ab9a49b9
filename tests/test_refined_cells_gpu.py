"""The kernel families on boxes with one level of 2:1 refinement (tests/unstructured.py REFINED: ref533, ref866, the quadtree ref2d87).

What refineMesh and snappyHexMesh produce and no other mesh of the suite has: a coarse hexahedron between refined ones has 24 faces (one
refined side: 9), beside the 6 of its neighbours' children in the same 64 cells; an unsplit face next to a split edge has 5 to 8 points, three
of them collinear, and under GaussVolPoint takes the nf (x) snGrad fallback (FK_OTHER) beside ordinary quadrilaterals of the same cell; the
hanging vertices have 5 or 6 cells; the linear weights across a coarse / fine face are near 1/3 and 2/3.  The most faces of a cell elsewhere:
10 (box654_tri, box654_poly), so no per-cell loop that takes eight faces per pass ever took a third pass, or a pass count with n % 8 == 0.

Most rows are rows of the files that hold their family's parametrisation; this file holds what has none there.  Where each loop is reached
with the 24-face cell of ref533 (or the 24 such cells of ref866), "file::test [row]":

    cellGradGauss (qgd_stencil_dev.hpp)             test_implicit_diffusion::test_device_implicit_branch_matches_oracle [ref533, kernels and fused];
                                                    test_unstructured_gpu::test_qhd_case_matches_oracle [ref533 kernels]
    qhdCellUpdateKernel (qgd_qhd.hip)               test_unstructured_gpu::test_qhd_case_matches_oracle [ref533 kernels / deep / deep plain, ref866 kernels]
    qhdImplicitRhsKernel (qgd_qhd.hip)              test_unstructured_families_gpu::test_qhd_implicit_branch_matches_oracle [ref533]
    assembleKernel (qgd_poisson.hip)                test_unstructured_gpu::test_qhd_case_matches_oracle [every ref533 / ref866 row]
    applyKernel, the row walk (qgd_poisson.hip)     the same rows (every pressure iteration); the cycle itself: test_mg_cycle_gpu [refined, double refined]
    implCellUKernel (qgd_implicit.hip)              test_implicit_diffusion::test_device_implicit_branch_matches_oracle [ref533 kernels];
                                                    here::test_fused_implicit_assembly_is_the_separate_kernels_to_rounding (its reference arm)
    implCellEKernel (qgd_implicit.hip)              the same two (both arms: the e system is assembled by this kernel on either)
    scalarRhsKernel (qgd_scalar.hip)                test_scalar_transport_case::test_device_case_steps_like_the_restatement [ref533 x 2]
    varSc7Kernel (qgd_varsc.hip)                    test_unstructured_families_gpu::test_var_sc_sensor_matches_the_restatement [ref533 x 3]
    qhdMonitorCellKernel (qgd_qhd_monitor.hip)      test_qhd_monitor_gpu::test_patch_totals_against_the_face_fields [ref533] (the continuity rows)
    fusedFaceCellKernel, the template tail          test_unstructured_gpu::test_update_fluxes_and_steps [ref533 / ref866, fused]: entries 7 .. 24 of an own
      (i < KE ? sE[..] : ent[i * 128], capE = 24)   cell come from the template in memory; test_adjust_time_step [ref533 fusedAdjust] (ADJ),
                                                    test_implicit_diffusion [ref533 fused] (IMPL), test_fused_packed_geometry_gpu::
                                                    test_refined_cells_whichever_way_the_rule_decides (bit for bit against three kernels), and the
                                                    uniform-flow and mass-balance checks below; the tables themselves: test_fused_blocks_host
    the ELL rows of the implicit matrix, 24 beside 6   the implicitDiffusion rows above; test_unstructured_families_gpu::
                                                    test_implicit_shards_match_unsharded_device_and_oracle [ref866, 2]
    the pressure matrix, rows of 25 entries         the QHDFoam rows above; test_qhd_shards_match_unsharded_device_and_oracle [ref866, 2]

The rest of section "which family runs where" is tests/test_unstructured_meshes.py::test_every_family_has_an_unstructured_row, which fails
without a GPU when one of these rows is dropped.  Bars are those of the hexahedral files (tests/test_unstructured_gpu.py lists them); each
test names the path it takes, asserts it, and prints its worst error (pytest -s).

Two checks do not lean on the oracle: a uniform flow stays uniform (1e-13 relative, a hundred times the oracle's own 7e-16: one missing or
doubled face entry of a coarse cell moves it by about 1e-4), and the mass of a box closed by slip walls changes by what goes through the
walls and by nothing else (1e-13 of the mass).

Not on these meshes: SRFQHDFoam, cyclic patches (the two sides of a checkerboard do not match point by point), symmetry patches, more than
one level of refinement."""
import numpy as np
import pytest

import qgdsolver_amd as q

import cases
import test_unstructured_families_gpu as families
import test_unstructured_gpu as tu
from test_case_parity_gpu import empty_z_bcs, mixed_box_bcs, plane_init
from util import assert_path, make_mesh

pytestmark = pytest.mark.gpu

UNIFORM = ((0.3, 0.2, -0.1), 1.0, 1.0)          # U, T, p


# ---- the quadtree: cells of 6 to 10 faces, z faces of 5 to 8 points, two solved directions ------------------------------------------------
@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("scheme", ["GaussVolPoint", "reduced", "leastSquares"])
def test_fvsc_operators_on_the_quadtree(scheme, entry):
    """test_unstructured_gpu.test_fvsc_operators_match_oracle (all of OPS, 1e-12) on ref2d87, with leastSquares too"""
    assert make_mesh("ref2d87").nGeometricD == 2
    tu.test_fvsc_operators_match_oracle("ref2d87", scheme, entry)


@pytest.mark.parametrize("scheme", ["GaussVolPoint", "reduced", "leastSquares"])
def test_explicit_step_on_the_quadtree(scheme):
    """test_unstructured_gpu.test_update_fluxes_and_steps on ref2d87 (z empty, the pulse of plane_init): the separate kernels, which are
    what steps a two-dimensional case (asserted), with the three stencils"""
    tu.test_update_fluxes_and_steps("ref2d87", scheme, empty_z_bcs, "kernels", init_fn=plane_init)


# ---- the explicit step: the fused kernel is the three kernels bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("bc_fn", [None, mixed_box_bcs], ids=["default", "mixed"])
@pytest.mark.parametrize("kind", ["ref533", "ref866"])
def test_fused_step_is_the_three_kernels_bit_for_bit(kind, bc_fn):
    """the cases of test_unstructured_gpu.test_update_fluxes_and_steps [ref533 / ref866], which hold either arm to the oracle: here the two
    arms against each other after 25 steps, np.array_equal -- the same inlined expressions in the same order, whatever the mesh; a face
    entry of a 24-face cell read from the wrong place of the template tail differs in the first step"""
    mesh = make_mesh(kind)
    fields = cases.box_initial_fields(mesh.array("C").reshape(-1, 3))
    out = {}
    for arm in ("kernels", "fused"):
        dev = q.Device(mesh, fused_tables="any" if arm == "fused" else False)
        gc = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", **tu.EXPLICIT))
        assert_path(gc, arm, (kind, "bit for bit"))
        tu.long_vertex_rows(kind, dev if arm == "fused" else None)
        if bc_fn:
            bc_fn(gc)
        gc.set_fields(*fields)
        rho0 = gc.field("rho").copy()
        gc.step(25)
        out[arm] = {f: gc.field(f).copy() for f in ("rho", "U", "p", "e", "rhoE", "U.boundary", "p.boundary")}
        gc.close(); dev.close()
    worst = {f: float(np.abs(out["fused"][f] - out["kernels"][f]).max()) for f in out["fused"]}
    print(f"refined explicit {kind} {'mixed' if bc_fn else 'default'} fused vs kernels: worst {max(worst.values()):.3e} ({max(worst, key=worst.get)}) bar 0")
    for f in worst:
        assert np.isfinite(out["fused"][f]).all() and np.array_equal(out["fused"][f], out["kernels"][f]), (kind, f, worst[f])
    assert np.abs(out["fused"]["rho"] - rho0).max() > 1e-4 * np.abs(rho0).max()       # (something happened)


# ---- implicitDiffusion: the block-fused assembly of the U systems against the separate kernels ---------------------------------------------
def test_fused_implicit_assembly_is_the_separate_kernels_to_rounding():
    """test_implicit_diffusion.test_block_fused_assembly_of_the_u_systems_is_the_separate_kernels_to_rounding on ref533 under mixed_box_bcs:
    states, phiTauMC and phiSigmaDotU to 1e-13 of each field's scale after six steps, and the same iteration counts of every solve.  (Both
    arms against the oracle, 1e-10: the ref533 rows of test_implicit_diffusion.test_device_implicit_branch_matches_oracle.)"""
    mesh = make_mesh("ref533")
    out, info = {}, {}
    for arm in ("kernels", "fused"):
        dev = q.Device(mesh, fused_tables="any" if arm == "fused" else False)
        gc = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", implicitDiffusion=1, deltaT=2e-4, mu=2e-2))
        fi = gc.fused_info()
        assert fi["fusedImplicit"] == (arm == "fused") and not fi["fused"], (arm, fi)        # the arm under test is the path that runs
        tu.long_vertex_rows("ref533", dev if arm == "fused" else None)
        mixed_box_bcs(gc)
        gc.set_fields(*cases.box_initial_fields(mesh.array("C").reshape(-1, 3)))
        gc.step(6)
        out[arm] = {n: gc.field(n).copy() for n in ("rho", "U", "p", "e", "rhoE", "phiTauMC", "phiSigmaDotU", "U.boundary", "p.boundary")}
        info[arm] = gc.implicit_info()
        gc.close(); dev.close()
    a, b = out["kernels"], out["fused"]
    worst = {k: float(np.abs(a[k] - b[k]).max() / max(np.abs(a[k]).max(), 1e-300)) for k in a}
    print(f"refined implicitDiffusion ref533 fused IMPL assembly vs separate kernels: worst {max(worst.values()):.3e} ({max(worst, key=worst.get)}) bar 1e-13; "
          f"iterations of the last step { {n: s['iterations'] for n, s in info['fused']['solves'].items()} }")
    assert all(np.isfinite(b[k]).all() for k in b) and all(v <= 1e-13 for v in worst.values()), worst
    assert info["kernels"]["solves"] == info["fused"]["solves"] and info["fused"]["unconverged_steps"] == 0, info
    assert np.abs(a["phiTauMC"]).max() > 0 and np.abs(a["phiSigmaDotU"]).max() > 0


# ---- species: a batch edge on cells of 24 faces -----------------------------------------------------------------------------------------
def test_species_batch_edge_on_refined_cells():
    """test_unstructured_families_gpu.species_batch_edge (batchWidth + 1 transported species, 1e-12 against the replay) on ref533: the second
    register batch of caseSpeciesCellKernel walks the same face rows of 6 to 24 entries"""
    families.species_batch_edge("ref533")


# ---- two checks that do not lean on the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ["fused", "kernels"])
def test_uniform_flow_stays_uniform(arm):
    """U = (0.3, 0.2, -0.1), T = p = 1 on ref533, every patch zeroGradient, 20 steps: every cell keeps rho, U, p and e to 1e-13 of the
    field's size.  The fluxes of a uniform state cancel over a closed cell only if every face of the cell is there once, with its sign: a
    coarse cell's 24 entries in three passes, the fused kernel's template tail, and the hanging-node faces' fallback gradient, which
    must vanish as the ordinary one does"""
    mesh = make_mesh("ref533")
    dev = q.Device(mesh, fused_tables="any" if arm == "fused" else False)
    gc = q.QGDFoamCase(dev, q.default_options(stencil="GaussVolPoint", **tu.EXPLICIT))
    assert_path(gc, arm, ("ref533", "uniform"))
    tu.long_vertex_rows("ref533", dev if arm == "fused" else None)
    n = mesh.nCells
    gc.set_fields(np.tile(UNIFORM[0], (n, 1)), np.full(n, UNIFORM[1]), np.full(n, UNIFORM[2]))
    before = {f: gc.field(f).copy() for f in ("rho", "U", "p", "e")}
    gc.step(20)
    worst = {f: float(np.abs(gc.field(f) - before[f]).max() / np.abs(before[f]).max()) for f in before}
    print(f"refined uniform flow ref533 {arm}: worst {max(worst.values()):.3e} ({max(worst, key=worst.get)}) bar 1e-13")
    assert all(np.isfinite(gc.field(f)).all() for f in before) and all(v <= 1e-13 for v in worst.values()), (arm, worst)
    assert gc.info()["steps"] == 20
    gc.close(); dev.close()


def test_mass_balance_of_a_refined_box_closed_by_slip_walls_on_the_fused_step():
    """test_unstructured_gpu.test_mass_balance_of_a_box_closed_by_slip_walls_on_the_fused_step on ref533: per step and over 20 steps the
    mass changes by what the step's own mass flux carries through the walls, to 1e-13 of the mass -- every internal face, the four
    quarters of a coarse side among them, gives one cell what it takes from the other"""
    tu.mass_balance_through_the_walls("ref533")


def test_mass_is_conserved_in_a_refined_box_where_the_wall_flux_vanishes():
    """... and constant to 1e-13 under `reduced` on the separate kernels, whose wall flux vanishes"""
    tu.mass_is_constant_with_the_reduced_stencil("ref533")
