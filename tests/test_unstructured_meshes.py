"""The generated tetrahedral / prismatic / mixed meshes (tests/unstructured.py) are what the device tests need them to be (CPU): point valences
beyond the eight register slots of the fused kernels' vertex walk, cells with fewer than six faces, prisms and hexahedra in one wavefront,
OpenFOAM face order (qgd_mesh_create accepts them), closed cells of positive volume, Morton-ordered shards, and an oracle that stays finite
and positive on them.  The same for the boxes with one level of 2:1 refinement (unstructured.REFINED): cells of 6 to 24 faces side by side,
faces of 5 to 8 points with their hanging nodes exactly on the edge they hang on, and an oracle that keeps a uniform flow uniform."""
import collections

import numpy as np
import pytest

import qgdsolver_amd as q
from qgdsolver_amd import _lib as L

import cases
import unstructured
from oracle import OracleCase
from util import make_mesh, oracle_mesh_of

EXPECT = {  # kind: (cells, maximum point valence, faces per cell)
    "tet433": (216, 24, [4]),
    "tet866": (1728, 24, [4]),
    "prism543": (120, 12, [5]),
    "mix643": (108, 12, [5, 6]),
}


# kind: (cells, faces per cell: count, points per face, point valences that must occur, the largest, nGeometricD, box (volume, surface, height))
EXPECT_REFINED = {
    "ref533": (143, {6: 125, 9: 5, 18: 12, 24: 1}, [4, 5, 7], {5, 6, 8}, 8, 3, (1.0, 6.0, 1.0)),
    "ref866": (918, {6: 810, 9: 18, 15: 4, 18: 22, 21: 40, 24: 24}, [4, 5, 6, 7, 8], {5, 6, 8}, 8, 3, (1.0, 6.0, 1.0)),
    "ref2d87": (110, {6: 89, 7: 4, 9: 10, 10: 7}, [4, 5, 7, 8], {3, 4}, 4, 2, (0.1, 2.4, 0.1)),
}


def test_the_four_kinds_are_the_ones_listed():
    assert sorted(unstructured.KINDS) == sorted(EXPECT)
    assert sorted(unstructured.REFINED) == sorted(EXPECT_REFINED) and not set(unstructured.REFINED) & set(unstructured.KINDS)


@pytest.mark.parametrize("kind", sorted(EXPECT_REFINED))
def test_refined_face_counts_hanging_nodes_order_and_geometry(kind):
    cells, histogram, face_points, valences, most, nD, (volume, surface, height) = EXPECT_REFINED[kind]
    a = unstructured.refined_primitives(kind)
    mesh = make_mesh(kind)          # qgd_mesh_create runs HostMesh::check: sizes, owner < neighbour, upper-triangular order, contiguous patches
    assert mesh.nCells == cells == a["nCells"] and mesh.nGeometricD == nD and mesh.nPatches == 6
    per_cell = unstructured.faces_per_cell(a)
    assert dict(collections.Counter(per_cell.tolist())) == histogram
    assert sorted(set(np.diff(a["faceOffsets"]).tolist())) == face_points
    valence = unstructured.point_valence(a)
    print(f"{kind}: point valences {sorted(collections.Counter(valence.tolist()).items())}")
    assert valences <= set(valence.tolist()) and int(valence.max()) == most
    if kind == "ref533":
        assert len(set(per_cell[:64].tolist())) >= 3                # 6, 9 and 18 faces side by side in the first wavefront of every per-cell walk
        assert int(per_cell.max()) == 24 == 3 * 8                   # the enclosed coarse cell: three full passes of eight
    own, nei, nif = a["owner"], a["neighbour"], a["neighbour"].size
    key = own[:nif].astype(np.int64) * cells + nei
    assert np.all(nei > own[:nif]) and np.all(np.diff(key) > 0)    # sorted by (owner, neighbour), no face twice
    assert np.array_equal(a["patchStart"], nif + np.concatenate([[0], np.cumsum(a["patchSize"])[:-1]])) and a["patchSize"].min() > 0
    assert list(mesh.array("patchType")[4:]) == ([L.PATCH_EMPTY] * 2 if nD == 2 else [L.PATCH_GENERIC] * 2)
    V, Sf = mesh.array("V"), mesh.array("Sf").reshape(-1, 3)
    assert V.min() > 0 and abs(V.sum() - volume) <= 1e-13
    closed = np.zeros((cells, 3))
    np.add.at(closed, own, Sf)
    np.subtract.at(closed, nei, Sf[:nif])
    print(f"{kind}: cells closed to {np.abs(closed).max():.1e}, volume off by {abs(V.sum() - volume):.1e}")
    assert np.abs(closed).max() <= 1e-15
    C, Cf = mesh.array("C").reshape(-1, 3), mesh.array("Cf").reshape(-1, 3)
    assert np.all(np.einsum("ij,ij->i", Sf[:nif], C[nei] - C[own[:nif]]) > 0)
    for patch in range(6):
        sl = slice(a["patchStart"][patch], a["patchStart"][patch] + a["patchSize"][patch])
        axis, sign = patch // 2, (1.0 if patch % 2 else -1.0)
        far = (patch % 2) * (height if axis == 2 else 1.0)
        assert np.all(sign * Sf[sl, axis] > 0) and np.abs(Cf[sl, axis] - far).max() <= 1e-15
    assert abs(np.abs(Sf[nif:]).sum() - surface) <= 1e-13
    # every mid-edge node, hanging or not, is the midpoint of the edge it halves: exactly, not to rounding
    P, mid = a["points"].reshape(-1, 3), a["midEdges"]
    assert mid.shape[0] > 0 and np.array_equal(P[mid[:, 0]], 0.5 * (P[mid[:, 1]] + P[mid[:, 2]]))
    # ... and some of them hang: a face lists three collinear points of which the middle one is such a node
    fo, fp = a["faceOffsets"], a["facePoints"]
    is_mid = np.zeros(P.shape[0], dtype=bool)
    is_mid[mid[:, 0]] = True
    hanging = 0
    for f in np.nonzero(np.diff(fo) > 4)[0]:
        loop = fp[fo[f]:fo[f + 1]]
        for s in range(loop.size):
            before, here, after = loop[s - 1], loop[s], loop[(s + 1) % loop.size]
            if is_mid[here] and np.array_equal(P[here], 0.5 * (P[before] + P[after])):
                hanging += 1
    assert hanging >= int((np.diff(fo) > 4).sum())
    # internal faces of more than four points (GaussVolPoint's FK_OTHER: the nf (x) snGrad fallback) beside quadrilaterals of the same cell
    many = np.diff(fo)[:nif] > 4
    with_many, with_four = set(own[:nif][many]) | set(nei[many]), set(own[:nif][~many]) | set(nei[~many])
    print(f"{kind}: {int(many.sum())} of {nif} internal faces have more than four points, in {len(with_many)} cells")
    assert (many.sum() > 0 and with_many <= with_four) or kind == "ref2d87"      # (the quadtree's long faces are its empty z faces)


@pytest.mark.parametrize("kind", sorted(EXPECT))
def test_valence_face_counts_order_and_geometry(kind):
    cells, valence, nfaces = EXPECT[kind]
    a = unstructured.primitives(kind)
    mesh = make_mesh(kind)          # qgd_mesh_create runs HostMesh::check: sizes, owner < neighbour, upper-triangular order, contiguous patches
    assert mesh.nCells == cells == a["nCells"] and mesh.nGeometricD == 3 and mesh.nPatches == 6
    assert int(unstructured.point_valence(a).max()) == valence
    per_cell = unstructured.faces_per_cell(a)
    assert sorted(np.unique(per_cell)) == nfaces
    if kind == "mix643":
        assert sorted(np.unique(per_cell[:64])) == [5, 6]          # both shapes in the first wavefront of every per-cell walk
    own, nei, nif = a["owner"], a["neighbour"], a["neighbour"].size
    key = own[:nif].astype(np.int64) * cells + nei
    assert np.all(nei > own[:nif]) and np.all(np.diff(key) > 0)    # sorted by (owner, neighbour), no face twice
    assert np.array_equal(a["patchStart"], nif + np.concatenate([[0], np.cumsum(a["patchSize"])[:-1]])) and a["patchSize"].min() > 0
    V, Sf = mesh.array("V"), mesh.array("Sf").reshape(-1, 3)
    assert V.min() > 0 and abs(V.sum() - 1.0) <= 1e-13
    closed = np.zeros((cells, 3))
    np.add.at(closed, own, Sf)
    np.subtract.at(closed, nei, Sf[:nif])
    assert np.abs(closed).max() <= 1e-15                            # every cell's outward area vectors sum to nothing
    # area vectors point from owner to neighbour, and out of the box on the six sides (xMin, xMax, yMin, yMax, zMin, zMax)
    C, Cf = mesh.array("C").reshape(-1, 3), mesh.array("Cf").reshape(-1, 3)
    assert np.all(np.einsum("ij,ij->i", Sf[:nif], C[nei] - C[own[:nif]]) > 0)
    for patch in range(6):
        sl = slice(a["patchStart"][patch], a["patchStart"][patch] + a["patchSize"][patch])
        axis, sign = patch // 2, (1.0 if patch % 2 else -1.0)
        assert np.all(sign * Sf[sl, axis] > 0) and np.abs(Cf[sl, axis] - (patch % 2)).max() <= 1e-15
    assert abs(np.abs(Sf[nif:]).sum() - 6.0) <= 1e-13               # the boundary faces tile the unit box's surface


@pytest.mark.parametrize("kind,world", [("tet433", 3), ("tet866", 2), ("tet866", 3), ("ref866", 2), ("ref866", 3)])
def test_morton_ordered_shards(kind, world):
    g = make_mesh(kind)
    g.renumber(g.morton_order())
    seen = np.zeros(g.nCells, dtype=int)
    for r in range(world):
        s = g.shard(world, r)
        cg = s.array("cellGlobal")
        own = (cg >= (g.nCells * r) // world) & (cg < (g.nCells * (r + 1)) // world)
        seen[cg[own]] += 1
        assert 0 < (~own).sum() and s.halo_slots >= 1
    assert np.all(seen == 1)


# ---- cyclic patches: the six sides of the lattice paired, tetrahedra and prisms copied behind sides, edges and corners ----------------------
PERIODIC_KINDS = {"tet433": 816, "prism543": 410}      # kind: cells of the unrolled mesh.  (mix643: triangles face quadrilaterals, refused)
PERIODIC_OPT = dict(deltaT=2e-4, mu=2e-3)


def periodic_mesh(kind):
    """(the mesh with its six sides cyclic, its unrolled form).  The jitter of unstructured.lattice_points keeps the boundary points where
    they are, and every cube is cut the same way: the halves of a pair match point by point, triangle for triangle"""
    g = make_mesh(kind, [L.PATCH_CYCLIC] * 6)
    return g, g.unroll_cyclic()


def periodic_fields(C):
    """the state of test_cyclic_patches.test_triply_periodic_box_conserves_mass_momentum_and_energy"""
    from test_cyclic_patches import smooth_fields
    U, T, p = smooth_fields(C)
    U[:, 2] += 0.04 * np.sin(2 * np.pi * C[:, 1])
    return U, T + 0.03 * np.sin(2 * np.pi * C[:, 2]), p


def conservation_defect(before, after):
    """|change| of (mass, momentum x y z, energy) relative to (mass, mass, mass, mass, energy): test_cyclic_patches"""
    return np.abs(after - before) / np.array([before[0], before[0], before[0], before[0], before[4]])


@pytest.mark.parametrize("kind", sorted(PERIODIC_KINDS))
def test_triply_periodic_unroll_keeps_the_real_mesh_and_mirrors_its_sides(kind):
    """the assertions of test_cyclic_patches.test_unrolled_mesh_keeps_the_real_mesh_and_mirrors_its_sides, with all three directions paired:
    26 slots (6 sides, 12 edges, 8 corners), every real label kept, each slot's ghosts its partner's send list moved by one lattice vector"""
    g, ext = periodic_mesh(kind)
    assert np.array_equal(unstructured.primitives(kind)["patchType"], np.zeros(6))        # the cached primitives were not written
    n = g.nCells
    assert ext.nCells == PERIODIC_KINDS[kind] > n and np.array_equal(ext.array("cellGlobal")[:n], np.arange(n))
    assert np.array_equal(ext.array("points")[:3 * g.nPoints], g.array("points"))
    ps, pz, pty = ext.array("patchStart"), ext.array("patchSize"), ext.array("patchType")
    assert ext.nPatches == 7 and pty[-1] == L.PATCH_HALO and pz[-1] > 0 and all(pz[i] == 0 for i in range(6))
    self_slot = ext.array("haloSelf")
    assert ext.halo_slots == 26 and sorted(self_slot) == list(range(26)) and all(self_slot[self_slot[k]] == k for k in range(26))
    cg, C = ext.array("cellGlobal"), ext.array("C").reshape(-1, 3)
    for k in range(26):
        ghost, send = ext.array(f"haloGhost{k}"), ext.array(f"haloSend{int(self_slot[k])}")
        assert ghost.size > 0 and np.array_equal(cg[ghost], send)
        shift = C[ghost] - C[send]
        assert np.abs(shift - shift[0]).max() < 1e-12 and np.abs(shift[0]).max() > 0.5
    assert (ext.array("owner")[ps[-1]: ps[-1] + pz[-1]] >= n).all()        # nothing of the real cells is left on the halo patch
    # the copies are tetrahedra / prisms like their originals
    per_cell = np.bincount(ext.array("owner"), minlength=ext.nCells) + np.bincount(ext.array("neighbour"), minlength=ext.nCells)
    assert np.array_equal(per_cell[n:], per_cell[cg[n:]]) and set(per_cell) == set(EXPECT[kind][2])


@pytest.mark.parametrize("scheme", ["GaussVolPoint", "reduced"])
@pytest.mark.parametrize("kind", sorted(PERIODIC_KINDS))
def test_triply_periodic_oracle_conserves_mass_momentum_and_energy(kind, scheme):
    from test_cyclic_patches import OraclePeriodic, conserved
    g, ext = periodic_mesh(kind)
    per = OraclePeriodic(ext, q.default_options(stencil=scheme, **PERIODIC_OPT))
    per.set_fields(*periodic_fields(g.array("C").reshape(-1, 3)))
    V, n = g.array("V"), g.nCells
    rho0 = per.field("rho", n).copy()
    before = conserved(per.case, V, n)
    per.step(10)
    defect = conservation_defect(before, conserved(per.case, V, n))
    assert (defect <= 1e-13).all(), (kind, scheme, defect)
    assert np.abs(per.field("rho", n) - rho0).max() > 1e-3                   # (something happened)


def test_mixed_halves_are_refused_by_name():
    """mix643 periodic in x: the prisms' rectangles on xMin face the hexahedra's on xMax, but their neighbours' layers differ (triangles
    against quadrilaterals on the sides next to them)"""
    g = make_mesh("mix643", [L.PATCH_CYCLIC, L.PATCH_CYCLIC, 0, 0, 0, 0])
    with pytest.raises(q.QgdError, match="do not match point by point"):
        g.unroll_cyclic()


# ---- which family runs on which of these meshes ------------------------------------------------------------------------------------------
def _kinds(module, test, argnames, column=0, where=lambda row: True):
    """the unstructured kinds among the rows of one parametrisation of module.test (util.param_rows), optionally of the rows `where` keeps"""
    import importlib
    from util import param_rows
    rows = param_rows(getattr(importlib.import_module(module), test), argnames)
    rows = [row if isinstance(row, (tuple, list)) else (row,) for row in rows]
    return {row[column] for row in rows if (row[column] in unstructured.KINDS or row[column] in unstructured.REFINED) and where(row)}


def test_every_family_has_an_unstructured_row():
    """family -> (file, test, parametrisation) and the meshes it must hold: an edit that drops a row fails here, without a GPU.  (What runs on
    these meshes elsewhere: the fvsc operators, the explicit step, adjustTimeStep, explicit QHDFoam and explicit shards in
    tests/test_unstructured_gpu.py, the block tables in tests/test_fused_blocks_host.py, implicitDiffusion in tests/test_implicit_diffusion.py,
    the multigrid cycle in tests/test_mg_cycle_gpu.py, SRFQHDFoam on tet433 in tests/test_srf_qhd_gpu.py.)"""
    fam = "test_unstructured_families_gpu"
    tets, three = {"tet433", "mix643"}, {"tet433", "prism543", "mix643"}
    table = [
        ("species, explicit", fam, "test_species_explicit_match_the_replay", "kind,scheme", three, {}),
        ("species, explicit, shards", fam, "test_species_on_range_shards_of_tetrahedra", None, {"tet433"}, {}),
        ("species, implicitDiffusion", fam, "test_species_implicit_match_the_replay", "kind", tets, {}),
        ("varScModel7 sensor", fam, "test_var_sc_sensor_matches_the_restatement", "kind", three, {}),
        ("varScModel7 first step", fam, "test_var_sc_first_step_matches_the_oracle_fed_by_the_restatement", "kind,arm", tets, {}),
        ("varScModel7 every step", fam, "test_var_sc_every_step_takes_the_restatement_of_its_pressures", "kind,arm", tets, {}),
        ("monitor cell rows", "test_monitor_gpu", "test_integrals_extrema_and_probes_against_numpy", "kind", three, {}),
        ("monitor patch totals", "test_monitor_gpu", "test_patch_totals_against_the_face_fields", "kind", three, {}),
        ("monitor balance, fused", "test_monitor_gpu", "test_patch_fluxes_close_the_balance_of_mass_momentum_and_energy", "arm,adjust,kind", three,
         dict(column=2, where=lambda row: row[0] == "fused")),
        ("monitor balance, kernels", "test_monitor_gpu", "test_patch_fluxes_close_the_balance_of_mass_momentum_and_energy", "arm,adjust,kind", three,
         dict(column=2, where=lambda row: row[0] == "kernels")),
        ("species monitor cell rows", "test_species_monitor_gpu", "test_masses_extrema_and_probes_against_numpy", "kind,nS", tets, {}),
        ("species monitor patch fluxes", "test_species_monitor_gpu", "test_patch_totals_against_the_kept_face_fields", "kind", {"tet433"}, {}),
        ("QHD monitor cell rows", "test_qhd_monitor_gpu", "test_integrals_extrema_and_probes_against_numpy", "kind", three, {}),
        ("QHD monitor patch totals and continuity", "test_qhd_monitor_gpu", "test_patch_totals_against_the_face_fields", "kind", {"tet433"}, {}),
        ("scalarTransportQHDFoam steps", "test_scalar_transport_case", "test_device_case_steps_like_the_restatement", "kind,stencil,mu,upwind", three, {}),
        ("scalarTransportQHDFoam face fields", "test_scalar_transport_case", "test_device_face_fields_of_the_initial_state", "kind,stencil", tets, {}),
        ("QHDFoam implicitDiffusion", fam, "test_qhd_implicit_branch_matches_oracle", "kind", tets, {}),
        ("QHDFoam shards", fam, "test_qhd_shards_match_unsharded_device_and_oracle", "kind,world", {"tet433", "tet866"}, {}),
        ("QGDFoam implicitDiffusion shards", fam, "test_implicit_shards_match_unsharded_device_and_oracle", "kind,world", {"tet433", "tet866"}, {}),
        ("symmetry QGDFoam", fam, "test_symmetry_patches_match_the_oracle", "kind", {"tet433", "prism543"}, {}),
        ("symmetry QHDFoam", fam, "test_qhd_case_on_symmetry_patches", "kind", {"tet433", "prism543"}, {}),
        ("cyclic", fam, "test_triply_periodic_case_matches_the_oracle_and_conserves", "kind", set(PERIODIC_KINDS), {}),
        ("cyclic, oracle", "test_unstructured_meshes", "test_triply_periodic_oracle_conserves_mass_momentum_and_energy", "kind", set(PERIODIC_KINDS), {}),
    ]
    # one level of 2:1 refinement: the rows of tests/test_refined_cells_gpu.py's table (argnames None: a test of its own, named for the mesh)
    gpu, ref, r5, r8, both = "test_unstructured_gpu", "test_refined_cells_gpu", {"ref533"}, {"ref866"}, {"ref533", "ref866"}
    explicit, qhd = "kind,scheme,bc_fn,arm", "kind,variant"
    refined = [
        ("fvsc operators", gpu, "test_fvsc_operators_match_oracle", "kind", r5, {}),
        ("fvsc operators, quadtree", ref, "test_fvsc_operators_on_the_quadtree", None, None, {}),
        ("explicit, fused", gpu, "test_update_fluxes_and_steps", explicit, both, dict(where=lambda row: row[3] == "fused")),
        ("explicit, kernels", gpu, "test_update_fluxes_and_steps", explicit, both, dict(where=lambda row: row[3] == "kernels")),
        ("explicit, mixed patches", gpu, "test_update_fluxes_and_steps", explicit, both, dict(where=lambda row: row[2] is not None)),
        ("explicit, quadtree", ref, "test_explicit_step_on_the_quadtree", None, None, {}),
        ("explicit, fused against kernels", ref, "test_fused_step_is_the_three_kernels_bit_for_bit", "kind", both, {}),
        ("packed tables", "test_fused_packed_geometry_gpu", "test_refined_cells_whichever_way_the_rule_decides", None, None, {}),
        ("adjustTimeStep", gpu, "test_adjust_time_step", "kind", r5, {}),
        ("implicitDiffusion, fused", "test_implicit_diffusion", "test_device_implicit_branch_matches_oracle", "kind,stencil,bc_fn,arm", r5,
         dict(where=lambda row: row[3] == "fused")),
        ("implicitDiffusion, kernels", "test_implicit_diffusion", "test_device_implicit_branch_matches_oracle", "kind,stencil,bc_fn,arm", r5,
         dict(where=lambda row: row[3] == "kernels")),
        ("implicitDiffusion, fused against kernels", ref, "test_fused_implicit_assembly_is_the_separate_kernels_to_rounding", None, None, {}),
        ("implicitDiffusion shards", fam, "test_implicit_shards_match_unsharded_device_and_oracle", "kind,world", r8, {}),
        ("QHDFoam shards", fam, "test_qhd_shards_match_unsharded_device_and_oracle", "kind,world", r8, {}),
        ("QHDFoam implicitDiffusion", fam, "test_qhd_implicit_branch_matches_oracle", "kind", r5, {}),
        ("QHDFoam kernels", gpu, "test_qhd_case_matches_oracle", qhd, both, dict(where=lambda row: row[1] == "kernels")),
        ("QHDFoam blocks", gpu, "test_qhd_case_matches_oracle", qhd, r5, dict(where=lambda row: row[1] == "blocks")),
        ("QHDFoam deep", gpu, "test_qhd_case_matches_oracle", qhd, r5, dict(where=lambda row: row[1] == "deep")),
        ("QHDFoam deep plain", gpu, "test_qhd_case_matches_oracle", qhd, both, dict(where=lambda row: row[1] == "deep plain")),
        ("explicit shards", gpu, "test_sharded_device_matches_unsharded_and_oracle", "kind,world", r8, dict(where=lambda row: row[1] == 3)),
        ("varScModel7 sensor", fam, "test_var_sc_sensor_matches_the_restatement", "kind", r5, {}),
        ("scalarTransportQHDFoam steps", "test_scalar_transport_case", "test_device_case_steps_like_the_restatement", "kind,stencil,mu,upwind", r5, {}),
        ("QHD monitor patch totals and continuity", "test_qhd_monitor_gpu", "test_patch_totals_against_the_face_fields", "kind", r5, {}),
        ("monitor balance, fused", "test_monitor_gpu", "test_patch_fluxes_close_the_balance_of_mass_momentum_and_energy", "arm,adjust,kind", r5,
         dict(column=2, where=lambda row: row[0] == "fused")),
        ("monitor balance, kernels", "test_monitor_gpu", "test_patch_fluxes_close_the_balance_of_mass_momentum_and_energy", "arm,adjust,kind", r5,
         dict(column=2, where=lambda row: row[0] == "kernels")),
        ("species, explicit", fam, "test_species_explicit_match_the_replay", "kind,scheme", r5, {}),
        ("species, batch edge", ref, "test_species_batch_edge_on_refined_cells", None, None, {}),
        ("uniform flow", ref, "test_uniform_flow_stays_uniform", None, None, {}),
        ("mass balance, fused", ref, "test_mass_balance_of_a_refined_box_closed_by_slip_walls_on_the_fused_step", None, None, {}),
        ("mass balance, reduced", ref, "test_mass_is_conserved_in_a_refined_box_where_the_wall_flux_vanishes", None, None, {}),
    ]
    import importlib
    import test_unstructured_families_gpu as families
    from util import param_rows
    for family, module, test, argnames, want, how in refined:
        if argnames is None:
            assert callable(getattr(importlib.import_module(module), test)), (family, module, test)
            continue
        got = _kinds(module, test, argnames, **how)
        assert want <= got, (family, module, test, sorted(want - got))
    import test_mg_cycle_gpu as mg
    import test_refined_cells_gpu as refined_gpu
    import test_unstructured_gpu as step
    assert mg.ROWS["refined"][0] == mg.ROWS["double refined"][0] == "refined" and mg.MESHES["refined"]().nCells == 143
    assert set(param_rows(step.test_adjust_time_step, "arm")) == {"fusedAdjust", "kernels"}
    assert set(param_rows(step.test_sharded_device_matches_unsharded_and_oracle, "fused")) == {"any", False}
    assert set(param_rows(step.test_sharded_device_matches_unsharded_and_oracle, "overlapped")) == {False, True}
    assert set(param_rows(step.test_fvsc_operators_match_oracle, "scheme")) == {"GaussVolPoint", "reduced"}
    assert set(param_rows(step.test_fvsc_operators_match_oracle, "entry")) == {"host", "dev"}
    assert set(param_rows(refined_gpu.test_fvsc_operators_on_the_quadtree, "scheme")) == {"GaussVolPoint", "reduced", "leastSquares"}
    assert set(param_rows(refined_gpu.test_fvsc_operators_on_the_quadtree, "entry")) == {"host", "dev"}
    assert set(param_rows(refined_gpu.test_explicit_step_on_the_quadtree, "scheme")) == {"GaussVolPoint", "reduced", "leastSquares"}
    assert set(param_rows(refined_gpu.test_uniform_flow_stays_uniform, "arm")) == {"fused", "kernels"}
    assert len([p for p in param_rows(families.test_var_sc_sensor_matches_the_restatement, "params")]) == 3
    assert {("ref533", "GaussVolPoint"), ("ref533", "reduced")} <= {row[:2] for row in param_rows(
        importlib.import_module("test_scalar_transport_case").test_device_case_steps_like_the_restatement, "kind,stencil,mu,upwind")}
    for family, module, test, argnames, want, how in table:
        if argnames is None:          # one mesh, named by the module
            assert families.SPECIES_SHARDS[0] in want and hasattr(families, test), family
            continue
        got = _kinds(module, test, argnames, **how)
        assert want <= got, (family, module, test, sorted(want - got))
    assert set(PERIODIC_KINDS) == {"tet433", "prism543"}
    # ... and the arms
    for test in (families.test_var_sc_first_step_matches_the_oracle_fed_by_the_restatement, families.test_var_sc_every_step_takes_the_restatement_of_its_pressures):
        for kind in tets:
            assert {arm for k, arm in param_rows(test, "kind,arm") if k == kind} == {"fused", "kernels", "fusedAdjust", "implicitDiffusion"}, (test.__name__, kind)
    assert set(param_rows(families.test_symmetry_patches_match_the_oracle, "arm")) == {"fused", "kernels", "implicitDiffusion"}
    assert set(param_rows(families.test_triply_periodic_case_matches_the_oracle_and_conserves, "arm")) == {"fused", "kernels"}
    assert {("tet433", "GaussVolPoint"), ("mix643", "GaussVolPoint"), ("prism543", "reduced")} <= set(param_rows(families.test_species_explicit_match_the_replay, "kind,scheme"))
    assert set(param_rows(families.test_species_explicit_match_the_replay, "adjust")) == {0, 1}
    assert set(param_rows(families.test_species_on_range_shards_of_tetrahedra, "layer_first")) == {False, True}


@pytest.mark.parametrize("kind", sorted(EXPECT))
def test_oracle_stays_finite_and_positive(kind):
    from test_case_parity_gpu import mixed_box_bcs
    mesh = make_mesh(kind)
    oc = OracleCase(oracle_mesh_of(mesh), q.default_options(stencil="GaussVolPoint", deltaT=2e-4, mu=2e-3))
    mixed_box_bcs(oc)
    oc.set_fields(*cases.box_initial_fields(mesh.array("C").reshape(-1, 3)))
    rho0 = oc.field("rho").copy()
    oc.step(25)
    for f in ("rho", "U", "p", "e"):
        assert np.isfinite(oc.field(f)).all(), f
    assert oc.field("rho").min() > 0 and oc.field("e").min() > 0 and np.abs(oc.field("rho") - rho0).max() > 1e-4 * rho0.max()


# ---- the oracle on the refined boxes ------------------------------------------------------------------------------------------------------
ORACLE_REFINED = [(kind, scheme) for kind in ("ref533", "ref866") for scheme in ("GaussVolPoint", "reduced")] + \
                 [("ref2d87", scheme) for scheme in ("GaussVolPoint", "reduced", "leastSquares")]
ORACLE_OPT = dict(deltaT=2e-4, mu=2e-3)


@pytest.mark.parametrize("kind,scheme", ORACLE_REFINED)
def test_oracle_stays_finite_and_positive_on_refined_cells(kind, scheme):
    """25 steps under mixed_box_bcs (the quadtree: z empty, the pulse of plane_init), with every stencil the oracle serves on the mesh"""
    from test_case_parity_gpu import empty_z_bcs, mixed_box_bcs, plane_init
    mesh = make_mesh(kind)
    oc = OracleCase(oracle_mesh_of(mesh), q.default_options(stencil=scheme, **ORACLE_OPT))
    C = mesh.array("C").reshape(-1, 3)
    if mesh.nGeometricD == 2:
        empty_z_bcs(oc)
        oc.set_fields(*plane_init(C))
    else:
        mixed_box_bcs(oc)
        oc.set_fields(*cases.box_initial_fields(C))
    rho0 = oc.field("rho").copy()
    oc.step(25)
    for f in ("rho", "U", "p", "e"):
        assert np.isfinite(oc.field(f)).all(), f
    assert oc.field("rho").min() > 0 and oc.field("e").min() > 0 and np.abs(oc.field("rho") - rho0).max() > 1e-4 * rho0.max()


@pytest.mark.parametrize("kind,scheme", ORACLE_REFINED)
def test_oracle_keeps_a_uniform_flow_uniform_on_refined_cells(kind, scheme):
    """U = (0.3, 0.2, -0.1), T = p = 1, default patches (the quadtree: z empty, no velocity across its plane), 20 steps: 1e-14 of each field's
    size (measured 7e-16 on ref533, 4e-15 on ref866, 2e-15 on ref2d87).  The fluxes of a uniform state cancel over a cell only if its faces close, hanging nodes and all"""
    from test_case_parity_gpu import empty_z_bcs
    mesh = make_mesh(kind)
    oc = OracleCase(oracle_mesh_of(mesh), q.default_options(stencil=scheme, **ORACLE_OPT))
    n = mesh.nCells
    U = np.tile([0.3, 0.2, -0.1], (n, 1))
    if mesh.nGeometricD == 2:
        empty_z_bcs(oc)
        U[:, 2] = 0.0
    oc.set_fields(U, np.ones(n), np.ones(n))
    before = {f: oc.field(f).copy() for f in ("rho", "U", "p", "e")}
    oc.step(20)
    worst = {f: float(np.abs(oc.field(f) - before[f]).max() / np.abs(before[f]).max()) for f in before}
    print(f"oracle uniform flow {kind} {scheme}: worst {max(worst.values()):.1e}")
    assert all(v <= 1e-14 for v in worst.values()), (kind, scheme, worst)
