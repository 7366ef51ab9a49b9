"""The generated tetrahedral / prismatic / mixed meshes (tests/unstructured.py) are what the device tests need them to be (CPU): point valences
beyond the eight register slots of the fused kernels' vertex walk, cells with fewer than six faces, prisms and hexahedra in one wavefront,
OpenFOAM face order (qgd_mesh_create accepts them), closed cells of positive volume, Morton-ordered shards, and an oracle that stays finite
and positive on them."""
import numpy as np
import pytest

import qgdsolver_amd as q

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


def test_the_four_kinds_are_the_ones_listed():
    assert sorted(unstructured.KINDS) == sorted(EXPECT)


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


@pytest.mark.parametrize("kind,world", [("tet433", 3), ("tet866", 2), ("tet866", 3)])
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
