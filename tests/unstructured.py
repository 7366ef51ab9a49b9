"""Conforming meshes of tetrahedra, prisms and prisms + hexahedra, built from a lattice of cubes (test code only: nothing here is the
library's).  What they have that a split or jittered box of hexahedra has not: vertices shared by more than eight cells (24 on Kuhn's six
tetrahedra per cube, 12 on two prisms per cube) and cells of four and five faces.

assemble() is the one polyhedra-to-polyMesh step: cells come as lists of vertex loops, faces are de-duplicated by their vertex set, oriented
owner -> neighbour (outwards on the boundary) and put into OpenFOAM's order -- internal faces sorted by (owner, neighbour), owner < neighbour,
then the boundary faces grouped by the six sides of the box (xMin, xMax, yMin, yMax, zMin, zMax: the patch order of PolyMesh.box)."""
import functools
import itertools

import numpy as np

# corner (a, b, c) of the unit cube -> local index a + 2 b + 4 c
_HEX_FACES = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]
# two prisms per cube: the xy square cut along its (0,0)-(1,1) diagonal, extruded in z
_PRISMS = [((0, 1, 3), (4, 5, 7)), ((0, 3, 2), (4, 7, 6))]


def _kuhn_tets():
    """Kuhn's six tetrahedra of the unit cube: one per order in which the three axes are walked from corner 0 to corner 7.  Every cube is cut
    the same way, so the diagonals of a face shared by two cubes coincide"""
    tets = []
    for perm in itertools.permutations(range(3)):
        v, path = [0, 0, 0], [0]
        for axis in perm:
            v[axis] = 1
            path.append(v[0] + 2 * v[1] + 4 * v[2])
        tets.append(tuple(path))
    return tets


def _tet_faces(t):
    return [(t[0], t[1], t[2]), (t[0], t[1], t[3]), (t[0], t[2], t[3]), (t[1], t[2], t[3])]


def _prism_faces(p):
    (a, b, c), (d, e, f) = p
    return [(a, b, c), (d, e, f), (a, b, e, d), (b, c, f, e), (c, a, d, f)]


def lattice_cells(nx, ny, nz, shape_of):
    """cells (lists of vertex loops over lattice point labels) of an nx x ny x nz lattice of cubes, cube by cube with i fastest;
    shape_of(i, j, k) in {"tet", "prism", "hex"} says how a cube is cut"""
    def pid(i, j, k):
        return i + (nx + 1) * (j + (ny + 1) * k)

    tets = _kuhn_tets()
    cells = []
    for k, j, i in itertools.product(range(nz), range(ny), range(nx)):
        corner = [pid(i + (l & 1), j + ((l >> 1) & 1), k + (l >> 2)) for l in range(8)]
        shape = shape_of(i, j, k)
        if shape == "hex":
            local = [_HEX_FACES]
        elif shape == "prism":
            local = [_prism_faces(p) for p in _PRISMS]
        elif shape == "tet":
            local = [_tet_faces(t) for t in tets]
        else:
            raise KeyError(shape)
        for faces in local:
            cells.append([[corner[l] for l in loop] for loop in faces])
    return cells


def lattice_points(nx, ny, nz, jitter=0.1, seed=2024):
    """lattice points of the unit box, those inside it moved by up to jitter * spacing along every axis; returns (points, integer coordinates)"""
    k, j, i = np.meshgrid(np.arange(nz + 1), np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    ijk = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)
    n = np.array([nx, ny, nz])
    pts = ijk / n
    inside = np.all((ijk > 0) & (ijk < n), axis=1)
    move = np.random.default_rng(seed).uniform(-1.0, 1.0, pts.shape) * (jitter / n)
    pts[inside] += move[inside]
    return pts, ijk


def assemble(points, cells, side_of):
    """primitives of the polyMesh of these cells: a dict with the arguments of PolyMesh.from_arrays.  cells[c] is a list of vertex loops
    (either sense); side_of(loop) names the patch (0..5) of a face that has one cell only.  Faces are oriented on the geometry: the area
    vector of a loop points away from the mean of its owner's vertices (the cells are convex)."""
    points = np.asarray(points, dtype=np.float64)
    faces = {}                                # vertex set -> [loop as the owner listed it, owner, neighbour]
    for c, loops in enumerate(cells):
        for loop in loops:
            key = frozenset(loop)
            assert len(key) == len(loop) >= 3, (c, loop)
            if key in faces:
                assert faces[key][2] < 0, ("a face of three cells", c, loop)
                faces[key][2] = c
            else:
                faces[key] = [list(loop), c, -1]     # cells come in ascending label: the first to list a face is its owner

    def outwards(loop, c):
        x = points[loop]
        fc = x.mean(axis=0)
        area = sum(np.cross(x[q] - fc, x[(q + 1) % len(loop)] - fc) for q in range(len(loop)))
        centre = points[sorted({v for l in cells[c] for v in l})].mean(axis=0)
        return loop if np.dot(area, fc - centre) > 0 else loop[::-1]

    internal = sorted((f for f in faces.values() if f[2] >= 0), key=lambda f: (f[1], f[2]))
    boundary = [[] for _ in range(6)]
    for loop, own, _ in (f for f in faces.values() if f[2] < 0):
        boundary[side_of(loop)].append((loop, own))
    for side in boundary:
        side.sort(key=lambda f: (f[1], sorted(f[0])))
    ordered = [(loop, own) for loop, own, _ in internal] + [f for side in boundary for f in side]
    loops = [outwards(loop, own) for loop, own in ordered]
    sizes = np.array([len(side) for side in boundary], dtype=np.int32)
    return dict(points=points.reshape(-1), faceOffsets=np.concatenate([[0], np.cumsum([len(l) for l in loops])]).astype(np.int32),
                facePoints=np.array([v for l in loops for v in l], dtype=np.int32), owner=np.array([own for _, own in ordered], dtype=np.int32),
                neighbour=np.array([f[2] for f in internal], dtype=np.int32), nCells=len(cells),
                patchStart=(len(internal) + np.concatenate([[0], np.cumsum(sizes)[:-1]])).astype(np.int32), patchSize=sizes,
                patchType=np.zeros(6, dtype=np.int32))


KINDS = {
    "tet433": ((4, 3, 3), lambda i, j, k: "tet"),
    "tet866": ((8, 6, 6), lambda i, j, k: "tet"),
    "prism543": ((5, 4, 3), lambda i, j, k: "prism"),
    "mix643": ((6, 4, 3), lambda i, j, k: "prism" if i < 3 else "hex"),       # prisms and hexahedra share wavefronts
}


@functools.lru_cache(maxsize=None)
def primitives(kind, jitter=0.1):
    """the named mesh as arrays (the dict PolyMesh.primitives() returns); built once per process and shared: do not write into them"""
    (nx, ny, nz), shape_of = KINDS[kind]
    pts, ijk = lattice_points(nx, ny, nz, jitter, seed=sum(map(ord, kind)))
    n = np.array([nx, ny, nz])

    def side_of(loop):
        x = ijk[loop]
        for axis in range(3):
            if np.all(x[:, axis] == 0):
                return 2 * axis
            if np.all(x[:, axis] == n[axis]):
                return 2 * axis + 1
        raise AssertionError(("an unmatched face inside the box", loop))

    return assemble(pts, lattice_cells(nx, ny, nz, shape_of), side_of)


def point_valence(prim):
    """cells per point"""
    fo, fp, own, nei = prim["faceOffsets"], prim["facePoints"].astype(np.int64), prim["owner"].astype(np.int64), prim["neighbour"].astype(np.int64)
    face = np.repeat(np.arange(own.size), np.diff(fo))
    inner = face < nei.size
    pairs = np.unique(np.concatenate([fp * prim["nCells"] + own[face], fp[inner] * prim["nCells"] + nei[face[inner]]]))
    return np.bincount(pairs // prim["nCells"], minlength=prim["points"].size // 3)


def faces_per_cell(prim):
    return np.bincount(prim["owner"], minlength=prim["nCells"]) + np.bincount(prim["neighbour"], minlength=prim["nCells"])


def write_primitives(path, prim):
    """plain text for tests/cpp/fused_blocks_test.cpp: the sizes, then the arrays in the order of qgd_mesh_create"""
    with open(path, "w") as f:
        f.write(f"{prim['points'].size // 3} {prim['owner'].size} {prim['neighbour'].size} {prim['nCells']} {prim['patchStart'].size} "
                f"{prim['facePoints'].size}\n")
        f.write(" ".join(repr(float(x)) for x in prim["points"]) + "\n")
        for name in ("faceOffsets", "facePoints", "owner", "neighbour", "patchStart", "patchSize", "patchType"):
            f.write(" ".join(str(int(x)) for x in prim[name]) + "\n")
