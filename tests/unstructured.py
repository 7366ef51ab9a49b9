"""Conforming meshes of tetrahedra, prisms and prisms + hexahedra, built from a lattice of cubes (test code only: nothing here is the
library's).  What they have that a split or jittered box of hexahedra has not: vertices shared by more than eight cells (24 on Kuhn's six
tetrahedra per cube, 12 on two prisms per cube) and cells of four and five faces.

assemble() is the one polyhedra-to-polyMesh step: cells come as lists of vertex loops, faces are de-duplicated by their vertex set, oriented
owner -> neighbour (outwards on the boundary) and put into OpenFOAM's order -- internal faces sorted by (owner, neighbour), owner < neighbour,
then the boundary faces grouped by the six sides of the box (xMin, xMax, yMin, yMax, zMin, zMax: the patch order of PolyMesh.box).

REFINED / refined_primitives(): boxes of hexahedra with one level of 2:1 refinement, as refineMesh (hexRef8) leaves them -- a coarse cube between
refined ones has 24 faces, an unsplit face next to a split edge 5 to 8 points of which three are collinear, a hanging vertex 5 or 6 cells.
They go through the same assemble().  Not built here: more than one level, refined boxes whose opposite sides match (for cyclic patches)."""
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


# ---- one level of 2:1 refinement, the way hexRef8 leaves a mesh ---------------------------------------------------------------------------
# kind: (lattice, refined(i, j, k), quadtree).  The checkerboards enclose coarse cubes on every side: 24 faces (18 / 21 / 15 / 9 next to the
# box and to the unrefined part), beside the 6 of their refined neighbours' children in the same 64 cells
REFINED = {
    "ref533": ((5, 3, 3), lambda i, j, k: i < 3 and (i + j + k) % 2 == 0, False),
    "ref866": ((8, 6, 6), lambda i, j, k: i < 5 and (i + j + k) % 2 == 0, False),
    "ref2d87": ((8, 7, 1), lambda i, j, k: i < 5 and (i + j) % 2 == 0, True),          # z empty, height 0.1: 2 x 2 x 1 children
}
REFINED_HEIGHT_2D = 0.1


def refined_cells(nx, ny, nz, refined, quadtree=False):
    """cells (lists of vertex loops) of the lattice with the cubes refined(i, j, k) names cut into 2 x 2 x 2 (quadtree: 2 x 2 x 1) hexahedra,
    over points named by their doubled integer coordinates: (2 i, 2 j, 2 k) is a lattice point, an odd coordinate lies half way.  Cubes with
    i fastest, the children of a cube (x fastest) in its place.  An unrefined cube lists the four (quadtree: two) quadrilaterals of a side whose
    neighbour is refined, and on every other side one loop with the mid-edge point of each edge that a cube around that edge refines: the
    hanging nodes"""
    n = (nx, ny, nz)
    halves = (2, 2, 1 if quadtree else 2)                                 # pieces per axis of a refined cube

    def is_refined(c):
        return all(0 <= c[a] < n[a] for a in range(3)) and bool(refined(*c))

    def edge_is_split(p, q):
        """p, q: lattice points (cube coordinates) one step apart along `axis`; the up to four cubes around the edge"""
        axis = next(a for a in range(3) if p[a] != q[a])
        if halves[axis] == 1:
            return False
        others = [a for a in range(3) if a != axis]
        for da, db in itertools.product((-1, 0), repeat=2):
            c = list(p)
            c[others[0]] += da
            c[others[1]] += db
            if is_refined(c):
                return True
        return False

    def hexahedron(lo, size):
        """lo: doubled coordinates of the low corner; size: doubled extent per axis"""
        corner = [tuple(lo[a] + size[a] * ((l >> a) & 1) for a in range(3)) for l in range(8)]
        return [[corner[l] for l in loop] for loop in _HEX_FACES]

    cells = []
    for k, j, i in itertools.product(range(nz), range(ny), range(nx)):
        cube = (i, j, k)
        if is_refined(cube):
            size = tuple(2 // h for h in halves)
            for dz, dy, dx in itertools.product(range(halves[2]), range(halves[1]), range(halves[0])):
                cells.append(hexahedron((2 * i + dx * size[0], 2 * j + dy * size[1], 2 * k + dz * size[2]), size))
            continue
        corner = [(i + (l & 1), j + ((l >> 1) & 1), k + (l >> 2)) for l in range(8)]
        loops = []
        for side, quad in enumerate(_HEX_FACES):
            axis, beyond = side // 2, list(cube)
            beyond[axis] += 1 if side % 2 else -1
            if is_refined(beyond):                                        # the children's faces, as the neighbour lists them
                u, v = [a for a in range(3) if a != axis]
                plane = 2 * corner[quad[0]][axis]
                for dv, du in itertools.product(range(halves[v]), range(halves[u])):
                    su, sv = 2 // halves[u], 2 // halves[v]
                    loop = []
                    for a, b in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        key = [0, 0, 0]
                        key[axis], key[u], key[v] = plane, 2 * cube[u] + (du + a) * su, 2 * cube[v] + (dv + b) * sv
                        loop.append(tuple(key))
                    loops.append(loop)
                continue
            loop = []
            for s in range(4):
                p, q = corner[quad[s]], corner[quad[(s + 1) % 4]]
                loop.append(tuple(2 * x for x in p))
                if edge_is_split(min(p, q), max(p, q)):
                    loop.append(tuple(x + y for x, y in zip(p, q)))
            loops.append(loop)
        cells.append(loops)
    return cells


@functools.lru_cache(maxsize=None)
def refined_primitives(kind, jitter=0.1):
    """the named refined box as arrays (primitives()), with "midEdges": rows (hanging node, end, end) of point labels.  Only the lattice points
    inside the box are jittered (quadtree: in the plane, alike on both z planes); a mid-edge, mid-face or mid-cell point is the mean of the
    2, 4 or 8 lattice points around it, so a hanging node lies on the edge it hangs on"""
    (nx, ny, nz), refined, quadtree = REFINED[kind]
    seed = sum(map(ord, kind))
    if quadtree:
        assert nz == 1
        plane, ij = lattice_points(nx, ny, 1, 0.0)
        plane, ij = plane[: (nx + 1) * (ny + 1)], ij[: (nx + 1) * (ny + 1)]
        inside = np.all((ij[:, :2] > 0) & (ij[:, :2] < (nx, ny)), axis=1)
        move = np.random.default_rng(seed).uniform(-1.0, 1.0, (plane.shape[0], 2)) * (jitter / np.array([nx, ny]))
        plane[inside, :2] += move[inside]
        pts = np.concatenate([plane, plane + (0.0, 0.0, REFINED_HEIGHT_2D)])
    else:
        pts, _ = lattice_points(nx, ny, nz, jitter, seed=seed)
    lattice = pts.reshape(nz + 1, ny + 1, nx + 1, 3)
    cells = refined_cells(nx, ny, nz, refined, quadtree)
    keys = sorted({key for loops in cells for loop in loops for key in loop}, key=lambda key: key[::-1])
    label = {key: l for l, key in enumerate(keys)}
    points = np.empty((len(keys), 3))
    for key, l in label.items():
        around = [lattice[c, b, a] for a, b, c in itertools.product(*[(x // 2,) if x % 2 == 0 else (x // 2, x // 2 + 1) for x in key])]
        points[l] = sum(around[1:], around[0]) / len(around)
    doubled, top = np.array(keys), 2 * np.array([nx, ny, nz])

    def side_of(loop):
        x = doubled[loop]
        for axis in range(3):
            if np.all(x[:, axis] == 0):
                return 2 * axis
            if np.all(x[:, axis] == top[axis]):
                return 2 * axis + 1
        raise AssertionError(("an unmatched face inside the box", loop))

    prim = assemble(points, [[[label[key] for key in loop] for loop in loops] for loops in cells], side_of)
    mids = [(key, axis) for key in keys for axis in range(3) if [x % 2 for x in key] == [int(a == axis) for a in range(3)]]
    ends = [[tuple(x + s * (a == axis) for a, x in enumerate(key)) for s in (-1, 1)] for key, axis in mids]
    prim["midEdges"] = np.array([[label[key], label[lo], label[hi]] for (key, _), (lo, hi) in zip(mids, ends)], dtype=np.int32).reshape(-1, 3)
    return prim


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
