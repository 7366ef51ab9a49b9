"""Host logic of the fused step (CPU): the block tables of qgd_setup.cpp buildFusedBlocks checked entry by entry against the mesh tables they are
made from, on bricks, ragged boxes, a jittered mesh with triangles and polygons, and a slab shard with two cuts (tests/cpp/fused_blocks_test.cpp,
compiled with plain g++ from the library's own host sources -- no HIP, no oracle).  The same program checks that thin meshes have more
blocks than 64-face tiles (the premise of tests/test_courant_small_blocks_gpu.py), and that blocks which share a template share its
tables: a second build truncates the topology fingerprint to one bit (QGD_TEST_TOPOHASH_BITS, a macro the library's own build never
defines), so that unlike blocks are certain to meet in one template unless the builder compares their tables.  Handed primitives files, the
program runs the same checks on them: the tetrahedral / prismatic / mixed meshes of tests/unstructured.py, whose vertices have up to 24 cells
(the vertex stride capPE is 24 / 12, not the 8 of every hexahedral mesh) and whose cells have 4 or 5 face entries, a Morton-ordered shard
of the 1728 tetrahedra, and the 2:1 refined boxes ref533 / ref866, whose cells have 6 to 24 face entries (stride capE 24)."""
import os
import subprocess

import unstructured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qgdsolver_amd", "csrc")


_BUILT = {}     # defines -> program: the tests that want the same build share it


def build_and_run(tmp_path, name, defines=(), args=()):
    exe = _BUILT.get(tuple(defines))
    if exe is None or not os.path.exists(exe):
        exe = str(tmp_path / name)
        cmd = ["g++", "-std=c++17", "-O2", "-fopenmp", "-I", CSRC, *defines, os.path.join(ROOT, "tests", "cpp", "fused_blocks_test.cpp")] + \
              [os.path.join(CSRC, f) for f in ("qgd_mesh.cpp", "qgd_partition.cpp", "qgd_setup.cpp")] + ["-o", exe]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        _BUILT[tuple(defines)] = exe
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS="4"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-2000:]
    return r.stdout


def test_block_tables_are_consistent_with_the_mesh(tmp_path):
    """... with the full fingerprint: no block differs from its template, the template counts are the pinned ones, and the thin meshes have
    more blocks than face tiles"""
    out = build_and_run(tmp_path, "fused_blocks_test")
    assert "thin 1024x1x1" in out and "thin 1x1x700" in out


def test_blocks_that_collide_in_a_template_get_their_own(tmp_path):
    """a fingerprint of one bit: every mesh with three unlike blocks puts two of them into one template.  The builder must notice (the
    program asserts a positive mismatch count) and every block's tables, read through its template, must still be the mesh's"""
    out = build_and_run(tmp_path, "fused_blocks_test_collide", ["-DQGD_TEST_TOPOHASH_BITS=1"])
    assert "matched a template by fingerprint and not by their tables" in out


def test_block_tables_of_tetrahedra_prisms_and_mixed_cells(tmp_path):
    """the entry-by-entry checks on cells of 4 / 5 / 5 + 6 faces and vertices of 24 / 12 cells: the vertex stride is the longest row (24 on
    tetrahedra, 12 on prisms and on the mix), the 1728 tetrahedra make many blocks, no block differs from its template, and the middle one of
    three Morton-ordered shards of the 1728 tetrahedra (more ghost cells than owned ones) passes the same checks"""
    args = []
    for kind, cap_pe, min_blocks, shard_of, least, most in (("tet433", 24, 2, 0, 4, 4), ("tet866", 24, 2, 0, 4, 4), ("prism543", 12, 1, 0, 5, 5),
                                                            ("mix643", 12, 1, 0, 5, 6), ("tet866", 24, 2, 3, 4, 4)):
        path = str(tmp_path / f"{kind}.txt")
        unstructured.write_primitives(path, unstructured.primitives(kind))
        args += [path, str(cap_pe), str(min_blocks), str(shard_of), str(least), str(most)]
    out = build_and_run(tmp_path, "fused_blocks_test_files", args=args)
    print(out)
    assert out.count(" cells, ") == 5 and "ghost cells for" in out


def test_block_tables_of_refined_cells(tmp_path):
    """the same checks on one level of 2:1 refinement: a coarse hexahedron between refined ones has 24 face entries beside the 6 of its
    neighbours' children in one block, so the entry stride capE is 24 (6 on every other mesh here); the vertices stay within eight cells.
    ref533, ref866 and the middle one of three Morton-ordered shards of ref866; no block differs from its template"""
    args = []
    for kind, min_blocks, shard_of in (("ref533", 1, 0), ("ref866", 2, 0), ("ref866", 2, 3)):
        path = str(tmp_path / f"{kind}.txt")
        unstructured.write_primitives(path, unstructured.refined_primitives(kind))
        args += [path, "8", str(min_blocks), str(shard_of), "6", "24"]
    out = build_and_run(tmp_path, "fused_blocks_test_files", args=args)
    print(out)
    assert out.count(" cells, ") == 3 and "ghost cells for" in out
    assert out.count("face entries per own cell: 6 .. 24 (stride 24)") == 3
    assert out.count(" 0 blocks matched a template by fingerprint and not by their tables") == 3
