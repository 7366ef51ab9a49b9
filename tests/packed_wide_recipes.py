"""Meshes whose packed tables of the fused step hold offsets that use all 16 bits: one list for the host test (tests/test_fused_packed_wide_host.py,
tests/cpp/fused_packed_wide_test.cpp) and the GPU tests (tests/test_fused_packed_wide_gpu.py).

A uniform box keeps every offset of its packed tables below 128 (vertex weights within [-30, 29], face words within 64 on box(17,9,9)), so on it
a decode that reads the low byte alone is right.  PolyMesh.jitter with an amplitude of ~1e-12 of the cell size moves the interior points by
thousands of ULPs: the mesh still satisfies the packing rule (a spread of at most 65 535 bit patterns) and its offsets fill the half words.  Beyond
roughly 3e-12 the spread is exceeded and nothing packs.

A recipe is box(*shape, hi=hi).jitter(amplitude, seed) and what the builder must make of it:

    packedWeights, packedFaces, hfClasses     exactly as listed
    max(maxWeightOffset, maxFaceOffset) >= 16384   wherever anything packs
    maxFaceOffset >= 16384                          wherever the faces pack

(the offsets themselves may move by a few patterns between compilers, which contract multiply-adds differently: every packing entry keeps about
a thousand patterns between its spread and the limit)."""
from collections import namedtuple

Recipe = namedtuple("Recipe", "tag shape hi amplitude seed packedWeights packedFaces hfClasses")

WIDE = 16384   # the floor on the largest |offset|: bit 14 and the sign bit are in use

ONE = (1.0, 1.0, 1.0)

RECIPES = {r.tag: r for r in (
    Recipe("two classes", (17, 9, 9), ONE, 2e-12, 2024, True, True, 2),
    Recipe("two classes, wider", (17, 9, 9), ONE, 2.6e-12, 7, True, True, 2),
    Recipe("three classes by split", (17, 9, 9), ONE, 2.8e-12, 2024, True, True, 3),     # class 0 wider than 65 535: cut in two
    Recipe("four classes", (17, 9, 9), (1.0, 1.0, 1.0 + 1.5e-11), 2.8e-12, 2024, True, True, 4),   # ... and dz a little off dy
    Recipe("three spacings", (16, 8, 12), ONE, 2e-12, 2024, True, True, 3),
    Recipe("weights only", (17, 9, 9), ONE, 2.8e-12, 1, True, False, 0),                 # w spreads beyond 65 535: level 1
    Recipe("nothing packs", (17, 9, 9), ONE, 4e-12, 2024, False, False, 0),              # level 0
    Recipe("implicit", (9, 5, 5), ONE, 3e-12, 2024, True, True, 2),
    Recipe("12 cells", (3, 2, 2), ONE, 7e-12, 75, True, True, 2),     # two interior points: few seeds move the face words that far
    Recipe("60 cells", (5, 4, 3), ONE, 3e-12, 8, True, True, 3),
)}

UNIFORM = ((17, 9, 9), (16, 8, 12), (9, 5, 5))   # the boxes the packed GPU tests ran on before: reported by the host program, not judged


def argument(r):
    """the recipe as tests/cpp/fused_packed_wide_test.cpp reads it (repr of a float reads back exactly)"""
    return "|".join([r.tag, ",".join(str(n) for n in r.shape), ",".join(repr(float(h)) for h in r.hi), repr(float(r.amplitude)), str(int(r.seed)),
                     str(int(r.packedWeights)), str(int(r.packedFaces)), str(int(r.hfClasses))])


def uniform_argument(shape):
    return "|".join(["uniform box " + "x".join(str(n) for n in shape), ",".join(str(n) for n in shape), "1.0,1.0,1.0", "0.0", "0", "-1", "-1", "0"])


def mesh_of(r):
    import qgdsolver_amd as q
    return q.PolyMesh.box(*r.shape, hi=r.hi).jitter(r.amplitude, seed=r.seed)


def check(r, blocks, tag=""):
    """the recipe's expectation on what Device.fused_blocks() reports"""
    got = {k: blocks[k] for k in ("packedWeights", "packedFaces", "hfClasses", "maxWeightOffset", "maxFaceOffset")}
    print(f"{r.tag}{tag}: {got}")
    assert got["packedWeights"] is r.packedWeights and got["packedFaces"] is r.packedFaces and got["hfClasses"] == r.hfClasses, (r, got)
    if r.packedWeights:
        assert max(got["maxWeightOffset"], got["maxFaceOffset"]) >= WIDE, (r, got)
    else:
        assert got["maxWeightOffset"] == 0, (r, got)
    if r.packedFaces:
        assert got["maxFaceOffset"] >= WIDE, (r, got)
    else:
        assert got["maxFaceOffset"] == 0, (r, got)
    return blocks
