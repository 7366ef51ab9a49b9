"""Meshes whose packed geometry tables of the fused step hold codes that use the high offset bits: one list for the host test
(tests/test_fused_packed_geometry_host.py, tests/cpp/fused_packed_geometry_test.cpp) and the GPU test (tests/test_fused_packed_geometry_gpu.py).

A uniform box keeps every 12-bit offset of its coordinate codes below 16 and gives every plane of cells or vertices one dictionary entry (17x9x9:
at most 10 entries on an axis), so on it a decode that reads the low byte of the offset alone is right.  PolyMesh.jitter with an amplitude of
4e-13 moves the interior points by thousands of ULPs: the planes' patterns spread over more than one window of 4 096, the dictionaries grow
(12 entries on 17x9x9, 7 on 9x5x5) and the offsets fill the 12 bits (4 094 and 4 082), while the mesh still packs at every level.  From 8e-13 on
some block of 17x9x9 needs a 17th entry and the mesh keeps level 2; the amplitudes and seeds below were found on the CPU with the host program.

A recipe is box(*shape).jitter(amplitude, seed) and what the builder must make of it:

    packedWeights, packedFaces, packedGeometry    all True
    maxGeoOffset >= min_offset                    2 048: bit 11 of the offset is in use (the issue's floor is 11 of the 12 bits)
    maxGeoDict >= min_dict                        more entries than the uniform box of the shape has, and never fewer than 3
"""
from collections import namedtuple

Recipe = namedtuple("Recipe", "tag shape amplitude seed min_offset min_dict")

RECIPES = {r.tag: r for r in (
    Recipe("many blocks", (17, 9, 9), 4e-13, 2024, 2048, 11),
    Recipe("implicit", (9, 5, 5), 4e-13, 2024, 2048, 7),
)}


def argument(r):
    """the recipe as tests/cpp/fused_packed_geometry_test.cpp reads it (repr of a float reads back exactly)"""
    return "|".join([r.tag, ",".join(str(n) for n in r.shape), repr(float(r.amplitude)), str(int(r.seed)), str(int(r.min_offset)), str(int(r.min_dict))])


def mesh_of(r):
    import qgdsolver_amd as q
    return q.PolyMesh.box(*r.shape).jitter(r.amplitude, seed=r.seed)


def check(r, blocks, tag=""):
    """the recipe's expectation on what Device.fused_blocks() reports"""
    got = {k: blocks[k] for k in ("packedWeights", "packedFaces", "packedGeometry", "maxGeoDict", "maxGeoOffset")}
    print(f"{r.tag}{tag}: {got}")
    assert got["packedWeights"] is True and got["packedFaces"] is True and got["packedGeometry"] is True, (r, got)
    assert got["maxGeoOffset"] >= r.min_offset >= 1024, (r, got)
    assert got["maxGeoDict"] >= r.min_dict >= 3, (r, got)
    return blocks
