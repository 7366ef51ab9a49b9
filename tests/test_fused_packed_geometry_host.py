"""The geometry of the fused step block-major and packed, host side (CPU): qgd_setup.cpp packFusedGeometry checked by
tests/cpp/fused_packed_geometry_test.cpp, compiled with plain g++ from the library's own host sources -- no HIP, no oracle.  Uniform boxes (17x9x9,
40x20x20, 16x8x12, 3x2x2, 9x5x5, 50^3), slab shards, the two cell-range shards of 16x8x12 and the thin slab 0..12 of a 400^3 box qualify and decode
to the mesh's Cc / X / V / hQGD bit for bit in every slot of every block, with the same tables under 1 and 16 threads and zero slots beyond a
block's counts; the rule holds on tables written by hand (16 dictionary entries on an axis pack, 17 do not; an offset of 4 095 stays in its
entry, 4 096 opens the next; negative coordinates and zero decode exactly; a span of V or hQGD of 65 535 packs, 65 536 does not; face streams
not packed means geometry not packed; QGD_FUSED_PACKED_G=0 builds no tables); box(1,1,40), a jittered mesh and a 2:1 graded box keep their arrays
alone.  The wide recipes of tests/packed_geometry_recipes.py pack at every level with offsets that use the high bits.  A second build runs the
same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code with its own main: no GPU, nothing preloaded)."""
import os
import subprocess

import packed_geometry_recipes as recipes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qgdsolver_amd", "csrc")


def build(tmp_path, name, flags=()):
    exe = str(tmp_path / name)
    sources = [os.path.join(ROOT, "tests", "cpp", "fused_packed_geometry_test.cpp")] + \
              [os.path.join(CSRC, f) for f in ("qgd_mesh.cpp", "qgd_partition.cpp", "qgd_setup.cpp")]
    objects = [str(tmp_path / (name + "_" + os.path.basename(s) + ".o")) for s in sources]
    # (the four units side by side: the sanitized build of the builder is the slow part of this file)
    jobs = [subprocess.Popen(["g++", "-std=c++17", "-fopenmp", *flags, "-I", CSRC, "-c", s, "-o", o], stderr=subprocess.PIPE, text=True)
            for s, o in zip(sources, objects)]
    for j in jobs:
        err = j.communicate()[1]
        assert j.returncode == 0, err[-3000:]
    r = subprocess.run(["g++", "-fopenmp", *flags, *objects, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(exe, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("QGD_FUSED_PACKED_W", "QGD_FUSED_PACKED_F", "QGD_FUSED_PACKED_G")}
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=dict(env, OMP_NUM_THREADS="4"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_uniform_meshes_pack_their_geometry_and_decode_exactly(tmp_path):
    exe = build(tmp_path, "fused_packed_geometry_test", ["-O2"])
    out = run(exe)
    print(out)
    for tag in ("box 17x9x9", "box 40x20x20", "box 16x8x12", "box 3x2x2", "box 9x5x5", "box 50x50x50", "slab 3..9 of a 12x6x12 box",
                "slab 0..12 of a 400x400x400 box", "shard 0 of 2 of box 16x8x12", "shard 1 of 2 of box 16x8x12"):
        assert f"{tag}: " in out and "largest dictionary" in out
    assert "16 entries on an axis: " in out and "largest offset 4095" in out
    assert out.count("not packed, arrays kept") == 3
    wide = run(exe, *[recipes.argument(r) for r in recipes.RECIPES.values()])
    print(wide)
    for r in recipes.RECIPES.values():
        assert f"recipe {r.tag}: " in wide


def test_the_geometry_packing_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = build(tmp_path, "fused_packed_geometry_test_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    out = run(exe) + run(exe, *[recipes.argument(r) for r in recipes.RECIPES.values()])
    assert "runtime error" not in out
