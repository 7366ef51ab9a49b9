"""The per-face streams of the fused step block-major and packed, host side (CPU): qgd_setup.cpp packFusedFaceStreams checked by
tests/cpp/fused_packed_faces_test.cpp, compiled with plain g++ from the library's own host sources -- no HIP, no oracle.  Uniform boxes (13x7x5,
17x9x9 with two classes of hQGDf, 16x8x12 with three, 50^3, 100x20x20) and a slab shard qualify and decode to the mesh's w / hQGDf / kind bit for
bit, with the same references, classes and tables under 1 and 4 threads and zero padding slots; the rule holds on streams written by hand (a
spread of w of 65 535 packs, 65 536 does not; four classes of hQGDf pack, five do not; a class straddling a power of two decodes exactly; a
negative value does not pack; weights not packed means faces not packed; QGD_FUSED_PACKED_F=0 builds no tables); jittered meshes and a 2:1 graded
box keep their streams alone.  A second build runs the same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code with its
own main: no GPU, nothing preloaded)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qgdsolver_amd", "csrc")


def build_and_run(tmp_path, name, flags=()):
    exe = str(tmp_path / name)
    sources = [os.path.join(ROOT, "tests", "cpp", "fused_packed_faces_test.cpp")] + \
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
    env = {k: v for k, v in os.environ.items() if k not in ("QGD_FUSED_PACKED_W", "QGD_FUSED_PACKED_F")}
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(env, OMP_NUM_THREADS="4"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_uniform_meshes_pack_their_face_streams_and_decode_exactly(tmp_path):
    out = build_and_run(tmp_path, "fused_packed_faces_test", ["-O2"])
    print(out)
    for tag in ("box 13x7x5", "box 17x9x9", "box 16x8x12", "box 50x50x50", "box 100x20x20", "slab 3..9 of a 12x6x12 box"):
        assert f"{tag}: " in out and "largest |offset|" in out
    assert "box 17x9x9: " in out and "hf in 2 classes" in out and "hf in 3 classes" in out
    assert out.count("not packed, streams kept") == 3


def test_the_face_packing_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    out = build_and_run(tmp_path, "fused_packed_faces_test_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "runtime error" not in out
