"""The packed tables of the fused step at offsets that use all 16 bits, host side (CPU): tests/cpp/fused_packed_wide_test.cpp, compiled with plain
g++ from the library's own host sources -- no HIP, no oracle -- and given the recipes of tests/packed_wide_recipes.py on its command line.  For
every recipe the tables are the same under 1 and 4 threads, the flags, classes and offset floors are what the list says, every used slot decodes
to the mesh's vW / w / hQGDf / kind bit for bit, and seven WRONG decodes (low byte only, zero-extended half word, offset taken as 0, the half
words of a face word swapped, the halves of a pair of weight offsets swapped, class forced to 0, class 3 read as class 2) each change at least
1 % of the used slots, one of them by more than 4096 patterns.

The recorded reason for this file: on the uniform boxes that the packed GPU tests ran on before -- 17x9x9, 16x8x12, 9x5x5 -- "low byte only"
changes ZERO slots, and "offset taken as 0" changes them by 64 patterns at most (1.4e-14 relative).  Those boxes alone could not tell such a
decode from the right one.

A second build runs the same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code with its own main: no GPU, nothing
preloaded)."""
import os
import re
import subprocess

import packed_wide_recipes as recipes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qgdsolver_amd", "csrc")


def build_and_run(tmp_path, name, flags=()):
    exe = str(tmp_path / name)
    sources = [os.path.join(ROOT, "tests", "cpp", "fused_packed_wide_test.cpp")] + \
              [os.path.join(CSRC, f) for f in ("qgd_mesh.cpp", "qgd_partition.cpp", "qgd_setup.cpp")]
    objects = [str(tmp_path / (name + "_" + os.path.basename(s) + ".o")) for s in sources]
    jobs = [subprocess.Popen(["g++", "-std=c++17", "-fopenmp", *flags, "-I", CSRC, "-c", s, "-o", o], stderr=subprocess.PIPE, text=True)
            for s, o in zip(sources, objects)]
    for j in jobs:
        err = j.communicate()[1]
        assert j.returncode == 0, err[-3000:]
    r = subprocess.run(["g++", "-fopenmp", *flags, *objects, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    args = [recipes.argument(x) for x in recipes.RECIPES.values()] + [recipes.uniform_argument(s) for s in recipes.UNIFORM]
    env = {k: v for k, v in os.environ.items() if k not in ("QGD_FUSED_PACKED_W", "QGD_FUSED_PACKED_F")}
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=dict(env, OMP_NUM_THREADS="4"))
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-6000:] + r.stderr[-4000:]
    return r.stdout


MUTANT = re.compile(r"^(.*): mutant '(.*)': weights (\d+) of (\d+) changed, worst (\d+); faces (\d+) of (\d+) changed, worst (\d+)$", re.M)
TABLES = re.compile(r"^(.*): packedWeights (\d) offsets \[(-?\d+), (-?\d+)\], packedFaces (\d) hfClasses (\d) w offsets \[(-?\d+), (-?\d+)\] "
                    r"hf offsets \[(-?\d+), (-?\d+)\] slots per class (\d+) (\d+) (\d+) (\d+)$", re.M)


def test_wide_recipes_pack_as_listed_and_wrong_decodes_show_where_uniform_boxes_hide_them(tmp_path):
    out = build_and_run(tmp_path, "fused_packed_wide_test", ["-O2"])
    tables = {m.group(1): m for m in TABLES.finditer(out)}
    mutants = {(m.group(1), m.group(2)): [int(x) for x in m.groups()[2:]] for m in MUTANT.finditer(out)}
    # the program judged the recipes; the printout holds every figure the judgement rests on
    for r in recipes.RECIPES.values():
        t = tables[r.tag]
        assert (int(t.group(2)), int(t.group(5)), int(t.group(6))) == (int(r.packedWeights), int(r.packedFaces), r.hfClasses), (r, t.group(0))
        if r.packedWeights:
            assert (r.tag, "low byte only") in mutants and (r.tag, "weight pair halves swapped") in mutants, r
        if r.packedFaces:
            assert (r.tag, "face half words swapped") in mutants and (r.tag, "class forced to 0") in mutants, r
        assert ((r.tag, "class 3 read as class 2") in mutants) == (r.hfClasses == 4), r
    four = [r for r in recipes.RECIPES.values() if r.hfClasses == 4]
    assert four and all(int(x) > 0 for x in tables[four[0].tag].groups()[10:14]), "no recipe with four populated classes of hQGDf"
    # the uniform boxes: the low byte is all there is, and leaving the offset out is within rounding of right
    for shape in recipes.UNIFORM:
        tag = "uniform box " + "x".join(str(n) for n in shape)
        w_changed, w_used, _, f_changed, f_used, _ = mutants[(tag, "low byte only")]
        assert w_used > 0 and f_used > 0 and w_changed == 0 and f_changed == 0, (tag, mutants[(tag, "low byte only")])
        _, _, w_worst, _, _, f_worst = mutants[(tag, "offset taken as 0")]
        assert max(w_worst, f_worst) < 128, (tag, w_worst, f_worst)


def test_the_wide_recipes_are_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    out = build_and_run(tmp_path, "fused_packed_wide_test_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "runtime error" not in out
