"""Time outside the steps of a plain bench.py run: each run is a fresh process, timed from start to exit, less
(steps + warmup) x ms_per_step.  Prints one JSON line per run, then the median.
    python scripts/plain_run_timing.py [--repeat R] [bench.py arguments, default --gpus 1 --steps 20 --warmup 5]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(bench_args):
    t0 = time.perf_counter()
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + bench_args, capture_output=True, text=True, cwd=ROOT)
    wall = time.perf_counter() - t0
    if pr.returncode != 0:
        sys.exit(f"bench.py exited {pr.returncode}: {pr.stderr[-600:]}")
    d = json.loads([ln for ln in pr.stdout.splitlines() if ln.startswith("{")][-1])
    steps_s = (d["steps"] + d["warmup"]) * d["ms_per_step"] * 1e-3
    return {"wall_s": wall, "steps": d["steps"], "warmup": d["warmup"], "ms_per_step": d["ms_per_step"], "steps_s": steps_s,
            "outside_steps_s": wall - steps_s, "setup_s": d.get("setup_s"), "value": d["value"]}


def main():
    args = sys.argv[1:]
    repeat = 3
    if args[:1] == ["--repeat"]:
        repeat, args = int(args[1]), args[2:]
    args = args or ["--gpus", "1", "--steps", "20", "--warmup", "5"]
    runs = []
    for _ in range(repeat):
        runs.append(one(args))
        print(json.dumps(runs[-1]), flush=True)
    print(json.dumps({"args": args, "runs": repeat, "median_outside_steps_s": statistics.median(r["outside_steps_s"] for r in runs),
                      "median_setup_s": statistics.median(r["setup_s"] for r in runs)}), flush=True)


if __name__ == "__main__":
    main()
