"""Extended seeded fuzz of the kernels around SGBM (resize, depth, fixed-point remap, median, rectify tables) against
their references, by hand on a GPU box:
    CAMD_GIT_SHA=<sha> python tools/gpu_fuzz_post.py N [first_seed [n_seeds]] [--only=NAME[,NAME...]]
N cases of every fuzzer for each of n_seeds consecutive seeds (tests/fuzzers.py holds the generators; the driver's GPU
suite runs bounded slices of the same).  Prints one FUZZ line per fuzzer and seed: git SHA, library hash, seed,
per-branch counts, mismatches."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: F401,E402
import oracle  # noqa: E402
import fuzzers  # noqa: E402

oracle.build()
args = [a for a in sys.argv[1:] if not a.startswith("--only")]
only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")]
names = only[0].split(",") if only else sorted(fuzzers.POST_FUZZERS)
n = int(args[0]) if args else 200
first = int(args[1]) if len(args) > 1 else 1000
total = 0
for seed in range(first, first + (int(args[2]) if len(args) > 2 else 1)):
    for name in names:
        res = fuzzers.POST_FUZZERS[name][1](n, seed, log=lambda *a: print(*a, flush=True))
        fuzzers.report(res, log=lambda *a: print(*a, flush=True))
        total += len(res["mismatches"])
sys.exit(1 if total else 0)
