"""Records of the exhaustive sweeps (tests/exhaustive_cases.py) for profiles/: --part cpu writes the table of tap-order mutants
against the CPU sets (no GPU needed), --part gpu per sweep and metric the frames, pixels, family shares from pass_stats() on the
default path, and the seconds of the pass and of the oracle.  Usage: python scripts/exhaustive_profile.py --part cpu|gpu --out FILE"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import exhaustive_cases as E  # noqa: E402
import parallel_model as PM  # noqa: E402
from oracle import oracle as O  # noqa: E402


def cpu_part(out):
    from test_exhaustive_cases import ALL_MUTANTS, MUTANTS_THAT_MATTER, mismatches, swapped

    sets = dict(E.cpu_sets())
    rng = np.random.default_rng(123)  # tests/test_parallel_model.py::test_small_random's frames
    rand = []
    for t in range(600):
        H, W = int(rng.integers(2, 24)), int(rng.integers(2, 30))
        p = rng.choice([0.01, 0.03, 0.1, 0.3, 0.6])
        x = np.where(rng.random((H, W)) < p, 5.0, 0.0).astype(np.float32)
        if t % 7 == 0:
            x[: H // 2] = 0
        if t % 11 == 0:
            x[:, W // 2:] = 0
        rand.append(x)
    labels = {name: O.fill_batch(x)[2] for name, x in sets.items()}
    rand_lbl = [O.nearest_point(x)[1] if (x >= 0.9).any() else None for x in rand]
    names = list(sets)
    print("tap-order mutants of tests/parallel_model.py (entries i and i + 1 of the table swapped): frames whose labels differ from the oracle's", file=out)
    print("%-8s %12s" % ("mutant", "random600") + "".join(" %20s" % n for n in names) + "   expected to matter", file=out)
    print("%-8s %12d" % ("frames", len(rand)) + "".join(" %20d" % len(sets[n]) for n in names), file=out)
    for table, i in ALL_MUTANTS:
        with swapped(table, i):
            nr = sum(1 for x, l in zip(rand, rand_lbl) if l is not None and not np.array_equal(PM.nearest_point(x)[1], l))
            row = [mismatches(sets[n], labels[n]) for n in names]
        print("%-8s %12d" % ("%s %d-%d" % (table, i, i + 1), nr) + "".join(" %20d" % v for v in row) +
              ("   yes" if (table, i) in MUTANTS_THAT_MATTER else "   no"), file=out)


def gpu_part(out):
    import torch

    pkg = importlib.import_module("distancetransform-depthcompletion_amd")
    pkg._lib.load()
    ops = {m: pkg.device.DtFill(device="cuda:0", metric=m) for m in ("l1_cv", "l2")}
    keys = ("window", "anydist", "sky", "points")
    print("exhaustive sweeps on the default path: frames, pixels, share of the pixels per kernel family (pass_stats), seconds", file=out)
    print("(route: frame_facts' rule as tests/exhaustive_cases.py restates it, on mask 0: 16 / 32 = the window kernel's halo (l2: k_l2win with", file=out)
    print(" radius 10 / 15), pts = k_pts (l2: the points route), any = the any-distance kernels (l2: the row search))", file=out)
    print("%-22s %-6s %5s %7s %10s" % ("sweep", "metric", "route", "frames", "pixels") + "".join(" %8s" % k for k in keys) + " %9s %9s" % ("gpu_s", "oracle_s"), file=out)

    def one(name, x, metric):
        t0 = time.perf_counter()
        O.fill_batch(x, metric=metric)
        t_or = time.perf_counter() - t0
        xd = torch.from_numpy(np.array(x, np.float32)).to("cuda:0")
        op = ops[metric]
        op.run(xd)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        op.run(xd)
        torch.cuda.synchronize()
        t_gpu = time.perf_counter() - t0
        s = op.pass_stats()
        r = {16: "16", 32: "32", -1: "pts", 0: "any"}[E.route(E.sources(x[0]), metric)["r"]]
        print("%-22s %-6s %5s %7d %10d" % (name, metric, r, len(x), x.size) + "".join(" %8.4f" % (s[k] / s["all"]) for k in keys) +
              " %9.5f %9.3f" % (t_gpu, t_or), file=out)
        out.flush()
        return s

    sky = []
    for H, W in E.WHOLE_SHAPES:
        for metric in ("l1_cv", "l2"):
            one("whole %dx%d" % (H, W), E.whole_frames(H, W), metric)
    for fam, anchor in E.sweep_names():
        x, _ = E.sweep(fam, anchor)
        for metric in ("l1_cv", "l2"):
            s = one("%s/%s" % (fam, anchor), x, metric)
            if fam == "sky" and metric == "l1_cv":
                r0 = E.sky_first_rows(fam, anchor)
                sky.append((anchor, s["sky"], int(r0.sum()) * x.shape[2]))
    print("\nsky sweeps, l1_cv: pixels k_sky owned against sum over the frames of r0 * W (every frame's sky, were none called off)", file=out)
    for anchor, got, full in sky:
        print("sky/%-10s sky %9d of %9d (%.4f)" % (anchor, got, full, got / full), file=out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("cpu", "gpu"), required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        (cpu_part if a.part == "cpu" else gpu_part)(f)
