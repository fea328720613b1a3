"""calitas_find_sites_scored timed on the bench genome recipe (bench.build_genome; scale 1 = hg38-sized), alone on the chip, interleaved
round by round in ONE process: python tools/activity_speed.py [scale] [rounds] [--once]

For N20 + nrg and a model with four bases before and six behind the protospacer (W = 30, every weight drawn at random), over a 10-kb
region, a 1-Mb region, the largest contig and the whole genome:

  find    : calitas_find_sites -- the yardstick, a call this scoring does not touch
  scored  : calitas_find_sites_scored without a threshold (every record and a score each come back)
  tenth   : calitas_find_sites_scored with a threshold that keeps about a tenth (taken from the 1-Mb region's scores)

A call is timed by the host clock around the library call, blocks freed inside it (it ends in a stream synchronise and hands over
blocks of the library's; no numpy copy is made).  Every row is first called once, shown as `first call`: it sizes the buffers.  Then
median / min / quartiles in ms over the rounds -- five calls per round for calls under 0.5 s, one otherwise, three rounds for calls over
2 s -- and per region the ratios scored / find and tenth / find.  No ratio is a pass criterion.
Before timing, the 10-kb region's records and scores are held against the host twin with and without the threshold, and the threshold's
share is printed.  --once: one call of each whole-genome row and nothing else (for a run under a profiler)."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FEW_OVER_S = 2.0


def quart(t):
    t = sorted(t)
    n = len(t)
    return t[n // 2], t[0], t[n // 4], t[3 * n // 4]


def main():
    argv = sys.argv[1:]
    once = "--once" in argv
    args = [a for a in argv if not a.startswith("--")]
    scale = float(args[0]) if len(args) > 0 else 1.0
    rounds = int(args[1]) if len(args) > 1 else 10
    import numpy as np
    import torch
    import bench
    import calitas_amd as C
    lib = C._lib.lib
    names, seqs = bench.build_genome(scale, torch.device("cuda", 0), contig_indices=None, guides=[bench.GUIDE0], log=None)
    ctx = C.Context(0)
    ctx.set_reference(names, seqs, genome_build="synthetic")
    del seqs
    bases = ctx.reference_info()["total_bases"]
    n20 = C.Guide("N" * 20 + "nrg")
    g = n20.to_c()
    rng = np.random.default_rng(30)
    draw = lambda *shape: rng.integers(-(1 << 15), (1 << 15) + 1, size=shape, dtype=np.int32)      # noqa: E731 (+-0.5)
    model = C.ActivityModel(20, 4, 6, draw(30, 4), draw(29, 16), draw(21), 0, "logistic")
    m = model.to_c()
    big = max(range(len(names)), key=lambda i: ctx.contig_lengths[i])
    mid = max(0, ctx.contig_lengths[big] - 1_000_000) // 2

    def find(chrom, start, end):
        out, n = ctypes.POINTER(C._lib.SiteT)(), ctypes.c_uint64()
        C._lib.check(ctx._h, lib.calitas_find_sites(ctx._h, ctypes.byref(g), chrom, start, end, ctypes.byref(out), ctypes.byref(n)))
        lib.calitas_free(out)
        return n.value

    def scored(chrom, start, end, floor):
        out, words, n = ctypes.POINTER(C._lib.SiteT)(), ctypes.POINTER(ctypes.c_int32)(), ctypes.c_uint64()
        C._lib.check(ctx._h, lib.calitas_find_sites_scored(ctx._h, ctypes.byref(g), None, ctypes.byref(m), floor, chrom, start, end, ctypes.byref(out),
                                                            ctypes.byref(words), ctypes.byref(n)))
        lib.calitas_free(out)
        lib.calitas_free(words)
        return n.value

    # the threshold that keeps about a tenth, and the device against the host twin on the small region
    _, mb = ctx.find_sites_scored(n20, model, chrom=big, start=mid, end=mid + 1_000_000)
    have = np.sort(mb[mb != C.ACTIVITY_NONE])
    floor = int(have[(9 * len(have)) // 10])
    for f in (None, floor):
        a = ctx.find_sites_scored(n20, model, f, chrom=big, start=mid, end=mid + 10_000)
        b = ctx.find_sites_scored(n20, model, f, chrom=big, start=mid, end=mid + 10_000, host=True)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), "the kernels and the host twin differ"
    print("checked: the 10-kb region against the host twin, with and without the threshold %d (%.4f), which keeps %d of the 1-Mb region's %d sites" % (
        floor, floor / 65536.0, int((mb >= floor).sum()), len(mb)), flush=True)

    regions = {"10 kb": (big, mid, mid + 10_000), "1 Mb": (big, mid, mid + 1_000_000), "contig": (big, 0, 0), "genome": (-1, 0, 0)}
    if once:
        for what, fn in (("find", lambda r: find(*r)), ("scored", lambda r: scored(*r, C.ACTIVITY_NONE)), ("tenth", lambda r: scored(*r, floor))):
            for _ in range(2):                                  # (the first call sizes the buffers)
                t0 = time.perf_counter()
                n = fn(regions["genome"])
                print("%-14s genome: one call %.1f ms, %d records" % (what, (time.perf_counter() - t0) * 1e3, n), flush=True)
        ctx.close()
        return

    calls, first, info = {}, {}, {}
    for label, r in regions.items():
        for what, fn in (("find", lambda r=r: find(*r)), ("scored", lambda r=r: scored(*r, C.ACTIVITY_NONE)), ("tenth", lambda r=r: scored(*r, floor))):
            name = "%s %s" % (what, label)
            t0 = time.perf_counter()
            n = fn()
            first[name] = time.perf_counter() - t0
            info[name] = "%d records" % n
            calls[name] = fn
            print("%-14s first call %.3f s, %d records" % (name, first[name], n), flush=True)
    res = {k: [] for k in calls}
    for r in range(rounds + 2):                                 # (two rounds of warm-up: buffers sized, clocks up)
        for k, fn in calls.items():
            if first[k] > FEW_OVER_S and r >= 5:
                continue
            reps = 1 if first[k] > 0.5 else 5
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            dt = (time.perf_counter() - t0) * 1e3 / reps
            if r >= 2:
                res[k].append(dt)
    med = {}
    for k in calls:
        med[k], lo, q1, q3 = quart(res[k])
        print("%-14s scale %g: median %.3f ms  min %.3f  p25 %.3f  p75 %.3f | %s" % (k, scale, med[k], lo, q1, q3, info[k]), flush=True)
    for label in regions:
        print("%-14s scored / find %.2f, tenth / find %.2f (%d bases in the genome)" % (
            label, med["scored " + label] / med["find " + label], med["tenth " + label] / med["find " + label], bases), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
