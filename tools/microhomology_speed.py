"""calitas_find_sites_microhomology timed on the bench genome recipe (bench.build_genome; scale 1 = hg38-sized), alone on the chip,
interleaved round by round in ONE process: python tools/microhomology_speed.py [scale] [rounds]

For N20 + nrg, the cut at L - 3 and the example model's shape (30 + 30 bases, exp(-d / 20), min_length 2), over a 10-kb region, a 1-Mb
region, the largest contig and the whole genome:

  find    : calitas_find_sites -- the yardstick, a call this scoring does not touch
  mh      : calitas_find_sites_microhomology without a threshold (every record and its two sums come back)
  mh667   : calitas_find_sites_microhomology with min_out_of_frame_permille = 667 (the kept records and sums come back)
  twin    : today's way, the sites listed and every window walked on the host: calitas_find_sites_microhomology_host, without and with
            the threshold, once each; left out, and said so, for regions of more than TWIN_MOST bases

A call is timed by the host clock around the library call, blocks freed inside it (it ends in a stream synchronise and hands over
blocks of the library's; no numpy copy is made).  Every device row is first called once, shown as `first call`: it sizes the buffers.
Then median / min / quartiles in ms over the rounds -- five calls per round for calls under 0.5 s, one otherwise, three rounds for calls
over 2 s -- and per region the ratios mh / find and mh667 / find.  No ratio is a pass criterion.
Before timing, the 10-kb region's records and scores are held against the host twin with and without the threshold."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FEW_OVER_S = 2.0
TWIN_MOST = 60_000_000
PERMILLE = 667


def quart(t):
    t = sorted(t)
    n = len(t)
    return t[n // 2], t[0], t[n // 4], t[3 * n // 4]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    scale = float(args[0]) if len(args) > 0 else 1.0
    rounds = int(args[1]) if len(args) > 1 else 10
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
    model = C.MicrohomologyModel.exponential(20.0, 30, 30)
    m = model.to_c(17)
    big = max(range(len(names)), key=lambda i: ctx.contig_lengths[i])
    mid = max(0, ctx.contig_lengths[big] - 1_000_000) // 2

    def find(chrom, start, end):
        out, n = ctypes.POINTER(C._lib.SiteT)(), ctypes.c_uint64()
        C._lib.check(ctx._h, lib.calitas_find_sites(ctx._h, ctypes.byref(g), chrom, start, end, ctypes.byref(out), ctypes.byref(n)))
        lib.calitas_free(out)
        return n.value

    def scored(chrom, start, end, permille, host=False):
        out, words, n = ctypes.POINTER(C._lib.SiteT)(), ctypes.POINTER(C._lib.MhScoreT)(), ctypes.c_uint64()
        fn = lib.calitas_find_sites_microhomology_host if host else lib.calitas_find_sites_microhomology
        C._lib.check(ctx._h, fn(ctx._h, ctypes.byref(g), None, ctypes.byref(m), permille, chrom, start, end, ctypes.byref(out), ctypes.byref(words),
                                ctypes.byref(n)))
        lib.calitas_free(out)
        lib.calitas_free(words)
        return n.value

    for permille in (0, PERMILLE):
        a = ctx.find_sites_microhomology(n20, model, 17, permille, chrom=big, start=mid, end=mid + 10_000)
        b = ctx.find_sites_microhomology(n20, model, 17, permille, chrom=big, start=mid, end=mid + 10_000, host=True)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), "the kernels and the host twin differ"
    print("checked: the 10-kb region against the host twin, with and without the threshold of %d per mille" % PERMILLE, flush=True)

    regions = {"10 kb": (big, mid, mid + 10_000), "1 Mb": (big, mid, mid + 1_000_000), "contig": (big, 0, 0), "genome": (-1, 0, 0)}
    size = {"10 kb": 10_000, "1 Mb": 1_000_000, "contig": ctx.contig_lengths[big], "genome": bases}
    calls, first, info = {}, {}, {}
    for label, r in regions.items():
        for what, fn in (("find", lambda r=r: find(*r)), ("mh", lambda r=r: scored(*r, 0)), ("mh667", lambda r=r: scored(*r, PERMILLE))):
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
    for label, r in regions.items():
        print("%-14s mh / find %.2f, mh667 / find %.2f (%d bases in the genome)" % (
            label, med["mh " + label] / med["find " + label], med["mh667 " + label] / med["find " + label], bases), flush=True)
        if size[label] > TWIN_MOST:
            print("%-14s twin left out: %d bases" % (label, size[label]), flush=True)
            continue
        for permille in (0, PERMILLE):
            t0 = time.perf_counter()
            n = scored(*r, permille, host=True)
            dt = (time.perf_counter() - t0) * 1e3
            arm = "mh" if permille == 0 else "mh667"
            print("%-14s twin, %s: one call %.3f ms, %d records; twin / %s %.1f" % (label, arm, dt, n, arm, dt / med[arm + " " + label]), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
