"""The guide-site calls timed on the bench genome recipe (bench.build_genome; scale 1 = hg38-sized), alone on the chip, interleaved
round by round in ONE process: python tools/sites_speed.py [scale] [rounds]

  count N20+nrg : calitas_count_sites of NNNNNNNNNNNNNNNNNNNNnrg over the whole genome (the kernel's first pass, a few KB back)
  count N20 1seg: the same with CALITAS_SITES_SEGS=1, a workgroup per 256 words (what the default of sixteen is measured against)
  count 23-mer  : the same for a fully specified 20-mer + tgg (every position costs a letter)
  count 1 Mb    : calitas_count_sites of N20+nrg for one 1-Mb region (what a call costs when the kernel has next to nothing to do)
  find 1 Mb     : calitas_find_sites of the same region (both passes, the records copied back and handed to numpy)

A call is timed by the host clock around it (it ends in a stream synchronise).  Per call: median / min / quartiles in ms; for the
whole-genome counts also the bases per second and the GB/s of the bit-planes (0.25 B/base; the exception mask the kernel reads
as well is half as much again).  Before timing, the region's listing is checked against the host twin and the counts against it."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def quart(t):
    t = sorted(t)
    n = len(t)
    return t[n // 2], t[0], t[n // 4], t[3 * n // 4]


def main():
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    import torch
    import bench
    import calitas_amd as C
    names, seqs = bench.build_genome(scale, torch.device("cuda", 0), contig_indices=None, guides=[bench.GUIDE0], log=None)
    ctx = C.Context(0)
    ctx.set_reference(names, seqs, genome_build="synthetic")
    del seqs
    bases = ctx.reference_info()["total_bases"]
    n20, fixed = C.Guide("NNNNNNNNNNNNNNNNNNNNnrg"), C.Guide(bench.GUIDE0[:20] + "tgg")
    big = max(range(len(names)), key=lambda i: ctx.contig_lengths[i])
    r0 = min(10_000_000, max(0, ctx.contig_lengths[big] - 1_000_000) // 2)
    r1 = min(ctx.contig_lengths[big], r0 + 1_000_000)

    listing = ctx.find_sites(n20, chrom=big, start=r0, end=r1)
    assert listing.tobytes() == ctx.find_sites(n20, chrom=big, start=r0, end=r1, host=True).tobytes(), "the kernel and the host twin differ"
    assert ctx.count_sites(n20, chrom=big, start=r0, end=r1)[0] == len(listing)
    total, table = ctx.count_sites(n20)
    assert int(table.sum()) == total
    print("checked: %d sites in %s:%d-%d equal the host twin's; %d N20+nrg sites and %d of the 23-mer in %d bases" % (
        len(listing), names[big], r0, r1, total, ctx.count_sites(fixed)[0], bases), flush=True)

    def one_segment(fn):                                        # a workgroup per segment of 256 words instead of sixteen
        def run():
            os.environ["CALITAS_SITES_SEGS"] = "1"
            try:
                return fn()
            finally:
                del os.environ["CALITAS_SITES_SEGS"]
        return run

    calls = {
        "count N20+nrg": lambda: ctx.count_sites(n20),
        "count N20 1seg": one_segment(lambda: ctx.count_sites(n20)),
        "count 23-mer": lambda: ctx.count_sites(fixed),
        "count 1 Mb": lambda: ctx.count_sites(n20, chrom=big, start=r0, end=r1),
        "find 1 Mb": lambda: ctx.find_sites(n20, chrom=big, start=r0, end=r1),
    }
    res = {k: [] for k in calls}
    for r in range(rounds + 2):                                 # (two rounds of warm-up: buffers sized, clocks up)
        for k, fn in calls.items():
            reps = 5
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            dt = (time.perf_counter() - t0) * 1e3 / reps
            if r >= 2:
                res[k].append(dt)
    for k in calls:
        med, lo, q1, q3 = quart(res[k])
        line = "%-14s scale %g: median %.3f ms  min %.3f  p25 %.3f  p75 %.3f" % (k, scale, med, lo, q1, q3)
        if k.startswith("count") and "Mb" not in k:
            line += " | %.0f Gbase/s, %.0f GB/s of bit-planes" % (bases / med / 1e6, bases * 0.25 / med / 1e6)
        elif k.startswith("find"):
            line += " | %d records, %d bytes" % (len(listing), listing.nbytes)
        print(line, flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
