"""The filtered guide-site calls timed on the bench genome recipe (bench.build_genome; scale 1 = hg38-sized), alone on the chip,
interleaved round by round in ONE process: python tools/site_filters_speed.py [scale] [rounds] [--unfiltered] [--tree DIR]

  count plain   : calitas_count_sites of NNNNNNNNNNNNNNNNNNNNnrg over the whole genome, no filter (sites_kernel<false, false>)
  count open    : the same through calitas_count_sites_filtered with a filter that has nothing set (what the scalar branches cost)
  count gc      : G + C of 40 - 60 % (8 .. 12 of 20)
  count runs3   : no run longer than 3 of any base
  count t3      : no run of T longer than 3
  count bsmbi   : no CGTCTC, no GAGACG
  count all     : G + C of 40 - 60 %, runs A C G <= 4 and T <= 3, no CGTCTC, GAGACG, GGNCC
  find 1 Mb     : calitas_find_sites of one 1-Mb region, no filter (both passes, the records copied back and handed to numpy)
  find 1 Mb all : the same with the filter `all`

A call is timed by the host clock around it (it ends in a stream synchronise).  Per call: median / min / quartiles in ms and the share
of the unfiltered sites the filter keeps.  Before timing, the region's filtered listing is checked against the host twin and against
the unfiltered listing (a subsequence of it), and every count against its per-contig table.
--unfiltered: `count plain` alone, which a checkout from before the filters has too; --tree DIR takes package and library from another
checkout (built), as tools/scores_speed.py does.  With both, two builds are compared on the unfiltered count, whole processes
alternated:  python tools/site_filters_speed.py 1.0 20 --unfiltered --tree PARENT  against  ... --unfiltered.  (tools/ab_lib.sh
alternates two libraries the same way, but what it times is calitas_search_hits through tools/ab_env.py, not the site calls, and it
loads the other library into this tree's package, which needs every symbol this tree declares.)"""
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
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    plain_only = "--unfiltered" in sys.argv[1:]
    if "--tree" in sys.argv:
        tree = sys.argv[sys.argv.index("--tree") + 1]
        args.remove(tree)
        sys.path.insert(0, os.path.abspath(tree))              # (in front of this checkout)
    scale = float(args[0]) if len(args) > 0 else 1.0
    rounds = int(args[1]) if len(args) > 1 else 20
    import torch
    import bench
    import calitas_amd as C
    names, seqs = bench.build_genome(scale, torch.device("cuda", 0), contig_indices=None, guides=[bench.GUIDE0], log=None)
    ctx = C.Context(0)
    ctx.set_reference(names, seqs, genome_build="synthetic")
    del seqs
    bases = ctx.reference_info()["total_bases"]
    n20 = C.Guide("NNNNNNNNNNNNNNNNNNNNnrg")
    big = max(range(len(names)), key=lambda i: ctx.contig_lengths[i])
    r0 = min(10_000_000, max(0, ctx.contig_lengths[big] - 1_000_000) // 2)
    r1 = min(ctx.contig_lengths[big], r0 + 1_000_000)
    region = dict(chrom=big, start=r0, end=r1)

    total, table = ctx.count_sites(n20)
    assert int(table.sum()) == total
    calls = {"count plain": lambda: ctx.count_sites(n20)}
    kept = {"count plain": total}
    if not plain_only:
        bsmbi = ("CGTCTC", "GAGACG")
        filters = {
            "open": C.SiteFilter(),
            "gc": C.SiteFilter(*C.SiteFilter.percent(20, 40, 60)),
            "runs3": C.SiteFilter(max_run=3),
            "t3": C.SiteFilter(max_run={"T": 3}),
            "bsmbi": C.SiteFilter(avoid=bsmbi),
            "all": C.SiteFilter(*C.SiteFilter.percent(20, 40, 60), max_run=(4, 4, 4, 3), avoid=bsmbi + ("GGNCC",)),
        }
        listing = ctx.find_sites(n20, **region)
        some = ctx.find_sites(n20, filter=filters["all"], **region)
        assert some.tobytes() == ctx.find_sites(n20, host=True, filter=filters["all"], **region).tobytes(), "the kernel and the host twin differ"
        left = iter(listing.tolist())
        assert all(any(rec == other for other in left) for rec in some.tolist()), "the filtered listing is no subsequence of the unfiltered one"
        for name, flt in filters.items():
            n, table = ctx.count_sites(n20, filter=flt)
            assert int(table.sum()) == n and n <= total and (name != "open" or n == total)
            kept["count " + name] = n
            calls["count " + name] = lambda flt=flt: ctx.count_sites(n20, filter=flt)
        calls["find 1 Mb"] = lambda: ctx.find_sites(n20, **region)
        calls["find 1 Mb all"] = lambda: ctx.find_sites(n20, filter=filters["all"], **region)
        kept["find 1 Mb"], kept["find 1 Mb all"] = len(listing), len(some)
        print("checked: %d of %d sites in %s:%d-%d pass `all`, as the host twin has it" % (len(some), len(listing), names[big], r0, r1), flush=True)
    print("%d N20+nrg sites in %d bases" % (total, bases), flush=True)

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
        whole = kept["find 1 Mb"] if k.startswith("find") else total
        print("%-14s scale %g: median %.3f ms  min %.3f  p25 %.3f  p75 %.3f | keeps %d of %d (%.4f)" % (
            k, scale, med, lo, q1, q3, kept[k], whole, kept[k] / max(1, whole)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
