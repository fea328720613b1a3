"""calitas_find_site_pairs timed on one contig of the bench genome recipe (bench.build_genome), alone on the chip, in ONE process:
python tools/site_pairs_speed.py [contig index = 20] [rounds = 5]

For N20 + nrg over a 10-kb region, a 1-Mb region and the whole contig, at two shapes -- "-+" with the cuts 30 .. 150 apart (paired
nickases) and any orientation with the cuts 1000 .. 5000 apart (an excision) -- these arms:

  count   : calitas_count_site_pairs (both site passes, the count kernel, no block comes back)
  pairs   : calitas_find_site_pairs (the same and the write kernel, records and pairs copied back once each); left out, and said so,
            where the pairs of the region are more than 2^27 (two gigabytes of records)
  find    : calitas_find_sites of the same region -- the listing a user pairs on the host today
  + walk  : the host twin's walk over that listing: the time of calitas_find_site_pairs_host less the time of
            calitas_find_sites_host over the same region (both enumerate the sites base by base; what is left is the walk and its block).
            find + walk is the baseline "the device lists, the host pairs".  Left out where the listing has more than 2^22 sites.
  + loop  : calitas_amd.site_pairs_of, the plain Python double loop, over find's records: find + loop is the baseline "pair in a
            Python loop".  Left out where the listing has more than 4000 sites: it is quadratic.

A call is timed by the host clock around the library call, blocks freed inside it and the library's deferred frees waited for
(calitas_reap_wait).  Every device arm is first called once (it sizes the buffers), then median / min / max over the rounds; the host arms
run once.  Where both exist the device's pairs are held against the host twin's byte for byte before timing.  No ratio is a pass
criterion."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("-+ 30..150", 30, 150, ["-+"]), ("any 1000..5000", 1000, 5000, ["++", "-+", "+-", "--"]))
MOST_PAIRS = 1 << 27
MOST_HOST_SITES = 1 << 22
MOST_LOOP_SITES = 4000


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    contig = int(args[0]) if len(args) > 0 else 20
    rounds = int(args[1]) if len(args) > 1 else 5
    import torch
    import bench
    import calitas_amd as C
    lib = C._lib.lib
    names, seqs = bench.build_genome(1.0, torch.device("cuda", 0), contig_indices=[contig], guides=[bench.GUIDE0], log=None)
    ctx = C.Context(0)
    ctx.set_reference(names, seqs, genome_build="synthetic")
    del seqs
    length = ctx.contig_lengths[0]
    print("contig %s, %d bases" % (names[0], length), flush=True)
    pat = C.Guide("N" * 20 + "nrg")
    mid = length // 2
    regions = (("10 kb", mid, mid + 10000), ("1 Mb", mid, mid + 1000000), ("contig", 0, length))

    def timed(fn, n):
        out = []
        for r in range(n + 1):                                  # (one call of warm-up: buffers sized, clocks up)
            lib.calitas_reap_wait()
            t0 = time.perf_counter()
            got = fn()
            lib.calitas_reap_wait()
            if r >= 1 or n == 0:
                out.append((time.perf_counter() - t0) * 1e3)
        out.sort()
        return got, out

    def show(region, shape, arm, t, note=""):
        print("%-7s %-15s %-7s median %10.2f ms  min %10.2f  max %10.2f  %s" % (region, shape, arm, t[len(t) // 2], t[0], t[-1], note), flush=True)

    for region, start, end in regions:
        where = dict(chrom=0, start=start, end=end)
        sites, t_find = timed(lambda: ctx.find_sites(pat, **where), rounds)
        n_sites = len(sites)
        show(region, "", "find", t_find, "%d sites" % n_sites)
        t_host_sites = None
        if n_sites <= MOST_HOST_SITES:
            _, t_host_sites = timed(lambda: len(ctx.find_sites(pat, host=True, **where)), 0)
        for shape, lo, hi, codes in SHAPES:
            spec = C.SitePairs(lo, hi, orientations=codes)
            (_, n_pairs, by), t = timed(lambda: ctx.count_site_pairs(pat, spec, **where), rounds)
            show(region, shape, "count", t, "%d pairs" % n_pairs)
            got = None
            if n_pairs <= MOST_PAIRS:
                got, t = timed(lambda: ctx.find_site_pairs(pat, spec, **where), rounds)
                assert len(got[1]) == n_pairs and got[0].tobytes() == sites.tobytes()
                show(region, shape, "pairs", t)
            else:
                print("%-7s %-15s pairs   left out: %d pairs" % (region, shape, n_pairs), flush=True)
            if t_host_sites is not None and n_pairs <= MOST_PAIRS:
                twin, t = timed(lambda: ctx.find_site_pairs(pat, spec, host=True, **where), 0)
                assert got is not None and twin[1].tobytes() == got[1].tobytes(), "the device's pairs and the host twin's differ"
                walk = max(0.0, t[0] - t_host_sites[0])
                print("%-7s %-15s + walk  %10.2f ms  (host twin %.2f ms less its site scan %.2f ms); find + walk %.2f ms" %
                      (region, shape, walk, t[0], t_host_sites[0], t_find[len(t_find) // 2] + walk), flush=True)
            else:
                print("%-7s %-15s + walk  left out" % (region, shape), flush=True)
            if n_sites <= MOST_LOOP_SITES:
                t0 = time.perf_counter()
                loop = C.site_pairs_of(sites, spec, pat)
                t_loop = (time.perf_counter() - t0) * 1e3
                assert got is not None and [tuple(int(x) for x in (p["left"], p["right"], p["distance"], p["orientation"])) for p in got[1]] == loop
                print("%-7s %-15s + loop  %10.2f ms; find + loop %.2f ms" % (region, shape, t_loop, t_find[len(t_find) // 2] + t_loop), flush=True)
            else:
                print("%-7s %-15s + loop  left out: quadratic in %d sites" % (region, shape, n_sites), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
