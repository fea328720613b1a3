"""calitas_count_copies timed on the bench genome recipe (bench.build_genome; scale 1 = hg38-sized), alone on the chip, interleaved
round by round in ONE process: python tools/copies_speed.py [scale] [rounds]

  count plain     : calitas_count_sites of NNNNNNNNNNNNNNNNNNNNnrg over the whole genome, no filter -- the floor: the same match work
  copies 10 kb    : calitas_count_copies over the whole genome, the queries the protospacers of every site of a 10-kb region (K = 20)
  copies 1 Mb     : ... of a 1-Mb region
  copies 10 Mb    : ... of a 10-Mb region
  ... K=12        : the same three with the PAM-proximal 12 bases as the key
  copies K=4, K=1 : the 10-kb region's guides cut to 4 bases and to 1: at most 256 counters, and 4, take every site of the genome
                    (hot counters)

A call is timed by the host clock around the library call (the queries are handed over as one prepared buffer, as a C caller has them;
the call removes duplicate keys, builds and uploads the table, runs the kernel and copies the counters back, and ends in a stream
synchronise).  Per row: median / min / quartiles in ms, the queries, and how many of them have more than one copy.  Before timing, the
10-kb set counted over its own region is checked against the host twin, and every guide of a region is required to count itself.
The bench genome is independent random bases with short tandem repeats planted (bench.gen_contig): the interspersed repeats and
duplications of a real genome do not occur in it, so nearly every 20-mer has one copy and the contention of a real genome's hot
20-mers is NOT measured here beyond the few keys the tandem repeats make; K = 4 and K = 1 show what hot counters cost."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L = 20


def quart(t):
    t = sorted(t)
    n = len(t)
    return t[n // 2], t[0], t[n // 4], t[3 * n // 4]


def region_keys(np, ctx, sites, chrom, K):
    """The PAM-proximal K bases of every site's protospacer as the guide reads (3' PAM: the last K), one row of K bytes per site."""
    lo = int(sites["protospacer_start"].min())
    hi = int(sites["protospacer_start"].max()) + L
    text = np.frombuffer(ctx.fetch_bases(chrom, lo, hi - lo).upper().replace("U", "T").encode(), dtype=np.uint8)
    windows = np.lib.stride_tricks.sliding_window_view(text, L)[sites["protospacer_start"] - lo]
    comp = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    minus = sites["strand"] == b"-"
    protos = np.where(minus[:, None], comp[windows[:, ::-1]], windows)
    return np.ascontiguousarray(protos[:, L - K:])


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
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
    n20 = C.Guide("N" * L + "nrg")
    g = n20.to_c()
    big = max(range(len(names)), key=lambda i: ctx.contig_lengths[i])
    total, _ = ctx.count_sites(n20)
    print("%d N20+nrg sites in %d bases" % (total, bases), flush=True)

    def counted(keys, K, chrom=-1, start=0, end=0, host=False):
        out = np.zeros(max(1, len(keys)), dtype=np.uint64)
        fn = lib.calitas_count_copies_host if host else lib.calitas_count_copies
        C._lib.check(ctx._h, fn(ctx._h, ctypes.byref(g), K, chrom, start, end, keys.ctypes.data_as(ctypes.c_char_p), len(keys),
                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out[:len(keys)]

    calls = {"count plain": (lambda: ctx.count_sites(n20), 5)}
    info = {"count plain": "%d sites" % total}
    for label, size in (("10 kb", 10_000), ("1 Mb", 1_000_000), ("10 Mb", 10_000_000)):
        r1 = min(ctx.contig_lengths[big], 1_000_000 + size)
        r0 = max(0, r1 - size)
        sites = ctx.find_sites(n20, chrom=big, start=r0, end=r1)
        for K in (20, 12) + ((4, 1) if size == 10_000 else ()):
            keys = region_keys(np, ctx, sites, big, K)
            got = counted(keys, K)
            assert int(got.min()) >= 1, "a guide cut from the reference does not count itself"
            if size == 10_000:
                assert got.tobytes() != b"" and counted(keys, K, big, r0, r1).tobytes() == counted(keys, K, big, r0, r1, host=True).tobytes(), \
                    "the kernel and the host twin differ"
            name = "copies %s" % label if K == 20 else "copies %s K=%d" % (label, K)
            calls[name] = (lambda keys=keys, K=K: counted(keys, K), 5 if size < 10_000_000 else 1)
            info[name] = "%d queries, %d distinct, %d with more than one copy, largest count %d" % (
                len(keys), len(np.unique(keys, axis=0)), int((got > 1).sum()), int(got.max()))
    print("checked: the 10-kb sets over their own region against the host twin; every guide counts itself", flush=True)

    res = {k: [] for k in calls}
    for r in range(rounds + 2):                                 # (two rounds of warm-up: buffers sized, clocks up)
        for k, (fn, reps) in calls.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            dt = (time.perf_counter() - t0) * 1e3 / reps
            if r >= 2:
                res[k].append(dt)
    for k in calls:
        med, lo, q1, q3 = quart(res[k])
        print("%-18s scale %g: median %.3f ms  min %.3f  p25 %.3f  p75 %.3f | %s" % (k, scale, med, lo, q1, q3, info[k]), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
