"""calitas_find_sites_regions timed on the bench genome recipe (bench.build_genome; scale 1 = hg38-sized), alone on the chip, interleaved
round by round in ONE process: python tools/site_regions_speed.py [scale] [rounds]

The region set is exon-like: about 2 x 10^5 x scale intervals of 50 .. 300 bases, one class, spread over the contigs in proportion to
their lengths without overlap, covering about 1.1 % of the genome (175 bases on average).  For N20 + nrg over the whole genome, the class of the whole
protospacer:

  skip    : calitas_find_sites_regions keeping the exon class (the default: segments no exon comes near are skipped)
  noskip  : the same call with CALITAS_SITES_SKIP=0 (every segment matched, every record classed on the device)
  find    : calitas_find_sites over the genome -- what a user does today, first half: every record comes to the host
  + host  : ... second half: the records classed on the host (numpy: one binary search per record in the contig's sorted intervals),
            timed once on the records of one call, not interleaved -- it runs on the CPU alone

A call is timed by the host clock around the library call, blocks freed inside it and the library's deferred frees waited for
(calitas_reap_wait: a block of gigabytes is handed back on a thread of the library's, which would otherwise run into the next arm's
time).  Every arm is first called once (it sizes the buffers), then median / min over the rounds; the arms' order rotates from round
to round.  Before timing, skip and noskip are held against each other byte for byte and against the
host classing of find's records.  The fraction of segments the skip leaves out comes from the presence table (calitas_site_presence).
No ratio is a pass criterion."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def exon_like(names, lengths, scale, rng):
    """[(chromosome, start, end, "exon")], sorted per contig, without overlap."""
    total = float(sum(lengths))
    out = []
    for name, n in zip(names, lengths):
        k = int(2e5 * scale * n / total)
        if k == 0 or n < 1000 * k:
            continue
        starts = (rng.permutation(n // 1000 - 1)[:k].astype("int64") + 1) * 1000 - rng.integers(0, 300, size=k)   # one per kilobase slot
        starts.sort()
        for s, w in zip(starts.tolist(), rng.integers(50, 301, size=k).tolist()):
            out.append((name, s, min(s + w, n), "exon"))
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    scale = float(args[0]) if len(args) > 0 else 1.0
    rounds = int(args[1]) if len(args) > 1 else 5
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
    iv = exon_like(ctx.contig_names, ctx.contig_lengths, scale, np.random.default_rng(420))
    covered = sum(e - s for _, s, e, _ in iv)
    ctx.set_regions(C.Regions(iv))
    print("genome %d bases, %d intervals covering %.2f %%" % (bases, len(iv), 100.0 * covered / bases), flush=True)
    table, _ = ctx.site_presence()
    live = int((table != 0).sum())
    print("segments: %d of contigs, %d (%.1f %%) without an exon near them: skipped" % (live, int(((table != 0) & (table & 2 == 0)).sum()),
                                                                                      100.0 * ((table != 0) & (table & 2 == 0)).sum() / max(1, live)), flush=True)
    g = C.Guide("N" * 20 + "nrg").to_c()
    opt = C._lib.SiteRegionsT(2, 0, 0, 0)
    index = {n: i for i, n in enumerate(ctx.contig_names)}
    by_contig = {}
    for name, s, e, _ in iv:
        by_contig.setdefault(index[name], ([], []))
        by_contig[index[name]][0].append(s)
        by_contig[index[name]][1].append(e)
    by_contig = {c: (np.array(s, dtype=np.int64), np.array(e, dtype=np.int64)) for c, (s, e) in by_contig.items()}

    def regions(keep_records=False):
        out, cls, n = ctypes.POINTER(C._lib.SiteT)(), ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
        C._lib.check(ctx._h, lib.calitas_find_sites_regions(ctx._h, ctypes.byref(g), None, ctypes.byref(opt), -1, 0, 0, ctypes.byref(out), ctypes.byref(cls),
                                                             ctypes.byref(n)))
        data = ctypes.string_at(out, n.value * 16) if keep_records else None
        lib.calitas_free(out)
        lib.calitas_free(cls)
        return n.value, data

    def skip():
        os.environ.pop("CALITAS_SITES_SKIP", None)
        return regions()[0]

    def noskip():
        os.environ["CALITAS_SITES_SKIP"] = "0"
        try:
            return regions()[0]
        finally:
            del os.environ["CALITAS_SITES_SKIP"]

    def find(classing=False):
        out, n = ctypes.POINTER(C._lib.SiteT)(), ctypes.c_uint64()
        C._lib.check(ctx._h, lib.calitas_find_sites(ctx._h, ctypes.byref(g), -1, 0, 0, ctypes.byref(out), ctypes.byref(n)))
        kept = None
        if classing:                                            # the records where they are: no copy but what numpy's own steps make
            t0 = time.perf_counter()
            block = (ctypes.c_char * (n.value * 16)).from_address(ctypes.addressof(out.contents))
            recs = np.frombuffer(block, dtype=C.aligner.SITE_DTYPE)
            contig, p = recs["contig_index"], recs["protospacer_start"]
            edges = np.searchsorted(contig, np.arange(len(names) + 1))
            keep = np.zeros(len(recs), dtype=bool)
            for c, (s, e) in by_contig.items():
                q = p[edges[c]:edges[c + 1]].astype(np.int64)
                at = np.searchsorted(s, q + 20, side="left") - 1        # the last interval that starts below the protospacer's end
                keep[edges[c]:edges[c + 1]] = (at >= 0) & (e[np.maximum(at, 0)] > q)
            kept = recs[keep].tobytes()
            print("host classing of %d records: %.3f s, %d kept" % (len(recs), time.perf_counter() - t0, int(keep.sum())), flush=True)
            del recs, block
        lib.calitas_free(out)
        return n.value, kept

    n_skip, fast = regions(keep_records=True)
    os.environ["CALITAS_SITES_SKIP"] = "0"
    n_slow, slow = regions(keep_records=True)
    del os.environ["CALITAS_SITES_SKIP"]
    assert fast == slow, "the listing with the skip and without it differ"
    n_all, by_host = find(classing=True)
    assert by_host == fast, "the device's listing and the host classing of calitas_find_sites' records differ"
    print("checked: skip == noskip == host classing, %d of %d records" % (n_skip, n_all), flush=True)
    del fast, slow, by_host

    calls = {"skip": skip, "noskip": noskip, "find": lambda: find()[0]}
    res = {k: [] for k in calls}
    order = list(calls)
    for r in range(rounds + 1):                                 # (one round of warm-up: buffers sized, clocks up)
        for k in order[r % 3:] + order[:r % 3]:
            fn = calls[k]
            lib.calitas_reap_wait()
            t0 = time.perf_counter()
            fn()
            lib.calitas_reap_wait()
            if r >= 1:
                res[k].append((time.perf_counter() - t0) * 1e3)
        print("round %d done" % r, flush=True)
    for k in calls:
        t = sorted(res[k])
        print("%-7s scale %g: median %.1f ms  min %.1f  max %.1f" % (k, scale, t[len(t) // 2], t[0], t[-1]), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
