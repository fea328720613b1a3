"""calitas_count_near timed on the bench genome recipe (bench.build_genome; scale 1 = hg38-sized), alone on the chip, interleaved round by
round in ONE process: python tools/near_speed.py [scale] [rounds] [--existing | --list] [--tree DIR] [--search-ms MS]

  count plain       : calitas_count_sites of NNNNNNNNNNNNNNNNNNNNnrg over the whole genome, no filter -- the same match work
  copies 10 kb      : calitas_count_copies over the whole genome, the queries the protospacers of every site of a 10-kb region (K = 20)
  near 10 kb M=1..3 : calitas_count_near of the same queries at max_mismatches 1, 2, 3
  scored 10 kb M=.. : calitas_score_near of the same queries and M under a model (every factor 0.6), beside each K = 20 near row
  listed 10 kb M=.. : calitas_list_near of the same queries, M and model with limit 1000, beside each scored row: the records returned
                      and the queries over the limit stand in the row
  ... K=12 M=2      : the PAM-proximal 12 bases as the key, copies and near at M = 2
  ... 1 Mb          : the same rows for the guides of a 1-Mb region

A call is timed by the host clock around the library call (the queries are handed over as one prepared buffer, as a C caller has them;
the call removes duplicate keys, builds and uploads the bucket tables, runs the kernel and copies the counters back, and ends in a
stream synchronise).  Every row is first called once, untimed as a measurement but shown (`first call`): it sizes the buffers, and a
row whose call takes longer than 8 s is not repeated -- that one figure is all it gets.  The others: median / min / quartiles in ms over the
rounds (three rounds for calls of more than 2 s), one call per round for calls of more than 0.5 s, five otherwise.  Per row the queries, how many of them have a copy within M
substitutions other than themselves, and what search_counts_batch costs for as many guides at --search-ms per guide (default 2.4, what
tools/counts_speed.py measures at this size).  Before timing, column 0 of every near call is held against the copies count, and the 10-kb
sets counted over their own region against the host twin.
The bench genome is independent random bases with short tandem repeats planted (bench.gen_contig): it has almost no near-duplicate
20-mers, so what a real genome's repeat families cost -- long buckets and hot counters -- is NOT measured here.

--list: the K = 20 rows alone (near, scored, listed), for a look at the listing by itself or under a profiler.
--existing: the calls that existed before calitas_list_near alone -- `count plain`, `copies 10 kb`, `near 10 kb M=2` and `scored 10 kb
M=2` -- which the parent commit's checkout has too; --tree DIR takes package and library from another checkout (built).  With both, two builds are compared, whole
processes alternated:  python tools/near_speed.py 1.0 20 --existing --tree PARENT  against  ... --existing."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L = 20
ONCE_OVER_S = 8.0
FEW_OVER_S = 2.0          # a call slower than this is timed in three rounds only


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
    argv = sys.argv[1:]
    existing = "--existing" in argv
    only_list = "--list" in argv
    search_ms = 2.4
    skip = set()
    for flag in ("--tree", "--search-ms"):
        if flag in argv:
            skip.add(argv.index(flag) + 1)
    if "--tree" in argv:
        sys.path.insert(0, os.path.abspath(argv[argv.index("--tree") + 1]))      # (in front of this checkout)
    if "--search-ms" in argv:
        search_ms = float(argv[argv.index("--search-ms") + 1])
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and i not in skip]
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

    def copies(keys, K, chrom=-1, start=0, end=0):
        out = np.zeros(max(1, len(keys)), dtype=np.uint64)
        C._lib.check(ctx._h, lib.calitas_count_copies(ctx._h, ctypes.byref(g), K, chrom, start, end, keys.ctypes.data_as(ctypes.c_char_p), len(keys),
                                                      out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out[:len(keys)]

    def near(keys, K, M, chrom=-1, start=0, end=0, host=False):
        out = np.zeros((max(1, len(keys)), M + 1), dtype=np.uint64)
        fn = lib.calitas_count_near_host if host else lib.calitas_count_near
        C._lib.check(ctx._h, fn(ctx._h, ctypes.byref(g), K, M, chrom, start, end, keys.ctypes.data_as(ctypes.c_char_p), len(keys),
                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out[:len(keys)]

    model = C.ScoreModel.uniform(L, mismatch=39322).to_c()

    def scored(keys, M, chrom=-1, start=0, end=0, host=False):
        out = np.zeros((max(1, len(keys)), M + 1), dtype=np.uint64)
        words = np.zeros((max(1, len(keys)), 2), dtype=np.uint64)
        fn = lib.calitas_score_near_host if host else lib.calitas_score_near
        C._lib.check(ctx._h, fn(ctx._h, ctypes.byref(g), M, ctypes.byref(model), chrom, start, end, keys.ctypes.data_as(ctypes.c_char_p), len(keys),
                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out[:len(keys)], words[:len(keys)]

    def listed(keys, M, chrom=-1, start=0, end=0, host=False, limit=1000):
        """(near, offsets, the records' bytes when asked for the host comparison else None, the number of records)"""
        out = np.zeros((max(1, len(keys)), M + 1), dtype=np.uint64)
        offsets = np.zeros(len(keys) + 1, dtype=np.uint64)
        hits, n = ctypes.POINTER(C._lib.NearHitT)(), ctypes.c_uint64()
        fn = lib.calitas_list_near_host if host else lib.calitas_list_near
        C._lib.check(ctx._h, fn(ctx._h, ctypes.byref(g), M, ctypes.byref(model), chrom, start, end, keys.ctypes.data_as(ctypes.c_char_p), len(keys), limit,
                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(hits),
                                ctypes.byref(n)))
        data = ctypes.string_at(hits, n.value * 32) if chrom >= 0 else None
        lib.calitas_free(hits)
        return out[:len(keys)], offsets, data, n.value

    calls = {"count plain": lambda: ctx.count_sites(n20)}
    info = {"count plain": "%d sites" % total}
    first = {}
    for label, size in (("10 kb", 10_000), ("1 Mb", 1_000_000)):
        if existing and size != 10_000:
            continue
        r1 = min(ctx.contig_lengths[big], 1_000_000 + size)
        r0 = max(0, r1 - size)
        sites = ctx.find_sites(n20, chrom=big, start=r0, end=r1)
        for K, Ms in ((20, (1, 2, 3)), (12, (2,))):
            if (existing or only_list) and K != 20:
                continue
            keys = region_keys(np, ctx, sites, big, K)
            tag = label if K == 20 else "%s K=%d" % (label, K)
            t0 = time.perf_counter()
            exact = copies(keys, K)
            first["copies " + tag] = time.perf_counter() - t0
            assert int(exact.min()) >= 1, "a guide cut from the reference does not count itself"
            calls["copies " + tag] = lambda keys=keys, K=K: copies(keys, K)
            info["copies " + tag] = "%d queries, %d with more than one copy | the search: %.1f s" % (len(keys), int((exact > 1).sum()), len(keys) * search_ms / 1e3)
            for M in (2,) if existing else Ms:
                name = "near %s M=%d" % (tag, M)
                t0 = time.perf_counter()
                got = near(keys, K, M)
                first[name] = time.perf_counter() - t0
                print("%-22s first call %.3f s" % (name, first[name]), flush=True)
                assert got[:, 0].tobytes() == exact.tobytes(), "column 0 is not the copies count"
                if size == 10_000 and not existing:
                    assert near(keys, K, M, big, r0, r1).tobytes() == near(keys, K, M, big, r0, r1, host=True).tobytes(), "the kernel and the host twin differ"
                others = got.sum(axis=1) - 1
                info[name] = "%d queries, %d with another copy within %d, most %d | the search: %.1f s" % (
                    len(keys), int((others > 0).sum()), M, int(others.max()), len(keys) * search_ms / 1e3)
                if first[name] <= ONCE_OVER_S:
                    calls[name] = lambda keys=keys, K=K, M=M: near(keys, K, M)
                else:
                    print("%-22s scale %g: one call %.1f ms | %s" % (name, scale, first[name] * 1e3, info[name]), flush=True)
                if K != L:
                    continue
                sname = "scored %s M=%d" % (tag, M)
                t0 = time.perf_counter()
                rows, words = scored(keys, M)
                first[sname] = time.perf_counter() - t0
                print("%-22s first call %.3f s" % (sname, first[sname]), flush=True)
                assert rows.tobytes() == got.tobytes(), "the scored call's counts are not count_near's"
                if size == 10_000 and not existing:
                    a, b = scored(keys, M, big, r0, r1), scored(keys, M, big, r0, r1, host=True)
                    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), "the scored kernel and the host twin differ"
                info[sname] = "%d queries, %d with a scored copy, largest sum %.3f" % (len(keys), int((words[:, 0] > 0).sum()), int(words[:, 0].max()) / 2.0 ** 32)
                if first[sname] <= ONCE_OVER_S:
                    calls[sname] = lambda keys=keys, M=M: scored(keys, M)
                else:
                    print("%-22s scale %g: one call %.1f ms | %s" % (sname, scale, first[sname] * 1e3, info[sname]), flush=True)
                if existing:
                    continue
                lname = "listed %s M=%d" % (tag, M)
                t0 = time.perf_counter()
                rows, offsets, _, n_records = listed(keys, M)
                first[lname] = time.perf_counter() - t0
                print("%-22s first call %.3f s" % (lname, first[lname]), flush=True)
                assert rows.tobytes() == got.tobytes() and int(offsets[-1]) == n_records, "the listing's counts are not count_near's"
                over = rows.sum(axis=1) > 1000
                assert n_records == int(rows.sum(axis=1)[~over].sum()), "the records are not as many as the listed queries' counts"
                if size == 10_000:
                    a, b = listed(keys, M, big, r0, r1), listed(keys, M, big, r0, r1, host=True)
                    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2], "the listing kernels and the host twin differ"
                info[lname] = "%d queries, %d over the limit of 1000, %d records (%.1f MB)" % (len(keys), int(over.sum()), n_records, n_records * 32 / 1e6)
                if first[lname] <= ONCE_OVER_S:
                    calls[lname] = lambda keys=keys, M=M: listed(keys, M)
                else:
                    print("%-22s scale %g: one call %.1f ms | %s" % (lname, scale, first[lname] * 1e3, info[lname]), flush=True)
    if not existing:
        print("checked: column 0 against the copies count; the scored and the listing calls' counts against count_near; the records against the counts; the 10-kb sets over their own region against the host twin", flush=True)

    res = {k: [] for k in calls}
    for r in range(rounds + 2):                                 # (two rounds of warm-up: buffers sized, clocks up)
        for k, fn in calls.items():
            if first.get(k, 0.0) > FEW_OVER_S and r >= 5:
                continue
            reps = 1 if first.get(k, 0.0) > 0.5 else 5
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            dt = (time.perf_counter() - t0) * 1e3 / reps
            if r >= 2:
                res[k].append(dt)
    for k in calls:
        med, lo, q1, q3 = quart(res[k])
        print("%-22s scale %g: median %.3f ms  min %.3f  p25 %.3f  p75 %.3f | %s" % (k, scale, med, lo, q1, q3, info[k]), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
