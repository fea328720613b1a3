"""The counts calls against the text calls of the same build, interleaved round by round in ONE process on one box (as tools/ab_env.py
does for a switch): python tools/counts_speed.py [scale] [rounds] [n_guides]

  batch : calitas_search_counts_batch against calitas_search_hits_batch, the 96 guides of BASELINE config 4 (guide #0 + 95 random 20-mers)
  single: calitas_search_counts against calitas_search_hits, guide #0 of BASELINE config 3

on the bench genome recipe (bench.build_genome; scale 1 = hg38-sized).  Per call it prints the median / min / quartiles in ms and the
ratio text / counts of the medians; before timing anything it checks that every guide's table is the table of its text's rows."""
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
    n_guides = int(sys.argv[3]) if len(sys.argv) > 3 else 96
    import numpy as np
    import torch
    import bench
    import calitas_amd as C
    from calitas_amd import synth
    params = C.make_params(max_guide_diffs=5, max_pam_mismatches=1, max_gaps_between_guide_and_pam=2)
    guides = ([bench.GUIDE0] + synth.random_guides(0xC4, 95))[:n_guides]
    G = [C.Guide(g) for g in guides]
    ids = ["g%d" % i for i in range(len(G))]
    names, seqs = bench.build_genome(scale, torch.device("cuda", 0), contig_indices=None, guides=guides, log=None)
    ctx = C.Context(0)
    ctx.set_reference(names, seqs, genome_build="synthetic")
    del seqs

    # the tables are the tables of the texts (guide #0 and three others in full; every guide by its row count)
    tables = ctx.search_counts_batch(G, params)
    rows = [n for _, n in ctx.search_hits_batch(G, ids, params, "v0", "stamp", decode=False)]
    assert [int(t.sum()) for t in tables] == rows, "row counts of the counts batch and the text batch differ"
    for i in sorted({0, len(G) // 3, len(G) // 2, len(G) - 1}):
        text, n = ctx.search_hits(G[i], ids[i], params, "v0", "stamp")
        assert np.array_equal(tables[i], C.counts_of_rows(C.read_hits(text), tables[i].shape)), "guide %d: table differs from its text" % i
        assert np.array_equal(tables[i], ctx.search_counts(G[i], params)), "guide %d: batch and single tables differ" % i
    print("checked: %d guides, %d rows in all, shape %s" % (len(G), sum(rows), tables[0].shape), flush=True)

    calls = {
        "batch text": lambda: ctx.search_hits_batch(G, ids, params, "v0", "stamp", decode=False),
        "batch counts": lambda: ctx.search_counts_batch(G, params),
        "single text": lambda: ctx.search_hits(G[0], ids[0], params, "v0", "stamp", decode=False),
        "single counts": lambda: ctx.search_counts(G[0], params),
    }
    res = {k: [] for k in calls}
    tms = {}
    for r in range(rounds + 2):                                 # (two rounds of warm-up: buffers sized, clocks up)
        for k, fn in calls.items():
            reps = 1 if k.startswith("batch") else 5
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            dt = (time.perf_counter() - t0) * 1e3 / reps
            if r >= 2:
                res[k].append(dt)
            tms[k] = ctx.timing()
    for k in calls:
        med, lo, q1, q3 = quart(res[k])
        tm = tms[k]
        print("%-13s scale %g: median %.3f ms  min %.3f  p25 %.3f  p75 %.3f | rows %d bytes %d binned_lanes %d lanes %d" % (
            k, scale, med, lo, q1, q3, tm["hit_rows"], tm["hits_bytes"], tm["binned_lanes"], tm["lanes"]), flush=True)
    for what in ("batch", "single"):
        a, b = quart(res[what + " text"]), quart(res[what + " counts"])
        print("%s: text / counts = %.3f (medians %.3f / %.3f ms); the text call's own spread p25-p75: %.3f-%.3f ms" % (
            what, a[0] / b[0], a[0], b[0], a[2], a[3]), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
