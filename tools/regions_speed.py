"""What a regions call costs over a top call of the same build, interleaved round by round in ONE process on one box (the twin of
tools/top_speed.py): python tools/regions_speed.py [scale] [rounds] [n_guides] [--existing] [--tree DIR]

  single: calitas_search_regions (k = 10, every class listed) against calitas_search_top (k = 10), guide #0 of BASELINE config 3
  batch : calitas_search_regions_batch against calitas_search_top_batch, guide #0 + random 20-mers

once with a set of about 3e5 x scale random exon-sized intervals (7 classes) and once with a set of 10 intervals, on the bench genome
recipe (bench.build_genome; scale 1 = hg38-sized), same guides and parameters as tools/top_speed.py.  Per call it prints the median /
min / quartiles in ms, the difference of the medians and the top call's own spread to hold it against; before timing anything it holds
search_regions_batch against regions_of_rows of the text for three guides, and against single calls.

--existing times the calls that existed before (search_counts, search_scores, search_top at k = 10 and their batches) alone, and
--tree DIR takes package and library from another checkout (built): with both, those calls of a parent commit's build are measured
against this one's by alternating whole processes in one session; the yardstick is the spread between the parent's own runs there."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from scores_speed import distinct_model, quart  # noqa: E402


def random_regions(C, names, lengths, n, seed):
    """n intervals of exon-like lengths (50 .. 1500 bases) spread over the contigs in proportion to their lengths, 7 classes."""
    import numpy as np
    rng = np.random.default_rng(seed)
    total = float(sum(lengths))
    iv = []
    for nm, ln in zip(names, lengths):
        m = max(1, int(round(n * ln / total)))
        starts = rng.integers(0, max(1, ln - 1500), size=m)
        widths = rng.integers(50, 1500, size=m)
        classes = rng.integers(1, 8, size=m)
        iv += [(nm, int(a), int(min(ln, a + w)), "c%d" % k) for a, w, k in zip(starts, widths, classes)]
    return C.Regions(iv[:max(n, 1)], classes=["c%d" % i for i in range(1, 8)])


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    existing = "--existing" in sys.argv
    tree = ROOT
    if "--tree" in sys.argv:
        tree = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
        args.remove(sys.argv[sys.argv.index("--tree") + 1])
    sys.path.insert(0, tree)
    scale = float(args[0]) if len(args) > 0 else 1.0
    rounds = int(args[1]) if len(args) > 1 else 20
    n_guides = int(args[2]) if len(args) > 2 else 24
    import torch
    import bench
    import calitas_amd as C
    from calitas_amd import synth
    params = C.make_params(max_guide_diffs=5, max_pam_mismatches=1, max_gaps_between_guide_and_pam=2)
    guides = ([bench.GUIDE0] + synth.random_guides(0xC4, 95))[:n_guides]
    G = [C.Guide(g) for g in guides]
    names, seqs = bench.build_genome(scale, torch.device("cuda", 0), contig_indices=None, guides=guides, log=None)
    ctx = C.Context(0)
    ctx.set_reference(names, seqs, genome_build="synthetic")
    del seqs
    model = distinct_model(C, G[0].protospacer_length)

    calls = {"single top 10": lambda: ctx.search_top(G[0], params, model, 10), "batch top 10": lambda: ctx.search_top_batch(G, params, model, 10)}
    sets = []
    if existing:
        calls["single counts"] = lambda: ctx.search_counts(G[0], params)
        calls["batch counts"] = lambda: ctx.search_counts_batch(G, params)
        calls["single scores"] = lambda: ctx.search_scores(G[0], params, model)
        calls["batch scores"] = lambda: ctx.search_scores_batch(G, params, model)
    else:
        sets = [("many", random_regions(C, ctx.contig_names, ctx.contig_lengths, int(3e5 * scale), 1)),
                ("ten", random_regions(C, ctx.contig_names, ctx.contig_lengths, 10, 2))]
        for tag, reg in sets:
            t0 = time.perf_counter()
            ctx.set_regions(reg)
            print("set_regions %s: %d intervals in %.1f ms" % (tag, len(reg.intervals), (time.perf_counter() - t0) * 1e3), flush=True)
            got = ctx.search_regions_batch(G, params, model, 10)
            for i in sorted({0, len(G) // 2, len(G) - 1}):
                text, n = ctx.search_hits(G[i], "g%d" % i, params, "v0", "stamp")
                want = C.regions_of_rows(C.read_hits(text), model, reg, 10, None, got[i].top.scores.table.shape)
                assert got[i] == want, "guide %d, %s: %r differs from the contract on its text %r" % (i, tag, got[i], want)
                assert ctx.search_regions(G[i], params, model, 10) == want, "guide %d, %s: batch and single differ" % (i, tag)
            print("checked %s: %d guides, %d rows in all; guide #0: %r" % (tag, len(G), sum(t.top.scores.rows for t in got), got[0]), flush=True)
    res, tms = {}, {}
    plans = sets or [("", None)]
    for tag, reg in plans:
        if reg is not None:
            ctx.set_regions(reg)
            calls["single regions"] = lambda: ctx.search_regions(G[0], params, model, 10)
            calls["batch regions"] = lambda: ctx.search_regions_batch(G, params, model, 10)
        for r in range(rounds + 2):                             # (two rounds of warm-up: buffers sized, clocks up)
            for k, fn in calls.items():
                reps = 1 if k.startswith("batch") else 5
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                dt = (time.perf_counter() - t0) * 1e3 / reps
                if r >= 2:
                    res.setdefault((tag, k), []).append(dt)
                tms[(tag, k)] = ctx.timing()
        for k in calls:
            med, lo, q1, q3 = quart(res[(tag, k)])
            tm = tms[(tag, k)]
            print("%-5s %-14s scale %g: median %.3f ms  min %.3f  p25 %.3f  p75 %.3f | rows %d bytes %d binned_lanes %d lanes %d" % (
                tag, k, scale, med, lo, q1, q3, tm["hit_rows"], tm["hits_bytes"], tm["binned_lanes"], tm["lanes"]), flush=True)
        if reg is not None:
            for what in ("single", "batch"):
                a, b = quart(res[(tag, what + " top 10")]), quart(res[(tag, what + " regions")])
                print("%s %s: regions - top = %+.3f ms (medians %.3f / %.3f ms, %+.2f %%; regions p25-p75 %.3f-%.3f); the top call's own spread p25-p75: %.3f-%.3f ms" % (
                    tag, what, b[0] - a[0], b[0], a[0], 100.0 * (b[0] - a[0]) / a[0], b[2], b[3], a[2], a[3]), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
