"""What a top call costs over a scores call of the same build, interleaved round by round in ONE process on one box (the twin of
tools/scores_speed.py): python tools/top_speed.py [scale] [rounds] [n_guides] [--existing] [--tree DIR]

  single: calitas_search_top at k = 10 and k = 256 against calitas_search_scores, guide #0 of BASELINE config 3
  batch : calitas_search_top_batch at k = 10 and k = 256 against calitas_search_scores_batch, guide #0 + random 20-mers

on the bench genome recipe (bench.build_genome; scale 1 = hg38-sized), same guides and parameters as tools/scores_speed.py.  Per call it
prints the median / min / quartiles in ms, the difference of the medians and the scores call's own spread to hold it against; before
timing anything it holds search_top_batch against top_of_rows of the text for three guides, and against single calls.

--existing times the calls that existed before (search_counts, search_scores and their batches) alone, and --tree DIR takes package and
library from another checkout (built): with both, those calls of a parent commit's build are measured against this one's by alternating
whole processes in one session; the yardstick is the spread between the parent's own runs there."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from scores_speed import distinct_model, quart  # noqa: E402


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

    calls = {"single scores": lambda: ctx.search_scores(G[0], params, model), "batch scores": lambda: ctx.search_scores_batch(G, params, model)}
    if existing:
        calls["single counts"] = lambda: ctx.search_counts(G[0], params)
        calls["batch counts"] = lambda: ctx.search_counts_batch(G, params)
    else:
        for k in (10, 256):
            got = ctx.search_top_batch(G, params, model, k)
            for i in sorted({0, len(G) // 2, len(G) - 1}):
                text, n = ctx.search_hits(G[i], "g%d" % i, params, "v0", "stamp")
                want = C.top_of_rows(C.read_hits(text), model, k, got[i].scores.table.shape)
                assert got[i] == want, "guide %d, k %d: %r differs from the top of its text %r" % (i, k, got[i], want)
                assert ctx.search_top(G[i], params, model, k) == want, "guide %d, k %d: batch and single differ" % (i, k)
            print("checked k %d: %d guides, %d rows in all; guide #0: %r, best %r" % (k, len(G), sum(t.scores.rows for t in got), got[0], got[0].hits[:1]),
                  flush=True)
            calls["single top %d" % k] = lambda k=k: ctx.search_top(G[0], params, model, k)
            calls["batch top %d" % k] = lambda k=k: ctx.search_top_batch(G, params, model, k)
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
        print("%-14s scale %g: median %.3f ms  min %.3f  p25 %.3f  p75 %.3f | rows %d bytes %d binned_lanes %d lanes %d" % (
            k, scale, med, lo, q1, q3, tm["hit_rows"], tm["hits_bytes"], tm["binned_lanes"], tm["lanes"]), flush=True)
    if not existing:
        for what in ("single", "batch"):
            a = quart(res[what + " scores"])
            for k in (10, 256):
                b = quart(res["%s top %d" % (what, k)])
                print("%s: top %d - scores = %+.3f ms (medians %.3f / %.3f ms, %+.2f %%; top p25-p75 %.3f-%.3f); the scores call's own spread p25-p75: %.3f-%.3f ms" % (
                    what, k, b[0] - a[0], b[0], a[0], 100.0 * (b[0] - a[0]) / a[0], b[2], b[3], a[2], a[3]), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
