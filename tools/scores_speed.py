"""What a scores call costs over a counts call of the same build, interleaved round by round in ONE process on one box (the twin of
tools/counts_speed.py): python tools/scores_speed.py [scale] [rounds] [n_guides] [--counts-only] [--tree DIR]

  single: calitas_search_scores against calitas_search_counts, guide #0 of BASELINE config 3
  batch : calitas_search_scores_batch against calitas_search_counts_batch, guide #0 + random 20-mers (BASELINE config 4's recipe)

on the bench genome recipe (bench.build_genome; scale 1 = hg38-sized).  Per call it prints the median / min / quartiles in ms, the
difference of the medians and the counts call's own spread to hold it against; before timing anything it checks that the scores are the
scores of the text's rows (scores_of_rows) and that a scores call's table is the counts call's.  The model has all L * 25 + 2 factors
distinct (seeded), so the check sees positions, letters and orientation.

--counts-only times the counts calls alone, and --tree DIR takes package and library from another checkout (built): with both, the
counts call of a parent commit's build is measured against this one's by alternating whole processes in one session
(tools/ab_lib.sh style); the yardstick is the spread between the parent's own runs there."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def quart(t):
    t = sorted(t)
    n = len(t)
    return t[n // 2], t[0], t[n // 4], t[3 * n // 4]


def distinct_model(C, L, seed=7):
    import numpy as np
    rng = np.random.default_rng(seed)
    seen, vals = set(), []
    while len(vals) < L * 25 + 2:
        v = int(rng.integers(1, 65536))
        if v not in seen:
            seen.add(v)
            vals.append(v)
    return C.ScoreModel(L, np.array(vals[:L * 25], dtype=np.uint32).reshape(L, 5, 5), vals[-2], vals[-1])


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    counts_only = "--counts-only" in sys.argv
    tree = ROOT
    if "--tree" in sys.argv:
        tree = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
        args.remove(sys.argv[sys.argv.index("--tree") + 1])
    sys.path.insert(0, tree)
    scale = float(args[0]) if len(args) > 0 else 1.0
    rounds = int(args[1]) if len(args) > 1 else 20
    n_guides = int(args[2]) if len(args) > 2 else 96
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

    calls = {"single counts": lambda: ctx.search_counts(G[0], params), "batch counts": lambda: ctx.search_counts_batch(G, params)}
    if not counts_only:
        import numpy as np
        model = distinct_model(C, G[0].protospacer_length)
        got = ctx.search_scores_batch(G, params, model)
        tables = ctx.search_counts_batch(G, params)
        assert all(np.array_equal(s.table, t) for s, t in zip(got, tables)), "a scores call's table differs from the counts call's"
        for i in sorted({0, len(G) // 2, len(G) - 1}):
            text, n = ctx.search_hits(G[i], "g%d" % i, params, "v0", "stamp")
            want = C.scores_of_rows(C.read_hits(text), model, got[i].table.shape)
            assert got[i] == want, "guide %d: %r differs from the score of its text %r" % (i, got[i], want)
            assert ctx.search_scores(G[i], params, model) == want, "guide %d: batch and single scores differ" % i
        print("checked: %d guides, %d rows in all; guide #0: %r specificity %.6f" % (len(G), sum(s.rows for s in got), got[0], got[0].specificity),
              flush=True)
        calls["single scores"] = lambda: ctx.search_scores(G[0], params, model)
        calls["batch scores"] = lambda: ctx.search_scores_batch(G, params, model)
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
    if not counts_only:
        for what in ("single", "batch"):
            a, b = quart(res[what + " counts"]), quart(res[what + " scores"])
            print("%s: scores - counts = %+.3f ms (medians %.3f / %.3f ms, %+.2f %%); the counts call's own spread p25-p75: %.3f-%.3f ms" % (
                what, b[0] - a[0], b[0], a[0], 100.0 * (b[0] - a[0]) / a[0], a[2], a[3]), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
