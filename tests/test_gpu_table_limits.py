"""GPU: the counts and score kernels (counts_kernel / scores_kernel in hits.hip, bin_counts_kernel / bin_scores_kernel in binned.hip, the
shared code in hits_dev.hpp) at the limits the host accepts -- tables around COUNTS_LDS_CELLS = 4096 cells (the last one kept in LDS,
the first ones added to the device table directly), the device table left clean between calls of different sizes, more items than one
stride of the 128 x 256 lanes covers, and score factors of 0 and of 65536.  Every comparison is equality: against the oracle's rows
(counts_of_rows, scores_of_rows) and against the same functions of the text calitas_search_hits returns on the same path.  What a case
is there for is asserted on the oracle's rows first, so that a case which has drifted off its target fails.

| id                | guide                    | params         | shape          | cells                                        |
|-------------------|--------------------------|----------------|----------------|----------------------------------------------|
| cells-4096        | L20 + nrg                | d=31 p=1 g=0   | (2, 32, 32, 2) | 4096: the last size in LDS, hist[] is full   |
| cells-4224        | L20 + nrg                | d=31 p=1 g=1   | (2, 32, 33, 2) | 4224: the first direct size                  |
| cells-9702-dense  | L32 + ngggtcagttcaagcn   | d=32 p=2 g=16  | (2, 33, 49, 3) | 9702: the largest table a search can ask for |
| cells-4524-sparse | L32 + ngggtcagttcaagcn   | d=12 p=5 g=16  | (2, 13, 29, 6) | 4524: direct, and few enough candidates for  |
|                   |                          |                |                | the per-bin kernels                          |
"""
import numpy as np
import pytest

from fasta_util import write_fasta
from parity_util import oracle_rows, synth_fasta
from scores_util import SITE, distinct_model
from test_gpu_counts import GUIDE, L32, planted
from test_gpu_limits import L20, SMALL
from test_gpu_scores import edge_genome

pytestmark = pytest.mark.gpu

LDS_CELLS = 4096                      # hits_dev.hpp COUNTS_LDS_CELLS
STRIDE = 128 * 256                    # counts_grid's cap times COUNTS_BLOCK: the items one pass of the lanes covers
PAM16 = "ngggtcagttcaagcn"
PATHS = [("default", {}), ("general", {"CALITAS_BINNED": "0"}), ("wave-per-bin", {"CALITAS_BINNED_COMPLEX": "1"}),
         ("host-hits", {"CALITAS_HOST_HITS": "1"})]
CASES = [
    # (id, guide, params, expected shape)
    ("cells-4096", L20 + "nrg", dict(d=31, p=1, g=0), (2, 32, 32, 2)),
    ("cells-4224", L20 + "nrg", dict(d=31, p=1, g=1), (2, 32, 33, 2)),
    ("cells-9702-dense", L32 + PAM16, dict(d=32, p=2, g=16), (2, 33, 49, 3)),
    ("cells-4524-sparse", L32 + PAM16, dict(d=12, p=5, g=16), (2, 13, 29, 6)),
]


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


def params_of(C, kw):
    return C.make_params(max_guide_diffs=kw["d"], max_pam_mismatches=kw["p"], max_gaps_between_guide_and_pam=kw["g"])


def sparse_fasta(tmp_path):
    """Two contigs over eight and six bins of 8192 bases, a copy of the 48-base site every 2000 bases (closer together a bin holds more
    than the 64 raw alignments of its wave, and the per-bin kernels decline) at 0, 3, 8, 10, 11 and 12 edits (mostly 11: a good part
    of the 11- and 12-edit copies align with gaps instead, below 11 mismatches), five of six reversed.  The minus half of the
    (2, 13, 29, 6) table starts at flat index 2262: a minus-strand hit with 11 or more mismatches lies at 4096 or above."""
    rng = np.random.default_rng(4574)
    edits = (0, 3, 8, 10, 11, 12, 11, 11, 11, 12, 11, 11, 11, 11)
    contigs, k = [], 0
    for ci, length in enumerate((7 * 8192 + 3000, 5 * 8192 + 2000)):
        sites = []
        for pos in range(700, length - 300, 2000):
            sites.append((pos + 37 * ci, edits[k % len(edits)], k % 6 != 0))
            k += 1
        contigs.append(("s%d" % ci, planted(rng, length, sites, site=L32 + "AGGGTCAGTTCAAGCT")))
    return write_fasta(str(tmp_path / "sparse.fa"), contigs)


def case_fasta(tmp_path, cid, guide, kw):
    if cid == "cells-4524-sparse":
        return sparse_fasta(tmp_path)
    step = 1000 - (len(guide) + kw["d"] + kw["g"] - 1)
    return synth_fasta(tmp_path, 31 + len(cid), [guide], lengths=SMALL if cid == "cells-9702-dense" else (9000, 3000, 31), step_hint=step)


def flat_index(r, shape):
    return (((r["strand"] == "-") * shape[1] + int(r["guide_mm"])) * shape[2] + int(r["guide_gaps"])) * shape[3] + int(r["pam_mm"])


def text_rows(C, ctx, G, params):
    text, n = ctx.search_hits(G, "a", params, "v0", "stamp")
    rows = C.read_hits(text)
    assert len(rows) == n
    return rows


@pytest.mark.parametrize("cfg", CASES, ids=lambda c: c[0])
def test_tables_around_the_lds_limit(C, cfg, tmp_path, monkeypatch):
    """A1: counts and scores of tables of 4096 cells and more on the per-bin kernels, the general kernels, the wave-per-bin kernel and
    the host stage, a fresh context per path (a decline is remembered by the context)."""
    cid, guide, kw, shape = cfg
    cells = int(np.prod(shape))
    fa = case_fasta(tmp_path, cid, guide, kw)
    G = C.Guide(guide)
    model = distinct_model(C, G.protospacer_length, seed=len(cid))
    want_rows = oracle_rows(fa, guide, **kw)
    want = C.counts_of_rows(want_rows, shape)
    want_scores = C.scores_of_rows(want_rows, model, shape)
    flat = [flat_index(r, shape) for r in want_rows]
    high = sum(1 for x in flat if x >= LDS_CELLS)
    minus = sum(1 for r in want_rows if r["strand"] == "-")
    print(cid, "shape", shape, "cells", cells, "rows", len(want_rows), "minus", minus, "rows at 4096 or above", high,
          "in cells", len({x for x in flat if x >= LDS_CELLS}), want_scores)
    # what the case is there for, on the oracle alone
    assert 0 < minus < len(want_rows)
    assert want_scores.perfect >= 1 and want_scores.sum_q32 > 0
    if cells > 4524:
        assert high >= 5
    if cid == "cells-4524-sparse":
        assert high >= 10 and cells > LDS_CELLS               # (above the 3 rows of a first try)
        assert max(len(r["padded_guide"]) for r in want_rows) <= 64          # (a wider row is one the per-bin kernels decline)
    if cid == "cells-4224":
        assert cells > LDS_CELLS and minus == sum(1 for x in flat if x >= cells // 2) and cells // 2 == 2112
    if cid == "cells-4096":
        assert cells == LDS_CELLS
    params = params_of(C, kw)
    for name, env in PATHS:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = C.Context(0)
        ctx.set_reference_fasta(fa)
        try:
            got = ctx.search_counts(G, params)
            tm = ctx.timing()
            scored = ctx.search_scores(G, params, model)
            ts = ctx.timing()
            print(cid, name, "shape", got.shape, "rows", int(got.sum()), "rows at 4096 or above", int(got.ravel()[LDS_CELLS:].sum()),
                  "binned_lanes", tm["binned_lanes"], "/", ts["binned_lanes"], "lanes", tm["lanes"], "accepted", tm["accepted_alignments"], scored)
            assert got.dtype == np.uint64 and got.shape == shape == scored.table.shape, (cid, name)
            assert np.array_equal(got, want), (cid, name)
            assert (scored.rows, scored.perfect, scored.sum_q32, scored.max_q32) == \
                (want_scores.rows, want_scores.perfect, want_scores.sum_q32, want_scores.max_q32), (cid, name)
            assert scored == want_scores, (cid, name)
            assert tm["hit_rows"] == len(want_rows) == ts["hit_rows"] and tm["hits_bytes"] == 0 == ts["hits_bytes"], (cid, name)
            rows = text_rows(C, ctx, G, params)
            assert np.array_equal(got, C.counts_of_rows(rows, shape)) and scored == C.scores_of_rows(rows, model, shape), (cid, name)
            # which kernels ran
            if name in ("general", "host-hits"):
                assert tm["binned_lanes"] == 0 == ts["binned_lanes"], (cid, name)
            elif cid == "cells-4524-sparse":
                assert tm["binned_lanes"] > 0 and ts["binned_lanes"] > 0, (cid, name)      # bin_counts_kernel / bin_scores_kernel, direct branch
            else:
                # E is about L: nearly every column is a candidate, the bins are crowded and the per-bin kernels decline
                assert tm["binned_lanes"] == 0 == ts["binned_lanes"], (cid, name)
        finally:
            ctx.close()
        for k in env:
            monkeypatch.delenv(k)


def test_the_device_table_is_left_clean(C, tmp_path, monkeypatch):
    """A2: calls of 9702, 4096, 192 and again 9702 cells on one context -- the kernels zero what they used, on the LDS branch and on the
    direct one, and in score mode the four words behind the cells, which move with the table's size -- equal a fresh context's, on the
    default path and on the general kernels."""
    big = CASES[2]
    fa = case_fasta(tmp_path, big[0], big[1], big[2])
    calls = [(C.Guide(big[1]), params_of(C, big[2]), big[3]), (C.Guide(CASES[0][1]), params_of(C, CASES[0][2]), CASES[0][3]),
             (C.Guide(GUIDE), C.make_params(max_gaps_between_guide_and_pam=2), (2, 6, 8, 2)), (C.Guide(big[1]), params_of(C, big[2]), big[3])]
    models = [distinct_model(C, g.protospacer_length, seed=11) for g, _, _ in calls]

    def fresh(fn):
        ctx = C.Context(0)
        ctx.set_reference_fasta(fa)
        try:
            return fn(ctx)
        finally:
            ctx.close()
    for env in ({}, {"CALITAS_BINNED": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        want = [fresh(lambda ctx: ctx.search_counts(g, p)) for g, p, _ in calls[:3]]
        want_scores = [fresh(lambda ctx: ctx.search_scores(g, p, m)) for (g, p, _), m in zip(calls[:3], models)]
        want.append(want[0])
        want_scores.append(want_scores[0])
        print(env, [(w.shape, int(w.sum()), int(w.ravel()[LDS_CELLS:].sum())) for w in want], want_scores)
        assert [w.shape for w in want] == [s for _, _, s in calls] and all(w.sum() > 0 for w in want)
        assert want[0].ravel()[LDS_CELLS:].sum() >= 5 and all(s.sum_q32 > 0 and s.perfect > 0 for s in want_scores)
        ctx = C.Context(0)
        ctx.set_reference_fasta(fa)
        try:
            for i, (g, p, _) in enumerate(calls):
                assert np.array_equal(ctx.search_counts(g, p), want[i]), (env, "counts", i)
            for i, ((g, p, _), m) in enumerate(zip(calls, models)):
                assert ctx.search_scores(g, p, m) == want_scores[i], (env, "scores", i)
            # a counts call between two score calls, large table and small
            for i in (0, 2, 3, 1):
                g, p, _ = calls[i]
                assert ctx.search_scores(g, p, models[i]) == want_scores[i], (env, "scores, interleaved", i)
                assert np.array_equal(ctx.search_counts(g, p), want[i]), (env, "counts, interleaved", i)
                assert ctx.search_scores(g, p, models[i]) == want_scores[i], (env, "scores again", i)
        finally:
            ctx.close()
        for k in env:
            monkeypatch.delenv(k)


REPEAT_UNITS = 4500                   # measured on an MI355X: accepted_alignments = 77 032 at this length (the bound is 65 536)
REPEAT_WINDOW = 300


def test_more_items_than_one_stride(C, tmp_path, monkeypatch):
    """A3: a tandem repeat, PAM-less at d = 8 and -O 100, one lane on the general kernels: more than 2 x 32 768 accepted alignments, so
    that every lane of counts_kernel / scores_kernel takes a second and a third item.  With all factors distinct a hit scored twice or
    skipped changes sum_q32.  Against the oracle's rows and the text of the same call.
    (Windows of 300 bases: the repeat gives two hits per base, and a window of 1000 keeps about 1000 of them per strand -- beyond the
    512 the device's per-window filter holds, so that the host stages would finish the call and the two kernels never run.)"""
    monkeypatch.setenv("CALITAS_CHUNKS", "1")
    monkeypatch.setenv("CALITAS_BINNED", "0")
    unit, guide, shape = "ACGTTGCA", "ACGTTGCAACGTTGCAACGT", (2, 9, 12, 1)
    fa = write_fasta(str(tmp_path / "repeat.fa"), [("rep", unit * REPEAT_UNITS)])
    G = C.Guide(guide)
    model = distinct_model(C, 20)
    params = C.make_params(window_size=REPEAT_WINDOW, max_guide_diffs=8, max_overlap=100)
    want_rows = oracle_rows(fa, guide, d=8, O=100, window_size=REPEAT_WINDOW)
    want = C.scores_of_rows(want_rows, model, shape)
    print("repeat", want, "minus", sum(1 for r in want_rows if r["strand"] == "-"))
    assert want.rows > 2 * STRIDE and want.perfect > 0 and np.count_nonzero(want.table) >= 12 and want.table[0].sum() > 0 and want.table[1].sum() > 0
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        got = ctx.search_counts(G, params)
        tm = ctx.timing()
        scored = ctx.search_scores(G, params, model)
        ts = ctx.timing()
        print("repeat accepted_alignments", tm["accepted_alignments"], ts["accepted_alignments"], "rows", int(got.sum()), "lanes", tm["lanes"],
              "binned_lanes", tm["binned_lanes"], "host_post_ms", tm["host_post_ms"], ts["host_post_ms"], scored)
        assert tm["accepted_alignments"] > 2 * STRIDE and ts["accepted_alignments"] > 2 * STRIDE
        assert tm["lanes"] == 1 == ts["lanes"] and tm["binned_lanes"] == 0 == ts["binned_lanes"]
        assert tm["host_post_ms"] == 0 == ts["host_post_ms"]          # (the time of the host's per-window filter: it did not run)
        assert got.shape == shape and np.array_equal(got, want.table)
        assert (scored.rows, scored.perfect, scored.sum_q32, scored.max_q32) == (want.rows, want.perfect, want.sum_q32, want.max_q32)
        assert scored == want
        rows = text_rows(C, ctx, G, params)
        assert scored == C.scores_of_rows(rows, model, shape) and np.array_equal(got, C.counts_of_rows(rows, shape))
    finally:
        ctx.close()


def test_factors_of_zero_and_one(C, tmp_path, monkeypatch):
    """A4: factors at the ends of their range on the device -- 65536 (1.0: the one value that needs 17 bits) and 0 -- against
    scores_of_rows and against closed forms that need no model arithmetic; and a call whose only hits are perfect (hits, no score)."""
    fa, _ = edge_genome(C, tmp_path)
    # ... with two hits that have no protospacer mismatch and are not perfect: a PAM mismatch (TCG under nrg) and a gap before the PAM
    contigs = [(name, seq.decode()) for name, seq in C.read_fasta(fa).items()]
    # (each in the last bin of its contig, which holds few other sites: a bin with more than 64 raw alignments declines)
    k2, k3 = contigs[2][1], contigs[3][1]
    contigs[2] = (contigs[2][0], k2[:36000] + SITE[:20] + "TCGTTT" + k2[36026:])
    contigs[3] = (contigs[3][0], k3[:27500] + SITE[:20] + "AC" + SITE[20:] + k3[27525:])
    assert [len(c[1]) for c in contigs[2:4]] == [40000, 30000]
    fa = write_fasta(str(tmp_path / "edge_ends.fa"), contigs)
    G = C.Guide(GUIDE)
    params = C.make_params(max_gaps_between_guide_and_pam=2)
    shape = (2, 6, 8, 2)
    want_rows = oracle_rows(fa, GUIDE, g=2)
    table = C.counts_of_rows(want_rows, shape)
    n, perfect, no_mm = len(want_rows), sum(1 for r in want_rows if int(r["total_mm_plus_gaps"]) == 0), int(table[:, 0].sum())
    print("edge rows", n, "perfect", perfect, "without a protospacer mismatch", no_mm)
    assert n > 92 and perfect >= 16 + 3 and no_mm >= perfect + 2               # (a hit with a gap or a PAM mismatch only scores 1.0)
    assert table[:, 0, 0, 1].sum() >= 1 and table[:, 0, 1:, 0].sum() >= 1
    one = C.ScoreModel.uniform(20)
    models = [("all 1.0", one, (n - perfect) << 32, 1 << 32),
              ("mismatch 0", C.ScoreModel.uniform(20, mismatch=0), (no_mm - perfect) << 32, 1 << 32),
              ("all 0", C.ScoreModel.uniform(20, mismatch=0, gap=0, pam_mismatch=0), 0, 0)]
    exact = planted(np.random.default_rng(65536), 20000, [(7777, 0, True)], site=SITE)
    fa1 = write_fasta(str(tmp_path / "one.fa"), [("one", exact)])
    p0 = C.make_params(max_guide_diffs=0, max_pam_mismatches=0, max_gaps_between_guide_and_pam=0)
    rows1 = oracle_rows(fa1, GUIDE, d=0, p=0, g=0)
    assert len(rows1) >= 1 and all(int(r["total_mm_plus_gaps"]) == 0 for r in rows1)
    for env in ({}, {"CALITAS_BINNED": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = C.Context(0)
        ctx.set_reference_fasta(fa)
        try:
            for name, model, want_sum, want_max in models:
                got = ctx.search_scores(G, params, model)
                tm = ctx.timing()
                print(env, name, got, "binned_lanes", tm["binned_lanes"])
                assert (tm["binned_lanes"] > 0) == (not env), (env, name)
                assert (got.rows, got.perfect, got.sum_q32, got.max_q32) == (n, perfect, want_sum, want_max), (env, name)
                assert got == C.scores_of_rows(want_rows, model, shape), (env, name)
        finally:
            ctx.close()
        ctx = C.Context(0)
        ctx.set_reference_fasta(fa1)
        try:
            got = ctx.search_scores(G, p0, distinct_model(C, 20))
            print(env, "perfect only", got, "binned_lanes", ctx.timing()["binned_lanes"])
            assert got.rows == got.perfect == len(rows1) and got.sum_q32 == 0 == got.max_q32
            assert got == C.scores_of_rows(rows1, distinct_model(C, 20), got.table.shape)
        finally:
            ctx.close()
        for k in env:
            monkeypatch.delenv(k)
