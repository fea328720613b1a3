"""GPU: calitas_search_regions / calitas_search_regions_batch (regions_kernel in hits.hip, bin_regions_kernel in binned.hip, the host
stage behind them) against regions_of_rows -- class_of_row, a plain scan of the RAW intervals, and score_of_row per row -- of the text
the same call returns through calitas_search_hits, on every path a call can take; against the oracle's rows; across workgroups; with
the classes' table in LDS and beyond it; as merges over window ranges; through the guide batch; and through the two command-line
tools.  The intervals are derived from the text's own rows (regions_util), and every test asserts the edge cases are in its input.
Every comparison is an equality of RegionScores objects."""
import os
import subprocess
import sys

import numpy as np
import pytest

from parity_util import oracle_rows, synth_fasta
from regions_util import check_regions, derive_regions, striped_regions
from scores_util import distinct_model
from test_gpu_counts import BIN, ENV_PATHS, GUIDE, SHAPES, STEP, genome, ranges_genome
from test_gpu_scores import edge_genome
from test_gpu_table_limits import REPEAT_UNITS, REPEAT_WINDOW, STRIDE
from test_gpu_top import bins_genome, graded_repeat, text_rows, uniform_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


def lengths_of(ctx):
    return dict(zip(ctx.contig_names, ctx.contig_lengths))


def sums_to(got):
    total = got.by_class[0]
    for s in got.by_class[1:]:
        total = total + s
    return total


def test_every_path_gives_the_classes_of_the_text(C, tmp_path, monkeypatch):
    """search_regions == regions_of_rows(read_hits(search_hits text)) on the per-bin kernels, the general kernels, the wave-per-bin
    kernel, three ranges and one, the host stages, one pass per contig and -O 0; by_class sums to search_scores; with a full mask
    .top == search_top; no text crosses; the error cases."""
    fa, _ = edge_genome(C, tmp_path)
    G = C.Guide(GUIDE)
    model = distinct_model(C, 20)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        params = C.make_params(max_gaps_between_guide_and_pam=2)
        with pytest.raises(C.CalitasError) as e:                  # no regions set
            ctx.search_regions(G, params, model, 8)
        assert e.value.code == C._lib.EINVAL
        rows = text_rows(C, ctx, G, params)
        reg, facts = derive_regions(C, rows, lengths_of(ctx), model)
        check_regions(C, rows, reg, facts, model)
        ctx.set_regions(reg)
        first = None
        for name, env in ENV_PATHS:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got = ctx.search_regions(G, params, model, 8, 0b10010010)
            tm = ctx.timing()
            full = ctx.search_regions(G, params, model, 8)
            rows = text_rows(C, ctx, G, params)
            shape = got.top.scores.table.shape
            print(name, got, "binned_lanes", tm["binned_lanes"], "lanes", tm["lanes"], "passes", tm["contig_passes"])
            assert got == C.regions_of_rows(rows, model, reg, 8, 0b10010010, shape), name
            assert full == C.regions_of_rows(rows, model, reg, 8, None, shape), name
            assert sums_to(got) == ctx.search_scores(G, params, model) == got.top.scores, name
            assert full.top == ctx.search_top(G, params, model, 8), name
            assert tm["hits_bytes"] == 0, name
            assert 3 <= len(got.top.hits) < 8 == len(full.top.hits) and set(got.hit_class) == {1, 4, 7}
            if name == "default":
                assert tm["binned_lanes"] > 0
                first = got
                assert got == C.regions_of_rows(oracle_rows(fa, GUIDE, g=2), model, reg, 8, 0b10010010, shape)
            if name in ("general", "host-hits"):
                assert tm["binned_lanes"] == 0
            assert got == first, name
            for k in env:
                monkeypatch.delenv(k)
        p0 = C.make_params(max_gaps_between_guide_and_pam=2, max_overlap=0)     # -O 0: no device row stage, the host stage classes
        for k in (2, 8):
            got = ctx.search_regions(G, p0, model, k)
            assert got == C.regions_of_rows(text_rows(C, ctx, G, p0), model, reg, k, None, got.top.scores.table.shape)
            assert got.top.scores.rows - got.top.scores.perfect > 2
        for k, mask in ((257, None), (8, 0), (8, 0xFFFFFF00)):
            with pytest.raises(C.CalitasError) as e:
                ctx.search_regions(G, params, model, k, mask)
            assert e.value.code == C._lib.EINVAL
        with pytest.raises(C.CalitasError):
            ctx.search_regions(G, params, distinct_model(C, 21), 8)
    finally:
        ctx.close()


def test_ties_under_a_mask_on_both_tails(C, tmp_path, monkeypatch):
    """A uniform model: k cuts between two equal scores AMONG THE MASKED CANDIDATES while a hit of a higher score outside the mask
    exists: the selection sees only the mask's hits (a mask applied after it would list fewer, or others) -- per-bin and general tail."""
    fa, _ = genome(tmp_path, crowded=False)
    G = C.Guide(GUIDE)
    model = uniform_model(C)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        params = C.make_params(max_gaps_between_guide_and_pam=2)
        rows = text_rows(C, ctx, G, params)
        reg, facts = derive_regions(C, rows, lengths_of(ctx), model)
        check_regions(C, rows, reg, facts, model)
        ctx.set_regions(reg)
        everything = C.regions_of_rows(rows, model, reg, 256)
        found = None
        for mask in range(1, 256):
            cand = [h for h, c in zip(everything.top.hits, everything.hit_class) if (mask >> c) & 1]
            out = [h for h, c in zip(everything.top.hits, everything.hit_class) if not (mask >> c) & 1]
            ks = [i for i in range(1, len(cand)) if cand[i - 1].score_q32 == cand[i].score_q32 and out and out[0].score_q32 > cand[i].score_q32]
            if ks:
                found = (mask, ks[0], cand, out)
                break
        assert found, "no mask with a tie among its candidates and a better hit outside it"
        mask, k, cand, out = found
        for env, binned in (({}, True), ({"CALITAS_BINNED": "0"}, False)):
            for kk, v in env.items():
                monkeypatch.setenv(kk, v)
            for kk in (k, k + 1, 256):
                got = ctx.search_regions(G, params, model, kk, mask)
                assert (ctx.timing()["binned_lanes"] > 0) == binned
                assert got == C.regions_of_rows(rows, model, reg, kk, mask, got.top.scores.table.shape), (env, kk)
                assert got.top.hits == cand[:kk] and out[0] not in got.top.hits
            for kk in env:
                monkeypatch.delenv(kk)
    finally:
        ctx.close()


def test_several_workgroups_of_the_per_bin_kernel_and_clean_state(C, tmp_path):
    """600 bins with a hit each and regions alternating by bin (8 classes): three workgroups of bin_regions_kernel.  Then, on one
    context and in this order: regions (8 classes), scores, counts, top, regions again after set_regions with another set of 2
    classes -- each equals its own contract: the larger area of one call leaves nothing to the next."""
    fa = bins_genome(tmp_path)
    G = C.Guide(GUIDE)
    params = C.make_params(max_gaps_between_guide_and_pam=2)
    model = distinct_model(C, 20)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        rows = text_rows(C, ctx, G, params)
        assert len(rows) >= 600 and {r["strand"] for r in rows} == {"+", "-"}
        shape = ctx.search_counts(G, params).shape
        reg8 = striped_regions(C, 600 * BIN, "big", BIN, 8)
        reg2 = striped_regions(C, 600 * BIN, "big", 3 * BIN + 11, 2)
        want8 = C.regions_of_rows(rows, model, reg8, 200, 0b01010101, shape)
        assert all(s.rows - s.perfect >= 1 for s in want8.by_class) and len(want8.top.hits) == 200
        ctx.set_regions(reg8)
        got = ctx.search_regions(G, params, model, 200, 0b01010101)
        tm = ctx.timing()
        assert tm["binned_lanes"] == tm["lanes"] >= 1 and got == want8
        for m, k, mask in ((uniform_model(C), 5, 0b10), (model, 1, None)):
            assert ctx.search_regions(G, params, m, k, mask) == C.regions_of_rows(rows, m, reg8, k, mask, shape), (k, mask)
        assert ctx.search_scores(G, params, model) == want8.top.scores
        assert np.array_equal(ctx.search_counts(G, params), want8.top.scores.table)
        assert ctx.search_top(G, params, model, 256) == C.top_of_rows(rows, model, 256, shape)
        ctx.set_regions(reg2)
        got = ctx.search_regions(G, params, model, 7, 0b10)
        assert got == C.regions_of_rows(rows, model, reg2, 7, 0b10, shape) and len(got.by_class) == 2 and all(s.rows for s in got.by_class)
    finally:
        ctx.close()


def test_strides_of_the_general_kernel(C, tmp_path, monkeypatch):
    """The graded tandem repeat on one lane of the general kernels (`-d 8 -O 100`, windows of 300): more than 2 x 32 768 sorted
    positions, 128 workgroups of three trips of regions_kernel, stripes of 8 classes over the repeat; k = 256 under a mask, and k = 0."""
    monkeypatch.setenv("CALITAS_CHUNKS", "1")
    monkeypatch.setenv("CALITAS_BINNED", "0")
    guide, shape = "ACGTTGCAACGTTGCAACGT", (2, 9, 12, 1)
    fa = graded_repeat(tmp_path)
    G = C.Guide(guide)
    params = C.make_params(window_size=REPEAT_WINDOW, max_guide_diffs=8, max_overlap=100)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        rows = text_rows(C, ctx, G, params)
        reg = striped_regions(C, 8 * REPEAT_UNITS, "rep", 1501, 8)
        ctx.set_regions(reg)
        for model, k, mask in ((distinct_model(C, 20), 256, 0b10010010), (uniform_model(C), 256, 0b1), (distinct_model(C, 20), 0, None)):
            got = ctx.search_regions(G, params, model, k, mask)
            tm = ctx.timing()
            assert tm["accepted_alignments"] > 2 * STRIDE and tm["lanes"] == 1 and tm["binned_lanes"] == 0 and tm["host_post_ms"] == 0
            want = C.regions_of_rows(rows, model, reg, k, mask, shape)
            assert got == want, (k, mask, got.top.hits[:3], want.top.hits[:3])
            assert len(got.top.hits) == k and all(s.rows - s.perfect >= 1 for s in got.by_class)
    finally:
        ctx.close()


@pytest.mark.parametrize("cid", ["costs-E3d", "pamless-d8", "5prime-tttv"])
def test_table_sizes_against_the_oracle(C, cid, tmp_path, monkeypatch):
    """costs-E3d with 8 classes has 780 x 8 = 6240 cells, above COUNTS_LDS_CELLS (4096): the direct-add path; the same shape with 2
    classes stays in LDS.  pamless-d8 and 5prime-tttv besides; all against the oracle's rows, on the three tails."""
    _, guide, aux, kw, lengths, shape = next(c for c in SHAPES if c[0] == cid)
    step = 1000 - (len(guide) + kw.get("d", 5) + kw.get("g", 3) - 1)
    fa = synth_fasta(tmp_path, 31 + len(cid), [guide], lengths=lengths, step_hint=step)
    pk = dict(max_guide_diffs=kw.get("d", 5), max_pam_mismatches=kw.get("p", 1), max_gaps_between_guide_and_pam=kw.get("g", 3))
    pk.update({k: v for k, v in kw.items() if k.endswith("_net_cost")})
    G = C.Guide(guide, aux)
    model = distinct_model(C, G.protospacer_length, seed=len(cid))
    want_rows = oracle_rows(fa, guide, aux, **kw)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        reg8, facts = derive_regions(C, want_rows, lengths_of(ctx), model, whole_contig=len(lengths) >= 3)
        check_regions(C, want_rows, reg8, facts, model, whole_contig=len(lengths) >= 3)
        cells = int(np.prod(shape))
        sets = [(reg8, 0b11110111)]
        if cid == "costs-E3d":
            assert cells * 8 == 6240 > 4096 >= cells * 2
            name = ctx.contig_names[0]
            sets.append((C.Regions([(name, 0, ctx.contig_lengths[0] // 2, "half")]), 0b11))
        for reg, mask in sets:
            ctx.set_regions(reg)
            want = C.regions_of_rows(want_rows, model, reg, 10, mask, shape)
            assert len(want.top.hits) >= 5 and len(set(want.hit_class)) > 1
            for env in ({}, {"CALITAS_BINNED": "0"}, {"CALITAS_HOST_HITS": "1"}):
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                got = ctx.search_regions(G, C.make_params(**pk), model, 10, mask)
                print(cid, env, got, "binned_lanes", ctx.timing()["binned_lanes"])
                assert got == want, (cid, env, len(reg.classes))
                for k in env:
                    monkeypatch.delenv(k)
    finally:
        ctx.close()


@pytest.mark.parametrize("cuts", [2, 3, 8])
def test_window_ranges_merge(C, tmp_path, monkeypatch, cuts):
    """Each window range's result is regions_of_rows of that range's text, and RegionScores.merge of the ranges in order is the whole
    call's: per-bin kernels, two lanes, general kernels, and the whole-contig fallback (which classes from the rows' columns)."""
    from calitas_amd import shard
    fa, lengths = ranges_genome(tmp_path, np.random.default_rng(100 + cuts))
    G = C.Guide(GUIDE)
    pk = dict(max_gaps_between_guide_and_pam=2)
    model, k, mask = uniform_model(C), 30, 0b11101111
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        rows = text_rows(C, ctx, G, C.make_params(**pk))
        reg, facts = derive_regions(C, rows, lengths_of(ctx), model)
        check_regions(C, rows, reg, facts, model)
        ctx.set_regions(reg)
        whole = ctx.search_regions(G, C.make_params(**pk), model, k, mask)
        shape = whole.top.scores.table.shape
        assert whole == C.regions_of_rows(rows, model, reg, k, mask, shape) and len(whole.top.hits) == k
        parts = shard.window_partition(lengths, cuts, STEP)
        for mode, env in (("default", {}), ("two lanes", {"CALITAS_CHUNKS": "2"}), ("general", {"CALITAS_BINNED": "0"}),
                          ("whole contigs", {"CALITAS_OWN_GENERAL_OFF": "1"})):
            for kk, v in env.items():
                monkeypatch.setenv(kk, v)
            pieces = []
            for first, n in parts:
                pr = C.make_params(first_window=first, n_windows=n, **pk)
                got = ctx.search_regions(G, pr, model, k, mask)
                assert got == C.regions_of_rows(text_rows(C, ctx, G, pr), model, reg, k, mask, shape), (mode, first, n)
                pieces.append(got)
            assert pieces[0].merge(*pieces[1:]) == whole, (cuts, mode)
            for kk in env:
                monkeypatch.delenv(kk)
    finally:
        ctx.close()


def test_batches(C, tmp_path, monkeypatch):
    """search_regions_batch of 6 guides equals 6 single calls: whole reference and a window range; five lanes (default), one, three."""
    from calitas_amd import shard, synth
    guides = [GUIDE] + synth.random_guides(0xC4, 5)
    fa = synth_fasta(tmp_path, 5, guides, lengths=(50000, 20000, 30000))
    G = [C.Guide(g) for g in guides]
    model = distinct_model(C, 20)
    first, n = shard.window_partition([50000, 20000, 30000], 3, STEP)[1]
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        reg = C.Regions([(nm, a, min(a + 700, ln), "c%d" % (1 + (a // 1000) % 7)) for nm, ln in lengths_of(ctx).items() for a in range(0, ln, 1000)])
        ctx.set_regions(reg)
        for pk in (dict(max_gaps_between_guide_and_pam=2), dict(max_gaps_between_guide_and_pam=2, first_window=first, n_windows=n)):
            params = C.make_params(**pk)
            single = [ctx.search_regions(g, params, model, 7, 0b11110101) for g in G]
            shape = single[0].top.scores.table.shape
            assert all(s == C.regions_of_rows(text_rows(C, ctx, g, params), model, reg, 7, 0b11110101, shape) for s, g in zip(single, G))
            assert sum(len(s.top.hits) for s in single) > (20 if "first_window" not in pk else 4)
            for lanes in (None, "1", "3"):
                if lanes:
                    monkeypatch.setenv("CALITAS_BATCH_LANES", lanes)
                got = ctx.search_regions_batch(G, params, model, 7, 0b11110101)
                assert len(got) == 6 and all(a == b for a, b in zip(got, single)), (pk, lanes)
                if lanes:
                    monkeypatch.delenv("CALITAS_BATCH_LANES")
        with pytest.raises(C.CalitasError):
            ctx.search_regions_batch(G, C.make_params(), model, 257)
    finally:
        ctx.close()


def test_k0_and_the_life_of_a_set(C, tmp_path, monkeypatch):
    """k = 0: no list, by_class unchanged, on both tails.  set_regions(n = 0), then a call: CALITAS_EINVAL.  set_reference drops the set."""
    fa, _ = edge_genome(C, tmp_path)
    G = C.Guide(GUIDE)
    model = distinct_model(C, 20)
    params = C.make_params(max_gaps_between_guide_and_pam=2)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        rows = text_rows(C, ctx, G, params)
        reg, facts = derive_regions(C, rows, lengths_of(ctx), model)
        check_regions(C, rows, reg, facts, model)
        ctx.set_regions(reg)
        with_list = ctx.search_regions(G, params, model, 8)
        for env in ({}, {"CALITAS_BINNED": "0"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got = ctx.search_regions(G, params, model, 0, 0)
            assert got.top.hits == [] and got.hit_class == [] and got.top.k == 0
            assert got.by_class == with_list.by_class and got.top.scores == with_list.top.scores
            assert got == C.regions_of_rows(rows, model, reg, 0, None, got.top.scores.table.shape)
            for k in env:
                monkeypatch.delenv(k)
        ctx.set_regions(None)
        with pytest.raises(C.CalitasError) as e:
            ctx.search_regions(G, params, model, 8)
        assert e.value.code == C._lib.EINVAL
        ctx.set_regions(reg)
        assert ctx.search_regions(G, params, model, 8) == with_list
        ctx.set_reference_fasta(fa)
        with pytest.raises(C.CalitasError) as e:
            ctx.search_regions(G, params, model, 8)
        assert e.value.code == C._lib.EINVAL
        assert ctx.search_top(G, params, model, 8) == with_list.top
    finally:
        ctx.close()


def test_regions_flag_end_to_end(C, tmp_path):
    """Both tools with `--scores m.tsv --regions r.bed --top 5 --top-classes exon,c4,c7 --counts` write the same bytes: the scores
    TSV, the classes' TSV, the top TSV with its class column, the counts TSV, an empty line between -- the contract's bytes for the
    hits.txt the same flags give without them.  The counts TSV stays the totals; --regions without --scores is refused by both."""
    fa, _ = edge_genome(C, tmp_path)
    model = distinct_model(C, 20)
    mpath, bed = str(tmp_path / "m.tsv"), str(tmp_path / "r.bed")
    model.write(mpath)
    flags = ["-i", GUIDE, "-I", "g1", "-r", fa, "-g", "2", "-d", "4"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    py_out, cli_out, hits = str(tmp_path / "py.tsv"), str(tmp_path / "cli.tsv"), str(tmp_path / "hits.txt")
    subprocess.run([sys.executable, "-m", "calitas_amd", "SearchReference", "-o", hits] + flags, check=True, env=env, cwd=ROOT, timeout=300)
    rows = C.read_hits(hits)
    lengths = {n: len(s) for n, s in C.read_fasta(fa).items()}
    reg, facts = derive_regions(C, rows, lengths, model)
    check_regions(C, rows, reg, facts, model)
    names = {"c1": "exon", "c2": "utr"}
    with open(bed, "w") as f:
        f.write("# derived from the rows\ntrack name=regions\n")
        f.write("chrNone\t5\t9\texon\n")                       # (a chromosome the reference lacks: skipped, and exon keeps the first priority)
        for c, a, b, k in sorted(reg.intervals, key=lambda iv: iv[3]):
            f.write("%s\t%d\t%d\t%s\n" % (c, a, b, names.get(reg.classes[k], reg.classes[k])))
    classes = ["elsewhere", "exon", "utr"] + ["c%d" % i for i in range(3, 8)]
    extra = ["--scores", mpath, "--regions", bed, "--top", "5", "--top-classes", "exon,c4,c7", "--counts"]
    p1 = subprocess.run([sys.executable, "-m", "calitas_amd", "SearchReference", "-o", py_out] + extra + flags, check=True, env=env, cwd=ROOT, timeout=300,
                        stderr=subprocess.PIPE, text=True)
    p2 = subprocess.run([os.path.join(ROOT, "calitas_amd", "calitas"), "SearchReference", "-o", cli_out] + extra + flags, check=True, timeout=300,
                        stderr=subprocess.PIPE, text=True)
    assert "1 intervals on chromosomes the reference does not have were skipped" in p1.stderr and "1 intervals on chromosomes" in p2.stderr
    text = open(py_out).read()
    assert text == open(cli_out).read()
    want = C.regions_of_rows(rows, model, reg, 5, 0b10010010, (2, 5, 7, 2))
    want.classes = classes
    assert 3 <= len(want.top.hits) <= 5 and set(want.hit_class) == {1, 4, 7}
    assert text == (C.scores_tsv("g1", want.top.scores) + "\n" + C.regions_tsv("g1", want) + "\n"
                    + C.top_tsv("g1", want.top, [classes[c] for c in want.hit_class]) + "\n" + C.counts_tsv("g1", want.top.scores.table))
    assert len(text.split("\n\n")) == 4
    for tool in ([os.path.join(ROOT, "calitas_amd", "calitas")], [sys.executable, "-m", "calitas_amd"]):
        assert subprocess.run(tool + ["SearchReference", "--regions", bed] + flags, env=env, cwd=ROOT, timeout=300).returncode == 2
