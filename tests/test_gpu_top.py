"""GPU: the top list of calitas_search_top / calitas_search_top_batch (top_kernel in hits.hip, bin_top_kernel in binned.hip, the host
stage behind them) against top_of_rows -- score_of_row per row, perfect rows dropped, a stable sort by descending score -- of the text
the same call returns through calitas_search_hits, on every path a call can take; against the oracle's rows; across workgroups, strides
and buffer overflows; as merges over window ranges; through the guide batch; and through the two command-line tools.  Every comparison
is an equality of Top objects (records field by field, and the scores)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fasta_util import write_fasta
from parity_util import oracle_rows, synth_fasta
from scores_util import distinct_model
from test_gpu_counts import BIN, ENV_PATHS, GUIDE, SHAPES, STEP, genome, planted, ranges_genome
from test_gpu_scores import edge_genome
from test_gpu_table_limits import REPEAT_UNITS, REPEAT_WINDOW, STRIDE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


def uniform_model(C, L=20):
    return C.ScoreModel.uniform(L, mismatch=32768, gap=16384, pam_mismatch=49152)


def text_rows(C, ctx, G, params):
    text, n = ctx.search_hits(G, "a", params, "v0", "stamp")
    rows = C.read_hits(text)
    assert len(rows) == n
    return rows


def tie_k(hits, at_least=2):
    """A k >= at_least such that the k-th and the (k+1)-th of the expected order have equal scores."""
    for i in range(at_least, len(hits)):
        if hits[i - 1].score_q32 == hits[i].score_q32:
            return i
    raise AssertionError("no two candidates with equal scores")


def test_every_path_gives_the_top_of_the_text(C, tmp_path, monkeypatch):
    """search_top == top_of_rows(read_hits(search_hits text)) and .scores == search_scores on the per-bin kernels, the general kernels,
    the wave-per-bin kernel, three ranges and one, the host stages, one pass per contig and -O 0; k = 8 is fewer than the candidates."""
    fa, _ = edge_genome(C, tmp_path)
    G = C.Guide(GUIDE)
    model = distinct_model(C, 20)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        params = C.make_params(max_gaps_between_guide_and_pam=2)
        first = None
        for name, env in ENV_PATHS:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got = ctx.search_top(G, params, model, 8)
            tm = ctx.timing()
            rows = text_rows(C, ctx, G, params)
            want = C.top_of_rows(rows, model, 8, got.scores.table.shape)
            print(name, got, [h.score_q32 for h in got.hits], "binned_lanes", tm["binned_lanes"], "lanes", tm["lanes"], "passes", tm["contig_passes"])
            assert len(got.hits) == 8 < got.scores.rows - got.scores.perfect, name
            assert got == want, (name, got.hits, want.hits)
            assert got.scores == ctx.search_scores(G, params, model), name
            assert tm["hits_bytes"] == 0, name
            if name == "default":
                assert tm["binned_lanes"] > 0
                first = got
                assert {h.strand for h in got.hits} == {"+", "-"} and len({h.chromosome for h in got.hits}) > 1
                assert got == C.top_of_rows(oracle_rows(fa, GUIDE, g=2), model, 8, got.scores.table.shape)
            if name in ("general", "host-hits"):
                assert tm["binned_lanes"] == 0
            assert got == first, name
            for k in env:
                monkeypatch.delenv(k)
        p0 = C.make_params(max_gaps_between_guide_and_pam=2, max_overlap=0)     # -O 0: no device row stage, the host stage lists
        for k in (2, 8):                      # (few rows survive -O 0: k = 2 is a selection among them, k = 8 takes them all)
            got = ctx.search_top(G, p0, model, k)
            assert got == C.top_of_rows(text_rows(C, ctx, G, p0), model, k, got.scores.table.shape)
            assert len(got.hits) == min(k, got.scores.rows - got.scores.perfect) and got.scores.rows - got.scores.perfect > 2
        for k in (0, 257):
            with pytest.raises(C.CalitasError) as e:
                ctx.search_top(G, params, model, k)
            assert e.value.code == C._lib.EINVAL
        with pytest.raises(C.CalitasError):
            ctx.search_top(G, params, distinct_model(C, 21), 8)
    finally:
        ctx.close()


def test_ties_at_the_boundary_on_both_tails(C, tmp_path, monkeypatch):
    """A uniform model: k cuts between two hits of equal score, and the one that comes earlier in the text is the last of the list --
    on the per-bin tail (rank = bin and slot) and on the general tail (rank = sorted position)."""
    fa, _ = genome(tmp_path, crowded=False)
    G = C.Guide(GUIDE)
    model = uniform_model(C)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        params = C.make_params(max_gaps_between_guide_and_pam=2)
        rows = text_rows(C, ctx, G, params)
        everything = C.top_of_rows(rows, model, 256)
        k = tie_k(everything.hits, at_least=5)
        assert everything.hits[k - 1].score_q32 == everything.hits[k].score_q32 and everything.hits[k - 1] != everything.hits[k]
        for env, binned in (({}, True), ({"CALITAS_BINNED": "0"}, False)):
            for kk, v in env.items():
                monkeypatch.setenv(kk, v)
            for kk in (k, k + 1, 256):
                got = ctx.search_top(G, params, model, kk)
                tm = ctx.timing()
                assert (tm["binned_lanes"] > 0) == binned
                assert got == C.top_of_rows(rows, model, kk, got.scores.table.shape), (env, kk)
            for kk in env:
                monkeypatch.delenv(kk)
    finally:
        ctx.close()


def test_crowded_bin_the_general_tail_finishes(C, tmp_path):
    """A bin with more alignments than its wave holds: the per-bin kernels decline (bin_top_kernel lists nothing) and the general
    kernels finish in top mode; the second call goes there at once."""
    fa, _ = genome(tmp_path, crowded=True)
    G = C.Guide(GUIDE)
    model = distinct_model(C, 20)
    params = C.make_params(max_gaps_between_guide_and_pam=2)
    ctx = C.Context(0)                    # (a fresh context: the decline is found, not remembered)
    ctx.set_reference_fasta(fa)
    try:
        got = ctx.search_top(G, params, model, 20)
        tm = ctx.timing()
        want = C.top_of_rows(text_rows(C, ctx, G, params), model, 20, got.scores.table.shape)
        print("crowded", got, "binned_lanes", tm["binned_lanes"], "lanes", tm["lanes"])
        assert got == want and got.scores.rows > 150 and len(got.hits) == 20
        assert tm["binned_lanes"] < tm["lanes"]          # a range finished on the general kernels
        assert ctx.search_top(G, params, model, 20) == want
    finally:
        ctx.close()


def graded_repeat(tmp_path):
    """The tandem repeat of test_gpu_table_limits with one base changed every 137 bases (three different changes in turn): the exact
    copies of the guide that cover a changed base become hits of one mismatch, at different guide positions and letters, so the best
    imperfect hits are spread over the whole contig instead of being the first of thousands of equal ones."""
    s = bytearray(("ACGTTGCA" * REPEAT_UNITS).encode())
    for i, pos in enumerate(range(60, len(s) - 60, 137)):
        s[pos] = ord("ACGT"[("ACGT".index(chr(s[pos])) + 1 + i % 3) % 4])
    return write_fasta(str(tmp_path / "graded_repeat.fa"), [("rep", s.decode())])


def test_strides_overflow_and_the_merge_of_128_lists(C, tmp_path, monkeypatch):
    """The graded tandem repeat on one lane of the general kernels, `-d 8 -O 100`, windows of 300: more than 2 x 32 768 sorted
    positions, so top_kernel runs 128 workgroups of three trips each.  A workgroup's first two trips cover 512 positions; its candidate
    buffer (512 keys) is compacted at the start of the third trip when more than 256 of them were listed, i.e. kept and not perfect.
    Of the accepted alignments (about 77 000) nearly nine in ten are listed (asserted below from the call's own numbers: more than
    three in five), spread evenly over the repeat, so every workgroup lists about 600 * 9 / 10 = 540 keys, some 450 of them in its
    first two trips: every workgroup's buffer overflows at k = 256.  The winners must come out of the last workgroup's fold of the 128
    lists: a hit's rank is its row's index plus the dropped hits before it (fewer than 256 in all, asserted), workgroup
    rank // 256 % 128 lists it, and the k = 256 winners' rows lie in at least 32 different workgroups by index (114 under the
    distinct model, 54 under the uniform one, where all 256 winners tie and the rank alone decides among thousands of equal scores).
    Against the oracle's rows and the text."""
    monkeypatch.setenv("CALITAS_CHUNKS", "1")
    monkeypatch.setenv("CALITAS_BINNED", "0")
    guide, shape = "ACGTTGCAACGTTGCAACGT", (2, 9, 12, 1)
    fa = graded_repeat(tmp_path)
    G = C.Guide(guide)
    params = C.make_params(window_size=REPEAT_WINDOW, max_guide_diffs=8, max_overlap=100)
    want_rows = oracle_rows(fa, guide, d=8, O=100, window_size=REPEAT_WINDOW)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        rows = text_rows(C, ctx, G, params)
        for model in (distinct_model(C, 20), uniform_model(C)):
            scored = [(s, i) for i, s in enumerate(C.score_of_row(r, model) for r in want_rows) if s is not None]
            ties = len(scored) - len({s for s, _ in scored})
            winners = sorted(scored, key=lambda x: -x[0])[:256]             # (stable: the tie rule), with each winner's row index
            for k in (256, 1):
                want = C.top_of_rows(want_rows, model, k, shape)
                got = ctx.search_top(G, params, model, k)
                tm = ctx.timing()
                listed = got.scores.rows - got.scores.perfect
                groups = {i // 256 % 128 for _, i in winners[:k]}
                print("repeat k", k, "accepted", tm["accepted_alignments"], "rows", got.scores.rows, "perfect", got.scores.perfect, "listed", listed,
                      "equal scores", ties, "workgroups of the winners", len(groups), "lanes", tm["lanes"], "binned_lanes", tm["binned_lanes"],
                      "host_post_ms", tm["host_post_ms"])
                assert tm["accepted_alignments"] > 2 * STRIDE and tm["lanes"] == 1 and tm["binned_lanes"] == 0 and tm["host_post_ms"] == 0
                assert 5 * listed > 3 * tm["accepted_alignments"] and got.scores.perfect > 0
                assert 0 <= tm["accepted_alignments"] - got.scores.rows < 256
                assert k == 1 or len(groups) >= 32
                assert got == want, (k, got.hits[:3], want.hits[:3])
                assert got == C.top_of_rows(rows, model, k, shape)
                assert len(got.hits) == k
            if model.gap == 16384:
                assert ties > 2000
    finally:
        ctx.close()


def bins_genome(tmp_path, n_bins=600):
    """One contig of n_bins bins with a site of 1-4 edits planted in every bin, on alternating strands."""
    rng = np.random.default_rng(600)
    sites = [(b * BIN + 1000 + int(rng.integers(0, 5000)), 1 + b % 4, bool(b & 1)) for b in range(n_bins)]
    return write_fasta(str(tmp_path / "bins.fa"), [("big", planted(rng, n_bins * BIN, sites))])


def test_several_workgroups_of_the_per_bin_kernel_and_clean_slots(C, tmp_path):
    """600 bins with a hit each: more than 256 listed bins, so bin_top_kernel runs three workgroups and the last one's merge of their
    lists decides the result; k = 256 and 5, all factors distinct and the uniform model (a site of e edits scores 2^-e: 150 ties per
    score).  Then, on the same context, k = 256, k = 1, a scores call, a counts call and k = 256 again: each is what it should be -- the
    slots of one call leave nothing to the next."""
    fa = bins_genome(tmp_path)
    G = C.Guide(GUIDE)
    params = C.make_params(max_gaps_between_guide_and_pam=2)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        rows = text_rows(C, ctx, G, params)
        assert len(rows) >= 600 and len({int(r["coordinate_start"]) // BIN for r in rows}) > 512 and {r["strand"] for r in rows} == {"+", "-"}
        shape = ctx.search_counts(G, params).shape
        for model in (distinct_model(C, 20), uniform_model(C)):
            for k in (256, 5):
                got = ctx.search_top(G, params, model, k)
                tm = ctx.timing()
                assert tm["binned_lanes"] == tm["lanes"] >= 1
                assert got == C.top_of_rows(rows, model, k, shape), (k, got.hits[:3])
                assert len(got.hits) == k
        model = distinct_model(C, 20)
        want = {k: C.top_of_rows(rows, model, k, shape) for k in (256, 1)}
        assert ctx.search_top(G, params, model, 256) == want[256]
        assert ctx.search_top(G, params, model, 1) == want[1]
        assert ctx.search_scores(G, params, model) == want[1].scores
        assert np.array_equal(ctx.search_counts(G, params), want[1].scores.table)
        assert ctx.search_top(G, params, model, 256) == want[256]
    finally:
        ctx.close()


@pytest.mark.parametrize("cuts", [2, 3, 8])
def test_window_ranges_merge(C, tmp_path, monkeypatch, cuts):
    """Each window range's top is top_of_rows of that range's text, and Top.merge of the ranges in order is the whole call's top: on
    the per-bin kernels, with the range cut once more into lanes, on the general kernels, and through the whole-contig fallback
    (which lists from the rows' columns)."""
    from calitas_amd import shard
    fa, lengths = ranges_genome(tmp_path, np.random.default_rng(100 + cuts))
    G = C.Guide(GUIDE)
    pk = dict(max_gaps_between_guide_and_pam=2)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        for model, k in ((distinct_model(C, 20), 12), (uniform_model(C), 30)):
            whole = ctx.search_top(G, C.make_params(**pk), model, k)
            shape = whole.scores.table.shape
            assert whole == C.top_of_rows(text_rows(C, ctx, G, C.make_params(**pk)), model, k, shape) and len(whole.hits) == k
            parts = shard.window_partition(lengths, cuts, STEP)
            assert len(parts) == cuts
            for mode, env in (("default", {}), ("two lanes", {"CALITAS_CHUNKS": "2"}), ("general", {"CALITAS_BINNED": "0"}),
                              ("whole contigs", {"CALITAS_OWN_GENERAL_OFF": "1"})):
                for kk, v in env.items():
                    monkeypatch.setenv(kk, v)
                pieces = []
                for first, n in parts:
                    pr = C.make_params(first_window=first, n_windows=n, **pk)
                    got = ctx.search_top(G, pr, model, k)
                    assert got == C.top_of_rows(text_rows(C, ctx, G, pr), model, k, shape), (mode, first, n)
                    pieces.append(got)
                assert pieces[0].merge(*pieces[1:]) == whole, (cuts, mode)
                for kk in env:
                    monkeypatch.delenv(kk)
    finally:
        ctx.close()


def test_batches(C, tmp_path, monkeypatch):
    """search_top_batch of 6 guides equals 6 single calls: whole reference and a window range, five lanes (default), one and three."""
    from calitas_amd import shard, synth
    guides = [GUIDE] + synth.random_guides(0xC4, 5)
    fa = synth_fasta(tmp_path, 5, guides, lengths=(50000, 20000, 30000))
    G = [C.Guide(g) for g in guides]
    model = distinct_model(C, 20)
    first, n = shard.window_partition([50000, 20000, 30000], 3, STEP)[1]
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        for pk in (dict(max_gaps_between_guide_and_pam=2), dict(max_gaps_between_guide_and_pam=2, first_window=first, n_windows=n)):
            params = C.make_params(**pk)
            single = [ctx.search_top(g, params, model, 7) for g in G]
            shape = single[0].scores.table.shape
            assert all(s == C.top_of_rows(text_rows(C, ctx, g, params), model, 7, shape) for s, g in zip(single, G))
            assert sum(len(s.hits) for s in single) > (30 if "first_window" not in pk else 6)
            for lanes in (None, "1", "3"):
                if lanes:
                    monkeypatch.setenv("CALITAS_BATCH_LANES", lanes)
                got = ctx.search_top_batch(G, params, model, 7)
                assert len(got) == 6 and all(a == b for a, b in zip(got, single)), (pk, lanes)
                if lanes:
                    monkeypatch.delenv("CALITAS_BATCH_LANES")
        with pytest.raises(C.CalitasError):
            ctx.search_top_batch(G, C.make_params(), model, 0)
    finally:
        ctx.close()


@pytest.mark.parametrize("cfg", SHAPES[:5], ids=lambda c: c[0])
def test_parameter_shapes_against_the_oracle(C, cfg, tmp_path, monkeypatch):
    """5' PAM, PAM-less d = 8, auxiliary PAMs, IUPAC protospacer, per-matrix: the three tails against the oracle's rows."""
    cid, guide, aux, kw, lengths, shape = cfg
    step = 1000 - (len(guide) + kw.get("d", 5) + kw.get("g", 3) - 1)
    fa = synth_fasta(tmp_path, 31 + len(cid), [guide], lengths=lengths, step_hint=step)
    pk = dict(max_guide_diffs=kw.get("d", 5), max_pam_mismatches=kw.get("p", 1), max_gaps_between_guide_and_pam=kw.get("g", 3),
              eqx_by_score=(1 if kw.get("switches", 0) & 2 else 0) | (2 if kw.get("switches", 0) & 1 else 0))
    G = C.Guide(guide, aux)
    model = distinct_model(C, G.protospacer_length, seed=len(cid))
    want_rows = oracle_rows(fa, guide, aux, **kw)
    want = C.top_of_rows(want_rows, model, 10, shape)
    assert len(want.hits) == 10 < want.scores.rows - want.scores.perfect
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        for env in ({}, {"CALITAS_BINNED": "0"}, {"CALITAS_HOST_HITS": "1"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got = ctx.search_top(G, C.make_params(**pk), model, 10)
            print(cid, env, got, "binned_lanes", ctx.timing()["binned_lanes"])
            assert got == want, (cid, env, got.hits, want.hits)
            for k in env:
                monkeypatch.delenv(k)
    finally:
        ctx.close()


def test_top_flag_end_to_end(C, tmp_path):
    """`python -m calitas_amd SearchReference --scores m.tsv --top 5 --counts` and `calitas SearchReference` with the same flags write
    the same bytes: the scores TSV, an empty line, the top TSV, an empty line, the counts TSV -- and they parse back to top_of_rows of
    the hits.txt the same flags give without them."""
    fa, _ = edge_genome(C, tmp_path)
    model = distinct_model(C, 20)
    mpath = str(tmp_path / "m.tsv")
    model.write(mpath)
    flags = ["-i", GUIDE, "-I", "g1", "-r", fa, "-g", "2", "-d", "4"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    py_out, cli_out, hits = str(tmp_path / "py.tsv"), str(tmp_path / "cli.tsv"), str(tmp_path / "hits.txt")
    extra = ["--scores", mpath, "--top", "5", "--counts"]
    subprocess.run([sys.executable, "-m", "calitas_amd", "SearchReference", "-o", py_out] + extra + flags, check=True, env=env, cwd=ROOT, timeout=300)
    subprocess.run([os.path.join(ROOT, "calitas_amd", "calitas"), "SearchReference", "-o", cli_out] + extra + flags, check=True, timeout=300)
    subprocess.run([sys.executable, "-m", "calitas_amd", "SearchReference", "-o", hits] + flags, check=True, env=env, cwd=ROOT, timeout=300)
    text = open(py_out).read()
    assert text == open(cli_out).read()
    shape = (2, 5, 7, 2)
    want = C.top_of_rows(C.read_hits(hits), model, 5, shape)
    assert len(want.hits) == 5 and want.scores.perfect > 0
    assert text == C.scores_tsv("g1", want.scores) + "\n" + C.top_tsv("g1", want) + "\n" + C.counts_tsv("g1", want.scores.table)
    sections = text.split("\n\n")
    assert len(sections) == 3
    lines = [ln.split("\t") for ln in sections[1].splitlines()]
    assert lines[0][:3] == ["guide_id", "rank", "chromosome"] and [int(f[1]) for f in lines[1:]] == [1, 2, 3, 4, 5]
    back = [C.TopHit(int(f[9]), f[2], int(f[3]), int(f[4]), f[5], int(f[6]), int(f[7]), int(f[8])) for f in lines[1:]]
    assert back == want.hits
    # --top without --scores is refused by both tools
    assert subprocess.run([os.path.join(ROOT, "calitas_amd", "calitas"), "SearchReference", "--top", "5"] + flags, timeout=300).returncode == 2
    assert subprocess.run([sys.executable, "-m", "calitas_amd", "SearchReference", "--top", "5"] + flags, env=env, cwd=ROOT, timeout=300).returncode == 2
