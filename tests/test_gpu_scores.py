"""GPU: the specificity score of calitas_search_scores / calitas_search_scores_batch (scores_kernel in hits.hip, bin_scores_kernel in
binned.hip, the host stage behind them) against scores_of_rows -- the contract in plain Python integers -- of the text the same call
returns through calitas_search_hits, on every path a call can take; against the oracle's rows for the parameter shapes; as sums over
window ranges; through the guide batch; and through the two command-line tools.  Every comparison is equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fasta_util import write_fasta
from parity_util import oracle_rows, synth_fasta
from scores_util import distinct_model, plant_edge_cases
from test_gpu_counts import ENV_PATHS, GUIDE, SHAPES, STEP, genome, ranges_genome

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


def edge_genome(C, tmp_path):
    """test_gpu_counts' plain genome with the plantings of the host tests written into contig k0: target letters Y, R, U and N under
    the guide, a site 3 bases from the contig's start and one on the minus strand at its very end."""
    fa, lengths = genome(tmp_path, crowded=False)
    contigs = [(n, s.decode()) for n, s in C.read_fasta(fa).items()]
    assert contigs[0][0] == "k0"
    contigs[0] = ("k0", plant_edge_cases(contigs[0][1]))
    return write_fasta(str(tmp_path / "edge.fa"), contigs), lengths


def text_scores(C, ctx, G, params, model, shape):
    text, n = ctx.search_hits(G, "a", params, "v0", "stamp")
    rows = C.read_hits(text)
    assert len(rows) == n
    return C.scores_of_rows(rows, model, shape), rows


def test_every_path_gives_the_score_of_the_text(C, tmp_path, monkeypatch):
    """search_scores == scores_of_rows(read_hits(search_hits text)) and its table == search_counts on the per-bin kernels, the general
    kernels, the wave-per-bin kernel, three ranges and one, the host stages, one pass per contig and -O 0."""
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
            got = ctx.search_scores(G, params, model)
            tm = ctx.timing()
            assert got.table.dtype == np.uint64 and got.table.shape == (2, 6, 8, 2), name
            want, rows = text_scores(C, ctx, G, params, model, got.table.shape)
            print(name, got, "want", want, "binned_lanes", tm["binned_lanes"], "lanes", tm["lanes"], "passes", tm["contig_passes"])
            assert (got.rows, got.perfect, got.sum_q32, got.max_q32) == (want.rows, want.perfect, want.sum_q32, want.max_q32), name
            assert got == want, name
            assert np.array_equal(got.table, ctx.search_counts(G, params)), name
            assert tm["hit_rows"] == got.rows == int(got.table.sum()) and tm["hits_bytes"] == 0, name
            if name == "default":
                assert tm["binned_lanes"] > 0
                first = got
                assert got.rows > 92 and got.perfect >= 16 + 3 and got.sum_q32 > 0 and 0 < got.max_q32 < 1 << 32
                assert {r["strand"] for r in rows} == {"+", "-"}
                # the planted letters reached the rows: Y on both strands, U, N (paired as '|': a perfect hit), both contig ends
                k0 = {(int(r["coordinate_start"]), r["strand"]): r for r in rows if r["chromosome"] == "k0"}
                assert k0[(1000, "+")]["padded_target"][3] == "Y" == k0[(3003, "-")]["padded_target"][3]
                assert k0[(5000, "+")]["padded_target"][0] == "U" and k0[(7000, "+")]["padded_target"][7] == "N"
                assert (3, "+") in k0 and any(s == "-" and p > 33000 for p, s in k0)
                assert got == C.scores_of_rows(oracle_rows(fa, GUIDE, g=2), model, got.table.shape)
            if name in ("general", "host-hits"):
                assert tm["binned_lanes"] == 0
            if name == "three-ranges":
                assert tm["lanes"] == 3
            if name == "per-contig":
                assert tm["contig_passes"] == 5
            assert got == first, name
            for k in env:
                monkeypatch.delenv(k)
        p0 = C.make_params(max_gaps_between_guide_and_pam=2, max_overlap=0)     # -O 0: no device row stage, the host stage scores
        got = ctx.search_scores(G, p0, model)
        want, _ = text_scores(C, ctx, G, p0, model, got.table.shape)
        print("-O 0", got)
        assert got == want and got.rows > 0
        # the U2 reading: the N column is '.', scored through index 4 -- one perfect hit less, on the device and in the text
        pu = C.make_params(max_gaps_between_guide_and_pam=2, eqx_by_score=1)
        got = ctx.search_scores(G, pu, model)
        want, _ = text_scores(C, ctx, G, pu, model, got.table.shape)
        print("eqx_by_score", got)
        assert got == want and got.perfect == first.perfect - 1
    finally:
        ctx.close()


def test_crowded_bin_the_general_tail_finishes(C, tmp_path, monkeypatch):
    """A bin with more alignments than its wave holds: the per-bin kernels decline and the general kernels finish in score mode; the
    second call goes there at once."""
    fa, _ = genome(tmp_path, crowded=True)
    G = C.Guide(GUIDE)
    model = distinct_model(C, 20)
    params = C.make_params(max_gaps_between_guide_and_pam=2)
    for env in ({}, {"CALITAS_CHUNKS": "2"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = C.Context(0)                    # (a fresh context: the decline is found, not remembered)
        ctx.set_reference_fasta(fa)
        try:
            got = ctx.search_scores(G, params, model)
            tm = ctx.timing()
            want, _ = text_scores(C, ctx, G, params, model, got.table.shape)
            print("crowded", env, got, "binned_lanes", tm["binned_lanes"], "lanes", tm["lanes"])
            assert got == want and got.rows > 150 and got.perfect > 100
            assert tm["binned_lanes"] < tm["lanes"]          # a range finished on the general kernels
            assert ctx.search_scores(G, params, model) == want
        finally:
            ctx.close()
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("cfg", SHAPES, ids=lambda c: c[0])
def test_parameter_shapes_against_the_oracle(C, cfg, tmp_path, monkeypatch):
    cid, guide, aux, kw, lengths, shape = cfg
    step = 1000 - (len(guide) + kw.get("d", 5) + kw.get("g", 3) - 1)
    fa = synth_fasta(tmp_path, 31 + len(cid), [guide], lengths=lengths, step_hint=step)
    pk = dict(max_guide_diffs=kw.get("d", 5), max_pam_mismatches=kw.get("p", 1), max_gaps_between_guide_and_pam=kw.get("g", 3),
              eqx_by_score=(1 if kw.get("switches", 0) & 2 else 0) | (2 if kw.get("switches", 0) & 1 else 0))
    pk.update({k: v for k, v in kw.items() if k.endswith("_net_cost")})
    G = C.Guide(guide, aux)
    model = distinct_model(C, G.protospacer_length, seed=len(cid))
    want_rows = oracle_rows(fa, guide, aux, **kw)
    want = C.scores_of_rows(want_rows, model, shape)
    with_gaps = sum(1 for r in want_rows if int(r["guide_gaps"]) > 0)
    print(cid, want, "rows with gaps", with_gaps, "minus", sum(1 for r in want_rows if r["strand"] == "-"))
    assert 6 <= want.perfect <= 8 and 18 <= with_gaps <= 755
    if cid == "iupac-protospacer":          # '.' columns under a guide letter outside ACGT: guide index 4
        assert any(a == "." and g in "NR" for r in want_rows for g, a in zip(r["padded_guide"], r["padded_alignment"]))
    if cid == "5prime-tttv":                # the reversed orientation
        assert (len(want_rows), sum(1 for r in want_rows if r["strand"] == "-")) == (47, 26)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        for env in ({}, {"CALITAS_BINNED": "0"}, {"CALITAS_HOST_HITS": "1"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got = ctx.search_scores(G, C.make_params(**pk), model)
            print(cid, env, got, "binned_lanes", ctx.timing()["binned_lanes"])
            assert got.table.shape == shape, (cid, env)
            assert (got.rows, got.perfect, got.sum_q32, got.max_q32) == (want.rows, want.perfect, want.sum_q32, want.max_q32), (cid, env)
            assert got == want, (cid, env)
            for k in env:
                monkeypatch.delenv(k)
    finally:
        ctx.close()


@pytest.mark.parametrize("cuts", [2, 3, 8])
def test_window_ranges_add_up(C, tmp_path, monkeypatch, cuts):
    """The scores of consecutive window ranges add up to the whole call's -- rows, perfect, sum_q32 and the table add, max_q32 is the
    maximum of the pieces -- and each is the score of the rows calitas_search_hits returns for that range: on the per-bin kernels,
    where a crowded bin hands a stretch to the general kernels, through the whole-contig fallback (which scores from the rows'
    columns), and with the range cut once more into lanes."""
    from calitas_amd import shard
    fa, lengths = ranges_genome(tmp_path, np.random.default_rng(100 + cuts))
    G = C.Guide(GUIDE)
    model = distinct_model(C, 20)
    pk = dict(max_gaps_between_guide_and_pam=2)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        whole = ctx.search_scores(G, C.make_params(**pk), model)
        want, _ = text_scores(C, ctx, G, C.make_params(**pk), model, whole.table.shape)
        assert whole == want and whole.rows > 60 and whole.perfect > 0 and whole.sum_q32 > 0
        parts = shard.window_partition(lengths, cuts, STEP)
        assert len(parts) == cuts
        own_general = 0
        for mode, env in (("default", {}), ("two lanes", {"CALITAS_CHUNKS": "2"}), ("general", {"CALITAS_BINNED": "0"}),
                          ("whole contigs", {"CALITAS_OWN_GENERAL_OFF": "1"})):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            total = None
            for first, n in parts:
                pr = C.make_params(first_window=first, n_windows=n, **pk)
                got = ctx.search_scores(G, pr, model)
                tm = ctx.timing()
                if mode == "default":
                    own_general += tm["owned_general_lanes"]
                piece, _ = text_scores(C, ctx, G, pr, model, whole.table.shape)
                assert got == piece, (mode, first, n)
                assert tm["hit_rows"] == got.rows and tm["hits_bytes"] == 0
                total = got if total is None else total + got
            print(cuts, mode, "sum", total, "whole", whole, "owned_general_lanes so far", own_general)
            assert total == whole, mode
            for k in env:
                monkeypatch.delenv(k)
        assert own_general >= 1               # the stretch with contig c's crowded bin: the general kernels, owned rows only
    finally:
        ctx.close()


def test_batches(C, tmp_path, monkeypatch):
    """search_scores_batch of 6 guides equals 6 single calls: whole reference and a window range, five lanes (default), one and three;
    a batch of mixed lengths is refused."""
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
            single = [ctx.search_scores(g, params, model) for g in G]
            texts = [text_scores(C, ctx, g, params, model, single[0].table.shape)[0] for g in G]
            assert all(s == t for s, t in zip(single, texts))
            assert sum(s.rows for s in single) > (100 if "first_window" not in pk else 10) and sum(s.sum_q32 for s in single) > 0
            for lanes in (None, "1", "3"):
                if lanes:
                    monkeypatch.setenv("CALITAS_BATCH_LANES", lanes)
                got = ctx.search_scores_batch(G, params, model)
                tm = ctx.timing()
                print("batch", pk.get("first_window"), lanes, got, "binned_lanes", tm["binned_lanes"])
                assert len(got) == 6 and all(a == b for a, b in zip(got, single)), (pk, lanes)
                if lanes != "1":
                    assert tm["hit_rows"] == sum(s.rows for s in single) and tm["hits_bytes"] == 0
                if lanes:
                    monkeypatch.delenv("CALITAS_BATCH_LANES")
        with pytest.raises(C.CalitasError):
            ctx.search_scores_batch([G[0], C.Guide("GTGACTTGAAGTCTCAGTATAnrg")], C.make_params(), model)
        with pytest.raises(C.CalitasError):
            ctx.search_scores(G[0], C.make_params(), distinct_model(C, 21))
    finally:
        ctx.close()


def test_scores_flag_end_to_end(C, tmp_path):
    """`python -m calitas_amd SearchReference --scores m.tsv` and `calitas SearchReference --scores m.tsv` write the same bytes, and
    they are the score of the hits.txt the same flags give without it; `FindGuides --scores m.tsv` adds perfect and specificity, equal to
    single search_scores calls."""
    fa, _ = edge_genome(C, tmp_path)
    model = distinct_model(C, 20)
    mpath = str(tmp_path / "m.tsv")
    model.write(mpath)
    flags = ["-i", GUIDE, "-I", "g1", "-r", fa, "-g", "2", "-d", "4"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    py_out, cli_out, hits = str(tmp_path / "py.tsv"), str(tmp_path / "cli.tsv"), str(tmp_path / "hits.txt")
    subprocess.run([sys.executable, "-m", "calitas_amd", "SearchReference", "--scores", mpath, "-o", py_out] + flags, check=True, env=env, cwd=ROOT, timeout=300)
    subprocess.run([os.path.join(ROOT, "calitas_amd", "calitas"), "SearchReference", "--scores", mpath, "-o", cli_out] + flags, check=True, timeout=300)
    subprocess.run([sys.executable, "-m", "calitas_amd", "SearchReference", "-o", hits] + flags, check=True, env=env, cwd=ROOT, timeout=300)
    assert open(py_out).read() == open(cli_out).read()
    want = C.scores_of_rows(C.read_hits(hits), model)
    assert want.rows > 40 and want.perfect > 0 and want.sum_q32 > 0
    assert open(py_out).read() == C.scores_tsv("g1", want)
    # --scores with --counts: the table of the same pass behind an empty line, the same bytes from both tools
    subprocess.run([os.path.join(ROOT, "calitas_amd", "calitas"), "SearchReference", "--scores", mpath, "--counts", "-o", cli_out] + flags, check=True, timeout=300)
    shape = (2, 5, 7, 2)
    assert open(cli_out).read() == C.scores_tsv("g1", want) + "\n" + C.counts_tsv("g1", C.counts_of_rows(C.read_hits(hits), shape))
    # FindGuides --scores on a 20-kb region
    out = str(tmp_path / "guides.tsv")
    pattern = "N" * 20 + "ngg"
    subprocess.run([sys.executable, "-m", "calitas_amd", "FindGuides", "-i", pattern, "-r", fa, "-c", "k1", "-s", "0", "-e", "20000", "-o", out,
                    "--scores", mpath, "-d", "2", "-g", "1"], check=True, env=env, cwd=ROOT, timeout=300)
    lines = [ln.split("\t") for ln in open(out).read().splitlines()]
    head = lines[0]
    assert head[8:] == ["hits", "hits_mm0", "hits_mm1", "hits_mm2", "perfect", "specificity"] and len(lines) > 100
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        params = C.make_params(max_guide_diffs=2, max_gaps_between_guide_and_pam=1)
        for f in (lines[1], lines[len(lines) // 2], lines[-1]):
            row = dict(zip(head, f))
            s = ctx.search_scores(C.Guide(row["guide"]), params, model)
            assert (int(row["hits"]), int(row["perfect"]), row["specificity"]) == (s.rows, s.perfect, "%.6f" % s.specificity)
            assert [int(row["hits_mm%d" % m]) for m in range(3)] == [int(s.table[:, m].sum()) for m in range(3)]
            assert s.perfect >= 1                               # the guide's own site
    finally:
        ctx.close()
