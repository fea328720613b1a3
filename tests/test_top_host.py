"""CPU tests of the top list (calitas_hits_top, top_of_rows, Top.merge, the top TSV): no GPU.

The contract is top_of_rows: score_of_row per hits.txt row, perfect rows dropped, a stable sort by descending score.  The host stage is
fed the ORACLE's per-window alignments (the recipe of test_scores_host) and held against top_of_rows of the text the product's own
hits_tsv stage writes for the same alignments, and of the oracle's rows.  Every comparison is an equality of Top objects."""
import numpy as np
import pytest

import oracle_lib as O
from fasta_util import write_fasta
from scores_util import GUIDE, distinct_model, plant_edge_cases
from test_counts_host import GUIDES, _genome
from test_host_logic import _oracle_alignments

GUIDE_5P = "cttGCCCCACAGGGCAGTAATGG"      # the planted site read as PAM + protospacer: a 5' PAM guide on the same plantings
SKIP = ("aligner_version", "time_stamp")


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


def _uniform(C, L=20):
    return C.ScoreModel.uniform(L, mismatch=32768, gap=16384, pam_mismatch=49152)


@pytest.fixture(scope="module")
def edge(C, tmp_path_factory):
    """The plant_edge_cases contig: (fasta, {guide: (Guide, alignments of the oracle)})"""
    rng = np.random.default_rng(99)
    seq = plant_edge_cases(rng.choice(list(b"ACGT"), size=12000).astype(np.uint8).tobytes().decode())
    fa = write_fasta(str(tmp_path_factory.mktemp("top_edge") / "edge.fa"), [("e0", seq)])
    return fa, {g: (C.Guide(g), _oracle_alignments(C, g, "e0", 0, seq, dict(d=3, p=1, g=2, D=6, O=10))) for g in (GUIDE, GUIDE_5P)}


@pytest.fixture(scope="module")
def synth_rows(C, tmp_path_factory):
    """The genome of test_counts_host for its 3' PAM guide: (Guide, fasta, alignments of the oracle, the oracle's rows, params)"""
    guide = GUIDES[0]
    G, contigs, fa = _genome(C, guide, tmp_path_factory.mktemp("top_synth"))
    alns = []
    for ci, (n, s) in enumerate(contigs):
        alns += _oracle_alignments(C, guide, n, ci, s, dict(d=4, p=1, g=2, D=7, O=10))
    _, want, _ = O.search_reference(fa, guide, "a", d=4, p=1, g=2, D=7)
    params = C.make_params(max_guide_diffs=4, max_pam_mismatches=1, max_gaps_between_guide_and_pam=2, max_total_diffs=7)
    return G, fa, alns, want, params


@pytest.mark.parametrize("guide", [GUIDE, GUIDE_5P], ids=["pam3", "pam5"])
def test_hits_top_equals_top_of_rows_of_the_text(C, edge, guide):
    """hits_top == top_of_rows(read_hits(hits_tsv text)) for k = 1, 3 and 256 under distinct_model, on the plantings with target letters
    outside ACGT, both strands and both contig ends, for a 3' PAM and a 5' PAM guide; .scores == hits_scores."""
    fa, by_guide = edge
    G, alns = by_guide[guide]
    model = distinct_model(C, 20)
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    try:
        params = C.make_params(max_guide_diffs=3, max_pam_mismatches=1, max_gaps_between_guide_and_pam=2)
        text, n_rows = ctx.hits_tsv(G, "a", params, alns)
        rows = C.read_hits(text)
        scores = ctx.hits_scores(G, params, model, alns)
        imperfect = [r for r in rows if C.score_of_row(r, model) is not None]
        print(guide, "rows", len(rows), "imperfect", len(imperfect), [(r["coordinate_start"], r["strand"]) for r in imperfect])
        assert n_rows == len(rows) and len(imperfect) >= 3 and {r["strand"] for r in imperfect} == {"+", "-"}
        assert len(imperfect) < len(rows)                        # perfect rows exist, and are never listed
        assert G.pam_is_five_prime == (guide == GUIDE_5P)
        for k in (1, 3, 256):
            got = ctx.hits_top(G, params, model, k, alns)
            want = C.top_of_rows(rows, model, k, scores.table.shape)
            assert got == want, (k, got.hits, want.hits)
            assert got.scores == scores and got.k == k and len(got.hits) == min(k, len(imperfect))
            assert [h.score_q32 for h in got.hits] == sorted((h.score_q32 for h in got.hits), reverse=True)
    finally:
        ctx.close()


def test_hits_top_on_the_oracles_rows_with_gaps(C, synth_rows):
    """The same against the ORACLE's rows (27 rows, 4 perfect, 22 with gaps, two contigs): chromosome names, gaps and PAM mismatches in
    the records."""
    G, fa, alns, want, params = synth_rows
    model = distinct_model(C, G.protospacer_length)
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    try:
        shape = ctx.hits_counts(G, params, alns).shape
        assert len(want) == 27 and {r["chromosome"] for r in want} == {"chrA", "chrB"}
        for k in (1, 5, 23, 256):
            got = ctx.hits_top(G, params, model, k, alns)
            expect = C.top_of_rows(want, model, k, shape)
            assert got == expect, k
        assert len(got.hits) == 23 and any(h.guide_gaps for h in got.hits) and any(h.pam_mm for h in got.hits)
        assert {h.chromosome for h in got.hits} == {"chrA", "chrB"}
    finally:
        ctx.close()


def _tie_k(hits):
    """A k such that the k-th and the (k+1)-th of the expected order have equal scores (1-based k)."""
    for i in range(1, len(hits)):
        if hits[i - 1].score_q32 == hits[i].score_q32:
            return i
    raise AssertionError("no two candidates with equal scores")


def test_ties_keep_the_order_of_the_text(C, synth_rows):
    """A uniform model with factors below 1 scores many rows alike: at a k that cuts between two equal scores the list ends with the row
    that comes earlier in the text."""
    G, fa, alns, want, params = synth_rows
    model = _uniform(C, G.protospacer_length)
    everything = C.top_of_rows(want, model, 256)
    k = _tie_k(everything.hits)
    assert everything.hits[k - 1].score_q32 == everything.hits[k].score_q32 and everything.hits[k - 1] != everything.hits[k]
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    try:
        shape = ctx.hits_counts(G, params, alns).shape
        for kk in (k, k + 1, 256):
            assert ctx.hits_top(G, params, model, kk, alns) == C.top_of_rows(want, model, kk, shape), kk
        got = ctx.hits_top(G, params, model, k, alns)
        assert got.hits == everything.hits[:k] and got.hits[-1] == everything.hits[k - 1]
    finally:
        ctx.close()


def test_list_shorter_than_k(C, synth_rows):
    G, fa, alns, want, params = synth_rows
    model = distinct_model(C, G.protospacer_length)
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    try:
        got = ctx.hits_top(G, params, model, 100, alns)
        assert got.scores.rows - got.scores.perfect == 23 < 100
        assert len(got.hits) == got.scores.rows - got.scores.perfect
        assert all(h.guide_mm + h.guide_gaps + h.pam_mm > 0 for h in got.hits)
        assert got == C.top_of_rows(want, model, 100, got.scores.table.shape)
    finally:
        ctx.close()


def test_merge_of_pieces_in_order(C, synth_rows):
    """top_of_rows of the rows cut at three places, merged in order, is top_of_rows of all rows; merged out of order it is not, where
    equal scores sit in different pieces: the order of the pieces is part of the contract."""
    G, fa, alns, want, params = synth_rows
    for model in (distinct_model(C, G.protospacer_length), _uniform(C, G.protospacer_length)):
        for k in (1, 4, 9, 256):
            whole = C.top_of_rows(want, model, k)
            for cuts in ((5, 11, 20), (1, 2, 26), (9, 9, 18)):
                a, b, c = cuts
                pieces = [C.top_of_rows(p, model, k) for p in (want[:a], want[a:b], want[b:c], want[c:])]
                assert pieces[0].merge(*pieces[1:]) == whole, (k, cuts)
    model = _uniform(C, G.protospacer_length)
    everything = C.top_of_rows(want, model, 256)
    k = _tie_k(everything.hits)
    first, second = everything.hits[k - 1], everything.hits[k]          # equal scores; `first` comes earlier in the text
    keys = [(r["chromosome"], int(r["coordinate_start"]), r["strand"]) for r in want]
    cut = keys.index((second.chromosome, second.coordinate_start, second.strand))
    assert keys.index((first.chromosome, first.coordinate_start, first.strand)) < cut
    lo, hi = C.top_of_rows(want[:cut], model, k), C.top_of_rows(want[cut:], model, k)
    whole = C.top_of_rows(want, model, k)
    assert lo.merge(hi) == whole
    assert hi.merge(lo) != whole and hi.merge(lo).scores == whole.scores
    with pytest.raises(ValueError):
        lo.merge(C.top_of_rows(want[cut:], model, k + 1))


def test_errors(C, edge):
    fa, by_guide = edge
    G, alns = by_guide[GUIDE]
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    try:
        params = C.make_params(max_guide_diffs=3, max_pam_mismatches=1, max_gaps_between_guide_and_pam=2)
        model = distinct_model(C, 20)
        assert len(ctx.hits_top(G, params, model, 256, alns).hits) == 3
        for k in (0, 257):
            with pytest.raises(C.CalitasError) as e:
                ctx.hits_top(G, params, model, k, alns)
            assert e.value.code == C._lib.EINVAL, k
        with pytest.raises(C.CalitasError) as e:
            ctx.hits_top(G, params, distinct_model(C, 21), 5, alns)
        assert e.value.code == C._lib.EINVAL
        for k in (0, 257):
            with pytest.raises(ValueError):
                C.top_of_rows([], model, k)
    finally:
        ctx.close()


def test_top_tsv_and_the_flag(C, synth_rows, tmp_path, monkeypatch):
    """top_tsv writes guide_id rank chromosome coordinate_start coordinate_end strand guide_mm guide_gaps pam_mm score_q32 score, one
    line per record; `SearchReference --scores MODEL --top K [--counts]` writes scores TSV, empty line, top TSV[, empty line, counts
    TSV]; --top without --scores and with --variants is refused.  No GPU here: the search behind SearchReference.scores() is replaced
    by the host stage (tests/test_gpu_top.py runs the flag end to end on the device)."""
    from calitas_amd import __main__ as M
    from calitas_amd import aligner
    G, fa, alns, want, params = synth_rows
    model = distinct_model(C, G.protospacer_length)
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    try:
        top = ctx.hits_top(G, params, model, 5, alns)
    finally:
        ctx.close()
    text = C.top_tsv("g7", top)
    lines = text.split("\n")
    assert lines[0].split("\t") == ["guide_id", "rank", "chromosome", "coordinate_start", "coordinate_end", "strand", "guide_mm", "guide_gaps",
                                    "pam_mm", "score_q32", "score"]
    assert len(lines) == 7 and lines[6] == ""
    for i, (ln, h) in enumerate(zip(lines[1:6], top.hits)):
        assert ln.split("\t") == ["g7", str(i + 1), h.chromosome, str(h.coordinate_start), str(h.coordinate_end), h.strand, str(h.guide_mm),
                                  str(h.guide_gaps), str(h.pam_mm), str(h.score_q32), "%.6f" % (h.score_q32 / 2.0 ** 32)]
    mpath = str(tmp_path / "model.tsv")
    model.write(mpath)
    seen = {}

    def fake_top(self, m, k):
        seen["top"] = k
        return top
    monkeypatch.setattr(aligner.SearchReference, "top", fake_top)
    monkeypatch.setattr(aligner.SearchReference, "scores", lambda self, m: top.scores)
    out = tmp_path / "top.tsv"
    flags = ["SearchReference", "-i", GUIDES[0], "-I", "g7", "-r", "unused.fa", "-o", str(out), "-d", "4", "-p", "1", "-g", "2", "-D", "7"]
    assert M.main(flags + ["--scores", mpath, "--top", "5"]) == 0 and seen["top"] == 5
    assert out.read_text() == C.scores_tsv("g7", top.scores) + "\n" + text
    assert M.main(flags + ["--scores", mpath, "--top", "5", "--counts"]) == 0
    assert out.read_text() == C.scores_tsv("g7", top.scores) + "\n" + text + "\n" + C.counts_tsv("g7", top.scores.table)
    with pytest.raises(SystemExit):
        M.main(flags + ["--top", "5"])
    with pytest.raises(SystemExit):
        M.main(flags + ["--scores", mpath, "--top", "5", "-v", "some.vcf"])
