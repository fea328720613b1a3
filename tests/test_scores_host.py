"""CPU tests of the specificity score (calitas_hits_scores, scores_of_rows, ScoreModel and its file, the --scores TSV): no GPU.

The contract is scores_of_rows: plain Python integers on hits.txt rows.  The host stage is fed the ORACLE's per-window alignments (the
recipe of test_counts_host._host_counts) and held against scores_of_rows of the oracle's own rows -- a text-based route to the same
integers.  Every comparison is equality."""
import numpy as np
import pytest

import oracle_lib as O
from fasta_util import write_fasta
from scores_util import GUIDE, SITE, distinct_model, plant_edge_cases
from test_counts_host import GUIDES, _genome
from test_host_logic import _oracle_alignments

ORACLE_ROWS_PERFECT = {GUIDES[0]: (27, 4), GUIDES[1]: (31, 3), GUIDES[2]: (30, 3)}
ORACLE_ROWS_WITH_GAPS = {GUIDES[0]: 22, GUIDES[1]: 23, GUIDES[2]: 21}


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


def _row(pg, pa, pt, total, gaps, pam_mm):
    return {"padded_guide": pg, "padded_alignment": pa, "padded_target": pt, "total_mm_plus_gaps": str(total), "guide_gaps": str(gaps),
            "pam_mm": str(pam_mm), "strand": "+", "guide_mm": "2"}


def test_scores_of_rows_by_hand(C):
    """Every mismatch 0.5, gap 0.25, pam_mismatch 0.75: two '.' columns under upper-case letters, one guide gap and one PAM mismatch
    give 2^32 * 0.5 * 0.5 * 0.25 * 0.75 = 201326592; a row without an edit is perfect, not scored; a row whose upper-case letters are
    not the model's length is an error."""
    m = C.ScoreModel.uniform(20, mismatch=32768, gap=16384, pam_mismatch=49152)
    hit = _row("CTTGCCCCAC-AGGGCAGTAAnrg", "|.||||||||~|||.|||||||.|", "CATGCCCCACTAGGTCAGTAATCG", 4, 1, 1)
    perfect = _row("CTTGCCCCACAGGGCAGTAAnrg", "|||||||||||||||||||||||", "CTTGCCCCACAGGGCAGTAATGG", 0, 0, 0)
    assert C.score_of_row(hit, m) == 201326592 == (1 << 32) // 2 // 2 // 4 * 3 // 4
    got = C.scores_of_rows([hit, perfect, hit], m)
    assert (got.rows, got.perfect, got.sum_q32, got.max_q32) == (3, 1, 2 * 201326592, 201326592)
    assert got.offtarget_sum == 2 * 201326592 / 2.0 ** 32 and got.specificity == 2.0 ** 32 / (2.0 ** 32 + 2 * 201326592)
    only_perfect = C.scores_of_rows([perfect], m)
    assert (only_perfect.perfect, only_perfect.sum_q32, only_perfect.max_q32, only_perfect.specificity) == (1, 0, 0, 1.0)
    # a '.' under a lower-case letter (the PAM) is not a mismatch factor: it is counted by pam_mm alone
    assert C.score_of_row(_row("CTTGCCCCACAGGGCAGTAAnrg", "|||||||||||||||||||||.|", "CTTGCCCCACAGGGCAGTAATCG", 1, 0, 1), m) == 49152 << 16
    with pytest.raises(ValueError):
        C.scores_of_rows([_row("CTTGCCCCACAGGGCAGTAnrg", "||||||||||||||||||||||", "CTTGCCCCACAGGGCAGTATGG", 0, 0, 0)], m)
    with pytest.raises(ValueError):
        C.scores_of_rows([hit], C.ScoreModel.uniform(21, mismatch=32768))


def _host_scores(C, guide, tmp_path):
    """(ctx.hits_scores on the oracle's alignments, ctx.hits_counts on the same, the oracle's hits.txt rows, the model)"""
    G, contigs, fa = _genome(C, guide, tmp_path)
    kw = dict(d=4, p=1, g=2, D=7, O=10)
    alns = []
    for ci, (n, s) in enumerate(contigs):
        alns += _oracle_alignments(C, guide, n, ci, s, kw)
    model = distinct_model(C, G.protospacer_length)
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    params = C.make_params(max_guide_diffs=4, max_pam_mismatches=1, max_gaps_between_guide_and_pam=2, max_total_diffs=7)
    got = ctx.hits_scores(G, params, model, alns)
    table = ctx.hits_counts(G, params, alns)
    _, want, _ = O.search_reference(fa, guide, "a", d=4, p=1, g=2, D=7)
    ctx.close()
    return got, table, want, model


@pytest.mark.parametrize("guide", GUIDES)
def test_hits_scores_stage_matches_oracle(C, guide, tmp_path):
    """removeOverlaps + table + score (product host code, from ops and packed bases) on the oracle's per-window alignments must give
    scores_of_rows of the oracle's hits.txt: a 3' PAM guide, a 5' PAM guide (reversed orientation), a PAM-less guide."""
    got, table, want, model = _host_scores(C, guide, tmp_path)
    expect = C.scores_of_rows(want, model, table.shape)
    with_gaps = sum(1 for r in want if int(r["guide_gaps"]) > 0)
    print(guide, "rows", expect.rows, "perfect", expect.perfect, "with gaps", with_gaps, "sum", expect.sum_q32, "max", expect.max_q32)
    assert (expect.rows, expect.perfect) == ORACLE_ROWS_PERFECT[guide] and with_gaps == ORACLE_ROWS_WITH_GAPS[guide]
    assert {r["strand"] for r in want} == {"+", "-"}
    assert (got.rows, got.perfect, got.sum_q32, got.max_q32) == (expect.rows, expect.perfect, expect.sum_q32, expect.max_q32)
    assert got == expect and np.array_equal(got.table, table)
    assert got.sum_q32 > 0 and 0 < got.max_q32 <= got.sum_q32 and 0.0 < got.specificity < 1.0


def _edge_contig():
    rng = np.random.default_rng(99)
    return plant_edge_cases(rng.choice(list(b"ACGT"), size=12000).astype(np.uint8).tobytes().decode())


@pytest.mark.parametrize("u2", [False, True], ids=["default", "eqx-by-score"])
def test_letters_outside_acgt_contig_edges_both_strands(C, tmp_path, monkeypatch, u2):
    """Target letters Y / R (both strands), U and N, and sites at both ends of the contig.  Default reading: N pairs as '|', so that
    site is perfect (4 of 7); with eqx_by_score bit 0 its column is '.', scored through index 4 (3 of 7)."""
    seq = _edge_contig()
    fa = write_fasta(str(tmp_path / "edge.fa"), [("e0", seq)])
    switches = 2 if u2 else 0                                   # (oracle bit 1 = ABI eqx_by_score bit 0)
    _, want, _ = O.search_reference(fa, GUIDE, "a", d=3, p=1, g=2, switches=switches)
    real_align = O.align
    monkeypatch.setattr(O, "align", lambda *a, **k: real_align(*a, **dict(k, switches=switches)))
    alns = _oracle_alignments(C, GUIDE, "e0", 0, seq, dict(d=3, p=1, g=2, D=6, O=10))
    G = C.Guide(GUIDE)
    model = distinct_model(C, 20)
    by_start = {(int(r["coordinate_start"]), r["strand"]): r for r in want}
    print(sorted(by_start), [r["total_mm_plus_gaps"] for r in want])
    assert len(want) == 7 and set(by_start) == {(3, "+"), (1000, "+"), (3003, "-"), (5000, "+"), (7000, "+"), (9000, "+"), (12000 - 20, "-")}
    y_plus, y_minus, u_row, n_row = by_start[(1000, "+")], by_start[(3003, "-")], by_start[(5000, "+")], by_start[(7000, "+")]
    for r in (y_plus, y_minus):
        assert (r["padded_guide"][3], r["padded_alignment"][3], r["padded_target"][3]) == ("G", ".", "Y")
    assert C.score_of_row(y_plus, model) == C.score_of_row(y_minus, model) == int(model.mismatch[3, 2, 4]) << 16
    assert (u_row["padded_alignment"][0], u_row["padded_target"][0]) == (".", "U")
    assert C.score_of_row(u_row, model) == int(model.mismatch[0, 1, 4]) << 16
    assert (n_row["padded_alignment"][7], n_row["padded_target"][7]) == ("." if u2 else "|", "N")
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    try:
        params = C.make_params(max_guide_diffs=3, max_pam_mismatches=1, max_gaps_between_guide_and_pam=2, eqx_by_score=1 if u2 else 0)
        got = ctx.hits_scores(G, params, model, alns)
        expect = C.scores_of_rows(want, model, got.table.shape)
        print("u2" if u2 else "default", got, expect)
        assert (expect.rows, expect.perfect) == (7, 3 if u2 else 4)
        assert got == expect
    finally:
        ctx.close()


def test_model_file_round_trip_and_refusals(C, tmp_path):
    model = distinct_model(C, 20, seed=11)
    path = str(tmp_path / "m.tsv")
    model.write(path)
    back = C.ScoreModel.read(path)
    assert back.L == 20 and np.array_equal(back.mismatch, model.mismatch) and (back.gap, back.pam_mismatch) == (model.gap, model.pam_mismatch)
    # `*` lines, overrides (later lines win), entries not given are 1.0, and the three conversions of the format's definition
    text = ("# a model\nlength\t20\ngap\t0.5\npam_mismatch\t1\n"
            "mismatch\t*\t*\t*\t0.25\nmismatch\t20\tG\t*\t0.0227\t# the PAM-proximal end\nmismatch\t20\tG\tT\t0.5\nmismatch\t1\tother\tA\t0\n"
            "gap\t0.0227\n")
    p2 = str(tmp_path / "star.tsv")
    open(p2, "w").write(text)
    m = C.ScoreModel.read(p2)
    assert (m.gap, m.pam_mismatch) == (1488, 65536)
    assert int(m.mismatch[5, 1, 2]) == 16384 and int(m.mismatch[19, 2, 0]) == 1488 and int(m.mismatch[19, 2, 4]) == 1488
    assert int(m.mismatch[19, 2, 3]) == 32768 and int(m.mismatch[0, 4, 0]) == 0 and int(m.mismatch[19, 1, 3]) == 16384
    open(p2, "w").write("length\t20\nmismatch\t3\tA\tC\t0.5\n")
    m = C.ScoreModel.read(p2)
    assert int(m.mismatch[2, 0, 1]) == 32768 and int((m.mismatch == 65536).sum()) == 20 * 25 - 1 and (m.gap, m.pam_mismatch) == (65536, 65536)
    for bad in ("length\t20\ngap\t1.5\n", "gap\t0.5\n", "length\t20\nmismatch\t21\tA\tC\t0.5\n", "length\t20\nmismatch\t2\tX\tC\t0.5\n",
                "length\t20\nweights\t1\n"):
        open(p2, "w").write(bad)
        with pytest.raises(ValueError):
            C.ScoreModel.read(p2)
    with pytest.raises(ValueError):
        C.ScoreModel(20, np.zeros((19, 5, 5)))
    # the library refuses a model of another length than the guide's, and a factor above 65536
    fa = write_fasta(str(tmp_path / "r.fa"), [("c", SITE * 10)])
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    try:
        params = C.make_params()
        assert ctx.hits_scores(C.Guide(GUIDE), params, model, []).rows == 0
        with pytest.raises(C.CalitasError) as e:
            ctx.hits_scores(C.Guide(GUIDE), params, distinct_model(C, 21), [])
        assert e.value.code == C._lib.EINVAL
        with pytest.raises(C.CalitasError):
            ctx.hits_scores(C.Guide("ACGTACATGCTCGATACGACGnrg"), params, model, [])
        for where in ("mismatch", "gap", "pam_mismatch"):
            mm = model.mismatch.copy()
            over = C.ScoreModel(20, mm, model.gap, model.pam_mismatch)
            if where == "mismatch":
                over.mismatch[19, 4, 4] = 65537
            else:
                setattr(over, where, 65537)
            with pytest.raises(C.CalitasError) as e:
                ctx.hits_scores(C.Guide(GUIDE), params, over, [])
            assert e.value.code == C._lib.EINVAL, where
        one = C.ScoreModel.uniform(20)                        # 65536 itself is 1.0: accepted
        assert ctx.hits_scores(C.Guide(GUIDE), params, one, []).sum_q32 == 0
    finally:
        ctx.close()


def test_scores_flag_writes_the_tsv(C, tmp_path, monkeypatch):
    """`python -m calitas_amd SearchReference --scores MODEL` writes the header guide_id rows perfect offtarget_sum_q32 max_q32
    specificity and one line; with --counts the table's TSV follows behind an empty line; with --variants it is refused.  No GPU here:
    the search behind SearchReference.scores() is replaced by the host stage on the oracle's alignments (tests/test_gpu_scores.py
    runs the flag end to end on the device)."""
    from calitas_amd import __main__ as M
    from calitas_amd import aligner
    guide = GUIDES[0]
    got, table, want, model = _host_scores(C, guide, tmp_path)
    mpath = str(tmp_path / "model.tsv")
    model.write(mpath)
    seen = {}

    def fake_scores(self, m):
        seen.update(self._kw, guide=self.guide_str, model=m)
        return got
    monkeypatch.setattr(aligner.SearchReference, "scores", fake_scores)
    out = tmp_path / "scores.tsv"
    flags = ["SearchReference", "-i", guide, "-I", "g7", "-r", "unused.fa", "-o", str(out), "-d", "4", "-p", "1", "-g", "2", "-D", "7"]
    assert M.main(flags + ["--scores", mpath]) == 0
    assert (seen["max_guide_diffs"], seen["max_total_diffs"]) == (4, 7) and np.array_equal(seen["model"].mismatch, model.mismatch)
    lines = out.read_text().split("\n")
    assert lines[0].split("\t") == ["guide_id", "rows", "perfect", "offtarget_sum_q32", "max_q32", "specificity"]
    assert len(lines) == 3 and lines[2] == ""
    f = lines[1].split("\t")
    expect = C.scores_of_rows(want, model)
    assert f[:5] == ["g7", str(expect.rows), str(expect.perfect), str(expect.sum_q32), str(expect.max_q32)]
    assert f[5] == "%.6f" % (2 ** 32 / (2 ** 32 + expect.sum_q32)) and 0.0 < float(f[5]) < 1.0
    assert M.main(flags + ["--scores", mpath, "--counts"]) == 0
    both = out.read_text()
    assert both == "\n".join(lines[:2]) + "\n\n" + C.counts_tsv("g7", table)
    with pytest.raises(SystemExit):
        M.main(flags + ["--scores", mpath, "-v", "some.vcf"])
