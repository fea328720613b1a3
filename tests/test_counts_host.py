"""CPU tests of the off-target table (calitas_hits_counts, counts_of_rows, the --counts TSV): no GPU.

The host stage is fed the ORACLE's per-window alignments and held against counts_of_rows of the oracle's own hits.txt, with the recipe
of test_host_logic.test_hits_tsv_stage_matches_oracle.  The oracle is the checker and the input generator only."""
import numpy as np
import pytest

import oracle_lib as O
from fasta_util import write_fasta
from test_host_logic import _oracle_alignments

GUIDES = ["CTTGCCCCACAGGGCAGTAAnrg", "tttvCTTGCCCCACAGGGCAGTAA", "CTTGCCCCACAGGGCAGTAA"]
# what the oracle alone gives for these inputs: rows and non-zero cells of the table
ORACLE_ROWS_CELLS = {"CTTGCCCCACAGGGCAGTAAnrg": (27, 18), "tttvCTTGCCCCACAGGGCAGTAA": (31, 19), "CTTGCCCCACAGGGCAGTAA": (30, 16)}


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


def _genome(C, guide, tmp_path, name="h.fa", seed=5, sizes=(("chrA", 30000), ("chrB", 12000))):
    from calitas_amd import synth
    G = C.Guide(guide)
    pam = G.pams[0] if G.pams else ""
    names, seqs = synth.make_genome(list(sizes), seed=seed, guides=[(G.guide, pam, G.pam_is_five_prime)],
                                    sites_per_guide=40, n_run_ends=150, n_block=1200, tandem_frac=0.05)
    contigs = [(n, s.tobytes().decode()) for n, s in zip(names, seqs)]
    return G, contigs, write_fasta(str(tmp_path / name), contigs)


def _host_counts(C, guide, tmp_path):
    """(table from ctx.hits_counts on the oracle's alignments, the oracle's hits.txt rows)"""
    G, contigs, fa = _genome(C, guide, tmp_path)
    kw = dict(d=4, p=1, g=2, D=7, O=10)
    alns = []
    for ci, (n, s) in enumerate(contigs):
        alns += _oracle_alignments(C, guide, n, ci, s, kw)
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    params = C.make_params(max_guide_diffs=4, max_pam_mismatches=1, max_gaps_between_guide_and_pam=2, max_total_diffs=7)
    table = ctx.hits_counts(G, params, alns)
    _, want, _ = O.search_reference(fa, guide, "a", d=4, p=1, g=2, D=7)
    ctx.close()
    return table, want


@pytest.mark.parametrize("guide", GUIDES)
def test_hits_counts_stage_matches_oracle(C, guide, tmp_path):
    """removeOverlaps + the table (product host code) on the oracle's per-window alignments must give counts_of_rows of the oracle's
    hits.txt, cell by cell."""
    table, want = _host_counts(C, guide, tmp_path)
    n_pam = 2 if C.Guide(guide).pams else 1
    assert table.dtype == np.uint64 and table.shape == (2, 5, 7, n_pam)          # d = 4, g = 2, p = 1 at the default costs
    expect = C.counts_of_rows(want, table.shape)
    print(guide, "rows", len(want), "non-zero cells", int(np.count_nonzero(expect)))
    assert (len(want), int(np.count_nonzero(expect))) == ORACLE_ROWS_CELLS[guide]
    assert np.array_equal(table, expect)
    assert int(table.sum()) == len(want)
    # not an all-in-one-cell table: many cells, both strands
    assert np.count_nonzero(table) >= 10
    assert table[0].sum() > 0 and table[1].sum() > 0
    if guide == GUIDES[0]:          # the 3' PAM guide reaches the corners: guide_mm 4, guide_gaps 4, pam_mm 1
        m, g, p = [int(x.max()) for x in np.nonzero(table)[1:]]
        assert (m, g, p) == (4, 4, 1)
    else:
        assert int(np.nonzero(table)[3].max()) == 0


def test_extents_do_not_depend_on_the_reference(C, tmp_path):
    """The same guide and params on two different genomes: the same shape (tables of contigs, ranges and ranks must add up)."""
    guide = GUIDES[0]
    params = C.make_params(max_guide_diffs=3, max_pam_mismatches=2, max_gaps_between_guide_and_pam=1)
    shapes = []
    for name, seed, sizes in (("a.fa", 5, (("chrA", 30000), ("chrB", 12000))), ("b.fa", 9, (("one", 5000),))):
        G, _, fa = _genome(C, guide, tmp_path, name, seed, sizes)
        ctx = C.Context(-1)
        ctx.set_reference_fasta(fa)
        shapes.append(ctx.hits_counts(G, params, []).shape)
        ctx.close()
    assert shapes[0] == shapes[1] == (2, 4, 5, 3)
    # ... and a PAM-less guide has no pam_mm axis to speak of, whatever -p says
    G, _, fa = _genome(C, GUIDES[2], tmp_path, "c.fa")
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    assert ctx.hits_counts(G, params, []).shape == (2, 4, 5, 1)
    ctx.close()


def test_extents_follow_the_edit_bound_with_custom_costs(C, tmp_path):
    """The least score a protospacer alignment may have is L * match + d * (the dearest edit); every edit takes at least the cheapest
    edit's cost off the all-match score, so an alignment can have up to d * dearest // cheapest edits -- more than -d when the costs differ.
    The extents must follow that bound, not -d."""
    guide = GUIDES[0]
    G, _, fa = _genome(C, guide, tmp_path)
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    d, g, p = 4, 2, 1
    for m, b, B in ((-120, -122, -121), (-120, -60, -121), (-100, -100, -40), (-200, -150, -100)):
        E = d * max(-m, -b, -B) // min(-m, -b, -B)
        params = C.make_params(max_guide_diffs=d, max_pam_mismatches=p, max_gaps_between_guide_and_pam=g, guide_mismatch_net_cost=m,
                               genome_gap_net_cost=b, guide_gap_net_cost=B)
        assert ctx.hits_counts(G, params, []).shape == (2, E + 1, E + g + 1, p + 1), (m, b, B)
    assert d * 122 // 60 > d            # (the second case does exceed -d)
    ctx.close()


def test_counts_of_rows_refuses_a_hit_outside_the_extents(C):
    row = {"strand": "-", "guide_mm": "2", "guide_gaps": "1", "pam_mm": "0"}
    t = C.counts_of_rows([row, row], (2, 3, 2, 1))
    assert t[1, 2, 1, 0] == 2 and t.sum() == 2
    with pytest.raises(ValueError):
        C.counts_of_rows([row], (2, 2, 2, 1))


def test_counts_flag_writes_the_tsv(C, tmp_path, monkeypatch):
    """`python -m calitas_amd SearchReference --counts` writes header guide_id strand guide_mm guide_gaps pam_mm hits and the non-zero
    cells in table order; parsed back it is the table.  No GPU here: the search behind SearchReference.counts() is replaced by the host
    stage on the oracle's alignments (tests/test_gpu_counts.py runs the flag end to end on the device)."""
    from calitas_amd import __main__ as M
    from calitas_amd import aligner
    guide = GUIDES[0]
    table, want = _host_counts(C, guide, tmp_path)
    seen = {}

    def fake_counts(self):
        seen.update(self._kw, guide=self.guide_str, ref=self.ref)
        return table
    monkeypatch.setattr(aligner.SearchReference, "counts", fake_counts)
    out = tmp_path / "counts.tsv"
    assert M.main(["SearchReference", "-i", guide, "-I", "g7", "-r", "unused.fa", "-o", str(out), "--counts", "-d", "4", "-p", "1", "-g", "2",
                   "-D", "7"]) == 0
    assert (seen["max_guide_diffs"], seen["max_pam_mismatches"], seen["max_gaps_between_guide_and_pam"], seen["max_total_diffs"]) == (4, 1, 2, 7)
    lines = out.read_text().splitlines()
    assert lines[0].split("\t") == ["guide_id", "strand", "guide_mm", "guide_gaps", "pam_mm", "hits"]
    assert len(lines) - 1 == np.count_nonzero(table)
    cells = [(0 if f[1] == "+" else 1, int(f[2]), int(f[3]), int(f[4])) for f in (ln.split("\t") for ln in lines[1:])]
    assert cells == sorted(cells) and all(ln.split("\t")[0] == "g7" for ln in lines[1:])      # table order, non-zero cells only
    assert all(int(ln.split("\t")[5]) > 0 for ln in lines[1:])
    back = C.read_counts_tsv(str(out), table.shape)
    assert np.array_equal(back, table) and np.array_equal(back, C.counts_of_rows(want, table.shape))
