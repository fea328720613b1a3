"""CPU tests of the regions split (calitas_set_regions, calitas_hits_regions, regions_of_rows, RegionScores.merge, BED reading, the
TSVs): no GPU.

The contract is regions_of_rows: class_of_row -- a plain scan of the RAW intervals per row -- and score_of_row per hits.txt row.  It
shares nothing with the library's flattened segments, coarse index and binary search.  The host stage is fed the ORACLE's per-window
alignments and held against regions_of_rows of the oracle's rows; the interval set is derived from those rows (regions_util), so the
edge cases of the class rule are in the input, and asserted to be.  Every comparison is an equality of RegionScores objects."""
import numpy as np
import pytest

from parity_util import oracle_rows
from regions_util import check_regions, derive_regions
from scores_util import distinct_model
from test_gpu_counts import GUIDE
from test_gpu_scores import edge_genome
from test_host_logic import _oracle_alignments


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


def _uniform(C, L=20):
    return C.ScoreModel.uniform(L, mismatch=32768, gap=16384, pam_mismatch=49152)


@pytest.fixture(scope="module")
def edge(C, tmp_path_factory):
    """The edge genome of the GPU tests (four contigs): (fasta, lengths by name, Guide, the oracle's alignments, the oracle's rows,
    params, Regions derived from the rows, their facts)"""
    fa, _ = edge_genome(C, tmp_path_factory.mktemp("regions_edge"))
    contigs = [(n, s.decode()) for n, s in C.read_fasta(fa).items()]
    lengths = {n: len(s) for n, s in contigs}
    alns = []
    for ci, (n, s) in enumerate(contigs):
        alns += _oracle_alignments(C, GUIDE, n, ci, s, dict(d=5, p=1, g=2, D=8, O=10))
    rows = oracle_rows(fa, GUIDE, g=2)
    params = C.make_params(max_gaps_between_guide_and_pam=2)
    model = distinct_model(C, 20)
    reg, facts = derive_regions(C, rows, lengths, model)
    return fa, lengths, C.Guide(GUIDE), alns, rows, params, reg, facts


def test_hits_regions_equals_the_contract_on_the_oracles_rows(C, edge):
    """hits_regions on a host-only context == regions_of_rows of the oracle's rows for k = 0, 1, 5, 256, every mask of interest and two
    models; by_class sums to hits_scores; with a full mask .top is hits_top."""
    fa, lengths, G, alns, rows, params, reg, facts = edge
    model = distinct_model(C, 20)
    cls = check_regions(C, rows, reg, facts, model)
    print("rows", len(rows), "classes of the rows", sorted(cls.values()), "intervals", len(reg.intervals))
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    try:
        ctx.set_regions(reg)
        shape = ctx.hits_counts(G, params, alns).shape
        for m in (model, _uniform(C)):
            scores = ctx.hits_scores(G, params, m, alns)
            for k in (0, 1, 5, 256):
                for mask in (None, 0b1, 0b10, 0b10000110, 0xFFFFFF00 | 0b100):
                    if k == 0 and mask is not None:
                        continue
                    got = ctx.hits_regions(G, params, m, k, alns, mask)
                    want = C.regions_of_rows(rows, m, reg, k, mask, shape)
                    assert got == want, (k, mask, got, want)
                    assert got.classes == ["elsewhere"] + ["c%d" % i for i in range(1, 8)] and len(got.by_class) == 8
                    total = got.by_class[0]
                    for s in got.by_class[1:]:
                        total = total + s
                    assert total == scores == got.top.scores
                    if mask is None and k:
                        assert got.top == ctx.hits_top(G, params, m, k, alns)
                        assert [got.classes[c] for c in got.hit_class] == [reg.classes[C.class_of_row(r, reg)] for h in got.top.hits
                                                                          for r in rows if (r["chromosome"], int(r["coordinate_start"]), r["strand"]) ==
                                                                          (h.chromosome, h.coordinate_start, h.strand)]
                    if mask == 0b10:
                        assert set(got.hit_class) == {1} and len(got.top.hits) == min(k, sum(1 for r in rows if cls[id(r)] == 1 and C.score_of_row(r, m) is not None))
            assert ctx.hits_regions(G, params, m, 0, alns).top.hits == []
    finally:
        ctx.close()


def test_a_mask_cuts_ties_among_its_own_candidates(C, edge):
    """A uniform model: k cuts between two equal scores among the candidates of the mask, while a hit of a higher score outside the
    mask exists -- it is not listed, and the earlier row of the two wins."""
    fa, lengths, G, alns, rows, params, reg, facts = edge
    model = _uniform(C)
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    try:
        ctx.set_regions(reg)
        everything = C.regions_of_rows(rows, model, reg, 256)
        for mask in range(1, 256):
            cand = [h for h, c in zip(everything.top.hits, everything.hit_class) if (mask >> c) & 1]
            out = [h for h, c in zip(everything.top.hits, everything.hit_class) if not (mask >> c) & 1]
            ks = [i for i in range(1, len(cand)) if cand[i - 1].score_q32 == cand[i].score_q32 and out and out[0].score_q32 > cand[i].score_q32]
            if ks:
                break
        else:
            raise AssertionError("no mask with a tie among its candidates and a better hit outside it")
        k = ks[0]
        got = ctx.hits_regions(G, params, model, k, alns, mask)
        assert got == C.regions_of_rows(rows, model, reg, k, mask, got.top.scores.table.shape)
        assert got.top.hits == cand[:k] and out[0] not in got.top.hits and cand[k].score_q32 == cand[k - 1].score_q32
    finally:
        ctx.close()


def test_set_regions_validation_and_state(C, edge):
    fa, lengths, G, alns, rows, params, reg, facts = edge
    model = distinct_model(C, 20)
    lib, RegionT = C._lib.lib, C._lib.RegionT
    ctx = C.Context(-1)
    try:
        assert lib.calitas_set_regions(ctx._h, 0, None, 0) == C._lib.ESTATE          # no reference yet
        ctx.set_reference_fasta(fa)
        with pytest.raises(C.CalitasError) as e:                                      # no regions set
            ctx.hits_regions(G, params, model, 3, alns)
        assert e.value.code == C._lib.EINVAL
        n0 = lengths["k0"]
        bad = [(RegionT(len(lengths), 0, 5, 1), 2), (RegionT(-1, 0, 5, 1), 2), (RegionT(0, 5, 5, 1), 2), (RegionT(0, 6, 5, 1), 2), (RegionT(0, -1, 5, 1), 2),
               (RegionT(0, 0, n0 + 1, 1), 2), (RegionT(0, 0, 5, 0), 2), (RegionT(0, 0, 5, 2), 2), (RegionT(0, 0, 5, 8), 8), (RegionT(0, 0, 5, 1), 1),
               (RegionT(0, 0, 5, 1), 9)]
        for r, nc in bad:
            arr = (RegionT * 1)(r)
            assert lib.calitas_set_regions(ctx._h, 1, arr, nc) == C._lib.EINVAL, (r.contig_index, r.start, r.end, r.cls, nc)
        ok = (RegionT * 2)(RegionT(0, 0, n0, 7), RegionT(3, lengths["k3"] - 1, lengths["k3"], 1))
        assert lib.calitas_set_regions(ctx._h, 2, ok, 8) == C._lib.OK
        assert ctx.region_class("k0", 5, 6) == 7 and ctx.region_class("k3", lengths["k3"] - 1, lengths["k3"]) == 1 and ctx.region_class("k1", 0, 10) == 0
        # a bad set leaves the old one in place; n = 0 clears it; a new reference drops it
        assert lib.calitas_set_regions(ctx._h, 1, (RegionT * 1)(RegionT(0, 6, 5, 1)), 2) == C._lib.EINVAL and ctx.region_class("k0", 5, 6) == 7
        ctx.set_regions(reg)
        for k, mask, code in ((257, None, C._lib.EINVAL), (3, 0, C._lib.EINVAL), (3, 0xFFFFFF00, C._lib.EINVAL)):
            with pytest.raises(C.CalitasError) as e:
                ctx.hits_regions(G, params, model, k, alns, mask)
            assert e.value.code == code
        assert ctx.hits_regions(G, params, model, 0, alns, 0).top.hits == []          # k = 0: the mask is not looked at
        with pytest.raises(C.CalitasError):
            ctx.hits_regions(G, params, distinct_model(C, 21), 3, alns)
        ctx.set_regions(None)
        assert ctx.region_class("k0", 5, 6) == -1
        with pytest.raises(C.CalitasError):
            ctx.hits_regions(G, params, model, 3, alns)
        ctx.set_regions(reg)
        ctx.set_reference_fasta(fa)
        assert ctx.regions is None and ctx.region_class("k0", 5, 6) == -1
        with pytest.raises(ValueError):
            ctx.set_regions(C.Regions([("nowhere", 0, 5, "x")]))
    finally:
        ctx.close()


def test_flattened_lookup_against_the_naive_scan(C, tmp_path):
    """Random interval sets (any order, overlapping, nested, abutting, one-base, at both contig ends and across multiples of 8192) on
    three contigs, one of them shorter than a coarse block and one without intervals: the library's class of random extents -- empty
    ones, ones that overhang the contig, ones that end or start exactly at an interval's edge -- equals class_of_row's plain scan."""
    from fasta_util import write_fasta
    rng = np.random.default_rng(8192)
    lengths = {"a": 3 * 8192 + 77, "b": 500, "c": 8192, "d": 8193}
    fa = write_fasta(str(tmp_path / "r.fa"), [(n, "ACGT" * (ln // 4) + "A" * (ln % 4)) for n, ln in lengths.items()])
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    try:
        for trial in range(12):
            n_classes = int(rng.integers(2, 9))
            iv = []
            for n, ln in lengths.items():
                if n == "c" and trial % 2:
                    continue
                for _ in range(int(rng.integers(1, 60))):
                    a = int(rng.integers(0, ln))
                    w = int(rng.choice([1, 1, 2, 7, 40, 300, 9000]))
                    iv.append((n, a, min(ln, a + w), "c%d" % rng.integers(1, n_classes)))
                iv += [(n, 0, 1, "c1"), (n, ln - 1, ln, "c%d" % (n_classes - 1))]
                for m in range(8192, ln, 8192):
                    iv.append((n, m - int(rng.integers(0, 3)), min(ln, m + int(rng.integers(1, 3))), "c%d" % rng.integers(1, n_classes)))
                    iv.append((n, m - 10, m - 5, "c1"))          # (decides extents across m from the segment they start in)
            reg = C.Regions(iv, classes=["c%d" % i for i in range(1, n_classes)])
            ctx.set_regions(reg)
            edges = {n: sorted({x for c, s, e, k in reg.intervals if c == n for x in (s, e)}) or [0] for n in lengths}
            for _ in range(1500):
                n = str(rng.choice(list(lengths)))
                ln = lengths[n]
                if rng.integers(0, 2):
                    a = int(rng.choice(edges[n])) + int(rng.integers(-24, 3))
                else:
                    a = int(rng.integers(-30, ln + 5))
                b = a + int(rng.choice([0, 1, 20, 23, 25, 100]))
                row = {"chromosome": n, "coordinate_start": str(a), "coordinate_end": str(b)}
                assert ctx.region_class(n, a, b) == C.class_of_row(row, reg), (trial, n, a, b)
            for n, ln in lengths.items():
                for m in range(8192, ln, 8192):
                    if any(c == n for c, s, e, k in reg.intervals):
                        assert ctx.region_class(n, m - 12, m + 8) == 1 and ctx.region_class(n, m - 5, m + 8) == C.class_of_row(
                            {"chromosome": n, "coordinate_start": str(m - 5), "coordinate_end": str(m + 8)}, reg)
    finally:
        ctx.close()


def test_merge_of_pieces_in_order(C, edge):
    """regions_of_rows of the rows cut at three places, merged in order, is regions_of_rows of all rows: by_class adds, the lists merge
    stably and every record keeps its class."""
    fa, lengths, G, alns, rows, params, reg, facts = edge
    for model in (distinct_model(C, 20), _uniform(C)):
        for k, mask in ((0, None), (1, None), (6, 0b110), (256, None), (9, 0b11111110)):
            whole = C.regions_of_rows(rows, model, reg, k, mask)
            n = len(rows)
            for cuts in ((n // 4, n // 2, 3 * n // 4), (1, 2, n - 1), (n // 3, n // 3, n // 2)):
                a, b, c = cuts
                pieces = [C.regions_of_rows(p, model, reg, k, mask) for p in (rows[:a], rows[a:b], rows[b:c], rows[c:])]
                assert pieces[0].merge(*pieces[1:]) == whole, (k, mask, cuts)
    with pytest.raises(ValueError):
        C.regions_of_rows(rows[:5], model, reg, 3).merge(C.regions_of_rows(rows[5:], model, reg, 4))


def test_bed_reading(C, tmp_path, capsys):
    p = tmp_path / "r.bed"
    p.write_text("# a comment\ntrack name=x\nbrowser position k0:1-5\n\nk1\t10\t20\tutr\textra\nk0\t0\t5\texon\nkX\t1\t2\tintron\nk0 7 9 utr\n")
    reg = C.Regions.read_bed(str(p), {"k0": 100, "k1": 50})
    assert reg.classes == ["elsewhere", "utr", "exon", "intron"]            # priority = order of first appearance, skipped chromosomes included
    assert reg.intervals == [("k1", 10, 20, 1), ("k0", 0, 5, 2), ("k0", 7, 9, 1)]
    assert "1 intervals on chromosomes the reference does not have were skipped" in capsys.readouterr().err
    assert reg.mask_of("exon,elsewhere") == 0b101 and reg.mask_of(["intron"]) == 0b1000
    with pytest.raises(ValueError):
        reg.mask_of("nothing")
    assert len(C.Regions.read_bed(str(p)).intervals) == 4                   # (without a reference nothing is skipped)
    for text in ("k0\t0\t101\texon\n", "k0\t5\t5\texon\n", "k0\t0\t5\n", "k0\tx\t5\texon\n", "k0\t0\t5\telsewhere\n",
                 "".join("k0\t0\t5\tn%d\n" % i for i in range(8))):
        p.write_text(text)
        with pytest.raises(ValueError):
            C.Regions.read_bed(str(p), {"k0": 100})
    p.write_text("".join("k0\t0\t5\tn%d\n" % i for i in range(7)))
    assert len(C.Regions.read_bed(str(p), {"k0": 100}).classes) == 8


def test_the_tsvs_and_the_flag(C, edge, tmp_path, monkeypatch):
    """regions_tsv: guide_id class rows perfect offtarget_sum_q32 max_q32 specificity, a line per class in class order; top_tsv with
    class names gains a last column; `--scores M --regions F [--top K [--top-classes ..]] [--counts]` writes scores, classes, top,
    counts with an empty line between; --regions without --scores or with --variants is refused.  No GPU here: the search behind
    SearchReference.regions() is replaced by the host stage (tests/test_gpu_regions.py runs the flag end to end on the device)."""
    from calitas_amd import __main__ as M
    from calitas_amd import aligner
    fa, lengths, G, alns, rows, params, reg, facts = edge
    model = distinct_model(C, 20)
    ctx = C.Context(-1)
    ctx.set_reference_fasta(fa)
    try:
        ctx.set_regions(reg)
        got = ctx.hits_regions(G, params, model, 5, alns, 0b110)
    finally:
        ctx.close()
    text = C.regions_tsv("g7", got)
    lines = text.split("\n")
    assert lines[0].split("\t") == ["guide_id", "class", "rows", "perfect", "offtarget_sum_q32", "max_q32", "specificity"]
    assert len(lines) == 10 and lines[9] == ""
    for ln, name, s in zip(lines[1:9], got.classes, got.by_class):
        assert ln.split("\t") == ["g7", name, str(s.rows), str(s.perfect), str(s.sum_q32), str(s.max_q32), "%.6f" % s.specificity]
    names = [got.classes[c] for c in got.hit_class]
    top_text = C.top_tsv("g7", got.top, names)
    tl = [ln.split("\t") for ln in top_text.splitlines()]
    assert tl[0][-1] == "class" and [f[-1] for f in tl[1:]] == names and set(names) <= {"c1", "c2"} and len(names) == 5
    assert [f[:-1] for f in tl] == [ln.split("\t") for ln in C.top_tsv("g7", got.top).splitlines()]
    mpath, bed = str(tmp_path / "model.tsv"), str(tmp_path / "r.bed")
    model.write(mpath)
    open(bed, "w").write("k0\t0\t5\tc1\n")
    seen = {}

    def fake(self, m, regions, k=0, top_classes=None):
        seen.update(regions=regions, k=k, top_classes=top_classes)
        return got
    monkeypatch.setattr(aligner.SearchReference, "regions", fake)
    out = tmp_path / "out.tsv"
    flags = ["SearchReference", "-i", GUIDE, "-I", "g7", "-r", "unused.fa", "-o", str(out), "-g", "2"]
    assert M.main(flags + ["--scores", mpath, "--regions", bed, "--top", "5", "--top-classes", "c1,c2", "--counts"]) == 0
    assert seen == dict(regions=bed, k=5, top_classes="c1,c2")
    assert out.read_text() == C.scores_tsv("g7", got.top.scores) + "\n" + text + "\n" + top_text + "\n" + C.counts_tsv("g7", got.top.scores.table)
    assert M.main(flags + ["--scores", mpath, "--regions", bed]) == 0 and seen["k"] == 0
    assert out.read_text() == C.scores_tsv("g7", got.top.scores) + "\n" + text
    for extra in (["--regions", bed], ["--scores", mpath, "--regions", bed, "-v", "some.vcf"], ["--scores", mpath, "--regions", bed, "--top-classes", "c1"],
                  ["--scores", mpath, "--top", "3", "--top-classes", "c1"]):
        with pytest.raises(SystemExit):
            M.main(flags + extra)
