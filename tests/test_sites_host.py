"""CPU tests of the guide-site enumeration: calitas_find_sites_host (the host twin of the kernel, on a host-only context) against the
brute force of sites_ref.py, find_guides' strings, and both FindGuides tools on the host twin (--device -1).  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sites_ref as R
from fasta_util import write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


@pytest.fixture(scope="module")
def genome(C):
    names, seqs = R.host_genome()
    ctx = C.Context(-1)
    ctx.set_reference(names, [s.encode() for s in seqs])
    yield ctx, names, seqs
    ctx.close()


def _pattern(C, name):
    text, aux = R.pattern_string(name)
    return C.Guide(text, aux)


@pytest.mark.parametrize("name", sorted(R.PATTERNS))
def test_host_twin_equals_brute_force(C, genome, name):
    ctx, names, seqs = genome
    proto, pams, five = R.PATTERNS[name]
    want = R.brute_sites(seqs, proto, pams, five)
    got = R.as_tuples(ctx.find_sites(_pattern(C, name), host=True))
    print(name, "sites", len(want), "plus", sum(1 for w in want if w[3] == "+"))
    assert got == want
    assert len(want) > 0
    assert got == sorted(got, key=lambda s: (s[0], s[1], s[3] == "-"))             # contig, protospacer start, '+' before '-'
    # the per-contig calls concatenate to the all-contigs call
    parts = []
    for i in range(len(names)):
        parts += R.as_tuples(ctx.find_sites(_pattern(C, name), chrom=i, host=True))
    assert parts == want


def test_the_cases_the_genome_was_built_for(C, genome):
    ctx, names, seqs = genome
    got = R.as_tuples(ctx.find_sites(_pattern(C, "fixed_nrg"), host=True))
    on_a = {(p, s) for c, p, _, s, _, _, _ in got if c == 0}
    n = len(seqs[0])
    assert (0, "+") in on_a and (n - 23, "+") in on_a          # first base, last base
    assert (203, "-") in on_a                                   # '-': the PAM lies to the left of the protospacer
    assert (300, "+") in on_a                                   # soft-masked
    assert (400, "+") not in on_a                               # an R of the reference in the footprint
    assert (500, "+") in on_a and (563, "-") in on_a            # U / u
    assert (740, "+") in on_a and (908, "-") in on_a            # abutting N runs
    on_b = {(p, s) for c, p, _, s, _, _, _ in got if c == 1}
    assert (3, "-") in on_b and (len(seqs[1]) - 20, "-") in on_b
    assert [(c, p, pm, s) for c, p, pm, s, _, _, _ in got if c == 2] == [(2, 0, 20, "+")]       # the 26-base contig holds one
    assert not [1 for s in got if s[0] == 3]
    # nngrrt first, nrg as the auxiliary PAM: where both match the first wins; nrg alone elsewhere
    got = R.as_tuples(ctx.find_sites(_pattern(C, "n20_nngrrt_nrg"), host=True))
    both = [s for s in got if s[0] == 0 and s[1] == 1000 and s[3] == "+"]
    assert both == [(0, 1000, 1020, "+", 0, 6, 20)]
    assert {s[4] for s in got} == {0, 1} and any(s[4] == 1 and s[5] == 3 for s in got)
    assert len({(s[0], s[1], s[3]) for s in got}) == len(got)                                   # one record per position and strand
    # the 48-base maximum does not fit the 26- and 12-base contigs
    got = R.as_tuples(ctx.find_sites(_pattern(C, "max48"), host=True))
    assert got and all(s[5] == 16 and s[6] == 32 and s[0] in (0, 1, 4) for s in got)
    # PAM-less
    got = R.as_tuples(ctx.find_sites(_pattern(C, "n21"), host=True))
    assert all(s[2] == -1 and s[4] == -1 and s[5] == 0 for s in got)
    assert [s for s in got if s[0] == 2] == [(2, p, -1, st, -1, 0, 21) for p in range(6) for st in "+-"]


@pytest.mark.parametrize("name", ["fixed_nrg", "tttv_n20", "n20_nngrrt_nrg"])
def test_region_bounds_off_by_one(C, genome, name):
    ctx, names, seqs = genome
    proto, pams, five = R.PATTERNS[name]
    whole = R.brute_sites(seqs, proto, pams, five, chrom=0)
    # a '+' and a '-' site in the middle of chrA; their footprints
    for strand in "+-":
        c, p, pm, s, k, pl, L = [w for w in whole if w[3] == strand and 100 < w[1] < 2500][0]
        lo, hi = min(p, pm), max(p + L, pm + pl)
        for a, b in ((lo, hi), (lo + 1, hi), (lo, hi - 1), (lo - 1, hi + 1), (lo - 7, hi + 40)):
            want = R.brute_sites(seqs, proto, pams, five, chrom=0, start=a, end=b)
            got = R.as_tuples(ctx.find_sites(_pattern(C, name), chrom="chrA", start=a, end=b, host=True))
            assert got == want, (strand, a, b)
            inside = any(w[1] == p and w[3] == strand for w in got)
            if name == "fixed_nrg":
                assert inside == (a <= lo and hi <= b), (strand, a, b)
    # end == 0 / None: the contig's end
    want = R.brute_sites(seqs, proto, pams, five, chrom=1, start=700)
    assert R.as_tuples(ctx.find_sites(_pattern(C, name), chrom=1, start=700, host=True)) == want
    assert R.as_tuples(ctx.find_sites(_pattern(C, name), chrom=1, start=700, end=len(seqs[1]), host=True)) == want


def test_bad_arguments_and_absent_contigs(C):
    ctx = C.Context(-1)
    ctx.set_reference(["a", "b"], [b"ACGTACGTACGTACGTACGTACGTAGGACGT", None], lengths=[31, 500])
    assert len(ctx.find_sites("NNNNNNNNNNNNNNNNNNNNnrg", chrom="a", host=True)) >= 1
    for chrom in ("b", None):
        with pytest.raises(C.CalitasError) as e:
            ctx.find_sites("NNNNNNNNNNNNNNNNNNNNnrg", chrom=chrom, host=True)
        assert e.value.code == C._lib.EINVAL and "absent" in str(e.value)
    with pytest.raises(C.CalitasError):
        ctx.find_sites("NNNNNNNNNNNNNNNNNNNNnrg", chrom="a", start=10, end=40, host=True)          # past the contig's end
    with pytest.raises(C.CalitasError):
        ctx.find_sites("NNNNNNNNNNNNNNNNNNNNnrg", chrom="a", start=20, end=10, host=True)
    with pytest.raises(ValueError):
        ctx.find_sites("NNNNNNNNNNNNNNNNNNNNnrg", chrom="nope", host=True)
    # the device calls on a host-only context fail as the searches do
    for call in (lambda: ctx.find_sites("NNNNNNNNNNNNNNNNNNNNnrg", chrom="a"), lambda: ctx.count_sites("NNNNNNNNNNNNNNNNNNNNnrg", chrom="a")):
        with pytest.raises(C.CalitasError) as e:
            call()
        assert e.value.code == C._lib.ENODEV and "no CPU fallback" in str(e.value)
    ctx.close()


def test_record_layout(C):
    from calitas_amd import _lib
    import ctypes
    assert ctypes.sizeof(_lib.SiteT) == 16 and np.dtype(C.aligner.SITE_DTYPE).itemsize == 16
    assert [(f, np.dtype(C.aligner.SITE_DTYPE).fields[f][1]) for f, _ in _lib.SiteT._fields_] == \
        [("contig_index", 0), ("protospacer_start", 4), ("pam_start", 8), ("strand", 12), ("pam_index", 13), ("pam_length", 14),
         ("protospacer_length", 15)]


@pytest.mark.parametrize("name", ["n20_nrg", "tttv_n20", "n20_nngrrt_nrg", "n21"])
def test_find_guides_strings(C, genome, name):
    """Each string re-parsed by Guide(...) has the pattern's matched PAM and an ACGT protospacer that is the text on the site's strand."""
    ctx, names, seqs = genome
    proto, pams, five = R.PATTERNS[name]
    pat = _pattern(C, name)
    rows = C.find_guides(ctx, pat, host=True)
    sites = R.brute_sites(seqs, proto, pams, five)
    assert len(rows) == len(sites) > 0
    for r, (c, p, pm, s, k, pl, L) in zip(rows, sites):
        g = C.Guide(r.guide)
        assert g.pams == ([pams[k]] if pams else []) and g.pam_is_five_prime == (five and bool(pams))
        assert set(g.guide) <= set("ACGT") and len(g.guide) == L
        text = seqs[c][p:p + L].upper().replace("U", "T")
        assert g.guide == (R.revcomp(text) if s == "-" else text)
        lo, hi = (p, p + L) if pm < 0 else (min(p, pm), max(p + L, pm + pl))
        assert (r.chromosome, r.start, r.end, r.strand, r.pam_index, r.protospacer_start) == (names[c], lo, hi, s, k, p)
        assert r.guide_id == "%s:%d:%s" % (names[c], lo, s)
        genomic = seqs[c][pm:pm + pl].upper() if pm >= 0 else ""
        assert r.pam_sequence.replace("U", "T") == (R.revcomp(genomic.replace("U", "T")) if s == "-" else genomic.replace("U", "T"))
        if pams:
            assert all(x in R.IUPAC[y.upper()] for x, y in zip(r.pam_sequence.replace("U", "T"), pams[k]))


def test_guides_tsv_with_counts_columns(C, genome):
    """The writer on host results; the tables stand in for a search (the GPU test runs --counts end to end)."""
    ctx, names, seqs = genome
    rows = C.find_guides(ctx, "NNNNNNNNNNNNNNNNNNNNnrg", chrom="c26", host=True) + C.find_guides(ctx, "NNNNNNNNNNNNNNNNNNNNnrg", chrom="chrB", host=True)[:3]
    tables = {}
    for i, g in enumerate(dict.fromkeys(r.guide for r in rows)):
        t = np.zeros((2, 3, 4, 2), dtype=np.uint64)
        t[0, 0, 0, 0], t[1, 2, 1, 1], t[0, 2, 3, 0] = 1, i, 5
        tables[g] = t
    lines = C.guides_tsv(rows, tables).splitlines()
    assert lines[0].split("\t") == ["guide_id", "chromosome", "start", "end", "strand", "pam_index", "guide", "pam_sequence", "hits", "hits_mm0",
                                    "hits_mm1", "hits_mm2"]
    assert len(lines) == 1 + len(rows)
    for ln, r in zip(lines[1:], rows):
        f = ln.split("\t")
        t = tables[r.guide]
        assert f[:8] == [str(x) for x in r.row()]
        assert [int(x) for x in f[8:]] == [int(t.sum()), 1, 0, int(t[:, 2].sum())]
    plain = C.guides_tsv(rows).splitlines()
    assert plain[0].split("\t") == C.tools.GUIDE_COLUMNS and [ln.split("\t") for ln in plain[1:]] == [[str(x) for x in r.row()] for r in rows]


def test_both_tools_write_the_same_table_on_the_host_twin(C, genome, tmp_path):
    """`python -m calitas_amd FindGuides` and `calitas FindGuides` with --device -1 (the host twin: no GPU needed)."""
    ctx, names, seqs = genome
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    binary = os.path.join(ROOT, "calitas_amd", "calitas")
    for k, extra in enumerate((["-i", "NNNNNNNNNNNNNNNNNNNNnngrrt", "-x", "nrg", "-c", "chrA", "-s", "350", "-e", "1100"],
                               ["-i", "tttvNNNNNNNNNNNNNNNNNNNN"])):
        py, cc = str(tmp_path / ("py%d.tsv" % k)), str(tmp_path / ("cc%d.tsv" % k))
        env = dict(os.environ, PYTHONPATH=ROOT)
        subprocess.check_call([sys.executable, "-m", "calitas_amd", "FindGuides", "-r", fa, "-o", py, "--device", "-1"] + extra, env=env, cwd=ROOT)
        subprocess.check_call([binary, "FindGuides", "-r", fa, "-o", cc, "--device", "-1"] + extra)
        a, b = open(py, "rb").read(), open(cc, "rb").read()
        assert a == b and a.count(b"\n") > 3
        pat = C.Guide(extra[1], extra[3:4] if "-x" in extra else [])
        rows = C.find_guides(ctx, pat, chrom="chrA" if "-c" in extra else None, start=350 if "-s" in extra else 0,
                             end=1100 if "-e" in extra else None, host=True)
        assert a.decode() == C.guides_tsv(rows)
