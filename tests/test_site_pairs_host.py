"""CPU tests of the site pairs: calitas_find_site_pairs_host and calitas_count_site_pairs_host (the host twin of site_pairs.hip's chain, on
a host-only context) against the referee of site_pairs_ref.py, byte for byte, over the grid -- N20nrg and tttvN20; the bounds (0, 0),
(0, 40), (30, 150) and (1000, 3000), the last through the bisection; the cut offsets 0, L - 3 and L; every orientation mask; with and
without a site filter; a sub-region and every contig -- what the genome was planted for, the degenerate listings, the errors in their
order, the struct sizes, a reference with Us, SitePairs' names, and both FindGuides tools with --pairs on the host twin.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import site_pairs_ref as P
import sites_ref as R
from fasta_util import write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = P.L


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


@pytest.fixture(scope="module")
def genome(C):
    names, seqs = P.genome()
    ctx = C.Context(-1)
    ctx.set_reference(names, [s.encode() for s in seqs])
    yield ctx, names, seqs
    ctx.close()


def _hold(C, ctx, name, seqs, cut, lo, hi, mask, filter=None, keep=None, **region):
    """One call of the twin and its count against the referee.  keep: the referee's sites that pass `filter` (indices)."""
    sites, wide = P.wide_pairs(C, name, seqs, cut, **region)
    want = P.cell(wide, lo, hi, mask)
    if keep is not None:
        new = {old: k for k, old in enumerate(keep)}
        want = np.array([(new[l], new[r], d, o) for l, r, d, o in want.tolist() if l in new and r in new], dtype=np.int64).reshape(-1, 4)
        sites = [sites[i] for i in keep]
    spec = C.SitePairs(lo, hi, cut, P.codes_of(mask))
    got_sites, got = ctx.find_site_pairs(P.pattern_of(C, name), spec, filter=filter, host=True, **region)
    assert R.as_tuples(got_sites) == sites
    assert np.array_equal(P.as_rows(got), want), (name, cut, lo, hi, mask)
    n, n_pairs, by = ctx.count_site_pairs(P.pattern_of(C, name), spec, filter=filter, host=True, **region)
    assert (n, n_pairs) == (len(sites), len(want)) and int(by.sum()) == n_pairs
    assert by.tolist() == [int((want[:, 3] == o).sum()) for o in range(4)]
    return got_sites, got


def test_the_genome_holds_what_it_was_planted_for(C):
    P.check_planted(C)


@pytest.mark.parametrize("name", P.NAMES)
@pytest.mark.parametrize("cut", P.CUTS)
def test_the_twin_against_the_referee(C, genome, name, cut):
    ctx, names, seqs = genome
    for lo, hi in P.BOUNDS:
        for mask in P.MASKS:
            _hold(C, ctx, name, seqs, cut, lo, hi, mask)


@pytest.mark.parametrize("name", P.NAMES)
def test_a_filter_one_contig_and_a_sub_region(C, genome, name):
    ctx, names, seqs = genome
    # a pair of a filtered listing is a pair of the whole listing whose members both pass: the indices are the filtered listing's
    flt = C.SiteFilter(gc_min=6, gc_max=14)
    sites = P.sites_of(name, seqs)
    passing = set(R.as_tuples(ctx.find_sites(P.pattern_of(C, name), host=True, filter=flt)))
    keep = [i for i, s in enumerate(sites) if s in passing]
    assert 0 < len(keep) < len(sites)
    for lo, hi in P.BOUNDS:
        _hold(C, ctx, name, seqs, L - 3, lo, hi, 15, filter=flt, keep=keep)
    for lo, hi in P.BOUNDS:
        for mask in (2, 4, 9, 15):
            _hold(C, ctx, name, seqs, L - 3, lo, hi, mask, chrom=0, start=250, end=3300)     # cuts into the dense stretch's head
            _hold(C, ctx, name, seqs, L - 3, lo, hi, mask, chrom=1)


def test_degenerate_listings(C, genome):
    ctx, names, seqs = genome
    pat = P.pattern_of(C, "n20_nrg")
    spec = C.SitePairs(0, 40, orientations="any")
    sites, pairs = ctx.find_site_pairs(pat, spec, chrom=0, start=P.PLANTED[0] + 100, end=P.PLANTED[0] + 130, host=True)
    assert len(sites) == 0 and len(pairs) == 0 and pairs.dtype == np.dtype(C.aligner.SITE_PAIR_DTYPE)
    assert ctx.count_site_pairs(pat, spec, chrom=0, start=P.PLANTED[0] + 100, end=P.PLANTED[0] + 130, host=True)[:2] == (0, 0)
    sites, pairs = ctx.find_site_pairs(pat, spec, chrom=0, start=P.PLANTED[0] + 5, end=P.PLANTED[0] + 10 + L + 3, host=True)
    assert len(sites) == 1 and len(pairs) == 0                                               # one site: the first planted one
    sites, pairs = ctx.find_site_pairs(pat, C.SitePairs(0, 40, orientations="+-,-+,--"), chrom=0, start=P.PLANTED[0] + 5,
                                       end=P.PLANTED[0] + 10 + 60, host=True)
    assert len(sites) == 3 and len(pairs) == 0                                               # three '+' sites, no pair among the orientations asked


def _call(C, ctx, pat, opt, f=None, chrom=-1, host=True):
    from calitas_amd import _lib
    g = pat.to_c()
    out, n = ctypes.POINTER(_lib.SiteT)(), ctypes.c_uint64()
    pairs, n_pairs = ctypes.POINTER(_lib.SitePairT)(), ctypes.c_uint64()
    fn = _lib.lib.calitas_find_site_pairs_host if host else _lib.lib.calitas_find_site_pairs
    rc = fn(ctx._h, ctypes.byref(g), ctypes.byref(f) if f is not None else None, ctypes.byref(opt) if opt is not None else None, chrom, 0, 0,
            ctypes.byref(out), ctypes.byref(n), ctypes.byref(pairs), ctypes.byref(n_pairs))
    msg = _lib.lib.calitas_last_error(ctx._h).decode()
    if rc == 0:
        _lib.lib.calitas_free(out)
        _lib.lib.calitas_free(pairs)
    else:
        assert not out and not pairs
    return rc, msg


def test_errors_in_their_order(C, genome):
    from calitas_amd import _lib
    ctx, names, seqs = genome
    pat = P.pattern_of(C, "n20_nrg")

    def T(lo, hi, cut, mask, r0=0, r1=0):
        t = _lib.SitePairsT()
        t.min_distance, t.max_distance, t.cut_offset, t.orientations = lo, hi, cut, mask
        t.reserved[0], t.reserved[1] = r0, r1
        return t
    bad_filter = C.SiteFilter(gc_min=0, gc_max=255).to_c()
    bad_filter.reserved = 1
    everything_wrong = T(-5, 70000, 21, 16, 1, 1)
    # what calitas_find_sites_filtered refuses comes first: the region, then the filter
    rc, msg = _call(C, ctx, pat, None, chrom=7)
    assert rc == _lib.EINVAL and "chrom_index" in msg
    rc, msg = _call(C, ctx, pat, everything_wrong, f=bad_filter)
    assert rc == _lib.EINVAL and "site filter" in msg
    rc, msg = _call(C, ctx, pat, None)
    assert rc == _lib.EINVAL and "opt" in msg
    # then opt's fields, in the order the header states
    rc, msg = _call(C, ctx, pat, everything_wrong)
    assert rc == _lib.EINVAL and "orientations" in msg
    rc, msg = _call(C, ctx, pat, T(-5, 70000, 21, 0, 1, 1))
    assert rc == _lib.EINVAL and "orientations" in msg
    for r in ((1, 0), (0, 1)):
        rc, msg = _call(C, ctx, pat, T(-5, 70000, 21, 15, *r))
        assert rc == _lib.EINVAL and "reserved" in msg
    rc, msg = _call(C, ctx, pat, T(-5, -7, 21, 15))
    assert rc == _lib.EINVAL and "min_distance" in msg and "negative" in msg
    rc, msg = _call(C, ctx, pat, T(70001, 70000, 21, 15))
    assert rc == _lib.EINVAL and "min_distance" in msg and "max_distance" in msg and "above max_distance" in msg
    rc, msg = _call(C, ctx, pat, T(0, _lib.PAIR_MAX_DISTANCE + 1, 21, 15))
    assert rc == _lib.EINVAL and "CALITAS_PAIR_MAX_DISTANCE" in msg
    rc, msg = _call(C, ctx, pat, T(0, _lib.PAIR_MAX_DISTANCE, 21, 15))
    assert rc == _lib.EINVAL and "cut_offset" in msg
    for ok in (T(0, 0, 0, 1), T(0, _lib.PAIR_MAX_DISTANCE, 20, 15), T(40, 40, 17, 8)):
        assert _call(C, ctx, pat, ok)[0] == 0
    # the device call on a host-only context, before everything
    rc, msg = _call(C, ctx, pat, everything_wrong, f=bad_filter, chrom=7, host=False)
    assert rc == _lib.ENODEV


def test_struct_sizes(C):
    from calitas_amd import _lib
    assert ctypes.sizeof(_lib.SitePairsT) == 12 and ctypes.sizeof(_lib.SitePairT) == 16
    assert np.dtype(C.aligner.SITE_PAIR_DTYPE).itemsize == 16
    assert _lib.PAIR_MAX_DISTANCE == 65535


def test_a_reference_with_us(C):
    names, seqs = P.u_genome()
    ctx = C.Context(-1)
    try:
        ctx.set_reference(names, [s.encode() for s in seqs])
        for lo, hi in ((0, 40), (30, 150)):
            for mask in (1, 2, 15):
                got_sites, got = _hold(C, ctx, "n20_nrg", seqs, L - 3, lo, hi, mask)
        assert len(got_sites) >= 6 and len(got) > 0
    finally:
        ctx.close()


def test_the_names_of_the_orientations(C):
    three, five, bare = C.Guide("N" * 20 + "nrg"), C.Guide("tttv" + "N" * 20), C.Guide("N" * 21)
    S = C.SitePairs
    assert S(0, 1).mask_of(three) == 2 and S(0, 1).mask_of(five) == 4                       # out: "-+" with a 3' PAM, "+-" with a 5' PAM
    assert S(0, 1, orientations="in").mask_of(three) == 4 and S(0, 1, 5, "in").mask_of(five) == 2
    assert S(0, 1, orientations="same").mask_of(three) == 9 and S(0, 1, orientations="any").mask_of(five) == 15
    assert S(0, 1, orientations="++,--").mask_of(bare) == 9 and S(0, 1, orientations=["-+", "in"]).mask_of(three) == 6
    assert S(0, 1).cut_of(three) == 17 and S(0, 1, 4).cut_of(five) == 4
    with pytest.raises(ValueError):
        S(0, 1).cut_of(five)                                                                # the default cut is a 3' PAM's
    with pytest.raises(ValueError):
        S(0, 1, 3).mask_of(bare)                                                            # names need a PAM
    with pytest.raises(ValueError):
        S(0, 1, orientations="sideways")
    assert [S(0, 1).name_of(o, three) for o in range(4)] == ["same", "out", "in", "same"]
    assert [S(0, 1).name_of(o, five) for o in range(4)] == ["same", "in", "out", "same"]
    assert [S(0, 1).name_of(o, bare) for o in range(4)] == ["++", "-+", "+-", "--"]
    # the contract function on three sites by hand: '+' at 100 (cut 117), '-' at 90 (cut 93), '-' at 140 (cut 143)
    sites = [(0, 90, "-"), (0, 100, "+"), (0, 140, "-"), (1, 100, "-")]
    assert C.site_pairs_of(sites, S(0, 40, orientations="any"), three) == [(0, 1, 24, 1), (1, 2, 26, 2)]
    assert C.site_pairs_of(sites, S(0, 50, orientations="same"), three) == [(0, 2, 50, 3)]


def _run(cmd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)


TOOLS = ([sys.executable, "-m", "calitas_amd", "FindGuides"], [os.path.join(ROOT, "calitas_amd", "calitas"), "FindGuides"])


def _bed(path):
    with open(path, "w") as f:
        f.write("chrA\t%d\t%d\texon\nchrA\t100\t200\tutr\n" % (P.PLANTED[0], P.PLANTED[0] + 400))
    return str(path)


@pytest.mark.parametrize("flags", [["--pair-distance", "30:150"], ["--pair-distance", "0:40", "--pair-orientation", "any", "--pair-cut", "0"],
                                   ["--pair-distance", "0:200", "--pair-orientation", "same,-+", "--max-copies", "1"],
                                   ["--pair-distance", "10:400", "--pair-orientation", "in,++", "--regions", "BED", "--gc-max", "60"]])
def test_both_tools_on_the_host_twin(C, genome, tmp_path, flags):
    ctx, names, seqs = genome
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    flags = [_bed(tmp_path / "r.bed") if x == "BED" else x for x in flags]
    text, aux = R.pattern_string("n20_nrg")
    start, end = (P.DENSE[1] - 120, P.PLANTED[1]) if "--max-copies" in flags else (P.PLANTED[0] - 60, P.PLANTED[1] + 60)
    common = ["-i", text, "-r", fa, "--device", "-1", "-c", "chrA", "-s", str(start), "-e", str(end)] + flags
    out = []
    for k, tool in enumerate(TOOLS):
        pairs = str(tmp_path / ("pairs%d.tsv" % k))
        r = _run(tool + common + ["--pairs", pairs])
        assert r.returncode == 0, r.stderr
        out.append((r.stdout, open(pairs).read()))
    assert out[0] == out[1]                                                     # the same bytes from each, table and pairs
    table, pairs = out[0]
    ids = {ln.split("\t")[0] for ln in table.splitlines()[1:]}
    lines = [ln.split("\t") for ln in pairs.splitlines()]
    assert lines[0] == C.tools.PAIR_COLUMNS and len(lines) > 1
    assert [ln[0] for ln in lines[1:]] == [str(k + 1) for k in range(len(lines) - 1)]
    assert {ln[1] for ln in lines[1:]} | {ln[2] for ln in lines[1:]} <= ids     # both members are rows of the table
    # against the library's contract: the rows as find_guides lists them, paired by guide_pairs
    pat = P.pattern_of(C, "n20_nrg")
    lo, hi = flags[flags.index("--pair-distance") + 1].split(":")
    spec = C.SitePairs(int(lo), int(hi), int(flags[flags.index("--pair-cut") + 1]) if "--pair-cut" in flags else None,
                       flags[flags.index("--pair-orientation") + 1] if "--pair-orientation" in flags else "out")
    flt = C.site_filter_of_flags(20, gc_max=60) if "--gc-max" in flags else None
    if "--regions" in flags:
        ctx.set_regions(C.Regions.read_bed(flags[flags.index("--regions") + 1], dict(zip(ctx.contig_names, ctx.contig_lengths))))
    rows = C.find_guides(ctx, pat, chrom="chrA", start=start, end=end, host=True, filter=flt, by_regions="--regions" in flags)
    if "--max-copies" in flags:
        copies = C.guide_copies(ctx, pat, rows, host=True)
        rows = [r for r, n in zip(rows, copies) if n <= 1]
        assert 0 < len(rows) < len(copies)
    assert [r.guide_id for r in rows] == [ln.split("\t")[0] for ln in table.splitlines()[1:]]
    paired = C.guide_pairs(ctx, pat, rows, spec, chrom="chrA", start=start, end=end, host=True, filter=flt)
    assert C.pairs_tsv(rows, [spec.name_of(o, pat) for o in range(4)], paired) == pairs
    # and against the referee: the pairs of the whole region's listing both of whose members are rows
    sites = R.brute_sites(seqs, *P.PATTERNS["n20_nrg"], chrom=0, start=start, end=end)
    row_at = {(r.chromosome, r.protospacer_start, r.strand): r for r in rows}
    want = []
    for l, r, d, o in C.site_pairs_of([(s[0], s[1], s[3]) for s in sites], spec, pat):
        a, b = row_at.get(("chrA", sites[l][1], sites[l][3])), row_at.get(("chrA", sites[r][1], sites[r][3]))
        if a is not None and b is not None:
            want.append((a.guide_id, b.guide_id, str(d), a.strand, b.strand, spec.name_of(o, pat)))
    assert [(ln[1], ln[2], ln[6], ln[7], ln[8], ln[9]) for ln in lines[1:]] == want
    assert all(int(ln[5]) - int(ln[4]) == int(ln[6]) for ln in lines[1:])


def test_the_tools_refuse_pair_flags_without_pairs(tmp_path, genome):
    ctx, names, seqs = genome
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    text, aux = R.pattern_string("n20_nrg")
    five, _ = R.pattern_string("tttv_n20")
    pairs = str(tmp_path / "p.tsv")
    for tool in TOOLS:
        base = tool + ["-r", fa, "--device", "-1", "-c", "chrC"]
        for extra in (["--pair-distance", "0:40"], ["--pair-cut", "17"], ["--pair-orientation", "any"]):
            r = _run(base + ["-i", text] + extra)
            assert r.returncode != 0 and "--pairs" in r.stderr
        r = _run(base + ["-i", text, "--pairs", pairs])
        assert r.returncode != 0 and "--pair-distance" in r.stderr
        for bad in ("40", "40:30", "0:65536", "a:b"):
            r = _run(base + ["-i", text, "--pairs", pairs, "--pair-distance", bad])
            assert r.returncode != 0 and "--pair-distance" in r.stderr
        r = _run(base + ["-i", five, "--pairs", pairs, "--pair-distance", "0:40"])
        assert r.returncode != 0 and "--pair-cut" in r.stderr                   # the default cut is a 3' PAM's
        r = _run(base + ["-i", text, "--pairs", pairs, "--pair-distance", "0:40", "--pair-cut", "21"])
        assert r.returncode != 0 and "--pair-cut" in r.stderr
        r = _run(base + ["-i", text, "--pairs", pairs, "--pair-distance", "0:40", "--pair-orientation", "sideways"])
        assert r.returncode != 0 and "--pair-orientation" in r.stderr
        r = _run(base + ["-i", five, "--pairs", pairs, "--pair-distance", "0:40", "--pair-cut", "18"])
        assert r.returncode == 0, r.stderr
