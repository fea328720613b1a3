"""CPU tests of the regions listing: calitas_find_sites_regions_host (the host twin of site_regions.hip's chain, on a host-only context)
against the referee of site_regions_ref.py -- every single-class mask, elsewhere alone, all classes and mixes, the extents {0, L},
{16, 18}, {0, 1} and {L - 1, L}, with and without a site filter, one contig and sub-regions -- the invariants of the contract, the errors
in their order, the counts, the presence table through its hook (kept and invalidated), the Python contract function, find_guides and
guides_tsv, and both FindGuides tools on the host twin (--device -1).  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import site_regions_ref as G
import sites_ref as R
from fasta_util import write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


@pytest.fixture(scope="module")
def genome(C):
    names, seqs = G.genome()
    ctx = C.Context(-1)
    ctx.set_reference(names, [s.encode() for s in seqs])
    ctx.set_regions(G.regions_of(C))
    assert ctx.regions.classes == G.CLASSES
    yield ctx, names, seqs, {}
    ctx.close()


def _sites(genome, name, **region):
    done = genome[3]
    key = (name, tuple(sorted(region.items())))
    if key not in done:
        done[key] = R.brute_sites(genome[2], *G.PATTERNS[name], **region)
    return done[key]


def _hold(C, ctx, names, name, sites, mask, extent, **kw):
    """The listing and the count of one call against the referee; returns the records."""
    cls = G.classes_of(names, sites, extent)
    if not kw:
        G.check_cover(sites, cls, mask)
    want, want_cls, hist = G.expected(sites, cls, mask)
    got, got_cls = ctx.find_sites_regions(G.pattern_of(C, name), classes=mask, extent=extent, host=True, **kw)
    assert R.as_tuples(got) == want
    assert got_cls.tolist() == want_cls
    table = ctx.count_sites_regions(G.pattern_of(C, name), classes=mask, extent=extent, host=True, **kw)
    assert table.tolist() == hist and int(table.sum()) == len(want)
    return got, got_cls


@pytest.mark.parametrize("name", G.NAMES)
def test_the_twin_against_the_referee(C, genome, name):
    ctx, names, seqs, _ = genome
    sites = _sites(genome, name)
    L = len(G.PATTERNS[name][0])
    for extent in G.extents(L):
        for mask in G.MASKS:
            _hold(C, ctx, names, name, sites, mask, extent)


def test_the_planted_places(C, genome):
    """What the intervals were placed for, by the referee: the halo, the boundary, the nesting, the U."""
    ctx, names, seqs, _ = genome
    sites = _sites(genome, "n20_nrg")
    cls = dict(zip([(s[0], s[1], s[3]) for s in sites], G.classes_of(names, sites, None)))
    hi, snp = G.CLASSES.index("hi"), G.CLASSES.index("snp")
    for strand in "+-":
        assert cls[(0, G.SEG - 1, strand)] == hi         # starts in the segment before 8192 and has its class from 8192 + 18, in the next
        assert cls[(0, G.SEG, strand)] == hi             # starts on 8192, reaches 8192 + 19
    one = dict(zip([(s[0], s[1], s[3]) for s in sites], G.classes_of(names, sites, (19, 20))))
    assert one[(0, G.SEG - 1, "+")] == hi and one[(0, G.SEG - 1, "-")] == G.CLASSES.index("edge")   # base 8192 + 18; base 8191
    with_u = [k for k in cls if k[0] == 0 and k[1] <= 12000 < k[1] + 20]
    assert with_u and {cls[k] for k in with_u} >= {0, snp}                 # the U at 12000 lies in protospacers of both kinds
    assert {cls[k] for k in cls if k[0] == 0 and 30131 <= k[1] <= 30150} == {1}
    assert {cls[k] for k in cls if k[0] == 2} == {0}
    assert {cls[k] for k in cls if k[0] == 0 and 2 * G.SEG <= k[1] < 3 * G.SEG - 100} == {0}
    assert {cls[k] for k in cls if k[0] == 0 and 4 * G.SEG <= k[1] < 5 * G.SEG - 20} == {G.CLASSES.index("utr")}


@pytest.mark.parametrize("name", ["n20_nrg", "n32"])
def test_filter_contig_and_sub_regions(C, genome, name):
    ctx, names, seqs, _ = genome
    L = len(G.PATTERNS[name][0])
    import site_filter_ref as F
    keep = C.SiteFilter(gc_min=L // 2 - 2, gc_max=L // 2 + 3, max_run=3)
    sites = _sites(genome, name)
    passing = F.keep(sites, seqs, gc_min=L // 2 - 2, gc_max=L // 2 + 3, max_run=(3, 3, 3, 3))
    assert 0 < len(passing) < len(sites)
    for extent in (None, (L - 1, L)):
        for mask in (G.ALL, G.mask_of(["utr"]), G.mask_of(["elsewhere", "hi"])):
            _hold(C, ctx, names, name, passing, mask, extent, filter=keep)
    for region in (dict(chrom=0, start=G.SEG - 40, end=G.SEG + 60), dict(chrom=1), dict(chrom=0, start=30000, end=30600), dict(chrom=2),
                   dict(start=100, end=8300)):
        part = _sites(genome, name, **{("chrom" if k == "chrom" else k): v for k, v in region.items()})
        for mask in (G.ALL, G.mask_of(["lo", "hi", "edge"]), 1):
            _hold(C, ctx, names, name, part, mask, (0, 1), **region)


def test_invariants(C, genome):
    ctx, names, seqs, _ = genome
    pat = G.pattern_of(C, "n20_nrg")
    plain = ctx.find_sites(pat, host=True)
    for extent in (None, (16, 18)):
        everything, cls = ctx.find_sites_regions(pat, classes=G.ALL, extent=extent, host=True)
        assert everything.tobytes() == plain.tobytes()                      # every bit set: the filtered listing byte for byte
        parts = [ctx.find_sites_regions(pat, classes=m, extent=extent, host=True) for m in (0b00000111, 0b00111000, 0b11000000)]
        assert sum(len(p[0]) for p in parts) == len(plain)
        merged = np.concatenate([p[0] for p in parts])
        order = np.lexsort((merged["strand"] == b"-", merged["protospacer_start"], merged["contig_index"]))
        assert merged[order].tobytes() == plain.tobytes()                   # masks that partition the classes partition the records
        for m, (recs, of) in zip((0b00000111, 0b00111000, 0b11000000), parts):
            assert all((m >> int(k)) & 1 for k in of)
            table = ctx.count_sites_regions(pat, classes=m, extent=extent, host=True)
            hist = np.zeros_like(table)
            np.add.at(hist, (of.astype(int), (recs["strand"] == b"-").astype(int)), 1)
            assert np.array_equal(table, hist) and int(table.sum()) == len(recs)
    # classes=None: every class but elsewhere; bits above n_classes are ignored
    named, _ = ctx.find_sites_regions(pat, host=True)
    same, _ = ctx.find_sites_regions(pat, classes=(G.ALL & ~1) | 0xFFFFFF00, host=True)
    assert named.tobytes() == same.tobytes() and 0 < len(named) < len(plain)
    by_name, _ = ctx.find_sites_regions(pat, classes="exon,snp", host=True)
    by_index, _ = ctx.find_sites_regions(pat, classes=[G.CLASSES.index("exon"), G.CLASSES.index("snp")], host=True)
    assert by_name.tobytes() == by_index.tobytes() and len(by_name)


def _call(C, ctx, pattern, opt, f=None, chrom=-1, start=0, end=0, host=True):
    from calitas_amd import _lib
    g = pattern.to_c()
    out, cls, n = ctypes.POINTER(_lib.SiteT)(), ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    fn = _lib.lib.calitas_find_sites_regions_host if host else _lib.lib.calitas_find_sites_regions
    rc = fn(ctx._h, ctypes.byref(g), ctypes.byref(f) if f is not None else None, ctypes.byref(opt) if opt is not None else None, chrom, start, end,
            ctypes.byref(out), ctypes.byref(cls), ctypes.byref(n))
    msg = _lib.lib.calitas_last_error(ctx._h).decode() if rc else ""
    if rc == 0:
        _lib.lib.calitas_free(out)
        _lib.lib.calitas_free(cls)
    return rc, msg


def test_errors_in_their_order(C, genome):
    from calitas_amd import _lib
    ctx, names, seqs, _ = genome
    pat = G.pattern_of(C, "n20_nrg")
    T = _lib.SiteRegionsT
    bad_filter = C.SiteFilter(gc_min=0, gc_max=255).to_c()
    bad_filter.reserved = 1
    everything_wrong = T(0xFFFFFF00, 5, 5, 7)
    # what calitas_find_sites_filtered refuses comes first: the region, then the filter
    rc, msg = _call(C, ctx, pat, None, chrom=7)
    assert rc == _lib.EINVAL and "chrom_index" in msg
    rc, msg = _call(C, ctx, pat, everything_wrong, f=bad_filter)
    assert rc == _lib.EINVAL and "site filter" in msg
    rc, msg = _call(C, ctx, pat, None)
    assert rc == _lib.EINVAL and "opt" in msg
    bare = C.Context(-1)
    try:
        bare.set_reference(names, [s.encode() for s in seqs])
        rc, msg = _call(C, bare, pat, everything_wrong)
        assert rc == _lib.EINVAL and "no regions" in msg
        rc, msg = _call(C, bare, pat, None)
        assert rc == _lib.EINVAL and "opt" in msg                            # NULL opt before the missing set
        with pytest.raises(C.CalitasError):
            bare.site_presence()
    finally:
        bare.close()
    rc, msg = _call(C, ctx, pat, everything_wrong)
    assert rc == _lib.EINVAL and "class_mask" in msg
    for a, b in ((5, 5), (6, 5), (0, 21), (20, 21), (3, 0)):
        rc, msg = _call(C, ctx, pat, T(2, a, b, 7))
        assert rc == _lib.EINVAL and "ext_from" in msg and "ext_to" in msg, (a, b, msg)
    rc, msg = _call(C, ctx, pat, T(2, 0, 0, 7))
    assert rc == _lib.EINVAL and "reserved" in msg
    for a, b in ((0, 0), (0, 20), (19, 20), (0, 1)):
        assert _call(C, ctx, pat, T(2, a, b, 0))[0] == 0
    # the device call on a host-only context
    rc, msg = _call(C, ctx, pat, T(2, 0, 0, 0), host=False)
    assert rc == _lib.ENODEV


def _segment_of(ctx, names, contig, p):
    from calitas_amd import _lib
    base = ctypes.c_uint64()
    _lib.check(ctx._h, _lib.lib.calitas_contig_packed_base(ctx._h, contig, ctypes.byref(base)))
    assert base.value % G.SEG == 0
    return (base.value + p) // G.SEG


def _check_presence(C, ctx, names, seqs, iv):
    table, first_word = ctx.site_presence()
    assert first_word % 256 == 0
    seg0 = first_word // 256
    # every site of class c under every legal extent starts in a segment whose byte has bit c: the protospacer start p with any
    # extent inside [p, p + L) -- held for every start position and L = 1 .. 32 through the per-base classes (a site's class is one
    # of its bases', or 0 when all of them are 0)
    for ci, (name, seq) in enumerate(zip(names, seqs)):
        col = [0] * len(seq)
        for c, s, e, k in iv:
            if c == name:
                kk = G.CLASSES.index(k)
                for x in range(s, e):
                    if col[x] == 0 or kk < col[x]:
                        col[x] = kk
        col = np.array(col)
        first = _segment_of(ctx, names, ci, 0) - seg0
        n_seg = (len(seq) + G.SEG - 1) // G.SEG
        for b in range(n_seg):
            byte = int(table[first + b])
            lo, hi = b * G.SEG, min(len(seq), (b + 1) * G.SEG)
            reach = set(col[lo:min(len(seq), hi + 31)].tolist())             # what a protospacer of <= 32 bases that starts here can cover
            for k in reach:
                assert (byte >> k) & 1, (name, b, k)
            near = set(col[max(0, lo - G.FOOT):min(len(seq), hi + G.FOOT)].tolist())
            for k in range(len(G.CLASSES)):                                  # farther than the halo from every base of class k: no bit
                assert ((byte >> k) & 1) == int(k in near), (name, b, k)
    return table


def test_the_presence_table(C, genome):
    ctx, names, seqs, _ = genome
    table = _check_presence(C, ctx, names, seqs, G.intervals())
    again, _ = ctx.site_presence()
    assert again.tobytes() == table.tobytes()
    a = _segment_of(ctx, names, 0, 0)
    hi = G.CLASSES.index("hi")
    assert (table[a] >> hi) & 1 and (table[a + 1] >> hi) & 1                 # the hi bases at 8192 + 18 ..: in segment 1, and in segment 0's halo
    snp, utr, edge = (1 << G.CLASSES.index(n) for n in ("snp", "utr", "edge"))
    assert table[a + 2] == 1 | snp                       # nothing but the base at 24576, in its halo
    assert table[a + 4] == 1 | utr | edge                # wholly inside the utr; the halo reaches the contig's last bases
    assert set(table[_segment_of(ctx, names, 2, 0):_segment_of(ctx, names, 2, 0) + 2].tolist()) == {1}


def test_another_set_and_another_reference_make_the_table_again(C):
    names, seqs = G.genome()
    ctx = C.Context(-1)
    try:
        ctx.set_reference(names, [s.encode() for s in seqs])
        ctx.set_regions(G.regions_of(C))
        first = _check_presence(C, ctx, names, seqs, G.intervals())
        other = [("chrC", 100, 200, "cut"), ("chrA", 20000, 20010, "exon")]
        ctx.set_regions(C.Regions(other, classes=G.CLASSES[1:]))
        second = _check_presence(C, ctx, names, seqs, other)
        assert second.tobytes() != first.tobytes()
        pat = G.pattern_of(C, "n20_nrg")
        got, of = ctx.find_sites_regions(pat, classes="exon", host=True)
        assert len(got) and set(got["contig_index"].tolist()) == {0} and all(19981 <= p < 20010 for p in got["protospacer_start"].tolist())
        # another reference drops the set; with the set given again the table is the new reference's
        ctx.set_reference(names[::-1], [s.encode() for s in seqs[::-1]])
        with pytest.raises(C.CalitasError):
            ctx.site_presence()
        ctx.set_regions(G.regions_of(C))
        third = _check_presence(C, ctx, names[::-1], seqs[::-1], G.intervals())
        assert third.tobytes() != first.tobytes() and sorted(third.tolist()) == sorted(first.tolist())
    finally:
        ctx.close()


def test_site_class_of_find_guides_and_guides_tsv(C, genome):
    ctx, names, seqs, _ = genome
    pat = G.pattern_of(C, "n20_nrg")
    regions = ctx.regions
    rows = C.find_guides(ctx, pat, chrom="chrA", start=30000, end=30600, host=True, classes=["cut", "exon", "utr"], extent=(16, 18))
    plain = C.find_guides(ctx, pat, chrom="chrA", start=30000, end=30600, host=True)
    assert 0 < len(rows) < len(plain)
    by_id = {r.guide_id: r for r in plain}
    assert [r.guide for r in rows] == [by_id[r.guide_id].guide for r in rows]            # the kept rows keep their guide_ids
    assert {r.region_class for r in rows} == {1, 2, 3}
    for r in plain:
        k = C.site_class_of(r, regions, (16, 18))
        assert k == G.class_of(r.chromosome, r.protospacer_start, r.strand, 20, (16, 18), G.intervals())
        assert (r.guide_id in {x.guide_id for x in rows}) == (k in (1, 2, 3))
    for r in rows:
        assert r.region_class == C.site_class_of((r.chromosome, r.protospacer_start, r.strand, 20), regions, (16, 18))
    text = C.guides_tsv(rows, class_names=regions.classes)
    lines = text.splitlines()
    head = lines[0].split("\t")
    assert head[head.index("pam_sequence") + 1] == "class" and len(lines) == len(rows) + 1
    assert [ln.split("\t")[head.index("class")] for ln in lines[1:]] == [G.CLASSES[r.region_class] for r in rows]
    # with an activity model: both listings joined on (contig, start, strand); class stands ahead of activity_q16
    model = C.ActivityModel.zeros(20, 4, 6)
    model.gc[:] = [1000 * i for i in range(21)]
    scored = C.find_guides(ctx, pat, chrom="chrA", start=30000, end=30600, host=True, classes=["cut", "exon", "utr"], extent=(16, 18), activity=model)
    assert [r.guide_id for r in scored] == [r.guide_id for r in rows] and [r.region_class for r in scored] == [r.region_class for r in rows]
    alone = {r.guide_id: r.activity_q16 for r in C.find_guides(ctx, pat, chrom="chrA", start=30000, end=30600, host=True, activity=model)}
    assert [r.activity_q16 for r in scored] == [alone[r.guide_id] for r in scored]
    floor = sorted(r.activity_q16 for r in scored)[len(scored) // 2]
    above = C.find_guides(ctx, pat, chrom="chrA", start=30000, end=30600, host=True, classes=["cut", "exon", "utr"], extent=(16, 18), activity=model,
                          min_activity=floor)
    assert [r.guide_id for r in above] == [r.guide_id for r in scored if r.activity_q16 >= floor] and 0 < len(above) < len(scored)
    head = C.guides_tsv(scored, activity=model, class_names=regions.classes).splitlines()[0].split("\t")
    assert head[head.index("pam_sequence") + 1:head.index("pam_sequence") + 3] == ["class", "activity_q16"]


def _bed(path, iv):
    with open(path, "w") as f:
        f.write("# chromosome start end class\n")
        for chrom, s, e, name in iv:
            f.write("%s\t%d\t%d\t%s\n" % (chrom, s, e, name))
        f.write("chrNowhere\t5\t9\texon\n")
    return str(path)


def _run(cmd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)


@pytest.mark.parametrize("flags", [[], ["--classes", "exon,elsewhere"], ["--classes", "hi,lo,edge", "--class-extent", "19:20", "--copies"],
                                   ["--class-extent", "16:18", "--gc-min", "40"]])
def test_both_tools_on_the_host_twin(C, genome, tmp_path, flags):
    ctx, names, seqs, _ = genome
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    bed = _bed(tmp_path / "r.bed", G.intervals())
    text, aux = R.pattern_string("n20_nrg")
    region = ["-c", "chrA", "-s", "8000", "-e", "8400"] if "--copies" in flags else ["-c", "chrA", "-s", "29000", "-e", "31000"]
    common = ["-i", text, "-r", fa, "--device", "-1", "--regions", bed] + region + flags
    py = _run([sys.executable, "-m", "calitas_amd", "FindGuides"] + common)
    assert py.returncode == 0, py.stderr
    assert "1 intervals on chromosomes the reference does not have were skipped" in py.stderr
    lines = py.stdout.splitlines()
    head = lines[0].split("\t")
    assert head[head.index("pam_sequence") + 1] == "class" and len(lines) > 1
    extent = None
    if "--class-extent" in flags:
        a, b = flags[flags.index("--class-extent") + 1].split(":")
        extent = (int(a), int(b))
    wanted = flags[flags.index("--classes") + 1].split(",") if "--classes" in flags else G.CLASSES[1:]
    rows = C.find_guides(ctx, G.pattern_of(C, "n20_nrg"), chrom="chrA", start=int(region[3]), end=int(region[5]), host=True, classes=wanted, extent=extent,
                         filter=C.site_filter_of_flags(20, gc_min=40) if "--gc-min" in flags else None)
    assert [ln.split("\t")[0] for ln in lines[1:]] == [r.guide_id for r in rows]
    assert [ln.split("\t")[head.index("class")] for ln in lines[1:]] == [G.CLASSES[r.region_class] for r in rows]
    if "--classes" in flags:
        assert {ln.split("\t")[head.index("class")] for ln in lines[1:]} <= set(wanted)
    cli = _run([os.path.join(ROOT, "calitas_amd", "calitas"), "FindGuides"] + common)
    assert cli.returncode == 0, cli.stderr
    assert cli.stdout == py.stdout                                           # the same bytes from each


def test_the_tools_refuse_classes_without_regions(tmp_path, genome):
    ctx, names, seqs, _ = genome
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    text, aux = R.pattern_string("n20_nrg")
    for extra in (["--classes", "exon"], ["--class-extent", "0:1"]):
        for tool in ([sys.executable, "-m", "calitas_amd", "FindGuides"], [os.path.join(ROOT, "calitas_amd", "calitas"), "FindGuides"]):
            r = _run(tool + ["-i", text, "-r", fa, "--device", "-1", "-c", "chrA", "-s", "0", "-e", "500"] + extra)
            assert r.returncode != 0 and "--regions" in r.stderr
