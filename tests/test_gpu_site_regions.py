"""GPU tests of the regions listing (site_regions.hip behind sites.hip's two passes): the device against the referee of
site_regions_ref.py and, byte for byte, against its host twin over the grid of masks and extents, at both lane chunks; the listing with
the skip off (CALITAS_SITES_SKIP=0); compaction across workgroups that keep everything and workgroups that keep nothing; the count
call, repeated calls and calls interleaved with the other users of the context's scratch; another region set between two listings; both
FindGuides tools on device 0.  Contigs of <= 60 kb; the referee's sites are enumerated once per pattern."""
import os
import subprocess
import sys

import numpy as np
import pytest

import site_regions_ref as G
import sites_ref as R
from fasta_util import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = {None: 64, "512": 512}          # CALITAS_CHUNK -> bases per scan lane: tiles of 16 kb (several per contig) and of 128 kb


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


_done = {}


def _genome():
    if "genome" not in _done:
        _done["genome"] = G.genome()
        assert all(len(s) <= 60000 for s in _done["genome"][1])
    return _done["genome"]


def _sites(name, **region):
    key = (name, tuple(sorted(region.items())))
    if key not in _done:
        _done[key] = R.brute_sites(_genome()[1], *G.PATTERNS[name], **region)
    return _done[key]


def _classes(name, extent):
    key = ("cls", name, extent)
    if key not in _done:
        _done[key] = G.classes_of(_genome()[0], _sites(name), extent)
    return _done[key]


def _context(C, chunk, monkeypatch, device=0):
    names, seqs = _genome()
    if chunk is None:
        monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("CALITAS_CHUNK", chunk)
    monkeypatch.delenv("CALITAS_SITES_SKIP", raising=False)
    ctx = C.Context(device)
    ctx.set_reference(names, [s.encode() for s in seqs])
    ctx.set_regions(G.regions_of(C))
    return ctx


@pytest.mark.parametrize("chunk", [None, "512"])
@pytest.mark.parametrize("name", G.NAMES)
def test_device_equals_referee_equals_host_twin(C, name, chunk, monkeypatch):
    # (512 also with five segments per workgroup, as a genome-sized call has several)
    monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False) if chunk is None else monkeypatch.setenv("CALITAS_SITES_SEGS", "5")
    ctx = _context(C, chunk, monkeypatch)
    try:
        assert ctx.tile_census()["tile_bases"] == CHUNKS[chunk] * 256
        pat = G.pattern_of(C, name)
        sites = _sites(name)
        L = len(G.PATTERNS[name][0])
        for extent in G.extents(L):
            cls = _classes(name, extent)
            for mask in G.MASKS:
                G.check_cover(sites, cls, mask)
                want, want_cls, hist = G.expected(sites, cls, mask)
                got, got_cls = ctx.find_sites_regions(pat, classes=mask, extent=extent)
                assert got.tobytes() == R.as_records(want, got.dtype).tobytes(), (extent, mask)
                assert got_cls.tolist() == want_cls, (extent, mask)
                twin, twin_cls = ctx.find_sites_regions(pat, classes=mask, extent=extent, host=True)
                assert got.tobytes() == twin.tobytes() and got_cls.tobytes() == twin_cls.tobytes()
                assert ctx.count_sites_regions(pat, classes=mask, extent=extent).tolist() == hist
    finally:
        ctx.close()


@pytest.mark.parametrize("chunk", [None, "512"])
def test_the_skip_off_gives_the_same_bytes(C, chunk, monkeypatch):
    monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False)
    ctx = _context(C, chunk, monkeypatch)
    try:
        keep = C.SiteFilter(gc_min=8, gc_max=13, max_run=3)
        for name in G.NAMES:
            pat = G.pattern_of(C, name)
            L = len(G.PATTERNS[name][0])
            for extent in (None, (L - 1, L)):
                for mask in G.MASKS:
                    for flt in (None, keep):
                        monkeypatch.delenv("CALITAS_SITES_SKIP", raising=False)
                        fast = ctx.find_sites_regions(pat, classes=mask, extent=extent, filter=flt)
                        table = ctx.count_sites_regions(pat, classes=mask, extent=extent, filter=flt)
                        monkeypatch.setenv("CALITAS_SITES_SKIP", "0")
                        slow = ctx.find_sites_regions(pat, classes=mask, extent=extent, filter=flt)
                        assert fast[0].tobytes() == slow[0].tobytes() and fast[1].tobytes() == slow[1].tobytes(), (name, extent, mask)
                        assert np.array_equal(table, ctx.count_sites_regions(pat, classes=mask, extent=extent, filter=flt))
                        if flt is None and mask == G.mask_of(["exon", "snp", "hi"]):
                            want = G.expected(_sites(name), _classes(name, extent), mask)
                            assert R.as_tuples(slow[0]) == want[0] and slow[1].tolist() == want[1]
        # with the filter the twin is the witness
        monkeypatch.delenv("CALITAS_SITES_SKIP", raising=False)
        pat = G.pattern_of(C, "n20_nrg")
        for mask in (G.ALL, G.mask_of(["utr"]), 1):
            got = ctx.find_sites_regions(pat, classes=mask, extent=(16, 18), filter=keep)
            twin = ctx.find_sites_regions(pat, classes=mask, extent=(16, 18), filter=keep, host=True)
            assert len(got[0]) and got[0].tobytes() == twin[0].tobytes() and got[1].tobytes() == twin[1].tobytes()
    finally:
        ctx.close()


def test_compaction_across_workgroups_and_contigs(C, monkeypatch):
    """The PAM-less pattern has a record at nearly every base on both strands: some 140 000 records, 550 workgroups of the class kernel.
    With the utr class alone the workgroups over chrA's segment 4 keep every record and most others none; with elsewhere alone it is
    the other way round; sub-regions and single contigs move the workgroups' boundaries."""
    monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False)
    ctx = _context(C, None, monkeypatch)
    try:
        pat = G.pattern_of(C, "n32")
        sites, cls = _sites("n32"), _classes("n32", None)
        utr = G.CLASSES.index("utr")
        for k in (utr, 0):
            flags = np.array([c == k for c in cls])
            blocks = [flags[i:i + 256] for i in range(0, len(flags) - 255, 256)]
            assert any(b.all() for b in blocks) and any(not b.any() for b in blocks) and any(b.any() and not b.all() for b in blocks)
            want = G.expected(sites, cls, 1 << k)
            got = ctx.find_sites_regions(pat, classes=1 << k)
            assert got[0].tobytes() == R.as_records(want[0], got[0].dtype).tobytes() and got[1].tolist() == want[1]
        for region in (dict(chrom=0, start=4 * G.SEG - 300, end=5 * G.SEG + 40), dict(chrom=1), dict(chrom=2), dict(start=8000, end=17000)):
            part = _sites("n32", **region)
            part_cls = G.classes_of(_genome()[0], part, (31, 32))
            for mask in (G.ALL, G.mask_of(["utr", "edge"]), 1, G.mask_of(["lo", "hi"])):
                want = G.expected(part, part_cls, mask)
                got = ctx.find_sites_regions(pat, classes=mask, extent=(31, 32), **region)
                assert R.as_tuples(got[0]) == want[0] and got[1].tolist() == want[1], (region, mask)
                assert ctx.count_sites_regions(pat, classes=mask, extent=(31, 32), **region).tolist() == want[2]
    finally:
        ctx.close()


def test_calls_interleaved_on_one_context_and_another_set(C, monkeypatch):
    """The presence table and SitesWork's shared buffers survive the other calls of the context; another region set makes the table
    again."""
    monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False)
    ctx = _context(C, None, monkeypatch)
    try:
        names, seqs = _genome()
        pat = G.pattern_of(C, "n20_nrg")
        sites = _sites("n20_nrg")
        mask = G.mask_of(["exon", "snp", "hi", "edge"])
        want = G.expected(sites, _classes("n20_nrg", (16, 18)), mask)
        plain = R.as_records(sites, np.dtype(C.aligner.SITE_DTYPE)).tobytes()
        model = C.ActivityModel.zeros(20, 4, 6)
        guide = C.Guide(seqs[0][30110:30130].upper() + "nrg")
        params = C.make_params(max_gaps_between_guide_and_pam=2)

        def listing():
            got = ctx.find_sites_regions(pat, classes=mask, extent=(16, 18))
            assert R.as_tuples(got[0]) == want[0] and got[1].tolist() == want[1]
            assert ctx.count_sites_regions(pat, classes=mask, extent=(16, 18)).tolist() == want[2]

        listing()
        listing()
        assert ctx.find_sites(pat).tobytes() == plain
        listing()
        scored = ctx.find_sites_scored(pat, model, min_score=0)
        assert scored[0].tobytes() == ctx.find_sites_scored(pat, model, min_score=0, host=True)[0].tobytes()
        listing()
        queries = [seqs[0][100:120].upper().replace("U", "T"), seqs[1][5000:5020].upper()]
        assert np.array_equal(ctx.count_near(pat, queries, 2), ctx.count_near(pat, queries, 2, host=True))
        listing()
        first = ctx.search_regions(guide, params, C.ScoreModel.uniform(20), 4)
        listing()
        assert ctx.search_regions(guide, params, C.ScoreModel.uniform(20), 4) == first
        assert ctx.find_sites(pat).tobytes() == plain
        # another set: the same class names, other intervals
        other = [("chrC", 100, 200, "cut"), ("chrA", 20000, 20010, "exon"), ("chrA", 8190, 8194, "snp")]
        ctx.set_regions(C.Regions(other, classes=G.CLASSES[1:]))
        other_named = [(c, s, e, k) for c, s, e, k in other]
        for m in (G.mask_of(["cut"]), G.mask_of(["exon", "snp"]), 1, G.ALL):
            cls = G.classes_of(names, sites, (0, 1), iv=other_named)
            w = G.expected(sites, cls, m)
            got = ctx.find_sites_regions(pat, classes=m, extent=(0, 1))
            assert R.as_tuples(got[0]) == w[0] and got[1].tolist() == w[1] and len(w[0])
        ctx.set_regions(G.regions_of(C))
        listing()
    finally:
        ctx.close()


def _run(cmd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.pop("CALITAS_SITES_SKIP", None)
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)


def test_both_tools_on_the_device(C, tmp_path):
    names, seqs = _genome()
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    bed = str(tmp_path / "r.bed")
    with open(bed, "w") as f:
        for chrom, s, e, name in G.intervals():
            f.write("%s\t%d\t%d\t%s\n" % (chrom, s, e, name))
    text, aux = R.pattern_string("n20_nrg")
    common = ["-i", text, "-r", fa, "--regions", bed, "--classes", "hi,lo,edge,cut", "--class-extent", "16:18", "-c", "chrA", "--copies"]
    host = _run([sys.executable, "-m", "calitas_amd", "FindGuides", "--device", "-1"] + common)
    assert host.returncode == 0, host.stderr
    lines = host.stdout.splitlines()
    head = lines[0].split("\t")
    assert head[head.index("pam_sequence") + 1:head.index("pam_sequence") + 3] == ["class", "copies"]
    assert {ln.split("\t")[head.index("class")] for ln in lines[1:]} == {"hi", "lo", "edge", "cut"}
    py = _run([sys.executable, "-m", "calitas_amd", "FindGuides", "--device", "0"] + common)
    assert py.returncode == 0, py.stderr
    assert py.stdout == host.stdout
    cli = _run([os.path.join(ROOT, "calitas_amd", "calitas"), "FindGuides", "--device", "0"] + common)
    assert cli.returncode == 0, cli.stderr
    assert cli.stdout == host.stdout
