"""GPU tests of the site pairs (site_pairs.hip behind sites.hip's two passes): the device against the referee of site_pairs_ref.py and,
byte for byte, against its host twin over the grid of bounds, cut offsets and orientation masks, at both lane chunks; the dense
stretch alone; a filter and sub-regions, which move the records across the workgroups; the count call; repeated calls; calls
interleaved with the other users of the context's scratch; a reference with Us; both FindGuides tools on device 0.  Contigs of <= 3.5 kb;
the referee's double loop runs once per pattern and cut offset."""
import os
import subprocess
import sys

import numpy as np
import pytest

import site_pairs_ref as P
import sites_ref as R
from fasta_util import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = P.L


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


def _context(C, chunk, monkeypatch, genome=None, device=0):
    names, seqs = genome or P.genome()
    if chunk is None:
        monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("CALITAS_CHUNK", chunk)
    monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False)
    ctx = C.Context(device)
    ctx.set_reference(names, [s.encode() for s in seqs])
    return ctx, names, seqs


def _hold(C, ctx, name, seqs, cut, lo, hi, mask, filter=None, referee=True, **region):
    """The device against the twin, byte for byte, the referee, and its own count call; returns (sites, pairs)."""
    pat = P.pattern_of(C, name)
    spec = C.SitePairs(lo, hi, cut, P.codes_of(mask))
    got_sites, got = ctx.find_site_pairs(pat, spec, filter=filter, **region)
    twin_sites, twin = ctx.find_site_pairs(pat, spec, filter=filter, host=True, **region)
    assert got_sites.tobytes() == twin_sites.tobytes() and got.tobytes() == twin.tobytes(), (name, cut, lo, hi, mask, region)
    if referee:
        sites, wide = P.wide_pairs(C, name, seqs, cut, **region)
        assert got_sites.tobytes() == R.as_records(sites, got_sites.dtype).tobytes()
        assert np.array_equal(P.as_rows(got), P.cell(wide, lo, hi, mask)), (name, cut, lo, hi, mask, region)
    n, n_pairs, by = ctx.count_site_pairs(pat, spec, filter=filter, **region)
    assert (n, n_pairs) == (len(got_sites), len(got))
    assert by.tolist() == np.bincount(got["orientation"], minlength=4).tolist()
    return got_sites, got


@pytest.mark.parametrize("chunk", [None, "512"])
@pytest.mark.parametrize("cut", P.CUTS)
@pytest.mark.parametrize("name", P.NAMES)
def test_device_equals_referee_equals_host_twin(C, name, cut, chunk, monkeypatch):
    ctx, names, seqs = _context(C, chunk, monkeypatch)
    try:
        assert ctx.tile_census()["tile_bases"] == (64 if chunk is None else 512) * 256
        for lo, hi in P.BOUNDS:
            for mask in P.MASKS:
                _hold(C, ctx, name, seqs, cut, lo, hi, mask)
    finally:
        ctx.close()


def test_the_dense_stretch_alone(C, monkeypatch):
    """Some 1300 records in five workgroups, a lane with up to 200 partners behind it on both strands, a workgroup's sum of some 4 10^4."""
    ctx, names, seqs = _context(C, None, monkeypatch)
    try:
        sites, pairs = _hold(C, ctx, "n20_nrg", seqs, L - 3, 0, 200, 15, chrom=0, start=P.DENSE[0], end=P.DENSE[1])
        assert len(sites) > 1024 and len(pairs) > 150000
        per_lane = np.bincount(np.minimum(pairs["left"], pairs["right"]), minlength=len(sites))
        assert per_lane.max() > 150 and per_lane[:256].sum() > 40000
    finally:
        ctx.close()


def test_a_filter_and_sub_regions(C, monkeypatch):
    ctx, names, seqs = _context(C, None, monkeypatch)
    try:
        flt = C.SiteFilter(gc_min=6, gc_max=14)
        for name in P.NAMES:
            for lo, hi in P.BOUNDS:
                got_sites, got = _hold(C, ctx, name, seqs, L - 3, lo, hi, 15, filter=flt, referee=False)
                assert 0 < len(got_sites) < len(P.sites_of(name, seqs))
                for mask in (2, 4, 9, 15):
                    _hold(C, ctx, name, seqs, L - 3, lo, hi, mask, chrom=0, start=250, end=3300)
                    _hold(C, ctx, name, seqs, L - 3, lo, hi, mask, chrom=1)
                    _hold(C, ctx, name, seqs, L - 3, lo, hi, mask, chrom=2, start=100, end=130, referee=False)     # room for one footprint
    finally:
        ctx.close()


def test_repeated_and_interleaved_calls(C, monkeypatch):
    """Two identical calls return identical bytes; the records the pairs are made from lie in the scratch find_sites_scored and
    find_sites_regions write their records to, and survive them."""
    ctx, names, seqs = _context(C, None, monkeypatch)
    try:
        pat = P.pattern_of(C, "n20_nrg")
        spec, wide_spec = C.SitePairs(30, 150), C.SitePairs(1000, 3000, orientations="any")
        first = ctx.find_site_pairs(pat, spec)
        again = ctx.find_site_pairs(pat, spec)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and len(first[1])
        twin = ctx.find_site_pairs(pat, spec, host=True)
        assert first[1].tobytes() == twin[1].tobytes()
        wide = ctx.find_site_pairs(pat, wide_spec)
        ctx.set_regions(C.Regions([("chrA", P.PLANTED[0], P.PLANTED[1], "exon"), ("chrB", 0, 400, "utr")]))
        model = C.ActivityModel.zeros(20, 4, 6)
        for _ in range(2):
            scored = ctx.find_sites_scored(pat, model, min_score=0, chrom=1)
            assert scored[0].tobytes() == ctx.find_sites_scored(pat, model, min_score=0, chrom=1, host=True)[0].tobytes()
            got = ctx.find_site_pairs(pat, spec)
            assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes()
            classed = ctx.find_sites_regions(pat, extent=(16, 18))
            assert classed[0].tobytes() == ctx.find_sites_regions(pat, extent=(16, 18), host=True)[0].tobytes() and len(classed[0])
            got = ctx.find_site_pairs(pat, wide_spec)
            assert got[0].tobytes() == wide[0].tobytes() and got[1].tobytes() == wide[1].tobytes()
            assert ctx.count_site_pairs(pat, wide_spec)[:2] == (len(wide[0]), len(wide[1]))
            assert ctx.find_sites(pat).tobytes() == first[0].tobytes()
    finally:
        ctx.close()


def test_a_reference_with_us(C, monkeypatch):
    """A U beside a site: the listing is the host's correction of the kernel's, the pairs the host walk's over it."""
    ctx, names, seqs = _context(C, None, monkeypatch, genome=P.u_genome())
    try:
        for lo, hi in ((0, 40), (30, 150)):
            for mask in (1, 2, 15):
                sites, pairs = _hold(C, ctx, "n20_nrg", seqs, L - 3, lo, hi, mask)
        assert len(sites) >= 6 and len(pairs) > 0
    finally:
        ctx.close()


def _run(cmd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)


def test_both_tools_on_the_device(C, tmp_path):
    names, seqs = P.genome()
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    text, aux = R.pattern_string("n20_nrg")
    common = ["-i", text, "-r", fa, "-c", "chrA", "-s", str(P.DENSE[1] - 200), "-e", str(P.PLANTED[1] + 100), "--gc-max", "70", "--copies", "--pair-distance", "20:160",
              "--pair-orientation", "out,same"]
    out = {}
    for tool, device in (("py", "-1"), ("py", "0"), ("cli", "0")):
        pairs = str(tmp_path / ("pairs_%s_%s.tsv" % (tool, device)))
        cmd = [sys.executable, "-m", "calitas_amd", "FindGuides"] if tool == "py" else [os.path.join(ROOT, "calitas_amd", "calitas"), "FindGuides"]
        r = _run(cmd + ["--device", device, "--pairs", pairs] + common)
        assert r.returncode == 0, r.stderr
        out[(tool, device)] = (r.stdout, open(pairs).read())
    host = out[("py", "-1")]
    assert len(host[1].splitlines()) > 10 and {ln.split("\t")[-1] for ln in host[1].splitlines()[1:]} == {"out", "same"}
    assert out[("py", "0")] == host and out[("cli", "0")] == host
