"""GPU tests of the allele sites (allele_sites.hip): the device against its host twin, byte for byte, and against the referee of
allele_sites_ref.py over every pattern at both lane chunks, on the planted SNVs and on the exhaustive 1 800; SNV lists that end on and
beside the wave and workgroup edges of the prefix, with lanes of no record at a workgroup's ends and a workgroup whose every lane has
the PAM-less maximum; the count call; repeated calls; calls interleaved with the other users of the context's scratch; a reference
with Us; both FindGuides tools on device 0.  Contigs of <= 3 kb; the referee runs once per pattern and SNV set."""
import os
import subprocess
import sys

import numpy as np
import pytest

import allele_sites_ref as A
import sites_ref as R
from fasta_util import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REFEREE = {}


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


def _context(C, chunk, monkeypatch, genome=None, device=0):
    names, seqs = genome or A.genome()
    if chunk is None:
        monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("CALITAS_CHUNK", chunk)
    ctx = C.Context(device)
    ctx.set_reference(names, [s.encode() for s in seqs])
    return ctx, names, seqs


def _referee(C, seqs, name, which):
    """(records, status) of the referee for the planted or the exhaustive SNVs: made once."""
    if (name, which) not in _REFEREE:
        snvs = A.planted_snvs(seqs) if which == "planted" else A.exhaustive_snvs(seqs)
        records, status = A.allele_sites(seqs, name, snvs, key="genome")
        _REFEREE[(name, which)] = (A.as_records(C, records), np.array(status, dtype=np.uint8))
    return _REFEREE[(name, which)]


def _hold(C, ctx, pat, snvs, want=None):
    """The device against the twin, byte for byte, against `want` ((records, status) of the referee) and its own count call."""
    arr = A.snv_array(C, snvs) if isinstance(snvs, list) else snvs
    got = ctx.find_allele_sites(pat, arr)
    twin = ctx.find_allele_sites(pat, arr, host=True)
    assert got.sites.tobytes() == twin.sites.tobytes() and got.status.tobytes() == twin.status.tobytes()
    if want is not None:
        assert got.sites.tobytes() == want[0].tobytes() and got.status.tobytes() == want[1].tobytes()
    n, by, status = ctx.count_allele_sites(pat, arr)
    assert n == len(got) and by.tolist() == np.bincount(got.sites["kind"], minlength=4).tolist() and status.tobytes() == got.status.tobytes()
    return got


@pytest.mark.parametrize("chunk", [None, "512"])
@pytest.mark.parametrize("name", A.NAMES)
def test_device_equals_referee_equals_host_twin(C, name, chunk, monkeypatch):
    ctx, names, seqs = _context(C, chunk, monkeypatch)
    try:
        assert ctx.tile_census()["tile_bases"] == (64 if chunk is None else 512) * 256
        pat = A.pattern_of(C, name)
        planted = _hold(C, ctx, pat, A.planted_snvs(seqs), _referee(C, seqs, name, "planted"))     # not sorted, all three contigs
        assert len(planted) and set(planted.sites["contig_index"].tolist()) == ({1} if name == "fixed_nrg" else {0, 1, 2})   # (FIXED stands on chrB alone)
        _hold(C, ctx, pat, A.exhaustive_snvs(seqs), _referee(C, seqs, name, "exhaustive"))
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_lists_that_end_at_the_edges_of_the_prefix(C, n, monkeypatch):
    ctx, names, seqs = _context(C, None, monkeypatch)
    try:
        snvs = A.exhaustive_snvs(seqs)
        for name in ("n20_nrg", "n20"):
            full, status = _referee(C, seqs, name, "exhaustive")
            for first in (0, 300):                       # from the contig's first base (lanes of few records), and from its inside
                want = full[(full["snv_index"] >= first) & (full["snv_index"] < first + n)].copy()
                want["snv_index"] -= first
                _hold(C, ctx, A.pattern_of(C, name), snvs[first:first + n], (want, status[first:first + n]))
    finally:
        ctx.close()


def test_empty_lanes_at_a_workgroups_ends_and_a_full_workgroup(C, monkeypatch):
    ctx, names, seqs = _context(C, None, monkeypatch)
    try:
        inside = [v for v in A.exhaustive_snvs(seqs) if 100 <= v[1] < 400]
        none = [(0, pos, "", seqs[0][pos]) for pos in range(100, 170)]           # alt is the reference's base: status 3, no record
        # workgroup 0: 70 empty lanes, 186 full ones; workgroup 1: 186 full, 70 empty; workgroup 2: every lane the maximum
        snvs = none + inside[:186] + inside[186:372] + none + inside[372:628]
        assert len(snvs) == 768
        got = _hold(C, ctx, A.pattern_of(C, "n20"), snvs)
        per = np.bincount(got.sites["snv_index"], minlength=len(snvs))
        assert per[:70].sum() == 0 and per[442:512].sum() == 0 and (per[512:] == 2 * A.L).all() and (per[70:442] == 2 * A.L).all()
        assert (got.status[:70] == 3).all() and (got.status[70:442] == 0).all()
        want, status = C.allele_sites_of(seqs, A.pattern_of(C, "n20"), snvs)
        assert got.sites.tobytes() == A.as_records(C, want).tobytes() and got.status.tolist() == status
        _hold(C, ctx, A.pattern_of(C, "n20_nrg"), snvs)
        assert len(_hold(C, ctx, A.pattern_of(C, "n20_nrg"), [])) == 0
    finally:
        ctx.close()


def test_repeated_and_interleaved_calls(C, monkeypatch):
    """Two identical calls return identical bytes, and the calls that share the context's scratch keep theirs."""
    ctx, names, seqs = _context(C, None, monkeypatch)
    try:
        pat = A.pattern_of(C, "n20_nrg")
        snvs = A.snv_array(C, A.planted_snvs(seqs))
        first = ctx.find_allele_sites(pat, snvs)
        again = ctx.find_allele_sites(pat, snvs)
        assert len(first) and first.sites.tobytes() == again.sites.tobytes() and first.status.tobytes() == again.status.tobytes()
        ctx.set_regions(C.Regions([("chrB", 150, 700, "exon"), ("chrA", 0, 400, "utr")]))
        model = C.ActivityModel.zeros(20, 4, 6)
        spec = C.SitePairs(30, 150)
        sites = ctx.find_sites(pat, host=True)
        scored = ctx.find_sites_scored(pat, model, min_score=0, chrom=1, host=True)
        classed = ctx.find_sites_regions(pat, extent=(16, 18), host=True)
        pairs = ctx.find_site_pairs(pat, spec, host=True)
        for _ in range(2):
            assert ctx.find_sites_scored(pat, model, min_score=0, chrom=1)[0].tobytes() == scored[0].tobytes()
            assert ctx.find_allele_sites(pat, snvs).sites.tobytes() == first.sites.tobytes()
            got = ctx.find_sites_regions(pat, extent=(16, 18))
            assert got[0].tobytes() == classed[0].tobytes() and got[1].tobytes() == classed[1].tobytes() and len(got[0])
            assert ctx.count_allele_sites(pat, snvs)[0] == len(first)
            got = ctx.find_site_pairs(pat, spec)
            assert got[0].tobytes() == pairs[0].tobytes() and got[1].tobytes() == pairs[1].tobytes() and len(got[1])
            assert ctx.find_allele_sites(pat, snvs[:300]).sites.tobytes() == first.sites[first.sites["snv_index"] < 300].tobytes()
            assert ctx.find_sites(pat).tobytes() == sites.tobytes()
            assert ctx.find_allele_sites(pat, snvs).sites.tobytes() == first.sites.tobytes()
    finally:
        ctx.close()


def test_a_reference_with_us(C, monkeypatch):
    """The SNVs with a U within reach are decided on the host and merged into place among the kernel's."""
    names, seqs, snvs = A.u_genome()
    ctx, names, seqs = _context(C, None, monkeypatch, genome=(names, seqs))
    try:
        for name in ("n20_nrg", "aux24", "n20"):
            records, status = A.allele_sites(seqs, name, snvs)
            got = _hold(C, ctx, A.pattern_of(C, name), snvs, (A.as_records(C, records), np.array(status, dtype=np.uint8)))
            assert len(got)
    finally:
        ctx.close()


def _run(cmd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)


def test_both_tools_on_the_device(C, tmp_path):
    names, seqs = A.genome()
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    vcf = A.write_vcf(str(tmp_path / "v.vcf"), names, seqs)
    text, aux = R.pattern_string("n20_nrg")
    common = ["-i", text, "-r", fa, "-c", "chrB", "-s", "100", "-e", "1600", "--alleles", vcf]
    out = {}
    for tool, device in (("py", "-1"), ("py", "0"), ("cli", "0")):
        table = str(tmp_path / ("alleles_%s_%s.tsv" % (tool, device)))
        cmd = [sys.executable, "-m", "calitas_amd", "FindGuides"] if tool == "py" else [os.path.join(ROOT, "calitas_amd", "calitas"), "FindGuides"]
        r = _run(cmd + ["--device", device, "--allele-sites", table] + common)
        assert r.returncode == 0, r.stderr
        counts = [ln for ln in r.stderr.splitlines() if ln.startswith("alleles: ")]
        assert len(counts) == 1, r.stderr
        out[(tool, device)] = (r.stdout, open(table).read(), counts[0])
    host = out[("py", "-1")]
    assert len(host[1].splitlines()) > 50 and {ln.split("\t")[5] for ln in host[1].splitlines()[1:]} == {"alt", "ref", "both"}
    assert out[("py", "0")] == host and out[("cli", "0")] == host
