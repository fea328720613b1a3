"""GPU tests of the site filters (sites.hip's FILTER instantiations): the device against its host twin and against the referee of
site_filter_ref.py, as record bytes and as counts per contig and strand, on the planted genome and on the seam genomes of
test_gpu_sites.py (whose brute force is shared, not repeated); regions, an absent contig, the unfiltered call around a filtered one,
find_guides with a filter in front of the search, FindGuides --counts with the flags, and the parameter sweep of
site_filter_ref.sweep_sets (every protospacer length, every bound) against the referee's masks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import site_filter_ref as F
import sites_ref as R
import test_gpu_sites as S
from fasta_util import write_fasta

pytestmark = pytest.mark.gpu

ROOT = S.ROOT
N20 = "NNNNNNNNNNNNNNNNNNNNnrg"
SEAM_PATTERNS = ["n20_nrg", "tttv_n20", "five16_L32", "n21"]
PLANTED_PATTERNS = SEAM_PATTERNS + ["eight_pams", "n20_nngrrt_nrg"]


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


_planted = {}


def _planted_genome():
    if not _planted:
        names, seqs, planted = F.filter_genome()
        _planted.update(names=names, seqs=seqs, planted=planted, sites={})
    return _planted


def _planted_sites(name):
    g = _planted_genome()
    if name not in g["sites"]:
        g["sites"][name] = R.brute_sites(g["seqs"], *R.PATTERNS[name])
    return g["sites"][name]


def _check(C, ctx, names, seqs, sites, name, min_each_way, **region):
    """Under each of the five filters: device listing == referee == host twin as bytes, and the counts per contig and strand.
    region: chrom, start, end of every call (`sites` is the brute force of that region)."""
    pat = S._pattern(C, name)
    plain = ctx.find_sites(pat, **region)
    assert plain.tobytes() == R.as_records(sites, plain.dtype).tobytes()
    for fname, flt in F.filters(len(R.PATTERNS[name][0])).items():
        want = F.keep(sites, seqs, **flt)
        print(name, fname, "sites", len(sites), "kept", len(want), "share %.3f" % (len(want) / len(sites)))
        # the referee itself rejects and keeps: a filter that does nothing, or everything, cannot pass
        assert len(want) >= min_each_way and len(sites) - len(want) >= min_each_way, (name, fname)
        keep = C.SiteFilter(**flt)
        got = ctx.find_sites(pat, filter=keep, **region)
        assert len(got) == len(want) and got.tobytes() == R.as_records(want, got.dtype).tobytes(), (name, fname)
        assert got.tobytes() == ctx.find_sites(pat, host=True, filter=keep, **region).tobytes(), (name, fname)
        n, table = ctx.count_sites(pat, filter=keep, **region)
        hist = np.zeros((len(names), 2), dtype=np.uint64)
        for w in want:
            hist[w[0], int(w[3] == "-")] += 1
        assert n == len(want) and np.array_equal(table, hist), (name, fname)
    assert ctx.find_sites(pat, filter=C.SiteFilter(), **region).tobytes() == plain.tobytes()     # the open filter through the FILTER kernels
    assert ctx.find_sites(pat, **region).tobytes() == plain.tobytes()                            # the filter on the device does not stick


@pytest.mark.parametrize("name", PLANTED_PATTERNS)
def test_planted_genome(C, name, monkeypatch):
    monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False)
    g = _planted_genome()
    ctx = C.Context(0)
    try:
        ctx.set_reference(g["names"], [s.encode() for s in g["seqs"]])
        sites = _planted_sites(name)
        if name == "n20_nrg":
            F.check_planted(g["seqs"], g["planted"], sites)
            # the planted cases one by one, each under its own filter
            filters = dict(F.filters(20), **F.EXTRA)
            for fname in sorted({p[3] for p in g["planted"]}):
                got = ctx.find_sites(N20, filter=C.SiteFilter(**filters[fname]))
                listed = {(int(s["protospacer_start"]), s["strand"].decode()) for s in got}
                for case, strand, p, f, kept in g["planted"]:
                    if f == fname:
                        assert ((p, strand) in listed) == kept, (case, strand, p)
                assert R.as_tuples(got) == F.keep(sites, g["seqs"], **filters[fname]), fname
        _check(C, ctx, g["names"], g["seqs"], sites, name, 50 if name == "n20_nrg" else 1)
    finally:
        ctx.close()


def test_long_and_asymmetric_motifs(C, monkeypatch):
    """The motif paths the five filters do not take: a motif as long as the protospacer (an occurrence window of one position), motifs
    of more than eight letters (the second word of letter sets, which reaches chain word 3), sixteen letters in a protospacer of 32, and
    non-palindromic motifs with IUPAC letters, whose reverse complement on '-' is another string.  Device == referee == host twin."""
    monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False)
    g = _planted_genome()
    seqs = g["seqs"]
    ctx = C.Context(0)
    try:
        ctx.set_reference(g["names"], [s.encode() for s in seqs])
        n8 = R.brute_sites(seqs, "NNNNNNNN", ["ngg"], False)
        n12 = R.brute_sites(seqs, "NNNNNNNNNNNN", ["ngg"], False)
        cases = [("NNNNNNNNngg", n8, ("SWNNNNKN",)), ("NNNNNNNNngg", n8, ("NNSWNNNA",)), ("NNNNNNNNngg", n8, ("WNNNNNNS",)),
                 ("NNNNNNNNNNNNngg", n12, ("RNNNNNNNNNNY",)), ("NNNNNNNNNNNNngg", n12, ("NNNNNNNNNSWB",)),      # L letters, more than eight
                 (S._pattern(C, "five16_L32"), _planted_sites("five16_L32"), ("NNNNNNNNNNNNCGSW",)),
                 (S._pattern(C, "five16_L32"), _planted_sites("five16_L32"), ("MNNNNNNNNNKNB", "ARYB")),
                 (N20, _planted_sites("n20_nrg"), ("ARYB",)), (N20, _planted_sites("n20_nrg"), ("VRYT",)),       # each other's reverse complement
                 (N20, _planted_sites("n20_nrg"), ("GACNNNNNNNNR", "HGG", "ARYB"))]
        kept_by = {}
        for pat, sites, avoid in cases:
            want = F.keep(sites, seqs, avoid=avoid)
            print(avoid, "sites", len(sites), "kept", len(want))
            assert 0 < len(want) < len(sites), avoid
            keep = C.SiteFilter(avoid=avoid)
            got = ctx.find_sites(pat, filter=keep)
            assert got.tobytes() == R.as_records(want, got.dtype).tobytes(), avoid
            assert got.tobytes() == ctx.find_sites(pat, host=True, filter=keep).tobytes(), avoid
            assert ctx.count_sites(pat, filter=keep)[0] == len(want), avoid
            kept_by[avoid] = want
        assert kept_by[("ARYB",)] != kept_by[("VRYT",)]             # the orientation matters
    finally:
        ctx.close()


@pytest.mark.parametrize("chunk", [None, "512"])
@pytest.mark.parametrize("name", SEAM_PATTERNS)
def test_seam_genomes(C, name, chunk, monkeypatch):
    # (as the site tests: 512 also with five segments per workgroup)
    monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False) if chunk is None else monkeypatch.setenv("CALITAS_SITES_SEGS", "5")
    ctx = S._context(C, chunk, monkeypatch)
    try:
        names, seqs, _ = S._genome(chunk)
        census = ctx.tile_census()
        assert census["tile_bases"] == S.CHUNKS[chunk] * 256
        if chunk is None:
            assert census["dead"] >= 1
        if name == "n21":
            # every position is a site on both strands: the first 12 kb of chrA, which hold the word-boundary offsets, the lane-chunk
            # edge and the workgroup edge at 8192 (the referee takes a second per 10 000 sites)
            region = dict(chrom=0, start=0, end=12000)
            _check(C, ctx, names, seqs, R.brute_sites(seqs, *R.PATTERNS[name], **region), name, 1, **region)
        else:
            _check(C, ctx, names, seqs, S._want(chunk, name), name, 50 if name == "n20_nrg" else 1)
    finally:
        ctx.close()


def test_regions_and_an_absent_contig(C, monkeypatch):
    monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False)
    ctx = S._context(C, None, monkeypatch)
    try:
        names, seqs, _ = S._genome(None)
        flt = F.filters(20)["all"]
        keep = C.SiteFilter(**flt)
        for a, b in ((3999, 5417), (8181, 8204), (8100, 8300), (16000, 0), (4097, 4127)):
            want = F.keep(R.brute_sites(seqs, *R.PATTERNS["n20_nrg"], chrom=0, start=a, end=b), seqs, **flt)
            got = ctx.find_sites(N20, chrom="chrA", start=a, end=b or None, filter=keep)
            assert R.as_tuples(got) == want, (a, b)
            n, table = ctx.count_sites(N20, chrom=0, start=a, end=b or None, filter=keep)
            assert n == len(want) and int(table[0].sum()) == n and int(table.sum()) == n
        assert len(F.keep(R.brute_sites(seqs, *R.PATTERNS["n20_nrg"], chrom=0, start=3999, end=5417), seqs, **flt)) > 10
    finally:
        ctx.close()
    import random
    ctx = C.Context(0)
    try:
        rng = random.Random(5)
        seq = "".join(rng.choice("ACGT") for _ in range(5000))
        ctx.set_reference(["here", "away", "there"], [seq.encode(), None, seq[::-1].encode()], lengths=[5000, 40000, 5000])
        flt = F.filters(20)["all"]
        want = F.keep(R.brute_sites([seq, None, seq[::-1]], *R.PATTERNS["n20_nrg"], chrom=2), [seq, None, seq[::-1]], **flt)
        assert R.as_tuples(ctx.find_sites(N20, chrom="there", filter=C.SiteFilter(**flt))) == want and want
        for chrom in ("away", None):
            errors = []
            for kw in (dict(), dict(filter=C.SiteFilter(**flt))):
                with pytest.raises(C.CalitasError) as e:
                    ctx.find_sites(N20, chrom=chrom, **kw)
                errors.append((e.value.code, str(e.value)))
                with pytest.raises(C.CalitasError):
                    ctx.count_sites(N20, chrom=chrom, **kw)
            assert errors[0] == errors[1] and errors[0][0] == C._lib.EINVAL
    finally:
        ctx.close()


def test_find_guides_filters_before_the_search(C, monkeypatch):
    """find_guides(filter=...) hands the search the kept guides and no others."""
    monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    names, seqs = S._acgt_n_genome()
    ctx = C.Context(0)
    try:
        ctx.set_reference(names, [s.encode() for s in seqs])
        flt = F.filters(20)["gc"]
        region = dict(chrom="g1", start=2450, end=2700)
        sites = R.brute_sites(seqs, *R.PATTERNS["n20_nrg"], chrom=0, start=2450, end=2700)
        want = F.keep(sites, seqs, **flt)
        rows = C.find_guides(ctx, N20, filter=C.SiteFilter(**flt), **region)
        assert [(r.protospacer_start, r.strand) for r in rows] == [(w[1], w[3]) for w in want] and 0 < len(want) < len(sites)
        searched = []
        batch = ctx.search_counts_batch
        monkeypatch.setattr(ctx, "search_counts_batch", lambda guides, params: searched.extend(g.guide for g in guides) or batch(guides, params))
        params = C.make_params(max_guide_diffs=1)
        tables = C.guide_counts(ctx, [r.guide for r in rows], params)
        assert sorted(searched) == sorted({F.protospacer(w, seqs) for w in want})
        plain = C.find_guides(ctx, N20, **region)
        unfiltered = C.guide_counts(ctx, [r.guide for r in plain], params)
        assert set(tables) < set(unfiltered) and all(np.array_equal(tables[g], unfiltered[g]) for g in tables)
    finally:
        ctx.close()


def test_find_guides_tool_counts_with_the_flags(C, tmp_path):
    """FindGuides --counts --gc-min 40 --gc-max 60: the referee's rows, each with the counts columns the unfiltered run has for the
    same guide_id; both tools agree on the plain filtered table."""
    names, seqs = S._acgt_n_genome()
    fa = write_fasta(str(tmp_path / "t.fa"), list(zip(names, seqs)))
    env = dict(os.environ, PYTHONPATH=ROOT)
    region = ["-r", fa, "-i", N20, "-c", "g1", "-s", "2450", "-e", "2700"]
    flags = ["--gc-min", "40", "--gc-max", "60"]
    out = {k: str(tmp_path / (k + ".tsv")) for k in ("all", "kept", "py", "cc")}
    tool = [sys.executable, "-m", "calitas_amd", "FindGuides"]
    subprocess.run(tool + ["-o", out["all"], "--counts", "-d", "1"] + region, check=True, env=env, cwd=ROOT, timeout=300)
    subprocess.run(tool + ["-o", out["kept"], "--counts", "-d", "1"] + region + flags, check=True, env=env, cwd=ROOT, timeout=300)
    subprocess.run(tool + ["-o", out["py"]] + region + flags, check=True, env=env, cwd=ROOT, timeout=300)
    subprocess.run([os.path.join(ROOT, "calitas_amd", "calitas"), "FindGuides", "-o", out["cc"]] + region + flags, check=True, timeout=300)
    assert open(out["py"], "rb").read() == open(out["cc"], "rb").read()
    every = [ln.split("\t") for ln in open(out["all"]).read().splitlines()]
    kept = [ln.split("\t") for ln in open(out["kept"]).read().splitlines()]
    sites = R.brute_sites(seqs, *R.PATTERNS["n20_nrg"], chrom=0, start=2450, end=2700)
    want = F.keep(sites, seqs, gc_min=8, gc_max=12)
    ids = ["g1:%d:%s" % (min(w[1], w[2]), w[3]) for w in want]
    assert kept[0] == every[0] and [f[0] for f in kept[1:]] == ids and 0 < len(ids) < len(every) - 1
    by_id = {f[0]: f for f in every[1:]}
    assert all(f == by_id[f[0]] for f in kept[1:])
    assert [ln.split("\t") for ln in open(out["py"]).read().splitlines()] == [f[:8] for f in kept]


# ---- the parameter sweep (site_filter_ref.sweep_sets): every protospacer length, every bound at which a verdict can change ----
# The host twin is held against the same masks in test_site_filters_host.py and is not called again here.

SWEEP_PARTS = [(kind, half) for kind in F.SWEEP_KINDS if kind != "with_pam" for half in ((1, 16), (17, 32))] + [("with_pam", (1, 32))]


@pytest.fixture(scope="module")
def sweep_referee():
    """The referee's listings of every sweep pattern, check_sweep asserted on each length: made before anything of the library runs."""
    F.check_motif_strings()
    return {(L, pam): F.checked_listing(L, pam) for L, pam in [(L, None) for L in F.SWEEP_LENGTHS] + [(L, pam) for L in F.PAM_LENGTHS for pam in F.PAM_PATTERNS]}


@pytest.mark.parametrize("kind,half", SWEEP_PARTS, ids=["%s-%d-%d" % (k, h[0], h[1]) for k, h in SWEEP_PARTS])
def test_sweep_device(C, sweep_referee, kind, half, monkeypatch):
    """Per parameter set: the device listing == plain[mask] as bytes, count_sites gives len(plain[mask]), and its table per strand the
    mask's counts per strand."""
    monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False)
    names, seqs = F.sweep_genome()
    sets = [s for s in F.sweep_sets(kind) if half[0] <= s[0] <= half[1]]
    ctx = C.Context(0)
    try:
        ctx.set_reference(names, [s.encode() for s in seqs])
        plains, each_way = {}, 0
        for L, pam, flt in sets:
            ls = sweep_referee[(L, pam)]
            if (L, pam) not in plains:
                got = ctx.find_sites(ls.pattern)
                plains[(L, pam)] = R.as_records(ls.sites, got.dtype)
                assert got.tobytes() == plains[(L, pam)].tobytes(), (L, pam, F.first_difference(got.tolist(), plains[(L, pam)].tolist()))
            plain = plains[(L, pam)]
            mask = ls.mask(**flt)
            want = plain[mask]
            keep = C.SiteFilter(**flt)
            got = ctx.find_sites(ls.pattern, filter=keep)
            assert got.tobytes() == want.tobytes(), (L, pam, flt, F.first_difference(got.tolist(), want.tolist()))
            n, table = ctx.count_sites(ls.pattern, filter=keep)
            minus = int((mask & ls.features.minus).sum())
            assert n == len(want) and table.tolist() == [[len(want) - minus, minus]], (L, pam, flt, n, table.tolist(), len(want), minus)
            each_way += 0 < len(want) < len(plain)
        print(kind, half, "sets", len(sets), "that keep and reject", each_way)
        assert each_way > len(sets) // 2
    finally:
        ctx.close()
