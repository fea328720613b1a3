"""GPU tests of the guide-site enumeration (sites.hip): the kernel against its host twin and against the brute force of sites_ref.py on
genomes built to hit the kernel's seams, dense output across many workgroups, regions, the search engine as a second witness, and
both FindGuides tools.  Contigs of <= 60 kb; the brute force of a genome is computed once per module."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import sites_ref as R
from fasta_util import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# CALITAS_CHUNK (bases per scan lane, read when the reference is packed) -> the lane it gives; None: what the packer picks for a genome
# of this size, 64 -- tiles of 16 kb, so that a contig of <= 60 kb spans several and can hold a dead one; 512: one tile per contig
CHUNKS = {None: 64, "512": 512}


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


_cache = {}


def _genome(chunk):
    """(names, strings, {pattern: brute force}) for a lane chunk; built and enumerated once."""
    lane = CHUNKS[chunk]
    if lane not in _cache:
        names, seqs = R.gpu_genome(1234 + lane, lane * 256, lane)
        assert all(len(s) <= 60000 for s in seqs)
        _cache[lane] = (names, seqs, {})
    return _cache[lane]


def _want(chunk, name):
    names, seqs, done = _genome(chunk)
    if name not in done:
        done[name] = R.brute_sites(seqs, *R.PATTERNS[name])
    return done[name]


def _pattern(C, name):
    text, aux = R.pattern_string(name)
    return C.Guide(text, aux)


def _context(C, chunk, monkeypatch, device=0):
    names, seqs, _ = _genome(chunk)
    if chunk is None:
        monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("CALITAS_CHUNK", chunk)
    ctx = C.Context(device)
    ctx.set_reference(names, [s.encode() for s in seqs])
    return ctx


@pytest.mark.parametrize("chunk", [None, "512"])
@pytest.mark.parametrize("name", sorted(R.PATTERNS))
def test_device_equals_host_twin_equals_brute_force(C, name, chunk, monkeypatch):
    # (512 also with five segments per workgroup, as a genome-sized call has several)
    monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False) if chunk is None else monkeypatch.setenv("CALITAS_SITES_SEGS", "5")
    ctx = _context(C, chunk, monkeypatch)
    try:
        names, seqs, _ = _genome(chunk)
        census = ctx.tile_census()
        assert census["tile_bases"] == CHUNKS[chunk] * 256
        if chunk is None:
            assert census["dead"] >= 1                  # chrB's N run covers a tile and its halos: the kernel skips it
        want = _want(chunk, name)
        got = ctx.find_sites(_pattern(C, name))
        twin = ctx.find_sites(_pattern(C, name), host=True)
        print(name, chunk, "sites", len(want))
        assert R.as_tuples(got) == want
        assert got.tobytes() == twin.tobytes()
        if name == "fixed_nrg":
            # the planted copies: 47 + 22 around word boundaries, 12 around the chunk / workgroup / tile edges, those at the N runs, the U,
            # the contig's first and last base, chrB's two and the 26-base contig's one; the R copy is not among them
            on_a = {(p, s) for c, p, _, s, _, _, _ in want if c == 0}
            assert len(want) >= 47 + 22 + 12 + 2 + 1 + 2 + 1
            assert (13000, "+") not in on_a and (13100, "+") in on_a
            assert (12050, "+") in on_a and (12336, "-") in on_a and (0, "+") in on_a and (len(seqs[0]) - 20, "-") in on_a
        n, table = ctx.count_sites(_pattern(C, name))
        assert n == len(want)
        hist = np.zeros((len(names), 2), dtype=np.uint64)
        for s in want:
            hist[s[0], int(s[3] == "-")] += 1
        assert np.array_equal(table, hist)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["eight_pams", "five_prime_eight"])
def test_every_pam_index_wins_on_both_strands(C, name, monkeypatch):
    """Eight PAMs: each of the indices 0 to 7 -- every combination of the three bit-planes sites_kernel keeps the winner in -- is the
    first matching PAM somewhere on both strands (by the brute force), and the device's records carry index and PAM length there."""
    monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False)
    proto, pams, five = R.PATTERNS[name]
    want = _want(None, name)
    classes = {}
    for w in want:
        classes[(w[3], w[4])] = classes.get((w[3], w[4]), 0) + 1
    print(name, "sites", len(want), "smallest class", min(classes.values()))
    assert len(pams) == 8 and set(classes) == {(s, k) for s in "+-" for k in range(8)}
    ctx = _context(C, None, monkeypatch)
    try:
        got = ctx.find_sites(_pattern(C, name))
        assert R.as_tuples(got) == want
        seen = {}
        for s in got:
            key = (s["strand"].decode(), int(s["pam_index"]))
            seen[key] = seen.get(key, 0) + 1
            assert int(s["pam_length"]) == len(pams[key[1]])
        assert seen == classes
    finally:
        ctx.close()


def _launch_segments(C, ctx, seqs):
    """Segments of 256 words (8192 bases) a call over every contig launches, as calitas_find_sites_impl works them out: from the first
    contig's first word, rounded down to a segment, to the last contig's last word."""
    import ctypes
    g = ctypes.c_uint64()
    base = []
    for i in (0, len(seqs) - 1):
        C._lib.check(ctx._h, C._lib.lib.calitas_contig_packed_base(ctx._h, i, ctypes.byref(g)))
        base.append(g.value)
    w0, w1 = base[0] // 32, (base[1] + len(seqs[-1]) + 31) // 32
    w0 -= w0 % 256
    return (w1 - w0 + 255) // 256


@pytest.mark.parametrize("n_contigs, per", [(70, 2), (140, 3)])
def test_many_segments_through_the_offsets_scan(C, monkeypatch, n_contigs, per):
    """More segments than sites_offsets_kernel has threads: with a tile per contig (lane chunk 512: 16 segments a tile) 70 contigs are
    more than 1024 segments, two counts per thread, and 140 more than 2048, three per thread -- stretches that straddle tiles, the
    clamp at n and threads whose stretch lies wholly past n.  Listing and counts against the brute force and the host twin, for one PAM,
    eight PAMs and the dense pattern (every segment of a contig counts), and once with 16 segments per workgroup."""
    monkeypatch.setenv("CALITAS_CHUNK", "512")
    monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False)
    names, seqs = R.many_contigs(500 + n_contigs, n_contigs)
    ctx = C.Context(0)
    try:
        ctx.set_reference(names, [s.encode() for s in seqs])
        census = ctx.tile_census()
        n_segs = _launch_segments(C, ctx, seqs)
        print(n_contigs, "contigs", sum(len(s) for s in seqs), "bases", census["tiles"], "tiles", n_segs, "segments, per", -(-n_segs // 1024))
        assert census["tile_bases"] == 512 * 256
        assert 1024 * (per - 1) < n_segs <= 1024 * per
        for pat, spec in (("n20_nrg", R.PATTERNS["n20_nrg"]), ("eight_pams", R.PATTERNS["eight_pams"]), ("NNNNn", ("NNNN", ["n"], False))):
            want = R.brute_sites(seqs, *spec)
            G = _pattern(C, pat) if pat in R.PATTERNS else C.Guide(pat)
            got = ctx.find_sites(G)
            print(pat, "sites", len(want))
            assert len(want) > 1000 and len({w[0] for w in want}) == n_contigs
            # neighbouring segments that both count something: a thread's stretch with more than one non-zero count
            assert {w[0] for w in want if w[1] < 8192} & {w[0] for w in want if 8192 <= w[1] < 16384}
            assert len(got) == len(want) and got.tobytes() == R.as_records(want, got.dtype).tobytes(), pat
            assert got.tobytes() == ctx.find_sites(G, host=True).tobytes(), pat
            hist = np.zeros((n_contigs, 2), dtype=np.uint64)
            for w in want:
                hist[w[0], int(w[3] == "-")] += 1
            n, table = ctx.count_sites(G)
            assert n == len(want) and np.array_equal(table, hist), pat
            if pat == "eight_pams":
                monkeypatch.setenv("CALITAS_SITES_SEGS", "16")
                assert ctx.find_sites(G).tobytes() == got.tobytes()
                monkeypatch.delenv("CALITAS_SITES_SEGS")
    finally:
        ctx.close()


@pytest.mark.parametrize("segs", [None, "3", "16"])
def test_dense_output_across_many_workgroups(C, monkeypatch, segs):
    """NNNN + n: every clean position is a site on both strands -- more than 1e5 records from two contigs, whose offsets run across
    a dozen segments; two calls return the same bytes.  segs: segments per workgroup (CALITAS_SITES_SEGS; a region of this size takes
    one per workgroup, a genome sixteen) -- 3 leaves the last workgroup short, 16 walks a workgroup across padding into the next contig."""
    if segs is None:
        monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False)
    else:
        monkeypatch.setenv("CALITAS_SITES_SEGS", segs)
    rng = random.Random(99)
    seqs = ["".join(rng.choice("ACGT") for _ in range(n)) for n in (33001, 21013)]
    seqs[1] = seqs[1][:9000] + "N" * 70 + seqs[1][9070:15000] + "r" + seqs[1][15001:]
    monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    ctx = C.Context(0)
    try:
        ctx.set_reference(["d1", "d2"], [s.encode() for s in seqs])
        want = R.brute_sites(seqs, "NNNN", ["n"], False)
        assert len(want) > 100000
        a = ctx.find_sites("NNNNn")
        b = ctx.find_sites("NNNNn")
        assert R.as_tuples(a) == want
        assert a.tobytes() == b.tobytes()
        assert a.tobytes() == ctx.find_sites("NNNNn", host=True).tobytes()
        n, table = ctx.count_sites("NNNNn")
        assert n == len(want) and [int(x) for x in table.ravel()] == [sum(1 for w in want if (w[0], w[3]) == cs) for cs in ((0, "+"), (0, "-"), (1, "+"), (1, "-"))]
    finally:
        ctx.close()


def test_u_inside_the_longer_pam_only(C, monkeypatch):
    """PAMs of different lengths and a U of the reference that lies in the longer PAM's footprint but not in the shorter one's: the
    kernel, to which a U is an exception base, matches the shorter (auxiliary) PAM there; the answer is the longer, earlier one -- one
    record per position and strand, smallest pam_index -- in the listing and in the counts, on both strands and across a word boundary."""
    monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False)
    rng = random.Random(77)
    seq = [rng.choice("ACGT") for _ in range(4000)]
    plus, minus = [500, 64 * 20 - 22, 3000], [900, 64 * 30 - 3, 3400]
    for p in plus:                                   # protospacer, then AGGAGT read as nngrrt (and AGG as nrg): the T a U
        seq[p + 20:p + 26] = "AGGAGU"
    for p in minus:                                  # the reverse complement of <protospacer>AGGAGT is ACTCCT...: its first T (an r of nngrrt) a U
        seq[p:p + 6] = "ACUCCT"
    seq[2000:2006] = "AGGAUT"                        # a U that breaks nngrrt (r is A or G) and lies outside nrg: the auxiliary PAM's site stays
    seq = "".join(seq)
    want = R.brute_sites([seq], *R.PATTERNS["n20_nngrrt_nrg"])
    for p in plus:
        assert [w for w in want if w[1] == p and w[3] == "+"] == [(0, p, p + 20, "+", 0, 6, 20)]
    for p in minus:
        assert [w for w in want if w[1] == p + 6 and w[3] == "-"] == [(0, p + 6, p, "-", 0, 6, 20)]
    assert [w for w in want if w[1] == 1980 and w[3] == "+"] == [(0, 1980, 2000, "+", 1, 3, 20)]
    ctx = C.Context(0)
    try:
        ctx.set_reference(["u"], [seq.encode()])
        pat = _pattern(C, "n20_nngrrt_nrg")
        got = ctx.find_sites(pat)
        assert R.as_tuples(got) == want
        assert got.tobytes() == ctx.find_sites(pat, host=True).tobytes()
        n, table = ctx.count_sites(pat)
        assert n == len(want) and [int(x) for x in table[0]] == [sum(1 for w in want if w[3] == s) for s in "+-"]
        for a, b in ((480, 530), (890, 940), (64 * 20 - 22, 64 * 20 + 4), (64 * 20 - 22, 64 * 20 + 3)):     # the last: room for nrg only
            sub = R.brute_sites([seq], *R.PATTERNS["n20_nngrrt_nrg"], chrom=0, start=a, end=b)
            assert R.as_tuples(ctx.find_sites(pat, chrom=0, start=a, end=b)) == sub and ctx.count_sites(pat, chrom=0, start=a, end=b)[0] == len(sub)
    finally:
        ctx.close()


def test_regions(C, monkeypatch):
    ctx = _context(C, None, monkeypatch)
    try:
        names, seqs, _ = _genome(None)
        for name in ("n20_nrg", "tttv_n20", "n20_nngrrt_nrg"):
            proto, pams, five = R.PATTERNS[name]
            pat = _pattern(C, name)
            regions = [(0, 4097, 4127), (0, 4100, 4122),          # inside one 32-base word: room for a footprint, and just not
                       (0, 3999, 5417), (0, 8181, 8204), (0, 8182, 8204), (0, 8181, 8203),   # mid-word on both sides; a planted site, off by one
                       (0, 16000, 0), (1, 250, 0), (1, 0, 300), (2, 0, 0), (2, 1, 26), (3, 0, 12), (0, 777, 777)]
            for chrom, a, b in regions:
                want = R.brute_sites(seqs, proto, pams, five, chrom=chrom, start=a, end=b)
                got = ctx.find_sites(pat, chrom=names[chrom], start=a, end=b or None)
                assert R.as_tuples(got) == want, (name, chrom, a, b)
                n, table = ctx.count_sites(pat, chrom=chrom, start=a, end=b or None)
                assert n == len(want) and int(table.sum()) == n and int(table[chrom].sum()) == n
                assert (int(table[chrom, 0]), int(table[chrom, 1])) == (sum(1 for w in want if w[3] == "+"), sum(1 for w in want if w[3] == "-"))
            # every contig, each cut to the same bounds
            want = R.brute_sites(seqs, proto, pams, five, start=20, end=30000)
            assert R.as_tuples(ctx.find_sites(pat, start=20, end=30000)) == want
        assert len(R.brute_sites(seqs, *R.PATTERNS["fixed_nrg"], chrom=0, start=8181, end=8204)) == 1
    finally:
        ctx.close()


def test_absent_contig(C):
    ctx = C.Context(0)
    try:
        rng = random.Random(5)
        seq = "".join(rng.choice("ACGT") for _ in range(5000))
        ctx.set_reference(["here", "away", "there"], [seq.encode(), None, seq[::-1].encode()], lengths=[5000, 40000, 5000])
        want = R.brute_sites([seq, None, seq[::-1]], *R.PATTERNS["n20_nrg"], chrom=2)
        assert R.as_tuples(ctx.find_sites("NNNNNNNNNNNNNNNNNNNNnrg", chrom="there")) == want
        for chrom in ("away", None):
            with pytest.raises(C.CalitasError) as e:
                ctx.find_sites("NNNNNNNNNNNNNNNNNNNNnrg", chrom=chrom)
            assert e.value.code == C._lib.EINVAL
            with pytest.raises(C.CalitasError):
                ctx.count_sites("NNNNNNNNNNNNNNNNNNNNnrg", chrom=chrom)
    finally:
        ctx.close()


def _acgt_n_genome():
    """ACGT and N only, with non-overlapping copies of FIXED + a PAM of nrg on both strands."""
    rng = random.Random(31)
    seqs = []
    for n, at in ((30000, (0, 977, 1990, 2500, 9000, 16380, 20000, 29977)), (12000, (40, 5000, 8191, 11000))):
        s = ["ACGT"[rng.randrange(4)] for _ in range(n)]
        for i, p in enumerate(at):
            site = R.FIXED + ("AGG", "TGG", "CAG", "GGG")[i % 4]
            s[p:p + 23] = list(site if i % 3 else R.revcomp(site))
        s[12000:12000 + 300] = "N" * 300
        seqs.append("".join(s)[:n])
    return ["g1", "g2"], seqs


def test_against_the_search_engine(C, monkeypatch):
    """A fully specified guide + nrg: its sites are the rows of an exact search (-d 0 -p 0 -g 0 -O 100), which the oracle validates.
    And the guides find_guides cuts from an N20 + nrg listing hit their own site in an exact search."""
    monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    names, seqs = _acgt_n_genome()
    ctx = C.Context(0)
    try:
        ctx.set_reference(names, [s.encode() for s in seqs])
        G = C.Guide(R.FIXED + "nrg")
        sites = R.as_tuples(ctx.find_sites(G))
        assert sites == R.brute_sites(seqs, R.FIXED, ["nrg"], False) and len(sites) >= 12
        exact = C.make_params(max_guide_diffs=0, max_pam_mismatches=0, max_gaps_between_guide_and_pam=0, max_overlap=100)
        text, n = ctx.search_hits(G, "g", exact, "v", "t")
        rows = C.read_hits(text)
        # coordinate_start / coordinate_end are the protospacer's 0-based half-open offsets (GuideAlignment.guideStartOffset / guideEndOffset)
        from_rows = sorted((r["chromosome"], r["strand"], int(r["coordinate_start"]), int(r["coordinate_end"])) for r in rows)
        from_sites = sorted((names[c], s, p, p + L) for c, p, _, s, _, _, L in sites)
        print("rows", len(rows), "sites", len(sites))
        assert from_rows == from_sites
        listing = C.find_guides(ctx, "NNNNNNNNNNNNNNNNNNNNnrg")
        rng = random.Random(8)
        for r in rng.sample(listing, 5):
            table = ctx.search_counts(C.Guide(r.guide), exact)
            assert table[0 if r.strand == "+" else 1, 0, 0, 0] >= 1, r.row()
    finally:
        ctx.close()


def test_tools_end_to_end(C, tmp_path):
    names, seqs = _acgt_n_genome()
    s0 = seqs[0]
    seqs[0] = s0[:2600] + s0[2500:2523] + s0[2623:]                 # the site at 2500 once more at 2600: duplicated guide strings
    fa = write_fasta(str(tmp_path / "t.fa"), list(zip(names, seqs)))
    env = dict(os.environ, PYTHONPATH=ROOT)
    region = ["-r", fa, "-i", "NNNNNNNNNNNNNNNNNNNNnrg", "-c", "g1", "-s", "2450", "-e", "2700"]
    py, cc, cnt = str(tmp_path / "py.tsv"), str(tmp_path / "cc.tsv"), str(tmp_path / "counts.tsv")
    subprocess.run([sys.executable, "-m", "calitas_amd", "FindGuides", "-o", py] + region, check=True, env=env, cwd=ROOT, timeout=300)
    subprocess.run([os.path.join(ROOT, "calitas_amd", "calitas"), "FindGuides", "-o", cc] + region, check=True, timeout=300)
    a = open(py, "rb").read()
    assert a == open(cc, "rb").read() and a.count(b"\n") > 10
    subprocess.run([sys.executable, "-m", "calitas_amd", "FindGuides", "-o", cnt, "--counts", "-d", "2"] + region, check=True, env=env, cwd=ROOT,
                   timeout=300)
    plain = [ln.split("\t") for ln in a.decode().splitlines()]
    lines = [ln.split("\t") for ln in open(cnt).read().splitlines()]
    assert lines[0] == plain[0] + ["hits", "hits_mm0", "hits_mm1", "hits_mm2"]
    assert [f[:8] for f in lines[1:]] == plain[1:]
    by_guide = {}
    for f in lines[1:]:
        assert int(f[8]) == sum(int(x) for x in f[9:]) >= 1 and int(f[9]) >= 1          # every guide hits at least its own site exactly
        by_guide.setdefault(f[6], set()).add(tuple(f[8:]))
    assert all(len(v) == 1 for v in by_guide.values())                                   # the same string, the same numbers
    twice = R.FIXED + "nrg"
    assert sum(1 for f in lines[1:] if f[6] == twice) == 2 and int([f for f in lines[1:] if f[6] == twice][0][9]) >= 2
    ctx = C.Context(0)
    try:
        ctx.set_reference_fasta(fa)
        params = C.make_params(max_guide_diffs=2)
        for f in random.Random(2).sample(lines[1:], 3):
            assert int(f[8]) == int(ctx.search_counts(C.Guide(f[6]), params).sum())
    finally:
        ctx.close()


def test_site_listing_interleaved_with_key_calls(C):
    """The site listing and the key calls share one context's pattern block and device buffers: listings and counts, filtered and
    not, between count_copies, list_near and count_near, each held byte for byte against the same call on the host twin.  Two
    contigs of 20 kb (more than two segments of 8192 bases each), one U inside a site's footprint."""
    rng = random.Random(20261019)
    seqs = ["".join(rng.choice("ACGT") for _ in range(n)) for n in (20011, 19997)]
    seqs[0] = seqs[0][:5000] + "ACGUACGTAGG" + seqs[0][5011:]          # the '+' site at 5000 holds the U
    pattern = C.Guide("NNNNNNNNngg")
    keep = C.SiteFilter(gc_min=2, gc_max=6, avoid=("TTT",))
    model = C.ScoreModel.uniform(8, mismatch=39322)
    ctx = C.Context(0)
    try:
        ctx.set_reference(["chrA", "chrB"], [s.encode() for s in seqs])
        every = ctx.find_sites(pattern, host=True)
        kept = ctx.find_sites(pattern, host=True, filter=keep)
        at_u = every[(every["contig_index"] == 0) & (every["protospacer_start"] == 5000) & (every["strand"] == b"+")]
        assert len(at_u) == 1 and 0 < len(kept) < len(every)
        plus = every[every["strand"] == b"+"]
        keys = [seqs[s["contig_index"]][s["protospacer_start"]:s["protospacer_start"] + 8].replace("U", "T") for s in plus[::len(plus) // 38][:38]]
        keys += ["ACGTACGT", keys[0]]
        assert len(keys) == 40

        assert ctx.find_sites(pattern, filter=keep).tobytes() == kept.tobytes()
        assert ctx.count_copies(pattern, keys).tobytes() == ctx.count_copies(pattern, keys, host=True).tobytes()
        assert ctx.find_sites(pattern).tobytes() == every.tobytes()
        got, twin = ctx.list_near(pattern, keys, 1, model=model), ctx.list_near(pattern, keys, 1, model=model, host=True)
        assert got.near.tobytes() == twin.near.tobytes() and got.offsets.tobytes() == twin.offsets.tobytes() and got.hits.tobytes() == twin.hits.tobytes()
        assert len(got.hits) >= 40 and int(got.near[38].sum()) >= 1          # every key lists itself, the one at the U as well
        n, table = ctx.count_sites(pattern, filter=keep)
        want = np.zeros((2, 2), dtype=np.uint64)
        for s in kept:
            want[s["contig_index"], 1 if s["strand"] == b"-" else 0] += 1
        assert n == len(kept) and table.tobytes() == want.tobytes()
        assert ctx.find_sites(pattern, filter=keep).tobytes() == kept.tobytes()
        assert ctx.count_near(pattern, keys, 2).tobytes() == ctx.count_near(pattern, keys, 2, host=True).tobytes()
    finally:
        ctx.close()
