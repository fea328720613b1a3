"""GPU tests of the copies count (the copies kernel of sites.hip): device, host twin and the referee of copies_ref.py return the same
arrays on the planted genome and on the site tests' seam genomes at both lane chunks; the sweep over every protospacer and key
length; the table-size steps; hot counters (G x 40, K = 1 and 2); the keys 0 and all ones at K = 32; stale work buffers; and the
search engine as a second witness.  Contigs of <= 60 kb but for the 200-kb witness; a genome's brute force is computed once."""
import random

import numpy as np
import pytest

import copies_ref as X
import site_filter_ref as F
import sites_ref as R

pytestmark = pytest.mark.gpu

N20_NRG = "NNNNNNNNNNNNNNNNNNNNnrg"
# CALITAS_CHUNK -> the lane chunk it gives, as in test_gpu_sites.py: None: 64 (tiles of 16 kb: several per contig, a dead one among
# them), "512": one tile per contig
CHUNKS = {None: 64, "512": 512}


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


_cache = {}


def _genome(which):
    """(names, strings, {pattern: brute_sites listing}) of "planted" or of a lane chunk's seam genome; built once."""
    if which not in _cache:
        if which == "planted":
            names, seqs, expect = X.copies_genome()
            X.check_planted(seqs, expect)
        else:
            lane = CHUNKS[which]
            names, seqs = R.gpu_genome(1234 + lane, lane * 256, lane)
            assert all(len(s) <= 60000 for s in seqs)
        _cache[which] = (names, seqs, {})
    return _cache[which]


def _listing(which, name):
    names, seqs, done = _genome(which)
    if name not in done:
        done[name] = R.brute_sites(seqs, *X.PATTERNS[name])
    return done[name]


def _pattern(C, name):
    text, aux = X.pattern_string(name)
    return C.Guide(text, aux)


def _open(C, names, seqs, monkeypatch, chunk=None):
    if chunk is None:
        monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("CALITAS_CHUNK", chunk)
    ctx = C.Context(0)
    ctx.set_reference(names, [s.encode() for s in seqs])
    return ctx


@pytest.mark.parametrize("which", ["planted", None, "512"])
@pytest.mark.parametrize("name, K", X.CASES)
def test_device_equals_host_twin_equals_referee(C, which, name, K, monkeypatch):
    """The patterns and key lengths of the CPU test: all distinct keys (their sum is count_sites' total), keys that do not occur,
    duplicates, lower case, U for T; one contig alone and a region inside one."""
    # (512 also with five segments per workgroup, as a genome-sized call has several)
    if which == "512":
        monkeypatch.setenv("CALITAS_SITES_SEGS", "5")
    else:
        monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False)
    names, seqs, _ = _genome(which)
    ctx = _open(C, names, seqs, monkeypatch, None if which == "planted" else which)
    try:
        if which is None:
            assert ctx.tile_census()["dead"] >= 1                # chrB's N run covers a tile and its halos: the kernel skips it
        pat = _pattern(C, name)
        sites = _listing(which, name)
        counts, n_sites = X.copies(seqs, name, K, sites=sites)
        keys = sorted(counts)
        got = ctx.count_copies(pat, keys, key_length=K)
        print(which, name, K, "sites", n_sites, "distinct keys", len(keys), "largest count", max(counts.values()))
        assert got.tolist() == [counts[k] for k in keys]
        assert int(got.sum()) == n_sites == ctx.count_sites(pat)[0] > 0
        queries, want = X.queries_for(counts, K, seed=K * 100 + len(name))
        got = ctx.count_copies(pat, queries, key_length=K)
        assert got.tolist() == want
        assert got.tobytes() == ctx.count_copies(pat, queries, key_length=K, host=True).tobytes()
        # one contig alone (the referee's listing of it is the whole listing's records of that contig) ...
        for chrom in (0, 1):
            part, _ = X.copies(seqs, name, K, sites=[s for s in sites if s[0] == chrom])
            got = ctx.count_copies(pat, queries, key_length=K, chrom=chrom)
            assert got.tolist() == [part.get(q.upper().replace("U", "T"), 0) for q in queries], chrom
        # ... and a region inside one, across base 8192 (a segment edge of the kernel)
        part, _ = X.copies(seqs, name, K, chrom=0, start=8100, end=8300)
        got = ctx.count_copies(pat, queries, key_length=K, chrom=0, start=8100, end=8300)
        assert got.tolist() == [part.get(q.upper().replace("U", "T"), 0) for q in queries]
    finally:
        ctx.close()


def test_the_planted_cases(C, monkeypatch):
    """Each case by itself, the hot counter G x 40 and the keys 0 (A x 32) and all ones (T x 32) of the PAM-less K = 32 among them."""
    names, seqs, expect = X.copies_genome()
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        for case, name, K, key, n in expect:
            assert ctx.count_copies(_pattern(C, name), [key], key_length=K).tolist() == [n], (case, name, K, key)
        assert ("g_run", "n20_nrg", 20, "G" * 20, 36) in expect
        # A x 32 and T x 32 together, with and without other keys around them, in either order
        counts, n_sites = X.copies(seqs, "n32", 32)
        assert counts["A" * 32] == counts["T" * 32] == 18
        others = [k for k in sorted(counts) if k not in ("A" * 32, "T" * 32)][:40]
        for queries in (["T" * 32, "A" * 32], ["A" * 32], ["T" * 32], others + ["T" * 32] + others[:3] + ["A" * 32], others):
            assert ctx.count_copies("N" * 32, queries).tolist() == [counts[q] for q in queries]
        keys = sorted(counts)
        got = ctx.count_copies("N" * 32, keys)
        assert got.tolist() == [counts[k] for k in keys] and int(got.sum()) == n_sites
    finally:
        ctx.close()


def sweep_key_lengths(L):
    return sorted({K for K in (1, L // 2, L - 1, L) if K >= 1})


@pytest.mark.parametrize("L", F.SWEEP_LENGTHS)
def test_sweep_of_protospacer_and_key_lengths(C, L, monkeypatch):
    names, seqs = F.sweep_genome()
    sites = F.listing(L).sites
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        for K in sweep_key_lengths(L):
            counts = X.count_keys(sites, seqs, K, False)
            queries = sorted(counts) + X.absent_keys(counts, K, 10, seed=L * 40 + K)
            got = ctx.count_copies("N" * L, queries, key_length=K)
            assert got.tolist() == [counts.get(q, 0) for q in queries], (L, K)
            assert int(got.sum()) == len(sites)
    finally:
        ctx.close()


TABLE_STEPS = (0, 1, 2, 3, 4, 5, 1023, 1024, 1025, None)


def test_table_sizes_contended_counters_and_reused_buffers(C, monkeypatch):
    """One 60-kb random contig.  The table-size steps at K = 8 -- each call smaller or larger than the one before, the dense table of
    every distinct key first: the work buffers are reused, and stale table contents must not count.  K = 1 and K = 2: every site falls
    into 4 or 16 counters (the atomics under contention)."""
    names, seqs = X.random_contig()
    sites = R.brute_sites(seqs, *X.PATTERNS["n20_nrg"])
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        counts = X.count_keys(sites, seqs, 8, False)
        keys = sorted(counts)
        assert len(keys) > 4096
        for n in (None, 5, 1025, 0, 1024, 1, 1023, 2, 4, 3, None, 3):
            queries = keys[::max(1, len(keys) // 1100)][:n] if n is not None else keys
            if n == 3:
                queries = queries[::-1]
            got = ctx.count_copies(N20_NRG, queries, key_length=8)
            assert got.tolist() == [counts[k] for k in queries], n
            if n is None:
                assert int(got.sum()) == len(sites)
        assert set(TABLE_STEPS) == {None, 5, 1025, 0, 1024, 1, 1023, 2, 4, 3}
        # a key of the large call that the small call after it does not ask for: absent from the table, not stale in it
        absent = X.absent_keys(counts, 8, 5, seed=3)
        assert ctx.count_copies(N20_NRG, keys[:7] + absent, key_length=8).tolist() == [counts[k] for k in keys[:7]] + [0] * len(absent)
        for K in (1, 2):
            hot = X.count_keys(sites, seqs, K, False)
            queries = sorted(hot)
            assert len(queries) == 4 ** K
            got = ctx.count_copies(N20_NRG, queries, key_length=K)
            print("K", K, got.tolist())
            assert got.tolist() == [hot[q] for q in queries] and int(got.sum()) == len(sites)
            assert ctx.count_copies(N20_NRG, queries[1:2], key_length=K).tolist() == [hot[queries[1]]]
    finally:
        ctx.close()


def test_copies_equal_the_perfect_hits_of_a_search(C, monkeypatch):
    """A 200-kb random ACGT contig with FIXED + TGG, the reverse complement of FIXED + AGG and FIXED + CGG planted more than 10 kb apart,
    and FIXED + TTT once: three copies, which is what a zero-difference search of FIXED + nrg finds as perfect hits."""
    rng = random.Random(5)
    seq = list(R._rand(rng, 200000))
    R._put(seq, 20000, R.FIXED + "TGG")
    R._put(seq, 90011, R.revcomp(R.FIXED + "AGG"))
    R._put(seq, 170005, R.FIXED + "CGG")
    R._put(seq, 130000, R.FIXED + "TTT")
    ctx = _open(C, ["chrW"], ["".join(seq)], monkeypatch)
    try:
        got = ctx.count_copies(N20_NRG, [R.FIXED])
        assert got.tolist() == [3]
        assert ctx.count_copies(N20_NRG, [R.FIXED], host=True).tolist() == [3]
        params = C.make_params(max_guide_diffs=0, max_pam_mismatches=0, max_gaps_between_guide_and_pam=0)
        scores = ctx.search_scores(C.Guide(R.FIXED + "nrg"), params, C.ScoreModel.uniform(20))
        assert scores.perfect == 3
    finally:
        ctx.close()
