"""GPU tests of the near-copies count (the near kernel of sites.hip): device, host twin and the referee of near_ref.py return the same
tables on the planted genome and on the site tests' seam genomes at both lane chunks; the planted cases one by one; the sweep over
every protospacer length; the closed form over all keys (contended counters); a large call followed by a small one with another M
(reused work buffers); column 0 against the device's copies count.  Contigs of <= 60 kb; a genome's brute force is computed once."""
import numpy as np
import pytest

import copies_ref as X
import near_ref as N
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
            names, seqs, expect = N.near_genome()
            N.check_planted(seqs, expect)
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
@pytest.mark.parametrize("name, K", N.CASES)
def test_device_equals_host_twin_equals_referee(C, which, name, K, monkeypatch):
    """The patterns and key lengths of the CPU test at every M the key allows: distinct site keys, their one- and two-substitution
    variants, keys that do not occur, duplicates, lower case, U for T; one contig alone and a region inside one."""
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
        queries = N.queries_for(counts, K, seed=K * 100 + len(name))
        whole = N.rows_for(counts, queries, N.MAX_M)             # (the row of a smaller M is this one's head)
        parts = [N.rows_for(X.copies(seqs, name, K, sites=[s for s in sites if s[0] == chrom])[0], queries, N.MAX_M) for chrom in (0, 1)]
        region = N.rows_for(X.copies(seqs, name, K, chrom=0, start=8100, end=8300)[0], queries, N.MAX_M)
        copies = ctx.count_copies(pat, queries, key_length=K)
        print(which, name, K, "sites", n_sites, "distinct keys", len(counts), "queries", len(queries), "column sums", np.array(whole).sum(axis=0).tolist())
        for M in range(4):
            if not N.legal(K, M):
                continue
            got = ctx.count_near(pat, queries, M, key_length=K)
            assert got.shape == (len(queries), M + 1) and got.tolist() == [r[:M + 1] for r in whole], M
            assert got.tobytes() == ctx.count_near(pat, queries, M, key_length=K, host=True).tobytes()
            assert got[:, 0].tobytes() == copies.tobytes()
            # one contig alone (the referee's listing of it is the whole listing's records of that contig) ...
            for chrom in (0, 1):
                got = ctx.count_near(pat, queries, M, key_length=K, chrom=chrom)
                assert got.tolist() == [r[:M + 1] for r in parts[chrom]], (M, chrom)
            # ... and a region inside one, across base 8192 (a segment edge of the kernel)
            got = ctx.count_near(pat, queries, M, key_length=K, chrom=0, start=8100, end=8300)
            assert got.tolist() == [r[:M + 1] for r in region], M
    finally:
        ctx.close()


def test_the_planted_cases(C, monkeypatch):
    """Each case by itself, then all of a pattern's queries together: a query alone in its buckets and among others."""
    names, seqs, expect = N.near_genome()
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        for case, name, K, M, query, row in expect:
            got = ctx.count_near(_pattern(C, name), [query], M, key_length=K)
            assert got.dtype == np.uint64 and got.tolist() == [row], (case, name, K, M, query)
        for M in (1, 2, 3):
            some = [(q, row) for _, name, K, m, q, row in expect if (name, K, m) == ("n20_nrg", 20, M)]
            assert len(some) >= 5
            assert ctx.count_near(N20_NRG, [q for q, _ in some], M).tolist() == [row for _, row in some]
        # A x 32 and T x 32 (keys 0 and all ones) together, in either order, with their neighbours
        runs = ["A" * 32, "T" * 32, "C" + "A" * 31, "T" * 31 + "C"]
        counts, _ = X.copies(seqs, "n32", 32)
        for queries in (runs, runs[::-1], runs[:1], runs[1:2]):
            assert ctx.count_near("N" * 32, queries, 3).tolist() == N.rows_for(counts, queries, 3)
        assert N.rows_for(counts, runs[:2], 3) == [[18, 4, 4, 4], [18, 4, 4, 4]]
    finally:
        ctx.close()


def sweep_cases(L):
    """(K, M) of a protospacer length: K of M + 1, L / 2 and L, M of 0, 1 and 3, where the key is long enough."""
    return sorted({(K, M) for M in (0, 1, 3) for K in (M + 1, L // 2, L) if M + 1 <= K <= L})


@pytest.mark.parametrize("L", F.SWEEP_LENGTHS)
def test_sweep_of_protospacer_and_key_lengths(C, L, monkeypatch):
    names, seqs = F.sweep_genome()
    sites = F.listing(L).sites
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        for K, M in sweep_cases(L):
            counts = X.count_keys(sites, seqs, K, False)
            queries = N.queries_for(counts, K, seed=L * 40 + K, cap=40, n_absent=5)
            got = ctx.count_near("N" * L, queries, M, key_length=K)
            assert got.tolist() == N.rows_for(counts, queries, M), (L, K, M)
    finally:
        ctx.close()


# per site, the keys of K letters at distance d: C(K, d) 3^d
CLOSED = {(4, 3): (1, 12, 54, 108), (3, 2): (1, 9, 27)}


def _random_contig():
    """(names, strings, brute_sites listing of N20 + nrg) of copies_ref.random_contig(), made once."""
    if "random" not in _cache:
        names, seqs = X.random_contig()
        _cache["random"] = (names, seqs, R.brute_sites(seqs, *X.PATTERNS["n20_nrg"]))
    return _cache["random"]


def test_closed_form_and_contended_counters(C, monkeypatch):
    """One 60-kb random contig.  All 4^K keys as queries: a site is at distance d of C(K, d) 3^d of them, so the column sums are n_sites
    times that, and every site adds to 175 (K = 4, M = 3) or 37 (K = 3, M = 2) of a few hundred counters."""
    names, seqs, sites = _random_contig()
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        for (K, M), factors in sorted(CLOSED.items()):
            queries = ["".join("ACGT"[(i >> (2 * j)) & 3] for j in range(K)) for i in range(4 ** K)]
            got = ctx.count_near(N20_NRG, queries, M, key_length=K)
            print("K", K, "M", M, got.sum(axis=0).tolist())
            assert got.sum(axis=0).tolist() == [len(sites) * f for f in factors]
            assert got.tolist() == N.rows_for(X.count_keys(sites, seqs, K, False), queries, M)
    finally:
        ctx.close()


def test_reused_work_buffers(C, monkeypatch):
    """Calls of different size and M one after the other on one context, the large one first: tables and counters are reused, and
    nothing stale may count."""
    names, seqs, sites = _random_contig()
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        counts = X.count_keys(sites, seqs, 8, False)
        keys = sorted(counts)
        assert len(keys) > 4096
        absent = X.absent_keys(counts, 8, 5, seed=3)
        # (every distinct key, M = 1) then (3 keys, M = 3), (7 keys and absent ones, M = 0), (1025 keys, M = 2), (2 keys, M = 1), ..
        for n, M in ((None, 1), (3, 3), (7, 0), (1025, 2), (2, 1), (600, 3), (1, 2)):
            queries = (keys if n is None else keys[::max(1, len(keys) // 1100)][:n]) + (absent if n == 7 else [])
            got = ctx.count_near(N20_NRG, queries, M, key_length=8)
            want = N.rows_for(counts, queries, M)
            assert got.tolist() == want, (n, M)
            if n is None:
                assert int(got[:, 0].sum()) == len(sites)
                assert got.sum(axis=0).tolist() == np.array(want).sum(axis=0).tolist()
        # the same context's copies count in between and after: the two share the counters
        assert ctx.count_copies(N20_NRG, keys[:9], key_length=8).tolist() == [counts[k] for k in keys[:9]]
        assert ctx.count_near(N20_NRG, keys[:9], 1, key_length=8)[:, 0].tolist() == [counts[k] for k in keys[:9]]
    finally:
        ctx.close()


def test_column_zero_is_the_device_copies_count(C, monkeypatch):
    names, seqs = R.gpu_genome(1234 + 64, 64 * 256, 64)
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        for name, K in (("n20_nrg", 20), ("n20_nrg", 12), ("tttv_n20", 12), ("n21", 10)):
            pat = _pattern(C, name)
            rows = ctx.find_sites(pat, chrom=0, start=4000, end=9000)
            assert len(rows) > 100
            five = X.PATTERNS[name][2] and bool(X.PATTERNS[name][1])
            keys = [X.key_of(s, seqs, K, five) for s in R.as_tuples(rows)]
            copies = ctx.count_copies(pat, keys, key_length=K)
            assert int(copies.min()) >= 1
            for M in (0, 1, 2, 3):
                got = ctx.count_near(pat, keys, M, key_length=K)
                assert got[:, 0].tobytes() == copies.tobytes(), (name, K, M)
                if M:
                    assert got[:, :M].tobytes() == ctx.count_near(pat, keys, M - 1, key_length=K).tobytes()
    finally:
        ctx.close()
