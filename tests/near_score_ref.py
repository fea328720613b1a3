"""The referee of the scored near-copies tests (test_near_score_host.py, test_gpu_near_score.py): Python on strings that shares no code
with the library.  The sites are sites_ref.brute_sites', their keys copies_ref.key_of's strings, the distance a count of differing
letters (near_ref.distance), and the score of a (query, key) pair the contract's loop written out on the two strings' letters:
s = 2^32, and for every differing position in ASCENDING guide position s = (s * mismatch[i][query letter][key letter]) >> 16.
scored() gives per query its row of counts, the sum and the maximum of the scores of the sites at d = 1 .. M.

Three models per protospacer length: `distinct` (every factor another odd value in (2^15, 2^16), so a wrong position or a swapped
letter pair gives another integer -- check_order() asserts that on the planted pairs at d = 3, and why the ORDER of at most three
factors cannot show in any integer), `zeros` (distinct with one factor at position 0, one that a pair of the test reads, set to 0)
and `uniform` (every factor 1.0)."""
import random

import numpy as np

import copies_ref as X
import near_ref as N
import sites_ref as R

IDX = {"A": 0, "C": 1, "G": 2, "T": 3}
ONE = 1 << 32


def pair_score(query, key, mismatch, descending=False):
    """The score of one pair, None at distance 0.  mismatch: [L][5][5] of Python ints.  descending: the factors in the WRONG order."""
    q = N.canon(query)
    assert len(q) == len(key) == len(mismatch)
    at = [i for i in range(len(q)) if q[i] != key[i]]
    if not at:
        return None
    s = ONE
    for i in (reversed(at) if descending else at):
        s = (s * mismatch[i][IDX[q[i]]][IDX[key[i]]]) >> 16
    return s


def scored(key_counts, queries, M, mismatch):
    """{canonical query: (row of M + 1 counts, sum, maximum, pairs scored 0)} from {key: sites that carry it}."""
    keys = sorted(key_counts)
    out = {}
    L = len(mismatch)
    letters = np.frombuffer("".join(keys).encode(), dtype=np.uint8).reshape(len(keys), L) if keys else np.zeros((0, L), dtype=np.uint8)
    for q in queries:
        q = N.canon(q)
        if q in out:
            continue
        assert len(q) == L
        d = (letters != np.frombuffer(q.encode(), dtype=np.uint8)).sum(axis=1)
        row, total, top, zeros = [0] * (M + 1), 0, 0, 0
        for k in np.nonzero(d <= M)[0]:
            key = keys[int(k)]
            n = key_counts[key]
            dist = N.distance(q, key)
            assert dist == int(d[k])
            row[dist] += n
            if dist:
                s = pair_score(q, key, mismatch)
                total += n * s
                top = max(top, s)
                zeros += n * (s == 0)
        out[q] = (row, total, top, zeros)
    return out


def table_for(key_counts, queries, M, mismatch):
    """(near rows, sums, maxima, pairs scored 0) in the queries' order: what a call returns."""
    t = scored(key_counts, queries, M, mismatch)
    got = [t[N.canon(q)] for q in queries]
    return [g[0] for g in got], [g[1] for g in got], [g[2] for g in got], sum(g[3] for g in got)


def merged(parts):
    """Tables of disjoint contig sets as one: counts and sums add, the maxima take the maximum."""
    rows = [[sum(c) for c in zip(*r)] for r in zip(*[p[0] for p in parts])]
    return rows, [sum(s) for s in zip(*[p[1] for p in parts])], [max(m) for m in zip(*[p[2] for p in parts])]


def distinct_mismatch(L, seed=16):
    """[L][5][5]: every entry another odd value in (2^15, 2^16)."""
    rng = random.Random(seed * 1000 + L)
    values = rng.sample(range((1 << 15) + 1, 1 << 16, 2), L * 25)
    assert len(set(values)) == L * 25 and all(v & 1 and (1 << 15) < v < (1 << 16) for v in values)
    return [[[values[(i * 5 + g) * 5 + t] for t in range(5)] for g in range(5)] for i in range(L)]


def zeros_mismatch(L, query_letter, key_letter, seed=16):
    """distinct with the factor of (position 0, query letter, key letter) set to 0."""
    m = distinct_mismatch(L, seed)
    m[0][IDX[query_letter]][IDX[key_letter]] = 0
    return m


def model_of(C, mismatch):
    return C.ScoreModel(len(mismatch), np.array(mismatch, dtype=np.uint32))


def planted():
    """near_ref's planted genome with its cases checked: (names, strings, expect)."""
    names, seqs, expect = N.near_genome()
    N.check_planted(seqs, expect)
    return names, seqs, expect


def planted_queries(expect, name, key_counts, L, seed):
    """The planted queries of a pattern -- at a shorter K the whole keys that carry them -- and near_ref's mix around them (keys,
    variants, absent keys, duplicates, case, U)."""
    own = set()
    for _, n, K, _, q, _ in expect:
        if n == name:
            own |= {q} if K == L else {k for k in key_counts if k.startswith(q) or k.endswith(q)}
    return sorted(own) + N.queries_for(key_counts, L, seed=seed, cap=60)


def zero_pair(key_counts, queries):
    """The (query letter, key letter) at position 0 of the first pair within 3 substitutions that differs there: the factor the
    `zeros` model sets to 0, so that it is read."""
    for q in sorted({N.canon(q) for q in queries}):
        for k in sorted(key_counts):
            if q[0] != k[0] and N.distance(q, k) <= 3:
                return q[0], k[0]
    raise AssertionError("no pair differs at position 0")


def check_order(key_counts, expect, mismatch):
    """What the `distinct` model can and cannot tell apart on the planted pairs at d = 3 (near_ref's `layouts` of x3).
    It CANNOT tell the order of the factors: from s = 2^32 the first step gives 2^16 a and the second a b, both exact (a b < 2^32),
    so three factors are floor(a b c / 2^16) in any order -- within M <= 3 the contract's order is not observable, and no model makes
    a pair that shows it.  That is asserted here, so that nobody looks for such a pair again.  It CAN tell a transposed letter pair
    (mismatch[i][key letter][query letter]) and a position off by one, each on every planted pair."""
    x3 = next(q for case, name, K, M, q, _ in expect if case == "pieces" and M == 3)
    at3 = [k for k in key_counts if N.distance(k, x3) == 3]
    assert len(at3) >= 4
    L = len(x3)
    for k in at3:
        s = pair_score(x3, k, mismatch)
        assert s == pair_score(x3, k, mismatch, descending=True)
        a, b, c = [mismatch[i][IDX[x3[i]]][IDX[k[i]]] for i in range(L) if x3[i] != k[i]]
        assert s == (a * b * c) >> 16
        assert s != pair_score(k, x3, mismatch)                                             # the letters the other way round
        assert s != pair_score(x3, k, mismatch[1:] + mismatch[:1])                          # the table one position off
    return x3, at3


def check_against_score_of_row(C, pairs, mismatch):
    """pair_score against aligner.score_of_row on a hand-built ungapped row of each pair."""
    model = model_of(C, mismatch)
    for q, key in pairs:
        q = N.canon(q)
        row = {"padded_guide": q, "padded_alignment": "".join("|" if a == b else "." for a, b in zip(q, key)), "padded_target": key,
               "guide_gaps": "0", "pam_mm": "0", "total_mm_plus_gaps": str(N.distance(q, key))}
        assert C.score_of_row(row, model) == pair_score(q, key, mismatch) == C.near_score(q, key, model), (q, key)


def search_genome(seed):
    """(names, strings, guide): a contig of a few kb of random flanks with one 20-mer next to TGG and planted copies with one and two
    substitutions, more than 100 bases apart, on both strands."""
    rng = random.Random(seed)
    guide = X._distinct(rng, 1, need="ACGT")[0]
    units = [(guide, False), (N.swap(guide, 3), False), (N.swap(guide, 17), True), (N.swap(guide, 0, 11), False), (N.swap(guide, 6, 19), True),
             (N.swap(guide, 9), True), (N.swap(guide, 2, 14), False)]
    parts = []
    for x, minus in units:
        parts.append(R._rand(rng, 300))
        parts.append(R.revcomp(x + "TGG") if minus else x + "TGG")
    parts.append(R._rand(rng, 300))
    return ["chrS"], ["".join(parts)], guide


def hold(C, ctx, pattern, queries, M, mismatch, key_counts, paths, **region):
    """One call on every path of `paths` (host=True: the host twin, False: the device) against the referee's table of `key_counts`,
    and the paths against each other byte for byte.  Returns (the last path's NearScores, the pairs the referee scored 0)."""
    rows, sums, tops, zeros = table_for(key_counts, queries, M, mismatch)
    model = model_of(C, mismatch)
    first = got = None
    for host in paths:
        got = ctx.score_near(pattern, queries, M, model, host=host, **region)
        assert got.near.dtype == got.sum_q32.dtype == got.max_q32.dtype == np.uint64
        assert got.near.shape == (len(queries), M + 1) and got.sum_q32.shape == got.max_q32.shape == (len(queries),)
        assert got.near.tolist() == rows, (host, M, region)
        assert got.sum_q32.tolist() == sums, (host, M, region)
        assert got.max_q32.tolist() == tops, (host, M, region)
        if first is None:
            first = got
        assert (got.near.tobytes(), got.sum_q32.tobytes(), got.max_q32.tobytes()) == (first.near.tobytes(), first.sum_q32.tobytes(), first.max_q32.tobytes())
    return got, zeros


# (pattern of copies_ref.PATTERNS, L) of the planted genome's runs
PLANTED = [("n20_nrg", 20), ("tttv_n20", 20), ("n32", 32)]
RUNS32 = ["A" * 32, "T" * 32, "C" + "A" * 31, "T" * 31 + "C"]


def hold_planted(C, ctx, name, L, M, kind, paths, seqs, expect, sites=None):
    """The planted genome under the `distinct` or the `zeros` model of a pattern."""
    counts, _ = X.copies(seqs, name, L, sites=sites)
    queries = RUNS32 if name == "n32" else planted_queries(expect, name, counts, L, seed=L + len(name))
    mismatch = distinct_mismatch(L) if kind == "distinct" else zeros_mismatch(L, *zero_pair(counts, queries))
    text, aux = X.pattern_string(name)
    got, zeros = hold(C, ctx, C.Guide(text, aux), queries, M, mismatch, counts, paths)
    if kind == "zeros" and M == 3:
        assert zeros > 0                                    # a pair that is counted, adds nothing and leaves the maximum
    if name == "n20_nrg" and kind == "distinct":
        x3, at3 = check_order(counts, expect, mismatch)
        check_against_score_of_row(C, [(x3, k) for k in at3], mismatch)
        if M == 3:
            i = queries.index(x3)
            assert int(got.near[i, 3]) == len(at3) == 4 and int(got.max_q32[i]) >= max(pair_score(x3, k, mismatch) for k in at3)
    return got


def hold_seams(C, ctx, name, seqs, sites, paths):
    """A seam genome: the table against the referee and against count_near byte for byte, per-contig results merging to the whole, a
    region across base 8192."""
    L = len(X.PATTERNS[name][0])
    text, aux = X.pattern_string(name)
    pat = C.Guide(text, aux)
    counts, _ = X.copies(seqs, name, L, sites=sites)
    queries = N.queries_for(counts, L, seed=L * 100 + len(name), cap=80)
    mismatch = distinct_mismatch(L)
    model = model_of(C, mismatch)
    for M in (1, 3):
        whole, _ = hold(C, ctx, pat, queries, M, mismatch, counts, paths)
        for host in paths:
            assert whole.near.tobytes() == ctx.count_near(pat, queries, M, host=host).tobytes()
        parts = [ctx.score_near(pat, queries, M, model, chrom=i, host=paths[-1]) for i in range(len(seqs))]
        want = [table_for(X.copies(seqs, name, L, sites=[s for s in sites if s[0] == i])[0], queries, M, mismatch) for i in range(len(seqs))]
        for i, part in enumerate(parts):
            assert (part.near.tolist(), part.sum_q32.tolist(), part.max_q32.tolist()) == want[i][:3], (M, i)
        assert parts[0].merge(*parts[1:]) == whole and sum(parts[1:], parts[0]) == whole
        assert (whole.near.tolist(), whole.sum_q32.tolist(), whole.max_q32.tolist()) == merged([w[:3] for w in want])
        hold(C, ctx, pat, queries, M, mismatch, X.copies(seqs, name, L, chrom=0, start=8100, end=8300)[0], paths, chrom=0, start=8100, end=8300)
    return whole


def sweep_ms(L):
    return [M for M in (0, 1, 3) if L >= M + 1]


def hold_sweep(C, ctx, L, seqs, sites, paths):
    counts = X.count_keys(sites, seqs, L, False)
    queries = N.queries_for(counts, L, seed=L * 40, cap=40, n_absent=5)
    for M in sweep_ms(L):
        hold(C, ctx, "N" * L, queries, M, distinct_mismatch(L), counts, paths)


def hold_uniform(C, ctx, paths):
    """All 4^4 keys at L = 4, M = 3 under the uniform model: every site adds to all 256 queries -- a few hot counters -- and the sum
    is the count of scored sites times 2^32."""
    queries = ["".join("ACGT"[(i >> (2 * j)) & 3] for j in range(4)) for i in range(256)]
    first = None
    for host in paths:
        got = ctx.score_near("NNNNngg", queries, 3, C.ScoreModel.uniform(4), host=host)
        assert got.sum_q32.tolist() == [int(x) << 32 for x in got.near[:, 1:].sum(axis=1)]
        assert set(got.max_q32.tolist()) <= {0, ONE} and got.max_q32.tolist() == [ONE if x else 0 for x in got.near[:, 1:].sum(axis=1)]
        assert got.near.tobytes() == ctx.count_near("NNNNngg", queries, 3, host=host).tobytes()
        n_sites = int(got.near[:, 0].sum())                 # (every site's key is one of the queries)
        assert n_sites > 5000 and got.near.sum(axis=0).tolist() == [n_sites * f for f in (1, 12, 54, 108)]
        assert np.allclose(got.specificity, 1.0 / (1.0 + got.near[:, 1:].sum(axis=1).astype(np.float64)))
        first = first or got
        assert got == first
    return first


def hold_reused(C, ctx, seqs, host):
    """score_near, count_near and count_copies interleaved on one context (of `seqs`), the large call first, with M changing: the
    counters are shared and their rows change length, nothing stale may count."""
    sites = R.brute_sites(seqs, "N" * 8, ["ngg"], False)
    counts = X.count_keys(sites, seqs, 8, False)
    keys = sorted(counts)
    assert len(keys) > 1100
    pat, mismatch = "NNNNNNNNngg", distinct_mismatch(8)
    model = model_of(C, mismatch)
    for n, M, what in ((None, 1, "score"), (3, 3, "near"), (9, 0, "copies"), (7, 0, "score"), (1025, 2, "score"), (2, 1, "near"), (600, 3, "score"),
                       (5, 2, "copies"), (1, 3, "score"), (40, 2, "near")):
        queries = keys if n is None else keys[::max(1, len(keys) // 1100)][:n]
        if what == "score":
            rows, sums, tops, _ = table_for(counts, queries, M, mismatch)
            got = ctx.score_near(pat, queries, M, model, host=host)
            assert (got.near.tolist(), got.sum_q32.tolist(), got.max_q32.tolist()) == (rows, sums, tops), (n, M)
            assert n is not None or (int(got.near[:, 0].sum()) == len(sites) and int(got.sum_q32.sum()) > 0)
        elif what == "near":
            assert ctx.count_near(pat, queries, M, host=host).tolist() == N.rows_for(counts, queries, M), (n, M)
        else:
            assert ctx.count_copies(pat, queries, host=host).tolist() == [counts[k] for k in queries], n


def hold_errors(C, ctx, host):
    """The errors in their order: what count_near refuses first, then the model's."""
    EINVAL = C._lib.EINVAL
    pat, q20, model = "N" * 20 + "nrg", ["ACGT" * 5], C.ScoreModel.uniform(20)
    bad_model = C.ScoreModel.uniform(19)
    over = C.ScoreModel.uniform(20)
    over.mismatch[7, 2, 1] = 65537

    def refused(word, *args, **kw):
        with pytest_raises(C) as e:
            ctx.score_near(*args, host=host, **kw)
        assert e.value.code == EINVAL and word in str(e.value), (word, str(e.value))

    for M in (-1, 4):
        refused("max_mismatches", pat, q20, M, bad_model)               # before the region, the queries and the model
        refused("max_mismatches", pat, ["ACGTN" * 4], M, None, chrom=0, start=50, end=20)
    refused("region", pat, ["ACGTN" * 4], 1, bad_model, chrom=0, start=50, end=20)     # the region before the queries and the model
    refused("queries[1]", pat, ["ACGT" * 5, "ACGTN" * 4], 2, bad_model)
    refused("max_mismatches + 1", "NNNngg", ["ACG"], 3, C.ScoreModel.uniform(2))    # the key is the protospacer: 3 bases, M + 1 = 4
    refused("no mismatch table", pat, q20, 1, None)
    refused("19 bases", pat, q20, 1, bad_model)
    refused("above 65536", pat, q20, 1, over)
    ok = C.ScoreModel.uniform(20, gap=1 << 20, pam_mismatch=1 << 20)     # gap and pam_mismatch are not used, so not looked at
    assert ctx.score_near(pat, q20, 1, ok, host=host).near.shape == (1, 2)
    with pytest_raises(C, ValueError):
        ctx.score_near(pat, ["ACGT"], 1, model, host=host)              # not the protospacer's length
    none = ctx.score_near(pat, [], 2, model, host=host)                 # no query is legal; the model is still checked
    assert none.near.shape == (0, 3) and none.sum_q32.shape == none.max_q32.shape == none.specificity.shape == (0,)
    refused("19 bases", pat, [], 2, bad_model)


class pytest_raises:
    """pytest.raises for CalitasError (or another type), without importing pytest into the referee."""

    def __init__(self, C, kind=None):
        self.kind, self.value = kind or C.CalitasError, None

    def __enter__(self):
        return self

    def __exit__(self, typ, value, tb):
        assert typ is not None and issubclass(typ, self.kind), "nothing was raised" if typ is None else repr(value)
        self.value = value
        return True


def hold_search_rows(C, names, seqs, guide, got, mismatch):
    """The CPU half of the agreement with the search: the reference's rows of the search with d = 2, p = 0, g = 0 are all ungapped with a
    clean PAM and as many as the guide's near row holds -- the condition under which search and near call answer one question -- and
    scores_of_rows on them gives the near call's numbers.  Returns the Scores of the rows."""
    import oracle_lib
    _, rows, _ = oracle_lib.search_memory(names, [s.encode() for s in seqs], guide + "ngg", d=2, p=0, g=0)
    assert rows and all(int(r["guide_gaps"]) == 0 and int(r["pam_mm"]) == 0 for r in rows)
    assert len(rows) == int(got.near[0].sum()) and got.near[0].tolist() == [1, 3, 3]
    want = C.scores_of_rows(rows, model_of(C, mismatch))
    assert (want.perfect, want.sum_q32, want.max_q32) == (int(got.near[0, 0]), int(got.sum_q32[0]), int(got.max_q32[0]))
    assert want.sum_q32 > want.max_q32 > 0
    return want
