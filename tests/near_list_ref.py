"""The referee of the near-copies listing tests (test_near_list_host.py, test_gpu_near_list.py): Python on strings that shares no code
with the library.  The sites are sites_ref.brute_sites', a site's letters copies_ref.key_of's string, and a query is held against every
site letter by letter: the positions that differ give the record's diff_mask and mismatches, the site's letters its two planes, and
near_score_ref.pair_score the score.  expected() gives per query its row of counts and its stretch -- ordered by contig, protospacer
start, '+' before '-', and empty where the row sums to more than the limit -- and answer() the block a call must return, byte for
byte.  No planes, no buckets."""
import random

import numpy as np

import copies_ref as X
import near_ref as N
import near_score_ref as S
import sites_ref as R

ONE = 1 << 32
LIST_MAX = 4096
IDX = {"A": 0, "C": 1, "G": 2, "T": 3}
# calitas_near_hit_t, written down a second time
DTYPE = np.dtype([("score_q32", "<u8"), ("contig_index", "<i4"), ("protospacer_start", "<i4"), ("target_lo", "<u4"), ("target_hi", "<u4"),
                  ("diff_mask", "<u4"), ("strand", "S1"), ("pam_index", "i1"), ("mismatches", "u1"), ("reserved", "u1")])
assert DTYPE.itemsize == 32
# (pattern of copies_ref.PATTERNS, L) of the planted genome's runs
PLANTED = [("n20_nrg", 20), ("n20_nngrrt_nrg", 20), ("tttv_n20", 20), ("n32", 32)]


def table_of(sites, seqs):
    """[(contig, protospacer start, strand, pam_index, the protospacer as the guide reads it)] of brute_sites' tuples, in their order."""
    return [(s[0], s[1], s[3], s[4], X.key_of(s, seqs, s[6], False)) for s in sites]


def record(query, site, mismatch):
    """One (site, query) pair as a record's fields, letter by letter."""
    c, p, strand, k, key = site
    at = [i for i in range(len(query)) if query[i] != key[i]]
    score = S.pair_score(query, key, mismatch) if mismatch is not None and at else ONE
    lo = sum((IDX[ch] & 1) << i for i, ch in enumerate(key))
    hi = sum((IDX[ch] >> 1) << i for i, ch in enumerate(key))
    return (score, c, p, lo, hi, sum(1 << i for i in at), strand.encode(), k, len(at), 0)


def expected(table, queries, M, mismatch, limit):
    """{canonical query: (row of M + 1 counts, [records in order], or [] over the limit)}."""
    L = len(queries[0]) if queries else 0
    letters = np.frombuffer("".join(t[4] for t in table).encode(), dtype=np.uint8).reshape(len(table), L) if table else np.zeros((0, L), dtype=np.uint8)
    out = {}
    for q in queries:
        q = N.canon(q)
        if q in out:
            continue
        d = (letters != np.frombuffer(q.encode(), dtype=np.uint8)).sum(axis=1)
        close = [int(i) for i in np.nonzero(d <= M)[0]]
        row = [0] * (M + 1)
        for i in close:
            assert N.distance(q, table[i][4]) == int(d[i])
            row[int(d[i])] += 1
        recs = []
        if sum(row) <= limit:
            recs = [record(q, table[i], mismatch) for i in close]
            recs.sort(key=lambda r: (r[1], r[2], r[6] != b"+"))
            assert len({(r[1], r[2], r[6]) for r in recs}) == len(recs)          # the order is total
        out[q] = (row, recs)
    return out


def answer(table, queries, M, mismatch, limit):
    """(near rows, offsets, the records' bytes, the records) in the queries' order: what a call returns."""
    exp = expected(table, queries, M, mismatch, limit)
    rows, offsets, recs = [], [0], []
    for q in queries:
        row, mine = exp[N.canon(q)]
        rows.append(row)
        recs += mine
        offsets.append(len(recs))
    return rows, offsets, np.array(recs, dtype=DTYPE).tobytes(), recs


def letters_of(hit, L):
    lo, hi = int(hit["target_lo"]), int(hit["target_hi"])
    return "".join("ACGT"[((lo >> i) & 1) | (((hi >> i) & 1) << 1)] for i in range(L))


def check_invariants(C, ctx, pattern, queries, M, mismatch, got, table, host, region):
    """What holds for every result, asserted on the result itself."""
    L = len(queries[0]) if queries else 0
    assert got.offsets.dtype == np.uint64 and got.offsets.shape == (len(queries) + 1,) and int(got.offsets[0]) == 0
    assert all(int(a) <= int(b) for a, b in zip(got.offsets, got.offsets[1:])) and int(got.offsets[-1]) == len(got.hits)
    assert got.hits.dtype == DTYPE == np.dtype(C.aligner.NEAR_HIT_DTYPE) and not got.hits["reserved"].any()
    scores = ctx.score_near(pattern, queries, M, S.model_of(C, mismatch), host=host, **region) if mismatch is not None and queries else None
    found = ctx.find_sites(pattern, region.get("chrom"), region.get("start", 0), region.get("end"), host=host)
    key_at = {(t[0], t[1], t[2]): t[4] for t in table}
    assert len(found) == len(table)
    own_of = {}
    for s in found:
        place = (int(s["contig_index"]), int(s["protospacer_start"]), s["strand"])
        own_of.setdefault(key_at[(place[0], place[1], place[2].decode())], []).append(place + (int(s["pam_index"]),))
    bit = np.arange(L, dtype=np.uint32)
    for i, q in enumerate(queries):
        q = N.canon(q)
        mine = got.of(i)
        if not got.listed(i):
            assert len(mine) == 0 and int(got.near[i].sum()) > got.limit
            continue
        assert np.bincount(mine["mismatches"], minlength=M + 1).tolist() == got.near[i].tolist(), (i, q)
        far = mine[mine["mismatches"] > 0]
        if scores is not None:
            assert int(far["score_q32"].astype(object).sum()) == int(scores.sum_q32[i]) and int(far["score_q32"].max(initial=0)) == int(scores.max_q32[i]), (i, q)
        else:
            assert (mine["score_q32"] == ONE).all()
        assert (mine[mine["mismatches"] == 0]["score_q32"] == ONE).all()
        assert [(int(h["contig_index"]), int(h["protospacer_start"]), h["strand"], int(h["pam_index"])) for h in mine[mine["mismatches"] == 0]] == own_of.get(q, []), (i, q)
        # diff_mask and the planes give the query back: a position differs exactly where the mask says so
        codes = ((mine["target_lo"][:, None] >> bit) & 1) | (((mine["target_hi"][:, None] >> bit) & 1) << 1)
        differs = codes != np.array([IDX[c] for c in q], dtype=np.uint32)
        assert (differs == (((mine["diff_mask"][:, None] >> bit) & 1) == 1)).all() and (mine["diff_mask"] >> np.uint32(L - 1) <= 1).all(), (i, q)
        assert (differs.sum(axis=1) == mine["mismatches"]).all() and (mine["mismatches"] <= M).all()
        for h in mine[:3]:
            t, mask = letters_of(h, L), int(h["diff_mask"])
            assert all((t[j] != q[j]) == bool((mask >> j) & 1) for j in range(L)), (q, t, mask)
            assert got.target(h).upper() == t and [c.islower() for c in got.target(h)] == [bool((mask >> j) & 1) for j in range(L)]


def hold(C, ctx, pattern, queries, M, mismatch, table, paths, limit=1000, **region):
    """One call on every path of `paths` (host=True: the host twin, False: the device) against the referee's bytes, a second call
    against the first, and the invariants.  Returns the last path's NearList."""
    rows, offsets, data, _ = answer(table, queries, M, mismatch, limit)
    model = None if mismatch is None else S.model_of(C, mismatch)
    got = None
    for host in paths:
        got = ctx.list_near(pattern, queries, M, model, limit=limit, host=host, **region)
        assert got.near.dtype == np.uint64 and got.near.shape == (len(queries), M + 1)
        assert got.near.tolist() == rows, (host, M, region)
        assert got.offsets.tolist() == offsets, (host, M, region)
        assert got.hits.tobytes() == data, (host, M, region, first_difference(got.hits, data))
        again = ctx.list_near(pattern, queries, M, model, limit=limit, host=host, **region)
        assert again == got and again.hits.tobytes() == data and again.near.tobytes() == got.near.tobytes()
        check_invariants(C, ctx, pattern, queries, M, mismatch, got, table, host, region)
    return got


def first_difference(hits, data):
    want = np.frombuffer(data, dtype=DTYPE)
    for i in range(min(len(hits), len(want))):
        if hits[i].tobytes() != want[i].tobytes():
            return i, hits[i], want[i]
    return len(hits), len(want)


def planted_case(name, L, seqs, expect, sites):
    """(pattern, queries, table) of a pattern on the planted genome."""
    counts, _ = X.copies(seqs, name, L, sites=sites)
    queries = S.RUNS32 if name == "n32" else S.planted_queries(expect, name, counts, L, seed=L + len(name))
    text, aux = X.pattern_string(name)
    return (text, aux), queries, table_of(sites, seqs)


def hold_planted(C, ctx, name, L, M, weighted, paths, seqs, expect, sites):
    (text, aux), queries, table = planted_case(name, L, seqs, expect, sites)
    got = hold(C, ctx, C.Guide(text, aux), queries, M, S.distinct_mismatch(L) if weighted else None, table, paths)
    if name == "n20_nrg":
        check_planted(got, queries, expect, M, table)
    if name == "n20_nngrrt_nrg":
        assert {int(k) for k in got.hits["pam_index"]} == {0, 1}
    if name == "n32":
        assert set(got.hits["pam_index"].tolist()) == {-1} and {int(h["target_lo"]) for h in got.hits if h["mismatches"] == 0} >= {0, 0xFFFFFFFF}
    return got


def check_planted(got, queries, expect, M, table):
    """The planted cases the listing is there for are in the result: '-' sites, the U / u sites, a duplicated query with its full
    stretch twice, and the two neighbours that list each other's site."""
    assert (got.hits["strand"] == b"-").any() and (got.hits["strand"] == b"+").any()
    canon = [N.canon(q) for q in queries]
    twice = next(q for q in canon if canon.count(q) > 1 and int(got.near[canon.index(q)].sum()) > 0)
    first, second = [i for i, q in enumerate(canon) if q == twice][:2]
    assert len(got.of(first)) > 0 and got.of(first).tobytes() == got.of(second).tobytes()
    xs = next(q for case, name, K, m, q, _ in expect if case == "rules" and m == M)
    assert got.near[canon.index(xs)].tolist() == ([0, 7, 0, 0])[:M + 1] and len(got.of(canon.index(xs))) == 7       # two of them beside a U / u
    y, y2 = [q for case, name, K, m, q, _ in expect if case == "neighbours" and m == M]
    a, b = got.of(canon.index(y)), got.of(canon.index(y2))
    assert a["mismatches"].tolist() == [0, 1] == b["mismatches"].tolist()[::-1]
    assert a["protospacer_start"].tolist() == b["protospacer_start"].tolist() and a["diff_mask"].tolist() == [0, 1 << 10]


def pick_limit(table, queries, M):
    """The largest limit that one query's counts sum to exactly while another's sum to one more -- both kinds exist."""
    sums = {sum(row) for row, _ in expected(table, queries, M, None, LIST_MAX).values()}
    limits = [s for s in sums if s >= 1 and s + 1 in sums]
    assert limits, sorted(sums)
    return max(limits)


def hold_limit(C, ctx, paths, seqs, expect, sites):
    (text, aux), queries, table = planted_case("n20_nrg", 20, seqs, expect, sites)
    limit = pick_limit(table, queries, 3)
    got = hold(C, ctx, C.Guide(text, aux), queries, 3, S.distinct_mismatch(20), table, paths, limit=limit)
    sums = got.near.sum(axis=1).tolist()
    at, over = sums.index(limit), sums.index(limit + 1)
    assert got.listed(at) and len(got.of(at)) == limit and not got.listed(over) and len(got.of(over)) == 0 and int(got.near[over].sum()) == limit + 1
    return limit


def hold_seams(C, ctx, name, seqs, sites, paths):
    """A seam genome: the listing against the referee at M = 1 and 3, per-contig listings merging to the whole, a region across base 8192."""
    L = len(X.PATTERNS[name][0])
    text, aux = X.pattern_string(name)
    pat = C.Guide(text, aux)
    counts, _ = X.copies(seqs, name, L, sites=sites)
    queries = N.queries_for(counts, L, seed=L * 100 + len(name), cap=80)
    mismatch = S.distinct_mismatch(L)
    table = table_of(sites, seqs)
    whole = None
    for M in (1, 3):
        whole = hold(C, ctx, pat, queries, M, mismatch, table, paths)
        assert {b"+", b"-"} == set(whole.hits["strand"].tolist())
        for host in paths:
            assert whole.near.tobytes() == ctx.count_near(pat, queries, M, host=host).tobytes()
        parts = [ctx.list_near(pat, queries, M, S.model_of(C, mismatch), chrom=i, host=paths[-1]) for i in range(len(seqs))]
        for i, part in enumerate(parts):
            rows, offsets, data, _ = answer([t for t in table if t[0] == i], queries, M, mismatch, 1000)
            assert (part.near.tolist(), part.offsets.tolist(), part.hits.tobytes()) == (rows, offsets, data), (M, i)
        assert parts[0].merge(*parts[1:]) == whole and parts[-1].merge(*parts[:-1]) == whole
    inside = [t for t in table_of(R.brute_sites(seqs, *X.PATTERNS[name], 0, 8100, 8300), seqs)]
    hold(C, ctx, pat, queries, 3, mismatch, inside, paths, chrom=0, start=8100, end=8300)
    return whole


def hold_sweep(C, ctx, L, seqs, sites, paths):
    """A protospacer length at its largest legal M.  The limit of 300 keeps the referee's work small and lies beyond the 64 records up
    to which a stretch is ordered by one wave; the shortest lengths, where every site is near every query, list nothing."""
    M = min(3, L - 1)
    counts = X.count_keys(sites, seqs, L, False)
    queries = N.queries_for(counts, L, seed=L * 40, cap=40, n_absent=5)
    return hold(C, ctx, "N" * L, queries, M, S.distinct_mismatch(L), table_of(sites, seqs), paths, limit=300)


def contended_genome(seed=91):
    """(names, strings, x, run): one contig of < 60 kb with 720 copies of a 20-mer + TGG -- every third one itself, the others with one
    substitution -- 40 bases apart over more than three segments of 8192 bases, alternating strands; behind them AGG x 5000, whose
    4990-odd overlapping '+' sites carry one key, `run`."""
    rng = random.Random(seed)
    x = X._distinct(rng, 1, need="ACGT")[0]
    parts = []
    for u in range(720):
        unit = (x if u % 3 == 0 else N.swap(x, u % 20)) + "TGG"
        parts.append(R.revcomp(unit) if u % 2 else unit)
        parts.append(R._rand(rng, 17))
    parts.append("AGG" * 5000)
    parts.append(R._rand(rng, 40))
    seq = "".join(parts)
    assert 3 * 8192 < 720 * 40 and len(seq) <= 60000
    return ["chrH"], [seq], x, ("AGG" * 7)[1:]


def hold_contended(C, ctx, paths, seqs, x, run, sites):
    """Many waves and workgroups on one cursor, a stretch longer than a workgroup; and a key beyond the largest limit."""
    table = table_of(sites, seqs)
    pat = "N" * 20 + "nrg"
    got = hold(C, ctx, pat, [x, run, N.swap(x, 4)], 1, S.distinct_mismatch(20), table, paths, limit=LIST_MAX)
    assert got.near[0].tolist()[0] >= 240 and int(got.near[0].sum()) >= 600 and len(got.of(0)) == int(got.near[0].sum())
    mine = got.of(0)
    assert len({int(p) // 8192 for p in mine["protospacer_start"]}) >= 3 and {b"+", b"-"} == set(mine["strand"].tolist())
    assert int(got.near[1].sum()) > LIST_MAX and not got.listed(1) and len(got.of(1)) == 0
    return got


def hold_reused(C, ctx, seqs, host):
    """list_near, score_near, count_near and count_copies interleaved on one context, the large call first, with M and the limit changing:
    the tables, counters and record buffers are shared, nothing stale may show."""
    sites = R.brute_sites(seqs, "N" * 8, ["ngg"], False)
    counts = X.count_keys(sites, seqs, 8, False)
    table = table_of(sites, seqs)
    keys = sorted(counts)
    assert len(keys) > 1100
    pat, mismatch = "NNNNNNNNngg", S.distinct_mismatch(8)
    model = S.model_of(C, mismatch)
    for n, M, what in ((None, 1, "list"), (3, 3, "near"), (7, 0, "list"), (9, 0, "copies"), (1025, 2, "list"), (2, 1, "score"), (600, 3, "list"),
                       (5, 2, "copies"), (1, 3, "list"), (40, 2, "near"), (40, 2, "plain")):
        queries = keys if n is None else keys[::max(1, len(keys) // 1100)][:n]
        if what in ("list", "plain"):
            limit = 50 if M == 3 else 1000
            weights = mismatch if what == "list" else None
            rows, offsets, data, _ = answer(table, queries, M, weights, limit)
            got = ctx.list_near(pat, queries, M, model if what == "list" else None, limit=limit, host=host)
            assert (got.near.tolist(), got.offsets.tolist()) == (rows, offsets) and got.hits.tobytes() == data, (n, M, what)
        elif what == "score":
            rows, sums, tops, _ = S.table_for(counts, queries, M, mismatch)
            got = ctx.score_near(pat, queries, M, model, host=host)
            assert (got.near.tolist(), got.sum_q32.tolist(), got.max_q32.tolist()) == (rows, sums, tops), (n, M)
        elif what == "near":
            assert ctx.count_near(pat, queries, M, host=host).tolist() == N.rows_for(counts, queries, M), (n, M)
        else:
            assert ctx.count_copies(pat, queries, host=host).tolist() == [counts[k] for k in queries], n


def hold_errors(C, ctx, host):
    """The errors in their order: what score_near refuses first -- a missing model is legal -- then the limit."""
    EINVAL = C._lib.EINVAL
    pat, q20 = "N" * 20 + "nrg", ["ACGT" * 5]
    bad_model = C.ScoreModel.uniform(19)
    over = C.ScoreModel.uniform(20)
    over.mismatch[7, 2, 1] = 65537

    def refused(word, *args, **kw):
        with S.pytest_raises(C) as e:
            ctx.list_near(*args, host=host, **kw)
        assert e.value.code == EINVAL and word in str(e.value), (word, str(e.value))

    for M in (-1, 4):
        refused("max_mismatches", pat, q20, M, bad_model, limit=0)      # before the region, the queries, the model and the limit
        refused("max_mismatches", pat, ["ACGTN" * 4], M, None, chrom=0, start=50, end=20)
    refused("region", pat, ["ACGTN" * 4], 1, bad_model, limit=0, chrom=0, start=50, end=20)
    refused("queries[1]", pat, ["ACGT" * 5, "ACGTN" * 4], 2, bad_model, limit=0)
    refused("max_mismatches + 1", "NNNngg", ["ACG"], 3, C.ScoreModel.uniform(2), limit=0)
    refused("19 bases", pat, q20, 1, bad_model, limit=0)                # the model before the limit
    refused("above 65536", pat, q20, 1, over, limit=4097)
    for limit in (0, 4097):
        refused("limit", pat, q20, 1, None, limit=limit)
        refused("limit", pat, q20, 1, C.ScoreModel.uniform(20), limit=limit)
        refused("limit", pat, [], 1, None, limit=limit)
    for limit in (1, 4096):
        assert ctx.list_near(pat, q20, 1, None, limit=limit, host=host).near.shape == (1, 2)
    with S.pytest_raises(C, ValueError):
        ctx.list_near(pat, ["ACGT"], 1, host=host)                      # not the protospacer's length
    none = ctx.list_near(pat, [], 2, host=host)                         # no query is legal
    assert none.near.shape == (0, 3) and none.offsets.tolist() == [0] and len(none.hits) == 0 and none.hits.dtype == DTYPE
    refused("19 bases", pat, [], 2, bad_model)


def check_contract_function(C, table, queries, M, mismatch):
    """near_hits_of, the contract on one query in plain Python, against the referee."""
    model = None if mismatch is None else S.model_of(C, mismatch)
    exp = expected(table, queries, M, mismatch, 1 << 30)
    for q in queries:
        got = C.near_hits_of(q, table, M, model)
        assert [tuple(h[f] if f != "strand" else h[f].encode() for f in DTYPE.names) for h in got] == exp[N.canon(q)][1], q
        assert all(h["target"] == letters_of(h, len(q)) for h in got)


def tsv_of(rows, names, table, M, mismatch, limit):
    """The --near-list file by the referee: rows are (guide_id, query) pairs."""
    exp = expected(table, [q for _, q in rows], M, mismatch, limit)
    key_at = {(t[0], t[1], t[2]): t[4] for t in table}
    lines = ["guide_id\tchromosome\tstart\tend\tstrand\tpam_index\tmismatches\ttarget\tscore_q32\tscore"]
    for guide_id, q in rows:
        for score, c, p, lo, hi, mask, strand, k, d, _ in exp[N.canon(q)][1]:
            key = key_at[(c, p, strand.decode())]
            target = "".join(ch.lower() if (mask >> i) & 1 else ch for i, ch in enumerate(key))
            lines.append("\t".join([guide_id, names[c], str(p), str(p + len(key)), strand.decode(), str(k), str(d), target, str(score), "%.6f" % (score / 2.0 ** 32)]))
    return "\n".join(lines) + "\n"
