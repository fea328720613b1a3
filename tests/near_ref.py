"""The referee of the near-copies tests (test_near_host.py, test_gpu_near.py): Python on strings that shares no code with the library.
It starts from sites_ref.brute_sites, cuts each site's key from the contig string as copies_ref.key_of does, and compares the keys'
LETTERS with each query's, position by position: near() gives {query: [sites at distance 0, 1, .. M]}.  The comparison is written
twice -- distance(), one letter after the other, and near()'s, the same comparison over a byte array of all distinct keys at once (the
genomes of the GPU tests hold 200 000 keys) -- and check_planted() holds the two against each other.  near_genome() is a contig set of
less than 16 kb with the cases the contract names planted; check_planted() asserts on this referee alone that each yields its row."""
import random

import numpy as np

import copies_ref as X
import sites_ref as R

MAX_M = 3
PATTERNS = X.PATTERNS
# (pattern, key length) of copies_ref.CASES; every M = 0 .. 3 with K >= M + 1 goes with each
CASES = X.CASES


def legal(K, M):
    return K >= M + 1


def piece_width(K, M):
    """The library's starting choice (the contract does not depend on it; the planted cases are laid out around it)."""
    return min(K // (M + 1), 8)


def distance(a, b):
    """The number of positions at which two strings of one length differ."""
    assert len(a) == len(b)
    return sum(1 for x, y in zip(a, b) if x != y)


def canon(q):
    return q.upper().replace("U", "T")


def near(key_counts, queries, M=MAX_M):
    """{canonical query: [number of sites whose key is at distance d, d = 0 .. M]} from {key: sites that carry it} (copies_ref.copies)."""
    keys = sorted(key_counts)
    out = {}
    if not keys:
        return {canon(q): [0] * (M + 1) for q in queries}
    K = len(keys[0])
    letters = np.frombuffer("".join(keys).encode(), dtype=np.uint8).reshape(len(keys), K)
    weight = np.array([key_counts[k] for k in keys], dtype=np.int64)
    for q in queries:
        q = canon(q)
        if q in out:
            continue
        assert len(q) == K
        d = (letters != np.frombuffer(q.encode(), dtype=np.uint8)).sum(axis=1)
        out[q] = [int(weight[d == x].sum()) for x in range(M + 1)]
    return out


def near_by_letters(key_counts, query, M=MAX_M):
    """near() for one query, one letter after the other."""
    row = [0] * (M + 1)
    for k, n in key_counts.items():
        d = distance(k, canon(query))
        if d <= M:
            row[d] += n
    return row


def rows_for(key_counts, queries, M):
    """The (len(queries), M + 1) table a call returns, as a list of lists."""
    table = near(key_counts, queries, M)
    return [table[canon(q)] for q in queries]


def swap(x, *at):
    """x with another letter at each of the positions."""
    for i in at:
        x = x[:i] + {"A": "C", "C": "G", "G": "T", "T": "A"}[x[i]] + x[i + 1:]
    return x


def queries_for(key_counts, K, seed, cap=200, n_absent=20):
    """Queries of a comparison: distinct site keys (every one up to `cap`, a spread of them beyond), one- and two-substitution variants
    of some of them, keys that do not occur, duplicates, lower case and U for T."""
    rng = random.Random(seed)
    keys = sorted(key_counts)
    some = keys if len(keys) <= cap else keys[::len(keys) // cap][:cap]
    queries = list(some)
    picked = [rng.choice(keys) for _ in range(12)] if keys else []
    for k in picked:
        i = rng.randrange(K)
        queries.append(swap(k, i))
        if K >= 2:
            queries.append(swap(k, i, (i + 1 + rng.randrange(K - 1)) % K))
    queries += X.absent_keys(key_counts, K, n_absent, seed)
    queries += picked[:6] + picked[:2]                                  # duplicates: each gets the full row
    queries += [k.lower() for k in picked[6:9]]
    queries += [k.replace("T", "U") for k in picked[9:11]] + [k.lower().replace("t", "u") for k in picked[11:]]
    rng.shuffle(queries)
    return queries


# ---- the planted genome ----

def near_genome(seed=53):
    """(names, strings, expect): expect is a list of (case, pattern name, K, M, query, row) that check_planted holds against the referee;
    row[d] = the sites at distance d.  For N20 + nrg at K = 20 the pieces are, at M = 1, 2, 3, of w = 8, 6, 5 bases: [0, 8) [8, 16) with
    positions 16 .. 19 in no piece; [0, 6) [6, 12) [12, 18) with 18, 19 in none; [0, 5) [5, 10) [10, 15) [15, 20).  A base 20-mer per M
    (x1, x2, x3) stands once itself (column 0) and then as copies with substitutions, each next to TGG on '+' unless said otherwise:
      ends        one substitution at guide position 0, one at L - 1: d = 1
      boundaries  one substitution on either side of every piece boundary (w, 2 w, .. and (M + 1) w where positions are left over): d = 1
      outside     M = 1: one substitution at position 17, which lies in no piece: d = 1
      layouts     M substitutions, one in the middle of every piece but one, for each choice of the clean piece: M + 1 copies at d = M
      every       M + 1 substitutions, one in every piece: not counted
      one_piece   M + 1 substitutions in piece 0, every other piece clean: d = M + 1, not counted
      (a copy with ONE substitution has M clean pieces and must count once: column 1 is exact)
    xs, at M = 1, 2, 3, and the same rows: a copy with one substitution on '-'; next to AGG, TGG, CGG; in front of TTT (no site); with
    an N and with a reference R inside (no site); soft-masked; with U for a T on '+' and with u for a T of the forward text of a
    reverse-complemented copy (counted through the host's correction).  xs itself does not stand anywhere: column 0 is 0.
    y and y' = y with another letter at position 10, each once: each sees the other's site at d = 1.
    xo, never itself: a copy with one substitution on cpA's first base, ending on cpB's last base, with base 8192 of cpA inside its
    protospacer, and at every start bit offset 0 .. 31 of a 32-base word, 16 on '+' and 16 on '-': [0, 35].
    Seeds at K = 12, M = 2 (w = 4): s once; with a substitution at guide position 7 (outside the seed: d = 0), at 8 (the seed's first
    base, d = 1), at 8 and 19 (d = 2), at 9, 13 and 17 (one per piece, not counted): [2, 1, 1].  The same for tttv + N20, where the seed
    is the first 12 bases: p; substitutions at 12 (outside), at 11, at 0 and 11, at 1, 5 and 9: [2, 1, 1].
    N x 32 (every window is a site) at K = 32, M = 3 (w = 8): GCGC + A x 40 + GCGC and GCGC + T x 40 + GCGC.  A x 32 (key 0) stands 9
    times in the first run on '+' and 9 times in the second on '-'; the windows that take 1, 2, 3 flank bases in at either end are its
    copies with that many substitutions, those with 4 are not counted: [18, 4, 4, 4], and the same for T x 32 (all ones).
    sites_ref.FIXED + AGG once on cpC, the one site of the pattern FIXED + nrg: a query one substitution from FIXED -- which the
    pattern's own letters exclude as a site -- sees it at d = 1."""
    rng = random.Random(seed)
    x1, x2, x3, xs, y, xo, s0, p0 = X._distinct(rng, 8, need="ACGT")
    expect = []
    a, at = [], [0]

    def put(text):
        a.append(text)
        at[0] += len(text)

    def gap(n=7):
        put(R._rand(rng, n))

    def unit(x, pam="TGG", minus=False):
        put(R.revcomp(x + pam) if minus else x + pam)
        gap()

    first = swap(xo, 5)
    unit(first)                                             # on cpA's first base
    gap(30)
    for M, x in ((1, x1), (2, x2), (3, x3)):
        w = piece_width(20, M)
        assert w == {1: 8, 2: 6, 3: 5}[M]
        row = [0] * (M + 1)
        unit(x)
        row[0] += 1
        singles = [0, 19] + [b + s for b in range(w, (M + 1) * w + 1, w) if b < 20 for s in (-1, 0)] + ([17] if M == 1 else [])
        assert len(set(singles)) == len(singles)
        for i in singles:
            unit(swap(x, i))
            row[1] += 1
        for clean in range(M + 1):                          # M substitutions, one per piece but `clean`
            unit(swap(x, *[p * w + w // 2 for p in range(M + 1) if p != clean]))
            row[M] += 1
        unit(swap(x, *[p * w + 1 for p in range(M + 1)]))   # one in every piece
        unit(swap(x, *range(M + 1)))                        # M + 1 in piece 0
        assert M + 1 <= w
        expect.append(("pieces", "n20_nrg", 20, M, x, row))
    # the site rules, on copies with one substitution
    i_t = xs.index("T")
    i_s = (i_t + 7) % 20                                    # the substituted position, not the T
    v = swap(xs, i_s)
    unit(v, minus=True)
    unit(v, "AGG"); unit(v, "TGG"); unit(v, "CGG")
    unit(v, "TTT")
    unit(v[:6] + "N" + v[7:]); unit(v[:11] + "R" + v[12:])
    put((v + "TGG").lower()); gap()
    unit(v[:i_t] + "U" + v[i_t + 1:])
    fwd = R.revcomp(v + "TGG")
    j = fwd.index("T", 3)
    put(fwd[:j] + "u" + fwd[j + 1:]); gap()
    for M in (1, 2, 3):
        expect.append(("rules", "n20_nrg", 20, M, xs, ([0, 7, 0, 0])[:M + 1]))
    y2 = swap(y, 10)
    unit(y); unit(y2)
    for M in (1, 2, 3):
        expect += [("neighbours", "n20_nrg", 20, M, y, ([1, 1, 0, 0])[:M + 1]), ("neighbours", "n20_nrg", 20, M, y2, ([1, 1, 0, 0])[:M + 1])]
    # every bit offset: contigs start on a multiple of 32, so protospacer_start % 32 is the bit of the lane's word
    for off in range(32):
        minus = off >= 16
        lead = 3 if minus else 0                            # on '-' the PAM's complement stands in front of the protospacer
        put(R._rand(rng, (off - (at[0] + lead)) % 32 + 32))
        unit(swap(xo, 14), minus=minus)
    # the seeds
    for sx in (s0, swap(s0, 7), swap(s0, 8), swap(s0, 8, 19), swap(s0, 9, 13, 17)):
        unit(sx)
    expect.append(("seed", "n20_nrg", 12, 2, s0[-12:], [2, 1, 1]))
    for px in (p0, swap(p0, 12), swap(p0, 11), swap(p0, 0, 11), swap(p0, 1, 5, 9)):
        put("TTTA" + px + "C"); gap()
    expect.append(("seed5", "tttv_n20", 12, 2, p0[:12], [2, 1, 1]))
    assert piece_width(12, 2) == 4
    assert at[0] < 8192 - 40, at[0]
    put(R._rand(rng, 8192 - 9 - at[0]))
    unit(swap(xo, 2))                                       # protospacer [8183, 8203)
    gap(200)
    b = [R._rand(rng, 1200), swap(xo, 9) + "TGG"]           # ends on cpB's last base
    for M in (1, 2, 3):
        expect.append(("places", "n20_nrg", 20, M, xo, ([0, 35, 0, 0])[:M + 1]))

    def calm(n):
        """n random bases without a run of three: no window of 32 comes near A x 32 or T x 32."""
        out = ""
        while len(out) < n:
            c = rng.choice("ACGT")
            if out[-2:] != c * 2:
                out += c
        return out

    c = [calm(300), "GCGC" + "A" * 40 + "GCGC", calm(150), "GCGC" + "T" * 40 + "GCGC", calm(200), R.FIXED + "AGG", calm(100)]
    expect += [("fixed", "fixed_nrg", 20, 3, R.FIXED, [1, 0, 0, 0]), ("fixed", "fixed_nrg", 20, 3, swap(R.FIXED, 3), [0, 1, 0, 0])]
    expect += [("runs", "n32", 32, 3, "A" * 32, [18, 4, 4, 4]), ("runs", "n32", 32, 3, "T" * 32, [18, 4, 4, 4])]
    seqs = ["".join(a), "".join(b), "".join(c)]
    assert sum(len(s) for s in seqs) <= 16000, [len(s) for s in seqs]
    return ["cpA", "cpB", "cpC"], seqs, expect


def check_planted(seqs, expect):
    """Every planted case yields its row, by this referee alone and by both of its comparisons; the copies of the `places` case lie on
    cpA's first base, on cpB's last, across base 8192 and at the 32 bit offsets, 16 on each strand."""
    done = {}
    for case, name, K, M, query, row in expect:
        if (name, K) not in done:
            done[(name, K)] = X.copies(seqs, name, K)[0]
        got = near(done[(name, K)], [query], M)[query]
        assert got == row, (case, name, K, M, query, got, row)
        assert near_by_letters(done[(name, K)], query, M) == row, (case, name, K, M, query)
    xo = next(q for case, _, _, _, q, _ in expect if case == "places")
    sites = [s for s in R.brute_sites(seqs, *R.PATTERNS["n20_nrg"]) if distance(X.key_of(s, seqs, 20, False), xo) == 1]
    assert len(sites) == 35
    assert any(s[0] == 0 and s[1] == 0 for s in sites) and any(s[0] == 1 and s[1] + 23 == len(seqs[1]) for s in sites)
    assert any(s[0] == 0 and s[1] < 8192 < s[1] + 19 for s in sites)
    swept = [s for s in sites if X.key_of(s, seqs, 20, False) == swap(xo, 14)]
    assert {s[1] % 32 for s in swept if s[3] == "+"} == set(range(16)) and {s[1] % 32 for s in swept if s[3] == "-"} == set(range(16, 32))
