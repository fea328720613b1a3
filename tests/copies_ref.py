"""The referee of the copies tests (test_copies_host.py, test_gpu_copies.py): plain Python on strings that shares no code with the
library.  It runs sites_ref.brute_sites over the genome without a filter, cuts each protospacer from the contig string with an
explicit reverse complement for '-', takes the PAM-proximal K letters -- the last K for a 3' PAM and for a PAM-less pattern, the first
K for a 5' PAM -- and counts them in a dict.  copies_genome() is a contig set of less than 12 kb with the cases the contract names
planted, for N20 + nrg unless said otherwise; check_planted() asserts on this referee alone that each case yields its count."""
import random

import sites_ref as R

X_LEN = 20
# sites_ref's patterns and the PAM-less one of the a_run case
PATTERNS = dict(R.PATTERNS, n32=("N" * 32, [], False))
# (pattern of sites_ref.PATTERNS, key length): what both test files run on every genome
CASES = [("n20_nrg", 20), ("n20_nrg", 12), ("n20_nrg", 1), ("tttv_n20", 20), ("tttv_n20", 12), ("n20_nngrrt_nrg", 20), ("fixed_nrg", 20),
         ("eight_pams", 20), ("n21", 21), ("n21", 10)]


def key_of(site, contigs, K, five):
    """The key of a brute_sites tuple: the protospacer as the guide reads (upper case, U as T, the reverse complement on '-'), its first
    K letters when the PAM stands in front of it, its last K otherwise."""
    c, p, _, strand, _, _, L = site
    text = contigs[c][p:p + L].upper().replace("U", "T")
    if strand == "-":
        text = R.revcomp(text)
    return text[:K] if five else text[L - K:]


def count_keys(sites, contigs, K, five):
    """{key: number of sites that carry it}."""
    out = {}
    for s in sites:
        k = key_of(s, contigs, K, five)
        out[k] = out.get(k, 0) + 1
    return out


def copies(contigs, name, K, chrom=None, start=0, end=None, sites=None):
    """({key: count}, number of sites) of a pattern of PATTERNS in a region; sites: its brute_sites listing, where the caller
    has it already."""
    proto, pams, five = PATTERNS[name]
    if sites is None:
        sites = R.brute_sites(contigs, proto, pams, five, chrom, start, end)
    return count_keys(sites, contigs, K, five and bool(pams)), len(sites)


def absent_keys(counts, K, n, seed):
    """Up to n distinct K-letter keys that no site carries (fewer where fewer exist: at K = 1 every letter may be taken)."""
    rng = random.Random(seed)
    out = []
    for _ in range(200 * n):
        k = R._rand(rng, K)
        if k not in counts and k not in out:
            out.append(k)
            if len(out) == n:
                break
    return out


def queries_for(counts, K, seed, n_absent=50):
    """(queries, expected): every distinct key, n_absent keys that do not occur, duplicates, lower case and U for T."""
    rng = random.Random(seed)
    keys = sorted(counts)
    queries = keys + absent_keys(counts, K, n_absent, seed)
    some = [rng.choice(keys) for _ in range(8)] if keys else []
    queries += some + some[:3]                                        # duplicates: each gets the full count
    queries += [k.lower() for k in some[:4]]
    queries += [k.replace("T", "U") for k in some[4:6]] + [k.lower().replace("t", "u") for k in some[6:]]
    rng.shuffle(queries)
    return queries, [counts.get(q.upper().replace("U", "T"), 0) for q in queries]


# ---- the planted genome ----

def _distinct(rng, n, need=""):
    """n random 20-mers, each holding the letters of `need`, no two sharing their last or their first 12 letters."""
    out = []
    while len(out) < n:
        x = R._rand(rng, X_LEN)
        if all(b in x for b in need) and all(x[-12:] != y[-12:] and x[:12] != y[:12] for y in out) and "GGGG" not in x and "CCCC" not in x:
            out.append(x)
    return out


def _swap(x, i):
    """x with another letter at guide position i."""
    return x[:i] + {"A": "C", "C": "G", "G": "T", "T": "A"}[x[i]] + x[i + 1:]


def copies_genome(seed=41):
    """(names, strings, expect): expect is a list of (case, pattern name, K, key, copies) that check_planted holds against the referee.
    The cases, for N20 + nrg and K = 20 where nothing else is said:
      once        X + TGG once
      twice       X + AGG twice on '+'
      both        X + TGG on '+' and its reverse complement: once on each strand
      three_pams  X + AGG, X + TGG, X + CGG
      non_pam     X + TGG and X + TTT: the second is no site
      n_inside    X + TGG, X with an N inside + TGG, X with a reference R inside + TGG: 1
      soft        X + TGG and the same in lower case: 2
      u           X + TGG, a copy with U for one T of the protospacer on '+', the reverse complement with u for one T of its forward text: 3
      contigs     X + TGG on the first base of cpA, ending on the last base of cpB and inside cpC: 3
      offsets     X + TGG once at every bit offset 0 .. 31 of a 32-base word, 16 offsets on '+' and the other 16 on '-': 32
      straddle    X + TGG with base 8192 of cpA inside its protospacer
      seed        K = 12: S twice, S' (differs from S at guide position 7 = L - K - 1: the same seed) once, S" (differs at 8 = L - K, the
                  seed's outermost base) once -- copies 2, 1, 1 and seed copies 3, 3, 1
      seed5       the same for tttv + N20, where the seed is the first 12 bases: P twice, P' (differs at 12) once, P" (differs at 11) once
      palindrome  CCA + a self-reverse-complementary 20-mer + TGG: a site on both strands with one key, 2
      g_run       G x 40: 18 overlapping '+' sites with the key G x 20 in two words of one wave (the hot counter); its reverse
                  complement C x 40 elsewhere holds 18 '-' sites with the same key: 36
      fixed       sites_ref.FIXED + AGG once on cpC: the one site of the pattern FIXED + nrg
      a_run       for the PAM-less N x 32 at K = 32: A x 40 and T x 40 give the keys A x 32 (key value 0) and T x 32 (all ones) 9 times on
                  '+' and 9 times on '-' each: 18 and 18"""
    rng = random.Random(seed)
    xs = _distinct(rng, 16, need="ACGT")
    (x_once, x_twice, x_both, x_three, x_non, x_n, x_soft, x_u, x_contigs, x_off, x_straddle, s0, p0, _, _, _) = xs
    half = R._rand(rng, 10)
    pal = half + R.revcomp(half)
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

    unit(x_contigs)                                         # on cpA's first base
    gap(30)
    unit(x_once)
    expect.append(("once", "n20_nrg", 20, x_once, 1))
    unit(x_twice, "AGG"); unit(x_twice, "AGG")
    expect.append(("twice", "n20_nrg", 20, x_twice, 2))
    unit(x_both); unit(x_both, minus=True)
    expect.append(("both", "n20_nrg", 20, x_both, 2))
    unit(x_three, "AGG"); unit(x_three, "TGG"); unit(x_three, "CGG")
    expect.append(("three_pams", "n20_nrg", 20, x_three, 3))
    unit(x_non); unit(x_non, "TTT")
    expect.append(("non_pam", "n20_nrg", 20, x_non, 1))
    unit(x_n); unit(x_n[:7] + "N" + x_n[8:]); unit(x_n[:9] + "R" + x_n[10:])
    expect.append(("n_inside", "n20_nrg", 20, x_n, 1))
    unit(x_soft); put((x_soft + "TGG").lower()); gap()
    expect.append(("soft", "n20_nrg", 20, x_soft, 2))
    unit(x_u)
    i = x_u.index("T")
    unit(x_u[:i] + "U" + x_u[i + 1:])
    fwd = R.revcomp(x_u + "TGG")                            # the PAM's complement CCA first, then the protospacer's
    j = fwd.index("T", 3)
    put(fwd[:j] + "u" + fwd[j + 1:]); gap()
    expect.append(("u", "n20_nrg", 20, x_u, 3))
    # every bit offset: contigs start on a multiple of 32, so protospacer_start % 32 is the bit of the lane's word
    for off in range(32):
        minus = off >= 16
        lead = 3 if minus else 0                            # on '-' the PAM's complement stands in front of the protospacer
        put(R._rand(rng, (off - (at[0] + lead)) % 32 + 32))
        unit(x_off, minus=minus)
    expect.append(("offsets", "n20_nrg", 20, x_off, 32))
    # the seeds
    s_same, s_other = _swap(s0, X_LEN - 12 - 1), _swap(s0, X_LEN - 12)
    unit(s0); unit(s0); unit(s_same); unit(s_other)
    expect += [("seed", "n20_nrg", 20, s0, 2), ("seed", "n20_nrg", 20, s_same, 1), ("seed", "n20_nrg", 20, s_other, 1),
               ("seed", "n20_nrg", 12, s0[-12:], 3), ("seed", "n20_nrg", 12, s_same[-12:], 3), ("seed", "n20_nrg", 12, s_other[-12:], 1)]
    assert s0[-12:] == s_same[-12:] != s_other[-12:]
    p_same, p_other = _swap(p0, 12), _swap(p0, 11)
    for p in (p0, p0, p_same, p_other):
        put("TTTA" + p + "C"); gap()
    expect += [("seed5", "tttv_n20", 20, p0, 2), ("seed5", "tttv_n20", 20, p_same, 1), ("seed5", "tttv_n20", 20, p_other, 1),
               ("seed5", "tttv_n20", 12, p0[:12], 3), ("seed5", "tttv_n20", 12, p_same[:12], 3), ("seed5", "tttv_n20", 12, p_other[:12], 1)]
    assert p0[:12] == p_same[:12] != p_other[:12]
    put("CCA" + pal + "TGG"); gap()
    expect.append(("palindrome", "n20_nrg", 20, pal, 2))
    put("A" + "G" * 40 + "A"); gap(40); put("T" + "C" * 40 + "T"); gap()
    expect.append(("g_run", "n20_nrg", 20, "G" * 20, 36))
    assert at[0] < 8192 - 40, at[0]
    put(R._rand(rng, 8192 - 9 - at[0]))
    unit(x_straddle)                                        # protospacer [8183, 8203)
    expect.append(("straddle", "n20_nrg", 20, x_straddle, 1))
    gap(200)
    b = [R._rand(rng, 1200), x_contigs + "TGG"]             # ends on cpB's last base
    c = [R._rand(rng, 300), x_contigs + "TGG", R._rand(rng, 200), "C" + "A" * 40 + "G", R._rand(rng, 90), "C" + "T" * 40 + "G", R._rand(rng, 50), R.FIXED + "AGG", R._rand(rng, 100)]
    expect.append(("fixed", "fixed_nrg", 20, R.FIXED, 1))
    expect.append(("contigs", "n20_nrg", 20, x_contigs, 3))
    expect += [("a_run", "n32", 32, "A" * 32, 18), ("a_run", "n32", 32, "T" * 32, 18)]
    seqs = ["".join(a), "".join(b), "".join(c)]
    assert sum(len(s) for s in seqs) <= 12000, [len(s) for s in seqs]
    return ["cpA", "cpB", "cpC"], seqs, expect


def pattern_string(name):
    """(the `-i` string, the auxiliary PAMs) of a pattern of PATTERNS."""
    proto, pams, five = PATTERNS[name]
    first = pams[0] if pams else ""
    return (first + proto) if five else (proto + first), pams[1:]


def check_planted(seqs, expect):
    """Every planted case yields its stated count, by this referee alone; the offsets case covers the 32 bit offsets, 16 on each
    strand; the straddle case lies across base 8192; the g_run sites on '+' lie in two words."""
    done = {}
    for case, name, K, key, n in expect:
        if (name, K) not in done:
            done[(name, K)] = copies(seqs, name, K)[0]
        assert done[(name, K)].get(key, 0) == n, (case, name, K, key, done[(name, K)].get(key, 0), n)
    sites = R.brute_sites(seqs, *R.PATTERNS["n20_nrg"])
    key = {case: k for case, name, K, k, _ in expect if name == "n20_nrg" and K == 20}
    seen = {"+": set(), "-": set()}
    for s in sites:
        k = key_of(s, seqs, 20, False)
        if k == key["offsets"]:
            seen[s[3]].add(s[1] % 32)
        if k == key["straddle"]:
            assert s[0] == 0 and s[1] < 8192 < s[1] + 19
        if k == key["contigs"]:
            assert (s[0], s[1]) in ((0, 0), (1, len(seqs[1]) - 23)) or s[0] == 2
    assert seen["+"] == set(range(16)) and seen["-"] == set(range(16, 32)), seen
    runs = [s for s in sites if key_of(s, seqs, 20, False) == "G" * 20]
    assert len({s[1] // 32 for s in runs if s[3] == "+"}) <= 2 and sum(s[3] == "+" for s in runs) == 18 and sum(s[3] == "-" for s in runs) == 18


def random_contig(seed=77, n=60000):
    """One contig of n random A C G T (the table-size steps and the contended counters)."""
    return ["chrR"], [R._rand(random.Random(seed), n)]
