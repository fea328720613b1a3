"""The referee of the site-filter tests (test_site_filters_host.py, test_gpu_site_filters.py): plain Python on strings that shares no
code with the library.  It takes sites_ref.brute_sites' tuples and the contig strings, cuts each protospacer out, takes an explicit
reverse complement for '-', counts G and C, searches `b * (r + 1) in proto` and holds motifs letter by letter against sites_ref.IUPAC.
filter_genome() is a contig of less than 12 kb with the cases the contract names planted for N20 + nrg on both strands."""
import random

import sites_ref as R

OPEN = dict(gc_min=0, gc_max=255, max_run=(0, 0, 0, 0), avoid=())

# The filters of the tests, as keyword arguments of passes() and of calitas_amd.SiteFilter alike; the GC bounds are those of 40 - 60 %
# for the protospacer length given.
BSMBI = ("CGTCTC", "GAGACG")


def percent(L, lo, hi):
    return -((-lo * L) // 100), (hi * L) // 100


def filters(L):
    g0, g1 = percent(L, 40, 60)
    return {
        "gc": dict(gc_min=g0, gc_max=g1),
        "runs3": dict(max_run=(3, 3, 3, 3)),
        "t3": dict(max_run=(0, 0, 0, 3)),
        "bsmbi": dict(avoid=BSMBI),
        "all": dict(gc_min=g0, gc_max=g1, max_run=(4, 4, 4, 3), avoid=BSMBI + ("GGNCC",)),
    }


# ... and those only the planted cases need
EXTRA = {
    "ggncc": dict(avoid=("GGNCC",)),
    "cgtctc_only": dict(avoid=("CGTCTC",)),
    "g3": dict(max_run=(0, 0, 3, 0)),
}


def protospacer(site, contigs):
    """The protospacer of a brute_sites tuple as the guide reads: upper case, U as T, the reverse complement on '-'."""
    c, p, _, strand, _, _, L = site
    text = contigs[c][p:p + L].upper().replace("U", "T")
    return R.revcomp(text) if strand == "-" else text


def passes(proto, gc_min=0, gc_max=255, max_run=(0, 0, 0, 0), avoid=()):
    gc = proto.count("G") + proto.count("C")
    if not gc_min <= gc <= min(gc_max, len(proto)):
        return False
    for b, r in zip("ACGT", max_run):
        if r > 0 and b * (r + 1) in proto:
            return False
    for motif in avoid:
        motif = motif.upper()
        for at in range(len(proto) - len(motif) + 1):
            if all(proto[at + i] in R.IUPAC[motif[i]] for i in range(len(motif))):
                return False
    return True


def keep(sites, contigs, **flt):
    """The subsequence of brute_sites' tuples whose protospacer passes."""
    return [s for s in sites if passes(protospacer(s, contigs), **flt)]


# ---- the planted genome ----

L20 = 20


def _calm(rng, n, gc, forbid_first="", forbid_last=""):
    """n bases, `gc` of them G or C, no base twice in a row, no BsmBI site and no GGNCC; not starting / ending with the given bases."""
    for _ in range(100000):
        s = [rng.choice("GC") for _ in range(gc)] + [rng.choice("AT") for _ in range(n - gc)]
        rng.shuffle(s)
        s = "".join(s)
        if any(s[i] == s[i + 1] for i in range(n - 1)) or (s and (s[0] in forbid_first or s[-1] in forbid_last)):
            continue
        if passes(s, avoid=BSMBI + ("GGNCC",)):
            return s
    raise AssertionError("no such string")


def _cases(rng):
    """(name, protospacer as the guide reads, PAM, 5' flank base, 3' flank base, filter name, kept, at every bit offset).  The flanks are
    on the guide's strand: 5' in front of the protospacer, 3' behind the PAM."""
    out = []

    def add(name, proto, flt, kept, pam="TGG", left=None, right=None, everywhere=False):
        assert len(proto) == L20 and len(pam) == 3 and pam[1] in "AG" and pam[2] == "G"
        left = left or next(b for b in "ACGT" if b != proto[0])            # a flank that continues no run
        right = right or next(b for b in "ACGT" if b != pam[-1])
        out.append((name, proto, pam, left, right, flt, kept, everywhere))

    # GC: 40 - 60 % of 20 is 8 .. 12
    for g in (7, 8, 12, 13):
        add("gc%d" % g, _calm(rng, L20, g), "gc", 8 <= g <= 12, everywhere=True)
    add("gc0", "AT" * 10, "gc", False)
    add("gc20", "GC" * 10, "gc", False)
    # runs: a limit of 3 on every base (runs3), of R and of R + 1 bases, at the protospacer's first and at its last bases
    for b in "ACGT":
        other = "ACGT".replace(b, "")
        for n in (3, 4):
            add("run_%s%d_first" % (b, n), b * n + _calm(rng, L20 - n, 8, forbid_first=b), "runs3", n == 3, everywhere=(n == 4 and b == "A"))
            add("run_%s%d_last" % (b, n), _calm(rng, L20 - n, 8, forbid_last=b) + b * n, "runs3", n == 3, pam=other[0] + "GG",
                everywhere=(n == 4 and b == "T"))
        # R + 1 long with R of it inside: the rest in the PAM, and in the flank on the other side -- kept
        add("run_%s_into_pam" % b, _calm(rng, L20 - 3, 8, forbid_last=b) + b * 3, "runs3", True, pam=b + "GG", everywhere=(b == "T"))
        add("run_%s_into_flank" % b, b * 3 + _calm(rng, L20 - 3, 8, forbid_first=b), "runs3", True, left=b, everywhere=(b == "A"))
    # a limit on one base only, a longer run of another one present
    add("t3_with_aaaaa", "AAAAA" + _calm(rng, L20 - 5, 9, forbid_first="A"), "t3", True)
    add("t3_with_tttt", _calm(rng, 8, 4, forbid_last="T") + "TTTT" + _calm(rng, 8, 4, forbid_first="T"), "t3", False)
    add("g3_with_cccc", _calm(rng, 8, 3, forbid_last="C") + "CCCC" + _calm(rng, 8, 3, forbid_first="C"), "g3", True)
    # motifs: CGTCTC at offset 0, at offset L - 6, and one base further out on either side
    m = "CGTCTC"
    add("motif_first", m + _calm(rng, L20 - 6, 6, forbid_first="C"), "bsmbi", False, everywhere=True)
    add("motif_last", _calm(rng, L20 - 6, 6, forbid_last="C") + m, "bsmbi", False, pam="AGG", everywhere=True)
    add("motif_out_5", m[1:] + _calm(rng, L20 - 5, 6, forbid_first="C"), "bsmbi", True, left="C", everywhere=True)
    add("motif_out_3", _calm(rng, L20 - 5, 6, forbid_last="C") + m[:5], "bsmbi", True, pam="CGG", everywhere=True)
    add("motif_iupac", _calm(rng, 7, 3, forbid_last="G") + "GGACC" + _calm(rng, 8, 3, forbid_first="C"), "ggncc", False)
    add("motif_iupac_not", _calm(rng, 7, 3, forbid_last="G") + "GGAAC" + _calm(rng, 8, 3, forbid_first="C"), "ggncc", True)
    # a non-palindromic motif present only as its reverse complement: kept unless that orientation was passed as well
    add("motif_rc_only", _calm(rng, 7, 3, forbid_last="G") + "GAGACG" + _calm(rng, 7, 3, forbid_first="G"), "cgtctc_only", True)
    add("motif_rc_both", _calm(rng, 7, 3, forbid_last="G") + "GAGACG" + _calm(rng, 7, 3, forbid_first="G"), "bsmbi", False)
    return out


def _unit(case, strand):
    """What the forward text shows of a case planted on a strand, and the offset of the protospacer's leftmost forward base in it."""
    _, proto, pam, left, right, _, _, _ = case
    text = left + proto + pam + right
    return (text, 1) if strand == "+" else (R.revcomp(text), 1 + len(pam))


def filter_genome(seed=20):
    """(names, strings, planted): one contig of random bases with the cases of _cases() for N20 + nrg.  The cases marked `everywhere`
    stand once at every bit offset 0 .. 31 of a 32-base word, half of the offsets on each strand (the next case takes the strands the other
    way round), so their windows cross into the next word at every offset; the others once per strand.  One planted protospacer lies
    across base 8192 (a segment boundary of the kernel).  Behind them: a U inside a protospacer and a u on a '-' copy, in a run and
    where it decides the GC count, and the protospacers in front of AGGAGU, the U in the longer PAM nngrrt only (as in
    test_gpu_sites.py's test_u_inside_the_longer_pam_only), one that a filter rejects and one that it keeps.
    planted: [(case name, strand, protospacer_start, filter name, kept)]."""
    rng = random.Random(seed)
    cases = _cases(rng)
    parts, planted, at = [], [], 0

    def put(text):
        nonlocal at
        parts.append(text)
        at += len(text)

    def plant(case, strand, offset=None):
        text, off = _unit(case, strand)
        if offset is not None:
            put(R._rand(rng, (offset - (at + off)) % 32))
        planted.append((case[0], strand, at + off, case[5], case[6]))
        put(text)

    put(R._rand(rng, 40))
    flip = 0
    for case in cases:
        if not case[7]:
            continue
        # 25-base units one behind the other: the offsets go round in steps of 25, all 32 of them; one gap where the strand changes
        first = "+-"[flip % 2]
        flip += 1
        r0 = (at + _unit(case, first)[1]) % 32
        for u in range(32):
            plant(case, first if u < 16 else "+-"[first == "+"], offset=(r0 + 25 * u) % 32)
    for case in cases:
        if not case[7]:
            for strand in "+-":
                plant(case, strand)
                put(R._rand(rng, 3))
    # U: TTUT reads TTTT (a run of four T; '+'), TUT + ... a run of three; on '-' the forward text shows the complement: a u among T is
    # an A of the guide
    body = _calm(rng, L20 - 4, 8, forbid_first="TA")
    for name, proto, strand, flt, kept, u_at in (("u_run4", "TTTT" + body, "+", "t3", False, 2), ("u_run3", "CTTT" + body, "+", "t3", True, 2),
                                                 ("u_minus_run4", "AAAA" + body, "-", "runs3", False, 1), ("u_minus_run3", "CAAA" + body, "-", "runs3", True, 1),
                                                 ("u_gc", "T" + _calm(rng, L20 - 1, 7, forbid_first="T"), "+", "gc", False, 0),
                                                 ("u_minus_gc", "A" + _calm(rng, L20 - 1, 8, forbid_first="A"), "-", "gc", True, 0)):
        case = (name, proto, "TGG", "C", "C", flt, kept, False)
        text, off = _unit(case, strand)
        i = off + (u_at if strand == "+" else L20 - 1 - u_at)
        assert text[i] == "T"
        text = text[:i] + ("U" if strand == "+" else "u") + text[i + 1:]
        planted.append((name, strand, at + off, flt, kept))
        put(text + R._rand(rng, 3))
    # the U in the longer PAM only: <protospacer>AGGAGU on '+', ACUCCT<protospacer> on '-'
    for name, proto, kept in (("u_in_pam_gc7", _calm(rng, L20, 7), False), ("u_in_pam_gc10", _calm(rng, L20, 10), True)):
        planted.append((name, "+", at + 1, "gc", kept))
        put("C" + proto + "AGGAGU" + "C")
        planted.append((name, "-", at + 7, "gc", kept))
        put("C" + "ACUCCT" + R.revcomp(proto) + "C")
    put(R._rand(rng, 200))
    seq = "".join(parts)
    assert len(seq) <= 12000, len(seq)
    return ["chrF"], [seq], planted


def check_planted(seqs, planted, sites):
    """The planted cases are what they claim, by this referee: each is a site of N20 + nrg (`sites`: brute_sites of it), its verdict
    under its filter is the one intended, the `everywhere` cases cover the 32 bit offsets on either strand's half, and a protospacer
    straddles base 8192."""
    by_place = {(s[1], s[3]): s for s in sites}
    all_filters = dict(filters(L20), **EXTRA)
    offsets = {}
    for name, strand, p, flt, kept in planted:
        site = by_place.get((p, strand))
        assert site is not None, (name, strand, p)
        assert passes(protospacer(site, seqs), **all_filters[flt]) == kept, (name, strand, p, protospacer(site, seqs))
        offsets.setdefault(name, set()).add(p % 32)
    every = [name for name, seen in offsets.items() if len(seen) > 2]
    assert len(every) >= 12 and all(len(offsets[name]) == 32 for name in every), {n: len(offsets[n]) for n in every}
    assert any(p < 8192 < p + L20 - 1 for _, _, p, _, _ in planted)
