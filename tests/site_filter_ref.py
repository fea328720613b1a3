"""The referee of the site-filter tests (test_site_filters_host.py, test_gpu_site_filters.py): plain Python on strings that shares no
code with the library.  It takes sites_ref.brute_sites' tuples and the contig strings, cuts each protospacer out, takes an explicit
reverse complement for '-', counts G and C, searches `b * (r + 1) in proto` and holds motifs letter by letter against sites_ref.IUPAC.
filter_genome() is a contig of less than 12 kb with the cases the contract names planted for N20 + nrg on both strands.
sweep_genome(), features(), check_sweep() and sweep_sets() serve the parameter sweep: "N" * L for L = 1 .. 32, every bound at which a
verdict can change, the expected listing as a mask over the unfiltered one."""
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


# ---- the parameter sweep: every protospacer length and every bound at which a verdict can change ----
# The patterns are PAM-less ("N" * L): every position with room is a site on both strands, so every bit offset and every word boundary
# of the kernel's 32-base words is covered without planting.  A filter's expected listing is plain[mask]: a boolean mask over the
# unfiltered listing, from per-site features (G + C count, longest run per base) that string operations give once per length.

SWEEP_LENGTHS = tuple(range(1, 33))
PAM_LENGTHS = (1, 2, 3, 7, 8, 15, 16, 17, 31, 32)
PAM_PATTERNS = {"nrg": (["nrg"], False), "tttv": (["tttv"], True)}
TUPLE_LENGTHS = (5, 20, 32)                # the lengths that get every max_run tuple of {0, 1, 2, L - 1}^4
SWEEP_KINDS = ("gc", "runs", "motifs", "together", "with_pam")
SEGMENT_EDGE = 8192                        # a segment boundary of the kernel for the first contig (as in check_planted)

# 16 letters; not a palindrome, and no prefix of two letters or more is its own reverse complement (check_motif_strings)
M16 = "GACTTGCAAGCTGTCA"
_TWO = {"A": "R", "C": "Y", "G": "K", "T": "W"}            # a two-base code that contains the letter
IUPAC_LENGTHS = (3, 8, 9, 16)
# every third letter a two-base code, letter 12 an N (which takes the place of that third letter's code)
M16_IUPAC = "".join("N" if i == 11 else _TWO[c] if i % 3 == 2 else c for i, c in enumerate(M16))
# eight motifs, none a palindrome, no two each other's reverse complement: with both orientations the sixteen entries the device holds
EIGHT = ("CGTCTC", "GAAGAC", "GGTCTC", "CACCTGC", "ARYBA", "TTTTV", "GACNNNNNNNNR", "SWNNNNKNNA")
_IUPAC_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "M": "K", "R": "Y", "W": "W", "S": "S", "Y": "R", "K": "M", "V": "B", "H": "D",
               "D": "H", "B": "V", "N": "N"}


def iupac_revcomp(motif):
    return "".join(_IUPAC_COMP[c] for c in reversed(motif))


def check_motif_strings():
    assert len(M16) == 16 and set(M16) <= set("ACGT") and M16 != R.revcomp(M16)
    assert all(M16[:n] != R.revcomp(M16[:n]) for n in range(2, 17))
    assert len(M16_IUPAC) == 16 and M16_IUPAC[11] == "N" and sum(c in "RYKW" for c in M16_IUPAC) == 4
    assert all(a in R.IUPAC[b] for a, b in zip(M16, M16_IUPAC))
    both = [m for m in EIGHT] + [iupac_revcomp(m) for m in EIGHT]
    assert len(EIGHT) == 8 and len(set(both)) == 16, both


def _ramps(rng):
    """A window sliding across these takes every G + C count from 0 to its length."""
    return "AT" * 20 + "GC" * 20 + "TA" * 20 + R._rand(rng, 32)


def _separator(b, r):
    """33 bases alternating two of the three bases that are not b; which two goes round with r."""
    other = "ACGT".replace(b, "")
    return ((other[r % 3] + other[(r + 1) % 3]) * 17)[:33]


def sweep_genome(seed=32):
    """(names, strings): one contig of plain ACGT.  In this order: 64 random bases; the GC ramps; the run ladder -- for each base b and
    each r = 1 .. 32 a separator without b and without a repeat, then b * r, and a closing separator per base; 600 random bases; random
    filler up to base 8152; the ramps once more, so that GC windows of every length lie across base 8192 (SEGMENT_EDGE); 200 random bases
    with M16 planted once per strand."""
    rng = random.Random(seed)
    parts = [R._rand(rng, 64), _ramps(rng)]
    for b in "ACGT":
        for r in range(1, 33):
            parts.append(_separator(b, r) + b * r)
        parts.append(_separator(b, 33))
    parts.append(R._rand(rng, 600))
    designed = sum(len(p) for p in parts)
    assert designed == 7284, designed
    parts.append(R._rand(rng, SEGMENT_EDGE - 40 - designed))
    parts.append(_ramps(rng))
    tail = list(R._rand(rng, 200))
    R._put(tail, 40, M16)
    R._put(tail, 120, R.revcomp(M16))
    parts.append("".join(tail))
    seq = "".join(parts)
    assert set(seq) == set("ACGT") and seq[SEGMENT_EDGE - 40:SEGMENT_EDGE + 40] == "AT" * 20 + "GC" * 20 and len(seq) < 10000
    return ["chrS"], [seq]


class Features:
    """Per brute_sites tuple, in the listing's order: minus (the strand), gc (G + C of the protospacer as the guide reads) and run
    (the longest run of A, C, G, T in it), numpy arrays; protos: the protospacers themselves."""

    def __init__(self, protos, minus, gc, run):
        self.protos, self.minus, self.gc, self.run = protos, minus, gc, run


def _longest(proto, b):
    r = 0
    while b * (r + 1) in proto:
        r += 1
    return r


def features(sites, contigs):
    import numpy as np
    protos = [protospacer(s, contigs) for s in sites]
    return Features(protos, np.array([s[3] == "-" for s in sites], dtype=bool),
                    np.array([p.count("G") + p.count("C") for p in protos], dtype=np.int64),
                    np.array([[_longest(p, b) for b in "ACGT"] for p in protos], dtype=np.int64).reshape(len(protos), 4))


def mask_of(feat, L, gc_min=0, gc_max=255, max_run=(0, 0, 0, 0), avoid=(), motif_mask=None):
    """passes() over a whole listing: the GC bounds and the run limits from the features, each motif's verdicts through
    motif_mask(motif) (passes() itself, protospacer by protospacer, kept per motif)."""
    keep = (feat.gc >= gc_min) & (feat.gc <= min(gc_max, L))
    for i, r in enumerate(max_run):
        if r > 0:
            keep &= feat.run[:, i] <= r
    for motif in avoid:
        keep &= motif_mask(motif)
    return keep


def occurrences(proto, motif):
    """The offsets at which the IUPAC motif occurs in the protospacer."""
    return [at for at in range(len(proto) - len(motif) + 1) if all(proto[at + i] in R.IUPAC[motif[i]] for i in range(len(motif)))]


def motifs_of(L):
    """The single-motif cases of a length: M16's prefixes of 1 .. 16 letters that fit, and its IUPAC version's of IUPAC_LENGTHS."""
    return [M16[:n] for n in range(1, min(16, L) + 1)] + [M16_IUPAC[:n] for n in IUPAC_LENGTHS if n <= L]


_occurrences = {}


def _occurs(seq, motif):
    """Per strand, per forward position q with room: passes() rejects the stretch seq[q:q + len(motif)] as that strand's guide reads it."""
    if motif not in _occurrences:
        n = len(motif)
        stretches = [seq[q:q + n] for q in range(len(seq) - n + 1)]
        _occurrences[motif] = ([not passes(t, avoid=(motif,)) for t in stretches], [not passes(R.revcomp(t), avoid=(motif,)) for t in stretches])
    return _occurrences[motif]


class Listing:
    """The unfiltered listing of one pattern by the referee: brute_sites' tuples, their features, and the motif verdicts asked for so far."""

    def __init__(self, contigs, L, pams=(), five=False):
        self.L, self.pams, self.five = L, list(pams), five
        self.pattern = ("".join(pams[:1]) + "N" * L) if five else ("N" * L + "".join(pams[:1]))
        self.sites = R.brute_sites(contigs, "N" * L, self.pams, five)
        self.features = features(self.sites, contigs)
        self.contig = contigs[0]
        self._motifs = {}
        self.checked = False

    def motif_mask(self, motif):
        """passes(protospacer, avoid=(motif,)) per site.  passes() rejects a protospacer when one of its windows of the motif's length
        is an occurrence, and a window is a stretch of the contig that protospacers of every length share: passes() judges every such
        stretch once per strand (_occurs), a site is rejected when a stretch inside its protospacer was, and passes() on the whole
        protospacer confirms the rejected sites (a seeded 1024 of them where there are more) and a seeded sample of the kept ones."""
        import numpy as np
        if motif not in self._motifs:
            n, L = len(motif), self.L
            first = np.array([s[1] for s in self.sites], dtype=np.int64)
            keep = np.ones(len(self.sites), dtype=bool)
            for minus, occurs in enumerate(_occurs(self.contig, motif)):
                before = np.concatenate(([0], np.cumsum(occurs)))                 # occurrences that start in front of a position
                here = self.features.minus == bool(minus)
                keep[here] = before[first[here] + L - n + 1] == before[first[here]]
            protos = self.features.protos
            sample = random.Random(len(motif) * 64 + L).sample(range(len(protos)), min(64, len(protos)))
            rejected = np.flatnonzero(~keep).tolist()
            if len(rejected) > 1024:                                              # (a one- or two-letter motif rejects nearly everything)
                rejected = random.Random(L).sample(rejected, 1024)
            for i in set(rejected) | set(sample):
                assert passes(protos[i], avoid=(motif,)) == bool(keep[i]), (L, motif, self.sites[i])
            self._motifs[motif] = keep
        return self._motifs[motif]

    def mask(self, **flt):
        return mask_of(self.features, self.L, motif_mask=self.motif_mask, **flt)


_listings = {}


def listing(L, pam=None):
    """The Listing of "N" * L (pam None), "N" * L + "nrg" or "tttv" + "N" * L on sweep_genome(), made once per session."""
    if "genome" not in _listings:
        _listings["genome"] = sweep_genome()
    if (L, pam) not in _listings:
        _listings[(L, pam)] = Listing(_listings["genome"][1], L, *(PAM_PATTERNS[pam] if pam else ()))
    return _listings[(L, pam)]


def checked_listing(L, pam=None):
    """listing(), with check_sweep asserted on it when it is first asked for (the PAM-less ones: every position is a site there)."""
    ls = listing(L, pam)
    if pam is None and not ls.checked:
        check_sweep(ls.features, L, ls.motif_mask)
        ls.checked = True
    return ls


def check_sweep(feat, L, motif_mask=None):
    """What sweep_genome() is there for, on the referee alone: per strand, every G + C count 0 .. L and, per base, every longest run
    0 .. L occurs among the protospacers of length L, so every bound keeps something and rejects something; the features are passes()'
    own verdicts at a few bounds; GC windows of every count's neighbourhood lie across SEGMENT_EDGE.  With motif_mask (a Listing's):
    every single-motif case keeps and rejects a protospacer per strand, and for motifs of eight letters and more one rejected
    protospacer has its only occurrence at offset 0 and one at offset L - len, the two ends of the occurrence window."""
    import numpy as np
    assert len(feat.protos) == len(feat.gc) == len(feat.run) == len(feat.minus) > 0 and all(len(p) == L for p in feat.protos[:50])
    for minus in (False, True):
        here = feat.minus == minus
        assert set(feat.gc[here].tolist()) == set(range(L + 1)), (L, minus, "gc", sorted(set(range(L + 1)) - set(feat.gc[here].tolist())))
        for i, b in enumerate("ACGT"):
            seen = set(feat.run[here, i].tolist())
            assert seen == set(range(L + 1)), (L, minus, b, sorted(set(range(L + 1)) - seen))
    for flt in (dict(gc_min=(L + 1) // 2), dict(gc_max=L // 2), dict(max_run=(1, 0, 2, 0)), dict(max_run=(0, L - 1, 0, 1)), dict(max_run=(L, 200, 1, 255))):
        assert mask_of(feat, L, **flt).tolist() == [passes(p, **flt) for p in feat.protos], (L, flt)
    if motif_mask is None:
        return
    for motif in motifs_of(L):
        keep = motif_mask(motif)
        n = len(motif)
        for minus in (False, True):
            here = feat.minus == minus
            assert 0 < int(keep[here].sum()) < int(here.sum()), (L, motif, minus)
        if n >= 8:
            where = [occurrences(feat.protos[i], motif) for i in np.flatnonzero(~keep)]
            assert all(where), (L, motif)
            assert [0] in where and [L - n] in where, (L, motif)


# The parameter sets: lists of keyword arguments of passes() / mask_of() and of calitas_amd.SiteFilter alike, in an order in which an
# open filter follows a closed one and a closed one an open one (nothing may stick between calls).

def gc_sets(L, bounds=None):
    g = sorted(set(range(L + 1)) if bounds is None else {b for b in bounds if 0 <= b <= L})
    return ([dict(gc_min=x) for x in g if x >= 1] + [dict(gc_min=0, gc_max=255)] + [dict(gc_max=x) for x in g if x < L] +
            [dict(gc_min=0, gc_max=L)] + [dict(gc_min=x, gc_max=x) for x in g])


def run_sets(L, bounds=None, tuples=None):
    r = sorted(set(range(1, L)) if bounds is None else {b for b in bounds if 1 <= b < L})
    out = []
    for i, everything in enumerate((L, 200, 255, None)):
        if everything is not None:
            out.append(dict(max_run=(everything,) * 4))                       # no limit: the plain listing
        out += [dict(max_run=tuple(x if j == i else 0 for j in range(4))) for x in r]                     # base i alone
    out += [dict(max_run=(x,) * 4) for x in r]
    if L in TUPLE_LENGTHS if tuples is None else tuples:
        values = (0, 1, 2, L - 1)
        out += [dict(max_run=(a, b, c, d)) for a in values for b in values for c in values for d in values]
    return out


def motif_sets(L):
    out = [dict(avoid=(m,)) for m in motifs_of(L)]
    if L in (20, 32):
        out.append(dict(avoid=EIGHT))
    return out


def together_sets(L):
    rng = random.Random(1000 + L)
    out = []
    for _ in range(20):
        lo = rng.randrange(L + 1)
        hi = rng.choice(list(range(lo, L + 1)) + [255])
        out.append(dict(gc_min=lo, gc_max=hi, max_run=tuple(rng.randrange(L + 1) for _ in range(4)),
                        avoid=tuple(rng.sample(motifs_of(L), min(rng.choice((1, 2)), len(motifs_of(L)))))))
    return out


def sweep_sets(kind):
    """[(L, pam or None, filter)] of a kind of SWEEP_KINDS."""
    if kind == "with_pam":
        out = []
        for L in PAM_LENGTHS:
            bounds = (0, 1, L // 2, L - 1, L)
            for pam in PAM_PATTERNS:
                out += [(L, pam, flt) for flt in gc_sets(L, bounds) + run_sets(L, bounds, tuples=False)]
        return out
    make = {"gc": gc_sets, "runs": run_sets, "motifs": motif_sets, "together": together_sets}[kind]
    return [(L, None, flt) for L in SWEEP_LENGTHS for flt in make(L)]


def first_difference(got, want):
    """Where two listings part, for an assertion's message."""
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    return "record %d of %d / %d: got %s, want %s" % (at, len(got), len(want), got[at] if at < len(got) else None, want[at] if at < len(want) else None)
