"""The referee of the regions listing (test_site_regions_host.py, test_gpu_site_regions.py): the class of a site by a letter-by-letter
scan of the raw interval list -- it never looks at the library's flattened tables -- and the planted genome with its intervals, placed
where the listing can go wrong: on the 8192-base boundaries between two segments of the site pass, one protospacer's reach to either
side of them, at a contig's first and last base, nested, beside a U, a segment wholly inside an interval, a segment and a contig
without any."""
import random

import sites_ref as R

SEG = 8192                      # bases per segment of the site pass = per bucket of the regions' coarse index
FOOT = 48                       # the longest footprint: the halo of the presence table
PATTERNS = dict(R.PATTERNS)
PATTERNS["n32"] = ("N" * 32, [], False)            # PAM-less, the longest protospacer: a site at every clean position on both strands
NAMES = ("n20_nrg", "tttv_n20", "n32")
# in order of priority: class 1 wins over class 2 where both cover a base; class 0 is "elsewhere"
CLASSES = ["elsewhere", "cut", "exon", "utr", "lo", "hi", "edge", "snp"]
LENGTHS = (("chrA", 41000), ("chrB", 20000), ("chrC", 9000))


def intervals():
    """(chromosome, start, end, class name) in the order a Regions object takes them: the class names appear in CLASSES' order."""
    iv = [("chrA", 30150, 30160, "cut"), ("chrA", 30100, 30200, "exon"), ("chrA", 30000, 30400, "utr")]     # nested: the smallest class wins
    iv += [("chrA", 30350, 30500, "exon")]                                                                   # overlaps the utr's end
    for chrom, b in (("chrA", SEG), ("chrB", 2 * SEG)):
        for L in (20, 32):
            # one base each, a protospacer's reach below and above a segment boundary: only a site that starts in the segment before b
            # reaches the `hi` ones at b + L - 2 (and none reaches b + L - 1 .. from there); the `lo` ones sit L and L - 1 below
            iv += [(chrom, b - L, b - L + 1, "lo"), (chrom, b - (L - 1), b - (L - 1) + 1, "lo")]
            iv += [(chrom, b + (L - 1), b + (L - 1) + 1, "hi"), (chrom, b + L, b + L + 1, "hi"), (chrom, b + L - 2, b + L - 1, "hi")]
    iv += [("chrA", SEG - 192, SEG, "edge"), ("chrB", SEG, SEG + 108, "edge")]                            # ends at 8192; starts at 8192
    iv += [("chrA", 0, 5, "edge"), ("chrA", 40999, 41000, "edge"), ("chrB", 0, 3, "cut"), ("chrB", 19990, 20000, "exon")]
    iv += [("chrA", 3 * SEG - 1, 3 * SEG, "snp"), ("chrA", 3 * SEG, 3 * SEG + 1, "snp")]                  # one base at 24575 and one at 24576
    iv += [("chrB", SEG - 1, SEG, "snp")]
    iv += [("chrA", 4 * SEG - 68, 5 * SEG + 10, "utr")]                                                   # segment 4 of chrA lies wholly inside
    iv += [("chrA", 12001, 12003, "snp")]                                                                 # beside the U at 12000
    # every small class also somewhere wide, so that a one-base extent finds it on both strands
    # (wide enough for tttv_n20, which has a site at one position in 85)
    iv += [("chrB", 500 + 800 * i, 1200 + 800 * i, name) for i, name in enumerate(["lo", "hi", "snp", "cut", "exon", "edge", "utr"])]
    # (chrA's segment 2, [16384, 24576) less the halo of 24575's snp, and all of chrC hold nothing)
    order = {n: i for i, n in enumerate(CLASSES)}
    assert sorted({x[3] for x in iv}, key=order.get) == CLASSES[1:]
    first = []
    for name in CLASSES[1:]:                             # one interval of every class up front: first appearance gives the priorities
        first.append(next(x for x in iv if x[3] == name))
    return first + [x for x in iv if x not in first]


def genome(seed=2024):
    """(names, strings): random bases; a U at chrA:12000; at the boundaries the halo intervals sit at, the PAMs that make a site of
    n20_nrg (chrA:8192) and of tttv_n20 (chrB:16384) start on the boundary's last base before it and on its first base, on both
    strands."""
    rng = random.Random(seed)
    seqs = [list(R._rand(rng, n)) for _, n in LENGTHS]
    a, b = seqs[0], seqs[1]
    a[12000] = "U"
    for p in (SEG - 1, SEG):                             # n20_nrg: '+' wants N R G behind the protospacer, '-' C Y N in front of it
        R._put(a, p + 20, "AGG")
        R._put(a, p - 3, "CCT")
    for p in (2 * SEG - 1, 2 * SEG + 4):                 # tttv_n20: '+' wants T T T V in front, '-' B A A A behind
        R._put(b, p - 4, "TTTA")
        R._put(b, p + 20, "TAAA")
    return [n for n, _ in LENGTHS], ["".join(s) for s in seqs]


def class_of(contig_name, p, strand, L, extent, iv):
    """The contract, letter by letter: the forward bases the extent covers, each held against every interval."""
    a, b = (0, L) if extent is None else extent
    assert 0 <= a < b <= L
    bases = range(p + L - b, p + L - a) if strand == "-" else range(p + a, p + b)
    best = 0
    for x in bases:
        for chrom, s, e, name in iv:
            if chrom == contig_name and s <= x < e:
                k = CLASSES.index(name)
                if best == 0 or k < best:
                    best = k
    return best


_by_base = {}


def classes_of(names, sites, extent, iv=None):
    """class_of for every site of brute_sites' list; the per-base class of the default intervals is worked out once (still from the
    raw list, base by base)."""
    if iv is not None:
        return [class_of(names[s[0]], s[1], s[3], s[6], extent, iv) for s in sites]
    if not _by_base:
        for chrom, n in LENGTHS:
            col = [0] * n
            for c, s, e, name in intervals():
                if c == chrom:
                    k = CLASSES.index(name)
                    for x in range(s, e):
                        if col[x] == 0 or k < col[x]:
                            col[x] = k
            _by_base[chrom] = col
    out = []
    for s in sites:
        L = s[6]
        a, b = (0, L) if extent is None else extent
        lo, hi = (s[1] + L - b, s[1] + L - a) if s[3] == "-" else (s[1] + a, s[1] + b)
        got = [k for k in _by_base[names[s[0]]][lo:hi] if k]
        out.append(min(got) if got else 0)
    return out


def mask_of(class_names):
    m = 0
    for n in class_names:
        m |= 1 << CLASSES.index(n)
    return m


ALL = (1 << len(CLASSES)) - 1
# every single class, elsewhere alone, all of them, a mix
MASKS = [1 << k for k in range(len(CLASSES))] + [ALL, mask_of(["exon", "snp", "hi"]), mask_of(["elsewhere", "cut", "edge"])]


def extents(L):
    out = [None, (0, 1), (L - 1, L)]
    if L >= 18:
        out.append((16, 18))
    return out


def check_cover(sites, cls, mask):
    """No comparison is empty: every class, 0 among them, has a site on each strand, so whatever the mask keeps and whatever it drops is
    there on both strands."""
    seen = {(k, s[3]) for s, k in zip(sites, cls)}
    for k in range(len(CLASSES)):
        for strand in "+-":
            assert (k, strand) in seen, "no %s site of class %s: the comparison would be empty" % (strand, CLASSES[k])
    for strand in "+-":
        assert any((mask >> k) & 1 for k, st in seen if st == strand)
        assert mask & ALL == ALL or any(not (mask >> k) & 1 for k, st in seen if st == strand)


def expected(sites, cls, mask):
    """(kept sites, their classes, the [n_classes][2] histogram)"""
    keep = [i for i, k in enumerate(cls) if (mask >> k) & 1]
    hist = [[0, 0] for _ in CLASSES]
    for i in keep:
        hist[cls[i]][int(sites[i][3] == "-")] += 1
    return [sites[i] for i in keep], [cls[i] for i in keep], hist


def pattern_of(C, name):
    proto, pams, five = PATTERNS[name]
    first = pams[0] if pams else ""
    return C.Guide((first + proto) if five else (proto + first), pams[1:])


def regions_of(C, iv=None):
    return C.Regions(iv if iv is not None else intervals())
