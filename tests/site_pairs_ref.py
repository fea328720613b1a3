"""The referee of the site pairs (test_site_pairs_host.py, test_gpu_site_pairs.py): calitas_amd.site_pairs_of -- the contract as a plain
double loop -- over sites_ref.brute_sites, and the planted genome.  The double loop runs once per pattern and cut offset, with every
orientation and the widest bounds of the grid; a cell of the grid is that list cut down by the two conditions of the contract, which
keeps its order.

The genome, three contigs:
  chrA  a random stretch; a dense stretch of 1.5 kb made of runs of C and runs of G, 2 to 12 long, so that N20nrg has a '+' site
        wherever two Gs stand 21 bases ahead and a '-' site wherever two Cs stand 3 bases behind -- most positions, many on both strands;
        a stretch of As, where no pattern of the grid has a site, with N20nrg sites planted at hand-chosen spacings ("TGG" makes one '+'
        site, "TGGG" two at neighbouring starts, "CCA" one '-' site); a second random stretch.  The random stretches are poor in G and C,
        which keeps the double loop quick.
  chrB  random; ends in a '+' site.
  chrC  starts with a '+' site; random."""
import random

import sites_ref as R

PATTERNS = {"n20_nrg": R.PATTERNS["n20_nrg"], "tttv_n20": R.PATTERNS["tttv_n20"]}
NAMES = ("n20_nrg", "tttv_n20")
L = 20
BOUNDS = [(0, 0), (0, 40), (30, 150), (1000, 3000)]            # (1000, 3000): min_distance > |L - 2c|, the bisection
WIDEST = 3001
CUTS = (0, L - 3, L)
MASKS = tuple(range(1, 16))
DENSE = (300, 1800)                                           # chrA's dense stretch
PLANTED = (1800, 2500)                                        # chrA's stretch of As
LENGTHS = (("chrA", 3500), ("chrB", 1300), ("chrC", 900))
# '+' sites of N20nrg planted in the stretch of As, as starts relative to PLANTED[0] + 10; a pair of neighbours is one "TGGG"
_PLUS = (0, 29, 30, 150, 151, 300, 340, 341)
_MINUS = (420, 434, 500)                                      # '-' sites: 434 - 420 = 14 = the distance of the two cuts at one start (c = 17)


def _lean(rng, n):
    return "".join(rng.choice("AAATTTCG") for _ in range(n))


def genome(seed=11):
    """(names, strings)"""
    rng = random.Random(seed)
    a = list(_lean(rng, LENGTHS[0][1]))
    at = DENSE[0]
    letter = "C"
    while at < DENSE[1]:
        k = min(rng.randrange(2, 13), DENSE[1] - at)
        R._put(a, at, letter * k)
        at += k
        letter = "G" if letter == "C" else "C"
    R._put(a, PLANTED[0], "A" * (PLANTED[1] - PLANTED[0]))
    base = PLANTED[0] + 10
    done = set()
    for p in _PLUS:
        if p in done:
            continue
        pair = p + 1 in _PLUS
        R._put(a, base + p + L, "TGGG" if pair else "TGG")
        done.update((p, p + 1) if pair else (p,))
    for p in _MINUS:
        R._put(a, base + p - 3, "CCA")
    # a '+' and a '-' site at one start: two Gs 21 ahead, two Cs 3 behind
    R._put(a, base + 600 - 3, "CCA")
    R._put(a, base + 600 + L, "TGG")
    # sites exactly 1000, 3000 and 3001 apart, whatever is between them
    R._put(a, 40 + L, "TGGA")
    R._put(a, 3040 + L, "TGGGA")
    R._put(a, 1040 + L, "TGGA")
    b = list(_lean(rng, LENGTHS[1][1]))
    R._put(b, L, "TGG")                                          # a site on chrB's first base: where chrC's first is, by coordinates alone
    R._put(b, len(b) - 3, "TGG")                                 # ends in a site
    c = list(_lean(rng, LENGTHS[2][1]))
    R._put(c, L, "TGG")                                          # starts with one
    return [n for n, _ in LENGTHS], ["".join(s) for s in (a, b, c)]


def u_genome():
    """Sites with a U in the protospacer, a U in the PAM's N, and a U where the pattern wants a G -- beside ordinary sites, at pairing
    distance of each other."""
    a = list("A" * 600)
    for at, text in ((100, "AGG"), (130, "AGG"), (160, "UGG"), (200, "AGG"), (300, "CCA"), (330, "CCU"), (400, "AGU")):
        R._put(a, at, text)
    a[90], a[310], a[150] = "U", "u", "U"
    return ["chrU"], ["".join(a)]


def pattern_of(C, name):
    proto, pams, five = PATTERNS[name]
    first = pams[0] if pams else ""
    return C.Guide((first + proto) if five else (proto + first), pams[1:])


def codes_of(mask):
    return [code for o, code in enumerate(("++", "-+", "+-", "--")) if (mask >> o) & 1]


_sites, _wide = {}, {}


def sites_of(name, seqs, **region):
    """brute_sites of the planted genome (or of `seqs`), once per pattern and region."""
    key = (name, tuple(seqs), tuple(sorted(region.items())))
    if key not in _sites:
        _sites[key] = R.brute_sites(seqs, *PATTERNS[name], **region)
    return _sites[key]


def wide_pairs(C, name, seqs, cut, **region):
    """(sites, pairs): site_pairs_of at every orientation and 0 .. WIDEST, as an (n, 4) array of left, right, distance, orientation."""
    import numpy as np
    key = (name, tuple(seqs), cut, tuple(sorted(region.items())))
    if key not in _wide:
        sites = sites_of(name, seqs, **region)
        triples = [(s[0], s[1], s[3]) for s in sites]
        pairs = C.site_pairs_of(triples, C.SitePairs(0, WIDEST, cut_offset=cut, orientations="++,-+,+-,--"), pattern_of(C, name))
        _wide[key] = np.array(pairs, dtype=np.int64).reshape(len(pairs), 4)
    return sites_of(name, seqs, **region), _wide[key]


def cell(wide, lo, hi, mask):
    """The pairs of one cell of the grid: the wide list's rows with lo <= distance <= hi and the orientation's bit in mask, in order."""
    assert hi <= WIDEST
    keep = (wide[:, 2] >= lo) & (wide[:, 2] <= hi) & (((mask >> wide[:, 3]) & 1) == 1)
    return wide[keep]


def as_rows(pairs):
    """A find_site_pairs array in the referee's form."""
    import numpy as np
    out = np.zeros((len(pairs), 4), dtype=np.int64)
    for k, f in enumerate(("left", "right", "distance", "orientation")):
        out[:, k] = pairs[f]
    assert not pairs["reserved"].any()
    return out


def check_planted(C):
    """What the genome was planted for, by the referee alone, over the grid of N20nrg."""
    import numpy as np
    names, seqs = genome()
    found = set()
    for cut in CUTS:
        sites, wide = wide_pairs(C, "n20_nrg", seqs, cut)
        contig = np.array([s[0] for s in sites])
        start = np.array([s[1] for s in sites])
        cuts = np.array([s[1] + (L - cut if s[3] == "-" else cut) for s in sites])
        all_d = set(wide[:, 2].tolist())
        last_of = [i for i in range(len(sites) - 1) if contig[i] != contig[i + 1]]     # the last site of a contig, before the next one's first
        for lo, hi in BOUNDS:
            got = cell(wide, lo, hi, 15)
            left, right = got[:, 0], got[:, 1]
            d = set(got[:, 2].tolist())
            found.update(("orientation", o) for o in set(got[:, 3].tolist()))
            if lo in d:
                found.add(("at min", lo, hi))
            if hi in d:
                found.add(("at max", lo, hi))
            if lo > 0 and lo - 1 in all_d and lo - 1 not in d:
                found.add(("below min", lo, hi))
            if hi + 1 in all_d and hi + 1 not in d:
                found.add(("above max", lo, hi))
            if 0 in d:
                found.add("distance 0")
            if (right < left).any():
                found.add("the lower index is the right member")
            if ((start[left] == start[right]) & (np.abs(left - right) == 1)).any():
                found.add("two records at one start")
            for i in (63, 255):
                if (((left == i) & (right == i + 1)) | ((left == i + 1) & (right == i))).any():
                    found.add(("indices", i))
            # a site of one contig and the first of the next: a pair by coordinates alone, and absent
            assert (contig[left] == contig[right]).all()
            for i in last_of:
                apart = np.abs(cuts[i + 1] - cuts[:i + 1][contig[:i + 1] == contig[i]])
                if ((apart >= lo) & (apart <= hi)).any():
                    found.add(("across contigs", lo, hi))
    want = {("orientation", o) for o in range(4)} | {"distance 0", "the lower index is the right member", "two records at one start",
                                                     ("indices", 63), ("indices", 255)}
    for lo, hi in BOUNDS:
        want |= {("at min", lo, hi), ("at max", lo, hi), ("above max", lo, hi), ("across contigs", lo, hi)}
        if lo > 0:
            want.add(("below min", lo, hi))
    missing = want - found
    assert not missing, "the planted genome lacks: %s" % sorted(map(str, missing))
