"""The referee of the guide-site tests (test_sites_host.py, test_gpu_sites.py): a brute-force enumeration that shares no code with the
library -- every contig string, every position, both strands, every PAM, letter by letter against explicit IUPAC sets, with an explicit
reverse complement -- and the genomes those tests run on."""
import random

IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "M": "AC", "R": "AG", "W": "AT", "S": "CG", "Y": "CT", "K": "GT", "V": "ACG",
         "H": "ACT", "D": "AGT", "B": "CGT", "N": "ACGT"}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}

FIXED = "GACGTTACCGGATCAAGTCC"
N20 = "N" * 20
# (protospacer, [PAMs], 5' PAM)
PATTERNS = {
    "n20_nrg": (N20, ["nrg"], False),
    "tttv_n20": (N20, ["tttv"], True),
    "n21": ("N" * 21, [], False),
    "fixed_nrg": (FIXED, ["nrg"], False),
    "n20_nngrrt_nrg": (N20, ["nngrrt", "nrg"], False),
    "max48": ("NNNNNNNNRNNNNNNNNNNNNNNNYNNNNNNN", ["nnnnnnnnnnnnnngg"], False),
    # eight PAMs: all three bit-planes of the winning PAM's index; the footprint goes 27, 24, 27, 26, 24, 26, 23, 24, so the run-length
    # mask is rebuilt before every PAM but the first, in both directions
    "eight_pams": (N20, ["nnagaaw", "ngcg", "nnngatt", "nngrrt", "ngaa", "nnnrrt", "nrg", "nrrh"], False),
    # the same on the 5' side, with a 16-nt PAM (lo = -16) and a 1-nt PAM among them
    "five_prime_eight": (N20, ["tttv", "tycv", "ttnnnnnnnnnnnnnv", "ctn", "nngrrtnn", "gn", "gnnnnnc", "a"], True),
    "five16_L32": ("NNNNNNNNRNNNNNNNNNNNNNNNYNNNNNNN", ["ttnnnnnnnnnnnnnv"], True),     # lo = -16 and a footprint of 48
    # footprints at the corners of the run-length doubling: 1 (no step), 33 (last step by 1), 47 (last step by 15)
    "one_letter": ("A", [], False),
    "foot33": ("N" * 30, ["ngg"], False),
    "foot47": ("N" * 31, ["nnnnnnnnnnnnnngg"], False),
}


def pattern_string(name):
    proto, pams, five = PATTERNS[name]
    first = pams[0] if pams else ""
    return (first + proto) if five else (proto + first), pams[1:]


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


def brute_sites(contigs, proto, pams, five, chrom=None, start=0, end=None):
    """[(contig_index, protospacer_start, pam_start, strand, pam_index, pam_length, protospacer_length)] in the output's order."""
    out, L = [], len(proto)
    clean = set("ACGTUacgtu")
    # per PAM: the letters to hold the text against, as (offset, set); an N holds for every base of a clean footprint
    letters = []
    for pam in pams or [""]:
        want = ((pam + proto) if five else (proto + pam)).upper()
        letters.append([(i, IUPAC[c]) for i, c in enumerate(want) if c != "N"])
    for ci, seq in enumerate(contigs):
        if chrom is not None and ci != chrom:
            continue
        if seq is None:
            raise ValueError("absent contig")
        r0, r1 = min(start, len(seq)), (len(seq) if not end else min(end, len(seq)))
        for p in range(len(seq)):
            for strand in "+-":
                for k, pam in enumerate(pams or [""]):
                    pl = len(pam)
                    pam_left = five != (strand == "-")
                    lo = p - pl if pam_left else p
                    hi = lo + L + pl
                    if lo < r0 or hi > r1:
                        continue
                    foot = seq[lo:hi]
                    if not clean.issuperset(foot):
                        continue
                    text = foot.upper().replace("U", "T")
                    if strand == "-":
                        text = revcomp(text)
                    if all(text[i] in allowed for i, allowed in letters[k]):
                        pam_start = -1 if not pams else (p - pl if pam_left else p + L)
                        out.append((ci, p, pam_start, strand, k if pams else -1, pl, L))
                        break
    return out


def as_tuples(sites):
    """A find_sites array in brute_sites' form."""
    return [(int(s["contig_index"]), int(s["protospacer_start"]), int(s["pam_start"]), s["strand"].decode(), int(s["pam_index"]),
             int(s["pam_length"]), int(s["protospacer_length"])) for s in sites]


def as_records(sites, dtype):
    """brute_sites' tuples as a find_sites array (for a comparison of bytes, where as_tuples of the records would take seconds)."""
    import numpy as np
    out = np.zeros(len(sites), dtype=dtype)
    if sites:
        cols = list(zip(*sites))
        for field, col in zip(("contig_index", "protospacer_start", "pam_start", None, "pam_index", "pam_length", "protospacer_length"), cols):
            if field:
                out[field] = np.array(col)
        out["strand"] = np.array([s.encode() for s in cols[3]], dtype="S1")
    return out


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _put(seq, at, what):
    assert 0 <= at and at + len(what) <= len(seq)
    seq[at:at + len(what)] = list(what)


def host_genome(seed=7):
    """Small contigs with every case the semantics names: a FIXED + nrg site on the first base and one ending on the last, copies on
    both strands, upper- and lower-case N runs, a reference R inside an otherwise matching footprint, soft-masked copies, U, contigs
    of 26 and 12 bases.  Returns (names, strings)."""
    rng = random.Random(seed)
    site, rc = FIXED + "AGG", revcomp(FIXED + "TGG")
    a = list(_rand(rng, 3000))
    _put(a, 0, site)                                    # starts on the first base
    _put(a, len(a) - 23, site)                          # ends on the last base
    _put(a, 200, rc)                                    # '-' copy
    _put(a, 300, site.lower())                          # soft-masked: found
    _put(a, 400, site[:7] + "R" + site[8:])             # an R of the reference inside: not a site
    _put(a, 500, site[:4] + "U" + site[5:])             # FIXED[4] is T: a U there is a plain base
    _put(a, 560, rc[:8] + "u" + rc[9:])                 # ... and a lower-case one on the '-' copy
    _put(a, 700, "N" * 40 + site + "n" * 37)            # abuts an N run on either side
    _put(a, 900, "N" * 5 + rc + "N")
    _put(a, 1000, FIXED + "AGGGGT")                     # nngrrt and nrg both match here
    _put(a, 1500, "n" * 300)
    _put(a, 2000, "TTTA" + _rand(rng, 20))              # a 5' tttv site
    _put(a, 2100, revcomp("TTTC" + _rand(rng, 20)))
    assert site[4] == "T" and rc[8] == "T"
    b = list(_rand(rng, 777))
    _put(b, 0, rc)
    _put(b, len(b) - 23, rc)
    _put(b, 100, "RYKM")
    c26 = list(FIXED + "CGGTAC")                        # 26 bases: one 23-base footprint fits, a 26-base one exactly, a 48-base one does not
    c12 = list("ACGTACGTAGGA")
    d = list(_rand(rng, 1200))
    _put(d, 64 - 10, site)                              # straddles a 32-base word boundary
    _put(d, 600, "N" * 200)
    return ["chrA", "chrB", "c26", "c12", "chrD"], ["".join(x) for x in (a, b, c26, c12, d)]


def many_contigs(seed, n):
    """n contigs of random bases, every ninth 2500 to 20000 bases long (one to three segments of 8192 bases with sites in them; every
    other one of these at most 5000, to keep the brute force quick), the others 90 to 250: with one scan tile per contig, a launch of
    about 16 n segments most of which count nothing.
    Returns (names, strings)."""
    rng = random.Random(seed)
    seqs = [_rand(rng, (rng.randrange(2500, 20001) if i % 18 == 4 else rng.randrange(2500, 5001)) if i % 9 == 4 else rng.randrange(90, 251))
            for i in range(n)]
    return ["m%d" % i for i in range(n)], seqs


def gpu_genome(seed, tile, chunk):
    """Contigs of <= 60 kb built to hit the kernel's seams, for a scan tile of `tile` bases and a lane chunk of `chunk` bases: FIXED + nrg
    footprints straddling a 32-base word boundary at every offset 1 .. 47 (the 23-base footprint at 1 .. 22 on both strands, a 48-base
    pattern's at the rest through the N-patterns), sites across a lane-chunk, a workgroup (8192 bases) and a scan-tile boundary on both
    strands, a site that abuts an N run on either side, an N run longer than a tile plus its halos (a dead tile), and the 26- and
    12-base contigs.  Returns (names, strings)."""
    rng = random.Random(seed)
    site, rc = FIXED + "TGG", revcomp(FIXED + "AGG")
    n_a = min(60000, max(3 * tile + 5000, 30000))
    a = list(_rand(rng, n_a))
    for off in range(1, 48):                            # footprint starts `off` bases before a word boundary (23 bases: 1 .. 22 straddle)
        _put(a, 64 * (off + 2) - off, site if off % 2 else rc)
    for off in range(1, 23):
        _put(a, 4000 + 64 * off - off, rc if off % 2 else site)
    for edge in ((6000 // chunk + 1) * chunk, 8192, tile if tile + 400 < n_a else 16384):     # lane chunk, workgroup, scan tile
        _put(a, edge - 11, site)
        _put(a, edge + 64 - 7, rc)
        _put(a, edge + 128 - 22, site)                  # ends exactly on the boundary ...
        _put(a, edge + 256, rc)                         # ... and starts exactly on it (edge is a multiple of 64)
    _put(a, 12000, "N" * 50 + site + "N" * 50)
    _put(a, 12300, "n" * 33 + rc + "n")
    _put(a, 13000, site[:11] + "R" + site[12:])
    _put(a, 13100, site[:4] + "U" + site[5:])
    _put(a, 0, site)
    _put(a, n_a - 23, rc)
    # a dead tile: N over a whole tile and both of its halo chunks, inside a contig
    n_b = min(60000, 2 * tile + 4 * chunk + 3000)
    b = list(_rand(rng, n_b))
    if tile + 2 * chunk + 400 < n_b:
        lo = 300
        _put(b, lo, "N" * (n_b - 700))                  # (covers at least one whole tile plus halos when the contig spans two tiles)
        _put(b, lo - 23, site)
        _put(b, n_b - 400, rc)
    c26 = list(FIXED + "CGGTAC")
    c12 = list("ACGTACGTAGGA")
    return ["chrA", "chrB", "c26", "c12"], ["".join(x) for x in (a, b, c26, c12)]
