"""The referee of the allele-site tests (test_allele_sites_host.py, test_gpu_allele_sites.py) and the genome they run on.  The referee
builds on sites_ref.brute_sites: the reference allele's sites from the contig string as it is, the alt allele's from the string with one
letter replaced, and a record wherever the SNV lies in the footprint of either.  It shares no code with the library."""
import random

import sites_ref as R

L = 20
N20 = "N" * L
# (protospacer, [PAMs], 5' PAM)
PATTERNS = {
    "n20_nrg": (N20, ["nrg"], False),
    "tttv_n20": (N20, ["tttv"], True),
    "aux24": (N20, ["ngg", "ng", "nnaa"], False),          # aux PAMs of lengths 2 and 4 behind a PAM of 3
    "n20": (N20, [], False),                                # PAM-less
    "fixed_nrg": R.PATTERNS["fixed_nrg"],
}
NAMES = list(PATTERNS)
REACH = 63                                                  # a footprint of a start whose footprint can hold the SNV lies within this of it


def pattern_of(C, name):
    proto, pams, five = PATTERNS[name]
    first = pams[0] if pams else ""
    return C.Guide((first + proto) if five else (proto + first), pams[1:])


def _letter(c):
    return c.upper().replace("U", "T")


def _by_start(sites):
    return {(s[1], s[3]): s for s in sites}


def _guide_bits(seq, site):
    ci, p, pam_start, strand, k, pl, n = site
    text = seq[p:p + n].upper().replace("U", "T")
    if strand == "-":
        text = R.revcomp(text)
    codes = ["ACGT".index(c) for c in text]
    return sum((c & 1) << i for i, c in enumerate(codes)), sum((c >> 1) << i for i, c in enumerate(codes))


_REF_SITES = {}


def allele_sites(seqs, name, snvs, key=None):
    """(records, status) of the SNVs [(contig_index, position, ref, alt)] under PATTERNS[name]: records as tuples in the field order of
    calitas_allele_site_t, in the output's order.  key: something hashable that names seqs, to keep the reference allele's sites."""
    proto, pams, five = PATTERNS[name]
    n = len(proto)
    ref_sites = _REF_SITES.get((key, name)) if key is not None else None
    if ref_sites is None:
        ref_sites = [_by_start(R.brute_sites(seqs, proto, pams, five, chrom=ci)) for ci in range(len(seqs))]
        if key is not None:
            _REF_SITES[(key, name)] = ref_sites
    records, status = [], []
    for i, (ci, pos, ref, alt) in enumerate(snvs):
        seq = seqs[ci]
        here = _letter(seq[pos])
        if here not in "ACGT":
            status.append(2)
            continue
        if ref and _letter(ref) != here:
            status.append(1)
            continue
        if _letter(alt) == here:
            status.append(3)
            continue
        status.append(0)
        # the alt allele's sites from a cut of the string wide enough that every footprint of the 64 starts lies inside it or leaves the contig
        lo, hi = max(0, pos - REACH), min(len(seq), pos + REACH + 1)
        cut = seq[lo:pos] + _letter(alt) + seq[pos + 1:hi]
        alt_sites = {(s[1] + lo, s[3]): (ci, s[1] + lo, s[2] + lo if s[2] >= 0 else -1) + s[3:] for s in R.brute_sites([cut], proto, pams, five)}
        with_alt = seq[:pos] + _letter(alt) + seq[pos + 1:]
        for p in range(pos - 47, pos + 17):
            for strand in "+-":
                on_ref, on_alt = ref_sites[ci].get((p, strand)), alt_sites.get((p, strand))
                covered = False
                for s in (on_ref, on_alt):
                    if s is not None:
                        f0, f1 = (p, p + n) if s[2] < 0 else (min(p, s[2]), max(p + n, s[2] + s[5]))
                        covered = covered or f0 <= pos < f1
                if not covered:
                    continue
                kind = (1 if on_alt else 0) + (2 if on_ref else 0)
                site = on_alt or on_ref
                g_lo, g_hi = _guide_bits(with_alt if on_alt else seq, site)
                records.append((ci, p, site[2], strand.encode(), site[4], site[5], n, i, kind, on_ref[4] if kind == 3 else -1,
                                (p + n - 1 - pos) if strand == "-" else (pos - p), 0, g_lo, g_hi))
    return records, status


def as_records(C, records):
    import numpy as np
    return np.array(records, dtype=C.ALLELE_SITE_DTYPE) if records else np.zeros(0, dtype=C.ALLELE_SITE_DTYPE)


def snv_array(C, snvs):
    import numpy as np
    out = np.zeros(len(snvs), dtype=C.SNV_DTYPE)
    for k, (ci, pos, ref, alt) in enumerate(snvs):
        out[k] = (ci, pos, ref.encode(), alt.encode(), 0)
    return out


# ---- the genome ----

X20 = "GATTACAGCTCATCGTACCA"                                 # no G run, no CC: a protospacer that brings no PAM of its own
PLUS, PLUS_NEW, MINUS, MINUS_NEW = 200, 300, 400, 500        # X20 + TGG, X20 + TCG, CCA + rc(X20), CGA + rc(X20)
SWITCH_OUT, SWITCH_IN = 600, 650                             # aux24: X20 + TGG (ngg -> ng, the SNV past the new footprint), X20 + TGAA (ng -> nnaa)
FIXED_PLUS, FIXED_MINUS = 700, 800
N_AT, N_PAIR = 1000, (1100, 1110)
EXHAUSTIVE = 600                                             # the first bases of contig A, every position and alt


def _other(base, k=1):
    return "ACGT"[("ACGT".index(_letter(base)) + k) % 4]


def genome(seed=23):
    """(names, strings): a random contig, one with the hand-planted cases, and one of 60 bases that ends in a site."""
    rng = random.Random(seed)
    a = R._rand(rng, 900)
    b = list(R._rand(rng, 3000))
    R._put(b, PLUS, X20 + "TGG")
    R._put(b, PLUS_NEW, X20 + "TCG")
    R._put(b, MINUS, "CCA" + R.revcomp(X20))
    R._put(b, MINUS_NEW, "CGA" + R.revcomp(X20))
    R._put(b, SWITCH_OUT, X20 + "TGGT")
    R._put(b, SWITCH_IN, X20 + "TGAA")
    R._put(b, FIXED_PLUS, R.FIXED + "AGG")
    R._put(b, FIXED_MINUS, R.revcomp(R.FIXED + "TGG"))
    R._put(b, N_AT, "N")
    R._put(b, N_PAIR[0], "N")
    R._put(b, N_PAIR[1], "n")
    R._put(b, 1300, (X20 + "tgg").lower())                   # a soft-masked site
    c = R._rand(rng, 60 - 23) + X20 + "TGG"
    return ["chrA", "chrB", "chrC"], [a, "".join(b), c]


def planted_snvs(seqs, seed=5):
    """The SNVs the planted cases need, some at random over all three contigs, and repeats: not sorted.  (contig, position, ref, alt)."""
    rng = random.Random(seed)
    b, c = seqs[1], seqs[2]
    snv = lambda ci, pos, k=1, ref=None: (ci, pos, seqs[ci][pos].upper() if ref is None else ref, _other(seqs[ci][pos], k))
    out = [(1, PLUS + 22, "G", "C"), (1, PLUS_NEW + 21, "C", "G"), (1, PLUS + 20, "T", "A"), snv(1, PLUS), snv(1, PLUS + 19),
           (1, MINUS, "C", "G"), (1, MINUS_NEW + 1, "G", "C"), (1, MINUS + 2, "A", "T"), snv(1, MINUS + 3 + 19), snv(1, MINUS + 3),
           (1, SWITCH_OUT + 22, "G", "C"), (1, SWITCH_IN + 21, "G", "C")]
    for ci in (1, 2):
        n = len(seqs[ci])
        out += [snv(ci, pos) for pos in (0, n - 1, 47, 48, n - 1 - 47, n - 1 - 48) if 0 <= pos < n]
    out += [snv(1, N_AT - 1), snv(1, N_AT + 1), (1, N_AT, "", "A"),                              # beside an N, on an N
            (1, 1500, _other(b[1500]), _other(b[1500], 2)), (1, 1501, b[1501], b[1501]),          # a wrong ref, alt = the reference
            (1, 1502, "", _other(b[1502])), (1, 1503, b[1503].lower(), _other(b[1503]).lower()),  # ref not given, lower case
            (1, 1305, b[1305], _other(b[1305])),
            snv(1, (N_PAIR[0] + N_PAIR[1]) // 2), snv(1, 2000)]                                   # PAM-less: no record, 2 x 20 records
    out += [snv(1, pos, 1 + pos % 3) for pos in range(FIXED_PLUS, FIXED_PLUS + 23)] + [snv(1, pos, 1 + pos % 3) for pos in range(FIXED_MINUS, FIXED_MINUS + 23)]
    for _ in range(150):
        ci = rng.randrange(3)
        pos = rng.randrange(len(seqs[ci]))
        if seqs[ci][pos] in "ACGT":
            out.append(snv(ci, pos, rng.randrange(1, 4)))
    out += [out[0], out[3], out[-1]]                                                              # repeats
    assert len(c) == 60
    return out


def exhaustive_snvs(seqs):
    """Every position of contig A's first EXHAUSTIVE bases with each of its three other letters: position-major."""
    return [(0, pos, "", _other(seqs[0][pos], k)) for pos in range(EXHAUSTIVE) for k in (1, 2, 3)]


def u_genome(seed=31):
    """A reference with Us: inside a protospacer, in a PAM's n, beside a SNV and far from every SNV.  (names, strings, snvs)."""
    rng = random.Random(seed)
    a = list(R._rand(rng, 1200))
    R._put(a, 100, X20[:4] + "U" + X20[5:] + "TGG")
    R._put(a, 200, X20 + "uGG")
    R._put(a, 300, "CCA" + R.revcomp(X20)[:6] + "U" + R.revcomp(X20)[7:])
    a[700] = "U"
    seq = "".join(a)
    snvs = [(0, pos, "", _other(seq[pos], 1 + pos % 3)) for pos in list(range(30, 400, 3)) + [104, 220, 221, 222, 309, 700, 701, 763, 764, 636, 637, 1000, 1100]]
    snvs.append((0, 104, "T", "C"))                         # a U is a T: the ref holds
    snvs.append((0, 104, "U", "T"))                         # ... and alt T is the reference's base: status 3
    return ["chrU"], [seq], snvs


def check_planted():
    """Asserts, by the referee alone, that genome() and planted_snvs() hold what the tests rely on."""
    names, seqs = genome()
    snvs = planted_snvs(seqs)
    assert all(len(s) <= 3000 for s in seqs) and len(seqs[2]) == 60

    def recs(name):
        return allele_sites(seqs, name, snvs, key="planted")

    def of(records, snv, **want):
        fields = ("contig", "start", "pam_start", "strand", "pam_index", "pam_length", "L", "snv", "kind", "other", "offset")
        i = snvs.index(snv)
        return [r for r in records if r[7] == i and all(r[fields.index(k)] == v for k, v in want.items())]

    records, status = recs("n20_nrg")
    # each strand: a PAM created, a PAM destroyed, the PAM's n, the protospacer's first and last base
    assert of(records, snvs[1], start=PLUS_NEW, strand=b"+", kind=1, offset=L + 1)
    assert of(records, snvs[0], start=PLUS, strand=b"+", kind=2, offset=L + 2)
    assert of(records, snvs[2], start=PLUS, strand=b"+", kind=3, offset=L)
    assert of(records, snvs[3], start=PLUS, strand=b"+", kind=3, offset=0) and of(records, snvs[4], start=PLUS, strand=b"+", kind=3, offset=L - 1)
    assert of(records, snvs[6], start=MINUS_NEW + 3, strand=b"-", kind=1, offset=L + 1)
    assert of(records, snvs[5], start=MINUS + 3, strand=b"-", kind=2, offset=L + 2)
    assert of(records, snvs[7], start=MINUS + 3, strand=b"-", kind=3, offset=L)
    assert of(records, snvs[8], start=MINUS + 3, strand=b"-", kind=3, offset=0) and of(records, snvs[9], start=MINUS + 3, strand=b"-", kind=3, offset=L - 1)
    for kind in (1, 2, 3):
        assert sum(r[8] == kind for r in records) >= 20, kind
    # the contig ends, and 47 and 48 bases from them; the short contig's last site
    for ci in (1, 2):
        n = len(seqs[ci])
        for pos in (0, n - 1, 47, 48, n - 1 - 47, n - 1 - 48):
            hit = [i for i, v in enumerate(snvs) if v[0] == ci and v[1] == pos]
            assert hit and status[hit[0]] == 0, (ci, pos)
    assert any(r[0] == 2 and r[1] == 37 and r[3] == b"+" for r in records)
    # statuses: on an N, a wrong ref, alt = the reference, and the two that are examined: no ref, lower case
    by_pos = {(v[0], v[1]): status[i] for i, v in enumerate(snvs)}
    assert by_pos[(1, N_AT)] == 2 and by_pos[(1, 1500)] == 1 and by_pos[(1, 1501)] == 3 and by_pos[(1, 1502)] == 0 and by_pos[(1, 1503)] == 0
    assert any(v[2] == "" for v in snvs) and any(v[2].islower() and v[3].islower() for v in snvs)
    assert len(set(snvs)) < len(snvs) and snvs != sorted(snvs) and {v[0] for v in snvs} == {0, 1, 2}
    # a switch from PAM 0 to an aux PAM of another length: the SNV in the reference's footprint alone, and in both
    records, _ = recs("aux24")
    out = of(records, snvs[10], start=SWITCH_OUT, strand=b"+", kind=3, pam_index=1, other=0, pam_length=2)
    assert out and out[0][10] == L + 2                        # the alt footprint ends at L + 2: the SNV is past it
    assert of(records, snvs[11], start=SWITCH_IN, strand=b"+", kind=3, pam_index=2, other=1, pam_length=4, offset=L + 1)
    # PAM-less: beside an N the footprints over it are absent and the one short of it is there; none; 2 x footprint
    records, _ = recs("n20")
    at = lambda pos: snvs[[v[:2] for v in snvs].index((1, pos))]
    assert [(r[1], r[3]) for r in of(records, at(N_AT + 1))] == [(N_AT + 1, b"+"), (N_AT + 1, b"-")]
    assert [(r[1], r[3]) for r in of(records, at(N_AT - 1))] == [(N_AT - L, b"+"), (N_AT - L, b"-")]
    assert not of(records, at((N_PAIR[0] + N_PAIR[1]) // 2))
    assert len(of(records, at(2000))) == 2 * L
    records, _ = recs("fixed_nrg")
    assert {2, 3} <= {r[8] for r in records}              # a fixed protospacer: a SNV inside it destroys the site
    records, _ = recs("tttv_n20")
    assert {r[8] for r in records} == {1, 2, 3} and any(r[10] < 0 for r in records)


def vcf_records(names, seqs):
    """The records of the tools' VCF, [(chrom, pos1, id, ref, [alts])] sorted by position within a chromosome: the planted SNVs of chrB
    with their REF, two ALTs on one line, an indel and an MNV (other alleles), a REF that is not the reference's, a SNV on the N, one
    beyond chrC's end, one on a chromosome the reference lacks."""
    b = seqs[1]
    at = {}
    for ci, pos, ref, alt in planted_snvs(seqs):
        if ci == 1 and seqs[ci][pos] in "ACGT" and alt.upper() != seqs[ci][pos]:
            at.setdefault(pos, []).append(alt.upper())
    recs = [("chrB", pos + 1, "rs%d" % pos if pos % 2 else "", b[pos], sorted(set(alts))) for pos, alts in at.items()]
    recs += [("chrB", 150, "", b[149], ["".join(_other(b[149], k) for k in (1, 2))[0], _other(b[149], 3)]),     # two ALTs on one line
             ("chrB", 160, "indel", b[159:161], [b[159]]), ("chrB", 170, "", b[169], [b[169] + "A", _other(b[169])]), ("chrB", 180, "mnv", b[179:181], ["TT" if b[179:181] != "TT" else "AA"]),
             ("chrB", 190, "", _other(b[189]), [_other(b[189], 2)]),                                            # another REF than the reference
             ("chrB", N_AT + 1, "", "A", ["C"]),                                                                # on the N
             ("chrB", 2500, "out", b[2499], [_other(b[2499])]),                                                 # outside the tests' region
             ("chrC", 61, "", "A", ["C"]), ("chrC", 40, "", seqs[2][39], [_other(seqs[2][39])]), ("chrZ", 5, "", "A", ["C"]),
             ("chrA", 10, "", seqs[0][9], [_other(seqs[0][9])])]
    order = {"chrA": 0, "chrB": 1, "chrC": 2, "chrZ": 3}
    return sorted(recs, key=lambda r: (order[r[0]], r[1]))


def write_vcf(path, names, seqs):
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for chrom, pos, vid, ref, alts in vcf_records(names, seqs):
            f.write("%s\t%d\t%s\t%s\t%s\t.\tPASS\t.\n" % (chrom, pos, vid or ".", ref, ",".join(alts)))
    return path
