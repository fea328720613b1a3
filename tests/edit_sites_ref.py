"""The referee of the edit-site tests (test_edit_sites_host.py, test_gpu_edit_sites.py) and the genome they run on.  The referee builds
on sites_ref.brute_sites over the background string -- the contig with the background allele's letter at the SNV -- and reads guides,
5' neighbours and editable bases off that string.  It shares no code with the library.

The genome is allele_sites_ref.genome() (chrA, chrB, chrC) and two contigs of its own: chrH, with a homopolymer of 128 A's between
random flanks and the plants the FIXED pattern, the N and the contig's ends need, and chrG, 80 bases.  chrB alone cannot give what
check_planted() asks of fixed_nrg: its two FIXED sites hold one C in positions 3 .. 7, so installing C->T finds one record per strand
there, and correcting finds none (a background that differs from FIXED is no site).  chrH therefore holds two more FIXED sites per
strand, and two per strand of FIXED with the C of position 7 written as T, which only the corrected allele turns into a site."""
import random

import allele_sites_ref as A
import sites_ref as R

L = A.L
PATTERNS, NAMES, pattern_of, u_genome = A.PATTERNS, A.NAMES, A.pattern_of, A.u_genome
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}

# an editor: (from, to, (window_from, window_to), context, correct, max_bystanders or None)
FIXED_T = R.FIXED[:7] + "T" + R.FIXED[8:]
H_FIXED_PLUS, H_FIXED_MINUS, H_FT_PLUS, H_FT_MINUS = (100, 150), (200, 250), (300, 350), (400, 450)
H_CNT, H_GNA = 520, 540                                      # an N between a C and a T, and between a G and an A
H_RUN, H_RUN_LEN = 600, 128                                  # the homopolymer


def editors(n=L):
    """The grid of the tests for a protospacer of n bases, without the mode: C->T 3:8, A->G 3:7, C->T over the whole protospacer after
    a T, C->G in the last position after an H."""
    return [("C", "T", (3, 8), "N"), ("A", "G", (3, 7), "N"), ("C", "T", (0, n), "T"), ("C", "G", (n - 1, n), "H")]


def edit_of(C, e):
    return C.BaseEdit(e[0], e[1], e[2], e[3], e[4], e[5])


def _letter(c):
    return c.upper().replace("U", "T")


def genome(seed=41):
    """(names, strings): allele_sites_ref.genome() and behind it chrH and chrG."""
    names, seqs = A.genome()
    rng = random.Random(seed)
    h = list(R._rand(rng, H_RUN + H_RUN_LEN + 300))
    for at in H_FIXED_PLUS:
        R._put(h, at, R.FIXED + "AGG")
    for at in H_FIXED_MINUS:
        R._put(h, at, R.revcomp(R.FIXED + "TGG"))
    for at in H_FT_PLUS:
        R._put(h, at, FIXED_T + "AGG")
    for at in H_FT_MINUS:
        R._put(h, at, R.revcomp(FIXED_T + "TGG"))
    R._put(h, H_CNT, "CNT")
    R._put(h, H_GNA, "GNA")
    R._put(h, H_RUN - 1, "C" + "A" * H_RUN_LEN + "C")
    h[0], h[-1] = "C", "A"                                   # installing C->T on '+' at the first base, correcting on '-' at the last
    g = list(R._rand(rng, 80))
    g[0], g[-1] = "T", "G"                                   # ... correcting on '+' at the first base, installing on '-' at the last
    return names + ["chrH", "chrG"], seqs + ["".join(h), "".join(g)]


def editor_targets(seqs, edit, contig, lo, hi):
    """At every position of [lo, hi) of the contig the SNV that the editor makes there on whichever strand fits, if one does:
    (contig, position, "", alt)."""
    f, t, correct = edit[0], edit[1], edit[4]
    seen, made = (t, f) if correct else (f, t)               # the reference's letter and the SNV's alt, on '+'
    for pos in range(max(0, lo), min(hi, len(seqs[contig]))):
        x = _letter(seqs[contig][pos])
        if x == seen:
            yield (contig, pos, "", made)
        elif x == _COMP[seen]:
            yield (contig, pos, "", _COMP[made])


def targets(seqs, edit):
    """The SNVs of the main tests under an editor: the exhaustive 1 800 of chrA, the allele tests' planted ones (not sorted, repeats,
    every status but 4 and 5), and the editor's own targets around chrB's ends, FIXED sites and N, over chrC, chrH and chrG."""
    out = A.exhaustive_snvs(seqs) + A.planted_snvs(seqs)
    n = len(seqs[1])
    for lo, hi in ((0, 100), (A.FIXED_PLUS - 30, A.FIXED_MINUS + 60), (A.N_AT - 30, A.N_AT + 31), (n - 100, n)):
        out += list(editor_targets(seqs, edit, 1, lo, hi))
    for ci in (2, 3, 4):
        out += list(editor_targets(seqs, edit, ci, 0, len(seqs[ci])))
    return out


_REF_SITES = {}


def edit_sites(seqs, name, edit, snvs, key=None):
    """(records, status) of the SNVs [(contig_index, position, ref, alt)] under PATTERNS[name] and the editor: records as tuples in
    the field order of calitas_edit_site_t, in the output's order.  key: something hashable that names seqs, to keep the sites of the
    contigs as they are (the background when installing)."""
    proto, pams, five = PATTERNS[name]
    n = len(proto)
    f, t, (w0, w1), context, correct, most = edit
    allowed = None if context.upper() == "N" else R.IUPAC[context.upper()]
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
        b, p_ = (_letter(alt), here) if correct else (here, _letter(alt))
        if (b, p_) == (f, t):
            strand = "+"
        elif (_COMP[b], _COMP[p_]) == (f, t):
            strand = "-"
        else:
            status.append(4)
            continue
        back = seq if not correct else seq[:pos] + b + seq[pos + 1:]

        def before(p, j):
            """The letter 5' of guide position j of the protospacer at p, or "" where there is none."""
            x = p + j - 1 if strand == "+" else p + n - 1 - j + 1
            if not 0 <= x < len(back) or _letter(back[x]) not in "ACGT":
                return ""
            return _letter(back[x]) if strand == "+" else _COMP[_letter(back[x])]

        o_first = pos if strand == "+" else pos - (n - 1)    # the start that has the target at guide position 0
        if allowed is not None and (before(o_first, 0) == "" or before(o_first, 0) not in allowed):
            status.append(5)
            continue
        status.append(0)
        starts = range(pos - w1 + 1, pos - w0 + 1) if strand == "+" else range(pos - n + 1 + w0, pos - n + w1 + 1)
        if not correct and key is not None:
            if (key, name, ci) not in _REF_SITES:
                _REF_SITES[(key, name, ci)] = {(s[1], s[3]): s for s in R.brute_sites(seqs, proto, pams, five, chrom=ci)}
            sites = _REF_SITES[(key, name, ci)]
        else:
            # a cut of the background that holds every footprint of these starts, or ends where the contig does
            lo, hi = max(0, starts[0] - 16), min(len(back), starts[-1] + 48)
            sites = {(s[1] + lo, s[3]): (ci, s[1] + lo, s[2] + lo if s[2] >= 0 else -1) + s[3:] for s in R.brute_sites([back[lo:hi]], proto, pams, five)}
        for p in starts:
            site = sites.get((p, strand))
            if site is None:
                continue
            guide = back[p:p + n].upper().replace("U", "T")
            if strand == "-":
                guide = R.revcomp(guide)
            editable = [j for j in range(w0, w1) if guide[j] == f and (allowed is None or (before(p, j) != "" and before(p, j) in allowed))]
            o = pos - p if strand == "+" else p + n - 1 - pos
            assert w0 <= o < w1 and o in editable
            if most is not None and len(editable) - 1 > most:
                continue
            codes = ["ACGT".index(c) for c in guide]
            records.append((ci, p, site[2], strand.encode(), site[4], site[5], n, i, sum(1 << j for j in editable),
                            sum((c & 1) << j for j, c in enumerate(codes)), sum((c >> 1) << j for j, c in enumerate(codes))))
    return records, status


_RESULTS = {}


def referee(C, seqs, name, edit, snvs=None):
    """(records as an array, status as an array, the SNVs) of edit_sites over targets(seqs, edit), or over snvs: made once per process
    for the main genome."""
    import numpy as np
    k = (name, edit, None if snvs is None else tuple(snvs))
    if k not in _RESULTS:
        used = targets(seqs, edit) if snvs is None else snvs
        records, status = edit_sites(seqs, name, edit, used, key="genome")
        _RESULTS[k] = (as_records(C, records), np.array(status, dtype=np.uint8), used)
    return _RESULTS[k]


def as_records(C, records):
    import numpy as np
    return np.array(records, dtype=C.EDIT_SITE_DTYPE) if records else np.zeros(0, dtype=C.EDIT_SITE_DTYPE)


snv_array = A.snv_array


def bystanders_of(record):
    """The bystanders of a referee's record."""
    return bin(record[8]).count("1") - 1


def homopolymer_targets(seqs, n):
    """The A->G targets inside chrH's homopolymer at which every start of a window over a whole protospacer of n bases lies in it."""
    return [(3, pos, "", "G") for pos in range(H_RUN + n - 1, H_RUN + H_RUN_LEN - n + 1)]


def vcf_records(names, seqs, edit):
    """The records of the tools' VCF: allele_sites_ref.vcf_records (other alleles, a wrong REF, a SNV on the N, a chromosome the
    reference lacks) and the editor's own targets on chrB where those leave the position free, sorted as a VCF is."""
    recs = A.vcf_records(names[:3], seqs[:3])
    taken = {(r[0], r[1]) for r in recs}
    for ci, pos, _, alt in editor_targets(seqs, edit, 1, 0, len(seqs[1])):
        if ("chrB", pos + 1) not in taken:
            recs.append(("chrB", pos + 1, "t%d" % pos if pos % 3 else "", seqs[1][pos].upper(), [alt]))
    order = {"chrA": 0, "chrB": 1, "chrC": 2, "chrZ": 3}
    return sorted(recs, key=lambda r: (order[r[0]], r[1]))


def write_vcf(path, names, seqs, edit):
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for chrom, pos, vid, ref, alts in vcf_records(names, seqs, edit):
            f.write("%s\t%d\t%s\t%s\t%s\t.\tPASS\t.\n" % (chrom, pos, vid or ".", ref, ",".join(alts)))
    return path


def check_planted():
    """Asserts, by the referee alone, that genome() and targets() hold what the tests rely on."""
    names, seqs = genome()
    assert all(len(s) <= 3000 for s in seqs) and seqs[3][H_RUN:H_RUN + H_RUN_LEN] == "A" * H_RUN_LEN and H_RUN_LEN >= 96
    b, c, h, g = seqs[1], seqs[2], seqs[3], seqs[4]
    main = editors()[0]
    for correct in (False, True):
        edit = main + (correct, None)
        snvs = targets(seqs, edit)
        at = {}
        for i, v in enumerate(snvs):
            at.setdefault(v[:2], []).append(i)
        for name in NAMES:
            records, status = edit_sites(seqs, name, edit, snvs, key="planted")
            plus, minus = sum(r[3] == b"+" for r in records), sum(r[3] == b"-" for r in records)
            need = 20 if name in ("n20_nrg", "aux24", "n20") else 2
            assert plus >= need and minus >= need, (name, correct, plus, minus)
            if name in ("n20_nrg", "aux24", "n20"):
                bins = [sum(min(bystanders_of(r), 3) == k for r in records) for k in range(4)]
                assert all(bins), (name, correct, bins)
            assert {0, 1, 2, 3, 4} <= set(status), (name, correct)
            # the contigs' ends: the SNVs are there, and where the editor's change fits the end it is examined
            for ci in (1, 2):
                assert (ci, 0) in at and (ci, len(seqs[ci]) - 1) in at
            ends = [(3, 0), (4, len(g) - 1)] if not correct else [(4, 0), (3, len(h) - 1)]
            assert all(e in at and status[at[e][-1]] == 0 for e in ends), (name, correct)
            # beside the N: chrH's N stands between two letters the editor changes, one of them on each strand in each mode
            beside = [(3, H_CNT), (3, H_GNA)] if not correct else [(3, H_CNT + 2), (3, H_GNA + 2)]
            assert all(e in at and status[at[e][-1]] == 0 for e in beside), (name, correct)
            if name == "n20":                             # ... whose every protospacer holds the N; further off some starts are left
                per = {}
                for r in records:
                    per[r[7]] = per.get(r[7], 0) + 1
                assert all(per.get(at[e][-1], 0) == 0 for e in beside)
                near = [per.get(i, 0) for i, v in enumerate(snvs) if v[0] == 3 and abs(v[1] - (H_CNT + 1)) <= 25 and status[i] == 0]
                assert any(0 < k < main[2][1] - main[2][0] for k in near), (correct, near)
        # a FIXED target that has a record in one mode and none in the other
        records, status = edit_sites(seqs, "fixed_nrg", edit, snvs, key="planted")
        inside = (1, A.FIXED_PLUS + 7)
        assert b[inside[1]] == "C"
        if not correct:
            assert inside in at and [r for r in records if r[7] == at[inside][-1] and r[1] == A.FIXED_PLUS]
        else:
            assert not [r for r in records if r[0] == 1 and A.FIXED_PLUS <= r[1] < A.FIXED_PLUS + L]
            assert [r for r in records if r[0] == 3 and r[1] == H_FT_PLUS[0]]
    # a context: every status 0 to 5 under every pattern; a target at guide position 0 reads its context off the flank, one at a
    # contig's end has none
    for correct in (False, True):
        edit = editors()[2] + (correct, None)
        snvs = targets(seqs, edit)
        for name in NAMES:
            records, status = edit_sites(seqs, name, edit, snvs, key="planted")
            assert set(status) == {0, 1, 2, 3, 4, 5}, (name, correct)
            end = (3, 0) if not correct else (3, len(h) - 1)
            where = [i for i, v in enumerate(snvs) if v[:2] == end]
            assert where and status[where[-1]] == 5, (name, correct)
            if name == "n20":
                flank = [r for r in records if r[8] & 1 and (snvs[r[7]][1] == r[1] if r[3] == b"+" else snvs[r[7]][1] == r[1] + L - 1)]
                assert flank, correct
    # the homopolymer: A->G over the whole protospacer, every start a site, every other base a bystander
    edit = ("A", "G", (0, L), "N", False, None)
    inside = homopolymer_targets(seqs, L)
    records, status = edit_sites(seqs, "n20", edit, inside, key="planted")
    assert len(inside) >= 64 and set(status) == {0} and len(records) == L * len(inside) and all(bystanders_of(r) == L - 1 for r in records)
