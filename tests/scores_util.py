"""Shared by the score tests (test_scores_host.py, test_gpu_scores.py): the model every mistake shows in, and the plantings that put
target letters outside ACGT, contig edges and both strands under a guide."""
import numpy as np

GUIDE = "CTTGCCCCACAGGGCAGTAAnrg"
SITE = "CTTGCCCCACAGGGCAGTAATGG"
_RC = str.maketrans("ACGTUMKRYVBHDWSN", "TGCAAKMYRBVDHWSN")


def revcomp(s):
    return s.translate(_RC)[::-1]


def distinct_model(C, L, seed=7):
    """All L * 25 + 2 factors distinct: seeded random integers in [1, 65535], duplicates drawn again.  (A uniform model would hide
    position, letter and orientation errors.)"""
    rng = np.random.default_rng(seed)
    seen, vals = set(), []
    while len(vals) < L * 25 + 2:
        v = int(rng.integers(1, 65536))
        if v not in seen:
            seen.add(v)
            vals.append(v)
    m = C.ScoreModel(L, np.array(vals[:L * 25], dtype=np.uint32).reshape(L, 5, 5), vals[-2], vals[-1])
    assert len(set(m.mismatch.ravel().tolist()) | {m.gap, m.pam_mismatch}) == L * 25 + 2
    return m


def with_base(site, k, b):
    return site[:k] + b + site[k + 1:]


def plant_edge_cases(seq):
    """The plantings of the score tests in a contig of at least 12 000 bases (a str): SITE with base 3 set to Y at 1000; the reverse
    complement of the same (the FASTA then holds R) at 3000; SITE with base 0 set to U at 5000; with base 7 set to N at 7000; the plain
    SITE at 9000, at position 3, and its reverse complement as the contig's last 23 bases."""
    s = list(seq)

    def put(pos, text):
        s[pos:pos + len(text)] = list(text)
    put(1000, with_base(SITE, 3, "Y"))
    put(3000, revcomp(with_base(SITE, 3, "Y")))
    put(5000, with_base(SITE, 0, "U"))
    put(7000, with_base(SITE, 7, "N"))
    put(9000, SITE)
    put(3, SITE)
    put(len(s) - len(SITE), revcomp(SITE))
    return "".join(s)
