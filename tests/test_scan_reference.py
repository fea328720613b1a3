"""CPU: tests/scan_reference.py -- the definition test_gpu_scan.py holds the scan kernels to -- against the oracle's restatement of
fgbio's glocal enumeration (Aligner.align(query, target, minScore)), which is what the aligner stage must see.

Every end column the oracle enumerates at minGuideScore must be a candidate at E = scan_edits(L, d, costs): the filter may keep more,
never fewer.  At default costs on a target of A/C/G/T/N the two sets are equal; other IUPAC codes in the target are wildcards for
the filter (the oracle matches them by set), so there the filter may only be wider.
"""
import numpy as np
import pytest

import oracle_lib as O
from scan_reference import _SETS, DEFAULT_COSTS, dp_candidates, scan_edits

IUPAC_GUIDE = "RYSWKMBDHVN"
IUPAC_TARGET = "RYKMSWBDHV"


def min_guide_score(L, d, costs):
    m, _, b, B = (abs(c) for c in costs)
    return (m // 2) * L - max(m, b, B) * d                         # SGA:239-243 with derive_scores' match score


def oracle_end_columns(proto, target, d, costs):
    """0-based end columns of the oracle's glocal enumeration ("targetStart-targetEnd:score:cigar", 1-based inclusive)."""
    return sorted({int(a.split(":")[0].split("-")[1]) - 1 for a in O.glocal(proto, target, min_guide_score(len(proto), d, costs), costs)})


def revcomp(s):
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K",
            "B": "V", "V": "B", "D": "H", "H": "D"}
    return "".join(comp[c.upper()].lower() if c.islower() else comp[c.upper()] for c in reversed(s))


def random_case(rng, iupac_target, default_costs):
    L = int(rng.integers(8, 33))
    proto = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, L))
    for _ in range(int(rng.integers(0, 3))):                       # IUPAC codes in the guide
        k = int(rng.integers(0, L))
        proto = proto[:k] + IUPAC_GUIDE[int(rng.integers(0, len(IUPAC_GUIDE)))] + proto[k + 1:]
    if default_costs:
        costs = DEFAULT_COSTS
    else:                                                          # cheapest edit down to a fifth of the dearest
        hi = int(rng.integers(100, 700))
        lo = int(rng.integers(max(2, hi // 5), hi + 1))
        pick = [hi, lo, int(rng.integers(lo, hi + 1))]
        rng.shuffle(pick)
        costs = (-pick[0], -int(rng.integers(100, 400)), -pick[1], -pick[2])
    # d up to the scan's L + E <= 64 edge
    d = int(rng.integers(0, 9))
    while d > 0 and L + scan_edits(L, d, costs) > 64:
        d -= 1
    n = int(rng.integers(60, 400))
    t = list("".join("ACGT"[int(x)] for x in rng.integers(0, 4, n)))
    for _ in range(int(rng.integers(1, 4))):                       # the guide planted with a few edits, so some columns pass
        pos = int(rng.integers(0, max(1, n - L)))
        site = [c if c in "ACGT" else "ACGT"[int(_SETS[c]).bit_length() - 1] for c in proto]   # IUPAC codes realised as a base
        for _ in range(int(rng.integers(0, d + 2))):
            k = int(rng.integers(0, len(site)))
            op = int(rng.integers(0, 3))
            if op == 0:
                site[k] = "ACGT"[int(rng.integers(0, 4))]
            elif op == 1 and len(site) > 1:
                del site[k]
            else:
                site.insert(k, "ACGT"[int(rng.integers(0, 4))])
        t[pos:pos + len(site)] = site
    t = t[:n]
    codes = "N" + (IUPAC_TARGET if iupac_target else "")
    for pos in rng.integers(0, n, size=int(rng.integers(0, 8))):   # N and IUPAC codes in the target
        t[pos] = codes[int(rng.integers(0, len(codes)))]
    for pos in rng.integers(0, n, size=int(rng.integers(0, n // 3 + 1))):   # lower case (soft-masking)
        t[pos] = t[pos].lower()
    target = "".join(t)
    return proto, target, d, costs


def _check(seed, iupac_target, default_costs):
    rng = np.random.default_rng(seed)
    for it in range(40):
        proto, target, d, costs = random_case(rng, iupac_target, default_costs)
        E = scan_edits(len(proto), d, costs)
        assert len(proto) + E <= 64
        cand = dp_candidates([("t", target)], [proto], E)
        fw = sorted(off for _, off, pas, _ in cand if pas == 0)
        rv = sorted(off for _, off, pas, _ in cand if pas == 1)
        want_fw = oracle_end_columns(proto, target, d, costs)
        # pass 1: the oracle on the reverse complement; its end column j is reported at the alignment's first base, len - 1 - j
        want_rv = sorted(len(target) - 1 - j for j in oracle_end_columns(proto, revcomp(target), d, costs))
        tag = (seed, it, proto, d, E, costs, target)
        if default_costs and not iupac_target:
            assert E == d, tag
            assert fw == want_fw, (tag, sorted(set(fw) ^ set(want_fw)))
            assert rv == want_rv, (tag, sorted(set(rv) ^ set(want_rv)))
        else:
            assert set(want_fw) <= set(fw), (tag, sorted(set(want_fw) - set(fw)))
            assert set(want_rv) <= set(rv), (tag, sorted(set(want_rv) - set(rv)))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_filter_equals_oracle_at_default_costs(seed):
    _check(seed, iupac_target=False, default_costs=True)


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_filter_never_drops_a_column_with_iupac_targets(seed):
    _check(seed, iupac_target=True, default_costs=True)


@pytest.mark.parametrize("seed", [21, 22, 23, 24])
def test_filter_never_drops_a_column_at_other_costs(seed):
    _check(seed, iupac_target=bool(seed % 2), default_costs=False)


def test_scan_edits_restates_build_guide_dev():
    assert scan_edits(20, 5) == 5 and scan_edits(32, 32) == 32 and scan_edits(20, 44) == 44     # 122 d // 120 below d = 60
    assert scan_edits(20, 4, (-100, -260, -300, -300)) == 12                                      # E = 3d
    assert scan_edits(20, 12, (-170, -260, -340, -341)) == 24
    assert scan_edits(20, 0, (-500, -260, -100, -400)) == 0
