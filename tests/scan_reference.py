"""The candidate filter (scan_rows.hip) by definition, in plain numpy: what calitas_scan_candidates must return.

The filter keeps every end column, on both strands, whose seamless glocal bottom-row score reaches minGuideScore.  With linear
costs that is "semi-global edit distance of the protospacer <= E" for E = scan_edits(L, d, costs) (search_plan.cpp, build_guide_dev):
an exact test at default costs, a superset of the passing columns otherwise.  tests/test_scan_reference.py holds this module
against the oracle's glocal enumeration; tests/test_gpu_scan.py holds the kernels against this module.
"""
import numpy as np

_SETS = {"A": 1, "C": 2, "G": 4, "T": 8, "U": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3, "B": 14, "D": 13, "H": 11, "V": 7, "N": 15}
_COMP4 = [0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15]   # IUPAC set of the complementary bases
DEFAULT_COSTS = (-120, -260, -122, -121)  # guideMismatch, pamMismatch, genomeGap, guideGap net costs (as oracle_lib.DEFAULT_COSTS)
TILE_LANES = 256                          # lanes of a scan tile (common.hpp LANES_PER_TILE): a tile is 256 x chunk bases


def scan_edits(L, d, costs=DEFAULT_COSTS):
    """The scan's edit budget E for a protospacer of L rows at max-guide-diffs d (build_guide_dev): the score budget
    |worst net cost| x d in units of the cheapest edit.  costs = (mismatch, pam mismatch, genome gap, guide gap) net costs."""
    m, _, b, B = (abs(c) for c in costs)
    budget = max(m, b, B) * d           # match x L - minGuideScore (SGA:239-243)
    return budget // min(m, b, B)


def target_sets(seq):
    """Per base of an ASCII contig: (set of ACGT it can stand for as a 4-bit mask, wildcard flag).  The filter's rule for the
    target: ACGT/U match their own letter, N / unknown bytes match nothing, any other IUPAC code matches every row."""
    s = np.frombuffer(seq.upper().encode(), dtype=np.uint8)
    sets = np.zeros(len(s), dtype=np.uint8)
    wild = np.zeros(len(s), dtype=bool)
    for ch, m in _SETS.items():
        sel = s == ord(ch)
        if ch in "ACGTU":
            sets[sel] = m
        elif ch != "N":
            wild[sel] = True
    return sets, wild


def last_row(query_sets, sets, wild):
    """Bottom row of the semi-global edit-distance matrix (free start in the target), one value per target position."""
    n = len(sets)
    prev = np.zeros(n + 1, dtype=np.int32)
    idx = np.arange(n + 1, dtype=np.int32)
    for i, q in enumerate(query_sets, start=1):
        match = wild | ((sets & q) != 0)
        sub = prev[:-1] + (~match).astype(np.int32)
        up = prev[1:] + 1
        m = np.minimum(sub, up)
        v = np.concatenate(([i], m)).astype(np.int32) - idx     # cur[j] = min over j' <= j of (v[j'] + j - j')
        prev = np.minimum.accumulate(v) + idx
    return prev[1:]


def dp_candidates(contigs, guides, E):
    """[(contig, offset, pass, guide)] by definition.  E: one edit budget for every guide, or one per guide.  Pass 1 = the guide
    against the reverse complement; its end column is reported at the contig offset of the alignment's first base in forward
    coordinates."""
    Es = list(E) if isinstance(E, (list, tuple)) else [E] * len(guides)
    assert len(Es) == len(guides)
    out = []
    for ci, (_, seq) in enumerate(contigs):
        if not seq:
            continue
        sets, wild = target_sets(seq)
        rsets = np.array([_COMP4[x] for x in sets[::-1]], dtype=np.uint8)
        rwild = wild[::-1]
        for gi, proto in enumerate(guides):
            q = [_SETS[c] for c in proto.upper()]
            fw = last_row(q, sets, wild)
            out += [(ci, int(j), 0, gi) for j in np.nonzero(fw <= Es[gi])[0]]
            rv = last_row(q, rsets, rwild)
            out += [(ci, len(seq) - 1 - int(j), 1, gi) for j in np.nonzero(rv <= Es[gi])[0]]
    out.sort()
    return out


def genome(seed, guides, lengths=(70000, 30011, 2000, 95, 31, 12), chunk=512):
    """Contigs of the given lengths with the guides planted (0-7 edits, both strands), soft-masking, N runs and blocks, tandem
    repeats and scattered IUPAC codes.  Some sites straddle the boundaries of scan lanes (chunk bases) and scan tiles
    (256 x chunk bases), some sit at the contig ends."""
    from calitas_amd import synth
    rng = np.random.default_rng(seed)
    tile = TILE_LANES * chunk
    contigs = []
    for ci, n in enumerate(lengths):
        seq = synth.make_contig(rng, n, softmask=0.3, n_run_ends=40 if n > 1000 else 0, n_block=700 if n > 20000 else 0, tandem_frac=0.02)
        if n > 1000:
            for proto in guides:
                for k in range(40):
                    pos = int(rng.integers(0, n - 40))
                    if k % 5 == 0:
                        pos = (pos // 512) * 512 - int(rng.integers(0, 24))       # straddling scan-lane and tile boundaries
                    if k % 10 == 3 and n > tile:
                        pos = (pos // tile) * tile - int(rng.integers(0, 40))     # straddling a tile boundary of this chunk size
                    if k % 7 == 0:
                        pos = int(rng.integers(0, 30)) if k % 2 else n - int(rng.integers(20, 60))
                    synth.plant_site(rng, seq, max(0, pos), proto, "", False, int(rng.integers(0, 8)), bool(rng.integers(0, 2)))
            for pos in rng.integers(0, n, size=n // 400):                             # IUPAC codes and stray N in the target
                seq[pos] = ord(rng.choice(list("RYKMSWBDHVNn")))
        contigs.append(("ctg%d" % ci, seq.tobytes().decode()))
    return contigs
