"""GPU: the candidate filter (scan_rows.hip) on its own, through calitas_scan_candidates.

The filter decides which end columns the aligner kernel looks at: every position and strand whose seamless glocal bottom-row
score reaches minGuideScore, which for the reference's linear costs is "semi-global edit distance of the protospacer <= E"
(SearchReference.scala:432-441; enumeration rule of fgbio's Aligner.align(query, target, minScore) as called at
SequentialGuideAligner.scala:261-299).  Checked here against (a) a plain numpy dynamic programme of that definition and
(b) the first-generation column-wise kernel, which must emit the same records bit for bit.
"""
import pytest

from scan_reference import TILE_LANES, dp_candidates, genome, scan_edits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


CASES = [
    # id, guides (same length), d, chunk
    ("d5-chunk512", ["CTTGCCCCACAGGGCAGTAA"], 5, "512"),
    ("d5-chunk64", ["CTTGCCCCACAGGGCAGTAA"], 5, "64"),
    ("d3-chunk128-two-guides", ["CTTGCCCCACAGGGCAGTAA", "GACCTTGAAGTCTCAGTATA"], 3, "128"),
    ("d8-chunk256", ["CTTGCCCCACAGGGCAGTAA"], 8, "256"),
    ("iupac-guide-d4", ["GAGAATTGNTTGAACCCRGG"], 4, "512"),
    ("L32-d6-two-warm-up-words", ["CTTGCCCCACAGGGCAGTAACGGTTCAATGCA"], 6, "512"),
    ("L32-d6-chunk64", ["CTTGCCCCACAGGGCAGTAACGGTTCAATGCA"], 6, "64"),
    ("L12-d2", ["GCAGTAACCTGA"], 2, "256"),
    ("d0", ["CTTGCCCCACAGGGCAGTAA"], 0, "512"),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_scan_candidates_equal_plain_dp_and_columnwise_kernel(C, case, monkeypatch):
    cid, guides, d, chunk = case
    contigs = genome(len(cid) + d, guides)
    monkeypatch.setenv("CALITAS_CHUNK", chunk)        # bases per scan lane (read when the reference is packed)
    ctx = C.Context(0)
    try:
        ctx.set_reference([n for n, _ in contigs], [s.encode() for _, s in contigs])
        G = [C.Guide(g) for g in guides]              # PAM-less: the filter only sees the protospacer
        params = C.make_params(max_guide_diffs=d, max_pam_mismatches=0, max_gaps_between_guide_and_pam=0)
        rows_kernel = ctx.scan_candidates(G, params)
        cols_kernel = ctx.scan_candidates(G, params, columnwise=True)   # round 1's kernel: an independent second implementation
    finally:
        ctx.close()
    want = dp_candidates(contigs, guides, d)          # default costs: a bottom-row score >= minGuideScore <=> <= d edits
    assert len(want) > 10
    assert rows_kernel == want, (cid, len(rows_kernel), len(want), sorted(set(rows_kernel) ^ set(want))[:5])
    assert cols_kernel == want, (cid, len(cols_kernel), len(want), sorted(set(cols_kernel) ^ set(want))[:5])


def test_scan_queue_overflow_on_dense_repeats(C, monkeypatch):
    """A homopolymer matched by a homopolymer guide flags every word of every lane: the tile's suspect queue and record stage
    overflow, and the kernel has to resolve / append in place without losing a column."""
    contigs = [("polyA", "A" * 40000 + "C" * 3000 + "A" * 9000), ("mixed", "ACGT" * 2000 + "A" * 5000)]
    monkeypatch.setenv("CALITAS_CHUNK", "512")
    ctx = C.Context(0)
    try:
        ctx.set_reference([n for n, _ in contigs], [s.encode() for _, s in contigs])
        got = ctx.scan_candidates([C.Guide("A" * 20)], C.make_params(max_guide_diffs=2, max_pam_mismatches=0, max_gaps_between_guide_and_pam=0))
    finally:
        ctx.close()
    want = dp_candidates(contigs, ["A" * 20], 2)
    assert len(want) > 50000
    assert got == want


# ---------------------------------------------------------------------------------------------------------------------
# the limits the host accepts (plan_search / build_guide_dev): every scan_rows_kernel<NW, NWARM> instantiation, L + E = 64,
# E >= L, E != d, mixed protospacer lengths in one launch, 64 guides, contigs across several tiles
# ---------------------------------------------------------------------------------------------------------------------
L20 = "CTTGCCCCACAGGGCAGTAA"
L24 = "CTTGCCCCACAGGGCAGTAACGGT"
L32 = "CTTGCCCCACAGGGCAGTAACGGTTCAATGCA"
COSTS_3D = dict(guide_mismatch_net_cost=-100, pam_mismatch_net_cost=-260, genome_gap_net_cost=-300, guide_gap_net_cost=-300)   # E = 3d
COLUMNWISE_REFUSES = {}   # case id -> message of a shape the column-wise kernel refuses (none so far: it takes every shape the host takes)


def _costs(kw):
    return (kw.get("guide_mismatch_net_cost", -120), kw.get("pam_mismatch_net_cost", -260), kw.get("genome_gap_net_cost", -122),
            kw.get("guide_gap_net_cost", -121))


def scan_both(C, contigs, guides, params, chunk, monkeypatch):
    """(row-wise records, column-wise records or the column-wise refusal as a string, (chunk, warm-up words) of the scan_rows_kernel
    instantiation the host launched) of one launch at this lane chunk."""
    monkeypatch.setenv("CALITAS_CHUNK", str(chunk))
    ctx = C.Context(0)
    try:
        ctx.set_reference([n for n, _ in contigs], [s.encode() for _, s in contigs])
        G = [C.Guide(g) for g in guides]
        rows = ctx.scan_candidates(G, params)
        v = ctx.timing()["scan_variant"]
        try:
            cols = ctx.scan_candidates(G, params, columnwise=True)
        except C.CalitasError as e:
            cols = "refused: %s" % e
    finally:
        ctx.close()
    return rows, cols, (v >> 8, v & 0xFF)


def check_scan(cid, rows, cols, want):
    assert rows == want, (cid, len(rows), len(want), sorted(set(rows) ^ set(want))[:5])
    if cid in COLUMNWISE_REFUSES:
        assert isinstance(cols, str) and COLUMNWISE_REFUSES[cid] in cols, (cid, cols if isinstance(cols, str) else len(cols))
    else:
        assert cols == want, (cid, cols if isinstance(cols, str) else (len(cols), sorted(set(cols) ^ set(want))[:5]))


# (chunk, warm words): L = 20, d = 4 needs one warm-up word (L + E - 1 = 23), L = 24, d = 12 two (35); the test reads back what ran.  Every contig list has one
# contig longer than two tiles of that chunk, so lanes read the previous tile's halo chunk and sites straddle tile boundaries.
INSTANTIATIONS = [(chunk, warm) for chunk in (64, 128, 256, 512) for warm in (1, 2)]


@pytest.mark.parametrize("chunk,warm", INSTANTIATIONS, ids=["chunk%d-warm%d" % x for x in INSTANTIATIONS])
def test_every_scan_rows_instantiation_across_tiles(C, chunk, warm, monkeypatch):
    proto, d = (L20, 4) if warm == 1 else (L24, 12)
    E = scan_edits(len(proto), d)
    tile = TILE_LANES * chunk
    contigs = genome(chunk + warm, [proto], lengths=(2 * tile + 5003, 3001, 95), chunk=chunk)
    params = C.make_params(max_guide_diffs=d, max_pam_mismatches=0, max_gaps_between_guide_and_pam=0)
    rows, cols, launched = scan_both(C, contigs, [proto], params, chunk, monkeypatch)
    assert launched == (chunk, warm)                           # the instantiation this case is about is the one that ran
    want = dp_candidates(contigs, [proto], E)
    assert len(want) > 10 and any(off >= 2 * tile for c, off, _, _ in want if c == 0)
    check_scan("chunk%d-warm%d" % (chunk, warm), rows, cols, want)


LIMIT_CASES = [
    # id, guides (one CLI length), d, costs, chunk, contig lengths
    # L + E = 64 exactly: the truncation argument (L + E - 1 <= 32 x NWARM) with no slack, and E >= L: every column is a candidate,
    # so the suspect queue and the record stage overflow on every tile
    ("L32-E32-chunk64", [L32], 32, {}, 64, (40000, 3001, 95)),
    ("L32-E32-chunk512", [L32], 32, {}, 512, (40000, 3001, 95)),
    ("L20-E44-chunk64", [L20], 44, {}, 64, (40000, 2000, 40)),
    ("L20-E44-chunk256", [L20], 44, {}, 256, (40000, 2000, 40)),
    ("E-above-L-L24-E30-chunk128", [L24], 30, {}, 128, (30000, 1500)),
    # E < L with two warm-up words: bottom-row values of random text sit around E, so a chain that starts too late (too few
    # warm-up columns in front of a lane's first positions) raises some of them above E
    ("L32-E31-chunk64", [L32], 31, {}, 64, (30000, 2000)),
    ("L32-E15-chunk64", [L32], 15, {}, 64, (60000, 2000)),
    ("L32-E15-chunk256", [L32], 15, {}, 256, (70000, 2000)),
    # E = 3d: only the E != d cases tell the scan's budget from max-guide-diffs
    ("costs-E3d-L20-d4-chunk128", [L20], 4, COSTS_3D, 128, (60000, 2000)),
    ("costs-E3d-L28-d12-chunk512", [L24 + "GATC"], 12, COSTS_3D, 512, (30000, 1200)),
    ("costs-E3d-L20-d3-chunk64", [L20], 3, COSTS_3D, 64, (40000, 1500)),
    # guides of different protospacer lengths in one launch (one CLI length, 32): the warm-up words come from the longest guide,
    # each guide runs with its own L and E
    ("mixed-L16-L20-L32", ["GACCTTGAAGTCTCAGacgtnnrgttcaagcg", L20 + "acgtnrgtcaag", L32], 6, {}, 512, (60000, 9000, 300)),
    ("mixed-L16-L20-L32-chunk64", ["GACCTTGAAGTCTCAGacgtnnrgttcaagcg", L20 + "acgtnrgtcaag", L32], 6, {}, 64, (60000, 9000, 300)),
    ("mixed-E3d-L20-L32-chunk256", [L20 + "acgtnrgtcaag", L32], 3, COSTS_3D, 256, (70000, 300)),
]


@pytest.mark.parametrize("case", LIMIT_CASES, ids=lambda c: c[0])
def test_scan_at_the_host_limits(C, case, monkeypatch):
    cid, guides, d, costs, chunk, lengths = case
    protos = [C.Guide(g).guide for g in guides]
    E = [scan_edits(len(p), d, _costs(costs)) for p in protos]
    assert all(len(p) + e <= 64 for p, e in zip(protos, E))
    contigs = genome(len(cid) + d, protos, lengths=lengths, chunk=chunk)
    params = C.make_params(max_guide_diffs=d, max_pam_mismatches=0, max_gaps_between_guide_and_pam=0, **costs)
    rows, cols, launched = scan_both(C, contigs, guides, params, chunk, monkeypatch)
    assert launched == (chunk, max((len(p) + e - 1 + 31) // 32 for p, e in zip(protos, E)))   # warm-up words of the longest L + E
    want = dp_candidates(contigs, protos, E)
    assert len(want) > 10 and {g for *_, g in want} == set(range(len(guides)))
    check_scan(cid, rows, cols, want)
    if any(e >= len(p) for p, e in zip(protos, E)):          # E >= L: every column of every live tile, on both strands
        n = sum(len(s) for _, s in contigs) * 2 * sum(1 for p, e in zip(protos, E) if e >= len(p))
        assert sum(1 for c, off, _, g in want if E[g] >= len(protos[g])) == n


def test_scan_64_guides_in_one_launch(C, monkeypatch):
    """MAX_GUIDES guides in one launch: the guide field of ScanRecord::info (bits 17-22) reaches 63."""
    from calitas_amd import synth
    guides = [g[:20] for g in synth.random_guides(0x64, 64)]
    contigs = genome(64, guides[-4:], lengths=(40000, 3000))      # sites of the last guides planted: they have candidates for sure
    params = C.make_params(max_guide_diffs=3, max_pam_mismatches=0, max_gaps_between_guide_and_pam=0)
    rows, cols, launched = scan_both(C, contigs, guides, params, 256, monkeypatch)
    assert launched == (256, 1)
    want = dp_candidates(contigs, guides, 3)
    assert any(g == 63 for *_, g in want)
    check_scan("64-guides", rows, cols, want)
