"""GPU: end-to-end searches at the limits the host accepts (post.cpp make_guide_host, search_plan.cpp plan_search / build_guide_dev), against
the CPU oracle, every column -- and one step past each limit, which must be refused with CalitasError and leave the context usable.

| limit                                  | at the limit                                   | one past it                         |
|----------------------------------------|------------------------------------------------|-------------------------------------|
| protospacer rows <= 32                 | L32-nrg-d10-p2-g16, L32-pamless-L+E=64         | refusal "33 rows"                   |
| scan budget L + E <= 64                | L32-pamless-L+E=64 (E >= L: every column),     | refusal "L+E=65"                    |
|                                        | test_mixed_lengths_with_32_rows_at_d32         |                                     |
| max-gaps-between-guide-and-pam <= 16   | L32-nrg-d10-p2-g16, L24-pam16-g16,             | refusal "g=17"                      |
|                                        | L32-pam16-g16-d32 (113 of trace_kernel's 144   |                                     |
|                                        | TB_LEN bytes: span 64 + g 16 + a 16-nt PAM)    |                                     |
| PAM <= 16 nt                           | L24-pam16-g16, L32-pam16-g16-d32               | refusal "17-nt PAM"                 |
| 8 PAMs                                 | main-pam-and-7-aux                             | (the ABI takes 8 at most)           |
| 64 guides per pass                     | test_64_guides_in_one_pass                     | refusal "65 guides"                 |
| windows per 16-base word <= 8          | eight-windows-per-word                         | refusal "9 windows per word"        |
| align_pk_kernel: 4 big (L + 2) < 30000 | pack16-edge-29920 / pack16-beyond-30008        | (the other kernel, same rows)       |
| E != d (scan budget from the costs)    | costs-E3d-L20, costs-E3d-L28                   |                                     |
| mixed L / PAM side in one pass         | test_mixed_guides_in_one_pass                  | another CLI length: refused         |

The limits of the counts, score and site kernels are held by tests of their own modules:

| limit                                  | at the limit                                   | one past it                         |
|----------------------------------------|------------------------------------------------|-------------------------------------|
| counts table <= 4096 cells in LDS      | test_gpu_table_limits: cells-4096              | cells-4224, cells-4524-sparse,      |
| (COUNTS_LDS_CELLS)                     |                                                | cells-9702-dense (the largest table |
|                                        |                                                | a search asks for): added directly  |
| device table zero between calls        | test_the_device_table_is_left_clean            |                                     |
| 128 x 256 lanes of a counts kernel     | test_more_items_than_one_stride (> 65 536      |                                     |
|                                        | items: a second and a third stride)            |                                     |
| score factors 0 .. 65536 (17 bits)     | test_factors_of_zero_and_one                   | (ScoreModel takes none above)       |
| 8 PAMs of a site pattern               | test_gpu_sites: eight_pams, five_prime_eight,  | (the ABI takes 8 at most)           |
|                                        | test_every_pam_index_wins_on_both_strands      |                                     |
| 5' PAM <= 16 nt (lo = -16)             | five_prime_eight, five16_L32                   | refusal "17-nt PAM" above           |
| footprint 1 .. 48 bases                | one_letter (1), foot33, foot47, max48,         |                                     |
|                                        | five16_L32 (48)                                |                                     |
| 1024 threads of sites_offsets_kernel   | test_many_segments_through_the_offsets_scan    |                                     |
|                                        | (two and three counts per thread)              |                                     |
"""
import re

import pytest

from parity_util import assert_same, oracle_rows, product_rows, synth_fasta

pytestmark = pytest.mark.gpu

L20 = "CTTGCCCCACAGGGCAGTAA"
L24 = "CTTGCCCCACAGGGCAGTAACGGT"
L28 = L24 + "GATC"
L32 = "CTTGCCCCACAGGGCAGTAACGGTTCAATGCA"
COSTS_3D = dict(guide_mismatch_net_cost=-100, pam_mismatch_net_cost=-260, genome_gap_net_cost=-300, guide_gap_net_cost=-300)
# align_pk_kernel takes a launch when 4 x big x (L + 2) < 30 000, big = the largest |score| of match, mismatch and the two gaps:
# at L = 20 big = 340 gives 29 920 (packed), 341 gives 30 008 (align_kernel).  The cheapest edit is half the dearest: E = 2d.
PACK_EDGE = dict(guide_mismatch_net_cost=-170, pam_mismatch_net_cost=-260, genome_gap_net_cost=-340, guide_gap_net_cost=-340)
PACK_BEYOND = dict(guide_mismatch_net_cost=-170, pam_mismatch_net_cost=-260, genome_gap_net_cost=-341, guide_gap_net_cost=-341)
SMALL = (22000, 6000, 700, 31)       # E >= L cases: the oracle enumerates every column of every window


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


CONFIGS = [
    # (id, guide, aux, params, contig lengths)
    ("L32-nrg-d10-p2-g16", L32 + "nrg", (), dict(d=10, p=2, g=16), (60000, 20000, 900)),
    ("L32-pamless-L+E=64", L32, (), dict(d=32, p=0, g=0), SMALL),
    ("L24-pam16-g16", L24 + "ngggtcagttcaagcn", (), dict(d=4, p=2, g=16), (60000, 20000, 900)),
    ("L32-pam16-g16-d32", L32 + "ngggtcagttcaagcn", (), dict(d=32, p=2, g=16), SMALL),
    ("main-pam-and-7-aux", L20 + "nrg", ("nag", "ngcg", "nnagaaw", "nnnrrt", "ngaa", "nnngatt", "nrrh"), dict(d=4, p=1, g=3), (60000, 20000, 900)),
    ("costs-E3d-L20", L20 + "nrg", (), dict(d=4, p=1, g=2, **COSTS_3D), (40000, 9000)),
    ("costs-E3d-L28", L28 + "nrg", (), dict(d=4, p=1, g=2, **COSTS_3D), (40000, 9000)),
    ("pack16-edge-29920", L20 + "nrg", (), dict(d=12, p=1, g=2, **PACK_EDGE), SMALL),
    ("pack16-beyond-30008", L20 + "nrg", (), dict(d=12, p=1, g=2, **PACK_BEYOND), SMALL),
    # window 35, step 35 - (23 + 4 + 2 - 1) = 7: (35 + 14) // 7 + 1 = 8 windows a 16-base word can fall into
    ("eight-windows-per-word", L20 + "nrg", (), dict(d=4, p=1, g=2, window_size=35), (20000, 4000)),
]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: c[0])
def test_search_at_the_limits(C, cfg, tmp_path):
    cid, guide, aux, params, lengths = cfg
    W = params.get("window_size", 1000)
    step = W - (len(guide) + params.get("d", 5) + params.get("g", 3) - 1)
    fa = synth_fasta(tmp_path, 101 + len(cid), [guide], lengths=lengths, step_hint=step)
    prod = product_rows(C, fa, guide, aux, **params)
    orac = oracle_rows(fa, guide, aux, **params)
    assert len(orac) > 0
    assert_same(prod, orac, cid)


# one CLI length (23), different protospacer lengths, 3' PAM, 5' PAM, PAM-less, IUPAC codes in the protospacer
MIXED = ["CTTGCCCCACAGGGCAGTAAnrg", "tttvAACCAACCAACCGGTTACG", "GTGACTTGAAGTCTCAGTATAGC", "GAGAATTGNTTGAACCCRGGnrg",
         "ACGTACATGCTCGATACGAnngg", "ttgaacgAGCTAGGCATCGATCG"]


def test_mixed_guides_in_one_pass(C, tmp_path):
    """calitas_search and calitas_search_hits_batch with guides that share a CLI length and nothing else: every guide's rows are
    its own oracle run's.  (align_pk_kernel is off for such a launch -- same_L -- and align_kernel runs each job with its own L.)"""
    fa = synth_fasta(tmp_path, 113, MIXED, lengths=(60000, 25000, 800))
    kw = dict(d=4, p=1, g=2)
    want = [oracle_rows(fa, g, **kw) for g in MIXED]
    assert all(len(w) > 0 for w in want)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        params = C.make_params(max_guide_diffs=4, max_pam_mismatches=1, max_gaps_between_guide_and_pam=2)
        G = [C.Guide(g) for g in MIXED]
        alns = ctx.search(G, params)
        for gi, g in enumerate(G):
            text, _ = ctx.hits_tsv(g, "a", params, [a for a in alns if a.guide_index == gi])
            assert_same(C.read_hits(text), want[gi], "search, guide %d" % gi)
        for gi, (text, n) in enumerate(ctx.search_hits_batch(G, ["a"] * len(G), params, "v0", "stamp")):
            assert_same(C.read_hits(text), want[gi], "batch, guide %d" % gi)
    finally:
        ctx.close()


def test_mixed_lengths_with_32_rows_at_d32(C, tmp_path):
    """Guides of 16, 20 and 32 rows in one launch (CLI length 32) at d = 32, E >= L for all: align_kernel puts two jobs of 32 lanes in
    a wave, and lane 63 is row 32 of the second job exactly when that job's guide has 32 rows, whatever the first job's guide is.
    (Each job now decides for its own last lane; before, both took the first job's L, and a first job without work this round left
    that L undefined -- L32-pamless-L+E=64 above failed with "inconsistent traceback" on a fresh context.)  Every guide's rows
    against its own oracle run, through calitas_search and calitas_search_hits_batch."""
    guides = [L20 + "acgtnrgtcaag", L32, "GACCTTGAAGTCTCAGacgtnnrgttcaagcg"]
    fa = synth_fasta(tmp_path, 131, guides, lengths=SMALL)
    kw = dict(d=32, p=2, g=0)
    want = [oracle_rows(fa, g, **kw) for g in guides]
    assert all(len(w) > 0 for w in want)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        params = C.make_params(max_guide_diffs=32, max_pam_mismatches=2, max_gaps_between_guide_and_pam=0)
        G = [C.Guide(g) for g in guides]
        alns = ctx.search(G, params)
        for gi, g in enumerate(G):
            text, _ = ctx.hits_tsv(g, "a", params, [a for a in alns if a.guide_index == gi])
            assert_same(C.read_hits(text), want[gi], "search, guide %d" % gi)
        for gi, (text, n) in enumerate(ctx.search_hits_batch(G, ["a"] * len(G), params, "v0", "stamp")):
            assert_same(C.read_hits(text), want[gi], "batch, guide %d" % gi)
    finally:
        ctx.close()


def test_64_guides_in_one_pass(C, tmp_path):
    """MAX_GUIDES guides in one calitas_search: guide by guide what single-guide passes return; the last guide against the oracle."""
    from calitas_amd import synth
    guides = synth.random_guides(0x40, 64)
    fa = synth_fasta(tmp_path, 64, guides[:4] + guides[-4:], lengths=(40000, 12000))
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        params = C.make_params(max_guide_diffs=4, max_gaps_between_guide_and_pam=2)
        G = [C.Guide(g) for g in guides]
        alns = ctx.search(G, params)
        key = lambda a: (a.contig_index, a.window_start, a.strand, a.start_offset, a.end_offset, a.score, a.ops, a.pam_index)
        assert any(a.guide_index == 63 for a in alns)
        for gi in range(64):
            single = [key(a) for a in ctx.search([G[gi]], params)]
            assert [key(a) for a in alns if a.guide_index == gi] == single, gi
        text, _ = ctx.hits_tsv(G[63], "a", params, [a for a in alns if a.guide_index == 63])
        assert_same(C.read_hits(text), oracle_rows(fa, guides[63], d=4, g=2), "guide 63")
    finally:
        ctx.close()


# one past each limit: (id, guides, params, message)
PAST = [
    ("L+E=65", [L32], dict(max_guide_diffs=33, max_pam_mismatches=0, max_gaps_between_guide_and_pam=0), "too large for the scan warm-up"),
    ("L20-L+E=65", [L20], dict(max_guide_diffs=45, max_pam_mismatches=0, max_gaps_between_guide_and_pam=0), "too large for the scan warm-up"),
    ("g=17", [L20 + "nrg"], dict(max_gaps_between_guide_and_pam=17), "max-gaps-between-guide-and-pam must be 0..16"),
    ("17-nt PAM", [L20 + "ngggtcagttcaagcnn"], dict(), "PAM longer than 16 nt"),
    ("33 rows", [L32 + "A"], dict(max_guide_diffs=2), "protospacer longer than 32 nt"),
    ("65 guides", [L20 + "nrg"] * 65, dict(), "n_guides must be 1..64"),
    # window 34: step 6, (34 + 14) // 6 + 1 = 9
    ("9 windows per word", [L20 + "nrg"], dict(window_size=34, max_guide_diffs=4, max_gaps_between_guide_and_pam=2), "more than 8 windows per position"),
]


def test_one_past_each_limit_is_refused(C, tmp_path):
    guide = L20 + "nrg"
    fa = synth_fasta(tmp_path, 117, [guide], lengths=(20000, 3000))
    want = oracle_rows(fa, guide, d=4, g=2)
    assert len(want) > 0
    ok = C.make_params(max_guide_diffs=4, max_gaps_between_guide_and_pam=2)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        for cid, guides, kw, msg in PAST:
            with pytest.raises(C.CalitasError, match=re.escape(msg)):
                ctx.search([C.Guide(g) for g in guides], C.make_params(**kw))
            if len(guides) == 1:
                with pytest.raises(C.CalitasError, match=re.escape(msg)):
                    ctx.search_hits(C.Guide(guides[0]), "a", C.make_params(**kw), "v0", "stamp")
            text, _ = ctx.search_hits(C.Guide(guide), "a", ok, "v0", "stamp")       # the context is still good
            assert_same(C.read_hits(text), want, "after %s" % cid)
        with pytest.raises(C.CalitasError, match=re.escape("same length")):          # a pass shares one CLI length
            ctx.search([C.Guide(guide), C.Guide(L20 + "nngg")], ok)
    finally:
        ctx.close()
