"""GPU: the off-target table of calitas_search_counts / calitas_search_counts_batch (counts_kernel in hits.hip, bin_counts_kernel in
binned.hip, the host stage behind them) against the table of the text the same call returns through calitas_search_hits --
counts_of_rows(read_hits(text)) -- on every path a call can take, against the oracle's rows for the parameter shapes, as sums over
window ranges, and through the guide batch."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fasta_util import write_fasta
from parity_util import oracle_rows, synth_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = 8192
GUIDE = "CTTGCCCCACAGGGCAGTAAnrg"
UNIT = b"CTTGCCCCACAGGGCAGTAATGG"
STEP = 1000 - (len(GUIDE) + 5 + 2 - 1)        # window step at d = 5, g = 2


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


def planted(rng, length, sites, site=UNIT.decode()):
    """Random contig with (position, edits, reverse) sites planted: the site itself, mutated at `edits` protospacer positions."""
    seq = rng.choice(list(b"ACGT"), size=length).astype(np.uint8)
    comp = {65: 84, 67: 71, 71: 67, 84: 65}
    for pos, edits, rev in sites:
        s = bytearray(site.encode())
        for k in rng.choice(20, size=edits, replace=False):
            s[k] = ord("ACGT"[("ACGT".index(chr(s[k])) + 1) % 4])
        if rev:
            s = bytearray(comp[c] for c in reversed(s))
        seq[pos:pos + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    return seq.tobytes().decode()


def genome(tmp_path, crowded):
    """Four contigs: sites at 0-5 edits on both strands around every bin boundary and around the window starts next to it, random
    sites elsewhere; crowded: plus a chain of tandem copies (8 bases apart, across a bin boundary) and 110 separate copies 30 bases apart
    -- more alignments than a bin's wave holds.  Returns (fasta, contig lengths)."""
    rng = np.random.default_rng(4242)
    contigs = []
    for ci, length in enumerate((3 * BIN + 9000, 2 * BIN + 5000, 40000, 30000)):
        sites = []
        for b in range(BIN, length - 200, BIN):
            w = (b // STEP) * STEP                                # the window starts left and right of the boundary
            for d in (-40 - ci, -1 - 11 * ci, 30 + ci):          # (a bin's wave holds 64 raw alignments: a handful of sites per bin)
                sites.append((b + d, int(rng.integers(0, 6)), bool(rng.integers(0, 2))))
            for ws, d in ((w, 5 + ci), (w + STEP, -20 - ci)):    # (inside the stretch two windows share: found twice)
                sites.append((ws + d, int(rng.integers(0, 6)), bool(rng.integers(0, 2))))
        sites += [(int(p), int(rng.integers(0, 6)), bool(rng.integers(0, 2))) for p in rng.integers(200, length - 200, size=6)]
        seq = bytearray(planted(rng, length, [s for s in sites if 100 < s[0] < length - 100]).encode())
        if crowded and ci == 2:
            for k in range(14):
                seq[BIN - 60 + 8 * k: BIN - 60 + 8 * k + len(UNIT)] = UNIT
        if crowded and ci == 3:
            for k in range(110):
                seq[12000 + 30 * k: 12000 + 30 * k + len(UNIT)] = UNIT
        contigs.append(("k%d" % ci, seq.decode()))
    fa = write_fasta(str(tmp_path / ("crowded.fa" if crowded else "plain.fa")), contigs + [("tiny", "ACGT" * 20)])
    return fa, [len(s) for _, s in contigs] + [80]


def text_table(C, ctx, G, params, shape):
    text, n = ctx.search_hits(G, "a", params, "v0", "stamp")
    rows = C.read_hits(text)
    assert len(rows) == n
    return C.counts_of_rows(rows, shape), n


ENV_PATHS = [("default", {}), ("general", {"CALITAS_BINNED": "0"}), ("wave-per-bin", {"CALITAS_BINNED_COMPLEX": "1"}),
             ("three-ranges", {"CALITAS_CHUNKS": "3"}), ("one-range", {"CALITAS_CHUNKS": "1"}), ("host-hits", {"CALITAS_HOST_HITS": "1"}),
             ("per-contig", {"CALITAS_SEQUENTIAL": "1"})]


def test_every_path_gives_the_table_of_the_text(C, tmp_path, monkeypatch):
    """search_counts == counts_of_rows(read_hits(search_hits text)) on the per-bin kernels, the general kernels, the wave-per-bin kernel,
    three ranges and one, the host stages, one pass per contig and -O 0 (which the device row stage declines)."""
    fa, _ = genome(tmp_path, crowded=False)
    G = C.Guide(GUIDE)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        params = C.make_params(max_gaps_between_guide_and_pam=2)
        first = None
        for name, env in ENV_PATHS:
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got = ctx.search_counts(G, params)
            tm = ctx.timing()
            assert got.dtype == np.uint64 and got.shape == (2, 6, 8, 2), name
            want, n = text_table(C, ctx, G, params, got.shape)
            print(name, "rows", n, "cells", int(np.count_nonzero(want)), "binned_lanes", tm["binned_lanes"], "lanes", tm["lanes"], "passes", tm["contig_passes"])
            assert np.array_equal(got, want), name
            assert tm["hit_rows"] == n == int(got.sum()) and tm["hits_bytes"] == 0, name
            if name == "default":
                assert tm["binned_lanes"] > 0
                first = got
                assert n > 40 and np.count_nonzero(got) >= 12 and got[0].sum() > 0 and got[1].sum() > 0
                assert int(np.nonzero(got)[1].max()) == 5                # sites at 0-5 edits
            if name in ("general", "host-hits"):
                assert tm["binned_lanes"] == 0
            if name == "three-ranges":
                assert tm["lanes"] == 3
            if name == "per-contig":
                assert tm["contig_passes"] == 5
            assert np.array_equal(got, first), name
            for k in env:
                monkeypatch.delenv(k)
        # -O 0: no device row stage (hits_supported), the host stage counts
        p0 = C.make_params(max_gaps_between_guide_and_pam=2, max_overlap=0)
        got = ctx.search_counts(G, p0)
        want, n = text_table(C, ctx, G, p0, got.shape)
        print("-O 0 rows", n)
        assert np.array_equal(got, want) and n > 0          # (at -O 0 every two hits of a strand "overlap": removeOverlaps keeps a handful)
    finally:
        ctx.close()


def test_crowded_bin_the_general_tail_finishes(C, tmp_path, monkeypatch):
    """A bin with more alignments than its wave holds: the per-bin kernels decline and the general kernels finish in counts mode from
    the same raw alignments, as the text path does."""
    fa, _ = genome(tmp_path, crowded=True)
    G = C.Guide(GUIDE)
    params = C.make_params(max_gaps_between_guide_and_pam=2)
    for env in ({}, {"CALITAS_CHUNKS": "2"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = C.Context(0)                    # (a fresh context: the decline is found, not remembered)
        ctx.set_reference_fasta(fa)
        try:
            got = ctx.search_counts(G, params)
            tm = ctx.timing()
            want, n = text_table(C, ctx, G, params, got.shape)
            print("crowded", env, "rows", n, "binned_lanes", tm["binned_lanes"], "lanes", tm["lanes"])
            assert np.array_equal(got, want) and n > 150
            assert tm["binned_lanes"] < tm["lanes"]          # a range finished on the general kernels
            again = ctx.search_counts(G, params)             # ... and the remembered decline goes there at once
            assert np.array_equal(again, want)
        finally:
            ctx.close()
        for k in env:
            monkeypatch.delenv(k)
    assert np.array_equal(want, C.counts_of_rows(oracle_rows(fa, GUIDE, g=2), want.shape))


L32 = "CTTGCCCCACAGGGCAGTAACGGTTCAATGCA"
SHAPES = [
    # (id, guide, aux, params, contig lengths, expected shape)
    ("5prime-tttv", "tttvAACCAACCAACCGGTTACGT", (), dict(d=4, p=1, g=2), (50000, 20000, 900), (2, 5, 7, 2)),
    ("pamless-d8", "GTGACTTGAAGTCTCAGTATA", (), dict(d=8), (20000, 6000), (2, 9, 12, 1)),
    ("aux-pams", "ACGTACATGCTCGATACGACGnngrrn", ("nngrrt", "nnagaaw"), dict(d=4, p=1, g=3), (50000, 20000, 900), (2, 5, 8, 2)),
    ("iupac-protospacer", "GAGAATTGNTTGAACCCRGG", (), dict(d=3), (50000, 20000, 900), (2, 4, 7, 1)),
    ("per-matrix", GUIDE, (), dict(d=5, p=1, g=2, switches=1), (50000, 20000, 900), (2, 6, 8, 2)),
    # the cheapest edit costs a third of the dearest: up to 3 d edits in a protospacer alignment
    ("costs-E3d", GUIDE, (), dict(d=4, p=1, g=2, guide_mismatch_net_cost=-100, pam_mismatch_net_cost=-260, genome_gap_net_cost=-300,
                                  guide_gap_net_cost=-300), (40000, 9000), (2, 13, 15, 2)),
    ("L32-nrg-d10-p2-g16", L32 + "nrg", (), dict(d=10, p=2, g=16), (60000, 20000, 900), (2, 11, 27, 3)),
]


@pytest.mark.parametrize("cfg", SHAPES, ids=lambda c: c[0])
def test_parameter_shapes_against_the_oracle(C, cfg, tmp_path, monkeypatch):
    cid, guide, aux, kw, lengths, shape = cfg
    step = 1000 - (len(guide) + kw.get("d", 5) + kw.get("g", 3) - 1)
    fa = synth_fasta(tmp_path, 31 + len(cid), [guide], lengths=lengths, step_hint=step)
    pk = dict(max_guide_diffs=kw.get("d", 5), max_pam_mismatches=kw.get("p", 1), max_gaps_between_guide_and_pam=kw.get("g", 3),
              eqx_by_score=(1 if kw.get("switches", 0) & 2 else 0) | (2 if kw.get("switches", 0) & 1 else 0))
    pk.update({k: v for k, v in kw.items() if k.endswith("_net_cost")})
    want_rows = oracle_rows(fa, guide, aux, **kw)
    want = C.counts_of_rows(want_rows, shape)
    assert len(want_rows) > 0
    G = C.Guide(guide, aux)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        for env in ({}, {"CALITAS_BINNED": "0"}, {"CALITAS_HOST_HITS": "1"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got = ctx.search_counts(G, C.make_params(**pk))
            print(cid, env, "rows", len(want_rows), "cells", int(np.count_nonzero(want)), "shape", got.shape, "binned_lanes", ctx.timing()["binned_lanes"])
            assert got.shape == shape, (cid, env)
            assert np.array_equal(got, want), (cid, env)
            for k in env:
                monkeypatch.delenv(k)
    finally:
        ctx.close()


def ranges_genome(tmp_path, rng):
    """test_gpu_binned's genome for window ranges: sites around cuts, a chain of tandem copies over a cut (contig b), a crowded bin
    without a chain (contig c: the general kernels then decide the stretch's owned rows), a tiny contig."""
    la, lb, lc = 61000, 45000, 30000
    ca = planted(rng, la, [(int(p), int(rng.integers(0, 4)), bool(rng.integers(0, 2))) for p in rng.integers(200, la - 200, size=40)])
    cb = bytearray(planted(rng, lb, [(int(p), int(rng.integers(0, 4)), bool(rng.integers(0, 2))) for p in rng.integers(200, lb - 200, size=20)]).encode())
    for k in range(12):
        cb[22 * STEP - 70 + 9 * k: 22 * STEP - 70 + 9 * k + len(UNIT)] = UNIT
    cc = bytearray(planted(rng, lc, [(int(p), 1, False) for p in rng.integers(200, lc - 200, size=10)]).encode())
    for k in range(110):
        cc[12000 + 30 * k: 12000 + 30 * k + len(UNIT)] = UNIT
    fa = write_fasta(str(tmp_path / "ranges.fa"), [("a", ca), ("b", cb.decode()), ("c", cc.decode()), ("d", "ACGT" * 20)])
    return fa, [la, lb, lc, 80]


@pytest.mark.parametrize("cuts", [2, 3, 8])
def test_window_ranges_add_up(C, tmp_path, monkeypatch, cuts):
    """The tables of consecutive window ranges (shard.window_partition) sum, element by element, to the whole call's table, and each is
    the table of the rows calitas_search_hits returns for that range -- on the per-bin kernels, where a crowded bin hands a stretch to
    the general kernels (owned_general_lanes), through the whole-contig fallback, and with the range cut once more into lanes."""
    from calitas_amd import shard
    fa, lengths = ranges_genome(tmp_path, np.random.default_rng(100 + cuts))
    G = C.Guide(GUIDE)
    pk = dict(max_gaps_between_guide_and_pam=2)
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        whole = ctx.search_counts(G, C.make_params(**pk))
        want, n_whole = text_table(C, ctx, G, C.make_params(**pk), whole.shape)
        assert np.array_equal(whole, want) and n_whole > 60
        parts = shard.window_partition(lengths, cuts, STEP)
        assert len(parts) == cuts
        own_general = 0
        for mode, env in (("default", {}), ("two lanes", {"CALITAS_CHUNKS": "2"}), ("general", {"CALITAS_BINNED": "0"}),
                          ("whole contigs", {"CALITAS_OWN_GENERAL_OFF": "1"})):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            total = np.zeros_like(whole)
            for first, n in parts:
                pr = C.make_params(first_window=first, n_windows=n, **pk)
                got = ctx.search_counts(G, pr)
                tm = ctx.timing()
                if mode == "default":
                    own_general += tm["owned_general_lanes"]
                assert got.shape == whole.shape
                piece, _ = text_table(C, ctx, G, pr, whole.shape)
                assert np.array_equal(got, piece), (mode, first, n)
                total += got
            print(cuts, mode, "sum", int(total.sum()), "whole", int(whole.sum()), "owned_general_lanes so far", own_general)
            assert np.array_equal(total, whole), mode
            for k in env:
                monkeypatch.delenv(k)
        assert own_general >= 1               # the stretch with contig c's crowded bin: the general kernels, owned rows only
    finally:
        ctx.close()


def test_batches(C, tmp_path, monkeypatch):
    """search_counts_batch of 6 guides equals 6 single calls: whole reference and a window range, five lanes (default), one and three."""
    from calitas_amd import shard, synth
    guides = [GUIDE] + synth.random_guides(0xC4, 5)
    fa = synth_fasta(tmp_path, 5, guides, lengths=(50000, 20000, 30000))
    G = [C.Guide(g) for g in guides]
    step = 1000 - (len(GUIDE) + 5 + 2 - 1)
    first, n = shard.window_partition([50000, 20000, 30000], 3, step)[1]
    ctx = C.Context(0)
    ctx.set_reference_fasta(fa)
    try:
        for pk in (dict(max_gaps_between_guide_and_pam=2), dict(max_gaps_between_guide_and_pam=2, first_window=first, n_windows=n)):
            params = C.make_params(**pk)
            single = [ctx.search_counts(g, params) for g in G]
            texts = [text_table(C, ctx, g, params, single[0].shape)[0] for g in G]
            assert all(np.array_equal(s, t) for s, t in zip(single, texts))
            assert sum(int(s.sum()) for s in single) > (100 if "first_window" not in pk else 10)
            for lanes in (None, "1", "3"):
                if lanes:
                    monkeypatch.setenv("CALITAS_BATCH_LANES", lanes)
                got = ctx.search_counts_batch(G, params)
                tm = ctx.timing()
                print("batch", pk.get("first_window"), lanes, [int(t.sum()) for t in got], "binned_lanes", tm["binned_lanes"])
                assert len(got) == 6 and all(np.array_equal(a, b) for a, b in zip(got, single)), (pk, lanes)
                if lanes != "1":
                    assert tm["hit_rows"] == sum(int(s.sum()) for s in single) and tm["hits_bytes"] == 0
                if lanes:
                    monkeypatch.delenv("CALITAS_BATCH_LANES")
        with pytest.raises(C.CalitasError, match="same length"):
            ctx.search_counts_batch([G[0], C.Guide("GTGACTTGAAGTCTCAGTATAnrg")], C.make_params())
    finally:
        ctx.close()


def test_counts_flag_end_to_end(C, tmp_path):
    """`python -m calitas_amd SearchReference --counts` and `calitas SearchReference --counts` write the same TSV, and it is the table
    of the hits.txt the same flags give without --counts."""
    fa, _ = genome(tmp_path, crowded=False)
    flags = ["-i", GUIDE, "-I", "g1", "-r", fa, "-g", "2", "-d", "4"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    py_out, cli_out, hits = str(tmp_path / "py.tsv"), str(tmp_path / "cli.tsv"), str(tmp_path / "hits.txt")
    subprocess.run([sys.executable, "-m", "calitas_amd", "SearchReference", "--counts", "-o", py_out] + flags, check=True, env=env, cwd=ROOT, timeout=300)
    subprocess.run([os.path.join(ROOT, "calitas_amd", "calitas"), "SearchReference", "--counts", "-o", cli_out] + flags, check=True, timeout=300)
    subprocess.run([sys.executable, "-m", "calitas_amd", "SearchReference", "-o", hits] + flags, check=True, env=env, cwd=ROOT, timeout=300)
    assert open(py_out).read() == open(cli_out).read()
    shape = (2, 5, 7, 2)
    table = C.read_counts_tsv(py_out, shape)
    assert table.sum() > 40 and np.array_equal(table, C.counts_of_rows(C.read_hits(hits), shape))
    assert open(py_out).read().splitlines()[0].split("\t") == ["guide_id", "strand", "guide_mm", "guide_gaps", "pam_mm", "hits"]
