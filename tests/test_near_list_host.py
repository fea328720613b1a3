"""CPU tests of the near-copies listing: calitas_list_near_host (the host twin of the listing kernels, on a host-only context) against
the referee of near_list_ref.py, byte for byte -- the planted genome with and without a model, the seam genomes, the sweep over every
protospacer length, the limit, the contended contig, interleaved calls, the errors in their order, the contract function, the merge
rules -- and both FindGuides tools with --near-list on the host twin (--device -1).  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import copies_ref as X
import near_list_ref as T
import near_score_ref as S
import site_filter_ref as F
import sites_ref as R
from fasta_util import write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N20_NRG = "NNNNNNNNNNNNNNNNNNNNnrg"
HOST = (True,)


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


def _open(C, names, seqs):
    ctx = C.Context(-1)
    ctx.set_reference(names, [s.encode() for s in seqs])
    return ctx


@pytest.fixture(scope="module")
def planted(C):
    names, seqs, expect = S.planted()
    ctx = _open(C, names, seqs)
    yield ctx, seqs, expect, {}
    ctx.close()


def _sites(planted, name):
    _, seqs, _, done = planted
    if name not in done:
        done[name] = R.brute_sites(seqs, *X.PATTERNS[name])
    return done[name]


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("M", [1, 2, 3])
@pytest.mark.parametrize("name, L", T.PLANTED)
def test_the_planted_genome(C, planted, name, L, M, weighted):
    ctx, seqs, expect, _ = planted
    T.hold_planted(C, ctx, name, L, M, weighted, HOST, seqs, expect, _sites(planted, name))


def test_the_limit(C, planted):
    ctx, seqs, expect, _ = planted
    assert T.hold_limit(C, ctx, HOST, seqs, expect, _sites(planted, "n20_nrg")) >= 1


def test_the_contract_function(C, planted):
    _, seqs, expect, _ = planted
    _, queries, table = T.planted_case("n20_nrg", 20, seqs, expect, _sites(planted, "n20_nrg"))
    T.check_contract_function(C, table, queries[:25], 3, S.distinct_mismatch(20))
    T.check_contract_function(C, table, queries[:25], 2, None)
    with pytest.raises(ValueError):
        C.near_hits_of("ACGT", [(0, 0, "+", 0, "ACG")], 1)


@pytest.mark.parametrize("lane", [64, 512])
def test_the_seam_genomes(C, lane):
    names, seqs = R.gpu_genome(1234 + lane, lane * 256, lane)
    ctx = _open(C, names, seqs)
    try:
        T.hold_seams(C, ctx, "n20_nrg", seqs, R.brute_sites(seqs, *X.PATTERNS["n20_nrg"]), HOST)
    finally:
        ctx.close()


@pytest.mark.parametrize("L", F.SWEEP_LENGTHS)
def test_sweep_of_protospacer_lengths(C, L):
    names, seqs = F.sweep_genome()
    ctx = _open(C, names, seqs)
    try:
        T.hold_sweep(C, ctx, L, seqs, F.listing(L).sites, HOST)
    finally:
        ctx.close()


def test_a_contended_cursor(C):
    names, seqs, x, run = T.contended_genome()
    ctx = _open(C, names, seqs)
    try:
        T.hold_contended(C, ctx, HOST, seqs, x, run, R.brute_sites(seqs, *X.PATTERNS["n20_nrg"]))
    finally:
        ctx.close()


def test_interleaved_calls(C):
    seqs = [X.random_contig()[1][0][:20000]]
    ctx = _open(C, ["r"], seqs)
    try:
        T.hold_reused(C, ctx, seqs, True)
    finally:
        ctx.close()


def test_errors(C, planted):
    ctx = planted[0]
    T.hold_errors(C, ctx, True)
    with pytest.raises(C.CalitasError) as e:
        ctx.list_near(N20_NRG, ["ACGT" * 5], 1)                          # the device call on a host-only context
    assert e.value.code == C._lib.ENODEV and "no CPU fallback" in str(e.value)


def test_merge_rules(C):
    def part(near, contig, starts):
        hits = np.zeros(len(starts), dtype=T.DTYPE)
        hits["contig_index"], hits["protospacer_start"], hits["strand"], hits["score_q32"] = contig, starts, b"+", T.ONE
        return C.NearList(np.array(near, dtype=np.uint64), np.array([0, len(starts), len(starts)], dtype=np.uint64), hits, 3, 20)

    a, b = part([[1, 1], [4, 0]], 0, [5, 9]), part([[0, 1], [0, 0]], 1, [2])
    c = b.merge(a)
    assert c.near.tolist() == [[1, 2], [4, 0]] and c.offsets.tolist() == [0, 3, 3] and c == a.merge(b) and c != a
    assert [(int(h["contig_index"]), int(h["protospacer_start"])) for h in c.of(0)] == [(0, 5), (0, 9), (1, 2)]
    assert c.listed(0) and not c.listed(1) and not a.listed(1) and len(c.of(1)) == 0
    d = a.merge(part([[1, 1], [0, 0]], 1, [2, 7]))                       # together over the limit: nothing is listed
    assert d.near.tolist() == [[2, 2], [4, 0]] and d.offsets.tolist() == [0, 0, 0] and len(d.hits) == 0
    with pytest.raises(ValueError):
        a.merge(C.NearList(a.near, a.offsets, a.hits, 4, 20))


def test_both_tools_on_the_host_twin(C, tmp_path):
    names, seqs = R.host_genome()
    ctx = _open(C, names, seqs)
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    binary = os.path.join(ROOT, "calitas_amd", "calitas")
    env = dict(os.environ, PYTHONPATH=ROOT)
    mismatch = S.distinct_mismatch(20)
    model_path = str(tmp_path / "model.tsv")
    S.model_of(C, mismatch).write(model_path)
    rows = C.find_guides(ctx, N20_NRG, chrom="chrA", start=350, end=1100, host=True)
    listing = C.guide_near_list(ctx, N20_NRG, rows, 2, S.model_of(C, mismatch), limit=1000, host=True)
    ctx.close()
    table = T.table_of(R.brute_sites(seqs, *X.PATTERNS["n20_nrg"]), seqs)
    pairs = [(r.guide_id, r.guide[:20]) for r in rows]
    want = T.tsv_of(pairs, names, table, 2, mismatch, 1000)
    assert C.near_list_tsv(rows, names, listing) == want and len(want.splitlines()) > len(rows)
    region = ["-i", N20_NRG, "-c", "chrA", "-s", "350", "-e", "1100"]

    def run(tool, flags):
        out, listed = str(tmp_path / (tool + ".tsv")), str(tmp_path / (tool + ".list.tsv"))
        head = [sys.executable, "-m", "calitas_amd"] if tool == "py" else [binary]
        flags = [listed if f == "LIST" else f for f in flags]
        subprocess.check_call(head + ["FindGuides", "-r", fa, "-o", out, "--device", "-1"] + region + flags, env=env, cwd=ROOT,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out, "rb").read(), (open(listed, "rb").read() if "LIST" in flags or listed in flags else None)

    # the guides table is what it is without the flag; the list is the referee's, from both tools
    base = run("py", ["--near-copies", "2", "--near-scores", model_path])[0]
    flags = ["--near-copies", "2", "--near-scores", model_path, "--near-list", "LIST"]
    a, b = run("py", flags), run("cc", flags)
    assert a == b and a[0] == base and a[1].decode() == want
    # without a model every score is 1.0
    plain = T.tsv_of(pairs, names, table, 2, None, 1000)
    flags = ["--near-copies", "2", "--near-list", "LIST"]
    a, b = run("py", flags), run("cc", flags)
    assert a == b and a[0] == run("py", ["--near-copies", "2"])[0] and a[1].decode() == plain and plain != want
    # a limit some guides exceed, and a row filter: the kept rows' guides alone, those over the limit without a line
    near = [sum(row) for row in listing.near.tolist()]
    sums = sorted(set(near))
    assert len(sums) >= 3
    limit, most = sums[0], sums[1]
    kept = [p for p, n in zip(pairs, near) if n <= most]
    assert 0 < len(kept) < len(pairs)
    flags = ["--near-copies", "2", "--max-near-copies", str(most), "--near-list", "LIST", "--near-list-limit", str(limit)]
    a, b = run("py", flags), run("cc", flags)
    assert a == b and a[1].decode() == T.tsv_of(kept, names, table, 2, None, limit)
    assert {ln.split("\t")[0] for ln in a[1].decode().splitlines()[1:]} == {g for (g, _), n in zip(pairs, near) if n <= limit}
    assert [ln.split("\t")[0] for ln in a[0].decode().splitlines()[1:]] == [g for g, _ in kept]
    # the flags' own rules
    for bad in (["--near-list", "LIST"], ["--near-copies", "2", "--near-list-limit", "5"], ["--near-copies", "2", "--near-list", "LIST", "--near-list-limit", "0"],
                ["--near-copies", "2", "--near-list", "LIST", "--near-list-limit", "4097"]):
        for tool in ("py", "cc"):
            with pytest.raises(subprocess.CalledProcessError):
                run(tool, bad)
