"""GPU tests of the near-copies listing (sites_kernel's KEYS_NEAR_LIST ending and near_order_kernel): device, host twin and the referee
of near_list_ref.py return the same bytes -- the planted genome at M = 1, 2, 3 with and without a model, the site tests' seam genomes at
both lane chunks and with five segments per workgroup, the sweep over every protospacer length, a limit that one query meets and another
exceeds by one, 720 copies on one cursor, list_near / score_near / count_near / count_copies interleaved on one context, the errors, both
FindGuides tools.  Contigs of <= 60 kb; a genome's brute force is computed once."""
import os
import subprocess
import sys

import pytest

import copies_ref as X
import near_list_ref as T
import near_score_ref as S
import site_filter_ref as F
import sites_ref as R
from fasta_util import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N20_NRG = "NNNNNNNNNNNNNNNNNNNNnrg"
BOTH = (True, False)             # the host twin, then the device, held against the referee and so against each other
# CALITAS_CHUNK -> the lane chunk it gives, as in test_gpu_sites.py
CHUNKS = {None: 64, "512": 512}


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


def _open(C, names, seqs, monkeypatch, chunk=None):
    if chunk is None:
        monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("CALITAS_CHUNK", chunk)
    ctx = C.Context(0)
    ctx.set_reference(names, [s.encode() for s in seqs])
    return ctx


_cache = {}


def _planted(name=None):
    if "planted" not in _cache:
        _cache["planted"] = S.planted() + ({},)
    names, seqs, expect, done = _cache["planted"]
    if name is not None and name not in done:
        done[name] = R.brute_sites(seqs, *X.PATTERNS[name])
    return names, seqs, expect, done.get(name)


@pytest.mark.parametrize("name, L", T.PLANTED)
def test_the_planted_genome(C, name, L, monkeypatch):
    """'-' sites, each PAM of two, the 5' PAM, N x 32 with the keys 0 and all ones, U / u sites (the host's patch of the stretch),
    duplicated queries, two queries one substitution apart."""
    names, seqs, expect, sites = _planted(name)
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        for M in (1, 2, 3):
            for weighted in (True, False):
                T.hold_planted(C, ctx, name, L, M, weighted, BOTH, seqs, expect, sites)
    finally:
        ctx.close()


def test_the_limit(C, monkeypatch):
    names, seqs, expect, sites = _planted("n20_nrg")
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        print("limit", T.hold_limit(C, ctx, BOTH, seqs, expect, sites))
    finally:
        ctx.close()


@pytest.mark.parametrize("which", [None, "512"])
def test_the_seam_genomes(C, which, monkeypatch):
    # (512 also with five segments per workgroup, as a genome-sized call has several)
    if which == "512":
        monkeypatch.setenv("CALITAS_SITES_SEGS", "5")
    else:
        monkeypatch.delenv("CALITAS_SITES_SEGS", raising=False)
    lane = CHUNKS[which]
    names, seqs = R.gpu_genome(1234 + lane, lane * 256, lane)
    assert all(len(s) <= 60000 for s in seqs)
    ctx = _open(C, names, seqs, monkeypatch, which)
    try:
        T.hold_seams(C, ctx, "n20_nrg", seqs, R.brute_sites(seqs, *X.PATTERNS["n20_nrg"]), BOTH)
    finally:
        ctx.close()


@pytest.mark.parametrize("L", F.SWEEP_LENGTHS)
def test_sweep_of_protospacer_lengths(C, L, monkeypatch):
    names, seqs = F.sweep_genome()
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        T.hold_sweep(C, ctx, L, seqs, F.listing(L).sites, BOTH)
    finally:
        ctx.close()


def test_a_contended_cursor(C, monkeypatch):
    """Many waves and workgroups take slots from one cursor, and the stretch is longer than a workgroup; a key with more copies than the
    largest limit lists nothing."""
    names, seqs, x, run = T.contended_genome()
    assert len(seqs[0]) <= 60000
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        got = T.hold_contended(C, ctx, BOTH, seqs, x, run, R.brute_sites(seqs, *X.PATTERNS["n20_nrg"]))
        print("rows", got.near.tolist(), "records", len(got.hits))
    finally:
        ctx.close()


def test_interleaved_calls_reuse_the_buffers(C, monkeypatch):
    seqs = [X.random_contig()[1][0][:20000]]
    ctx = _open(C, ["r"], seqs, monkeypatch)
    try:
        T.hold_reused(C, ctx, seqs, False)
    finally:
        ctx.close()


def test_errors(C, monkeypatch):
    names, seqs, _, _ = _planted()
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        T.hold_errors(C, ctx, False)
    finally:
        ctx.close()


def test_both_tools(C, tmp_path, monkeypatch):
    monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    names, seqs = R.host_genome()
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    binary = os.path.join(ROOT, "calitas_amd", "calitas")
    env = dict(os.environ, PYTHONPATH=ROOT)
    mismatch = S.distinct_mismatch(20)
    model_path = str(tmp_path / "model.tsv")
    S.model_of(C, mismatch).write(model_path)
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        rows = C.find_guides(ctx, N20_NRG, chrom="chrA", start=350, end=1100)
        listing = C.guide_near_list(ctx, N20_NRG, rows, 2, S.model_of(C, mismatch), limit=1000)
        scored = C.guide_near_scores(ctx, N20_NRG, rows, 2, S.model_of(C, mismatch))
    finally:
        ctx.close()
    table = T.table_of(R.brute_sites(seqs, *X.PATTERNS["n20_nrg"]), seqs)
    want = T.tsv_of([(r.guide_id, r.guide[:20]) for r in rows], names, table, 2, mismatch, 1000)
    assert C.near_list_tsv(rows, names, listing) == want and len(want.splitlines()) > len(rows)
    region = ["-i", N20_NRG, "-c", "chrA", "-s", "350", "-e", "1100"]

    def run(tool, flags, listed=None):
        out = str(tmp_path / (tool + ".tsv"))
        head = [sys.executable, "-m", "calitas_amd"] if tool == "py" else [binary]
        more = ["--near-list", str(tmp_path / listed)] if listed else []
        subprocess.check_call(head + ["FindGuides", "-r", fa, "-o", out] + region + flags + more, env=env, cwd=ROOT, stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
        return open(out, "rb").read(), (open(str(tmp_path / listed), "rb").read() if listed else None)

    flags = ["--near-copies", "2", "--near-scores", model_path]
    a, b, host = run("py", flags, "py.list"), run("cc", flags, "cc.list"), run("py", flags + ["--device", "-1"], "host.list")
    assert a == b == host and a[1].decode() == want
    assert a[0].decode() == C.guides_tsv(rows, near=scored.near, near_scores=scored) and a[0] == run("cc", flags)[0]
