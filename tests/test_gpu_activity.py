"""GPU tests of the on-target activity score (activity.hip: activity_score_kernel, activity_compact_kernel behind the site kernel's two
passes): the device is held against the referee of activity_ref.py and, byte for byte in records and scores, against the host twin --
the site tests' seam genomes at both lane chunks with windows of 30 and 64 bases, the planted contig under every model, the sweep over
protospacer lengths and flank corners, compaction across workgroups and contigs, a site filter with a threshold, the call without
blocks, a repeated call, calls interleaved with the other site calls on one context, the errors, both FindGuides tools.  Contigs of
<= 60 kb; a genome's brute force is computed once.  A window that leaves its contig is legal input with a defined answer: no test here
provokes a fault."""
import os
import subprocess
import sys

import numpy as np
import pytest

import activity_ref as A
import site_filter_ref as F
import sites_ref as R
from fasta_util import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = (True, False)             # the host twin, then the device, held against the referee and so against each other
CHUNKS = {None: 64, "512": 512}  # CALITAS_CHUNK -> the lane chunk it gives, as in test_gpu_sites.py


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


def _host_genome(name):
    if "genome" not in _cache:
        _cache["genome"] = A.host_contigs() + ({},)
    names, seqs, where, index, done = _cache["genome"]
    if name not in done:
        done[name] = R.brute_sites(seqs, *R.PATTERNS[name])
    return names, seqs, where, index, done[name]


@pytest.mark.parametrize("which", [None, "512"])
def test_the_seam_genomes(C, which, monkeypatch):
    """Sites at every word offset 1 .. 47 on both strands, across lane chunks, workgroups and scan tiles: the three words a window
    takes start anywhere.  W = 30, and W = 64 with both flanks at their limit (L = 32 through the PAM-less N x 32)."""
    lane = CHUNKS[which]
    names, seqs = R.gpu_genome(1234 + lane, lane * 256, lane)
    assert all(len(s) <= 60000 for s in seqs)
    ctx = _open(C, names, seqs, monkeypatch, which)
    try:
        sites = R.brute_sites(seqs, *R.PATTERNS["n20_nrg"])
        m, floors = A.thresholds(seqs, sites, A.distinct(20, 4, 6))
        for what in ("all", "half", "exact"):
            A.hold(C, ctx, seqs, A.N20_NRG, sites, m, floors[what], BOTH, floors.scores)
        m = A.distinct(32, 16, 16)
        for start, end, halve in ((0, 3300, False), (5900, 8500, True)):             # the word offsets; a lane chunk's and a workgroup's edge
            wide = R.brute_sites(seqs[:1], "N" * 32, [], False, start=start, end=end)
            scores = A.scores_of(seqs, wide, m)
            floor = sorted(s for s in scores if s != A.NONE)[len(wide) // 2] if halve else None
            assert A.hold(C, ctx, seqs, "N" * 32, wide, m, floor, BOTH, scores, chrom=0, start=start, end=end) > 1000
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["n20_nrg", "n20_nngrrt_nrg", "tttv_n20"])
def test_the_planted_contig_under_every_model(C, name, monkeypatch):
    """Windows that touch a contig's first and last base and ones a base beyond, an N, an R, an n, a U in the flank and in the footprint,
    soft-masked bases; with two PAMs, the record the kernel has beside a U in place of the longer PAM's."""
    names, seqs, where, index, sites = _host_genome(name)
    if name != "tttv_n20":
        A.check_planted(seqs, index, where, sites, A.distinct(20, 4, 6))
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        for model, m in A.models(20, 4, 6).items():
            assert A.hold(C, ctx, seqs, A.pattern_of(C, name), sites, m, None, BOTH) == len(sites)
        m, floors = A.thresholds(seqs, sites, A.distinct(20, 4, 6))
        for what in ("exact", "half", "tenth", "above"):
            A.hold(C, ctx, seqs, A.pattern_of(C, name), sites, m, floors[what], BOTH)
        # the nrg record beside the U of the nngrrt PAM is scored by the kernel when the window ends before the U, left to the host otherwise
        for down in (0, 4, 5, 16):
            m, floors = A.thresholds(seqs, sites, A.distinct(20, 3, down))
            for what in ("all", "half"):
                A.hold(C, ctx, seqs, A.pattern_of(C, name), sites, m, floors[what], BOTH)
    finally:
        ctx.close()


@pytest.mark.parametrize("L", range(1, 33))
def test_sweep_of_lengths_and_flank_corners(C, L, monkeypatch):
    names, seqs = A.sweep_contigs()
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        sites = A.pamless_sites(seqs, L)
        for up, down in A.CORNERS:
            m, floors = A.thresholds(seqs, sites, A.distinct(L, up, down))
            for what in ("all", "exact"):
                A.hold(C, ctx, seqs, "N" * L, sites, m, floors[what], BOTH)
        for model in ("extremes_plus", "extremes_minus"):
            A.hold(C, ctx, seqs, "N" * L, sites, A.models(L, 16, 16)[model], 0, BOTH)
    finally:
        ctx.close()


def test_compaction_across_workgroups_and_contigs(C, monkeypatch):
    names, seqs = R.many_contigs(77, 40)
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        sites = R.brute_sites(seqs, *R.PATTERNS["n20_nrg"])
        assert len(sites) > 8 * 256 and len({s[0] for s in sites}) >= 30
        m, floors = A.thresholds(seqs, sites, A.distinct(20, 4, 6))
        kept = {what: A.hold(C, ctx, seqs, A.N20_NRG, sites, m, floor, BOTH, floors.scores) for what, floor in floors.items()}
        assert kept["above"] == 0 and 0.3 * len(sites) < kept["half"] < 0.7 * len(sites)
        assert A.hold(C, ctx, seqs, A.N20_NRG, sites, m, floors["exact"] + 1, BOTH) < kept["exact"] < A.hold(C, ctx, seqs, A.N20_NRG, sites, m, floors["exact"] - 1, BOTH)
        # the call without blocks, and a second call with the same bytes
        model = A.model_of(C, m)
        for what in ("all", "half", "above"):
            assert ctx.count_sites_scored(A.N20_NRG, model, floors[what]) == kept[what]
        first = ctx.find_sites_scored(A.N20_NRG, model, floors["half"])
        again = ctx.find_sites_scored(A.N20_NRG, model, floors["half"])
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and len(first[1]) == kept["half"]
    finally:
        ctx.close()


@pytest.mark.parametrize("flt", ["gc40_60", "g3"])
def test_a_site_filter_with_a_threshold(C, flt, monkeypatch):
    names, seqs, _, _, sites = _host_genome("n20_nrg")
    rules = dict(F.EXTRA, gc40_60=dict(zip(("gc_min", "gc_max"), F.percent(20, 40, 60))))[flt]
    kept = F.keep(sites, seqs, **rules)
    assert 0 < len(kept) < len(sites)
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        m, floors = A.thresholds(seqs, kept, A.distinct(20, 4, 6))
        for what in ("all", "exact", "half"):
            A.hold(C, ctx, seqs, A.N20_NRG, kept, m, floors[what], BOTH, filter=C.SiteFilter(**rules))
    finally:
        ctx.close()


def test_interleaved_calls_on_one_context(C, monkeypatch):
    """find_sites_scored, count_copies, find_sites, list_near and find_sites_scored with another model share a context's buffers; the
    per-contig results concatenate to the whole."""
    names, seqs, _, _, sites = _host_genome("n20_nrg")
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        m1, floors1 = A.thresholds(seqs, sites, A.distinct(20, 4, 6))
        m2 = A.distinct(20, 16, 0, seed=3)
        A.hold(C, ctx, seqs, A.N20_NRG, sites, m1, floors1["half"], (False,))
        queries = [R.FIXED, "ACGTACGTACGTACGTACGT"]
        assert ctx.count_copies(A.N20_NRG, queries).tolist() == ctx.count_copies(A.N20_NRG, queries, host=True).tolist()
        assert ctx.find_sites(A.N20_NRG).tobytes() == R.as_records(sites, C.aligner.SITE_DTYPE).tobytes()
        near, twin = ctx.list_near(A.N20_NRG, queries, 2), ctx.list_near(A.N20_NRG, queries, 2, host=True)
        assert near.hits.tobytes() == twin.hits.tobytes() and len(near.hits) > 0
        A.hold(C, ctx, seqs, A.N20_NRG, sites, m2, None, (False,))
        for floor in (None, floors1["half"]):
            parts = [ctx.find_sites_scored(A.N20_NRG, A.model_of(C, m1), floor, chrom=i) for i in range(len(names))]
            whole = ctx.find_sites_scored(A.N20_NRG, A.model_of(C, m1), floor)
            assert np.concatenate([p[0] for p in parts]).tobytes() == whole[0].tobytes()
            assert np.concatenate([p[1] for p in parts]).tobytes() == whole[1].tobytes()
    finally:
        ctx.close()


def test_errors_in_their_order(C, monkeypatch):
    names, seqs, _, _, _ = _host_genome("n20_nrg")
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        A.hold_errors(C, ctx, False)
        A.hold_errors(C, ctx, True)
    finally:
        ctx.close()


def test_both_tools(C, tmp_path, monkeypatch):
    monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    names, seqs, _, index, sites = _host_genome("n20_nrg")
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    binary = os.path.join(ROOT, "calitas_amd", "calitas")
    env = dict(os.environ, PYTHONPATH=ROOT)
    m, floors = A.thresholds(seqs, sites, A.distinct(20, 4, 6))
    model_path = str(tmp_path / "activity.tsv")
    A.model_of(C, m).write(model_path)

    def run(tool, flags):
        out = str(tmp_path / (tool + ".tsv"))
        head = [sys.executable, "-m", "calitas_amd"] if tool == "py" else [binary]
        subprocess.check_call(head + ["FindGuides", "-r", fa, "-o", out, "-i", A.N20_NRG] + flags, env=env, cwd=ROOT, stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
        return open(out, "rb").read()

    for flags in (["--activity", model_path], ["--activity", model_path, "--min-activity", A.decimal_of(floors["half"])],
                  ["--activity", model_path, "--min-activity", A.decimal_of(floors["exact"]), "--copies", "-c", "planted"]):
        a, b, host = run("py", flags), run("cc", flags), run("cc", flags + ["--device", "-1"])
        assert a == b == host and len(a.splitlines()) > 10
