"""GPU tests of the scored near-copies call (sites_kernel's KEYS_NEAR_SCORE ending): device, host twin and the referee of
near_score_ref.py return the same integers -- the planted genome under the distinct and the zeros model, the site tests' seam genomes
at both lane chunks, the sweep over every protospacer length, the uniform invariant on a few hot counters, score_near / count_near /
count_copies interleaved on one context, the errors, both FindGuides tools -- and the search's scores of a guide whose hits are all
ungapped with a clean PAM equal its near scores.  Contigs of <= 60 kb; a genome's brute force is computed once."""
import os
import subprocess
import sys

import numpy as np
import pytest

import copies_ref as X
import near_score_ref as S
import site_filter_ref as F
import sites_ref as R
from fasta_util import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N20_NRG = "NNNNNNNNNNNNNNNNNNNNnrg"
BOTH = (True, False)             # the host twin, then the device, held against each other
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


def _planted():
    if "planted" not in _cache:
        _cache["planted"] = S.planted() + ({},)
    return _cache["planted"]


@pytest.mark.parametrize("name, L", S.PLANTED)
def test_the_planted_genome(C, name, L, monkeypatch):
    """M = 1, 2, 3 under both models: substitutions at position 0 and L - 1, around every piece boundary and in no piece, on '-', next
    to each PAM, with U / u (the host's correction of counts, sums and maxima), N x 32 with the keys 0 and all ones."""
    names, seqs, expect, done = _planted()
    if name not in done:
        done[name] = R.brute_sites(seqs, *X.PATTERNS[name])
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        for M in (1, 2, 3):
            for kind in ("distinct", "zeros"):
                S.hold_planted(C, ctx, name, L, M, kind, BOTH, seqs, expect, sites=done[name])
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
        S.hold_seams(C, ctx, "n20_nrg", seqs, R.brute_sites(seqs, *X.PATTERNS["n20_nrg"]), BOTH)
    finally:
        ctx.close()


@pytest.mark.parametrize("L", F.SWEEP_LENGTHS)
def test_sweep_of_protospacer_lengths(C, L, monkeypatch):
    names, seqs = F.sweep_genome()
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        S.hold_sweep(C, ctx, L, seqs, F.listing(L).sites, BOTH)
    finally:
        ctx.close()


def test_the_uniform_invariant_on_hot_counters(C, monkeypatch):
    names, seqs = X.random_contig()
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        got = S.hold_uniform(C, ctx, BOTH)
        print("sites", int(got.near[:, 0].sum()), "adds per counter column", got.near.sum(axis=0).tolist())
    finally:
        ctx.close()


def test_interleaved_calls_reuse_the_buffers(C, monkeypatch):
    seqs = [X.random_contig()[1][0][:20000]]
    ctx = _open(C, ["r"], seqs, monkeypatch)
    try:
        S.hold_reused(C, ctx, seqs, False)
    finally:
        ctx.close()


def test_errors(C, monkeypatch):
    names, seqs, _, _ = _planted()
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        S.hold_errors(C, ctx, False)
    finally:
        ctx.close()


def test_the_search_scores_of_an_ungapped_guide(C, monkeypatch):
    """A guide whose hits at d = 2, p = 0, g = 0 are all substitution-only with a clean PAM: search_scores and the near call answer the
    same question, and so do the reference's rows through scores_of_rows."""
    names, seqs, guide = S.search_genome(5)
    ctx = _open(C, names, seqs, monkeypatch)
    try:
        mismatch = S.distinct_mismatch(20)
        counts = X.count_keys(R.brute_sites(seqs, "N" * 20, ["ngg"], False), seqs, 20, False)
        got, _ = S.hold(C, ctx, "N" * 20 + "ngg", [guide], 2, mismatch, counts, BOTH)
        want = S.hold_search_rows(C, names, seqs, guide, got, mismatch)
        params = C.make_params(max_guide_diffs=2, max_pam_mismatches=0, max_gaps_between_guide_and_pam=0)
        found = ctx.search_scores(C.Guide(guide + "ngg"), params, S.model_of(C, mismatch))
        print(found, got.near.tolist(), got.sum_q32.tolist(), got.max_q32.tolist())
        assert (found.rows, found.perfect, found.sum_q32, found.max_q32) == (want.rows, want.perfect, want.sum_q32, want.max_q32)
        assert (found.perfect, found.sum_q32, found.max_q32) == (int(got.near[0, 0]), int(got.sum_q32[0]), int(got.max_q32[0]))
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
        scored = C.guide_near_scores(ctx, N20_NRG, rows, 2, S.model_of(C, mismatch))
    finally:
        ctx.close()
    near, sums, tops, _ = S.table_for(X.copies(seqs, "n20_nrg", 20)[0], [r.guide[:20] for r in rows], 2, mismatch)
    assert (scored.near.tolist(), scored.sum_q32.tolist(), scored.max_q32.tolist()) == (near, sums, tops) and sum(sums) > 0
    region = ["-i", N20_NRG, "-c", "chrA", "-s", "350", "-e", "1100"]

    def run(tool, out, flags):
        head = [sys.executable, "-m", "calitas_amd"] if tool == "py" else [binary]
        subprocess.check_call(head + ["FindGuides", "-r", fa, "-o", out] + region + flags, env=env, cwd=ROOT, stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
        return open(out, "rb").read()

    a, b = run("py", str(tmp_path / "py0.tsv"), ["--near-copies", "2"]), run("cc", str(tmp_path / "cc0.tsv"), ["--near-copies", "2"])
    assert a == b and a.decode() == C.guides_tsv(rows, near=near)
    flags = ["--near-copies", "2", "--near-scores", model_path]
    a, b = run("py", str(tmp_path / "py1.tsv"), flags), run("cc", str(tmp_path / "cc1.tsv"), flags)
    assert a == b and a.decode() == C.guides_tsv(rows, near=near, near_scores=scored)
    assert a == run("py", str(tmp_path / "host.tsv"), flags + ["--device", "-1"])
