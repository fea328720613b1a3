"""GPU tests of the microhomology score (microhomology.hip: mh_score_kernel, mh_compact_kernel behind the site kernel's two passes):
the device is held against the referee of microhomology_ref.py and, byte for byte in records and scores, against the host twin -- every
window, min_length and cut under a 3' and a 5' PAM pattern at both lane chunks, listings cut to the workgroup's edges, every per-mille
with the kept records held against find_sites_filtered's, an empty listing, repeated calls and calls interleaved with
find_sites_scored, the U path, both FindGuides tools.  Contigs of <= 3 kb; the referee's scores are computed once per model.  A window
that leaves its contig is legal input with a defined answer: no test here provokes a fault."""
import os
import subprocess
import sys

import numpy as np
import pytest

import microhomology_ref as M
import sites_ref as R
from fasta_util import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = (True, False)             # the host twin, then the device, held against the referee and so against each other
DEVICE = (False,)


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


def _open(C, monkeypatch, chunk=None):
    if chunk is None:
        monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("CALITAS_CHUNK", chunk)
    names, seqs, _ = M.the_genome()
    ctx = C.Context(0)
    ctx.set_reference(names, [s.encode() for s in seqs])
    return ctx


@pytest.mark.parametrize("chunk", [None, "512"])
@pytest.mark.parametrize("name", M.PATTERNS)
def test_the_device_against_the_referee(C, name, chunk, monkeypatch):
    """Windows of 2, 33, 60 and 64 bases and the ones that fit their contig exactly or leave it by one base, min_length 2, 3 and 8, the cut
    at either end of the protospacer and at L - 3: the three words a window takes start anywhere, on both strands."""
    ctx = _open(C, monkeypatch, chunk)
    try:
        for left, right in M.WINDOWS + M.EDGE_WINDOWS:
            for min_length in M.MIN_LENGTHS:
                for cut in M.cuts():
                    assert M.hold(C, ctx, name, M.distinct(left, right, min_length), cut, 0, BOTH if chunk is None else DEVICE) == len(M.the_sites(name))
    finally:
        ctx.close()


def test_the_planted_cases(C, monkeypatch):
    names, seqs, where = M.the_genome()
    M.check_planted(seqs, where, M.the_sites("n20_nrg"))
    ctx = _open(C, monkeypatch)
    try:
        sites, scores = ctx.find_sites_microhomology(M.N20_NRG, M.model_of(C, M.unit(32, 32)), chrom="planted")
        at = {(int(s["protospacer_start"]), s["strand"].decode()): (int(v["total_q16"]), int(v["out_of_frame_q16"])) for s, v in zip(sites, scores)}
        assert at[where["poly_g"]] == (133955584, 89391104) and at[where["total_0"]] == (0, 0) and at[where["first_plus"]] == M.UNSCORED
        for m in (M.unit(32, 32), M.unit(30, 30), M.exponential(30, 30, 3)):
            M.hold(C, ctx, "n20_nrg", m, M.CUT, 0, BOTH)
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_listings_at_the_workgroup_edges(C, n, monkeypatch):
    start, end = M.region_with("n20_nrg", 1, n)
    ctx = _open(C, monkeypatch)
    try:
        m = M.exponential(30, 30)
        assert M.hold(C, ctx, "n20_nrg", m, M.CUT, 0, BOTH, chrom=1, start=start, end=end) == n
        for permille in M.PERMILLES[1:]:
            assert M.hold(C, ctx, "n20_nrg", m, M.CUT, permille, BOTH, chrom=1, start=start, end=end) <= n
    finally:
        ctx.close()


@pytest.mark.parametrize("permille", M.PERMILLES)
def test_thresholds(C, permille, monkeypatch):
    """Every per-mille under three models; the records kept are find_sites_filtered's, filtered on the host by the device's own scores."""
    ctx = _open(C, monkeypatch)
    try:
        listing = ctx.find_sites(M.N20_NRG)
        for m in (M.unit(32, 32), M.exponential(30, 30, 3), M.distinct(30, 30, 8), M.model(30, 30, 2, [0] + [1] * 5 + [0] * 53)):
            n = M.hold(C, ctx, "n20_nrg", m, M.CUT, permille, BOTH)
            _, every = ctx.find_sites_microhomology(M.N20_NRG, M.model_of(C, m), M.CUT, 0)
            keep = [i for i in range(len(listing)) if M.kept((int(every[i]["total_q16"]), int(every[i]["out_of_frame_q16"])), permille)]
            kept, _ = ctx.find_sites_microhomology(M.N20_NRG, M.model_of(C, m), M.CUT, permille)
            assert kept.tobytes() == listing[keep].tobytes() and len(keep) == n
            assert (n == len(listing)) == (permille == 0)
    finally:
        ctx.close()


def test_an_empty_listing_and_repeated_calls(C, monkeypatch):
    ctx = _open(C, monkeypatch)
    try:
        m = M.exponential(30, 30)
        model = M.model_of(C, m)
        for permille in (0, 667):
            sites, scores = ctx.find_sites_microhomology(M.N20_NRG, model, M.CUT, permille, chrom=1, start=10, end=12)      # before any buffer exists
            assert len(sites) == 0 == len(scores)
            assert M.hold(C, ctx, "n20_nrg", m, M.CUT, permille, BOTH, chrom=1, start=10, end=12) == 0
        for permille in (0, 667):
            first = ctx.find_sites_microhomology(M.N20_NRG, model, M.CUT, permille)
            again = ctx.find_sites_microhomology(M.N20_NRG, model, M.CUT, permille)
            assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and len(first[0]) > 100
            parts = [ctx.find_sites_microhomology(M.N20_NRG, model, M.CUT, permille, chrom=i) for i in range(3)]
            assert np.concatenate([p[0] for p in parts]).tobytes() == first[0].tobytes()
            assert np.concatenate([p[1] for p in parts]).tobytes() == first[1].tobytes()
            assert ctx.find_sites_microhomology(M.N20_NRG, model, M.CUT, permille, chrom=1, start=10, end=12)[1].shape == (0,)    # ... and after
    finally:
        ctx.close()


def test_interleaved_with_the_other_site_calls(C, monkeypatch):
    """find_sites_microhomology, find_sites_scored, find_sites and count_copies share a context's buffers."""
    ctx = _open(C, monkeypatch)
    try:
        activity = C.ActivityModel.read(os.path.join(ROOT, "models", "example_activity30.tsv"))
        m1, m2 = M.exponential(30, 30), M.distinct(32, 32, 3)
        want = ctx.find_sites_scored(M.N20_NRG, activity, host=True)
        for _ in range(2):
            M.hold(C, ctx, "n20_nrg", m1, M.CUT, 667, DEVICE)
            got = ctx.find_sites_scored(M.N20_NRG, activity)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
            M.hold(C, ctx, "n20_nrg", m2, M.CUT, 0, DEVICE)
            assert ctx.find_sites(M.N20_NRG).tobytes() == R.as_records(M.the_sites("n20_nrg"), C.aligner.SITE_DTYPE).tobytes()
            M.hold(C, ctx, "tttv_n20", m2, 18, 1, DEVICE)
            queries = [R.FIXED, "ACGTACGTACGTACGTACGT"]
            assert ctx.count_copies(M.N20_NRG, queries).tolist() == ctx.count_copies(M.N20_NRG, queries, host=True).tolist()
    finally:
        ctx.close()


def test_the_u_path(C, monkeypatch):
    """A U in a window is an exception base to the kernel: the host scores the window; a U in a footprint is a site the site kernel does
    not see: the host lists and scores it; a threshold applies to both."""
    names, seqs, where = M.the_genome()
    ctx = _open(C, monkeypatch)
    try:
        for m in (M.exponential(30, 30), M.distinct(32, 1, 2), M.distinct(5, 5, 2)):
            scores = M.the_scores("n20_nrg", M.CUT, m, 1, 1400, 1750)
            sites = M.the_sites("n20_nrg", 1, 1400, 1750)
            at = {(s[1], s[3]): v for s, v in zip(sites, scores)}
            assert at[where["u_flank"]] != M.UNSCORED != at[where["u_foot"]]
            for permille in (0, 1, 667):
                M.hold(C, ctx, "n20_nrg", m, M.CUT, permille, BOTH, chrom=1, start=1400, end=1750)
        got = ctx.find_sites_microhomology(M.N20_NRG, M.model_of(C, M.exponential(30, 30)), chrom=1, start=1400, end=1750)
        have = {(int(s["protospacer_start"]), s["strand"].decode()) for s in got[0]}
        assert where["u_flank"] in have and where["u_foot"] in have
    finally:
        ctx.close()


def test_errors_in_their_order(C, monkeypatch):
    ctx = _open(C, monkeypatch)
    try:
        M.hold_errors(C, ctx, False)
        M.hold_errors(C, ctx, True)
    finally:
        ctx.close()


def test_both_tools(C, tmp_path, monkeypatch):
    monkeypatch.delenv("CALITAS_CHUNK", raising=False)
    names, seqs, _ = M.the_genome()
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    binary = os.path.join(ROOT, "calitas_amd", "calitas")
    env = dict(os.environ, PYTHONPATH=ROOT)
    model_path = str(tmp_path / "mh.tsv")
    M.model_of(C, M.exponential(30, 30, 3)).write(model_path)
    activity = os.path.join(ROOT, "models", "example_activity30.tsv")

    def run(tool, flags):
        out = str(tmp_path / (tool + ".tsv"))
        head = [sys.executable, "-m", "calitas_amd"] if tool == "py" else [binary]
        subprocess.check_call(head + ["FindGuides", "-r", fa, "-o", out, "-i", M.N20_NRG] + flags, env=env, cwd=ROOT, stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
        return open(out, "rb").read()

    for flags in (["--microhomology", model_path], ["--microhomology", model_path, "--min-out-of-frame", "67", "--copies"],
                  ["--microhomology", model_path, "--activity", activity, "--min-out-of-frame", "50", "--mh-cut", "10", "-c", "planted"]):
        a, b, host = run("py", flags), run("cc", flags), run("cc", flags + ["--device", "-1"])
        assert a == b == host and len(a.splitlines()) > 10
