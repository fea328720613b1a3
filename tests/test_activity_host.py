"""CPU tests of the on-target activity score: calitas_find_sites_scored_host (the host twin of activity.hip's kernels, on a host-only
context) against the referee of activity_ref.py -- the host genome plus the planted contig under every pattern and model, the sweep
over window widths and flank corners, thresholds taken from the referee's scores, a site filter, a region that cuts footprints but not
contexts, the errors in their order -- the model file, the contract function, the guides table's columns, and both FindGuides tools
with --activity on the host twin (--device -1).  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import activity_ref as A
import site_filter_ref as F
import sites_ref as R
from fasta_util import write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
def genome(C):
    names, seqs, where, index = A.host_contigs()
    ctx = _open(C, names, seqs)
    yield ctx, names, seqs, where, index, {}
    ctx.close()


def _sites(genome, name):
    done = genome[5]
    if name not in done:
        done[name] = R.brute_sites(genome[2], *R.PATTERNS[name])
    return done[name]


def test_the_referee_on_its_planted_contig(genome):
    _, _, seqs, where, index, _ = genome
    m = A.distinct(20, 4, 6)
    for name in ("n20_nrg", "n20_nngrrt_nrg"):
        kinds = A.check_planted(seqs, index, where, _sites(genome, name), m)
        assert len(kinds) == len(where)
    A.check_sensitive(seqs, index, where, _sites(genome, "n20_nrg"), m)
    long_pam = [s for s in _sites(genome, "n20_nngrrt_nrg") if s[0] == index and s[1] == 1000 and s[3] == "+"]
    assert long_pam and long_pam[0][4] == 0 and long_pam[0][5] == 6           # nngrrt wins there, through the U


@pytest.mark.parametrize("model", A.MODEL_NAMES)
@pytest.mark.parametrize("name", A.HOST_PATTERNS)
def test_the_twin_against_the_referee(C, genome, name, model):
    ctx, _, seqs, _, _, _ = genome
    L = len(R.PATTERNS[name][0])
    m = A.models(L, 4, 6)[model]
    sites = _sites(genome, name)
    n = A.hold(C, ctx, seqs, A.pattern_of(C, name), sites, m, None, HOST)
    assert n == len(sites) > 0
    scores = A.scores_of(seqs, sites, m)
    assert A.NONE in scores and any(s != A.NONE for s in scores)
    if model.startswith("extremes"):                                         # 2 W terms of 2^20: the bound, far inside 32 bits
        W = 4 + L + 6
        assert {s for s in scores if s != A.NONE} == {(2 * W + 1) * (A.MAX_WEIGHT if model.endswith("plus") else -A.MAX_WEIGHT)}


@pytest.mark.parametrize("name", A.HOST_PATTERNS)
def test_thresholds_from_the_referee(C, genome, name):
    ctx, _, seqs, _, _, _ = genome
    sites = _sites(genome, name)
    m, floors = A.thresholds(seqs, sites, A.distinct(len(R.PATTERNS[name][0]), 4, 6))
    kept = {what: A.hold(C, ctx, seqs, A.pattern_of(C, name), sites, m, floor, HOST) for what, floor in floors.items()}
    assert kept["above"] == 0 and kept["all"] == len(sites) and 1 <= kept["exact"] <= len(sites) - 1
    assert kept["exact"] - A.hold(C, ctx, seqs, A.pattern_of(C, name), sites, m, floors["exact"] + 1, HOST) >= 1      # the site that meets it exactly
    assert A.hold(C, ctx, seqs, A.pattern_of(C, name), sites, m, floors["exact"] - 1, HOST) - kept["exact"] >= 1      # the one a point below
    # a threshold other than NONE drops the unscored sites, however low it is
    assert A.hold(C, ctx, seqs, A.pattern_of(C, name), sites, m, A.NONE + 1, HOST) == sum(1 for s in A.scores_of(seqs, sites, m) if s != A.NONE)
    assert ctx.count_sites_scored(A.pattern_of(C, name), A.model_of(C, m), floors["half"], host=True) == kept["half"]


@pytest.mark.parametrize("W, up, down, L", A.sweep_cases())
def test_sweep_of_window_widths(C, W, up, down, L):
    names, seqs = A.sweep_contigs()
    ctx = _open(C, names, seqs)
    try:
        sites = A.pamless_sites(seqs, L)
        for model in ("distinct", "extremes_plus", "extremes_minus"):
            m = A.models(L, up, down)[model]
            assert A.hold(C, ctx, seqs, "N" * L, sites, m, None, HOST) == len(sites)
        m, floors = A.thresholds(seqs, sites, A.distinct(L, up, down))
        for what in ("exact", "half", "above"):
            A.hold(C, ctx, seqs, "N" * L, sites, m, floors[what], HOST)
    finally:
        ctx.close()


@pytest.mark.parametrize("flt", ["gc40_60", "cgtctc_only", "g3"])
def test_with_a_site_filter(C, genome, flt):
    ctx, _, seqs, _, _, _ = genome
    rules = dict(F.EXTRA, gc40_60=dict(zip(("gc_min", "gc_max"), F.percent(20, 40, 60))))[flt]
    kept = F.keep(_sites(genome, "n20_nrg"), seqs, **rules)
    assert 0 < len(kept) < len(_sites(genome, "n20_nrg"))
    m, floors = A.thresholds(seqs, kept, A.distinct(20, 4, 6))
    for what in ("all", "exact", "half"):
        A.hold(C, ctx, seqs, A.N20_NRG, kept, m, floors[what], HOST, filter=C.SiteFilter(**rules))


def test_a_region_cuts_footprints_not_contexts(C, genome):
    ctx, _, seqs, where, index, _ = genome
    m = A.distinct(20, 4, 6)
    # [100, 123) is exactly the footprint of the planted '+' site at 100: its window reaches four bases before and three behind the region
    sites = R.brute_sites(seqs, *R.PATTERNS["n20_nrg"], chrom=index, start=100, end=123)
    assert [(s[1], s[3]) for s in sites] == [(100, "+")]
    A.hold(C, ctx, seqs, A.N20_NRG, sites, m, None, HOST, chrom=index, start=100, end=123)
    for start, end in ((0, 50), (390, 640), (1250, None), (99, 122)):
        sites = R.brute_sites(seqs, *R.PATTERNS["n20_nrg"], chrom=index, start=start, end=end)
        A.hold(C, ctx, seqs, A.N20_NRG, sites, m, None, HOST, chrom="planted", start=start, end=end)
    scores = A.scores_of(seqs, R.brute_sites(seqs, *R.PATTERNS["n20_nrg"], chrom=index, start=390, end=640), m)
    assert scores and A.NONE not in scores[:3]                               # scored from bases outside the region


def test_errors_in_their_order(C, genome):
    ctx = genome[0]
    A.hold_errors(C, ctx, True)
    with pytest.raises(C.CalitasError) as e:
        ctx.find_sites_scored(A.N20_NRG, C.ActivityModel.zeros(21, 4, 6))    # the model before the missing device
    assert e.value.code == C._lib.EINVAL and "protospacer_length" in str(e.value)
    with pytest.raises(C.CalitasError) as e:
        ctx.find_sites_scored(A.N20_NRG, C.ActivityModel.zeros(20, 4, 6))    # the device call on a host-only context
    assert e.value.code == C._lib.ENODEV and "no CPU fallback" in str(e.value)


def test_the_model_file(C, tmp_path):
    path = str(tmp_path / "m.tsv")
    for L, up, down in ((20, 4, 6), (1, 0, 0), (32, 16, 16), (7, 0, 3)):
        for name, m in A.models(L, up, down).items():
            model = A.model_of(C, m)
            model.write(path)
            back = C.ActivityModel.read(path)
            assert back == model and back.link == m["link"], (L, up, down, name)
    text = ("# a comment\nlength\t3\ncontext\t1\t2   # W = 6\nlink\tlogistic\nintercept\t-0.5\nsingle\t*\tG\t0.25\nsingle\t2\t*\t-1\nsingle\t2\tc\t16\n"
            "pair\t*\tA\t*\t0.125\npair\t5\tT\tT\t-16\ngc\t*\t1\ngc\t0\t.5\n")
    with open(path, "w") as f:
        f.write(text)
    m = C.ActivityModel.read(path)
    assert (m.L, m.up, m.down, m.W, m.link, m.intercept) == (3, 1, 2, 6, "logistic", -32768)
    single = np.zeros((6, 4), np.int32)
    single[:, 2] = 16384
    single[1, :] = -65536
    single[1, 1] = 1 << 20
    pair = np.zeros((5, 16), np.int32)
    pair[:, 0:4] = 8192
    pair[4, 15] = -(1 << 20)
    assert np.array_equal(m.single, single) and np.array_equal(m.pair, pair) and m.gc.tolist() == [32768, 65536, 65536, 65536]
    assert C.activity_of("AcGTuA", m) == A.score_of("ACGTTA", {"L": 3, "up": 1, "down": 2, "intercept": -32768, "single": single.tolist(),
                                                             "pair": pair.tolist(), "gc": m.gc.tolist()})
    for bad in ("context\t1\t2\n", "length\t0\n", "length\t33\n", "length\t3\ncontext\t17\t0\n", "length\t3\nlink\tprobit\n", "length\t3\nintercept\t16.001\n",
                "length\t3\nsingle\t4\tA\t1\n", "length\t3\nsingle\t0\tA\t1\n", "length\t3\npair\t3\tA\tA\t1\n", "length\t3\ngc\t4\t1\n",
                "length\t3\nsingle\t1\tN\t1\n", "length\t3\nsingle\t1\tA\t1e-3\n", "length\t3\nsingle\t1\tA\tnan\n", "length\t3\nsingle 1 A 1\n",
                "length\t3\nsingle\t1\tA\n", "length\t3x\n", "length\t3\nweights\t1\n", "length\t3\ngc\t-1\t1\n"):
        with open(path, "w") as f:
            f.write(bad)
        with pytest.raises(ValueError):
            C.ActivityModel.read(path)
    assert os.path.exists(os.path.join(ROOT, "models", "example_activity30.tsv"))
    example = C.ActivityModel.read(os.path.join(ROOT, "models", "example_activity30.tsv"))
    assert (example.L, example.up, example.down, example.W) == (20, 4, 6, 30) and example.single.any() and example.pair.any() and example.gc.any()


def test_the_contract_function(C, genome):
    _, _, seqs, _, _, _ = genome
    for name in ("n20_nrg", "five16_L32"):
        L = len(R.PATTERNS[name][0])
        m = A.distinct(L, 4, 6)
        model = A.model_of(C, m)
        for s in _sites(genome, name)[::7]:
            text = A.context_of(seqs[s[0]], s[1], s[3], L, 4, 6)
            if text is None:
                continue
            raw = seqs[s[0]][s[1] - (4 if s[3] == "+" else 6):s[1] + L + (6 if s[3] == "+" else 4)]
            want = A.score_of(text, m)
            assert C.activity_of(text, model) == (None if want == A.NONE else want)
            if s[3] == "+":
                assert C.activity_of(raw, model) == (None if want == A.NONE else want)      # either case, U as T
    with pytest.raises(ValueError):
        C.activity_of("ACGT", A.model_of(C, A.distinct(20, 4, 6)))
    ident, logi = C.ActivityModel.zeros(20), C.ActivityModel.zeros(20, link="logistic")
    assert C.activity_value(32768, ident) == 0.5 and C.activity_value(0, logi) == 0.5 and C.activity_value(A.NONE, logi) is None
    assert abs(C.activity_value(65536, logi) - 0.7310585786300049) < 1e-15


def test_the_guides_table(C, genome):
    ctx, names, seqs, _, index, _ = genome
    sites = R.brute_sites(seqs, *R.PATTERNS["n20_nrg"], chrom=index)
    m = A.distinct(20, 4, 6)                                                 # link logistic
    model = A.model_of(C, m)
    rows = C.find_guides(ctx, A.N20_NRG, chrom="planted", host=True, activity=model)
    scores = A.scores_of(seqs, sites, m)
    assert [r.activity_q16 for r in rows] == scores and A.NONE in scores
    assert [r.guide_id for r in rows] == [r.guide_id for r in C.find_guides(ctx, A.N20_NRG, chrom="planted", host=True)]
    lines = C.guides_tsv(rows, activity=model).splitlines()
    header = lines[0].split("\t")
    assert header[header.index("pam_sequence") + 1:] == ["activity_q16", "activity"]
    import math
    for line, score in zip(lines[1:], scores):
        q16, value = line.split("\t")[-2:]
        assert (q16, value) == (("NA", "NA") if score == A.NONE else (str(score), "%.6f" % (1.0 / (1.0 + math.exp(-score / 65536.0)))))
    m["link"] = "identity"
    assert C.guides_tsv(rows[:40], activity=A.model_of(C, m)).splitlines()[1:] == [
        ln.rsplit("\t", 1)[0] + "\t" + ("NA" if r.activity_q16 == A.NONE else "%.6f" % (r.activity_q16 / 65536.0)) for ln, r in zip(lines[1:41], rows)]
    # with copies behind: the new columns stand directly behind pam_sequence
    header = C.guides_tsv(rows[:3], copies=[1, 1, 1], activity=model).splitlines()[0].split("\t")
    assert header[-3:] == ["activity_q16", "activity", "copies"]
    # a threshold keeps the guide_ids of the full listing
    m2, floors = A.thresholds(seqs, sites, A.distinct(20, 4, 6))
    kept = C.find_guides(ctx, A.N20_NRG, chrom="planted", host=True, activity=A.model_of(C, m2), min_activity=floors["half"])
    want = [r.guide_id for r, s in zip(rows, A.scores_of(seqs, sites, m2)) if s != A.NONE and s >= floors["half"]]
    assert [r.guide_id for r in kept] == want and 0 < len(want) < len(rows)
    with pytest.raises(ValueError):
        C.find_guides(ctx, A.N20_NRG, host=True, min_activity=0)


def test_both_tools_on_the_host_twin(C, genome, tmp_path):
    ctx, names, seqs, _, index, _ = genome
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    binary = os.path.join(ROOT, "calitas_amd", "calitas")
    env = dict(os.environ, PYTHONPATH=ROOT)
    sites = R.brute_sites(seqs, *R.PATTERNS["n20_nrg"], chrom=index)
    m, floors = A.thresholds(seqs, sites, A.distinct(20, 4, 6))
    model = A.model_of(C, m)
    model_path = str(tmp_path / "activity.tsv")
    model.write(model_path)
    region = ["-i", A.N20_NRG, "-c", "planted"]

    def run(tool, flags):
        out = str(tmp_path / (tool + ".tsv"))
        head = [sys.executable, "-m", "calitas_amd"] if tool == "py" else [binary]
        subprocess.check_call(head + ["FindGuides", "-r", fa, "-o", out, "--device", "-1"] + region + flags, env=env, cwd=ROOT,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out, "rb").read()

    rows = C.find_guides(ctx, A.N20_NRG, chrom="planted", host=True, activity=model)
    a, b = run("py", ["--activity", model_path]), run("cc", ["--activity", model_path])
    assert a == b and a.decode() == C.guides_tsv(rows, activity=model) and b"\tNA\tNA\n" in a
    # the threshold: the site that meets it exactly stays, the one a point below goes; the rows go before --copies counts anything
    exact = A.decimal_of(floors["exact"])
    a, b = run("py", ["--activity", model_path, "--min-activity", exact, "--copies"]), run("cc", ["--activity", model_path, "--min-activity=" + exact, "--copies"])
    kept = [r for r in rows if r.activity_q16 != A.NONE and r.activity_q16 >= floors["exact"]]
    assert a == b and [ln.split("\t")[0] for ln in a.decode().splitlines()[1:]] == [r.guide_id for r in kept]
    assert min(r.activity_q16 for r in kept) == floors["exact"] and floors["exact"] - 1 in [r.activity_q16 for r in rows]
    assert a.decode().splitlines()[0].split("\t")[-3:] == ["activity_q16", "activity", "copies"] and b"NA" not in a
    # a negative threshold, a filter, a link identity model through its file, the example file
    m["link"] = "identity"
    A.model_of(C, m).write(model_path)
    flags = ["--activity", model_path, "--min-activity", "-2.25", "--gc-min", "40", "--near-copies", "1"]
    a, b = run("py", flags), run("cc", flags)
    assert a == b and len(a.splitlines()) > 5
    example = os.path.join(ROOT, "models", "example_activity30.tsv")
    a, b = run("py", ["--activity", example, "--min-activity", "0"]), run("cc", ["--activity", example, "--min-activity", "0"])
    assert a == b and 5 < len(a.splitlines()) < len(rows)
    # the `*` forms, overriding lines, a lower-case base, signs and bare points, through both readers
    stars = str(tmp_path / "stars.tsv")
    with open(stars, "w") as f:
        f.write("length\t20\ncontext\t4\t6\nlink\tlogistic\nintercept\t-0.5\nsingle\t*\tG\t0.25\nsingle\t2\t*\t-1\npair\t*\tA\t*\t0.125\npair\t29\tT\tT\t-16\n"
                "gc\t*\t1\ngc\t0\t.5\n  # an indented comment\n\nsingle\t30\tt\t+2.\ncontext\t4\t6\n")
    a, b = run("py", ["--activity", stars]), run("cc", ["--activity", stars])
    assert a == b and a.decode() == C.guides_tsv(C.find_guides(ctx, A.N20_NRG, chrom="planted", host=True, activity=C.ActivityModel.read(stars)),
                                                 activity=C.ActivityModel.read(stars))
    # the flags' own rules, and files both tools refuse
    short = str(tmp_path / "short.tsv")
    C.ActivityModel.zeros(19, 4, 6).write(short)
    bad_files = []
    for k, text in enumerate(("length\t20\nsingle\t31\tA\t1\n", "length\t20\ncontext\t4\t6\nsingle\t1\tA\t1e-3\n", "context\t4\t6\n", "length\t20\ngc\t21\t1\n",
                              "length\t20\nintercept\t17\n", "length\t20\ncontext\t4 6\n")):
        bad_files.append(str(tmp_path / ("bad%d.tsv" % k)))
        with open(bad_files[-1], "w") as f:
            f.write(text)
    for bad in ([["--min-activity", "1"], ["--activity", short], ["--activity", model_path, "--min-activity", "1e3"],
                 ["--activity", model_path, "--min-activity", "2065"], ["--activity", str(tmp_path / "missing.tsv")]] + [["--activity", p] for p in bad_files]):
        for tool in ("py", "cc"):
            with pytest.raises(subprocess.CalledProcessError):
                run(tool, bad)
