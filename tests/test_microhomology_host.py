"""CPU tests of the microhomology score: calitas_find_sites_microhomology_host (the host twin of microhomology.hip's kernels, on a
host-only context) against the referee of microhomology_ref.py and against microhomology_of -- every window, min_length and cut under
a 3' and a 5' PAM pattern, the planted cases, the two strands of one cut, the per-mille thresholds, a site filter and a region, the
errors in their order -- the model file, the guides table's columns, and both FindGuides tools with --microhomology on the host twin
(--device -1).  No GPU."""
import os
import random
import subprocess
import sys

import pytest

import microhomology_ref as M
import site_filter_ref as F
from fasta_util import write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = (True,)


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


@pytest.fixture(scope="module")
def genome(C):
    names, seqs, where = M.the_genome()
    ctx = C.Context(-1)
    ctx.set_reference(names, [s.encode() for s in seqs])
    yield ctx, names, seqs, where
    ctx.close()


def test_the_referee_on_its_planted_cases(genome):
    _, names, seqs, where = genome
    assert [len(s) for s in seqs] == [900, 3000, 60]
    M.check_planted(seqs, where, M.the_sites("n20_nrg"))


def test_the_two_referees_agree():
    """The diagonal walk against the literal enumeration of k-mer pairs, on about 50 windows (the enumeration is cubic)."""
    _, seqs, where = M.the_genome()
    sites = M.the_sites("n20_nrg")
    rng = random.Random(9)
    sample = rng.sample(sites, 40) + [s for s in sites if s[0] == 1 and (s[1], s[3]) in set(where.values())][:10]
    scored = 0
    for k, s in enumerate(sample):
        left, right = M.WINDOWS[k % len(M.WINDOWS)] if k % 3 else (rng.randrange(1, 33), rng.randrange(1, 33))
        m = M.distinct(left, right, M.MIN_LENGTHS[k % 2] if k % 7 else 4)
        x = M.window_of(seqs[s[0]], s[1], s[3], M.CUT, left, right)
        assert M.walk(x, left, m) == M.literal(x, left, m), (s, left, right)
        scored += M.walk(x, left, m) != M.UNSCORED and M.walk(x, left, m)[0] > 0
    assert scored > 20
    for letters in ("ACGT", "AC", "AT"):                                     # few letters: long runs, many nested pairs
        for _ in range(4):
            left, right = rng.randrange(1, 33), rng.randrange(1, 33)
            x = "".join(rng.choice(letters) for _ in range(left + right))
            m = M.distinct(left, right, rng.choice((2, 3, 4)))
            assert M.walk(x, left, m) == M.literal(x, left, m), (x, left)


@pytest.mark.parametrize("name", M.PATTERNS)
@pytest.mark.parametrize("left, right", M.WINDOWS + M.EDGE_WINDOWS)
def test_the_twin_against_the_referee(C, genome, name, left, right):
    ctx = genome[0]
    for min_length in M.MIN_LENGTHS:
        for cut in M.cuts():
            m = M.distinct(left, right, min_length)
            assert M.hold(C, ctx, name, m, cut, 0, HOST) == len(M.the_sites(name)) > 50
    scores = [s for cut in M.cuts() for s in M.the_scores(name, cut, M.distinct(left, right, 2))]
    assert (M.UNSCORED in scores or name != "n20_nrg") and any(s != M.UNSCORED for s in scores)
    if min(left, right) > 1:
        assert any(s[0] > 0 for s in scores if s != M.UNSCORED)
    else:
        assert all(s == (0, 0) for s in scores if s != M.UNSCORED)           # one position a diagonal: no run of two (the twin still walks all W - 1 of them)


def test_the_contract_function(C, genome):
    _, _, seqs, where = genome
    sites = M.the_sites("n20_nrg")
    for left, right in M.WINDOWS:
        m = M.exponential(left, right, 3)
        model = M.model_of(C, m)
        assert model == C.MicrohomologyModel.exponential(20.0, left, right, 3)
        for s, want in list(zip(sites, M.the_scores("n20_nrg", M.CUT, m)))[::5]:
            x = M.window_of(seqs[s[0]], s[1], s[3], M.CUT, left, right)
            if x is not None:
                assert C.microhomology_of(x, left, model) == (None if want == M.UNSCORED else want)
    p, _ = where["u_flank"]
    raw = seqs[1][p + M.CUT - 30:p + M.CUT + 30]
    assert "U" in raw and C.microhomology_of(raw.lower(), 30, M.model_of(C, M.unit(30, 30))) == M.walk(raw.replace("U", "T"), 30, M.unit(30, 30))
    assert C.microhomology_of("G" * 64, 32, M.model_of(C, M.unit(32, 32))) == (133955584, 89391104)
    assert C.microhomology_of("ACGTN" * 12, 30, M.model_of(C, M.unit(30, 30))) is None
    with pytest.raises(ValueError):
        C.microhomology_of("ACGT", 2, M.model_of(C, M.unit(30, 30)))
    with pytest.raises(ValueError):
        C.microhomology_of("A" * 60, 29, M.model_of(C, M.unit(30, 30)))


def test_the_planted_cases_through_the_twin(C, genome):
    ctx, _, seqs, where = genome
    got = {}
    for left, right in ((30, 30), (32, 32)):
        sites, scores = ctx.find_sites_microhomology(M.N20_NRG, M.model_of(C, M.unit(left, right)), chrom="planted", host=True)     # cut: L - 3
        got[left] = {(int(s["protospacer_start"]), s["strand"].decode()): (int(v["total_q16"]), int(v["out_of_frame_q16"])) for s, v in zip(sites, scores)}
    assert got[32][where["poly_g"]] == (133955584, 89391104)
    assert got[30][where["total_0"]] == (0, 0) == got[32][where["total_0"]]
    assert got[30][where["n_inside"]] == M.UNSCORED != got[30][where["n_beside"]]
    assert got[30][where["r_flank"]] == M.UNSCORED and got[30][where["first_plus"]] == M.UNSCORED == got[30][where["last_minus"]]
    for what in ("u_flank", "u_foot", "soft", "repeat_d9", "repeat_d10", "clipped", "short_run"):
        assert got[30][where[what]] != M.UNSCORED and got[30][where[what]][0] > 0, what


def test_both_strands_of_one_cut_score_the_same(C, genome):
    """left == right: the '-' site's window is the reverse complement of the '+' site's, and x[i] == x[i + d] is kept by both turns."""
    ctx, _, seqs, _ = genome
    seen = 0
    for left in (30, 32, 5):
        m = M.distinct(left, left, 2)
        sites, scores = ctx.find_sites_microhomology(M.N20_NRG, M.model_of(C, m), host=True)
        by_cut = {}
        for s, v in zip(sites, scores):
            cut = int(s["protospacer_start"]) + (M.CUT if s["strand"] == b"+" else M.L - M.CUT)
            by_cut.setdefault((int(s["contig_index"]), cut), {})[s["strand"]] = tuple(v)
        both = [v for v in by_cut.values() if len(v) == 2]
        assert all(v[b"+"] == v[b"-"] for v in both)
        seen += sum(1 for v in both if v[b"+"][0] not in (0, M.NONE))
    assert seen > 20


@pytest.mark.parametrize("permille", M.PERMILLES)
def test_thresholds(C, genome, permille):
    ctx = genome[0]
    kept = {}
    for m in (M.unit(32, 32), M.exponential(30, 30, 3), M.distinct(30, 30, 8)):
        scores = M.the_scores("n20_nrg", M.CUT, m)
        assert M.UNSCORED in scores and (0, 0) in scores                     # the rows a threshold drops whatever it is
        kept[m["min_length"]] = M.hold(C, ctx, "n20_nrg", m, M.CUT, permille, HOST)
        if permille == 0:
            assert kept[m["min_length"]] == len(scores)
        else:
            assert kept[m["min_length"]] <= sum(1 for s in scores if s != M.UNSCORED and s[0] > 0)
    if permille == 1000:
        assert 0 < kept[3] < 100                                             # only sites all of whose deletions shift the frame
    if permille == 667:
        assert 0.2 * 1016 < kept[3] < 0.8 * 1016


def test_the_exact_share_is_kept(C, genome):
    """out_of_frame * 1000 >= permille * total with equality: weights of one Q16 unit for d = 2 .. 6 and 0 elsewhere make the sums small
    integers, so some site's share is a whole per-mille exactly: it is kept at that per-mille and dropped one above."""
    ctx = genome[0]
    m = M.model(30, 30, 2, [0] + [1] * 5 + [0] * 53)
    scores = M.the_scores("n20_nrg", M.CUT, m)
    exact = sorted({s[1] * 1000 // s[0] for s in scores if s != M.UNSCORED and 0 < s[1] < s[0] and s[1] * 1000 % s[0] == 0})
    assert exact
    for permille in exact[:3]:
        meet = sum(1 for s in scores if s != M.UNSCORED and s[0] > 0 and s[1] * 1000 == permille * s[0])
        assert M.hold(C, ctx, "n20_nrg", m, M.CUT, permille, HOST) - M.hold(C, ctx, "n20_nrg", m, M.CUT, permille + 1, HOST) == meet >= 1


@pytest.mark.parametrize("flt", ["gc40_60", "g3"])
def test_with_a_site_filter(C, genome, flt):
    ctx, _, seqs, _ = genome
    rules = dict(F.EXTRA, gc40_60=dict(zip(("gc_min", "gc_max"), F.percent(20, 40, 60))))[flt]
    sites = M.the_sites("n20_nrg")
    kept = F.keep(sites, seqs, **rules)
    assert 0 < len(kept) < len(sites)
    m = M.exponential(30, 30)
    for permille in (0, 667):
        M.hold(C, ctx, "n20_nrg", m, M.CUT, permille, HOST, scores=M.scores_of(seqs, kept, M.CUT, m), sites=kept, filter=C.SiteFilter(**rules))


def test_a_region_cuts_footprints_not_windows(C, genome):
    ctx = genome[0]
    m = M.exponential(30, 30)
    for n in (1, 255):
        start, end = M.region_with("n20_nrg", 1, n)
        assert M.hold(C, ctx, "n20_nrg", m, M.CUT, 0, HOST, chrom=1, start=start, end=end) == n
    start, end = M.region_with("n20_nrg", 1, 255)
    assert M.hold(C, ctx, "n20_nrg", m, M.CUT, 667, HOST, chrom=1, start=start, end=end) < 255
    scores = M.the_scores("n20_nrg", M.CUT, m, 1, 500, 523)
    assert len(scores) == 1 and scores[0] != M.UNSCORED                      # scored from bases outside the region
    M.hold(C, ctx, "n20_nrg", m, M.CUT, 0, HOST, chrom=1, start=500, end=523)
    assert M.hold(C, ctx, "n20_nrg", m, M.CUT, 0, HOST, chrom=1, start=10, end=12) == 0      # an empty listing


def test_errors_in_their_order(C, genome):
    ctx = genome[0]
    M.hold_errors(C, ctx, True)
    with pytest.raises(C.CalitasError) as e:
        ctx.find_sites_microhomology(M.N20_NRG, M.model_of(C, M.unit(30, 30)), 21)       # the model before the missing device
    assert e.value.code == C._lib.EINVAL and "cut_offset" in str(e.value)
    with pytest.raises(C.CalitasError) as e:
        ctx.find_sites_microhomology(M.N20_NRG, M.model_of(C, M.unit(30, 30)), min_out_of_frame=1001)
    assert e.value.code == C._lib.EINVAL and "permille" in str(e.value)
    with pytest.raises(C.CalitasError) as e:
        ctx.find_sites_microhomology(M.N20_NRG, M.model_of(C, M.unit(30, 30)))           # the device call on a host-only context
    assert e.value.code == C._lib.ENODEV and "no CPU fallback" in str(e.value)
    with pytest.raises(ValueError):
        ctx.find_sites_microhomology("tttvNNNNNNNNNNNNNNNNNNNN", M.model_of(C, M.unit(30, 30)), host=True)     # no default cut with a 5' PAM
    for s in ("calitas_find_sites_microhomology", "calitas_find_sites_microhomology_host"):
        assert s in C._lib.SYMBOLS and hasattr(C._lib.lib, s)


def test_the_model_file(C, tmp_path):
    path = str(tmp_path / "m.tsv")
    for left, right in M.WINDOWS + ((7, 3),):
        for m in (M.unit(left, right, 8), M.exponential(left, right, 3), M.distinct(left, right)):
            model = M.model_of(C, m)
            model.write(path)
            assert C.MicrohomologyModel.read(path) == model, (left, right)
    text = "# a comment\nwindow\t3\t2   # W = 5\nweight\t*\t0.25\nweight\t2\t1\nweight\t4\t.5\n  # indented\n\nmin_length\t4\nweight\t4\t1.\n"
    with open(path, "w") as f:
        f.write(text)
    m = C.MicrohomologyModel.read(path)
    assert (m.left, m.right, m.W, m.min_length, m.weight.tolist()) == (3, 2, 5, 4, [16384, 65536, 16384, 65536])
    with open(path, "w") as f:
        f.write("window\t2\t2\n")
    m = C.MicrohomologyModel.read(path)
    assert (m.min_length, m.weight.tolist()) == (2, [0, 0, 0])
    for bad in ("weight\t1\t1\n", "window\t0\t2\n", "window\t33\t2\n", "window\t2\t33\n", "window\t2\t2\nmin_length\t1\n", "window\t2\t2\nmin_length\t9\n",
                "window\t2\t2\nweight\t4\t1\n", "window\t2\t2\nweight\t0\t1\n", "window\t2\t2\nweight\t1\t1.001\n", "window\t2\t2\nweight\t1\t-0.5\n",
                "window\t2\t2\nweight\t1\t1e-3\n", "window\t2\t2\nweight\t1\tnan\n", "window\t2 2\n", "window\t2\t2\nweight\t1\n", "window\t2\t2x\n",
                "window\t2\t2\nweights\t1\t1\n", "window\t2\t2\nweight\t1\t.\n"):
        with open(path, "w") as f:
            f.write(bad)
        with pytest.raises(ValueError):
            C.MicrohomologyModel.read(path)
    example = C.MicrohomologyModel.read(os.path.join(ROOT, "models", "example_microhomology60.tsv"))
    assert example == C.MicrohomologyModel.exponential(20.0, 30, 30) and example.weight[0] == 62340 and example.min_length == 2


def test_the_guides_table(C, genome):
    ctx, names, seqs, where = genome
    m = M.exponential(30, 30)
    model = M.model_of(C, m)
    scores = M.the_scores("n20_nrg", M.CUT, m, 1)
    rows = C.find_guides(ctx, M.N20_NRG, chrom="planted", host=True, microhomology=model)
    assert [(r.mh_total_q16, r.mh_oof_q16) for r in rows] == scores and M.UNSCORED in scores and (0, 0) in scores
    plain = C.find_guides(ctx, M.N20_NRG, chrom="planted", host=True)
    assert [r.guide_id for r in rows] == [r.guide_id for r in plain] and plain[0].mh_total_q16 is None
    lines = C.guides_tsv(rows, microhomology=model).splitlines()
    header = lines[0].split("\t")
    assert header[header.index("pam_sequence") + 1:] == ["mh_total_q16", "mh_oof_q16", "mh_score", "out_of_frame"]
    for line, (total, oof) in zip(lines[1:], scores):
        want = ["NA"] * 4 if total == M.NONE else [str(total), str(oof), "%.3f" % (100.0 * total / 65536.0), "%.2f" % (100.0 * oof / total) if total else "NA"]
        assert line.split("\t")[-4:] == want
    # behind activity when present, ahead of copies
    activity = C.ActivityModel.read(os.path.join(ROOT, "models", "example_activity30.tsv"))
    both = C.find_guides(ctx, M.N20_NRG, chrom="planted", host=True, microhomology=model, activity=activity)
    assert [(r.guide_id, r.mh_total_q16, r.mh_oof_q16) for r in both] == [(r.guide_id, r.mh_total_q16, r.mh_oof_q16) for r in rows]
    header = C.guides_tsv(both[:3], copies=[1, 1, 1], activity=activity, microhomology=model).splitlines()[0].split("\t")
    assert header[-7:] == ["activity_q16", "activity", "mh_total_q16", "mh_oof_q16", "mh_score", "out_of_frame", "copies"]
    # a threshold keeps the guide_ids of the full listing; with activity the two listings are joined
    want = [r.guide_id for r, s in zip(rows, scores) if M.kept(s, 667)]
    for extra in ({}, {"activity": activity}):
        kept = C.find_guides(ctx, M.N20_NRG, chrom="planted", host=True, microhomology=model, min_out_of_frame=667, **extra)
        assert [r.guide_id for r in kept] == want and 0 < len(want) < len(rows)
    assert [r.activity_q16 for r in kept] == [r.activity_q16 for r in both if r.guide_id in set(want)]
    with pytest.raises(ValueError):
        C.find_guides(ctx, M.N20_NRG, host=True, min_out_of_frame=10)
    with pytest.raises(ValueError):
        C.find_guides(ctx, M.N20_NRG, host=True, mh_cut=3)


def test_both_tools_on_the_host_twin(C, genome, tmp_path):
    ctx, names, seqs, _ = genome
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    binary = os.path.join(ROOT, "calitas_amd", "calitas")
    env = dict(os.environ, PYTHONPATH=ROOT)
    model = M.model_of(C, M.exponential(30, 30, 3))
    model_path = str(tmp_path / "mh.tsv")
    model.write(model_path)
    activity = os.path.join(ROOT, "models", "example_activity30.tsv")

    def run(tool, flags, pattern=M.N20_NRG):
        out = str(tmp_path / (tool + ".tsv"))
        head = [sys.executable, "-m", "calitas_amd"] if tool == "py" else [binary]
        subprocess.check_call(head + ["FindGuides", "-r", fa, "-o", out, "--device", "-1", "-i", pattern] + flags, env=env, cwd=ROOT,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out, "rb").read()

    rows = C.find_guides(ctx, M.N20_NRG, host=True, microhomology=model)
    a, b = run("py", ["--microhomology", model_path]), run("cc", ["--microhomology", model_path])
    assert a == b and a.decode() == C.guides_tsv(rows, microhomology=model) and b"\tNA\tNA\tNA\tNA\n" in a
    assert any(ln.endswith("\t0\t0\t0.000\tNA") for ln in a.decode().splitlines())              # a total of 0: no share
    # the threshold: PCT * 10 per mille; the rows go before --copies counts anything and keep their guide_ids
    flags = ["--microhomology", model_path, "--min-out-of-frame", "67", "--copies"]
    a, b = run("py", flags), run("cc", flags[:2] + ["--min-out-of-frame=67", "--copies"])
    kept = [r for r in rows if M.kept((r.mh_total_q16, r.mh_oof_q16), 670)]
    assert a == b and [ln.split("\t")[0] for ln in a.decode().splitlines()[1:]] == [r.guide_id for r in kept] and 0 < len(kept) < len(rows)
    assert a.decode().splitlines()[0].split("\t")[-5:] == ["mh_total_q16", "mh_oof_q16", "mh_score", "out_of_frame", "copies"] and b"NA" not in a
    # with --activity: joined on (contig, start, strand); the columns stand behind activity
    for flags in (["--microhomology", model_path, "--activity", activity], ["--microhomology", model_path, "--activity", activity, "--min-activity", "0", "--min-out-of-frame", "50"],
                  ["--microhomology", model_path, "--mh-cut", "10", "--gc-min", "40", "--near-copies", "1", "-c", "planted", "-s", "100", "-e", "2000"]):
        a, b = run("py", flags), run("cc", flags)
        assert a == b and len(a.splitlines()) > 5, flags
    assert a.decode().splitlines()[0].split("\t")[8:12] == ["mh_total_q16", "mh_oof_q16", "mh_score", "out_of_frame"]
    flags = ["--microhomology", model_path, "--activity", activity]
    assert run("cc", flags).decode().splitlines()[0].split("\t")[8:14] == ["activity_q16", "activity", "mh_total_q16", "mh_oof_q16", "mh_score", "out_of_frame"]
    # a 5' PAM needs --mh-cut; the example file; the `*` form and overriding lines through both readers
    flags = ["--microhomology", os.path.join(ROOT, "models", "example_microhomology60.tsv"), "--mh-cut", "18"]
    a, b = run("py", flags, "tttvNNNNNNNNNNNNNNNNNNNN"), run("cc", flags, "tttvNNNNNNNNNNNNNNNNNNNN")
    assert a == b and len(a.splitlines()) > 5
    stars = str(tmp_path / "stars.tsv")
    with open(stars, "w") as f:
        f.write("# c\nwindow\t12\t9\nweight\t*\t0.25\nweight\t2\t1\nweight\t4\t.5\n  # indented\n\nmin_length\t3\nweight\t4\t1.\nwindow\t12\t9\n")
    a, b = run("py", ["--microhomology", stars, "--min-out-of-frame", "100"]), run("cc", ["--microhomology", stars, "--min-out-of-frame", "100"])
    assert a == b and a.decode() == C.guides_tsv(C.find_guides(ctx, M.N20_NRG, host=True, microhomology=C.MicrohomologyModel.read(stars), min_out_of_frame=1000),
                                                 microhomology=C.MicrohomologyModel.read(stars))
    # the flags' own rules, and files both tools refuse
    bad_files = []
    for k, text in enumerate(("weight\t1\t1\n", "window\t33\t2\n", "window\t2\t2\nmin_length\t9\n", "window\t2\t2\nweight\t4\t1\n", "window\t2\t2\nweight\t1\t1e-3\n",
                              "window\t2\t2\nweight\t1\t1.5\n", "window\t2 2\n")):
        bad_files.append(str(tmp_path / ("bad%d.tsv" % k)))
        with open(bad_files[-1], "w") as f:
            f.write(text)
    for bad in ([["--mh-cut", "17"], ["--min-out-of-frame", "10"], ["--microhomology", model_path, "--mh-cut", "21"], ["--microhomology", model_path, "--mh-cut", "x"],
                 ["--microhomology", model_path, "--min-out-of-frame", "101"], ["--microhomology", model_path, "--min-out-of-frame", "6.5"],
                 ["--microhomology", str(tmp_path / "missing.tsv")]] + [["--microhomology", p] for p in bad_files]):
        for tool in ("py", "cc"):
            with pytest.raises(subprocess.CalledProcessError):
                run(tool, bad)
    for tool in ("py", "cc"):
        with pytest.raises(subprocess.CalledProcessError):
            run(tool, ["--microhomology", model_path], "tttvNNNNNNNNNNNNNNNNNNNN")               # no default cut with a 5' PAM
