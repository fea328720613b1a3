"""CPU tests of the site filters (calitas_find_sites_filtered_host on a host-only context): the host twin against the referee of
site_filter_ref.py as record bytes, the planted cases, the open filter, validation, SiteFilter.percent, and both FindGuides tools with
--device -1 and the filter flags; the parameter sweep of site_filter_ref.sweep_sets (every length, every bound).  No GPU."""
import os
import random
import subprocess
import sys

import pytest

import site_filter_ref as F
import sites_ref as R
from fasta_util import write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = ["n20_nrg", "tttv_n20", "n21", "five16_L32", "one_letter"]
N20 = "NNNNNNNNNNNNNNNNNNNNnrg"


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


_brute = {}


def _genome(which):
    if which not in _brute:
        if which == "host":
            names, seqs = R.host_genome()
            planted = None
        else:
            names, seqs, planted = F.filter_genome()
        _brute[which] = (names, seqs, planted, {})
    return _brute[which]


def _sites(which, name):
    names, seqs, _, done = _genome(which)
    if name not in done:
        done[name] = R.brute_sites(seqs, *R.PATTERNS[name])
    return done[name]


@pytest.fixture(scope="module")
def contexts(C):
    made = {}
    for which in ("host", "planted"):
        names, seqs, _, _ = _genome(which)
        made[which] = C.Context(-1)
        made[which].set_reference(names, [s.encode() for s in seqs])
    yield made
    for ctx in made.values():
        ctx.close()


def _pattern(C, name):
    text, aux = R.pattern_string(name)
    return C.Guide(text, aux)


def _filters(name):
    """{GC only, runs only, a limit on one base, motifs only, all together} for a pattern.  40 - 60 % of the one base of one_letter is no
    count at all (1 .. 0) and no six-letter motif fits it: there the GC bound is "at least one", the motif a one-letter IUPAC code."""
    L = len(R.PATTERNS[name][0])
    if L >= 6:
        return F.filters(L)
    return {"gc": dict(gc_min=1), "runs3": dict(max_run=(3, 3, 3, 3)), "t3": dict(max_run=(0, 0, 0, 3)), "bsmbi": dict(avoid=("K",)),
            "all": dict(gc_max=0, max_run=(1, 1, 1, 1), avoid=("Y",))}


@pytest.mark.parametrize("which", ["host", "planted"])
@pytest.mark.parametrize("name", PATTERNS)
def test_host_twin_equals_referee(C, contexts, name, which):
    ctx = contexts[which]
    _, seqs, _, _ = _genome(which)
    sites = _sites(which, name)
    plain = ctx.find_sites(_pattern(C, name), host=True)
    assert plain.tobytes() == R.as_records(sites, plain.dtype).tobytes()
    for fname, flt in _filters(name).items():
        want = F.keep(sites, seqs, **flt)
        got = ctx.find_sites(_pattern(C, name), host=True, filter=C.SiteFilter(**flt))
        print(which, name, fname, "sites", len(sites), "kept", len(want))
        assert got.tobytes() == R.as_records(want, got.dtype).tobytes(), (name, fname)
        # the subsequence of the unfiltered listing
        it = iter(plain.tolist())
        assert all(any(rec == other for other in it) for rec in got.tolist()), (name, fname)
    if name == "n20_nrg":
        for fname, flt in F.filters(20).items():
            kept = len(F.keep(sites, seqs, **flt))
            assert 0 < kept < len(sites), fname


def test_the_planted_cases(C, contexts):
    """Every planted protospacer is a site of N20 + nrg, and the library's verdict on it under its filter is the intended one."""
    ctx = contexts["planted"]
    _, seqs, planted, _ = _genome("planted")
    sites = _sites("planted", "n20_nrg")
    F.check_planted(seqs, planted, sites)
    filters = dict(F.filters(20), **F.EXTRA)
    listed = {}
    for fname in sorted({p[3] for p in planted}):
        got = ctx.find_sites(N20, host=True, filter=C.SiteFilter(**filters[fname]))
        listed[fname] = {(int(s["protospacer_start"]), s["strand"].decode()) for s in got}
    for name, strand, p, fname, kept in planted:
        assert ((p, strand) in listed[fname]) == kept, (name, strand, p)
    assert {p[0] for p in planted} >= {"gc7", "gc8", "gc12", "gc13", "gc0", "gc20", "run_T_into_pam", "run_A_into_flank", "t3_with_aaaaa",
                                        "motif_first", "motif_last", "motif_out_5", "motif_out_3", "motif_iupac", "motif_rc_only", "u_run4",
                                        "u_minus_run4", "u_gc", "u_in_pam_gc7", "u_in_pam_gc10"}


@pytest.mark.parametrize("name", ["n20_nngrrt_nrg", "eight_pams"])
def test_u_in_the_longer_pam_only(C, contexts, name):
    """<protospacer>AGGAGU: nngrrt is the first PAM that matches (the U a T), nrg a later one.  The filter's verdict is the
    protospacer's, whichever PAM is recorded: rejected by one filter, kept by another, with the unfiltered pam_index."""
    ctx = contexts["planted"]
    _, seqs, planted, _ = _genome("planted")
    sites = _sites("planted", name)
    k_long = R.PATTERNS[name][1].index("nngrrt")
    by_place = {(s[1], s[3]): s for s in sites}
    gc = F.filters(20)["gc"]
    got = R.as_tuples(ctx.find_sites(_pattern(C, name), host=True, filter=C.SiteFilter(**gc)))
    assert got == F.keep(sites, seqs, **gc)
    for case, strand, p, _, kept in planted:
        if case.startswith("u_in_pam"):
            assert by_place[(p, strand)][4] == k_long and by_place[(p, strand)][5] == 6
            assert (by_place[(p, strand)] in got) == kept


def test_a_motif_of_the_protospacers_length(C, contexts):
    """A motif as long as the protospacer (the window of occurrences is one position wide) and one letter longer (an error)."""
    ctx = contexts["planted"]
    _, seqs, _, _ = _genome("planted")
    sites = R.brute_sites(seqs, "NNNNNNNN", ["ngg"], False)
    for motif in ("SWNNNNKN", "NNSWNNNA", "WNNNNNNS"):
        want = F.keep(sites, seqs, avoid=(motif,))
        got = ctx.find_sites("NNNNNNNNngg", host=True, filter=C.SiteFilter(avoid=[motif]))
        assert 0 < len(want) < len(sites) and R.as_tuples(got) == want
    with pytest.raises(C.CalitasError) as e:
        ctx.find_sites("NNNNNNNNngg", host=True, filter=C.SiteFilter(avoid=["ACGTNNNNA"]))
    assert e.value.code == C._lib.EINVAL and "motifs[0]" in str(e.value)
    # sixteen letters, the longest, in a protospacer of 32
    sites = _sites("planted", "five16_L32")
    want = F.keep(sites, seqs, avoid=("NNNNNNNNNNNNCGSW",))
    got = ctx.find_sites(_pattern(C, "five16_L32"), host=True, filter=C.SiteFilter(avoid=["nnnnnnnnnnnncgsw"]))
    assert 0 < len(want) < len(sites) and R.as_tuples(got) == want


def test_no_filter_and_the_open_filter(C, contexts):
    for which in ("host", "planted"):
        ctx = contexts[which]
        for name in PATTERNS:
            plain = ctx.find_sites(_pattern(C, name), host=True).tobytes()
            assert ctx.find_sites(_pattern(C, name), host=True, filter=None).tobytes() == plain
            assert ctx.find_sites(_pattern(C, name), host=True, filter=C.SiteFilter()).tobytes() == plain
            assert ctx.find_sites(_pattern(C, name), host=True, filter=C.SiteFilter(0, 255, 0, ())).tobytes() == plain
            # limits no protospacer can exceed, and a filter that rejects everything
            assert ctx.find_sites(_pattern(C, name), host=True, filter=C.SiteFilter(max_run=32, gc_max=32)).tobytes() == plain
            assert len(ctx.find_sites(_pattern(C, name), host=True, filter=C.SiteFilter(avoid=["A", "C", "G", "T"]))) == 0


def test_null_filter_through_the_abi(C, contexts):
    """filter == NULL in the filtered entry point is the unfiltered call."""
    import ctypes
    from calitas_amd import _lib
    ctx = contexts["host"]
    g = _pattern(C, "n20_nrg").to_c()
    out, n = ctypes.POINTER(_lib.SiteT)(), ctypes.c_uint64()
    _lib.check(ctx._h, _lib.lib.calitas_find_sites_filtered_host(ctx._h, ctypes.byref(g), None, -1, 0, 0, ctypes.byref(out), ctypes.byref(n)))
    try:
        raw = ctypes.string_at(out, n.value * ctypes.sizeof(_lib.SiteT))
    finally:
        _lib.lib.calitas_free(out)
    assert raw == ctx.find_sites(_pattern(C, "n20_nrg"), host=True).tobytes() and n.value > 0
    assert ctypes.sizeof(_lib.SiteFilterT) == 8 + 8 * 16


def test_validation(C, contexts):
    ctx = contexts["host"]

    def fails(field, **flt):
        with pytest.raises(C.CalitasError) as e:
            ctx.find_sites(N20, host=True, filter=C.SiteFilter(**flt))
        assert e.value.code == C._lib.EINVAL and field in str(e.value), str(e.value)

    fails("gc_min", gc_min=13, gc_max=12)
    fails("gc_min", gc_min=21)                       # above L, which is what the open gc_max means
    fails("motifs[1]", avoid=["ACGT", "ACXT"])
    fails("motifs[0]", avoid=["NNN"])
    fails("motifs[0]", avoid=[""])
    fails("motifs[2]", avoid=["A", "C", "N"])
    with pytest.raises(C.CalitasError) as e:          # longer than L
        ctx.find_sites("NNNNngg", host=True, filter=C.SiteFilter(avoid=["ACGTA"]))
    assert e.value.code == C._lib.EINVAL and "motifs[0]" in str(e.value)
    # what the struct itself can say and SiteFilter cannot: nine motifs, a reserved byte
    for field, change in (("n_motifs", lambda f: setattr(f, "n_motifs", 9)), ("reserved", lambda f: setattr(f, "reserved", 1))):
        class Raw(C.SiteFilter):
            def to_c(self, change=change):
                f = C.SiteFilter.to_c(self)
                change(f)
                return f
        with pytest.raises(C.CalitasError) as e:
            ctx.find_sites(N20, host=True, filter=Raw())
        assert e.value.code == C._lib.EINVAL and field in str(e.value)
    with pytest.raises(ValueError):
        C.SiteFilter(avoid=["A"] * 9).to_c()
    with pytest.raises(ValueError):
        C.SiteFilter(avoid=["A" * 17]).to_c()
    # legal: gc_min == gc_max == L, a limit of L and more, sixteen letters, lower case
    assert len(ctx.find_sites(N20, host=True, filter=C.SiteFilter(gc_min=20, gc_max=20, max_run=200, avoid=["acgtacgtacgtacgt"]))) >= 0
    # the error does not stick
    assert len(ctx.find_sites(N20, host=True, filter=C.SiteFilter(gc_min=8, gc_max=12))) > 0


def test_site_filter_arguments(C):
    assert C.SiteFilter.percent(20, 40, 60) == (8, 12)
    assert C.SiteFilter.percent(21, 40, 60) == (9, 12)            # 8.4 up, 12.6 down
    assert C.SiteFilter.percent(32, 40, 60) == (13, 19)           # 12.8 up, 19.2 down
    assert C.SiteFilter.percent(21, 0, 100) == (0, 21) and C.SiteFilter.percent(32, 50, 50) == (16, 16) and C.SiteFilter.percent(21, 50, 50) == (11, 10)
    assert C.SiteFilter(max_run=3).max_run == (3, 3, 3, 3)
    assert C.SiteFilter(max_run={"T": 3, "g": 4}).max_run == (0, 0, 4, 3)
    assert C.SiteFilter(max_run=[1, 2, 3, 4]).max_run == (1, 2, 3, 4)
    with pytest.raises(ValueError):
        C.SiteFilter(max_run={"X": 3})
    f = C.SiteFilter(8, 12, {"T": 3}, ["CGTCTC", "ggncc"]).to_c()
    assert (f.gc_min, f.gc_max, list(f.max_run), f.n_motifs, f.reserved) == (8, 12, [0, 0, 0, 3], 2, 0)
    assert f.motifs[0].value == b"CGTCTC" and f.motifs[1].value == b"ggncc" and f.motifs[2].value == b""
    assert C.iupac_revcomp("CGTCTC") == "GAGACG" and C.iupac_revcomp("ggncc") == "GGNCC" and C.iupac_revcomp("ARYB") == "VRYT"
    flt = C.site_filter_of_flags(20, 40, 60, "T=3,g=4", ["cgtctc", "GGNCC"])
    assert (flt.gc_min, flt.gc_max, flt.max_run, flt.avoid) == (8, 12, (0, 0, 4, 3), ("CGTCTC", "GAGACG", "GGNCC"))
    assert C.site_filter_of_flags(20) is None and C.site_filter_of_flags(20, max_run="4").max_run == (4, 4, 4, 4)
    with pytest.raises(ValueError):
        C.site_filter_of_flags(20, avoid=["AAC", "AAG", "AAT", "ACC", "ACG"])          # ten with the reverse complements


def test_find_guides_with_a_filter(C, contexts):
    ctx = contexts["host"]
    _, seqs, _, _ = _genome("host")
    flt = F.filters(20)["all"]
    rows = C.find_guides(ctx, N20, host=True, filter=C.SiteFilter(**flt))
    plain = C.find_guides(ctx, N20, host=True)
    want = F.keep(_sites("host", "n20_nrg"), seqs, **flt)
    assert [(r.protospacer_start, r.strand) for r in rows] == [(w[1], w[3]) for w in want] and 0 < len(rows) < len(plain)
    assert [r.row() for r in rows] == [r.row() for r in plain if (r.protospacer_start, r.strand, r.chromosome) in
                                       {(x.protospacer_start, x.strand, x.chromosome) for x in rows}]
    assert all(F.passes(r.guide[:20], **flt) for r in rows)


def test_both_tools_with_the_filter_flags_on_the_host_twin(C, contexts, tmp_path):
    """`python -m calitas_amd FindGuides` and `calitas FindGuides` with --device -1: identical text, the referee's rows."""
    names, seqs, _, _ = _genome("planted")
    fa = write_fasta(str(tmp_path / "f.fa"), list(zip(names, seqs)))
    binary = os.path.join(ROOT, "calitas_amd", "calitas")
    env = dict(os.environ, PYTHONPATH=ROOT)
    sites = _sites("planted", "n20_nrg")
    plain = C.find_guides(contexts["planted"], N20, host=True)
    by_place = {(r.protospacer_start, r.strand): r for r in plain}
    runs = [
        (["--gc-min", "40", "--gc-max", "60"], dict(gc_min=8, gc_max=12)),
        (["--max-run", "3"], dict(max_run=(3, 3, 3, 3))),
        (["--max-run", "T=3"], dict(max_run=(0, 0, 0, 3))),
        (["--avoid", "CGTCTC"], dict(avoid=("CGTCTC", "GAGACG"))),
        (["--gc-min=40", "--gc-max=60", "--max-run", "A=4,C=4,G=4,T=3", "--avoid", "CGTCTC", "--avoid", "ggncc", "-c", "chrF", "-s", "100", "-e", "11000"],
         dict(gc_min=8, gc_max=12, max_run=(4, 4, 4, 3), avoid=("CGTCTC", "GAGACG", "GGNCC"))),
    ]
    for k, (flags, flt) in enumerate(runs):
        py, cc = str(tmp_path / ("py%d.tsv" % k)), str(tmp_path / ("cc%d.tsv" % k))
        subprocess.check_call([sys.executable, "-m", "calitas_amd", "FindGuides", "-r", fa, "-i", N20, "-o", py, "--device", "-1"] + flags, env=env, cwd=ROOT)
        subprocess.check_call([binary, "FindGuides", "-r", fa, "-i", N20, "-o", cc, "--device", "-1"] + flags)
        a = open(py, "rb").read()
        assert a == open(cc, "rb").read(), flags
        region = R.brute_sites(seqs, *R.PATTERNS["n20_nrg"], chrom=0, start=100, end=11000) if "-s" in flags else sites
        want = F.keep(region, seqs, **flt)
        assert 0 < len(want) < len(region)
        assert a.decode() == C.guides_tsv([by_place[(w[1], w[3])] for w in want]), flags
    for tool in ([sys.executable, "-m", "calitas_amd"], [binary]):         # nine motifs with the reverse complements
        bad = subprocess.run(tool + ["FindGuides", "-r", fa, "-i", N20, "--device", "-1"] + sum([["--avoid", m] for m in ("AAC", "AAG", "AAT", "ACC", "ACG")], []),
                             env=env, cwd=ROOT, capture_output=True)
        assert bad.returncode != 0


# ---- the parameter sweep (site_filter_ref.sweep_sets): every protospacer length, every bound at which a verdict can change ----

@pytest.fixture(scope="module")
def sweep_ctx(C):
    names, seqs = F.sweep_genome()
    ctx = C.Context(-1)
    ctx.set_reference(names, [s.encode() for s in seqs])
    yield ctx
    ctx.close()


_sweep_plain = {}


def _sweep_plain_listing(C, ctx, L, pam):
    """The referee's unfiltered listing of a sweep pattern as records, held against the host twin's as bytes when first asked for."""
    if (L, pam) not in _sweep_plain:
        ls = F.listing(L, pam)
        got = ctx.find_sites(ls.pattern, host=True)
        plain = R.as_records(ls.sites, got.dtype)
        assert got.tobytes() == plain.tobytes(), (L, pam, F.first_difference(got.tolist(), plain.tolist()))
        _sweep_plain[(L, pam)] = plain
    return _sweep_plain[(L, pam)]


def test_sweep_genome_is_on_target():
    """check_sweep on the referee alone, for every length."""
    F.check_motif_strings()
    for L in F.SWEEP_LENGTHS:
        ls = F.checked_listing(L)
        some = random.Random(L).sample(range(len(ls.sites)), 1500)                 # (the combined masks are passes()' verdicts)
        for flt in F.motif_sets(L)[-1:] + F.together_sets(L)[:2]:
            mask = ls.mask(**flt)
            assert all(bool(mask[i]) == F.passes(ls.features.protos[i], **flt) for i in some), (L, flt)
    for L in (20, 32):
        for minus in (False, True):
            here = F.listing(L).features.minus == minus
            assert 0 < int(F.listing(L).mask(avoid=F.EIGHT)[here].sum()) < int(here.sum())
    for L in F.PAM_LENGTHS:
        for pam in F.PAM_PATTERNS:
            ls = F.listing(L, pam)
            assert 50 < len(ls.sites) < len(F.listing(L).sites) // 2 and 0 < int(ls.features.minus.sum()) < len(ls.sites)


@pytest.mark.parametrize("kind", F.SWEEP_KINDS)
def test_sweep_host_twin(C, sweep_ctx, kind):
    """find_sites(host=True, filter=...) == plain[mask] as bytes for every parameter set of the kind."""
    each_way = 0
    for L, pam, flt in F.sweep_sets(kind):
        ls = F.checked_listing(L, pam)
        plain = _sweep_plain_listing(C, sweep_ctx, L, pam)
        mask = ls.mask(**flt)
        want = plain[mask]
        got = sweep_ctx.find_sites(ls.pattern, host=True, filter=C.SiteFilter(**flt))
        assert got.tobytes() == want.tobytes(), (L, pam, flt, F.first_difference(got.tolist(), want.tolist()))
        each_way += 0 < len(want) < len(plain)
    print(kind, "sets", len(F.sweep_sets(kind)), "that keep and reject", each_way)
    assert each_way > len(F.sweep_sets(kind)) // 2
