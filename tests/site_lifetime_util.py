"""What the lifetime tests of the guide-site calls share (test_site_lifetime_host.py, test_gpu_site_lifetime.py): one ROUND that runs
every entry point of the family once on a context's current reference, the SEQUENCE of references a long-lived context is taken through,
the calls that shrink inside one reference, the calls the library refuses, and patterns drawn at random with a genome they are planted in.

Everything a round passes -- queries, SNVs, regions, the searched guide -- is derived from the reference's strings alone, so the same round
can be replayed on any context that holds the same strings: the long-lived one, a fresh one, a host-only one.  A round returns a dict of
bytes, integers and lists of them; two rounds agree when the dicts are equal.  Every output is an integer: there are no tolerances."""
import os
import random

import numpy as np

import edit_sites_ref as E
import sites_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# consecutive calls change the protospacer's length (20, 20, 32), the PAM's side (3', 5', 3') and the number of PAMs (1, 8, 1)
PATTERN_NAMES = ("n20_nrg", "five_prime_eight", "max48")
MOST = 700                                       # the longest list of a round
EDIT = ("C", "T", (3, 8), "N", False, None)
STAMP = ("v0", "stamp")                          # version and time stamp of a hits text: two runs give the same bytes


def pattern_of(C, name):
    text, aux = R.pattern_string(name)
    return C.Guide(text, aux)


def site_filter(C, L):
    """A filter that keeps some sites and drops others at every length: 35 .. 65 % G + C, no run above 4, one motif."""
    lo, hi = C.SiteFilter.percent(L, 35, 65)
    return C.SiteFilter(lo, hi, max_run=4, avoid=("GGNCC",))


_MODELS = {}


def models(C):
    """(the activity model, the microhomology model) of models/."""
    if not _MODELS:
        _MODELS["activity"] = C.ActivityModel.read(os.path.join(ROOT, "models", "example_activity30.tsv"))
        _MODELS["mh"] = C.MicrohomologyModel.read(os.path.join(ROOT, "models", "example_microhomology60.tsv"))
    return _MODELS["activity"], _MODELS["mh"]


def _letter(c):
    return c.upper().replace("U", "T")


def snvs_of_strings(seqs, seed=17, most=MOST):
    """[(contig_index, position, ref, alt)]: every 7th position of every contig and, behind them, the first and the last base of every
    contig; alt is drawn from the letters that differ from the reference's (any letter where the reference has no A C G T U), ref is given
    for every third.  A list above `most` keeps the contigs' ends and an even share of the rest.  Not sorted, with repeats (position 0)."""
    rng = random.Random(seed)

    def snv(ci, pos, k):
        here = _letter(seqs[ci][pos])
        alt = rng.choice([x for x in "ACGT" if x != here])
        return (ci, pos, here if (k % 3 == 0 and here in "ACGT") else "", alt)

    body = [(ci, pos) for ci, s in enumerate(seqs) for pos in range(0, len(s), 7)]
    ends = [(ci, pos) for ci, s in enumerate(seqs) for pos in (0, len(s) - 1)]
    room = max(0, most - len(ends))
    if len(body) > room:
        body = [body[(i * len(body)) // room] for i in range(room)]
    return [snv(ci, pos, k) for k, (ci, pos) in enumerate(body + ends)]


def queries_of_strings(seqs, L, n=24):
    """At most n + 1 keys of L letters: cuts of the contigs' own text at positions spread over them (the '+' guide of whatever site stands
    there) and one key of the repeated word ACGT."""
    out = []
    fit = [ci for ci, s in enumerate(seqs) if len(s) >= L]
    for k in range(n if fit else 0):
        s = seqs[fit[k % len(fit)]]
        at = (k * 37 + 11) % (len(s) - L + 1)
        text = _letter(s[at:at + L])
        if set(text) <= set("ACGT"):
            out.append(text)
    return out + [("ACGT" * 8)[:L]]


def guide_of_strings(seqs):
    """A 20-base guide with nrg behind it, cut from the first place from a third into a contig on that has an N R G behind 20 plain
    bases: the reference has at least that hit."""
    for s in seqs:
        for at in range(len(s) // 3, len(s) - 22):
            text = s[at:at + 23].upper()
            if set(text) <= set("ACGT") and text[21] in "AG" and text[22] == "G":
                return text[:20] + "nrg"
    return R.FIXED + "nrg"


def regions_of_strings(C, names, seqs):
    """A Regions in the strings' own coordinates: every contig's first and last base, a fifth and a half of it, and an interval across
    every multiple of 8192 (the boundary between two segments of the site pass)."""
    iv = []
    for nm, s in zip(names, seqs):
        n = len(s)
        iv += [(nm, 0, 1, "edge"), (nm, n - 1, n, "edge")]
        if n >= 10:
            iv += [(nm, n // 5, n // 5 + max(1, n // 10), "exon"), (nm, n // 2, n // 2 + max(1, n // 4), "utr")]
        iv += [(nm, b - 30, b + 30, "cut") for b in range(8192, n - 30, 8192)]
    return C.Regions(iv, classes=["cut", "exon", "utr", "edge"])


def _count_sites(ctx, pat, host, **kw):
    """count_sites as a list; the host has no call of its own: it counts the twin's listing."""
    if not host:
        n, table = ctx.count_sites(pat, **kw)
        return [int(n), np.ascontiguousarray(table).tobytes()]
    sites = ctx.find_sites(pat, host=True, **kw)
    table = np.zeros((len(ctx.contig_names), 2), dtype=np.uint64)
    np.add.at(table, (sites["contig_index"].astype(np.int64), (sites["strand"] == b"-").astype(np.int64)), 1)
    return [len(sites), table.tobytes()]


def _near_list(x):
    return [x.near.tobytes(), x.offsets.tobytes(), x.hits.tobytes()]


def _near_scores(x):
    return [x.near.tobytes(), x.sum_q32.tobytes(), x.max_q32.tobytes()]


def region_calls(C, ctx, pat, L, host):
    """The three calls that need the context's region set, as (name, thunk)."""
    return [("find_sites_regions", lambda: [x.tobytes() for x in ctx.find_sites_regions(pat, host=host)]),
            ("count_sites_regions", lambda: ctx.count_sites_regions(pat, classes=0b10101, extent=(0, 1), filter=site_filter(C, L), host=host).tobytes()),
            ("site_presence", lambda: [ctx.site_presence()[0].tobytes(), int(ctx.site_presence()[1])])]


def round_of(C, ctx, names, seqs, *, host):
    """Every entry point of the family once on the context's current reference, which holds `seqs`.  host: the host twins (a host-only
    context has nothing else); the search calls, which have no twin, are then left out.  The region calls run when the context has a
    region set (ctx.regions)."""
    out = {}
    activity, mh = models(C)
    raw = snvs_of_strings(seqs)
    snvs = E.snv_array(C, raw)
    edit = E.edit_of(C, EDIT)
    for name in PATTERN_NAMES:
        pat = pattern_of(C, name)
        L = pat.protospacer_length
        flt = site_filter(C, L)
        put = lambda key, value: out.__setitem__("%s/%s" % (key, name), value)
        # the block of the pattern takes the long copy (patterns and filter), the short one (patterns), the long one, the short one
        put("find_sites filtered", ctx.find_sites(pat, host=host, filter=flt).tobytes())
        put("find_sites", ctx.find_sites(pat, host=host).tobytes())
        put("count_sites filtered", _count_sites(ctx, pat, host, filter=flt))
        put("count_sites", _count_sites(ctx, pat, host))
        queries = queries_of_strings(seqs, L)
        score = C.ScoreModel.uniform(L, mismatch=39322)
        put("count_copies", ctx.count_copies(pat, queries, host=host).tobytes())
        put("count_near", ctx.count_near(pat, queries, 2, host=host).tobytes())
        put("score_near", _near_scores(ctx.score_near(pat, queries, 2, score, host=host)))
        put("list_near", _near_list(ctx.list_near(pat, queries, 2, score, limit=1000, host=host)))
        if L == activity.L:
            put("find_sites_scored", [x.tobytes() for x in ctx.find_sites_scored(pat, activity, filter=flt, host=host)])
            put("count_sites_scored", int(ctx.count_sites_scored(pat, activity, min_score=0, host=host)))
        for permille, f in ((0, None), (667, flt)):
            put("find_sites_microhomology %d" % permille,
                [x.tobytes() for x in ctx.find_sites_microhomology(pat, mh, cut_offset=L - 3, min_out_of_frame=permille, filter=f, host=host)])
            put("count_sites_microhomology %d" % permille,
                int(ctx.count_sites_microhomology(pat, mh, cut_offset=L - 3, min_out_of_frame=permille, filter=f, host=host)))
        if ctx.regions is not None:
            for key, call in region_calls(C, ctx, pat, L, host):
                put(key, call())
        spec = C.SitePairs(10, 24, cut_offset=L - 3, orientations="out")
        put("find_site_pairs", [x.tobytes() for x in ctx.find_site_pairs(pat, spec, host=host)])
        n, n_pairs, by = ctx.count_site_pairs(pat, C.SitePairs(0, 40, cut_offset=L - 3, orientations="any"), filter=flt, host=host)
        put("count_site_pairs", [int(n), int(n_pairs), by.tobytes()])
        got = ctx.find_allele_sites(pat, snvs, host=host)
        put("find_allele_sites", [got.sites.tobytes(), got.status.tobytes()])
        n, by, status = ctx.count_allele_sites(pat, snvs, host=host)
        put("count_allele_sites", [int(n), by.tobytes(), status.tobytes()])
        got = ctx.find_edit_sites(pat, edit, snvs, host=host)
        put("find_edit_sites", [got.sites.tobytes(), got.status.tobytes()])
        n, by, status = ctx.count_edit_sites(pat, edit, snvs, host=host)
        put("count_edit_sites", [int(n), by.tobytes(), status.tobytes()])
    if not host:
        guide, params = C.Guide(guide_of_strings(seqs)), C.make_params(max_guide_diffs=2)
        text, rows = ctx.search_hits(guide, "g", params, *STAMP)
        out["search_hits"] = [text, int(rows)]
        table = ctx.search_counts(guide, params)
        out["search_counts"] = [list(table.shape), table.tobytes()]
    return out


def differing(a, b, keys=None):
    """The keys at which two rounds differ (of `keys`, or of either round)."""
    return sorted(k for k in (keys if keys is not None else set(a) | set(b)) if a.get(k) != b.get(k))


# ---- the sequence of references ----

C12 = (["c12"], ["ACGTACGTAGGA"])                 # sites_ref's c12: shorter than any footprint of the round's patterns
LABELS = ("first", "many", "with_u", "first_again", "c12", "host_genome")


def reference_of(label):
    """(names, strings) of a step of the sequence."""
    if label in ("first", "first_again"):
        return E.genome()
    if label == "many":
        return R.many_contigs(5, 70)
    if label == "with_u":
        return E.u_genome()[:2]
    if label == "c12":
        return C12
    if label == "host_genome":
        return R.host_genome()
    raise KeyError(label)


def _strings_label(label):
    return "first" if label == "first_again" else label


_BRUTE = {}


def brute_bytes(C, label, name):
    """The referee's find_sites of a step's reference under a pattern, as the records' bytes: made once per process."""
    key = (_strings_label(label), name)
    if key not in _BRUTE:
        proto, pams, five = R.PATTERNS[name]
        _BRUTE[key] = R.as_records(R.brute_sites(reference_of(label)[1], proto, pams, five), np.dtype(C.aligner.SITE_DTYPE)).tobytes()
    return _BRUTE[key]


def set_step(C, ctx, label, index_path):
    """Takes the context to a step's reference: set_reference, but "first_again" through load_index of the index that "first" saved
    at index_path.  Asserts that the region calls are refused (a new reference drops the set), then sets the step's regions."""
    import pytest
    names, seqs = reference_of(label)
    if label == "first_again":
        ctx.load_index(index_path)
        assert ctx.contig_names == names
    else:
        ctx.set_reference(names, [s.encode() for s in seqs])
    host = ctx.device < 0
    pat = pattern_of(C, "n20_nrg")
    for key, call in region_calls(C, ctx, pat, 20, host):
        with pytest.raises(C.CalitasError) as e:
            call()
        assert e.value.code == C._lib.EINVAL and "no regions" in str(e.value), key
    ctx.set_regions(regions_of_strings(C, names, seqs))
    if label == "first":
        ctx.save_index(index_path)
    return names, seqs


def walk(C, ctx, index_path):
    """One context through the six references, a round after each: {label: round}."""
    host = ctx.device < 0
    out = {}
    for label in LABELS:
        names, seqs = set_step(C, ctx, label, index_path)
        out[label] = round_of(C, ctx, names, seqs, host=host)
    return out


_FRESH = {}


def fresh_round(C, label, device):
    """The round of a step on a context of its own that has seen nothing else: made once per process and device."""
    key = (_strings_label(label), device)
    if key not in _FRESH:
        names, seqs = reference_of(label)
        ctx = C.Context(device)
        try:
            ctx.set_reference(names, [s.encode() for s in seqs])
            ctx.set_regions(regions_of_strings(C, names, seqs))
            _FRESH[key] = round_of(C, ctx, names, seqs, host=device < 0)
        finally:
            ctx.close()
    return _FRESH[key]


# ---- shrinking inside one reference ----

def _distinct_keys(seqs, L, n, seed):
    """n distinct keys of L letters: cuts of the contigs' text first (keys that sites have), drawn ones behind them."""
    rng = random.Random(seed)
    out, seen = [], set()
    for s in seqs:
        for at in range(0, len(s) - L + 1, 5):
            text = _letter(s[at:at + L])
            if set(text) <= set("ACGT") and text not in seen and len(out) < (2 * n) // 3:
                seen.add(text)
                out.append(text)
    while len(out) < n:
        text = "".join(rng.choice("ACGT") for _ in range(L))
        if text not in seen:
            seen.add(text)
            out.append(text)
    return out


def shrink_keys(C, ctx, seqs, host):
    """count_copies and count_near (M = 2) with 600 distinct keys, 1, 5, 500 and 3: a table of 2 048 slots, then of 16 in the same
    allocation, of 1 024, of 16.  The pattern is 32 N's and the 600 hold the key of 32 T's, which the table cannot store."""
    pat = C.Guide("N" * 32)
    keys = _distinct_keys(seqs, 32, 599, 3) + ["T" * 32]
    assert len(set(keys)) == 600
    out = []
    for n in (600, 1, 5, 500, 3):
        q = keys[-n:] if n in (600, 5) else keys[:n]             # (the 600 and the 5 end in the T's)
        out.append(ctx.count_copies(pat, q, host=host).tobytes())
        out.append(ctx.count_near(pat, q, 2, host=host).tobytes())
    return out


def shrink_limit(C, ctx, seqs, host):
    """list_near with limit 1 000, 1, 1 000: FIXED has several copies at d = 0 and at d = 1 in edit_sites_ref.genome()."""
    pat = pattern_of(C, "n20_nrg")
    queries = [R.FIXED, E.FIXED_T] + queries_of_strings(seqs, 20)
    return [_near_list(ctx.list_near(pat, queries, 2, C.ScoreModel.uniform(20, mismatch=39322), limit=limit, host=host)) for limit in (1000, 1, 1000)]


def shrink_snvs(C, ctx, seqs, host):
    """find_allele_sites and find_edit_sites with 700 SNVs, 1, 257 and none."""
    raw = snvs_of_strings(seqs)
    assert len(raw) == 700
    pat, edit = pattern_of(C, "n20_nrg"), E.edit_of(C, EDIT)
    out = []
    for n in (700, 1, 257, 0):
        snvs = E.snv_array(C, raw[:n])
        a, e = ctx.find_allele_sites(pat, snvs, host=host), ctx.find_edit_sites(pat, edit, snvs, host=host)
        out.append([a.sites.tobytes(), a.status.tobytes(), e.sites.tobytes(), e.status.tobytes()])
    return out


def shrink_region(C, ctx, seqs, host):
    """Every listing call over the whole genome, over chrom = 1, start = 10, end = 12 (two bases: nothing fits), over the whole genome.
    The context has a region set.  {call: [whole, empty, whole]}."""
    pat = pattern_of(C, "n20_nrg")
    activity, mh = models(C)
    queries = [R.FIXED] + queries_of_strings(seqs, 20)
    calls = {
        "find_sites": lambda kw: [ctx.find_sites(pat, host=host, **kw).tobytes()],
        "find_sites_scored": lambda kw: [x.tobytes() for x in ctx.find_sites_scored(pat, activity, host=host, **kw)],
        "find_sites_microhomology": lambda kw: [x.tobytes() for x in ctx.find_sites_microhomology(pat, mh, host=host, **kw)],
        "find_sites_regions": lambda kw: [x.tobytes() for x in ctx.find_sites_regions(pat, classes=0b11111, host=host, **kw)],
        "find_site_pairs": lambda kw: [x.tobytes() for x in ctx.find_site_pairs(pat, C.SitePairs(0, 60, orientations="any"), host=host, **kw)],
        "list_near": lambda kw: _near_list(ctx.list_near(pat, queries, 2, limit=1000, host=host, **kw)),
    }
    return {key: [call(kw) for kw in ({}, dict(chrom=1, start=10, end=12), {})] for key, call in calls.items()}


# ---- the calls the library refuses ----

def refusals(C, ctx, names, seqs, host):
    """[(what, refused call, good call)]: each refused call is one the library answers CALITAS_EINVAL to from its plan, before any
    device work; the good call is a call of the same entry point, which returns the same bytes before and after."""
    pat = pattern_of(C, "n20_nrg")
    activity, mh = models(C)
    snvs = E.snv_array(C, snvs_of_strings(seqs, most=100))
    beyond = E.snv_array(C, [(0, 3, "", "A"), (1, len(seqs[1]), "", "A")])
    queries = queries_of_strings(seqs, 20)
    find = lambda pattern=pat, **kw: ctx.find_sites(pattern, host=host, **kw).tobytes()
    allele = lambda v: ctx.find_allele_sites(pat, v, host=host).sites.tobytes()
    scored = lambda m: [x.tobytes() for x in ctx.find_sites_scored(pat, m, host=host)]
    mh_call = lambda m: [x.tobytes() for x in ctx.find_sites_microhomology(pat, m, host=host)]
    near = lambda M: ctx.count_near(pat, queries, M, host=host).tobytes()
    pairs = lambda far: [x.tobytes() for x in ctx.find_site_pairs(pat, C.SitePairs(0, far), host=host)]
    return [
        ("a pattern of 33 bases", lambda: find(pattern=C.Guide("N" * 33 + "nrg")), find),
        ("chrom out of range", lambda: find(chrom=len(names)), find),
        ("a region that ends before it starts", lambda: find(chrom=1, start=50, end=10), lambda: find(chrom=1, start=10, end=500)),
        ("a SNV beyond its contig", lambda: allele(beyond), lambda: allele(snvs)),
        ("an activity model with up = 17", lambda: scored(C.ActivityModel.zeros(20, up=17)), lambda: scored(activity)),
        ("a microhomology model with left = 33", lambda: mh_call(C.MicrohomologyModel(33, 3, [0] * 35)), lambda: mh_call(mh)),
        ("max_mismatches above the limit", lambda: near(4), lambda: near(3)),
        ("a pair spec above CALITAS_PAIR_MAX_DISTANCE", lambda: pairs(C._lib.PAIR_MAX_DISTANCE + 1), lambda: pairs(100)),
    ]


def run_refusals(C, ctx, names, seqs, host):
    """Asserts that each refused call is refused and leaves the good call's bytes as they were; returns the good calls' results."""
    import pytest
    out = []
    for what, bad, good in refusals(C, ctx, names, seqs, host):
        before = good()
        with pytest.raises(C.CalitasError) as e:
            bad()
        assert e.value.code == C._lib.EINVAL, what
        assert good() == before, what
        out.append(before)
    return out


def entry_points(C, ctx, seqs, host):
    """Every entry point of the family as (name, thunk), with arguments that are good for a context holding `seqs`: what a context
    without a reference answers CALITAS_ESTATE to.  count_sites has no host twin and is left out on the host."""
    pat = pattern_of(C, "n20_nrg")
    activity, mh = models(C)
    flt = site_filter(C, 20)
    snvs = E.snv_array(C, snvs_of_strings(seqs, most=50))
    edit = E.edit_of(C, EDIT)
    queries = queries_of_strings(seqs, 20)
    score = C.ScoreModel.uniform(20)
    spec = C.SitePairs(0, 40)
    calls = [("find_sites", lambda: ctx.find_sites(pat, host=host)),
             ("find_sites filtered", lambda: ctx.find_sites(pat, filter=flt, host=host)),
             ("count_copies", lambda: ctx.count_copies(pat, queries, host=host)),
             ("count_near", lambda: ctx.count_near(pat, queries, 2, host=host)),
             ("score_near", lambda: ctx.score_near(pat, queries, 2, score, host=host)),
             ("list_near", lambda: ctx.list_near(pat, queries, 2, score, host=host)),
             ("find_sites_scored", lambda: ctx.find_sites_scored(pat, activity, host=host)),
             ("count_sites_scored", lambda: ctx.count_sites_scored(pat, activity, host=host)),
             ("find_sites_microhomology", lambda: ctx.find_sites_microhomology(pat, mh, host=host)),
             ("count_sites_microhomology", lambda: ctx.count_sites_microhomology(pat, mh, host=host)),
             ("find_sites_regions", lambda: ctx.find_sites_regions(pat, host=host)),
             ("count_sites_regions", lambda: ctx.count_sites_regions(pat, host=host)),
             ("site_presence", lambda: ctx.site_presence()),
             ("find_site_pairs", lambda: ctx.find_site_pairs(pat, spec, host=host)),
             ("count_site_pairs", lambda: ctx.count_site_pairs(pat, spec, host=host)),
             ("find_allele_sites", lambda: ctx.find_allele_sites(pat, snvs, host=host)),
             ("count_allele_sites", lambda: ctx.count_allele_sites(pat, snvs, host=host)),
             ("find_edit_sites", lambda: ctx.find_edit_sites(pat, edit, snvs, host=host)),
             ("count_edit_sites", lambda: ctx.count_edit_sites(pat, edit, snvs, host=host))]
    if not host:
        calls += [("count_sites", lambda: ctx.count_sites(pat)), ("count_sites filtered", lambda: ctx.count_sites(pat, filter=flt))]
    return calls


def assert_no_reference(C, ctx, seqs, host):
    """Every entry point answers CALITAS_ESTATE."""
    import pytest
    for name, call in entry_points(C, ctx, seqs, host):
        with pytest.raises(C.CalitasError) as e:
            call()
        assert e.value.code == C._lib.ESTATE, name


# ---- drawn patterns ----

MAX_L, MAX_PAM, MAX_PAMS, SITE_MAX_FOOT = 32, 16, 8, 48     # what make_guide_host and make_site_patterns take
CODES = "ACGTMRWSYKVHDB"                                     # the IUPAC codes but N
SEED_BASE = 1000
N_DRAWS = 40


def _acceptable(proto, pams):
    return (1 <= len(proto) <= MAX_L and len(pams) <= MAX_PAMS and all(1 <= len(p) <= MAX_PAM and set(p.upper()) != {"N"} for p in pams)
            and len(proto) + max([len(p) for p in pams], default=0) <= SITE_MAX_FOOT)


def draw_pattern(rng):
    """(protospacer, [PAMs], 5' PAM): a protospacer of 1 .. 32 letters, each an N with probability 0.8 and otherwise a drawn IUPAC code;
    0 .. 8 PAMs of 1 .. 16 letters with at least one letter that is no N each, on the 5' or the 3' side.  A draw the library would
    refuse is drawn again."""
    while True:
        letter = lambda: "N" if rng.random() < 0.8 else rng.choice(CODES)
        proto = "".join(letter() for _ in range(rng.randint(1, MAX_L)))
        pams = []
        for _ in range(rng.randint(0, MAX_PAMS)):
            pam = [letter() for _ in range(rng.randint(1, MAX_PAM))]
            if set(pam) == {"N"}:
                pam[rng.randrange(len(pam))] = rng.choice(CODES)
            pams.append("".join(pam).lower())
        five = bool(pams) and rng.random() < 0.5
        if _acceptable(proto, pams):
            return proto, pams, five


def guide_of(C, drawn):
    proto, pams, five = drawn
    first = pams[0] if pams else ""
    return C.Guide((first + proto) if five else (proto + first), pams[1:])


def planted_genome(rng, drawn):
    """(names, strings): two contigs of 2 kb, the first of a length that is no multiple of 32, with two instances of the drawn pattern per
    strand; one per strand lies across a 32-base word boundary (a footprint of one base cannot)."""
    proto, pams, five = drawn
    seqs = [list(R._rand(rng, 2003)), list(R._rand(rng, 2000))]

    def instance():
        pam = rng.choice(pams) if pams else ""
        text = (pam + proto) if five else (proto + pam)
        return "".join(rng.choice(R.IUPAC[c]) for c in text.upper())

    foot = len(proto) + max([len(p) for p in pams], default=0)
    for ci, (straddling, plain) in enumerate((("+", "-"), ("-", "+"))):
        for strand, at in ((straddling, 32 * (9 + ci)), (plain, 1100 + 3 * ci)):
            text = instance()
            if at % 32 == 0:
                at -= len(text) // 2
            R._put(seqs[ci], at, text if strand == "+" else R.revcomp(text))
    assert foot <= SITE_MAX_FOOT
    return ["d0", "d1"], ["".join(s) for s in seqs]


_DRAWS = {}


def draw(C, k):
    """Draw k of the forty: (the drawn pattern, names, strings, the referee's find_sites as tuples), made once per process."""
    if k not in _DRAWS:
        rng = random.Random(SEED_BASE + k)
        drawn = draw_pattern(rng)
        names, seqs = planted_genome(rng, drawn)
        _DRAWS[k] = (drawn, names, seqs, R.brute_sites(seqs, *drawn))
    return _DRAWS[k]


def drawn_snvs(seqs):
    """The SNVs of a draw's allele and edit listings: 150 of snvs_of_strings (the plain-Python contracts they are held against walk
    every start, PAM and letter)."""
    return snvs_of_strings(seqs, most=150)


def drawn_edit(L):
    """C -> T over the whole protospacer."""
    return ("C", "T", (0, L), "N", False, None)
