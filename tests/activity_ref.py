"""The referee of the on-target activity tests (test_activity_host.py, test_gpu_activity.py).  It shares no code with the library: the
records are sites_ref.brute_sites', the context of a site is cut from the contig STRINGS with an explicit reverse complement, and the
score is the contract's three sums written out letter by letter in Python integers over models kept as plain lists.  Also the planted
contig, the models and the checks both test files run, on the host twin and on the device."""
import random

import sites_ref as R

NONE = -(1 << 31)
MAX_WEIGHT = 1 << 20
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
N20_NRG = "NNNNNNNNNNNNNNNNNNNNnrg"
HOST_PATTERNS = ("n20_nrg", "tttv_n20", "n21", "n20_nngrrt_nrg", "five16_L32", "one_letter")
CORNERS = ((0, 0), (16, 0), (0, 16), (16, 16))
SWEEP_W = (1, 2, 31, 32, 33, 63, 64)


# ---- the contract, letter by letter ----

def context_of(seq, p, strand, L, up, down):
    """The W letters as the guide reads, upper case and U as T; None when the window leaves the contig."""
    lo, hi = (p - up, p + L + down) if strand == "+" else (p - down, p + L + up)
    if lo < 0 or hi > len(seq):
        return None
    text = seq[lo:hi].upper().replace("U", "T")
    if strand == "-":
        text = "".join(_COMP.get(ch, ch) for ch in reversed(text))
    return text


def score_of(text, m):
    """The score of a context, or NONE when it is None or holds a letter outside A C G T."""
    if text is None or any(ch not in "ACGT" for ch in text):
        return NONE
    up, L = m["up"], m["L"]
    assert len(text) == up + L + m["down"]
    total = m["intercept"]
    for i, ch in enumerate(text):
        total += m["single"][i][_CODE[ch]]
    for i in range(len(text) - 1):
        total += m["pair"][i][4 * _CODE[text[i]] + _CODE[text[i + 1]]]
    gc = 0
    for ch in text[up:up + L]:
        if ch == "G" or ch == "C":
            gc += 1
    return total + m["gc"][gc]


def kind_of(seq, site, m):
    """'scored', 'outside' (the window leaves the contig) or 'letter' (it holds something else than A C G T U)."""
    text = context_of(seq, site[1], site[3], m["L"], m["up"], m["down"])
    if text is None:
        return "outside"
    return "scored" if score_of(text, m) != NONE else "letter"


def scores_of(contigs, sites, m):
    return [score_of(context_of(contigs[s[0]], s[1], s[3], m["L"], m["up"], m["down"]), m) for s in sites]


def expected(contigs, sites, m, min_score=None, scores=None):
    """(the sites kept, their scores): every site without a threshold, those that score at least min_score with one.  scores: what
    scores_of gave for these sites and this model, where a caller has it already."""
    scores = scores_of(contigs, sites, m) if scores is None else scores
    keep = [i for i, s in enumerate(scores) if min_score is None or (s != NONE and s >= min_score)]
    return [sites[i] for i in keep], [scores[i] for i in keep]


# ---- models: plain lists ----

def _model(L, up, down, single=None, pair=None, gc=None, intercept=0, link="identity"):
    W = up + L + down
    return {"L": L, "up": up, "down": down, "intercept": intercept, "link": link,
            "single": single if single is not None else [[0] * 4 for _ in range(W)],
            "pair": pair if pair is not None else [[0] * 16 for _ in range(W - 1)],
            "gc": gc if gc is not None else [0] * (L + 1)}


def distinct(L, up, down, seed=11):
    """Every weight another value out of +-2^19."""
    W = up + L + down
    rng = random.Random(seed * 1000003 + 4096 * L + 64 * up + down)
    draw = rng.sample(range(-(1 << 19), (1 << 19) + 1), 4 * W + 16 * (W - 1) + L + 2)
    take = iter(draw)
    single = [[next(take) for _ in range(4)] for _ in range(W)]
    pair = [[next(take) for _ in range(16)] for _ in range(W - 1)]
    gc = [next(take) for _ in range(L + 1)]
    return _model(L, up, down, single, pair, gc, next(take), "logistic")


def models(L, up, down):
    """name -> model, every kind the issue names; the extremes are the bound at any W."""
    W = up + L + down
    d = distinct(L, up, down)
    flat = lambda v: _model(L, up, down, [[v] * 4 for _ in range(W)], [[v] * 16 for _ in range(W - 1)], [v] * (L + 1), v)   # noqa: E731
    return {"distinct": d, "extremes_plus": flat(MAX_WEIGHT), "extremes_minus": flat(-MAX_WEIGHT),
            "single_only": _model(L, up, down, single=d["single"]), "pair_only": _model(L, up, down, pair=d["pair"]),
            "gc_only": _model(L, up, down, gc=d["gc"]), "intercept_only": _model(L, up, down, intercept=d["intercept"]),
            "zeros": _model(L, up, down)}


MODEL_NAMES = tuple(models(1, 0, 0))


def model_of(C, m):
    import numpy as np
    pair = np.array(m["pair"], dtype=np.int64).reshape(-1, 16)           # (W = 1: no row)
    return C.ActivityModel(m["L"], m["up"], m["down"], m["single"], pair, m["gc"], m["intercept"], m["link"])


def with_exact_pair(m, contigs, sites):
    """A copy of the model with one `single` weight moved so that some site scores exactly one more than another, and that higher
    score: the threshold some site meets exactly while another has exactly one less.  The two are neighbours in score order, so the
    move is small; the weight is one the higher site's context reads and the lower one's does not."""
    L, up, down = m["L"], m["up"], m["down"]
    texts = {context_of(contigs[s[0]], s[1], s[3], L, up, down) for s in sites}
    rows = sorted(row for row in ((score_of(text, m), text) for text in texts) if row[0] != NONE)
    best = None
    for (lo, text_lo), (hi, text_hi) in zip(rows, rows[1:]):
        if best is None or hi - lo < best[0]:
            best = (hi - lo, text_lo, text_hi, hi)
    assert best is not None, "fewer than two distinct scored contexts"
    gap, text_lo, text_hi, hi = best
    at = next(i for i in range(len(text_hi)) if text_lo[i] != text_hi[i])
    out = dict(m, single=[list(row) for row in m["single"]])
    out["single"][at]["ACGT".index(text_hi[at])] += 1 - gap   # the higher one comes down to the lower one's score + 1
    assert abs(out["single"][at]["ACGT".index(text_hi[at])]) <= MAX_WEIGHT
    return out, hi + 1 - gap


class Floors(dict):
    """name -> threshold; .scores: scores_of for the sites and the model they were taken from (hold's `scores`)."""


def decimal_of(q16):
    """The shortest decimal a tool's flag turns into this Q16 number: floor(x * 65536 + 0.5)."""
    import math
    for digits in range(1, 13):
        text = "%.*f" % (digits, q16 / 65536.0)
        if math.floor(float(text) * 65536.0 + 0.5) == q16:
            return text
    raise ValueError(q16)


def thresholds(contigs, sites, m):
    """(the model to use, {name: threshold}) with the properties the tests rely on asserted on the referee alone."""
    m2, exact = with_exact_pair(m, contigs, sites)
    scores = scores_of(contigs, sites, m2)
    scored = sorted(s for s in scores if s != NONE)
    assert exact in scored and exact - 1 in scored
    kept = sum(1 for s in scored if s >= exact)
    assert 1 <= kept <= len(sites) - 1
    floors = Floors({"exact": exact, "half": scored[len(scored) // 2], "tenth": scored[(9 * len(scored)) // 10], "above": scored[-1] + 1, "all": None})
    floors.scores = scores
    return m2, floors


# ---- the planted contig ----

def planted(up=4, down=6, seed=5):
    """A contig for N20 + nrg patterns and a model with these flanks.  Returns (name, string, {what: (protospacer start, strand)}):
    clean windows that touch the contig's first and last base exactly and ones a base short of them, on both strands; windows with an
    N, an R and an n outside the footprint; a U / u in the flank only and in the footprint, on both strands; a soft-masked window; a
    footprint whose nngrrt PAM ends on a U while its nrg PAM is clean."""
    rng = random.Random(seed)
    n = 1300
    a = [rng.choice("ACGT") for _ in range(n)]
    put = lambda at, what: R._put(a, at, what)                # noqa: E731
    where = {}
    # '+' at p: nrg at p + 20; '-' at p: its reverse complement, cyn, at p - 3
    lo_plus, lo_minus = max(up, 1), max(down, 4)
    put(lo_plus - 1 + 20, "GGGG"); where["first_plus"], where["first_plus_short"] = (lo_plus, "+"), (lo_plus - 1, "+")
    put(lo_minus - 1 - 3, "CCCC"); where["first_minus"], where["first_minus_short"] = (lo_minus, "-"), (lo_minus - 1, "-")
    hi_plus, hi_minus = n - 20 - max(down, 3), n - 20 - up
    put(hi_plus + 20, "GGGG"[:n - hi_plus - 20]); where["last_plus"], where["last_plus_short"] = (hi_plus, "+"), (hi_plus + 1, "+")
    put(hi_minus - 3, "CCCC"); where["last_minus"], where["last_minus_short"] = (hi_minus, "-"), (hi_minus + 1, "-")
    for p in (100, 200, 300, 400, 500, 600, 900):
        put(p + 20, "AGG")
    for p in (700, 800):
        put(p - 3, "CCA")
    if up >= 2:
        put(100 - 2, "N"); where["N_outside"] = (100, "+")
        put(300 - 1, "n"); where["n_outside"] = (300, "+")
        put(400 - min(up, 3), "U"); where["U_flank"] = (400, "+")
        put(800 + 20 + min(up, 2) - 1, "U"); where["U_flank_minus"] = (800, "-")
    if down >= 5:
        put(200 + 24, "R"); where["R_outside"] = (200, "+")
        put(500 + 20 + min(down, 6) - 1, "u"); where["u_flank"] = (500, "+")
    put(600 + 5, "U"); where["U_footprint"] = (600, "+")
    put(700 + 10, "u"); where["u_footprint_minus"] = (700, "-")
    put(880, "".join(a[880:950]).lower()); where["soft_masked"] = (900, "+")
    put(1000 + 20, "AGGAGU"); where["U_in_long_pam"] = (1000, "+")
    return "planted", "".join(a), where


def host_contigs(up=4, down=6):
    """sites_ref.host_genome plus the planted contig: (names, strings, where, index of the planted contig)."""
    names, seqs = R.host_genome()
    name, seq, where = planted(up, down)
    return names + [name], seqs + [seq], where, len(names)


def check_planted(contigs, index, where, sites, m):
    """On the referee alone: the planted cases are what they were planted as, and each kind of unscored site occurs."""
    seq = contigs[index]
    at = {(s[1], s[3]): s for s in sites if s[0] == index}
    kinds = {what: kind_of(seq, at[place], m) for what, place in where.items() if place in at}
    for what in ("first_plus", "first_minus", "last_plus", "last_minus", "soft_masked"):
        assert kinds.get(what) == "scored", (what, kinds)
    up, L, down = m["up"], m["L"], m["down"]
    if up >= 1:
        assert kinds["first_plus_short"] == "outside" and kinds["last_minus_short"] == "outside", kinds
        p, _ = where["first_plus"]
        assert p - up == 0
        p, _ = where["last_minus"]
        assert p + L + up == len(seq)
    if down >= 4:
        assert kinds["first_minus_short"] == "outside" and kinds["last_plus_short"] == "outside", kinds
        assert where["first_minus"][0] - down == 0 and where["last_plus"][0] + L + down == len(seq)
    for what in ("N_outside", "n_outside", "R_outside"):
        if what in where:
            assert kinds[what] == "letter", (what, kinds)
    for what in ("U_flank", "U_flank_minus", "u_flank", "U_footprint", "u_footprint_minus", "U_in_long_pam"):
        if what in where:
            assert kinds[what] == "scored", (what, kinds)
    every = {kind_of(contigs[s[0]], s, m) for s in sites}
    if up + down >= 1:
        assert every == {"scored", "outside", "letter"}, every
    return kinds


def check_sensitive(contigs, index, where, sites, m):
    """The distinct model tells apart what must be told apart: on the planted sites a window one base further, the other strand's
    reading of the same bases and a transposed pair of letters all give another integer."""
    seq = contigs[index]
    L, up, down = m["L"], m["up"], m["down"]
    seen = 0
    for what in ("soft_masked", "first_plus", "last_minus"):
        p, strand = where[what]
        text = context_of(seq, p, strand, L, up, down)
        score = score_of(text, m)
        assert score != NONE
        step = 1 if what != "last_minus" else -1
        moved = score_of(context_of(seq, p + step, strand, L, up, down), m)
        other = "".join(_COMP[ch] for ch in reversed(text))
        assert moved != NONE and moved != score and score_of(other, m) != score
        for i in range(len(text) - 1):
            if text[i] != text[i + 1]:
                swapped = text[:i] + text[i + 1] + text[i] + text[i + 2:]
                assert score_of(swapped, m) != score
                seen += 1
    assert seen >= 10


# ---- the checks both files run ----

def pattern_of(C, name):
    text, aux = R.pattern_string(name)
    return C.Guide(text, aux)


def call(C, ctx, pattern, m, min_score, host, **kw):
    return ctx.find_sites_scored(pattern, model_of(C, m), min_score=min_score, host=host, **kw)


def hold(C, ctx, contigs, pattern, sites, m, min_score, hosts, scores=None, **kw):
    """find_sites_scored on every path of `hosts` (True: the twin, False: the device) against the referee; the paths' bytes agree.
    Returns the number of sites kept."""
    import numpy as np
    want_sites, want_scores = expected(contigs, sites, m, min_score, scores)
    want = R.as_records(want_sites, C.aligner.SITE_DTYPE).tobytes()
    got = None
    for host in hosts:
        got_sites, got_scores = call(C, ctx, pattern, m, min_score, host, **kw)
        assert got_scores.dtype == np.int32 and len(got_scores) == len(got_sites)
        assert got_scores.tolist() == want_scores, (host, min_score, _first_difference(got_scores.tolist(), want_scores))
        assert np.asarray(got_sites).tobytes() == want, (host, min_score)
        pair = (np.asarray(got_sites).tobytes(), got_scores.tobytes())
        assert got is None or got == pair
        got = pair
    return len(want_scores)


def _first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i, x, y
    return min(len(a), len(b)), len(a), len(b)


def sweep_cases():
    """(W, up, down, L) for W in SWEEP_W and the four corners, where a protospacer of 1 .. 32 bases is left."""
    return [(W, up, down, W - up - down) for W in SWEEP_W for up, down in CORNERS if 1 <= W - up - down <= 32]


def sweep_contigs():
    """The planted contig for the widest flanks, and the short contigs of the host genome: PAM-less patterns match everywhere."""
    names, seqs = R.host_genome()
    name, seq, _ = planted(16, 16)
    return [name] + names[2:4], [seq] + seqs[2:4]


def pamless_sites(contigs, L):
    return R.brute_sites(contigs, "N" * L, [], False)


def hold_errors(C, ctx, host):
    """The errors in their order: what find_sites refuses, then the model field by field; ENODEV (the device call on a host-only
    context) comes after both and is the caller's to check."""
    import numpy as np
    m = model_of(C, distinct(20, 4, 6))

    def fails(code, word, pattern=N20_NRG, model=m, **kw):
        try:
            ctx.find_sites_scored(pattern, model, host=host, **kw)
        except C.CalitasError as e:
            assert e.code == code and word in str(e), (code, word, str(e))
        else:
            raise AssertionError("no error: " + word)

    EINVAL = C._lib.EINVAL
    bad = C.ActivityModel.zeros(21, 4, 6)
    fails(EINVAL, "chrom_index", chrom=99, model=bad)                                      # the region before the model
    fails(EINVAL, "non-IUPAC", pattern="NNNNNNNNNNNNNNNNNNNJnrg", model=bad)
    fails(EINVAL, "gc_min", model=bad, filter=C.SiteFilter(gc_min=21))                     # the filter before the model
    fails(EINVAL, "model is NULL", model=None)
    fails(EINVAL, "protospacer_length", model=bad)
    for field, value in (("up", 17), ("up", -1), ("down", 17), ("down", -1)):
        wrong = C.ActivityModel.zeros(20, 4, 6)
        setattr(wrong, field, value)                                                       # (the arrays keep their size: the field is refused first)
        fails(EINVAL, "%s is %d" % (field, value), model=wrong)
        wrong.L = 21                                                                       # the length before the flanks
        fails(EINVAL, "protospacer_length", model=wrong)
    wrong = C.ActivityModel.zeros(20, 4, 6)
    wrong.to_c = lambda: _with(C.ActivityModel.zeros(20, 4, 6).to_c(), "link", 2)
    fails(EINVAL, "link is 2", model=wrong)
    for field, index in (("single", 7), ("pair", 100), ("gc", 20)):
        for value in (MAX_WEIGHT + 1, -MAX_WEIGHT - 1):
            wrong = C.ActivityModel.zeros(20, 4, 6)
            getattr(wrong, field).reshape(-1)[index] = value
            wrong.intercept = 0
            fails(EINVAL, "%s[%d]" % (field, index), model=wrong)
        ok = C.ActivityModel.zeros(20, 4, 6)
        getattr(ok, field).reshape(-1)[index] = -MAX_WEIGHT
        ctx.find_sites_scored(N20_NRG, ok, host=host, chrom=2)
    wrong = C.ActivityModel.zeros(20, 4, 6)
    wrong.intercept = MAX_WEIGHT + 1
    wrong.single[0, 0] = MAX_WEIGHT + 1                                                    # the intercept before the tables
    fails(EINVAL, "intercept", model=wrong)
    for table in ("single", "pair", "gc"):
        wrong = C.ActivityModel.zeros(20, 4, 6)
        wrong.to_c = lambda table=table: _with(C.ActivityModel.zeros(20, 4, 6).to_c(), table, None)
        fails(EINVAL, table + " is NULL", model=wrong)
    assert np.int32(NONE) == NONE


def _with(c_model, field, value):
    import ctypes
    setattr(c_model, field, ctypes.POINTER(ctypes.c_int32)() if value is None else value)
    return c_model
