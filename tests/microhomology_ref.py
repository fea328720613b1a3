"""The referee of the microhomology tests (test_microhomology_host.py, test_gpu_microhomology.py): the contract of
calitas_find_sites_microhomology over strings, sharing no code with the library.  Windows are cut from the contig strings around the
sites sites_ref.brute_sites lists; `walk` goes along every diagonal letter by letter; `literal` enumerates every pair of equal k-mers
either side of the cut and drops the ones nested in a longer pair on the same diagonal (cubic: used on a sample).  The genome has three
contigs: 900 random bases, 3 kb with the planted cases, 60 bases that begin and end in a site."""
import math
import random

import sites_ref as R

NONE = 0xFFFFFFFF
UNSCORED = (NONE, NONE)
MAX_WEIGHT = 1 << 16
N20_NRG = "NNNNNNNNNNNNNNNNNNNNnrg"
PATTERNS = ("n20_nrg", "tttv_n20")                     # a 3' and a 5' PAM
WINDOWS = ((1, 1), (1, 32), (32, 1), (30, 30), (32, 32))
EDGE_WINDOWS = ((17, 6), (18, 6), (17, 7))             # with cut 17: the planted edge sites' windows fit exactly, or leave by one base
MIN_LENGTHS = (2, 3, 8)
PERMILLES = (0, 1, 667, 1000)
L = 20
CUT = L - 3
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def cuts():
    return (0, L - 3, L)


# ---- the contract, letter by letter ----

def window_of(seq, p, strand, cut, left, right):
    """The W letters as the guide reads, upper case and U as T; None when the window leaves the contig."""
    if strand == "+":
        c = p + cut
        lo, hi = c - left, c + right
    else:
        c = p + L - cut
        lo, hi = c - right, c + left
    if lo < 0 or hi > len(seq):
        return None
    text = seq[lo:hi].upper().replace("U", "T")
    if strand == "-":
        text = "".join(_COMP.get(ch, ch) for ch in reversed(text))
    return text


def runs(x, left, min_length):
    """[(d, first position, length)] of every microhomology: the maximal runs of x[i] == x[i + d] within [lo(d), hi(d))."""
    W, out = len(x), []
    for d in range(1, W):
        lo, hi = max(0, left - d), min(left, W - d)
        i = lo
        while i < hi:
            if x[i] != x[i + d]:
                i += 1
                continue
            j = i
            while j < hi and x[j] == x[j + d]:
                j += 1
            if j - i >= min_length:
                out.append((d, i, j - i))
            i = j
    return out


def walk(x, left, m):
    """(total_q16, out_of_frame_q16) of a window, or UNSCORED when it is None or holds a letter outside A C G T."""
    if x is None or any(ch not in "ACGT" for ch in x):
        return UNSCORED
    total = oof = 0
    for d, i, k in runs(x, left, m["min_length"]):
        term = m["weight"][d - 1] * (k + sum(1 for ch in x[i:i + k] if ch in "GC"))
        total += term
        if d % 3:
            oof += term
    return total, oof


def literal(x, left, m):
    """The same numbers the long way: every (i, j, k) with the k-mer at i wholly left of the cut, the k-mer at j wholly right of it and
    the two equal, k >= min_length; a pair nested in a longer pair of the same deletion length j - i is dropped."""
    if x is None or any(ch not in "ACGT" for ch in x):
        return UNSCORED
    W = len(x)
    pairs = [(i, j, k) for k in range(m["min_length"], left + 1) for i in range(0, left - k + 1) for j in range(left, W - k + 1)
             if x[i:i + k] == x[j:j + k]]
    total = oof = 0
    for i, j, k in pairs:
        if any(j2 - i2 == j - i and k2 > k and i2 <= i and i + k <= i2 + k2 for i2, j2, k2 in pairs):
            continue
        term = m["weight"][j - i - 1] * (k + sum(1 for ch in x[i:i + k] if ch in "GC"))
        total += term
        if (j - i) % 3:
            oof += term
    return total, oof


def scores_of(contigs, sites, cut, m):
    return [walk(window_of(contigs[s[0]], s[1], s[3], cut, m["left"], m["right"]), m["left"], m) for s in sites]


def kept(score, permille):
    if permille == 0:
        return True
    return score != UNSCORED and score[0] > 0 and score[1] * 1000 >= permille * score[0]


# ---- models ----

def model(left, right, min_length, weight):
    assert len(weight) == left + right - 1
    return {"left": left, "right": right, "min_length": min_length, "weight": list(weight)}


def unit(left, right, min_length=2):
    return model(left, right, min_length, [MAX_WEIGHT] * (left + right - 1))


def exponential(left, right, min_length=2, tau=20.0):
    return model(left, right, min_length, [int(math.floor(math.exp(-d / tau) * 65536.0 + 0.5)) for d in range(1, left + right)])


def distinct(left, right, min_length=2, seed=23):
    """Every deletion length another weight, 0 and 65536 among them."""
    rng = random.Random(seed * 1000003 + 64 * left + right)
    w = [rng.randrange(1, MAX_WEIGHT) for _ in range(left + right - 1)]
    w[rng.randrange(len(w))] = 0
    w[rng.randrange(len(w))] = MAX_WEIGHT
    return model(left, right, min_length, w)


def model_of(C, m):
    return C.MicrohomologyModel(m["left"], m["right"], m["weight"], m["min_length"])


# ---- the genome ----

def _rand(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def _put(seq, at, what):
    assert 0 <= at and at + len(what) <= len(seq)
    seq[at:at + len(what)] = list(what)


M6 = "TCGGAT"                                          # M6[1:4] is the PAM of the sites it is planted in


def genome(seed=41):
    """(names, strings, where): where[what] = (protospacer start, strand) of a planted N20 + nrg site of the contig `planted`, cut 17.
    Every planted site is a '+' site unless its name says otherwise; c is its forward cut, p + 17."""
    rng = random.Random(seed)
    a = _rand(rng, 900)
    b = list(_rand(rng, 3000))
    where = {}
    _put(b, 200, "G" * 80)                                                  # 64 G's around the cut of the sites at 215 .. 231
    where["poly_g"] = (220, "+")
    c = 500 + CUT                                                           # the 6-mer at [c - 7, c - 1) and at [c + 2, c + 8): d = 9
    _put(b, c - 8, "A" + M6 + "A" + "T" + "C" + M6 + "C")
    where["repeat_d9"] = (500, "+")
    c = 600 + CUT                                                           # ... at [c - 8, c - 2) and at [c + 2, c + 8): d = 10
    _put(b, c - 9, "A" + M6 + "A" + "TT" + "C" + M6 + "C")
    where["repeat_d10"] = (600, "+")
    c = 700 + CUT                                                           # period 5 from c - 3 to c + 6: the run of d = 5 would go on past the cut
    _put(b, c - 4, "C" + "ACAGT" + "ACAGT")
    where["clipped"] = (700, "+")
    c = 800 + CUT                                                           # GC at [c - 2, c) and at [c + 5, c + 7), nothing more: d = 7, k = 2
    _put(b, c - 3, "C" + "GC" + "TTTT" + "A" + "GC")
    where["short_run"] = (800, "+")
    c = 900 + CUT                                                           # A and C left of the cut, G and T right of it: no match anywhere
    _put(b, c - 32, _rand(rng, 32, "AC") + _rand(rng, 4, "GT") + "GG" + _rand(rng, 26, "GT"))
    where["total_0"] = (900, "+")
    q = 1300                                                                # an N: the last base of one site's 30 + 30 window, a base beyond the next one's
    _put(b, q - 47 + 20, "AGGG")
    _put(b, q, "N")
    where["n_beside"] = (q - 47, "+")                                       # c + 30 == q
    where["n_inside"] = (q - 46, "+")                                       # c + 29 == q
    _put(b, 1500 + 20, "TGG")
    _put(b, 1500 + CUT + 10, "U")                                           # a U in the window, outside the footprint
    where["u_flank"] = (1500, "+")
    _put(b, 1600 + 20, "TGG")
    _put(b, 1600 + 5, "u")                                                  # ... and in the footprint
    where["u_foot"] = (1600, "+")
    _put(b, 1700 + 20, "AGG")
    _put(b, 1700 + CUT + 12, "R")                                           # an IUPAC code of the reference
    where["r_flank"] = (1700, "+")
    _put(b, 1800, "".join(b[1800:1900]).lower())                            # soft-masked
    _put(b, 1830 + 20, "cgg")
    where["soft"] = (1830, "+")
    _put(b, 20, "AGG")                                                      # '+' on the first base: c = 17, 17 bases left of it
    where["first_plus"] = (0, "+")
    _put(b, len(b) - 23, "CCT")                                             # '-' on the last base: c = len - 17
    where["last_minus"] = (len(b) - 20, "-")
    t = list(_rand(rng, 60))
    _put(t, 0, "CCA")                                                       # '-' on the first base: c = 6
    _put(t, 57, "TGG")                                                      # '+' on the last base: c = 54
    where["tail_first_minus"] = (3, "-")
    where["tail_last_plus"] = (37, "+")
    return ["rand", "planted", "tail"], [a, "".join(b), "".join(t)], where


def check_planted(contigs, where, sites):
    """On the referee alone: the planted cases are what they were planted as."""
    at = {(s[0], s[1], s[3]) for s in sites}
    for what, (p, strand) in where.items():
        assert ((2 if what.startswith("tail") else 1), p, strand) in at, what
    seq = contigs[1]
    win = lambda what, left, right: window_of(seq, where[what][0], where[what][1], CUT, left, right)   # noqa: E731
    g = win("poly_g", 32, 32)
    assert g == "G" * 64 and walk(g, 32, unit(32, 32)) == (133955584, 89391104)
    assert (9, 30 - 7, 6) in runs(win("repeat_d9", 30, 30), 30, 2) and (10, 30 - 8, 6) in runs(win("repeat_d10", 30, 30), 30, 2)
    only9, only10 = model(30, 30, 2, [0] * 8 + [MAX_WEIGHT] + [0] * 50), model(30, 30, 2, [0] * 9 + [MAX_WEIGHT] + [0] * 49)
    t9, t10 = walk(win("repeat_d9", 30, 30), 30, only9), walk(win("repeat_d10", 30, 30), 30, only10)
    assert t9[0] >= 9 * MAX_WEIGHT and t9[1] == 0 and t10[0] == t10[1] >= 9 * MAX_WEIGHT          # k + g = 6 + 3; 9 is in frame, 10 is not
    x = win("clipped", 30, 30)
    assert (5, 27, 3) in runs(x, 30, 2) and x[30] == x[35] and x[31] == x[36]                      # it would be 5 long
    x = win("short_run", 30, 30)
    assert (7, 28, 2) in runs(x, 30, 2) and not [r for r in runs(x, 30, 3) if r[0] == 7 and r[1] <= 28 < r[1] + r[2]]
    assert walk(win("total_0", 30, 30), 30, unit(30, 30)) == (0, 0) == walk(win("total_0", 32, 32), 32, unit(32, 32))
    assert "N" in win("n_inside", 30, 30) and walk(win("n_inside", 30, 30), 30, unit(30, 30)) == UNSCORED
    assert "N" not in win("n_beside", 30, 30) and walk(win("n_beside", 30, 30), 30, unit(30, 30)) != UNSCORED
    assert "N" in win("n_beside", 30, 31)
    assert "U" in seq[1500:1560] and walk(win("u_flank", 30, 30), 30, unit(30, 30)) != UNSCORED
    assert "u" in seq[1600:1623] and walk(win("u_foot", 30, 30), 30, unit(30, 30)) != UNSCORED
    assert walk(win("r_flank", 30, 30), 30, unit(30, 30)) == UNSCORED != walk(win("r_flank", 30, 12), 30, unit(30, 12))
    assert win("soft", 30, 30).isupper() and seq[1830:1853].islower()
    # the contig's ends, by one base, on both strands
    assert win("first_plus", 17, 6) is not None and win("first_plus", 18, 6) is None
    assert win("last_minus", 17, 6) is not None and win("last_minus", 18, 6) is None
    tail = contigs[2]
    assert window_of(tail, 3, "-", CUT, 17, 6) is not None and window_of(tail, 3, "-", CUT, 17, 7) is None
    assert window_of(tail, 37, "+", CUT, 17, 6) is not None and window_of(tail, 37, "+", CUT, 17, 7) is None


_cache = {}


def the_genome():
    if "genome" not in _cache:
        _cache["genome"] = genome()
    return _cache["genome"]


def the_sites(name, chrom=None, start=0, end=None):
    key = ("sites", name, chrom, start, end)
    if key not in _cache:
        _cache[key] = R.brute_sites(the_genome()[1], *R.PATTERNS[name], chrom=chrom, start=start, end=end)
    return _cache[key]


def the_scores(name, cut, m, chrom=None, start=0, end=None):
    """The referee's scores of the_sites(name, ...) under m, computed once."""
    key = ("scores", name, cut, m["left"], m["right"], m["min_length"], tuple(m["weight"]), chrom, start, end)
    if key not in _cache:
        _cache[key] = scores_of(the_genome()[1], the_sites(name, chrom, start, end), cut, m)
    return _cache[key]


def region_with(name, chrom, n):
    """(start, end) of a region of contig `chrom` that holds exactly n sites of the pattern."""
    sites = the_sites(name, chrom)
    proto, pams, five = R.PATTERNS[name]
    feet = []
    for s in sites:
        lo = min(s[1], s[2]) if s[2] >= 0 else s[1]
        feet.append((lo, lo + len(proto) + s[5]))
    for start in range(0, 40):
        for end in sorted({hi for _, hi in feet}):
            if sum(1 for lo, hi in feet if lo >= start and hi <= end) == n:
                return start, end
    raise AssertionError("no region of contig %d holds exactly %d sites" % (chrom, n))


# ---- the library against the referee ----

def pattern_of(C, name):
    text, aux = R.pattern_string(name)
    return C.Guide(text, aux)


def hold(C, ctx, name, m, cut, permille, hosts, scores=None, sites=None, **kw):
    """find_sites_microhomology on every path of `hosts` (True: the twin, False: the device) against the referee, in records and in
    scores; so the paths' bytes agree.  Returns the number of sites kept."""
    import numpy as np
    region = (kw.get("chrom"), kw.get("start", 0), kw.get("end"))
    sites = the_sites(name, *region) if sites is None else sites
    scores = the_scores(name, cut, m, *region) if scores is None else scores
    keep = [i for i, s in enumerate(scores) if kept(s, permille)]
    want_sites = R.as_records([sites[i] for i in keep], C.aligner.SITE_DTYPE)
    want_scores = np.array([scores[i] for i in keep], dtype=C.aligner.MH_SCORE_DTYPE)
    for host in hosts:
        got_sites, got_scores = ctx.find_sites_microhomology(pattern_of(C, name), model_of(C, m), cut, permille, host=host, **kw)
        what = (name, m["left"], m["right"], m["min_length"], cut, permille, "twin" if host else "device")
        assert len(got_sites) == len(keep) == len(got_scores), (what, len(got_sites), len(keep))
        if got_scores.tobytes() != want_scores.tobytes():
            i = next(i for i in range(len(keep)) if tuple(got_scores[i]) != tuple(want_scores[i]))
            raise AssertionError((what, "site", sites[keep[i]], "got", tuple(got_scores[i]), "want", tuple(want_scores[i])))
        assert got_sites.tobytes() == want_sites.tobytes(), what
        assert ctx.count_sites_microhomology(pattern_of(C, name), model_of(C, m), cut, permille, host=host, **kw) == len(keep), what
    return len(keep)


def hold_errors(C, ctx, host):
    """The errors in their order: what find_sites_filtered refuses, then the model field by field, then the per-mille; ENODEV (the device
    call on a host-only context) comes after all of them and is the caller's to check."""
    import ctypes
    good = model_of(C, unit(30, 30))

    def fails(code, word, pattern=N20_NRG, model=good, cut=CUT, permille=0, **kw):
        try:
            ctx.find_sites_microhomology(pattern, model, cut, permille, host=host, **kw)
        except C.CalitasError as e:
            assert e.code == code and word in str(e), (code, word, str(e))
        else:
            raise AssertionError("no error: " + word)

    def wrong(**fields):
        m = model_of(C, unit(30, 30))
        for k, v in fields.items():
            setattr(m, k, v)                            # (the array keeps its size: the field is refused before a weight is read)
        return m

    EINVAL = C._lib.EINVAL
    bad = wrong(left=0)
    fails(EINVAL, "chrom_index", chrom=99, model=bad)                                      # the region before the model
    fails(EINVAL, "non-IUPAC", pattern="NNNNNNNNNNNNNNNNNNNJnrg", model=bad)
    fails(EINVAL, "gc_min", model=bad, filter=C.SiteFilter(gc_min=21))                     # the filter before the model
    fails(EINVAL, "model is NULL", model=None, permille=2000)
    null = model_of(C, unit(30, 30))
    null.to_c = lambda cut: _without_weight(model_of(C, unit(30, 30)).to_c(cut), ctypes)
    fails(EINVAL, "weight is NULL", model=null, cut=21)
    for value in (0, 33, -1):
        fails(EINVAL, "left is %d" % value, model=wrong(left=value, right=0), cut=21)      # left before right, cut_offset and the rest
        fails(EINVAL, "right is %d" % value, model=wrong(right=value, min_length=1), cut=21)
    for value in (-1, 21):
        fails(EINVAL, "cut_offset is %d" % value, model=wrong(min_length=9), cut=value)
    for value in (1, 9):
        heavy = wrong(min_length=value)
        heavy.weight[3] = MAX_WEIGHT + 1
        fails(EINVAL, "min_length is %d" % value, model=heavy)                             # min_length before the weights
    for index in (0, 31, 58):
        heavy = wrong()
        heavy.weight[index] = MAX_WEIGHT + 1
        fails(EINVAL, "weight[%d]" % index, model=heavy, permille=1001)                    # the weights before the per-mille
    for value in (-1, 1001):
        fails(EINVAL, "permille is %d" % value, permille=value)
    for c in (0, 20):                                                                      # the limits themselves pass
        ctx.find_sites_microhomology(N20_NRG, model_of(C, unit(32, 32, 8)), c, 1000, host=host, chrom=2)
    ctx.find_sites_microhomology(N20_NRG, model_of(C, unit(1, 1)), 0, 0, host=host, chrom=2)


def _without_weight(c_model, ctypes):
    c_model.weight = ctypes.POINTER(ctypes.c_uint32)()
    return c_model
