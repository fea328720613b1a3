"""What the regions tests share: an interval set derived from a text's own rows, so that the edge cases of the class rule are hit by
construction, and the assertions that they are (a test that cannot see them would pass vacuously).

derive_regions(C, rows, lengths, model) gives 8 classes (the most the library takes):

  elsewhere  hits A and B: an interval ENDS exactly at A's coordinate_start and another STARTS exactly at B's coordinate_end
  c1         hit F: starts in a c3 segment and reaches a c1 interval only with its last base; hit E inside the c2 contig
  c2         an interval over a whole contig (with c1 intervals inside); a wide interval over hit J
  c3         a wide interval over hit I (and the segment hit F starts in)
  c4         one-base intervals at the coordinate_start of hit C
  c5         ... and at coordinate_end - 1 of hit D
  c6         an interval across a multiple of 8192 that has hits on both sides; a wide interval over hit H
  c7         one-base intervals at base 0 and at the last base of a contig; a wide interval over hit G

and one contig that has hits keeps no interval at all.  The role hits are imperfect and isolated (no other hit within 12 bases; no interval reaches further than 8), so
an interval meant for one touches no other."""
import collections

MARGIN = 12


def _key(r):
    return r["chromosome"], int(r["coordinate_start"]), int(r["coordinate_end"])


def derive_regions(C, rows, lengths, model, whole_contig=True):
    """(Regions, facts): facts maps a property's name to the rows / numbers that show it; check_regions asserts them."""
    by = collections.defaultdict(list)
    for r in rows:
        by[r["chromosome"]].append(r)
    names = [n for n in lengths if by[n]]

    def isolated(n):
        out = []
        hits = sorted(by[n], key=lambda r: int(r["coordinate_start"]))
        for r in hits:
            a, b = int(r["coordinate_start"]), int(r["coordinate_end"])
            if a < MARGIN or b > lengths[n] - MARGIN or C.score_of_row(r, model) is None:
                continue
            if any(o is not r and int(o["coordinate_start"]) < b + MARGIN and int(o["coordinate_end"]) > a - MARGIN for o in hits):
                continue
            out.append(r)
        return out

    iso = {n: isolated(n) for n in names}
    whole = none = None
    if whole_contig and len(names) >= 3:
        order = sorted(names, key=lambda n: len(iso[n]))        # (the contigs with the most isolated hits do the work)
        none = order[0]
        whole = next(n for n in order[1:] if len(iso[n]) >= 1 and len(by[n]) >= 2)
    work = [n for n in names if n not in (whole, none)]
    iv, facts = [], {}
    # an interval across a multiple of 8192 with hits on both sides of it
    cross = None
    for n in work:
        for m in range(8192, lengths[n] - 200, 8192):
            starts = [int(r["coordinate_start"]) for r in by[n]]
            if any(m - 8192 <= s < m for s in starts) and any(m <= s < m + 8192 for s in starts):
                cross = (n, m)
                break
        if cross:
            break
    # ... and, where the text has one, a hit X that lies ACROSS such a multiple: the interval across the multiple then starts one base
    # before it, and X takes its class from a c4 interval over its first base -- from the segment its coordinate_start lies in, which
    # the coarse entry of its coordinate_end does not lead to
    lo_x = 100
    for n in work:
        for r in by[n]:
            a, b = int(r["coordinate_start"]), int(r["coordinate_end"])
            m = b // 8192 * 8192
            if a + 1 < m < b and 8192 <= m < lengths[n] - 200 and not any(o is not r and int(o["coordinate_start"]) < b + MARGIN and
                                                                          int(o["coordinate_end"]) > a - MARGIN for o in by[n]):
                cross, lo_x = (n, m), 1
                iv.append((n, a - 3, a + 1, "c4"))
                facts["X"] = r
                break
        if "X" in facts:
            break
    if cross:
        iv.append((cross[0], cross[1] - lo_x, cross[1] + 100, "c6"))
        facts["across 8192"] = cross + (lo_x,)
    # the role hits: isolated, imperfect, away from the crossing interval and from each other
    pool = [r for n in work for r in iso[n] if not (cross and n == cross[0] and int(r["coordinate_start"]) < cross[1] + 100 + MARGIN
                                                   and int(r["coordinate_end"]) > cross[1] - 100 - MARGIN)]
    roles = "ABCDFGHIJ"
    assert len(pool) >= len(roles), "the text has %d isolated imperfect hits outside the crossing interval, %d are needed" % (len(pool), len(roles))
    step = len(pool) // len(roles)
    hit = {role: pool[i * step] for i, role in enumerate(roles)}          # (spread over the contigs and both strands)
    for role, r in hit.items():
        n, a, b = _key(r)
        iv += {"A": [(n, a - 7, a, "c3")], "B": [(n, b, b + 7, "c4")], "C": [(n, a, a + 1, "c4")], "D": [(n, b - 1, b, "c5")],
               "F": [(n, a - 2, a + 2, "c3"), (n, b - 1, b + 3, "c1")], "G": [(n, a - 3, b + 3, "c7")], "H": [(n, a - 3, b + 3, "c6")],
               "I": [(n, a - 3, b + 3, "c3")], "J": [(n, a - 8, b + 8, "c2")]}[role]
        facts[role] = r
    if whole:
        e = iso[whole][0]
        n, a, b = _key(e)
        iv += [(whole, 0, lengths[whole], "c2"), (whole, a + 2, a + 5, "c1"), (whole, b + 5, b + 9, "c1")]
        facts["E"], facts["whole"], facts["none"] = e, whole, none
    ends = work[0]
    iv += [(ends, 0, 1, "c7"), (ends, lengths[ends] - 1, lengths[ends], "c7")]
    facts["ends"] = ends
    # the class names in priority order, whatever order the intervals come in (and they come shuffled: any order is allowed)
    reg = C.Regions(iv[::-1][::2] + iv[::-1][1::2], classes=["c%d" % i for i in range(1, 8)])
    return reg, facts


def check_regions(C, rows, reg, facts, model, whole_contig=True):
    """The properties of the input the tests rely on, asserted from the rows and the raw intervals alone."""
    cls = {id(r): C.class_of_row(r, reg) for r in rows}
    iv = reg.intervals
    a_, b_ = facts["A"], facts["B"]
    assert any(c == a_["chromosome"] and e == int(a_["coordinate_start"]) for c, s, e, k in iv) and cls[id(a_)] == 0
    assert any(c == b_["chromosome"] and s == int(b_["coordinate_end"]) for c, s, e, k in iv) and cls[id(b_)] == 0
    c_, d_ = facts["C"], facts["D"]
    assert (c_["chromosome"], int(c_["coordinate_start"]), int(c_["coordinate_start"]) + 1, 4) in iv and cls[id(c_)] == 4
    assert (d_["chromosome"], int(d_["coordinate_end"]) - 1, int(d_["coordinate_end"]), 5) in iv and cls[id(d_)] == 5
    f_ = facts["F"]
    n, a, b = _key(f_)
    assert cls[id(f_)] == 1 and (n, a - 2, a + 2, 3) in iv and (n, b - 1, b + 3, 1) in iv      # c3 at its start, c1 at its last base only
    assert not any(c == n and k == 1 and s < b - 1 and e > a for c, s, e, k in iv)
    if "whole" in facts:
        w = facts["whole"]
        assert any(c == w and s == 0 and k == 2 for c, s, e, k in iv) and cls[id(facts["E"])] == 1
        assert any(r["chromosome"] == w and cls[id(r)] == 2 for r in rows)
        assert not any(c == facts["none"] for c, s, e, k in iv) and any(r["chromosome"] == facts["none"] for r in rows)
    else:                                                    # (fewer than three contigs have hits: no room for these two)
        assert not whole_contig or len({r["chromosome"] for r in rows}) < 3
    assert "across 8192" in facts
    n, m, lo_x = facts["across 8192"]
    assert (n, m - lo_x, m + 100, 6) in iv
    if "X" in facts:                                         # a hit across the multiple, classed by the segment it starts in
        x = facts["X"]
        assert int(x["coordinate_start"]) < m - 1 and m < int(x["coordinate_end"]) and cls[id(x)] == 4
    assert any(r["chromosome"] == n and int(r["coordinate_start"]) < m for r in rows) and any(r["chromosome"] == n and int(r["coordinate_start"]) >= m for r in rows)
    assert any(s == 0 and c == facts["ends"] for c, s, e, k in iv) and any(c == facts["ends"] and e - s == 1 and s > 0 and k == 7 for c, s, e, k in iv)
    assert {r["strand"] for r in rows} == {"+", "-"}
    imperfect = collections.Counter(cls[id(r)] for r in rows if C.score_of_row(r, model) is not None)
    assert all(imperfect[k] >= 1 for k in range(8)), imperfect
    return cls


def striped_regions(C, length, name, width, n_classes=8):
    """Stripes of `width` bases over one contig, classes 1 .. n_classes - 1 and a gap in turn (regions alternating by bin: width 8192)."""
    iv = []
    for i, a in enumerate(range(0, length, width)):
        k = i % n_classes
        if k:
            iv.append((name, a, min(a + width, length), "c%d" % k))
    return C.Regions(iv, classes=["c%d" % i for i in range(1, n_classes)])
