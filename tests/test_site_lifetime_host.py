"""CPU tests of what a long-lived context keeps between the guide-site calls (site_lifetime_util.py): one host-only context through the
six references, a round of every entry point after each, against the referee and a context of its own per reference -- which holds the
context's own presence table, kept per region set and reference, and the inputs of test_gpu_site_lifetime.py; the calls that shrink
inside one reference, the refused calls, a context without a reference, and forty drawn patterns against the referee."""
import random

import numpy as np
import pytest

import allele_sites_ref as A
import edit_sites_ref as E
import site_lifetime_util as U
import sites_ref as R


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


@pytest.fixture(scope="module")
def walked(C, tmp_path_factory):
    """{label: round} of one Context(-1) taken through the sequence."""
    ctx = C.Context(-1)
    try:
        return U.walk(C, ctx, str(tmp_path_factory.mktemp("lifetime") / "first.idx"))
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def first(C):
    """(a host-only context that holds the first reference and its regions, names, strings)"""
    names, seqs = U.reference_of("first")
    ctx = C.Context(-1)
    ctx.set_reference(names, [s.encode() for s in seqs])
    ctx.set_regions(U.regions_of_strings(C, names, seqs))
    yield ctx, names, seqs
    ctx.close()


@pytest.mark.parametrize("label", U.LABELS)
def test_one_host_context_through_the_sequence(C, walked, label):
    got = walked[label]
    want = U.fresh_round(C, label, -1)
    assert U.differing(got, want) == []
    for name in U.PATTERN_NAMES:
        assert got["find_sites/" + name] == U.brute_bytes(C, label, name), name
        assert (len(got["find_sites/" + name]) > 0) == (label != "c12"), name
        assert 0 < len(got["find_sites filtered/" + name]) < len(got["find_sites/" + name]) or label in ("c12", "with_u") or name == "max48"
        assert "find_sites_regions/" + name in got and "search_hits" not in got
    if label != "c12":
        for key in ("list_near", "find_site_pairs", "find_allele_sites", "find_edit_sites", "find_sites_regions"):
            assert all(len(x) for x in got[key + "/n20_nrg"]), key
    else:                                                # nothing fits 12 bases: every listing is empty, every SNV is examined
        for key, value in got.items():
            if key.startswith(("find_sites", "find_site_pairs")):
                assert not any(len(x) for x in ([value] if isinstance(value, bytes) else value)), key
        assert got["find_allele_sites/n20_nrg"] == [b"", bytes(len(U.snvs_of_strings(U.C12[1])))]


def test_the_sequence_moves_what_it_is_meant_to_move(C, walked):
    sizes = {label: [len(s) for s in U.reference_of(label)[1]] for label in U.LABELS}
    assert len(sizes["many"]) == 70 > len(sizes["first"]) == 5 and max(max(v) for v in sizes.values()) <= 20000
    assert "U" in U.reference_of("with_u")[1][0] and not any("U" in s.upper() for s in U.reference_of("first")[1])
    assert sizes["c12"] == [12] and len(U.snvs_of_strings(U.C12[1])) == 4
    assert walked["first_again"] == walked["first"]
    # the region set differs from step to step, and so does the presence table; at "first_again" it is the first one's again
    tables = [walked[label]["site_presence/n20_nrg"] for label in U.LABELS]
    assert tables[0] == tables[3] and len({t[0] for t in tables}) >= 3 and len(tables[1][0]) > len(tables[0][0]) > len(tables[4][0])
    for label in U.LABELS:
        raw = U.snvs_of_strings(U.reference_of(label)[1])
        assert len(raw) <= U.MOST
        ends = {(ci, pos) for ci, n in enumerate(sizes[label]) for pos in (0, n - 1)}
        assert ends <= {v[:2] for v in raw} and all(v[3] != v[2] for v in raw)


def test_a_context_without_a_reference_answers_estate(C):
    ctx = C.Context(-1)
    try:
        U.assert_no_reference(C, ctx, U.reference_of("first")[1], host=True)
    finally:
        ctx.close()


def test_refusals_leave_the_context_as_it_was(C, first):
    ctx, names, seqs = first
    got = U.run_refusals(C, ctx, names, seqs, host=True)
    assert len(got) == 8 and all(len(x) for x in got)


def test_shrinking_inside_one_reference(C, first):
    """The inputs of the GPU test: what is large is large, what is small is smaller, and large again gives the first bytes again."""
    ctx, names, seqs = first
    keys = U.shrink_keys(C, ctx, seqs, host=True)
    copies = np.frombuffer(keys[0], dtype=np.uint64)
    assert len(copies) == 600 and copies[-1] >= 64 and (copies > 0).sum() >= 300         # (the T's: the '-' sites of chrH's run of A's)
    near = np.frombuffer(keys[1], dtype=np.uint64).reshape(600, 3)
    assert (near[:, 0] == copies).all() and near[:, 1:].sum() > 0
    assert np.frombuffer(keys[4], dtype=np.uint64)[-1] == copies[-1] and len(keys[2]) == 8 and keys[2] == keys[0][:8]
    big, one, again = U.shrink_limit(C, ctx, seqs, host=True)
    assert big == again and len(one[2]) < len(big[2]) and one[0] == big[0]
    listed = np.diff(np.frombuffer(big[1], dtype=np.uint64))
    assert listed[0] >= 6 and (np.diff(np.frombuffer(one[1], dtype=np.uint64)) <= 1).all()
    snvs = U.shrink_snvs(C, ctx, seqs, host=True)
    assert [len(x[1]) for x in snvs] == [700, 1, 257, 0] and len(snvs[0][0]) > len(snvs[2][0]) > 0 and snvs[3] == [b"", b"", b"", b""]
    assert len(snvs[0][2]) > len(snvs[2][2]) > 0
    for key, (whole, empty, again) in U.shrink_region(C, ctx, seqs, host=True).items():
        assert whole == again and len(whole[-1]) > 0 and not any(len(x) for x in empty[-1:]), key


@pytest.mark.parametrize("k", range(U.N_DRAWS))
def test_drawn_patterns_on_the_host(C, k):
    drawn, names, seqs, want = U.draw(C, k)
    pat = U.guide_of(C, drawn)
    assert (pat.guide, pat.pams, pat.pam_is_five_prime) == (drawn[0], drawn[1], drawn[2])
    ctx = C.Context(-1)
    try:
        ctx.set_reference(names, [s.encode() for s in seqs])
        assert ctx.find_sites(pat, host=True).tobytes() == R.as_records(want, np.dtype(C.aligner.SITE_DTYPE)).tobytes()
        if k % 4 == 0:
            raw = U.drawn_snvs(seqs)
            edit = E.edit_of(C, U.drawn_edit(len(drawn[0])))
            got = ctx.find_allele_sites(pat, E.snv_array(C, raw), host=True)
            records, status = C.allele_sites_of(seqs, pat, raw)
            assert got.sites.tobytes() == A.as_records(C, records).tobytes() and got.status.tolist() == list(status)
            got = ctx.find_edit_sites(pat, edit, E.snv_array(C, raw), host=True)
            records, status = C.edit_sites_of(seqs, pat, edit, raw)
            assert got.sites.tobytes() == E.as_records(C, records).tobytes() and got.status.tolist() == list(status)
    finally:
        ctx.close()


def test_the_draws_are_what_the_issue_asks_for(C):
    """From the referee alone: at most a quarter of the draws has an empty listing on a strand; the draws differ in length, side and
    number of PAMs; a planted instance lies across a word boundary on each strand."""
    empty = 0
    shapes = set()
    for k in range(U.N_DRAWS):
        (proto, pams, five), names, seqs, sites = U.draw(C, k)
        assert 1 <= len(proto) <= 32 and len(pams) <= 8 and all(1 <= len(p) <= 16 and set(p) != {"n"} for p in pams)
        assert len(seqs[0]) % 32 != 0 and [len(s) for s in seqs] == [2003, 2000]
        empty += not all(any(s[3] == strand for s in sites) for strand in "+-")
        shapes.add((len(proto), len(pams), five))
        foot = len(proto) + max([len(p) for p in pams], default=0)
        if foot >= 2:
            for strand in "+-":
                lo = lambda s: min(s[1], s[2]) if s[2] >= 0 else s[1]
                assert any(s[3] == strand and lo(s) // 32 != (lo(s) + s[5] + s[6] - 1) // 32 for s in sites), (k, strand)
    assert 4 * empty <= U.N_DRAWS
    assert len(shapes) >= 30 and {f for _, _, f in shapes} == {False, True} and {n for _, n, _ in shapes} >= {0, 1, 8}
    rng = random.Random(1)
    assert all(U._acceptable(*U.draw_pattern(rng)[:2]) for _ in range(200))
