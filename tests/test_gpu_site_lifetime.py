"""GPU tests of what a long-lived context keeps between the guide-site calls (site_lifetime_util.py): one Context(0) through six
references -- more contigs, fewer, Us that come and go, an index loaded, a reference shorter than any footprint, growth again -- with a
round of every entry point after each, held byte for byte against a fresh Context(0), a host-only context and the referee; lists, limits
and regions that shrink and grow again inside one reference; refused calls; a failed upload; forty drawn patterns through one context.

What the device is given here is what test_site_lifetime_host.py gives the host twins: every refused call is refused by the call's plan
on the host (plan_site_pattern and what follows it in sites_host.cpp), before anything is launched."""
import numpy as np
import pytest

import allele_sites_ref as A
import edit_sites_ref as E
import site_lifetime_util as U
import sites_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


@pytest.fixture(scope="module")
def walked(C, tmp_path_factory):
    """{label: round} of one Context(0) taken through the sequence."""
    ctx = C.Context(0)
    try:
        return U.walk(C, ctx, str(tmp_path_factory.mktemp("lifetime") / "first.idx"))
    finally:
        ctx.close()


def _with_first(C, device):
    names, seqs = U.reference_of("first")
    ctx = C.Context(device)
    ctx.set_reference(names, [s.encode() for s in seqs])
    ctx.set_regions(U.regions_of_strings(C, names, seqs))
    return ctx, names, seqs


@pytest.fixture(scope="module")
def first(C):
    """(a Context(0) and a host-only one that hold the first reference and its regions, names, strings): every test of one reference
    goes through this one device context, one after the other."""
    ctx, names, seqs = _with_first(C, 0)
    twin = _with_first(C, -1)[0]
    yield ctx, twin, names, seqs
    ctx.close()
    twin.close()


@pytest.mark.parametrize("label", U.LABELS)
def test_one_device_context_through_the_sequence(C, walked, label):
    got = walked[label]
    assert U.differing(got, U.fresh_round(C, label, 0)) == []
    host = U.fresh_round(C, label, -1)
    assert len(host) >= 60 and U.differing(got, host, keys=host) == []
    for name in U.PATTERN_NAMES:
        assert got["find_sites/" + name] == U.brute_bytes(C, label, name), name
    text, rows = got["search_hits"]
    assert len(C.read_hits(text)) == rows
    assert (rows >= 1) == (label != "c12") and int(np.frombuffer(got["search_counts"][1], dtype=np.uint64).sum()) == rows


def test_the_index_brings_the_first_rounds_back(C, walked):
    assert walked["first_again"] == walked["first"]
    # the hits text names the contigs: the first reference's names are back, not the reference's before it
    rows = C.read_hits(walked["first_again"]["search_hits"][0])
    assert rows and {r["chromosome"] for r in rows} <= set(U.reference_of("first")[0])


@pytest.mark.parametrize("opener", ["find_sites", "find_allele_sites", "find_edit_sites"])
def test_each_of_the_three_calls_refills_the_u_runs(C, opener):
    """The runs of U are kept per reference and filled where they are first needed, in three places.  A round opens with find_sites;
    here each of the three is the first call after the reference changes, from one without Us to one with them and back."""
    plain = U.reference_of("first")
    names, seqs, raw = E.u_genome()
    pat, edit = U.pattern_of(C, "n20_nrg"), E.edit_of(C, U.EDIT)

    def first_call(c, strings, host):
        targets = list(E.editor_targets(seqs, U.EDIT, 0, 0, len(seqs[0]))) if opener == "find_edit_sites" else raw
        snvs = E.snv_array(C, targets if strings is seqs else U.snvs_of_strings(strings, most=200))
        if opener == "find_sites":
            return [c.find_sites(pat, host=host).tobytes()]
        got = c.find_allele_sites(pat, snvs, host=host) if opener == "find_allele_sites" else c.find_edit_sites(pat, edit, snvs, host=host)
        return [got.sites.tobytes(), got.status.tobytes()]

    ctx, twin = C.Context(0), C.Context(-1)
    try:
        for nm, strings in (plain, (names, seqs), plain, (names, seqs)):
            for c in (ctx, twin):
                c.set_reference(nm, [s.encode() for s in strings])
            got = first_call(ctx, strings, False)
            assert len(got[0]) and got == first_call(twin, strings, True)
        assert "U" in seqs[0].upper() and not any("U" in s.upper() for s in plain[1])
    finally:
        ctx.close()
        twin.close()


@pytest.mark.parametrize("what", ["keys", "limit", "snvs", "region"])
def test_shrinking_inside_one_reference(C, first, what):
    ctx, twin, names, seqs = first
    call = getattr(U, "shrink_" + what)
    assert call(C, ctx, seqs, host=False) == call(C, twin, seqs, host=True)


def test_refusals_leave_the_context_as_it_was(C, first):
    ctx, twin, names, seqs = first
    assert U.run_refusals(C, ctx, names, seqs, host=False) == U.run_refusals(C, twin, names, seqs, host=True)
    assert U.round_of(C, ctx, names, seqs, host=False) == U.fresh_round(C, "first", 0)


def test_a_failed_upload_leaves_no_reference_to_the_site_calls(C, monkeypatch):
    """After an upload that fails every entry point answers CALITAS_ESTATE -- from its plan, which looks at has_ref before anything
    else -- and after a good one the round is a fresh context's."""
    from calitas_amd import synth
    names, seqs = U.reference_of("first")
    big = synth.make_genome([("big", 3_000_000)], 72)
    ctx = C.Context(0)
    try:
        ctx.set_reference(names, [s.encode() for s in seqs])
        ctx.set_regions(U.regions_of_strings(C, names, seqs))
        assert U.round_of(C, ctx, names, seqs, host=False) == U.fresh_round(C, "first", 0)      # every buffer of the scratch is there
        monkeypatch.setenv("CALITAS_DEVICE_BUDGET_MB", "1")
        with pytest.raises(C.CalitasError) as e:
            ctx.set_reference(*big)
        assert e.value.code == C._lib.ENOMEM
        monkeypatch.delenv("CALITAS_DEVICE_BUDGET_MB")
        U.assert_no_reference(C, ctx, seqs, host=False)
        with pytest.raises(C.CalitasError) as e:
            ctx.search_counts(C.Guide(U.guide_of_strings(seqs)), C.make_params(max_guide_diffs=2))
        assert e.value.code == C._lib.ESTATE
        ctx.set_reference(names, [s.encode() for s in seqs])
        ctx.set_regions(U.regions_of_strings(C, names, seqs))
        assert U.round_of(C, ctx, names, seqs, host=False) == U.fresh_round(C, "first", 0)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def drawing(C):
    """One Context(0) and one host-only context for all forty draws."""
    ctx, twin = C.Context(0), C.Context(-1)
    yield ctx, twin
    ctx.close()
    twin.close()


@pytest.mark.parametrize("k", range(U.N_DRAWS))
def test_drawn_patterns_on_the_device(C, drawing, k):
    ctx, twin = drawing
    drawn, names, seqs, want = U.draw(C, k)
    pat = U.guide_of(C, drawn)
    for c in (ctx, twin):
        c.set_reference(names, [s.encode() for s in seqs])
    got = ctx.find_sites(pat)
    assert got.tobytes() == R.as_records(want, got.dtype).tobytes() and got.tobytes() == twin.find_sites(pat, host=True).tobytes()
    if k % 4 == 0:
        raw = U.drawn_snvs(seqs)
        snvs = E.snv_array(C, raw)
        edit = E.edit_of(C, U.drawn_edit(len(drawn[0])))
        got = ctx.find_allele_sites(pat, snvs)
        records, status = C.allele_sites_of(seqs, pat, raw)
        assert got.sites.tobytes() == A.as_records(C, records).tobytes() and got.status.tolist() == list(status)
        got = ctx.find_edit_sites(pat, edit, snvs)
        records, status = C.edit_sites_of(seqs, pat, edit, raw)
        assert got.sites.tobytes() == E.as_records(C, records).tobytes() and got.status.tolist() == list(status)
