"""CPU tests of the edit sites: calitas_find_edit_sites_host and calitas_count_edit_sites_host (the host twin of edit_sites.hip, on a
host-only context) against the referee of edit_sites_ref.py and against the contract in plain Python (edit_sites_of), byte for byte,
over every pattern, the four editors and both modes -- what the genome was planted for, max_bystanders, the count call, the errors in
their order, no SNV at all, the struct sizes, a reference with Us, EditSites, and both FindGuides tools with --edit-sites on the host
twin.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import allele_sites_ref as A
import edit_sites_ref as E
import sites_ref as R
from fasta_util import write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = E.L


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


@pytest.fixture(scope="module")
def genome(C):
    names, seqs = E.genome()
    ctx = C.Context(-1)
    ctx.set_reference(names, [s.encode() for s in seqs])
    yield ctx, names, seqs
    ctx.close()


def _bins(sites):
    return np.bincount(np.minimum([bin(int(x)).count("1") - 1 for x in sites["editable"]], 3), minlength=4).tolist() if len(sites) else [0, 0, 0, 0]


def _hold(C, ctx, name, edit, snvs, want, status):
    """The twin and its count call against the referee's (records, status); returns the EditSites."""
    got = ctx.find_edit_sites(E.pattern_of(C, name), E.edit_of(C, edit), E.snv_array(C, snvs), host=True)
    assert got.sites.tobytes() == want.tobytes(), (name, edit)
    assert got.status.tobytes() == status.tobytes()
    n, by, st = ctx.count_edit_sites(E.pattern_of(C, name), E.edit_of(C, edit), E.snv_array(C, snvs), host=True)
    assert n == len(want) and by.tolist() == _bins(want) and st.tobytes() == status.tobytes()
    return got


def test_the_genome_holds_what_it_was_planted_for():
    E.check_planted()


@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("name", E.NAMES)
def test_the_twin_against_the_referee_and_the_contract(C, genome, name, which):
    ctx, names, seqs = genome
    for correct in (False, True):
        edit = E.editors()[which] + (correct, None)
        want, status, snvs = E.referee(C, seqs, name, edit)
        got = _hold(C, ctx, name, edit, snvs, want, status)
        plain, plain_status = C.edit_sites_of(seqs, E.pattern_of(C, name), E.edit_of(C, edit), snvs)
        assert E.as_records(C, plain).tobytes() == want.tobytes() and plain_status == status.tolist()
        # the order: by SNV, then start -- total; at most a window of records per SNV
        keys = [(int(r["snv_index"]), int(r["protospacer_start"])) for r in got.sites]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        w0, w1 = edit[2]
        assert not len(got) or np.bincount(got.sites["snv_index"]).max() <= w1 - w0
        for r in got.sites[::17]:
            # the guide is the background's protospacer: the editor's `from` at the target, and at every editable position
            proto, o = got.protospacer(r), got.offset(r)
            assert w0 <= o < w1 and proto[o] == edit[0] and (int(r["editable"]) >> o) & 1
            assert all(proto[i] == edit[0] and w0 <= i < w1 for i in got.bystanders(r)) and o not in got.bystanders(r)
            v = snvs[int(r["snv_index"])]
            letter = (v[3] if correct else seqs[v[0]][v[1]]).upper()
            assert proto[o] == (letter if r["strand"] == b"+" else R.revcomp(letter))


@pytest.mark.parametrize("name", ["n20_nrg", "n20"])
def test_max_bystanders_gives_the_sub_listings(C, genome, name):
    ctx, names, seqs = genome
    for correct in (False, True):
        base = E.editors()[0] + (correct,)
        full, status, snvs = E.referee(C, seqs, name, base + (None,))
        counts = np.array([bin(int(x)).count("1") - 1 for x in full["editable"]])
        for most in (0, 2):
            want = full[counts <= most]
            assert 0 < len(want) < len(full)
            got = _hold(C, ctx, name, base + (most,), snvs, want, status)
            records, st = E.edit_sites(seqs, name, base + (most,), snvs, key="genome")
            assert E.as_records(C, records).tobytes() == got.sites.tobytes() and st == status.tolist()
        got = _hold(C, ctx, name, base + (31,), snvs, full, status)                 # the largest bound there is: everything


def test_the_homopolymer(C, genome):
    ctx, names, seqs = genome
    edit = ("A", "G", (0, L), "N", False, None)
    snvs = E.homopolymer_targets(seqs, L)
    want, status, _ = E.referee(C, seqs, "n20", edit, snvs)
    got = _hold(C, ctx, "n20", edit, snvs, want, status)
    assert len(got) == L * len(snvs) and all(len(got.bystanders(r)) == L - 1 for r in got.sites[::7])
    assert len(ctx.find_edit_sites(E.pattern_of(C, "n20"), E.edit_of(C, edit[:5] + (L - 2,)), E.snv_array(C, snvs), host=True)) == 0


def _call(C, ctx, pat, edit, snvs, n=None, host=True, with_status=True):
    """edit: (from, to, window_from, window_to, context, correct, max_bystanders, reserved) as bytes and integers."""
    from calitas_amd import _lib
    g = pat.to_c()
    e = _lib.BaseEditT(*edit)
    arr = (_lib.SnvT * max(1, len(snvs)))()
    for k, (ci, pos, ref, alt, reserved) in enumerate(snvs):
        arr[k].contig_index, arr[k].position, arr[k].ref, arr[k].alt, arr[k].reserved = ci, pos, ref or b"\0", alt or b"\0", reserved
    out, n_out = ctypes.POINTER(_lib.EditSiteT)(), ctypes.c_uint64()
    status = (ctypes.c_uint8 * max(1, len(snvs)))()
    fn = _lib.lib.calitas_find_edit_sites_host if host else _lib.lib.calitas_find_edit_sites
    rc = fn(ctx._h, ctypes.byref(g), ctypes.byref(e), ctypes.addressof(arr), len(snvs) if n is None else n, ctypes.byref(out), ctypes.byref(n_out),
            ctypes.addressof(status) if with_status else None)
    msg = _lib.lib.calitas_last_error(ctx._h).decode()
    if rc == 0:
        assert bool(out)                                  # one block, also when there are no records
        _lib.lib.calitas_free(out)
    else:
        assert not out
    return rc, msg, n_out.value


def test_errors_in_their_order(C, genome):
    from calitas_amd import _lib
    ctx, names, seqs = genome
    pat = E.pattern_of(C, "n20_nrg")
    ok = (1, 10, b"", b"A", 0)
    bad_snvs = [ok, (1, 5000, b"x", b"N", 7), (9, 0, b"x", b"N", 7)]
    fine = (b"C", b"T", 3, 8, b"N", 0, 255, 0)
    # each field of the editor, everything behind it wrong as well: the first one is named
    wrong = [(0, b"x", "from_base"), (1, b"N", "to_base"), (1, b"c", "the same base"), (3, 8, "empty window"), (3, 9, "empty window"), (3, L + 1, "window_to"),
             (4, b"!", "context"), (5, 2, "correct"), (6, 32, "max_bystanders"), (6, 254, "max_bystanders"), (7, 1, "reserved")]
    for field, value, said in wrong:
        edit = list(fine)
        # what comes behind the field in the order of the checks is wrong too
        for later, junk in ((7, 9), (6, 100), (5, 7), (4, b"?"), (3, 0), (1, b"C"), (0, b"z")):
            if later > (3 if field in (2, 3) else field):
                edit[later] = junk
        if said == "empty window":
            edit[2], edit[3] = value, 8
        elif said == "window_to":
            edit[2], edit[3] = 3, value
        else:
            edit[field] = value
        rc, msg, _ = _call(C, ctx, pat, tuple(edit), bad_snvs)
        assert rc == _lib.EINVAL and said in msg, (field, value, msg)
    # what calitas_find_sites refuses about the pattern comes before the editor, the SNVs come behind it
    rc, msg, _ = _call(C, ctx, C.Guide("NNNN!NNN" + "nrg"), (b"x", b"x", 9, 3, b"!", 2, 99, 1), bad_snvs)
    assert rc == _lib.EINVAL and "non-IUPAC" in msg
    rc, msg, _ = _call(C, ctx, pat, fine, [ok], n=1 << 32)
    assert rc == _lib.EINVAL and "n_snvs" in msg
    rc, msg, _ = _call(C, ctx, pat, fine, bad_snvs)
    assert rc == _lib.EINVAL and "snvs[2].contig_index" in msg
    rc, msg, _ = _call(C, ctx, pat, fine, bad_snvs[:2])
    assert rc == _lib.EINVAL and "snvs[1].position" in msg
    rc, msg, _ = _call(C, ctx, pat, fine, [ok, (1, 11, b"x", b"A", 7), (1, 12, b"x", b"N", 7)])
    assert rc == _lib.EINVAL and "snvs[2].alt" in msg
    rc, msg, _ = _call(C, ctx, pat, fine, [ok, (1, 11, b"x", b"A", 7)])
    assert rc == _lib.EINVAL and "snvs[1].ref" in msg
    rc, msg, _ = _call(C, ctx, pat, fine, [ok, ok, (1, 11, b"u", b"a", 7)])
    assert rc == _lib.EINVAL and "snvs[2].reserved" in msg
    # the legal corners: either case and U, a context of 0, the window's limits, the bound's limits, no status
    for edit in (fine, (b"c", b"u", 0, L, b"\0", 1, 0, 0), (b"U", b"a", L - 1, L, b"h", 0, 31, 0)):
        assert _call(C, ctx, pat, edit, [ok, (1, 11, b"u", b"a", 0)])[0] == 0
    assert _call(C, ctx, pat, fine, [ok, ok], with_status=False)[0] == 0
    # no SNV at all is legal
    assert _call(C, ctx, pat, fine, [])[::2] == (0, 0)
    edit = C.BaseEdit("C", "T", (3, 8))
    empty = ctx.find_edit_sites(pat, edit, np.zeros(0, dtype=C.SNV_DTYPE), host=True)
    assert len(empty) == 0 and empty.sites.dtype == np.dtype(C.EDIT_SITE_DTYPE) and len(empty.status) == 0
    n, by, st = ctx.count_edit_sites(pat, edit, [], host=True)
    assert n == 0 and by.tolist() == [0, 0, 0, 0] and len(st) == 0
    # the device call on a host-only context, before everything
    rc, msg, _ = _call(C, ctx, C.Guide("NNNN!NNN" + "nrg"), (b"x", b"x", 9, 3, b"!", 2, 99, 1), bad_snvs, host=False)
    assert rc == _lib.ENODEV


def test_struct_sizes(C):
    from calitas_amd import _lib
    assert ctypes.sizeof(_lib.BaseEditT) == 8 and ctypes.sizeof(_lib.EditSiteT) == 32
    assert np.dtype(C.EDIT_SITE_DTYPE).itemsize == 32
    assert _lib.EditSiteT.snv_index.offset == 16 and _lib.EditSiteT.editable.offset == 20 and _lib.EditSiteT.guide_lo.offset == 24
    assert [_lib.BaseEditT.window_from.offset, _lib.BaseEditT.context.offset, _lib.BaseEditT.max_bystanders.offset, _lib.BaseEditT.reserved.offset] == [2, 4, 6, 7]
    for s in ("calitas_find_edit_sites", "calitas_count_edit_sites", "calitas_find_edit_sites_host", "calitas_count_edit_sites_host"):
        assert s in _lib.SYMBOLS and hasattr(_lib.lib, s)
    header = open(os.path.join(ROOT, "include", "calitas_hip.h")).read()
    assert all("int %s(" % s in header for s in _lib.SYMBOLS if "edit_sites" in s)


def test_a_reference_with_us(C):
    names, seqs, _ = E.u_genome()
    ctx = C.Context(-1)
    try:
        ctx.set_reference(names, [s.encode() for s in seqs])
        for edit in (("C", "T", (3, 8), "N", False, None), ("C", "T", (0, L), "T", True, None)):
            snvs = list(E.editor_targets(seqs, edit, 0, 0, len(seqs[0])))
            assert not edit[4] or any(seqs[0][v[1]] in "Uu" for v in snvs)                  # a U is a T: correcting to T, the targets stand on them
            for name in ("n20_nrg", "aux24", "n20"):
                records, status = E.edit_sites(seqs, name, edit, snvs)
                got = _hold(C, ctx, name, edit, snvs, E.as_records(C, records), np.array(status, dtype=np.uint8))
                assert len(got)
        # a protospacer that holds the U: the guide reads a T there
        edit = ("C", "T", (3, 8), "N", False, None)
        snvs = list(E.editor_targets(seqs, edit, 0, 90, 130))
        got = ctx.find_edit_sites(E.pattern_of(C, "n20"), E.edit_of(C, edit), E.snv_array(C, snvs), host=True)
        recs = [r for r in got.sites if int(r["protospacer_start"]) == 100 and r["strand"] == b"+"]
        assert recs and all(got.protospacer(r)[4] == "T" for r in recs)
    finally:
        ctx.close()


def _run(cmd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)


TOOLS = ([sys.executable, "-m", "calitas_amd", "FindGuides"], [os.path.join(ROOT, "calitas_amd", "calitas"), "FindGuides"])


def _edit_line(stderr):
    lines = [ln for ln in stderr.splitlines() if ln.startswith("edits: ")]
    assert len(lines) == 1, stderr
    return lines[0]


def check_table(C, names, seqs, text, name, edit, start, end, counts):
    """The --edit-sites table of chrB's [start, end) against the referee over the tools' VCF and against the strings."""
    lines = [ln.split("\t") for ln in text.splitlines()]
    assert lines[0] == C.EDIT_COLUMNS
    rows = []
    n_other = n_lacks = 0
    for chrom, pos1, vid, ref, alts in E.vcf_records(names, seqs, edit):
        if chrom not in names:
            n_lacks += 1
            continue
        if chrom != "chrB" or not start <= pos1 - 1 < end:
            continue
        for alt in alts:
            if len(ref) != 1 or len(alt) != 1:
                n_other += 1
            else:
                rows.append((chrom, pos1, vid, ref, alt))
    records, status = E.edit_sites(seqs, name, edit, [(names.index(c), p - 1, ref, alt) for c, p, _, ref, alt in rows], key="genome")
    assert counts == ("edits: %d SNVs examined, %d records; skipped: %d other alleles, %d records on chromosomes the reference lacks, 0 beyond a contig's end, "
                      "%d with another REF than the reference, %d on a base that is not A C G T, %d with ALT equal to the reference, "
                      "%d that are not the editor's change, %d whose 5' neighbour fails the context"
                      % (status.count(0), len(records), n_other, n_lacks, status.count(1), status.count(2), status.count(3), status.count(4), status.count(5)))
    assert len(records) == len(lines) - 1
    pat = E.pattern_of(C, name)
    for ln, r in zip(lines[1:], records):
        chrom, pos1, vid, ref, alt = rows[r[7]]
        lo, hi = (r[1], r[1] + L) if r[2] < 0 else (min(r[1], r[2]), max(r[1] + L, r[2] + r[5]))
        o = (pos1 - 1 - r[1]) if r[3] == b"+" else (r[1] + L - 1 - (pos1 - 1))
        assert ln[:11] == [chrom, str(pos1), vid or ".", ref, alt, "correct" if edit[4] else "install", str(lo), str(hi), r[3].decode(), str(r[4]), str(o)]
        back = seqs[1][:pos1 - 1] + (alt if edit[4] else ref) + seqs[1][pos1:]
        proto, pam = back[r[1]:r[1] + L].upper(), back[r[2]:r[2] + r[5]].upper() if r[2] >= 0 else ""
        if r[3] == b"-":
            proto, pam = R.revcomp(proto), R.revcomp(pam)
        assert ln[11] == proto + (pat.pams[r[4]] if r[4] >= 0 else "") and ln[12] == pam
        others = [i for i in range(L) if (r[8] >> i) & 1 and i != o]
        assert ln[13] == str(len(others)) and ln[14] == (",".join(map(str, others)) or ".")
        assert ln[15] == "".join(edit[1].lower() if (r[8] >> i) & 1 else ch for i, ch in enumerate(proto)) and ln[15][o] == edit[1].lower()
    return records


EDIT_FLAGS = [(["--editor", "C:T", "--edit-window", "3:8"], "n20_nrg", ("C", "T", (3, 8), "N", False, None)),
              (["--editor", "A:G", "--edit-window", "0:20", "--edit-context", "h", "--edit-mode", "correct", "--max-bystanders", "2", "-x", "ng", "nnaa"], "aux24",
               ("A", "G", (0, 20), "H", True, 2)),
              (["--editor=G:A", "--edit-window=2:12", "--edit-mode=install"], "n20_nrg", ("G", "A", (2, 12), "N", False, None))]


@pytest.mark.parametrize("flags, name, edit", EDIT_FLAGS)
def test_both_tools_on_the_host_twin(C, genome, tmp_path, flags, name, edit):
    ctx, names, seqs = genome
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    vcf = E.write_vcf(str(tmp_path / "v.vcf"), names, seqs, edit)
    text = "N" * 20 + ("ngg" if "-x" in flags else "nrg")
    start, end = 100, 1600
    common = ["-i", text, "-r", fa, "--device", "-1", "-c", "chrB", "-s", str(start), "-e", str(end)]
    out = []
    for k, tool in enumerate(TOOLS):
        table, alleles = str(tmp_path / ("edits%d.tsv" % k)), str(tmp_path / ("alleles%d.tsv" % k))
        r = _run(tool + common + ["--alleles", vcf, "--edit-sites", table] + flags)
        assert r.returncode == 0, r.stderr
        out.append((r.stdout, open(table).read(), _edit_line(r.stderr)))
        if k == 0:
            plain = _run(tool + common + (["-x", "ng", "nnaa"] if "-x" in flags else []))
            assert plain.returncode == 0 and plain.stdout == r.stdout                   # the guides table does not change
        # --allele-sites beside it: both tables, each what it is alone
        both = _run(tool + common + ["--alleles", vcf, "--edit-sites", table + ".2", "--allele-sites", alleles] + flags)
        alone = _run(tool + common + ["--alleles", vcf, "--allele-sites", alleles + ".1"] + (["-x", "ng", "nnaa"] if "-x" in flags else []))
        assert both.returncode == 0 and alone.returncode == 0, both.stderr + alone.stderr
        assert open(table + ".2").read() == out[-1][1] and open(alleles).read() == open(alleles + ".1").read()
        assert _edit_line(both.stderr) == out[-1][2] and [ln for ln in both.stderr.splitlines() if ln.startswith("alleles: ")]
    assert out[0] == out[1]                                                         # the same bytes from each: table, edit sites, counts
    records = check_table(C, names, seqs, out[0][1], name, edit, start, end, out[0][2])
    assert len(records) >= 20 and {r[3] for r in records} == {b"+", b"-"} and any(E.bystanders_of(r) for r in records)


def test_the_tools_refuse_flags_that_lack_their_partner(tmp_path, genome):
    ctx, names, seqs = genome
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    vcf = A.write_vcf(str(tmp_path / "v.vcf"), names[:3], seqs[:3])
    out = str(tmp_path / "e.tsv")
    whole = ["--alleles", vcf, "--edit-sites", out, "--editor", "C:T", "--edit-window", "3:8"]
    for tool in TOOLS:
        base = tool + ["-i", "N" * 20 + "nrg", "-r", fa, "--device", "-1", "-c", "chrC"]
        r = _run(base + whole)
        assert r.returncode == 0, r.stderr
        # --edit-sites needs --alleles, --editor and --edit-window
        for drop in ("--alleles", "--editor", "--edit-window"):
            at = whole.index(drop)
            r = _run(base + whole[:at] + whole[at + 2:])
            assert r.returncode != 0 and "--edit-sites" in r.stderr and drop in r.stderr, (drop, r.stderr)
        # the other edit flags need --edit-sites
        for extra in (["--editor", "C:T"], ["--edit-window", "3:8"], ["--edit-context", "T"], ["--edit-mode", "correct"], ["--max-bystanders", "1"]):
            r = _run(base + extra)
            assert r.returncode != 0 and "--edit-sites" in r.stderr and extra[0] in r.stderr, (extra, r.stderr)
        # --alleles alone names both of the tables it serves
        r = _run(base + ["--alleles", vcf])
        assert r.returncode != 0 and "--allele-sites" in r.stderr and "--edit-sites" in r.stderr
        # values
        for flag, value in (("--editor", "C:C"), ("--editor", "CT"), ("--editor", "N:T"), ("--edit-window", "8:3"), ("--edit-window", "3:21"), ("--edit-window", "3"),
                            ("--edit-context", "X"), ("--edit-context", "TT"), ("--edit-mode", "revert"), ("--max-bystanders", "32"), ("--max-bystanders", "-1")):
            args = list(whole)
            if flag in args:
                args[args.index(flag) + 1] = value
                r = _run(base + args)
            else:
                r = _run(base + args + [flag + "=" + value])
            assert r.returncode != 0 and flag in r.stderr, (flag, value, r.stderr)
