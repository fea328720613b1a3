"""CPU tests of the allele sites: calitas_find_allele_sites_host and calitas_count_allele_sites_host (the host twin of
allele_sites.hip, on a host-only context) against the referee of allele_sites_ref.py, byte for byte, over every pattern on the planted
SNVs and on the exhaustive 1 800 -- what the genome was planted for, the contract in plain Python, the count call, the errors in their
order, no SNV at all, the struct sizes, a reference with Us, AlleleSites, and both FindGuides tools with --alleles on the host twin.
No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import allele_sites_ref as A
import sites_ref as R
from fasta_util import write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = A.L


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


@pytest.fixture(scope="module")
def genome(C):
    names, seqs = A.genome()
    ctx = C.Context(-1)
    ctx.set_reference(names, [s.encode() for s in seqs])
    yield ctx, names, seqs
    ctx.close()


def _hold(C, ctx, name, seqs, snvs, key=None):
    """The twin and its count call against the referee; returns the AlleleSites."""
    records, status = A.allele_sites(seqs, name, snvs, key=key)
    want = A.as_records(C, records)
    got = ctx.find_allele_sites(A.pattern_of(C, name), A.snv_array(C, snvs), host=True)
    assert got.sites.tobytes() == want.tobytes(), name
    assert got.status.tolist() == status
    n, by, st = ctx.count_allele_sites(A.pattern_of(C, name), A.snv_array(C, snvs), host=True)
    assert n == len(want) and by.tolist() == np.bincount(want["kind"], minlength=4).tolist() and st.tolist() == status
    return got


def test_the_genome_holds_what_it_was_planted_for():
    A.check_planted()


@pytest.mark.parametrize("name", A.NAMES)
def test_the_twin_against_the_referee(C, genome, name):
    ctx, names, seqs = genome
    snvs = A.planted_snvs(seqs)
    got = _hold(C, ctx, name, seqs, snvs, key="genome")
    assert len(got)
    # the order: by SNV, then start, then '+' before '-' -- total
    keys = [(int(r["snv_index"]), int(r["protospacer_start"]), r["strand"] == b"-") for r in got.sites]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert np.bincount(got.sites["snv_index"]).max() <= 2 * 48 and not got.sites["reserved"].any()
    # a record's guide is the protospacer of the allele named, with the alt letter where the SNV is
    for r in got.sites[::37]:
        proto, offset, v = got.protospacer(r), int(r["guide_offset"]), snvs[int(r["snv_index"])]
        if 0 <= offset < L:
            letter = (v[3] if int(r["kind"]) & 1 else seqs[v[0]][v[1]]).upper()
            assert proto[offset] == (letter if r["strand"] == b"+" else R.revcomp(letter))


@pytest.mark.parametrize("name", A.NAMES)
def test_the_exhaustive_set(C, genome, name):
    ctx, names, seqs = genome
    snvs = A.exhaustive_snvs(seqs)
    assert len(snvs) == 1800
    got = _hold(C, ctx, name, seqs, snvs, key="genome")
    if name == "n20":
        per = np.bincount(got.sites["snv_index"], minlength=len(snvs))
        assert per[3 * 100:].min() == 2 * L and per[0] == 2 and (got.sites["kind"] == 3).all() and (got.sites["other_pam_index"] == -1).all()


def test_the_contract_in_plain_python(C, genome):
    ctx, names, seqs = genome
    snvs = A.planted_snvs(seqs)
    for name in ("n20_nrg", "aux24", "tttv_n20"):
        want, status = C.allele_sites_of(seqs, A.pattern_of(C, name), snvs)
        got = ctx.find_allele_sites(A.pattern_of(C, name), snvs_of_tuples(C, ctx, names, snvs), host=True)
        assert got.sites.tobytes() == A.as_records(C, want).tobytes() and got.status.tolist() == status


def snvs_of_tuples(C, ctx, names, snvs):
    """Through snvs_of: chromosome names and 1-based positions."""
    out = C.snvs_of([(names[ci], pos + 1, ref, alt) for ci, pos, ref, alt in snvs], ctx)
    assert out.tobytes() == A.snv_array(C, snvs).tobytes()
    return out


def test_allele_sites_of_and_merge(C, genome):
    ctx, names, seqs = genome
    pat = A.pattern_of(C, "n20_nrg")
    snvs = A.planted_snvs(seqs)
    whole = ctx.find_allele_sites(pat, A.snv_array(C, snvs), host=True)
    head, tail = ctx.find_allele_sites(pat, A.snv_array(C, snvs[:50]), host=True), ctx.find_allele_sites(pat, A.snv_array(C, snvs[50:]), host=True)
    both = head.merge(tail)
    assert both.sites.tobytes() == whole.sites.tobytes() and both.status.tobytes() == whole.status.tobytes()
    assert sum(len(whole.of(i)) for i in range(len(snvs))) == len(whole) and len(whole.of(1)) > 0
    r = whole.of(1)[0]
    assert whole.guide(r) == whole.protospacer(r) + "nrg" and len(whole.guide(r)) == 23


def _call(C, ctx, pat, snvs, n=None, host=True, with_status=True):
    from calitas_amd import _lib
    g = pat.to_c()
    arr = (_lib.SnvT * max(1, len(snvs)))()
    for k, (ci, pos, ref, alt, reserved) in enumerate(snvs):
        arr[k].contig_index, arr[k].position, arr[k].ref, arr[k].alt, arr[k].reserved = ci, pos, ref or b"\0", alt or b"\0", reserved
    out, n_out = ctypes.POINTER(_lib.AlleleSiteT)(), ctypes.c_uint64()
    status = (ctypes.c_uint8 * max(1, len(snvs)))()
    fn = _lib.lib.calitas_find_allele_sites_host if host else _lib.lib.calitas_find_allele_sites
    rc = fn(ctx._h, ctypes.byref(g), ctypes.addressof(arr), len(snvs) if n is None else n, ctypes.byref(out), ctypes.byref(n_out), ctypes.addressof(status) if with_status else None)
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
    pat = A.pattern_of(C, "n20_nrg")
    ok = (1, 10, b"", b"A", 0)
    everything_wrong = [ok, (1, 5000, b"x", b"N", 7), (9, 0, b"x", b"N", 7)]
    # what calitas_find_sites refuses about the pattern comes first
    rc, msg, _ = _call(C, ctx, C.Guide("NNNN!NNN" + "nrg"), everything_wrong)
    assert rc == _lib.EINVAL and "non-IUPAC" in msg
    rc, msg, _ = _call(C, ctx, pat, [ok], n=1 << 32)
    assert rc == _lib.EINVAL and "n_snvs" in msg
    # then the first field that some SNV has wrong, and the first SNV that has it wrong
    rc, msg, _ = _call(C, ctx, pat, everything_wrong)
    assert rc == _lib.EINVAL and "snvs[2].contig_index" in msg
    rc, msg, _ = _call(C, ctx, pat, [ok, (-1, 0, b"", b"A", 0)])
    assert rc == _lib.EINVAL and "snvs[1].contig_index" in msg
    rc, msg, _ = _call(C, ctx, pat, everything_wrong[:2] + [(1, -1, b"", b"A", 0)])
    assert rc == _lib.EINVAL and "snvs[1].position" in msg
    rc, msg, _ = _call(C, ctx, pat, [(2, 60, b"", b"A", 0)])
    assert rc == _lib.EINVAL and "snvs[0].position" in msg
    rc, msg, _ = _call(C, ctx, pat, [ok, (1, 11, b"x", b"A", 7), (1, 12, b"x", b"N", 7)])
    assert rc == _lib.EINVAL and "snvs[2].alt" in msg
    rc, msg, _ = _call(C, ctx, pat, [ok, (1, 11, b"x", b"A", 7), (1, 12, b"", b"", 0)][:2])
    assert rc == _lib.EINVAL and "snvs[1].ref" in msg
    rc, msg, _ = _call(C, ctx, pat, [ok, ok, ok, (1, 11, b"u", b"a", 7)])
    assert rc == _lib.EINVAL and "snvs[3].reserved" in msg
    for fine in ([ok], [(1, 11, b"u", b"a", 0), ok], [(2, 59, b"", b"T", 0)]):
        assert _call(C, ctx, pat, fine)[0] == 0
    assert _call(C, ctx, pat, [ok, ok], with_status=False)[0] == 0            # status may be NULL
    # no SNV at all is legal
    assert _call(C, ctx, pat, [])[::2] == (0, 0)
    empty = ctx.find_allele_sites(pat, np.zeros(0, dtype=C.SNV_DTYPE), host=True)
    assert len(empty) == 0 and empty.sites.dtype == np.dtype(C.ALLELE_SITE_DTYPE) and len(empty.status) == 0
    assert ctx.count_allele_sites(pat, [], host=True)[0] == 0
    # the device call on a host-only context, before everything
    rc, msg, _ = _call(C, ctx, C.Guide("NNNN!NNN" + "nrg"), everything_wrong, host=False)
    assert rc == _lib.ENODEV
    # an absent contig is refused by name
    part = C.Context(-1)
    try:
        part.set_reference(names, [seqs[0].encode(), None, seqs[2].encode()], lengths=[len(s) for s in seqs])
        rc, msg, _ = _call(C, part, pat, [(0, 5, b"", b"A", 0), (1, 5000, b"x", b"N", 7)])
        assert rc == _lib.EINVAL and "snvs[1].contig_index" in msg and "absent" in msg
        assert _call(C, part, pat, [(0, 5, b"", b"A", 0), (2, 59, b"", b"A", 0)])[0] == 0
    finally:
        part.close()


def test_struct_sizes(C):
    from calitas_amd import _lib
    assert ctypes.sizeof(_lib.SnvT) == 12 and ctypes.sizeof(_lib.AlleleSiteT) == 32
    assert np.dtype(C.SNV_DTYPE).itemsize == 12 and np.dtype(C.ALLELE_SITE_DTYPE).itemsize == 32
    assert _lib.AlleleSiteT.snv_index.offset == 16 and _lib.AlleleSiteT.guide_lo.offset == 24
    for s in ("calitas_find_allele_sites", "calitas_count_allele_sites", "calitas_find_allele_sites_host", "calitas_count_allele_sites_host"):
        assert s in _lib.SYMBOLS and hasattr(_lib.lib, s)
    header = open(os.path.join(ROOT, "include", "calitas_hip.h")).read()
    assert all("int %s(" % s in header for s in _lib.SYMBOLS if "allele" in s)


def test_a_reference_with_us(C):
    names, seqs, snvs = A.u_genome()
    ctx = C.Context(-1)
    try:
        ctx.set_reference(names, [s.encode() for s in seqs])
        for name in ("n20_nrg", "aux24", "n20"):
            got = _hold(C, ctx, name, seqs, snvs)
            assert len(got)
        got = _hold(C, ctx, "n20_nrg", seqs, snvs)
        assert got.status[-2] == 0 and got.status[-1] == 3 and len(got.of(len(snvs) - 2))      # a U is a T, to ref and to alt
        # a site whose protospacer holds the U: the guide reads a T there
        recs = [r for r in got.sites if int(r["protospacer_start"]) == 100 and r["strand"] == b"+" and snvs[int(r["snv_index"])][1] != 104]
        assert recs and all(got.protospacer(r)[4] == "T" for r in recs)
    finally:
        ctx.close()


def _run(cmd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)


TOOLS = ([sys.executable, "-m", "calitas_amd", "FindGuides"], [os.path.join(ROOT, "calitas_amd", "calitas"), "FindGuides"])


def _allele_line(stderr):
    lines = [ln for ln in stderr.splitlines() if ln.startswith("alleles: ")]
    assert len(lines) == 1, stderr
    return lines[0]


@pytest.mark.parametrize("flags", [[], ["--allele-kinds", "alt"], ["--allele-kinds", "ref,both", "-x", "ng", "nnaa"]])
def test_both_tools_on_the_host_twin(C, genome, tmp_path, flags):
    ctx, names, seqs = genome
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    vcf = A.write_vcf(str(tmp_path / "v.vcf"), names, seqs)
    text = "N" * 20 + ("ngg" if "-x" in flags else "nrg")
    start, end = 100, 1600
    kinds = flags[flags.index("--allele-kinds") + 1].split(",") if "--allele-kinds" in flags else ["alt", "ref", "both"]
    common = ["-i", text, "-r", fa, "--device", "-1", "-c", "chrB", "-s", str(start), "-e", str(end), "--alleles", vcf] + flags
    out, plain = [], None
    for k, tool in enumerate(TOOLS):
        table = str(tmp_path / ("alleles%d.tsv" % k))
        r = _run(tool + common + ["--allele-sites", table])
        assert r.returncode == 0, r.stderr
        out.append((r.stdout, open(table).read(), _allele_line(r.stderr)))
        if k == 0:
            plain = _run(tool + [x for x in common if x != vcf and x != "--alleles" and x not in kinds and x != "--allele-kinds" and x != ",".join(kinds)])
    assert out[0] == out[1]                                                     # the same bytes from each: table, allele sites, counts
    assert plain.returncode == 0 and plain.stdout == out[0][0]                  # the guides table does not change
    table, alleles, counts = out[0]
    lines = [ln.split("\t") for ln in alleles.splitlines()]
    assert lines[0] == C.ALLELE_COLUMNS and len(lines) > 20
    assert {ln[5] for ln in lines[1:]} == set(kinds)
    # against the referee: the VCF's single-letter alleles of the region, in the file's order
    name = "aux24" if "-x" in flags else "n20_nrg"
    rows = []
    n_other = n_lacks = n_beyond = 0
    for chrom, pos1, vid, ref, alts in A.vcf_records(names, seqs):
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
    records, status = A.allele_sites(seqs, name, [(names.index(c), p - 1, ref, alt) for c, p, _, ref, alt in rows], key="genome")
    assert n_other == 3 and n_lacks == 1 and status.count(1) == 1 and status.count(2) == 1
    assert counts == ("alleles: %d SNVs examined, %d records; skipped: %d other alleles, %d records on chromosomes the reference lacks, 0 beyond a contig's end, "
                      "%d with another REF than the reference, %d on a base that is not A C G T, %d with ALT equal to the reference"
                      % (status.count(0), len(records), n_other, n_lacks, status.count(1), status.count(2), status.count(3)))
    want = [r for r in records if C.ALLELE_KINDS[r[8]] in kinds]
    assert len(want) == len(lines) - 1
    pat = A.pattern_of(C, name)
    for ln, r in zip(lines[1:], want):
        chrom, pos1, vid, ref, alt = rows[r[7]]
        lo, hi = (r[1], r[1] + L) if r[2] < 0 else (min(r[1], r[2]), max(r[1] + L, r[2] + r[5]))
        assert ln[:11] == [chrom, str(pos1), vid or ".", ref, alt, C.ALLELE_KINDS[r[8]], str(lo), str(hi), r[3].decode(), str(r[4]), str(r[10])]
        assert ln[13] == (str(r[9]) if r[8] == 3 else ".")
        allele = seqs[1][:pos1 - 1] + alt + seqs[1][pos1:] if r[8] & 1 else seqs[1]
        proto, pam = allele[r[1]:r[1] + L].upper(), allele[r[2]:r[2] + r[5]].upper()
        if r[3] == b"-":
            proto, pam = R.revcomp(proto), R.revcomp(pam)
        assert ln[11] == proto + pat.pams[r[4]] and ln[12] == pam


def test_the_tools_refuse_one_flag_without_the_other(tmp_path, genome):
    ctx, names, seqs = genome
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    vcf = A.write_vcf(str(tmp_path / "v.vcf"), names, seqs)
    out = str(tmp_path / "a.tsv")
    for tool in TOOLS:
        base = tool + ["-i", "N" * 20 + "nrg", "-r", fa, "--device", "-1", "-c", "chrC"]
        for extra in (["--alleles", vcf], ["--allele-sites", out], ["--allele-kinds", "alt"]):
            r = _run(base + extra)
            assert r.returncode != 0 and "--allele-sites" in r.stderr
        r = _run(base + ["--alleles", vcf, "--allele-sites", out, "--allele-kinds", "alt,neither"])
        assert r.returncode != 0 and "--allele-kinds" in r.stderr
        r = _run(base + ["--alleles", vcf, "--allele-sites", out, "--allele-kinds", "both"])
        assert r.returncode == 0, r.stderr
