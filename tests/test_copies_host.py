"""CPU tests of the copies count: calitas_count_copies_host (the host twin of the copies kernel, on a host-only context) against the
referee of copies_ref.py -- the planted genome, the site tests' host genome, regions, the sweep over every protospacer and key length,
the table-size steps, the errors -- and both FindGuides tools with the copies flags on the host twin (--device -1).  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import copies_ref as X
import site_filter_ref as F
import sites_ref as R
from fasta_util import write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N20_NRG = "NNNNNNNNNNNNNNNNNNNNnrg"


@pytest.fixture(scope="module")
def C():
    import calitas_amd
    return calitas_amd


def _open(C, names, seqs):
    ctx = C.Context(-1)
    ctx.set_reference(names, [s.encode() for s in seqs])
    return ctx


@pytest.fixture(scope="module")
def genomes(C):
    """{genome name: (host-only context, names, strings, {pattern: brute_sites listing})}."""
    names, seqs, expect = X.copies_genome()
    X.check_planted(seqs, expect)
    out = {"planted": (_open(C, names, seqs), names, seqs, {})}
    names, seqs = R.host_genome()
    out["host"] = (_open(C, names, seqs), names, seqs, {})
    yield out
    for g in out.values():
        g[0].close()


def _pattern(C, name):
    text, aux = X.pattern_string(name)
    return C.Guide(text, aux)


def _listing(genome, name):
    _, _, seqs, done = genome
    if name not in done:
        done[name] = R.brute_sites(seqs, *X.PATTERNS[name])
    return done[name]


def test_the_planted_cases(C, genomes):
    ctx, names, seqs, _ = genomes["planted"]
    _, _, expect = X.copies_genome()
    for case, name, K, key, n in expect:
        got = ctx.count_copies(_pattern(C, name), [key], key_length=K, host=True)
        assert got.dtype == np.uint64 and got.tolist() == [n], (case, name, K, key)


@pytest.mark.parametrize("which", ["planted", "host"])
@pytest.mark.parametrize("name, K", X.CASES)
def test_host_twin_equals_referee(C, genomes, which, name, K):
    ctx, names, seqs, _ = genomes[which]
    sites = _listing(genomes[which], name)
    counts, n_sites = X.copies(seqs, name, K, sites=sites)
    pat = _pattern(C, name)
    # every distinct key: the sum is the number of sites
    keys = sorted(counts)
    got = ctx.count_copies(pat, keys, key_length=K, host=True)
    assert got.tolist() == [counts[k] for k in keys]
    assert int(got.sum()) == n_sites == len(ctx.find_sites(pat, host=True)) > 0
    # ... with keys that do not occur, duplicates, lower case and U for T
    queries, want = X.queries_for(counts, K, seed=K * 100 + len(name))
    if name == "fixed_nrg":
        # a protospacer that stands in front of a PAM but that the pattern's own letters exclude
        other = next(k for k in sorted(X.copies(seqs, "n20_nrg", 20, sites=_listing(genomes[which], "n20_nrg"))[0]) if k != R.FIXED)
        queries.append(other)
        want.append(0)
        assert counts == {R.FIXED: n_sites}
    assert K == 1 or want.count(0) >= 50
    assert ctx.count_copies(pat, queries, key_length=K, host=True).tolist() == want
    if K == len(X.PATTERNS[name][0]):
        assert ctx.count_copies(pat, queries, host=True).tolist() == want            # key_length None: the protospacer's length
    # the per-contig calls add up to the whole-reference call, each is the referee's for that contig
    total = np.zeros(len(queries), dtype=np.uint64)
    for i in range(len(names)):
        part = ctx.count_copies(pat, queries, key_length=K, chrom=i, host=True)
        own = X.copies(seqs, name, K, chrom=i)[0]
        assert part.tolist() == [own.get(q.upper().replace("U", "T"), 0) for q in queries], names[i]
        total += part
    assert total.tolist() == want


@pytest.mark.parametrize("name, K", [("n20_nrg", 20), ("n20_nrg", 12), ("tttv_n20", 12), ("n21", 10)])
def test_regions(C, genomes, name, K):
    ctx, names, seqs, _ = genomes["planted"]
    pat = _pattern(C, name)
    whole, _ = X.copies(seqs, name, K, sites=_listing(genomes["planted"], name))
    keys = sorted(whole)
    for chrom, start, end in ((0, 100, 2000), (0, 1000, 1023), (0, 8183, 8206), (0, 8184, 8206), (0, 8183, 8205), (2, 200, None), (1, 0, 1223)):
        want, _ = X.copies(seqs, name, K, chrom=chrom, start=start, end=end)
        got = ctx.count_copies(pat, keys, key_length=K, chrom=names[chrom], start=start, end=end, host=True)
        assert got.tolist() == [want.get(k, 0) for k in keys], (chrom, start, end)
    # chrom None: the bounds apply to every contig
    want, _ = X.copies(seqs, name, K, start=50, end=900)
    assert ctx.count_copies(pat, keys, key_length=K, start=50, end=900, host=True).tolist() == [want.get(k, 0) for k in keys]


def sweep_key_lengths(L):
    return sorted({K for K in (1, L // 2, L - 1, L) if K >= 1})


@pytest.mark.parametrize("L", F.SWEEP_LENGTHS)
def test_sweep_of_protospacer_and_key_lengths(C, L):
    names, seqs = F.sweep_genome()
    sites = F.listing(L).sites
    ctx = _open(C, names, seqs)
    try:
        for K in sweep_key_lengths(L):
            counts = X.count_keys(sites, seqs, K, False)
            queries = sorted(counts) + X.absent_keys(counts, K, 10, seed=L * 40 + K)
            got = ctx.count_copies("N" * L, queries, key_length=K, host=True)
            assert got.tolist() == [counts.get(q, 0) for q in queries], (L, K)
            assert int(got.sum()) == len(sites)
    finally:
        ctx.close()


TABLE_STEPS = (0, 1, 2, 3, 4, 5, 1023, 1024, 1025, None)     # distinct keys in a call; None: every one the contig holds (a dense table)


@pytest.fixture(scope="module")
def random_contig(C):
    names, seqs = X.random_contig()
    counts, n_sites = X.copies(seqs, "n20_nrg", 8)
    ctx = _open(C, names, seqs)
    yield ctx, counts, n_sites
    ctx.close()


@pytest.mark.parametrize("n", TABLE_STEPS)
def test_table_size_steps(C, random_contig, n):
    ctx, counts, n_sites = random_contig
    keys = sorted(counts)
    assert len(keys) > 4096
    queries = keys[::max(1, len(keys) // 1100)][:n] if n is not None else keys
    assert len(queries) == (len(keys) if n is None else n)
    got = ctx.count_copies(N20_NRG, queries, key_length=8, host=True)
    assert got.shape == (len(queries),) and got.tolist() == [counts[k] for k in queries]
    if n is None:
        assert int(got.sum()) == n_sites


def test_errors(C, genomes):
    ctx, names, seqs, _ = genomes["planted"]
    EINVAL = C._lib.EINVAL
    for K, queries in ((-1, []), (21, ["A" * 21])):
        with pytest.raises(C.CalitasError) as e:
            ctx.count_copies(N20_NRG, queries, key_length=K, host=True)
        assert e.value.code == EINVAL and "key_length" in str(e.value)
    with pytest.raises(C.CalitasError) as e:
        ctx.count_copies(N20_NRG, ["ACGT" * 5] * 3 + ["ACGTN" * 4, "ACGT" * 5], host=True)
    assert e.value.code == EINVAL and "queries[3]" in str(e.value)
    # more queries than a call takes, in a zero-filled buffer: the count is refused before any letter is looked at
    g = C.Guide(N20_NRG).to_c()
    n = (1 << 24) + 1
    buf = ctypes.create_string_buffer(n)
    out = np.zeros(n, dtype=np.uint64)
    rc = C._lib.lib.calitas_count_copies_host(ctx._h, ctypes.byref(g), 1, -1, 0, 0, buf, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    assert rc == EINVAL
    with pytest.raises(C.CalitasError) as e:
        C._lib.check(ctx._h, rc)
    assert "n_queries" in str(e.value)
    with pytest.raises(ValueError):
        ctx.count_copies(N20_NRG, ["ACGT"], host=True)                       # not the key's length
    assert ctx.count_copies(N20_NRG, [], host=True).shape == (0,)            # no query is legal
    # the device call on a host-only context
    with pytest.raises(C.CalitasError) as e:
        ctx.count_copies(N20_NRG, ["ACGT" * 5])
    assert e.value.code == C._lib.ENODEV and "no CPU fallback" in str(e.value)
    # a region on an absent contig
    part = C.Context(-1)
    part.set_reference(["a", "b"], [b"ACGTACGTACGTACGTACGTACGTAGGACGT", None], lengths=[31, 500])
    assert part.count_copies(N20_NRG, ["ACGT" * 5], chrom="a", host=True).tolist() == [1]
    for chrom in ("b", None):
        with pytest.raises(C.CalitasError) as e:
            part.count_copies(N20_NRG, ["ACGT" * 5], chrom=chrom, host=True)
        assert e.value.code == EINVAL and "absent" in str(e.value)
    part.close()


def test_guide_copies_and_the_table(C, genomes):
    ctx, names, seqs, _ = genomes["host"]
    rows = C.find_guides(ctx, N20_NRG, chrom="chrA", start=0, end=1100, host=True)
    whole, _ = X.copies(seqs, "n20_nrg", 20, sites=_listing(genomes["host"], "n20_nrg"))
    seeds, _ = X.copies(seqs, "n20_nrg", 12, sites=_listing(genomes["host"], "n20_nrg"))
    copies = C.guide_copies(ctx, N20_NRG, rows, host=True)
    seed = C.guide_copies(ctx, N20_NRG, rows, key_length=12, host=True)
    # over the whole reference, whatever region the rows come from
    assert copies == [whole[r.guide[:20]] for r in rows] and max(copies) >= 10
    assert seed == [seeds[r.guide[8:20]] for r in rows]
    lines = C.guides_tsv(rows, copies=copies, seed_copies=seed).splitlines()
    assert lines[0].split("\t") == C.tools.GUIDE_COLUMNS + ["copies", "seed_copies"]
    assert [ln.split("\t") for ln in lines[1:]] == [[str(x) for x in r.row()] + [str(a), str(b)] for r, a, b in zip(rows, copies, seed)]
    tables = {r.guide: np.ones((2, 2, 1, 1), dtype=np.uint64) for r in rows}
    head = C.guides_tsv(rows, tables, copies=copies).splitlines()[0].split("\t")
    assert head == C.tools.GUIDE_COLUMNS + ["copies", "hits", "hits_mm0", "hits_mm1"]            # behind pam_sequence, before hits
    assert C.guides_tsv(rows, seed_copies=seed).splitlines()[0].split("\t") == C.tools.GUIDE_COLUMNS + ["seed_copies"]
    # a 5' PAM: the protospacer is the string's tail, the seed its first bases
    rows5 = C.find_guides(ctx, "tttvNNNNNNNNNNNNNNNNNNNN", host=True)
    seeds5, _ = X.copies(seqs, "tttv_n20", 12, sites=_listing(genomes["host"], "tttv_n20"))
    assert C.guide_copies(ctx, "tttvNNNNNNNNNNNNNNNNNNNN", rows5, key_length=12, host=True) == [seeds5[r.guide[4:16]] for r in rows5]


def test_both_tools_with_the_copies_flags_on_the_host_twin(C, genomes, tmp_path):
    ctx, names, seqs, _ = genomes["host"]
    fa = write_fasta(str(tmp_path / "g.fa"), list(zip(names, seqs)))
    binary = os.path.join(ROOT, "calitas_amd", "calitas")
    env = dict(os.environ, PYTHONPATH=ROOT)
    whole, _ = X.copies(seqs, "n20_nrg", 20, sites=_listing(genomes["host"], "n20_nrg"))
    rows = C.find_guides(ctx, N20_NRG, chrom="chrA", start=350, end=1100, host=True)
    copies = [whole[r.guide[:20]] for r in rows]
    region = ["-i", N20_NRG, "-c", "chrA", "-s", "350", "-e", "1100"]

    def run(tool, out, flags):
        head = [sys.executable, "-m", "calitas_amd"] if tool == "py" else [binary]
        subprocess.check_call(head + ["FindGuides", "-r", fa, "-o", out, "--device", "-1"] + region + flags, env=env, cwd=ROOT)
        return open(out, "rb").read()

    # without the new flags: what the table has always been
    assert run("py", str(tmp_path / "plain.tsv"), []).decode() == C.guides_tsv(rows)
    # --max-copies 1 drops exactly the rows the referee says; the kept rows keep their guide_ids
    kept = [(r, n) for r, n in zip(rows, copies) if n <= 1]
    assert 0 < len(kept) < len(rows)
    text = run("py", str(tmp_path / "max1.tsv"), ["--max-copies", "1"])
    assert text.decode() == C.guides_tsv([r for r, _ in kept], copies=[n for _, n in kept])
    assert text == run("cc", str(tmp_path / "max1_cc.tsv"), ["--max-copies", "1"])
    # both tools, byte for byte
    flags = ["--copies", "--seed-copies", "12", "--max-copies", "2"]
    a, b = run("py", str(tmp_path / "py.tsv"), flags), run("cc", str(tmp_path / "cc.tsv"), flags)
    assert a == b and a.count(b"\n") > 3
    lines = a.decode().splitlines()
    assert lines[0].split("\t") == C.tools.GUIDE_COLUMNS + ["copies", "seed_copies"]
    assert [ln.split("\t")[0] for ln in lines[1:]] == [r.guide_id for r, n in zip(rows, copies) if n <= 2]
    flags = ["--seed-copies", "12", "--max-seed-copies", "1"]
    a, b = run("py", str(tmp_path / "py2.tsv"), flags), run("cc", str(tmp_path / "cc2.tsv"), flags)
    assert a == b and all(ln.split("\t")[-1] == "1" for ln in a.decode().splitlines()[1:])
    # the flags' own rules
    for bad in (["--max-copies", "0"], ["--max-seed-copies", "3"], ["--seed-copies", "21"], ["--seed-copies", "0"]):
        for tool in ("py", "cc"):
            with pytest.raises(subprocess.CalledProcessError):
                head = [sys.executable, "-m", "calitas_amd"] if tool == "py" else [binary]
                subprocess.check_call(head + ["FindGuides", "-r", fa, "--device", "-1"] + region + bad, env=env, cwd=ROOT,
                                      stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
