"""End-to-end parity helpers shared by the GPU test modules: a seeded synthetic FASTA, the product's rows through every tail path
and kernel variant (product_rows), the oracle's rows for the same search (oracle_rows), and the row comparison (assert_same)."""
import json
import os

import oracle_lib as O
from fasta_util import write_fasta

SKIP_COLS = {"aligner_version", "time_stamp"}


def product_rows(C, fasta, guide, aux=(), chrom=None, paths=None, **kw):
    pk = dict(window_size=kw.get("window_size", 1000), max_guide_diffs=kw.get("d", 5), max_pam_mismatches=kw.get("p", 1),
              max_gaps_between_guide_and_pam=kw.get("g", 3), max_total_diffs=kw.get("D"), max_overlap=kw.get("O", 10),
              eqx_by_score=(1 if kw.get("switches", 0) & 2 else 0) | (2 if kw.get("switches", 0) & 1 else 0))   # oracle bits -> ABI bits
    for k in ("guide_mismatch_net_cost", "pam_mismatch_net_cost", "genome_gap_net_cost", "guide_gap_net_cost"):
        if k in kw:
            pk[k] = kw[k]
    # the fused call (calitas_search_hits: filter, removeOverlaps, sorts and rows on the device) and the two-stage call
    # (calitas_search + calitas_hits_tsv: the same stages on the host) must agree byte for byte
    ctx = C.Context(0)
    ctx.set_reference_fasta(fasta)
    try:
        text, n = C.SearchReference(guide=guide, guide_id="a", context=ctx, auxiliary_pams=aux, chrom=chrom, **pk).run("v0", "stamp")
        if paths is not None:
            paths.append(ctx.timing()["binned_lanes"])
        text2, n2 = C.SearchReference(guide=guide, guide_id="a", context=ctx, auxiliary_pams=aux, chrom=chrom, two_stage=True, **pk).run("v0", "stamp")
        # ... and so must the general device kernels (select.hip / hits.hip), which the per-bin kernels (binned.hip) stand in front of
        os.environ["CALITAS_BINNED"] = "0"
        try:
            text3, n3 = C.SearchReference(guide=guide, guide_id="a", context=ctx, auxiliary_pams=aux, chrom=chrom, **pk).run("v0", "stamp")
            assert ctx.timing()["binned_lanes"] == 0
        finally:
            del os.environ["CALITAS_BINNED"]
        os.environ["CALITAS_BINNED_COMPLEX"] = "1"     # binned.hip's wave-per-bin kernel for every bin (by default: the crowded ones)
        try:
            text4, _ = C.SearchReference(guide=guide, guide_id="a", context=ctx, auxiliary_pams=aux, chrom=chrom, **pk).run("v0", "stamp")
        finally:
            del os.environ["CALITAS_BINNED_COMPLEX"]
        assert text4 == text
        # align_kernel packs three jobs of 21 lanes into a wave for guides of up to 20 rows; two jobs of 32 lanes must give the same bytes
        os.environ["CALITAS_ALIGN_LPJ"] = "32"
        try:
            text5, _ = C.SearchReference(guide=guide, guide_id="a", context=ctx, auxiliary_pams=aux, chrom=chrom, **pk).run("v0", "stamp")
        finally:
            del os.environ["CALITAS_ALIGN_LPJ"]
        assert text5 == text, "align_kernel with two and with three jobs per wave differ"
        # one job per lane group (align_kernel) against two in sixteen-bit halves (align_pk_kernel, the default where the cells fit)
        os.environ["CALITAS_ALIGN_PACK"] = "0"
        try:
            text7, _ = C.SearchReference(guide=guide, guide_id="a", context=ctx, auxiliary_pams=aux, chrom=chrom, **pk).run("v0", "stamp")
        finally:
            del os.environ["CALITAS_ALIGN_PACK"]
        assert text7 == text, "align_kernel and align_pk_kernel differ"
        # the lane's small inputs as separate stream commands instead of the one setup launch (kernels.hpp, LaneSetupArgs)
        os.environ["CALITAS_LANE_SETUP"] = "0"
        try:
            text6, _ = C.SearchReference(guide=guide, guide_id="a", context=ctx, auxiliary_pams=aux, chrom=chrom, **pk).run("v0", "stamp")
        finally:
            del os.environ["CALITAS_LANE_SETUP"]
        assert text6 == text, "setup launch and separate input commands differ"
        tm = ctx.timing()
        assert tm["scan_kernel_ms"] > 0 and tm["align_kernel_ms"] > 0 and tm["gpu_total_ms"] >= tm["align_kernel_ms"]   # (stamps or events)
    finally:
        ctx.close()
    assert n == n2 == n3
    assert text3 == text, "binned and general device kernels differ"
    if text != text2:
        a, b = text.splitlines(), text2.splitlines()
        diff = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y][:2]
        raise AssertionError("fused and two-stage hits.txt differ: %d vs %d lines, first differences: %s" % (len(a), len(b), diff))
    rows = C.read_hits(text)
    assert len(rows) == n
    return rows


def oracle_rows(fasta, guide, aux=(), chrom=None, **kw):
    ok = dict(window_size=kw.get("window_size", 1000), d=kw.get("d", 5), p=kw.get("p", 1), g=kw.get("g", 3),
              D=-1 if kw.get("D") is None else kw["D"], O=kw.get("O", 10), switches=kw.get("switches", 0), threads=4)
    if "guide_mismatch_net_cost" in kw: ok["m"] = kw["guide_mismatch_net_cost"]
    if "pam_mismatch_net_cost" in kw: ok["M"] = kw["pam_mismatch_net_cost"]
    if "genome_gap_net_cost" in kw: ok["b"] = kw["genome_gap_net_cost"]
    if "guide_gap_net_cost" in kw: ok["B"] = kw["guide_gap_net_cost"]
    _, rows, _ = O.search_reference(fasta, guide, "a", aux=aux, chrom=chrom or "", **ok)
    return rows


def assert_same(prod, orac, tag=""):
    def strip(rows):
        return [{k: v for k, v in r.items() if k not in SKIP_COLS} for r in rows]
    p, o = strip(prod), strip(orac)
    if p != o:
        ps = {json.dumps(r, sort_keys=True) for r in p}
        os_ = {json.dumps(r, sort_keys=True) for r in o}
        only_p = [json.loads(x) for x in sorted(ps - os_)][:3]
        only_o = [json.loads(x) for x in sorted(os_ - ps)][:3]
        raise AssertionError("%s: product %d rows, oracle %d rows\nonly product: %s\nonly oracle: %s" % (tag, len(p), len(o), only_p, only_o))



def synth_fasta(tmp_path, seed, guides, lengths=(60000, 35000, 1500, 700, 26, 12), extra=None, **kw):
    from calitas_amd import synth
    spec = [("ctg%d" % i, l) for i, l in enumerate(lengths)]
    glist = []
    for g in guides:
        G = __import__("calitas_amd").Guide(g)
        pam = G.pams[0] if G.pams else ""
        glist.append((G.guide, pam, G.pam_is_five_prime))
    names, seqs = synth.make_genome(spec, seed, guides=glist, sites_per_guide=60, softmask=0.4, tandem_frac=0.03,
                                    n_run_ends=kw.get("n_run_ends", 300), n_block=kw.get("n_block", 2500), step_hint=kw.get("step_hint", 971))
    contigs = [(n, s.tobytes().decode()) for n, s in zip(names, seqs)]
    if extra:
        contigs += extra
    return write_fasta(str(tmp_path / ("synth%d.fa" % seed)), contigs)
