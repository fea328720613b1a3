"""Mirrors of SequentialGuideAligner's per-target entry points and of the two small tools built on them, on top of
calitas_align_windows (GPU).  Reference: SequentialGuideAligner.scala:228-418, PairwiseAlignSequences.scala:24-87,
AlignToReference.scala:34-148.  Padded strings keep the case of the target bytes, as the reference does."""
import ctypes

from . import _lib
from ._lib import AlnT, GuideT, lib
from .aligner import Alignment, Context, Defaults, Guide, SiteFilter, iupac_revcomp, make_params


class GuideAlignment:
    """GuideAlignment (GuideAlignment.scala:72-183) with the padded strings materialised."""

    def __init__(self, rec, guide, target, target_offset, chrom="n/a"):
        self.chrom = chrom
        self.start_offset, self.end_offset = rec.start_offset, rec.end_offset
        self.guide_start_offset, self.guide_end_offset = rec.guide_start_offset, rec.guide_end_offset
        self.strand, self.score, self.cigar, self.ops = rec.strand, rec.score, rec.cigar, rec.ops
        pam = guide.pams[rec.pam_index] if rec.pam_index >= 0 and guide.pams else ""
        self.guide = (pam + guide.guide) if guide.pam_is_five_prime else (guide.guide + pam)  # GuideAlignment.guide
        g, a = guide.to_c(), rec.to_c()
        bufs = [ctypes.create_string_buffer(_lib.MAX_OPS + 1) for _ in range(3)]
        rc = lib.calitas_padded_strings_target(ctypes.byref(g), ctypes.byref(a), target, len(target), target_offset, *bufs)
        if rc != _lib.OK:
            raise _lib.CalitasError(rc, "calitas_padded_strings_target")
        self.padded_guide, self.padded_alignment, self.padded_target = (b.value.decode() for b in bufs)

    # GuideAlignment.scala:99-108
    @property
    def mismatches(self):
        return self.padded_alignment.count(".")

    @property
    def gap_bases(self):
        return self.padded_alignment.count("~")

    @property
    def edits(self):
        return self.mismatches + self.gap_bases

    def _count(self, lower, both_sides, mms, gaps):  # GuideAlignment.scala:139-163
        n, pg, pa = 0, self.padded_guide, self.padded_alignment
        for i, ch in enumerate(pa):
            if mms and ch == "." and pg[i].islower() == lower:
                n += 1
            elif gaps and ch == "~":
                gb = pg[i]
                me = gb != "-" and gb.islower() == lower
                if not me:
                    pi = i
                    while pi > 0 and pg[pi] == "-":
                        pi -= 1
                    ni = i
                    while ni < len(pg) - 1 and pg[ni] == "-":
                        ni += 1
                    prev, nxt = pg[pi], pg[ni]
                    if both_sides:
                        me = (prev == "-" or prev.islower() == lower) and (nxt == "-" or nxt.islower() == lower)
                    else:
                        me = (prev.isalpha() and prev.islower() == lower) or (nxt.isalpha() and nxt.islower() == lower)
                if me:
                    n += 1
        return n

    guide_mismatches = property(lambda s: s._count(False, False, True, False))
    guide_gap_bases = property(lambda s: s._count(False, False, False, True))
    pam_mismatches = property(lambda s: s._count(True, True, True, False))
    pam_gap_bases = property(lambda s: s._count(True, True, False, True))
    pam_mms_plus_gaps = property(lambda s: s._count(True, True, True, True))


class SequentialGuideAligner:
    """SequentialGuideAligner(refFile, costs) (SequentialGuideAligner.scala:170-175).  `ref` maps contig name -> bases
    (bytes, case preserved) for alignToRef."""

    def __init__(self, context=None, ref=None, mismatch_net_cost=Defaults.MismatchNetCost, genome_gap_net_cost=Defaults.GenomeGapNetCost,
                 guide_gap_net_cost=Defaults.GuideGapNetCost, pam_mismatch_net_cost=Defaults.PamMismatchNetCost, device=0, eqx_by_score=0):
        self.ctx = context or Context(device)
        self.ref = ref or {}
        self._costs = dict(guide_mismatch_net_cost=mismatch_net_cost, pam_mismatch_net_cost=pam_mismatch_net_cost,
                           genome_gap_net_cost=genome_gap_net_cost, guide_gap_net_cost=guide_gap_net_cost, eqx_by_score=eqx_by_score)

    def align_many(self, guides, targets, offsets=None, names=None, max_guide_diffs=None, max_gaps_between_guide_and_pam=
                   Defaults.MaxGapsBetweenGuideAndPam, max_pam_diffs=None, max_total_diffs=None, max_overlap=0):
        """One calitas_align_windows call for a list of (guide, target) tasks. max_guide_diffs=None selects alignBest's
        limits.  Returns a list (per task) of lists of GuideAlignment in the order align() returns them."""
        n = len(guides)
        tb = [t if isinstance(t, bytes) else t.encode() for t in targets]
        offsets = list(offsets) if offsets is not None else [0] * n
        cache = {}                                          # the variant branch passes one Guide object thousands of times
        keep = [cache[id(g)] if id(g) in cache else cache.setdefault(id(g), g.to_c()) for g in guides]
        garr = (GuideT * max(1, n))(*keep)
        tptr = (ctypes.c_void_p * max(1, n))(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in tb])
        tlen = (ctypes.c_uint32 * max(1, n))(*[len(b) for b in tb])
        toff = (ctypes.c_int32 * max(1, n))(*offsets)
        if max_guide_diffs is None:
            params = make_params(max_guide_diffs=-1, max_gaps_between_guide_and_pam=max_gaps_between_guide_and_pam, **self._costs)
        else:
            params = make_params(max_guide_diffs=max_guide_diffs, max_pam_mismatches=max_pam_diffs,
                                 max_gaps_between_guide_and_pam=max_gaps_between_guide_and_pam, max_total_diffs=max_total_diffs,
                                 max_overlap=max_overlap, **self._costs)
        out, cnt, counts = ctypes.POINTER(AlnT)(), ctypes.c_uint64(), ctypes.POINTER(ctypes.c_uint32)()
        _lib.check(self.ctx._h, lib.calitas_align_windows(self.ctx._h, n, garr, tptr, tlen, toff, ctypes.byref(params), ctypes.byref(out),
                                                          ctypes.byref(cnt), ctypes.byref(counts)))
        try:
            res, k = [], 0
            for t in range(n):
                lst = []
                for _ in range(counts[t]):
                    lst.append(GuideAlignment(Alignment(out[k]), guides[t], tb[t], offsets[t], names[t] if names else "n/a"))
                    k += 1
                res.append(lst)
            return res
        finally:
            lib.calitas_free(out)
            lib.calitas_free(counts)

    def align(self, guide, target, max_guide_diffs, max_gaps_between_guide_and_pam, max_pam_diffs, max_total_diffs, max_overlap=0,
              target_name="n/a", target_offset=0):
        """SequentialGuideAligner.align (SequentialGuideAligner.scala:228-323)."""
        return self.align_many([guide], [target], [target_offset], [target_name], max_guide_diffs, max_gaps_between_guide_and_pam,
                               max_pam_diffs, max_total_diffs, max_overlap)[0]

    def align_best(self, guide, target, max_gaps_between_guide_and_pam=Defaults.MaxGapsBetweenGuideAndPam):
        """alignBest (SequentialGuideAligner.scala:333-345): maxBy(score) keeps the first maximum."""
        alns = self.align_many([guide], [target], max_gaps_between_guide_and_pam=max_gaps_between_guide_and_pam)[0]
        if not alns:
            raise ValueError("empty.maxBy")
        return max(alns, key=lambda a: a.score)  # max() returns the first maximal element

    def _region(self, guide, chrom, pos, window_size):
        if chrom not in self.ref:
            raise ValueError("Unknown chromosome: %s" % chrom)
        contig = self.ref[chrom]
        padding = window_size // 2 if window_size else guide.length * 2            # SequentialGuideAligner.scala:372
        start, end = max(pos - padding, 1), min(pos + padding, len(contig))         # :373
        return contig[start - 1:end], start - 1

    def align_to_ref(self, guide, chrom, pos, window_size=None, max_guide_diffs=None, max_gaps_between_guide_and_pam=
                     Defaults.MaxGapsBetweenGuideAndPam, max_pam_diffs=None, max_total_diffs=None, max_overlap=0):
        """alignToRef (SequentialGuideAligner.scala:359-387): result sorted by (score desc, gap bases asc)."""
        target, off = self._region(guide, chrom, pos, window_size)
        alns = self.align_many([guide], [target], [off], [chrom], max_guide_diffs, max_gaps_between_guide_and_pam, max_pam_diffs,
                               max_total_diffs, max_overlap)[0]
        return sorted(alns, key=lambda a: (-a.score, a.gap_bases))                 # stable, GuideAlignment.scala:125-129

    def align_to_ref_best(self, guide, chrom, pos, window_size=None, max_gaps_between_guide_and_pam=Defaults.MaxGapsBetweenGuideAndPam):
        """alignToRefBest (SequentialGuideAligner.scala:402-418)."""
        return self.align_to_ref(guide, chrom, pos, window_size, None, max_gaps_between_guide_and_pam)[0]


def pairwise_align_sequences(input_path, output_path, max_gaps_between_guide_and_pam=Defaults.MaxGapsBetweenGuideAndPam, aligner=None,
                             **costs):
    """PairwiseAlignSequences.execute (PairwiseAlignSequences.scala:42-85): `query target` per line -> 11-column TSV.
    (`-O` is declared but unused by the reference, so it is not a parameter here.)"""
    aligner = aligner or SequentialGuideAligner(**costs)
    tasks = []
    with open(input_path) as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            fields = line.split()
            if len(fields) != 2:
                raise ValueError("Line found with %d fields: %s" % (len(fields), " ".join(fields)))
            tasks.append((fields[0], fields[1].upper()))
    cols = ["query", "target", "score", "query_start", "target_start", "cigar", "mismatches", "gap_bases", "padded_query", "alignment",
            "padded_target"]
    with open(output_path, "w") as out:
        out.write("\t".join(cols) + "\n")
        for b in range(0, len(tasks), 10000):
            batch = tasks[b:b + 10000]
            res = aligner.align_many([Guide(q) for q, _ in batch], [t for _, t in batch],
                                     max_gaps_between_guide_and_pam=max_gaps_between_guide_and_pam)
            for (q, t), alns in zip(batch, res):
                a = max(alns, key=lambda x: x.score)
                out.write("\t".join(str(x) for x in (q, t, a.score, 1, a.start_offset, a.cigar, a.mismatches, a.gap_bases, a.padded_guide,
                                                     a.padded_alignment, a.padded_target)) + "\n")


def read_fasta(path):
    """Contig name -> bases (bytes, case preserved), in file order."""
    ref, name, parts = {}, None, []
    with open(path, "rb") as f:
        for line in f:
            line = line.rstrip(b"\r\n")
            if not line:
                continue
            if line.startswith(b">"):
                if name is not None:
                    ref[name] = b"".join(parts)
                name, parts = line[1:].split()[0].decode(), []
            elif name is not None:
                parts.append(line)
    if name is not None:
        ref[name] = b"".join(parts)
    return ref


_COMP = bytes.maketrans(b"ACGTUMKRYVBHDWSNacgtumkryvbhdwsn", b"TGCAAKMYRBVDHWSNtgcaakmyrbvdhwsn")

HIT_COLUMNS = ["guide_id", "unpadded_guide_sequence", "genome_build", "chromosome", "coordinate_start", "coordinate_end", "strand",
               "unpadded_target_sequence", "ten_bases_5_prime", "ten_bases_3_prime", "pam_used", "variant_id", "variant_description",
               "variant_vcf", "allele_frequency", "score", "guide_mm", "guide_gaps", "guide_mm_plus_gaps", "pam_mm", "total_mm_plus_gaps",
               "padded_guide", "padded_alignment", "padded_target", "padded_extra_8_bases_5_prime", "padded_extra_8_bases_3_prime", "cigar",
               "unpadded_guide_sequence_length", "unpadded_target_sequence_length", "aligner", "aligner_version", "aligner_search_pam",
               "aligner_other_parameters", "time_stamp"]


def reference_hit_row(aln, guide, guide_id, contig, genome_build, aligner_id, version, arguments, time_stamp):
    """ReferenceHit.Builder.build without variants (ReferenceHit.scala:210-254) for a tools.GuideAlignment on `contig` (bytes)."""
    neg = aln.strand == "-"

    def fetch(start, end):                                      # fetchBases ReferenceHit.scala:261-266, 1-based closed
        a_s, a_e = max(1, start), min(len(contig), end)
        bases = b"N" * (a_s - start) + contig[a_s - 1:a_e] + b"N" * (end - a_e)
        if neg:
            bases = bases.translate(_COMP)[::-1]
        return bases.decode().upper()

    ten_left, ten_right = fetch(aln.guide_start_offset + 1 - 10, aln.guide_start_offset), fetch(aln.guide_end_offset + 1, aln.guide_end_offset + 10)
    eight_left, eight_right = fetch(aln.start_offset + 1 - 8, aln.start_offset), fetch(aln.end_offset + 1, aln.end_offset + 8)
    pg, pt = aln.padded_guide, aln.padded_target
    ups = [i for i, ch in enumerate(pg) if ch.isupper()]        # unpaddedTargetWithoutPam GuideAlignment.scala:111-115
    unpadded_target = "".join(ch for ch in pt[ups[0]:ups[-1] + 1] if ch != "-")
    row = [guide_id, guide.guide, genome_build, aln.chrom, aln.guide_start_offset, aln.guide_end_offset, aln.strand, unpadded_target,
           ten_right if neg else ten_left, ten_left if neg else ten_right, "".join(ch for ch in aln.guide if ch.islower()), "", "", "", "",
           aln.score, aln.guide_mismatches, aln.guide_gap_bases, aln.guide_mismatches + aln.guide_gap_bases, aln.pam_mismatches, aln.edits,
           pg, aln.padded_alignment, pt, eight_right if neg else eight_left, eight_left if neg else eight_right, aln.cigar, len(guide.guide),
           len(unpadded_target), aligner_id, version, ",".join(guide.pams), arguments, time_stamp]
    return "\t".join(str(x) for x in row)


def align_to_reference(input_path, ref, output_path=None, window_size=None, max_guide_diffs=None, max_pam_mismatches=None,
                       max_gaps_between_guide_and_pam=Defaults.MaxGapsBetweenGuideAndPam, max_total_diffs=None, max_overlap=None,
                       guide_mismatch_net_cost=Defaults.MismatchNetCost, pam_mismatch_net_cost=Defaults.PamMismatchNetCost,
                       genome_gap_net_cost=Defaults.GenomeGapNetCost, guide_gap_net_cost=Defaults.GuideGapNetCost, threads=8, context=None,
                       device=0, version=None, time_stamp=None, eqx_by_score=0):
    """AlignToReference.execute (AlignToReference.scala:95-146): a tab-delimited file with a header (id optional, query, chrom,
    position) -> ReferenceHit rows.  All of -d/-p/-O given: every alignment meeting them (alignToRef); none given: the single best
    alignment per query (alignToRefBest).  Batches of 10000 tasks go to the GPU in one calitas_align_windows call each and are
    sorted on their own (AlignToReference.scala:104,140).  `threads` is accepted and ignored.  Returns the TSV text."""
    import time as _time
    given = [x is not None for x in (max_guide_diffs, max_pam_mismatches, max_overlap)]
    if any(given) and not all(given):
        raise ValueError("Must specify all or none of: --max-guide-diffs, --max-pam-mismatches, --max-overlap")
    limits = all(given)
    contigs = read_fasta(ref)
    ctx = context or Context(device)
    own = context is None
    try:
        if not ctx.contig_names:
            ctx.set_reference_fasta(ref)
        genome_build = ctx.genome_build()
        order = {n: i for i, n in enumerate(ctx.contig_names)}
        aligner = SequentialGuideAligner(context=ctx, ref=contigs, mismatch_net_cost=guide_mismatch_net_cost,
                                         genome_gap_net_cost=genome_gap_net_cost, guide_gap_net_cost=guide_gap_net_cost,
                                         pam_mismatch_net_cost=pam_mismatch_net_cost, eqx_by_score=eqx_by_score)
        opt = lambda v: "Some(%d)" % v if v is not None else "None"          # Scala prints the Option-typed flags this way
        arguments = ";".join(sorted("%s=%s" % kv for kv in {
            "max-guide-diffs": opt(max_guide_diffs), "max-pam-mismatches": opt(max_pam_mismatches),
            "max-gaps-between-guide-and-pam": max_gaps_between_guide_and_pam, "max-overlap": opt(max_overlap),
            "guide-mismatch-net-cost": guide_mismatch_net_cost, "pam-mismatch-net-cost": pam_mismatch_net_cost,
            "genome-gap-net-cost": genome_gap_net_cost, "guide-gap-net-cost": guide_gap_net_cost}.items()))   # AlignToReference.scala:70-79
        version = version or _time.strftime("unknown-%Y-%m-%d", _time.gmtime())
        time_stamp = time_stamp or _time.strftime("%a %b %d %H:%M:%S UTC %Y", _time.gmtime())

        tasks = []
        with open(input_path) as f:
            header = f.readline().rstrip("\r\n").split("\t")
            for need in ("query", "chrom", "position"):
                if need not in header:
                    raise ValueError("input needs the columns query, chrom and position")
            for line in f:
                line = line.rstrip("\r\n")
                if not line:
                    continue
                row = dict(zip(header, line.split("\t")))
                tasks.append((row.get("id") or row["query"], row["query"], row["chrom"], int(row["position"])))

        lines = ["\t".join(HIT_COLUMNS)]
        for b0 in range(0, len(tasks), 10000):
            batch = tasks[b0:b0 + 10000]
            guides = [Guide(q) for _, q, _, _ in batch]
            regions = [aligner._region(g, chrom, pos, window_size) for g, (_, _, chrom, pos) in zip(guides, batch)]
            D = None
            if limits:
                D = max_total_diffs if max_total_diffs is not None else max_guide_diffs + max_gaps_between_guide_and_pam + max_pam_mismatches
            res = aligner.align_many(guides, [t for t, _ in regions], [o for _, o in regions], [c for _, _, c, _ in batch],
                                     max_guide_diffs if limits else None, max_gaps_between_guide_and_pam,
                                     max_pam_mismatches if limits else None, D, max_overlap if limits else 0)
            hits = []
            for (tid, _, chrom, _), g, alns in zip(batch, guides, res):
                alns = sorted(alns, key=lambda a: (-a.score, a.gap_bases))    # alignToRef's order, SequentialGuideAligner.scala:386
                if not limits:
                    if not alns:
                        raise ValueError("head of empty list")
                    alns = alns[:1]
                for a in alns:
                    key = (order[chrom], a.guide_start_offset, a.strand, -a.score)               # ReferenceHit.scala:284
                    hits.append((key, reference_hit_row(a, g, tid, contigs[chrom], genome_build, "CALITAS:AlignToReference", version,
                                                        arguments, time_stamp)))
            hits.sort(key=lambda h: h[0])                                     # stable
            lines += [r for _, r in hits]
        text = "\n".join(lines) + "\n"
        if output_path is not None:
            with open(output_path, "w") as f:
                f.write(text)
        return text
    finally:
        if own:
            ctx.close()


# ---- FindGuides: the sites of an IUPAC pattern as guides a search takes (no reference counterpart) ----

GUIDE_COLUMNS = ["guide_id", "chromosome", "start", "end", "strand", "pam_index", "guide", "pam_sequence"]
_RC = str.maketrans("ACGTU", "TGCAA")


class GuideSite:
    """One site of Context.find_sites as a guide: `guide` is the `-i` string a search takes -- the protospacer as it reads on the site's
    strand, upper case, with the PATTERN's matched PAM in lower case behind it (in front of it for a 5' PAM) -- and pam_sequence the
    genomic PAM bases on that strand; [start, end) is the footprint (protospacer + PAM), 0-based half-open."""
    __slots__ = ("chromosome", "start", "end", "strand", "pam_index", "guide", "pam_sequence", "protospacer_start", "activity_q16", "region_class", "mh_total_q16",
                 "mh_oof_q16")

    def __init__(self, *v):
        self.mh_total_q16 = self.mh_oof_q16 = None     # (find_guides with a microhomology model: the site's two sums, MH_NONE where it has none)
        self.activity_q16 = None                       # (find_guides with a model: the site's score, ACTIVITY_NONE when it has none)
        self.region_class = None                       # (find_guides with classes or an extent: the site's class index under the context's regions)
        for k, x in zip(self.__slots__, v):
            setattr(self, k, x)

    @property
    def guide_id(self):
        return "%s:%d:%s" % (self.chromosome, self.start, self.strand)

    def row(self):
        return [self.guide_id, self.chromosome, self.start, self.end, self.strand, self.pam_index, self.guide, self.pam_sequence]


def find_guides(ctx, pattern, chrom=None, start=0, end=None, host=False, filter=None, activity=None, min_activity=None, classes=None, extent=None,
                by_regions=False, microhomology=None, mh_cut=None, min_out_of_frame=0):
    """Context.find_sites turned into guides: a list of GuideSite in the sites' order.  pattern: a Guide or its `-i` string; filter: a
    SiteFilter -- only the sites that pass it come back at all.  activity: an ActivityModel -- every GuideSite carries its site's
    on-target score as activity_q16 (Context.find_sites_scored; ACTIVITY_NONE where the site has none); min_activity: a Q16 integer,
    only the sites that score at least that much come back.  classes, extent (or by_regions=True for their defaults): only the sites
    whose class under the context's regions is one of `classes` come back (Context.find_sites_regions), each with its class index as
    region_class.  Together with activity both listings are made over the same region and joined on (contig, protospacer start,
    strand) in one walk over the two: both are in that order.  microhomology: a MicrohomologyModel -- every GuideSite carries its site's
    microhomology score around the cut as mh_total_q16 and mh_oof_q16 (Context.find_sites_microhomology; MH_NONE in both where the
    site has none); mh_cut: the cut's position in the protospacer as the guide reads (None: L - 3, with a 3' PAM); min_out_of_frame: a
    per-mille 0 .. 1000, only the sites whose out-of-frame share reaches it come back.  With activity or regions this listing is
    joined to the others in the same way."""
    if not isinstance(pattern, Guide):
        pattern = Guide(pattern)
    if microhomology is None and (mh_cut is not None or min_out_of_frame):
        raise ValueError("mh_cut and min_out_of_frame need a microhomology model")
    cls_of = mh = None
    plain = activity is None and classes is None and extent is None and not by_regions
    if microhomology is not None:
        mh_sites, mh_scores = ctx.find_sites_microhomology(pattern, microhomology, cut_offset=mh_cut, min_out_of_frame=min_out_of_frame, filter=filter,
                                                           chrom=chrom, start=start, end=end, host=host)
    if classes is not None or extent is not None or by_regions:
        if activity is None and min_activity is not None:
            raise ValueError("min_activity needs an activity model")
        sites, cls_of = ctx.find_sites_regions(pattern, classes=classes, extent=extent, filter=filter, chrom=chrom, start=start, end=end, host=host)
        q16 = None
        if activity is not None:
            scored, all_q16 = ctx.find_sites_scored(pattern, activity, min_score=min_activity, filter=filter, chrom=chrom, start=start, end=end, host=host)
            keep, q16, j = [], [], 0
            key = lambda r: (int(r["contig_index"]), int(r["protospacer_start"]), r["strand"] == b"-")
            for i in range(len(sites)):                # the merge walk: a classed site below the threshold has no partner and goes
                k = key(sites[i])
                while j < len(scored) and key(scored[j]) < k:
                    j += 1
                if j < len(scored) and key(scored[j]) == k:
                    keep.append(i)
                    q16.append(int(all_q16[j]))
            sites, cls_of = sites[keep], cls_of[keep]
    elif activity is None:
        if min_activity is not None:
            raise ValueError("min_activity needs an activity model")
        sites, q16 = (mh_sites if microhomology is not None else ctx.find_sites(pattern, chrom, start, end, host=host, filter=filter)), None
    else:
        sites, q16 = ctx.find_sites_scored(pattern, activity, min_score=min_activity, filter=filter, chrom=chrom, start=start, end=end, host=host)
    if microhomology is not None and plain:
        mh = mh_scores
    elif microhomology is not None:                    # the merge walk again: a site the per-mille dropped has no partner and goes
        keep, rows, j = [], [], 0
        key = lambda r: (int(r["contig_index"]), int(r["protospacer_start"]), r["strand"] == b"-")
        for i in range(len(sites)):
            k = key(sites[i])
            while j < len(mh_sites) and key(mh_sites[j]) < k:
                j += 1
            if j < len(mh_sites) and key(mh_sites[j]) == k:
                keep.append(i)
                rows.append(j)
        sites, mh = sites[keep], mh_scores[rows]
        q16 = None if q16 is None else [q16[i] for i in keep]
        cls_of = None if cls_of is None else cls_of[keep]
    out = []
    L = pattern.protospacer_length
    bounds = {}
    for s in sites:                                    # one fetch per contig: the stretch its footprints cover
        c, ps, pm, pl = int(s["contig_index"]), int(s["protospacer_start"]), int(s["pam_start"]), int(s["pam_length"])
        lo, hi = (ps, ps + L) if pm < 0 else (min(ps, pm), max(ps + L, pm + pl))
        b = bounds.get(c)
        bounds[c] = (lo, hi) if b is None else (min(b[0], lo), max(b[1], hi))
    text = {c: (lo, ctx.fetch_bases(c, lo, hi - lo)) for c, (lo, hi) in bounds.items()}
    for s in sites:
        c, ps, pm, pl = int(s["contig_index"]), int(s["protospacer_start"]), int(s["pam_start"]), int(s["pam_length"])
        minus = s["strand"] == b"-"
        off, t = text[c]
        proto = t[ps - off:ps - off + L]
        pam_seq = t[pm - off:pm - off + pl] if pm >= 0 else ""
        if minus:
            proto, pam_seq = proto.translate(_RC)[::-1], pam_seq.translate(_RC)[::-1]
        proto = proto.replace("U", "T")               # an ACGT guide
        k = int(s["pam_index"])
        pam = pattern.pams[k] if k >= 0 else ""
        lo, hi = (ps, ps + L) if pm < 0 else (min(ps, pm), max(ps + L, pm + pl))
        out.append(GuideSite(ctx.contig_names[c], lo, hi, "-" if minus else "+", k, (pam + proto) if pattern.pam_is_five_prime else (proto + pam),
                             pam_seq, ps))
        if q16 is not None:
            out[-1].activity_q16 = int(q16[len(out) - 1])
        if cls_of is not None:
            out[-1].region_class = int(cls_of[len(out) - 1])
        if mh is not None:
            out[-1].mh_total_q16, out[-1].mh_oof_q16 = int(mh[len(out) - 1]["total_q16"]), int(mh[len(out) - 1]["out_of_frame_q16"])
    return out


def guide_counts(ctx, guides, params, batch=64):
    """Off-target tables of distinct `-i` strings: {string: table of Context.search_counts}, searched in batches (search_counts_batch
    takes guides of one length, at most 64 at a time)."""
    by_len = {}
    for g in dict.fromkeys(guides):
        by_len.setdefault(len(g), []).append(g)
    tables = {}
    for same in by_len.values():
        for b in range(0, len(same), batch):
            part = same[b:b + batch]
            for g, t in zip(part, ctx.search_counts_batch([Guide(g) for g in part], params)):
                tables[g] = t
    return tables


def guide_scores(ctx, guides, params, model, batch=64):
    """guide_counts in score mode: {string: Scores of Context.search_scores} through search_scores_batch (the model's length is the
    guides' length)."""
    got = {}
    same = list(dict.fromkeys(guides))
    for b in range(0, len(same), batch):
        part = same[b:b + batch]
        for g, s in zip(part, ctx.search_scores_batch([Guide(g) for g in part], params, model)):
            got[g] = s
    return got


COPIES_MAX_QUERIES = 1 << 24                 # what one calitas_count_copies call takes


def guide_copies(ctx, pattern, rows, key_length=None, host=False):
    """Context.count_copies for the GuideSites of find_guides: per row the number of sites of `pattern` in the WHOLE resident reference
    -- whatever region the rows were listed in -- whose protospacer (key_length None) or PAM-proximal key_length bases equal the
    row's, the row's own site among them.  A list of ints aligned with rows."""
    if not isinstance(pattern, Guide):
        pattern = Guide(pattern)
    L = pattern.protospacer_length
    K = L if key_length is None else int(key_length)
    if not 1 <= K <= L:
        raise ValueError("the key length is 1 .. %d (the protospacer's length), not %d" % (L, K))
    five = pattern.pam_is_five_prime and bool(pattern.pams)
    keys = []
    for r in rows:
        proto = r.guide[len(r.guide) - L:] if five else r.guide[:L]
        keys.append(proto[:K] if five else proto[L - K:])
    out = []
    for at in range(0, len(keys), COPIES_MAX_QUERIES):           # the queries are independent: a call's worth at a time
        out += [int(x) for x in ctx.count_copies(pattern, keys[at:at + COPIES_MAX_QUERIES], key_length=K, host=host)]
    return out


def guide_near(ctx, pattern, rows, max_mismatches, key_length=None, host=False):
    """Context.count_near for the GuideSites of find_guides: per row the numbers of sites of `pattern` in the WHOLE resident reference
    whose protospacer (key_length None) or PAM-proximal key_length bases differ from the row's at exactly 0 .. max_mismatches
    positions, the row's own site in column 0.  A list of lists of ints aligned with rows."""
    if not isinstance(pattern, Guide):
        pattern = Guide(pattern)
    L = pattern.protospacer_length
    K = L if key_length is None else int(key_length)
    if not 1 <= K <= L:
        raise ValueError("the key length is 1 .. %d (the protospacer's length), not %d" % (L, K))
    five = pattern.pam_is_five_prime and bool(pattern.pams)
    keys = []
    for r in rows:
        proto = r.guide[len(r.guide) - L:] if five else r.guide[:L]
        keys.append(proto[:K] if five else proto[L - K:])
    out = []
    for at in range(0, len(keys), COPIES_MAX_QUERIES):           # the queries are independent: a call's worth at a time
        out += [[int(x) for x in row] for row in ctx.count_near(pattern, keys[at:at + COPIES_MAX_QUERIES], max_mismatches, key_length=K, host=host)]
    return out


def guide_near_scores(ctx, pattern, rows, max_mismatches, model, host=False):
    """Context.score_near for the GuideSites of find_guides: per row the near copies of its protospacer in the WHOLE resident
    reference -- guide_near's table -- and the sum and maximum of their scores under `model`, from one pass.  A NearScores aligned
    with rows."""
    import numpy as np
    from .aligner import NearScores
    if not isinstance(pattern, Guide):
        pattern = Guide(pattern)
    L = pattern.protospacer_length
    five = pattern.pam_is_five_prime and bool(pattern.pams)
    keys = [r.guide[len(r.guide) - L:] if five else r.guide[:L] for r in rows]
    M = int(max_mismatches)
    parts = [ctx.score_near(pattern, keys[at:at + COPIES_MAX_QUERIES], M, model, host=host)
             for at in range(0, len(keys), COPIES_MAX_QUERIES)]  # the queries are independent: a call's worth at a time
    if not parts:
        return ctx.score_near(pattern, [], M, model, host=host)
    return NearScores(np.concatenate([p.near for p in parts]), np.concatenate([p.sum_q32 for p in parts]), np.concatenate([p.max_q32 for p in parts]))


NEAR_LIST_COLUMNS = ["guide_id", "chromosome", "start", "end", "strand", "pam_index", "mismatches", "target", "score_q32", "score"]


def guide_near_list(ctx, pattern, rows, max_mismatches, model=None, limit=1000, host=False):
    """Context.list_near for the GuideSites of find_guides: per row the records of its protospacer's copies within max_mismatches
    substitutions in the WHOLE resident reference, its own site among them, scored under `model` (None: no weights).  A NearList
    aligned with rows; a row whose copies are more than `limit` lists nothing."""
    if not isinstance(pattern, Guide):
        pattern = Guide(pattern)
    L = pattern.protospacer_length
    five = pattern.pam_is_five_prime and bool(pattern.pams)
    keys = [r.guide[len(r.guide) - L:] if five else r.guide[:L] for r in rows]
    if len(keys) > COPIES_MAX_QUERIES:
        raise ValueError("more than %d guides: list them in pieces" % COPIES_MAX_QUERIES)
    return ctx.list_near(pattern, keys, int(max_mismatches), model, limit=limit, host=host)


def near_list_tsv(rows, names, listing):
    """The --near-list table: NEAR_LIST_COLUMNS, a line per record of `listing` (guide_near_list of `rows`) in the rows' and the
    records' order.  guide_id is the row's; chromosome (names: the contigs' names), start and end (0-based, half open), strand and
    pam_index are the copy's protospacer's; target is its letters as the guide reads them, lower case where they differ from the
    guide's; score is score_q32 / 2^32 (%.6f).  A row over the limit writes no line."""
    lines = ["\t".join(NEAR_LIST_COLUMNS)]
    for i, r in enumerate(rows):
        for h in listing.of(i):
            start = int(h["protospacer_start"])
            lines.append("\t".join([r.guide_id, names[int(h["contig_index"])], str(start), str(start + listing.L), h["strand"].decode(), str(int(h["pam_index"])),
                                    str(int(h["mismatches"])), listing.target(h), str(int(h["score_q32"])), "%.6f" % (int(h["score_q32"]) / 4294967296.0)]))
    return "\n".join(lines) + "\n"


PAIR_COLUMNS = ["pair_id", "left_guide_id", "right_guide_id", "chromosome", "left_cut", "right_cut", "distance", "left_strand", "right_strand", "orientation"]


def guide_pairs(ctx, pattern, rows, spec, chrom=None, start=0, end=None, host=False, filter=None):
    """Context.find_site_pairs for the GuideSites of find_guides: the pairs of the region's sites under `spec` (a SitePairs) both of
    whose members are among `rows` -- what is left of the listing after the other cuts (activity, regions, copies, near copies).
    pattern, filter and the region are those the rows were listed with.  The two listings are joined on (contig, protospacer start,
    strand).  A list of (left row, right row, left cut, right cut, distance, orientation) in the pairs' order, the first two indices
    into rows."""
    from .aligner import site_cut_of
    if not isinstance(pattern, Guide):
        pattern = Guide(pattern)
    sites, pairs = ctx.find_site_pairs(pattern, spec, filter=filter, chrom=chrom, start=start, end=end, host=host)
    at = {(r.chromosome, r.protospacer_start, r.strand): i for i, r in enumerate(rows)}
    row_of = [at.get((ctx.contig_names[int(s["contig_index"])], int(s["protospacer_start"]), s["strand"].decode())) for s in sites]
    L, c = pattern.protospacer_length, spec.cut_of(pattern)
    out = []
    for p in pairs:
        a, b = row_of[int(p["left"])], row_of[int(p["right"])]
        if a is None or b is None:
            continue
        cuts = [site_cut_of(rows[i].protospacer_start, rows[i].strand, L, c) for i in (a, b)]
        out.append((a, b, cuts[0], cuts[1], int(p["distance"]), int(p["orientation"])))
    return out


def pairs_tsv(rows, names, pairs):
    """The --pairs table: PAIR_COLUMNS, a line per pair of guide_pairs(rows) in its order, pair_id from 1.  names: what the four
    orientation codes are called (SitePairs.name_of: out / in / same, or the code itself for a PAM-less pattern); the cuts are 0-based
    positions between two bases of the chromosome: the number of bases to the cut's left."""
    lines = ["\t".join(PAIR_COLUMNS)]
    for k, (a, b, left_cut, right_cut, distance, o) in enumerate(pairs):
        lines.append("\t".join([str(k + 1), rows[a].guide_id, rows[b].guide_id, rows[a].chromosome, str(left_cut), str(right_cut), str(distance),
                                rows[a].strand, rows[b].strand, names[o]]))
    return "\n".join(lines) + "\n"


def site_pairs_of_flags(pattern, pairs=None, pair_distance=None, pair_cut=None, pair_orientation=None):
    """The SitePairs of FindGuides' --pair-* flags for `pattern` (a Guide), None without --pairs.  pair_distance "MIN:MAX" is required
    with --pairs; pair_cut N: default L - 3 with a 3' PAM, required otherwise; pair_orientation: out | in | same | any | CODE,...,
    default out."""
    from .aligner import PAIR_MAX_DISTANCE, SitePairs
    if pairs is None:
        if pair_distance is not None or pair_cut is not None or pair_orientation is not None:
            raise ValueError("--pair-distance, --pair-cut and --pair-orientation require --pairs FILE")
        return None
    if pair_distance is None:
        raise ValueError("--pairs requires --pair-distance MIN:MAX")
    a, sep, b = str(pair_distance).partition(":")
    if not (sep and a.isdigit() and b.isdigit() and len(a) <= 9 and len(b) <= 9):
        raise ValueError("--pair-distance MIN:MAX: two integers, 0 <= MIN <= MAX <= %d, not %s" % (PAIR_MAX_DISTANCE, pair_distance))
    if not int(a) <= int(b) <= PAIR_MAX_DISTANCE:
        raise ValueError("--pair-distance MIN:MAX: two integers, 0 <= MIN <= MAX <= %d, not %s" % (PAIR_MAX_DISTANCE, pair_distance))
    L = pattern.protospacer_length
    if pair_cut is None and not pattern.pam_is_three_prime:
        raise ValueError("--pair-cut N is required: the default, L - 3, is the Cas9 cut of a pattern with a 3' PAM")
    if pair_cut is not None and not (str(pair_cut).isdigit() and len(str(pair_cut)) <= 3 and int(pair_cut) <= L):
        raise ValueError("--pair-cut N: N is 0 .. %d, the protospacer's length, not %s" % (L, pair_cut))
    try:
        spec = SitePairs(int(a), int(b), None if pair_cut is None else int(pair_cut), "out" if pair_orientation is None else str(pair_orientation))
        spec.mask_of(pattern)
    except ValueError as e:
        raise ValueError("--pair-orientation: %s" % e)
    return spec


def activity_q16_of_flag(text):
    """--min-activity X as a Q16 integer: a decimal as in a model file (digits, at most one point, an optional sign), within what a
    score can be (+-2064 = 129 weights of 16.0), floor(x * 65536 + 0.5)."""
    import math
    import re
    text = str(text)
    if not re.fullmatch(r"[+-]?([0-9]+\.?[0-9]*|\.[0-9]+)", text, re.ASCII) or not -2064.0 <= float(text) <= 2064.0:
        raise ValueError("--min-activity X: X is a decimal in [-2064, 2064], not %s" % text)
    return int(math.floor(float(text) * 65536.0 + 0.5))


def guides_tsv(rows, tables=None, scores=None, copies=None, seed_copies=None, near=None, near_scores=None, activity=None, class_names=None,
               microhomology=None):
    """The FindGuides table: GUIDE_COLUMNS, one row per GuideSite; with tables (guide_counts) also hits -- the table's sum -- and
    hits_mm0 .. hits_mmE, the hits per number of protospacer mismatches, summed over strands, gaps and PAM mismatches; with scores
    (guide_scores) those columns come from the same pass's tables and perfect and specificity (%.6f) follow them.  copies,
    seed_copies: lists aligned with rows (guide_copies) -- the columns of those names, directly behind pam_sequence.  near: a list of
    rows of M + 1 counts aligned with rows (guide_near), or an array of that shape -- the columns copies_mm0 .. copies_mmM behind those.
    near_scores: a NearScores aligned with rows (guide_near_scores) -- near_sum_q32, near_max_q32 and near_specificity (%.6f) directly
    behind copies_mmM.  activity: the ActivityModel the rows were scored with (find_guides) -- activity_q16, the score as it is, and
    activity, the number its link makes of it (activity_value, %.6f), directly behind pam_sequence and before all of the above; NA in
    both for a site without a score.  class_names: the names of the regions' classes ("elsewhere" first) -- the column class, the name
    of the row's region_class (find_guides with classes), directly behind pam_sequence and ahead of activity_q16.  microhomology: the
    MicrohomologyModel the rows were scored with (find_guides) -- mh_total_q16 and mh_oof_q16, the two sums as they are, mh_score,
    100 * total / 65536 (%.3f), and out_of_frame, 100 * oof / total (%.2f), directly behind activity; NA in all four for a site
    without a score and in out_of_frame where the total is 0."""
    from .aligner import ACTIVITY_NONE, MH_NONE, activity_value
    header = list(GUIDE_COLUMNS)
    if class_names is not None:
        header.append("class")
    if activity is not None:
        header += ["activity_q16", "activity"]
    if microhomology is not None:
        header += ["mh_total_q16", "mh_oof_q16", "mh_score", "out_of_frame"]
    if copies is not None:
        header.append("copies")
    if seed_copies is not None:
        header.append("seed_copies")
    if near is not None:
        # (an array of shape (n, M + 1) names its columns without a row; a list of rows needs one)
        header += ["copies_mm%d" % d for d in range(near.shape[1] if hasattr(near, "shape") else len(near[0]) if len(near) else 0)]
    if near_scores is not None:
        header += ["near_sum_q32", "near_max_q32", "near_specificity"]
        near_spec = near_scores.specificity
    n_mm = 0
    if scores is not None:
        tables = {g: s.table for g, s in scores.items()}
    if tables is not None:
        n_mm = max([t.shape[1] for t in tables.values()], default=1)
        header += ["hits"] + ["hits_mm%d" % m for m in range(n_mm)]
    if scores is not None:
        header += ["perfect", "specificity"]
    lines = ["\t".join(header)]
    for i, r in enumerate(rows):
        f = [str(x) for x in r.row()]
        if class_names is not None:
            f.append(class_names[r.region_class])
        if activity is not None:
            unscored = r.activity_q16 is None or r.activity_q16 == ACTIVITY_NONE
            f += ["NA", "NA"] if unscored else [str(r.activity_q16), "%.6f" % activity_value(r.activity_q16, activity)]
        if microhomology is not None:
            total, oof = r.mh_total_q16, r.mh_oof_q16
            if total is None or total == MH_NONE:
                f += ["NA"] * 4
            else:
                f += [str(total), str(oof), "%.3f" % (100.0 * total / 65536.0), "%.2f" % (100.0 * oof / total) if total else "NA"]
        if copies is not None:
            f.append(str(int(copies[i])))
        if seed_copies is not None:
            f.append(str(int(seed_copies[i])))
        if near is not None:
            f += [str(int(x)) for x in near[i]]
        if near_scores is not None:
            f += [str(int(near_scores.sum_q32[i])), str(int(near_scores.max_q32[i])), "%.6f" % near_spec[i]]
        if tables is not None:
            t = tables[r.guide]
            f += [str(int(t.sum()))] + [str(int(t[:, m].sum())) if m < t.shape[1] else "0" for m in range(n_mm)]
        if scores is not None:
            f += [str(scores[r.guide].perfect), "%.6f" % scores[r.guide].specificity]
        lines.append("\t".join(f))
    return "\n".join(lines) + "\n"


def site_filter_of_flags(L, gc_min=None, gc_max=None, max_run=None, avoid=()):
    """The SiteFilter of FindGuides' flags for a protospacer of L bases, None when none is given.  gc_min / gc_max: integer percentages
    0 .. 100 (SiteFilter.percent); max_run: "N" for every base or "T=3,G=4" with unnamed bases unlimited; avoid: IUPAC motifs, each
    joined by its reverse complement when that differs -- more than 8 after that is an error."""
    if gc_min is None and gc_max is None and max_run is None and not avoid:
        return None
    lo, hi = 0 if gc_min is None else int(gc_min), 100 if gc_max is None else int(gc_max)
    if not (0 <= lo <= 100 and 0 <= hi <= 100):
        raise ValueError("--gc-min and --gc-max are percentages, 0 .. 100")
    g0, g1 = SiteFilter.percent(L, lo, hi)
    runs = [0, 0, 0, 0]
    if max_run is not None:
        for part in str(max_run).split(","):
            base, eq, n = part.strip().rpartition("=")
            if not n.isdigit() or int(n) > 255 or (eq and (len(base) != 1 or base.upper() not in "ACGT")):
                raise ValueError("--max-run takes N or BASE=N,... (A C G T; 0 .. 255), not %s" % max_run)
            if eq:
                runs["ACGT".index(base.upper())] = int(n)
            else:
                runs = [int(n)] * 4
    motifs = []
    for m in avoid:
        for x in (m.upper(), iupac_revcomp(m)):
            if x not in motifs:
                motifs.append(x)
    if len(motifs) > 8:
        raise ValueError("--avoid: more than 8 motifs once the reverse complements are added")
    return SiteFilter(g0, g1, runs, motifs)


ALLELE_COLUMNS = ["chromosome", "position", "id", "ref", "alt", "allele", "start", "end", "strand", "pam_index", "snv_offset", "guide", "pam_sequence",
                  "other_pam_index"]


def snvs_of_vcf(ctx, vcf, chrom=None, start=0, end=None):
    """The SNVs of a VCF for Context.find_allele_sites, read through the library's reader (Context.vcf_records): every ALT of a record
    whose REF and ALT are single letters of A C G T, on the chromosome `chrom` (None: any) at a 0-based position in [start, end).
    Returns (rows, skipped): rows a list of (chrom, pos1, id, ref, alt) and skipped a dict of counts -- "other" alleles, "lacks":
    records on chromosomes the reference lacks, "beyond": SNVs past their contig's end."""
    lengths = dict(zip(ctx.contig_names, ctx.contig_lengths))
    rows, skipped = [], {"other": 0, "lacks": 0, "beyond": 0}
    for c, pos, _, vid, ref, alts, _ in ctx.vcf_records(vcf):
        if c not in lengths:
            skipped["lacks"] += 1
            continue
        if (chrom is not None and c != chrom) or pos - 1 < start or (end and pos - 1 >= end):
            continue
        for alt in alts:
            if not (len(ref) == 1 and len(alt) == 1 and ref in "ACGT" and alt in "ACGT"):
                skipped["other"] += 1
            elif pos > lengths[c]:
                skipped["beyond"] += 1
            else:
                rows.append((c, pos, vid, ref, alt))
    return rows, skipped


def allele_sites_tsv(ctx, found, rows, kinds=("alt", "ref", "both")):
    """The --allele-sites table: ALLELE_COLUMNS, a line per record of `found` (an AlleleSites over snvs_of(rows)) whose kind is among
    `kinds`, in the call's order.  position is 1-based as in the VCF, [start, end) the footprint of the record's site, 0-based and
    half-open; guide is the `-i` string a search takes, cut from the allele named (alt for both); pam_sequence the PAM's bases of that
    allele on the site's strand; other_pam_index is . unless the line is both."""
    from .aligner import ALLELE_KINDS
    lines = ["\t".join(ALLELE_COLUMNS)]
    L = found.pattern.protospacer_length
    for r in found.sites:
        name = ALLELE_KINDS[int(r["kind"])]
        if name not in kinds:
            continue
        c, pos1, vid, ref, alt = rows[int(r["snv_index"])]
        ci, ps, pm, pl = int(r["contig_index"]), int(r["protospacer_start"]), int(r["pam_start"]), int(r["pam_length"])
        lo, hi = (ps, ps + L) if pm < 0 else (min(ps, pm), max(ps + L, pm + pl))
        pam_seq = ""
        if pm >= 0 and pl:
            pam_seq = ctx.fetch_bases(ci, pm, pl)
            if name != "ref" and pm <= pos1 - 1 < pm + pl:
                pam_seq = pam_seq[:pos1 - 1 - pm] + alt + pam_seq[pos1 - pm:]
            if r["strand"] == b"-":
                pam_seq = pam_seq.translate(_RC)[::-1]
            pam_seq = pam_seq.replace("U", "T")
        lines.append("\t".join([c, str(pos1), vid or ".", ref, alt, name, str(lo), str(hi), r["strand"].decode(), str(int(r["pam_index"])),
                                str(int(r["guide_offset"])), found.guide(r), pam_seq, str(int(r["other_pam_index"])) if name == "both" else "."]))
    return "\n".join(lines) + "\n"


def allele_sites_tool(ctx, pat, vcf, out_path, kinds=None, chrom=None, start=0, end=None, host=False):
    """FindGuides --alleles VCF --allele-sites OUT: the table of allele_sites_tsv to out_path, and the counts of what was examined and
    skipped as one line on stderr."""
    import sys
    from .aligner import snvs_of
    names = ("alt", "ref", "both")
    wanted = names if kinds is None else tuple(k for k in str(kinds).split(",") if k)
    if not wanted or any(k not in names for k in wanted):
        raise ValueError("--allele-kinds: names among alt, ref, both, separated by commas, not %s" % kinds)
    rows, skipped = snvs_of_vcf(ctx, vcf, chrom, start, end)
    found = ctx.find_allele_sites(pat, snvs_of([(c, pos1, ref, alt) for c, pos1, _, ref, alt in rows], ctx), host=host)
    by = [int((found.status == k).sum()) for k in range(4)]
    keep = [i for i in range(len(rows)) if found.status[i] == 0]
    if len(keep) < len(rows):                          # the table speaks of the examined SNVs alone
        new = {old: k for k, old in enumerate(keep)}
        found.sites["snv_index"] = [new[int(i)] for i in found.sites["snv_index"]]
        rows = [rows[i] for i in keep]
    with open(out_path, "w") as f:
        f.write(allele_sites_tsv(ctx, found, rows, wanted))
    sys.stderr.write("alleles: %d SNVs examined, %d records; skipped: %d other alleles, %d records on chromosomes the reference lacks, %d beyond a contig's end, "
                     "%d with another REF than the reference, %d on a base that is not A C G T, %d with ALT equal to the reference\n"
                     % (by[0], len(found.sites), skipped["other"], skipped["lacks"], skipped["beyond"], by[1], by[2], by[3]))


EDIT_COLUMNS = ["chromosome", "position", "id", "ref", "alt", "mode", "start", "end", "strand", "pam_index", "edit_offset", "guide", "pam_sequence",
                "bystanders", "bystander_offsets", "edited"]


def _ascii_digits(text):
    """1 .. 9 of the digits 0 .. 9: what the command line tool takes for a number."""
    return 1 <= len(text) <= 9 and all(c in "0123456789" for c in text)


def base_edit_of_flags(pat, editor, edit_window, edit_context=None, edit_mode=None, max_bystanders=None):
    """The BaseEdit of FindGuides' flags: --editor FROM:TO (two different letters of A C G T), --edit-window FROM:TO (positions of the
    protospacer as the guide reads, 0-based and half-open), --edit-context LETTER (IUPAC; default N), --edit-mode install|correct
    (default install), --max-bystanders N (0 .. 31; default no bound)."""
    from .aligner import _IUPAC_SETS, BaseEdit
    a, sep, b = str(editor).partition(":")
    if not (sep and len(a) == 1 and len(b) == 1 and a in "ACGT" and b in "ACGT" and a != b):
        raise ValueError("--editor FROM:TO: two different letters of A C G T (C:T a CBE, A:G an ABE), not %s" % editor)
    w0, sep, w1 = str(edit_window).partition(":")
    if not (sep and _ascii_digits(w0) and _ascii_digits(w1)):
        raise ValueError("--edit-window FROM:TO: two integers, 0-based and half-open in the protospacer, not %s" % edit_window)
    if not int(w0) < int(w1) <= pat.protospacer_length:
        raise ValueError("--edit-window FROM:TO: 0 <= FROM < TO <= %d, the protospacer's length" % pat.protospacer_length)
    context = "N" if edit_context is None else str(edit_context)
    if not (len(context) == 1 and context.upper() in _IUPAC_SETS):
        raise ValueError("--edit-context: one IUPAC letter, not %s" % edit_context)
    if edit_mode not in (None, "install", "correct"):
        raise ValueError("--edit-mode: install or correct, not %s" % edit_mode)
    if max_bystanders is not None and not (_ascii_digits(str(max_bystanders)) and int(max_bystanders) <= 31):
        raise ValueError("--max-bystanders N: an integer 0 .. 31, not %s" % max_bystanders)
    return BaseEdit(a, b, (int(w0), int(w1)), context.upper(), edit_mode == "correct", None if max_bystanders is None else int(max_bystanders))


def edit_sites_tsv(ctx, found, rows):
    """The --edit-sites table: EDIT_COLUMNS, a line per record of `found` (an EditSites over snvs_of(rows)), in the call's order.
    position is 1-based as in the VCF, [start, end) the footprint of the record's site, 0-based and half-open; edit_offset where the
    SNV is in the protospacer as the guide reads; guide is the `-i` string a search takes, cut from the background allele;
    pam_sequence the PAM's bases on the site's strand; bystanders their number and bystander_offsets their positions, comma-separated
    or . for none; edited the protospacer with every editable base replaced by the editor's product in lower case."""
    lines = ["\t".join(EDIT_COLUMNS)]
    L = found.pattern.protospacer_length
    mode, to = "correct" if found.edit.correct else "install", found.edit.to_base.lower().replace("u", "t")
    for r in found.sites:
        c, pos1, vid, ref, alt = rows[int(r["snv_index"])]
        ci, ps, pm, pl = int(r["contig_index"]), int(r["protospacer_start"]), int(r["pam_start"]), int(r["pam_length"])
        lo, hi = (ps, ps + L) if pm < 0 else (min(ps, pm), max(ps + L, pm + pl))
        pam_seq = ""
        if pm >= 0 and pl:
            pam_seq = ctx.fetch_bases(ci, pm, pl)
            if r["strand"] == b"-":
                pam_seq = pam_seq.translate(_RC)[::-1]
            pam_seq = pam_seq.replace("U", "T")
        by, bits = found.bystanders(r), int(r["editable"])
        edited = "".join(to if (bits >> i) & 1 else ch for i, ch in enumerate(found.protospacer(r)))
        lines.append("\t".join([c, str(pos1), vid or ".", ref, alt, mode, str(lo), str(hi), r["strand"].decode(), str(int(r["pam_index"])), str(found.offset(r)),
                                found.guide(r), pam_seq, str(len(by)), ",".join(map(str, by)) or ".", edited]))
    return "\n".join(lines) + "\n"


def edit_sites_tool(ctx, pat, vcf, out_path, edit, chrom=None, start=0, end=None, host=False):
    """FindGuides --alleles VCF --edit-sites OUT: the table of edit_sites_tsv to out_path, and the counts of what was examined and
    skipped as one line on stderr."""
    import sys
    from .aligner import snvs_of
    rows, skipped = snvs_of_vcf(ctx, vcf, chrom, start, end)
    found = ctx.find_edit_sites(pat, edit, snvs_of([(c, pos1, ref, alt) for c, pos1, _, ref, alt in rows], ctx), host=host)
    by = [int((found.status == k).sum()) for k in range(6)]
    with open(out_path, "w") as f:
        f.write(edit_sites_tsv(ctx, found, rows))
    sys.stderr.write("edits: %d SNVs examined, %d records; skipped: %d other alleles, %d records on chromosomes the reference lacks, %d beyond a contig's end, "
                     "%d with another REF than the reference, %d on a base that is not A C G T, %d with ALT equal to the reference, "
                     "%d that are not the editor's change, %d whose 5' neighbour fails the context\n"
                     % (by[0], len(found.sites), skipped["other"], skipped["lacks"], skipped["beyond"], by[1], by[2], by[3], by[4], by[5]))


def find_guides_tool(ref, pattern, auxiliary_pams=(), chrom=None, start=0, end=None, output=None, counts=False, device=0, scores=None,
                     gc_min=None, gc_max=None, max_run=None, avoid=(), copies=False, seed_copies=None, max_copies=None, max_seed_copies=None,
                     near_copies=None, max_near_copies=None, near_scores=None, near_list=None, near_list_limit=None, activity=None, min_activity=None,
                     regions=None, classes=None, class_extent=None, pairs=None, pair_distance=None, pair_cut=None, pair_orientation=None, alleles=None, allele_sites=None,
                     allele_kinds=None, microhomology=None, mh_cut=None, min_out_of_frame=None, edit_sites=None, editor=None, edit_window=None, edit_context=None, edit_mode=None,
                     max_bystanders=None, **search):
    """`python -m calitas_amd FindGuides`: the guides of a region as a TSV (guides_tsv); counts=True: every distinct guide also goes
    through the off-target search with the SearchReference flags in `search` (make_params names); scores=ScoreModel (or its file):
    through search_scores_batch instead, which adds perfect and specificity.  gc_min, gc_max, max_run, avoid: the site filter's flags
    (site_filter_of_flags) -- fewer rows, the same columns and guide_ids, and only the kept guides are searched.  device -1: the host
    twin of the enumeration (no GPU; not with counts or scores).  copies=True: the column copies (guide_copies over the whole
    reference); seed_copies=K: the column seed_copies, the same for the PAM-proximal K bases; max_copies=N (implies copies) and
    max_seed_copies=N (needs seed_copies) drop the rows with more than N before anything is searched, the kept rows keep their
    guide_ids.  near_copies=M (0 .. 3): the columns copies_mm0 .. copies_mmM (guide_near over the whole reference, the whole
    protospacer); max_near_copies=N (N >= 1, needs near_copies) drops the rows whose columns sum to more than N, likewise before
    anything is searched.  near_scores=ScoreModel (or its file; needs near_copies, the model's length is the protospacer's): the
    columns near_sum_q32, near_max_q32 and near_specificity, from the one guide_near_scores pass that then gives the copies_mm columns
    as well.  near_list=FILE (needs near_copies): the kept rows' copies within M substitutions, one per line, to FILE (near_list_tsv;
    scored under near_scores' model when given); near_list_limit=N (1 .. 4096, default 1000): a row with more copies writes no line.
    activity=ActivityModel (or its file; the model's length is the protospacer's): the columns activity_q16 and activity, every site
    scored in the listing's own call; min_activity=X (needs activity): a decimal on the LINEAR score (under link logistic a probability
    p is X = ln(p / (1 - p))) -- the rows that score less, and those without a score, are dropped before any of the flags above looks
    at anything, the kept rows keep their guide_ids.  regions=FILE.bed (the parser and rules of SearchReference --regions): the column
    class, and only the sites of the named classes; classes="name,..." (needs regions) the classes to keep instead, "elsewhere" among
    them if wanted; class_extent="FROM:TO" (needs regions) the positions of the protospacer as the guide reads, 0-based and half-open,
    that are classed instead of all of it.  The dropped rows are gone before any of the flags above looks at anything, the kept rows
    keep their guide_ids.  pairs=FILE: the pairs of the kept rows (guide_pairs, pairs_tsv) to FILE, the table itself unchanged;
    pair_distance="MIN:MAX" (required with pairs) the bounds on the distance of the two cuts; pair_cut=N the cut's position in the
    protospacer as the guide reads (default L - 3 with a 3' PAM, required otherwise); pair_orientation=out|in|same|any|CODE,...
    (default out).  alleles=FILE.vcf[.gz] with allele_sites=OUT.tsv (each needs the other): the sites every SNV of the file whose
    position lies in the region creates, destroys or changes (Context.find_allele_sites, allele_sites_tsv) to OUT, the table itself
    unchanged; allele_kinds="alt,ref,both" the kinds to write (default all).  microhomology=MicrohomologyModel (or its file): the
    columns mh_total_q16, mh_oof_q16, mh_score and out_of_frame, every site's window around its cut scored in a listing of its own
    (joined to the others as find_guides does); mh_cut=N the cut's position in the protospacer as the guide reads (default L - 3 with a
    3' PAM, required otherwise); min_out_of_frame=PCT (0 .. 100, needs microhomology): the rows whose out-of-frame share is below PCT
    per cent, those with a total of 0 and those without a score are dropped before any of the flags above looks at anything, the kept
    rows keep their guide_ids.  edit_sites=OUT.tsv (needs alleles, editor="FROM:TO" and edit_window="FROM:TO"; alleles now needs
    allele_sites or edit_sites, and may have both): the guides that put every SNV of the file whose position lies in the region into
    the base editor's window, and their bystanders (Context.find_edit_sites, edit_sites_tsv) to OUT, the table itself unchanged;
    edit_context=LETTER, edit_mode="install"|"correct" and max_bystanders=N as base_edit_of_flags reads them.  These thirty work with
    device -1 through the host twin.  Returns the text."""
    if edit_sites is not None and (alleles is None or editor is None or edit_window is None):
        raise ValueError("--edit-sites OUT.tsv requires --alleles FILE.vcf, --editor FROM:TO and --edit-window FROM:TO")
    if edit_sites is None and any(x is not None for x in (editor, edit_window, edit_context, edit_mode, max_bystanders)):
        raise ValueError("--editor, --edit-window, --edit-context, --edit-mode and --max-bystanders require --edit-sites OUT.tsv")
    if alleles is None and allele_sites is not None:
        raise ValueError("--alleles FILE.vcf and --allele-sites OUT.tsv require each other")
    if alleles is not None and allele_sites is None and edit_sites is None:
        raise ValueError("--alleles FILE.vcf requires --allele-sites OUT.tsv or --edit-sites OUT.tsv")
    if allele_kinds is not None and allele_sites is None:
        raise ValueError("--allele-kinds requires --alleles FILE.vcf and --allele-sites OUT.tsv")
    if regions is None and (classes is not None or class_extent is not None):
        raise ValueError("--classes and --class-extent require --regions FILE.bed")
    extent = None
    if class_extent is not None:
        a, sep, b = str(class_extent).partition(":")
        if not (sep and a.isdigit() and b.isdigit()):
            raise ValueError("--class-extent FROM:TO: two integers, 0-based and half-open in the protospacer, not %s" % class_extent)
        extent = (int(a), int(b))
    if (counts or scores is not None) and device < 0:
        raise ValueError("--counts and --scores search on the GPU: they cannot run with --device -1")
    if isinstance(scores, str):
        from .aligner import ScoreModel
        scores = ScoreModel.read(scores)
    pat = Guide(pattern, auxiliary_pams)
    keep = site_filter_of_flags(pat.protospacer_length, gc_min, gc_max, max_run, avoid)
    pair_spec = site_pairs_of_flags(pat, pairs, pair_distance, pair_cut, pair_orientation)
    edit = base_edit_of_flags(pat, editor, edit_window, edit_context, edit_mode, max_bystanders) if edit_sites is not None else None
    if seed_copies is not None and not 1 <= int(seed_copies) <= pat.protospacer_length:
        raise ValueError("--seed-copies K: K is 1 .. %d, the protospacer's length" % pat.protospacer_length)
    if max_copies is not None and int(max_copies) < 1:
        raise ValueError("--max-copies N: N is at least 1 (a guide counts itself)")
    if max_seed_copies is not None and seed_copies is None:
        raise ValueError("--max-seed-copies requires --seed-copies K")
    if max_seed_copies is not None and int(max_seed_copies) < 1:
        raise ValueError("--max-seed-copies N: N is at least 1 (a guide counts itself)")
    if near_copies is not None and not 0 <= int(near_copies) <= 3:
        raise ValueError("--near-copies M: M is 0 .. 3")
    if near_copies is not None and pat.protospacer_length < int(near_copies) + 1:
        raise ValueError("--near-copies M: the protospacer has fewer than M + 1 bases")
    if max_near_copies is not None and near_copies is None:
        raise ValueError("--max-near-copies requires --near-copies M")
    if max_near_copies is not None and int(max_near_copies) < 1:
        raise ValueError("--max-near-copies N: N is at least 1 (a guide counts itself)")
    if near_scores is not None and near_copies is None:
        raise ValueError("--near-scores requires --near-copies M")
    if isinstance(near_scores, str):
        from .aligner import ScoreModel
        near_scores = ScoreModel.read(near_scores)
    if near_scores is not None and near_scores.L != pat.protospacer_length:
        raise ValueError("--near-scores: the model is for protospacers of %d bases, the pattern's has %d" % (near_scores.L, pat.protospacer_length))
    if near_list is not None and near_copies is None:
        raise ValueError("--near-list requires --near-copies M")
    if near_list_limit is not None and near_list is None:
        raise ValueError("--near-list-limit requires --near-list FILE")
    if near_list_limit is not None and not 1 <= int(near_list_limit) <= 4096:
        raise ValueError("--near-list-limit N: N is 1 .. 4096")
    if min_activity is not None and activity is None:
        raise ValueError("--min-activity requires --activity MODEL")
    if isinstance(activity, str):
        from .aligner import ActivityModel
        activity = ActivityModel.read(activity)
    if activity is not None and activity.L != pat.protospacer_length:
        raise ValueError("--activity: the model is for protospacers of %d bases, the pattern's has %d" % (activity.L, pat.protospacer_length))
    floor = activity_q16_of_flag(min_activity) if min_activity is not None else None
    if microhomology is None and (mh_cut is not None or min_out_of_frame is not None):
        raise ValueError("--mh-cut and --min-out-of-frame require --microhomology MODEL")
    if isinstance(microhomology, str):
        from .aligner import MicrohomologyModel
        microhomology = MicrohomologyModel.read(microhomology)
    permille = 0
    if microhomology is not None:
        L = pat.protospacer_length
        if mh_cut is None and not pat.pam_is_three_prime:
            raise ValueError("--mh-cut N is required: the default, L - 3, is the Cas9 cut of a pattern with a 3' PAM")
        if mh_cut is not None and not (str(mh_cut).isdigit() and len(str(mh_cut)) <= 3 and int(mh_cut) <= L):
            raise ValueError("--mh-cut N: N is 0 .. %d, the protospacer's length, not %s" % (L, mh_cut))
        mh_cut = L - 3 if mh_cut is None else int(mh_cut)
        if min_out_of_frame is not None:
            if not (str(min_out_of_frame).isdigit() and len(str(min_out_of_frame)) <= 3 and int(min_out_of_frame) <= 100):
                raise ValueError("--min-out-of-frame PCT: PCT is an integer 0 .. 100, not %s" % min_out_of_frame)
            permille = 10 * int(min_out_of_frame)
    ctx = Context(device)
    try:
        ctx.set_reference_fasta(ref)
        class_names = None
        if regions is not None:
            from .aligner import Regions
            if extent is not None and not 0 <= extent[0] < extent[1] <= pat.protospacer_length:
                raise ValueError("--class-extent FROM:TO: 0 <= FROM < TO <= %d, the protospacer's length" % pat.protospacer_length)
            reg = Regions.read_bed(regions, dict(zip(ctx.contig_names, ctx.contig_lengths)))
            if classes is not None:
                reg.mask_of(classes)                   # (an unknown name is refused here, by name)
            if not reg.intervals:
                raise ValueError("--regions: no interval lies on a chromosome of the reference")
            ctx.set_regions(reg)
            class_names = reg.classes
        rows = find_guides(ctx, pat, chrom, start, end, host=device < 0, filter=keep, activity=activity, min_activity=floor, classes=classes, extent=extent,
                           by_regions=regions is not None, microhomology=microhomology, mh_cut=mh_cut, min_out_of_frame=permille)
        n_copies = guide_copies(ctx, pat, rows, host=device < 0) if copies or max_copies is not None else None
        n_seed = guide_copies(ctx, pat, rows, key_length=int(seed_copies), host=device < 0) if seed_copies is not None else None
        scored_near = guide_near_scores(ctx, pat, rows, int(near_copies), near_scores, host=device < 0) if near_scores is not None else None
        if scored_near is not None:
            n_near = [[int(x) for x in row] for row in scored_near.near]
        else:
            n_near = guide_near(ctx, pat, rows, int(near_copies), host=device < 0) if near_copies is not None else None
        kept = [i for i in range(len(rows)) if (max_copies is None or n_copies[i] <= int(max_copies)) and
                (max_seed_copies is None or n_seed[i] <= int(max_seed_copies)) and
                (max_near_copies is None or sum(n_near[i]) <= int(max_near_copies))]
        rows = [rows[i] for i in kept]
        n_copies = None if n_copies is None else [n_copies[i] for i in kept]
        n_seed = None if n_seed is None else [n_seed[i] for i in kept]
        if n_near is not None:
            import numpy as np
            n_near = np.array([n_near[i] for i in kept], dtype=np.uint64).reshape(len(kept), int(near_copies) + 1)
        if scored_near is not None:
            from .aligner import NearScores
            scored_near = NearScores(n_near, scored_near.sum_q32[kept], scored_near.max_q32[kept])
        tables = guide_counts(ctx, [r.guide for r in rows], make_params(**search)) if counts and scores is None else None
        scored = guide_scores(ctx, [r.guide for r in rows], make_params(**search), scores) if scores is not None else None
        text = guides_tsv(rows, tables, scored, copies=n_copies, seed_copies=n_seed, near=n_near, near_scores=scored_near, activity=activity, class_names=class_names,
                          microhomology=microhomology)
        if near_list is not None:
            listing = guide_near_list(ctx, pat, rows, int(near_copies), near_scores, limit=1000 if near_list_limit is None else int(near_list_limit), host=device < 0)
            with open(near_list, "w") as f:
                f.write(near_list_tsv(rows, ctx.contig_names, listing))
        if pair_spec is not None:
            paired = guide_pairs(ctx, pat, rows, pair_spec, chrom, start, end, host=device < 0, filter=keep)
            with open(pairs, "w") as f:
                f.write(pairs_tsv(rows, [pair_spec.name_of(o, pat) for o in range(4)], paired))
        if allele_sites is not None:
            allele_sites_tool(ctx, pat, alleles, allele_sites, allele_kinds, chrom, start, end, host=device < 0)
        if edit_sites is not None:
            edit_sites_tool(ctx, pat, alleles, edit_sites, edit, chrom, start, end, host=device < 0)
        if output is not None:
            with open(output, "w") as f:
                f.write(text)
        return text
    finally:
        ctx.close()
