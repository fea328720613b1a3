"""Host-side mirror of the reference's operator interface for the SearchReference path, on top of the C ABI.

Names, argument meaning and error behaviour follow
  calitas/src/main/scala/com/editasmedicine/aligner/SequentialGuideAligner.scala (Guide, Defaults)
  calitas/src/main/scala/com/editasmedicine/aligner/SearchReference.scala (SearchReference flags, execute)
so the parity tests read like the reference's own tests.  All alignment work happens in libcalitas_hip.so.
"""
import collections
import contextlib
import ctypes
import time

from . import _lib
from ._lib import AlnT, CalitasError, CountsT, GuideT, ParamsT, RegionsT, RegionT, ScoreModelT, ScoresT, SiteFilterT, SiteT, TimingT, TopT, lib


class Defaults:  # SequentialGuideAligner.scala:17-28
    MismatchNetCost = -120
    GuideGapNetCost = -121
    GenomeGapNetCost = -122
    PamMismatchNetCost = -260
    MaxGuideDiffs = 5
    MaxPamMismatches = 1
    MaxGapsBetweenGuideAndPam = 3
    MaxOverlap = 10
    MaxVariantsInCluster = 16


def _split_by_case(s):  # SequentialGuideAligner.scala:110-121
    parts, i = [], 0
    while i < len(s):
        first = s[i].islower()
        j = i
        while j < len(s) and s[j].islower() == first:
            j += 1
        parts.append(s[i:j])
        i = j
    return parts


class Guide:
    """SequentialGuideAligner.Guide (SequentialGuideAligner.scala:32-107): protospacer in upper case, optional PAM in
    lower case at either end, optional auxiliary PAMs."""

    def __init__(self, sequence, aux_pams=()):
        aux_pams = list(aux_pams)
        self.sequence = sequence
        parts = _split_by_case(sequence.strip())
        if not (1 <= len(parts) <= 2):
            raise ValueError("Invalid Guide sequence %s." % sequence)
        if not (len(parts) == 2 or parts[0][0].isupper()):
            raise ValueError("Guide sequence cannot be all lower case.")
        if aux_pams and len(parts) != 2:
            raise ValueError("Cannot provide auxiliary PAMs without providing a PAM in the guide sequence.")
        if any(p != p.lower() for p in aux_pams):
            raise ValueError("All PAMs must be lower case. PAMs given: %s" % ", ".join(aux_pams))
        if len(parts) == 1:
            guide, pam, five = parts[0], None, False
        elif parts[0][0].isupper():
            guide, pam, five = parts[0], parts[1], False
        else:
            guide, pam, five = parts[1], parts[0], True
        self.guide = guide.upper()
        self.pams = ([pam] if pam is not None else []) + aux_pams
        self.pams = [p.lower() for p in self.pams]
        self.pam_is_five_prime = five
        self.pam_is_three_prime = pam is not None and not five
        self.protospacer_length = len(self.guide)
        self.pam_length = max([len(p) for p in self.pams], default=0)
        self.length = self.protospacer_length + self.pam_length
        self.cli_length = len(sequence)  # SearchReference.scala:528 uses the raw `-i` string

    def to_c(self):
        g = GuideT()
        g.protospacer = self.guide.encode()
        g.n_pams = len(self.pams)
        self._pam_arr = (ctypes.c_char_p * max(1, len(self.pams)))(*[p.encode() for p in self.pams])
        g.pams = self._pam_arr
        g.pam_is_5prime = 1 if self.pam_is_five_prime else 0
        g.cli_length = self.cli_length
        return g


def make_params(window_size=1000, max_guide_diffs=Defaults.MaxGuideDiffs, max_pam_mismatches=Defaults.MaxPamMismatches,
                max_gaps_between_guide_and_pam=Defaults.MaxGapsBetweenGuideAndPam, max_total_diffs=None,
                max_overlap=Defaults.MaxOverlap, guide_mismatch_net_cost=Defaults.MismatchNetCost,
                pam_mismatch_net_cost=Defaults.PamMismatchNetCost, genome_gap_net_cost=Defaults.GenomeGapNetCost,
                guide_gap_net_cost=Defaults.GuideGapNetCost, chrom_index=-1, eqx_by_score=0, per_matrix=0,
                max_variants=Defaults.MaxVariantsInCluster, first_window=0, n_windows=0):
    p = ParamsT()
    p.window_size = window_size
    p.max_guide_diffs = max_guide_diffs
    p.max_pam_mismatches = max_pam_mismatches
    p.max_gaps_between_guide_and_pam = max_gaps_between_guide_and_pam
    p.max_total_diffs = -1 if max_total_diffs is None else max_total_diffs
    p.max_overlap = max_overlap
    p.guide_mismatch_net_cost = guide_mismatch_net_cost
    p.pam_mismatch_net_cost = pam_mismatch_net_cost
    p.genome_gap_net_cost = genome_gap_net_cost
    p.guide_gap_net_cost = guide_gap_net_cost
    p.chrom_index = chrom_index
    p.eqx_by_score = (eqx_by_score & 3) | (2 if per_matrix else 0)   # bit flags, see calitas_hip.h
    p.max_variants = max_variants
    p.first_window, p.n_windows = first_window, n_windows   # calitas_search only: a window range of the job (shard.window_partition)
    return p


class Alignment:
    """One GuideAlignment (GuideAlignment.scala:72-88) as returned through the C ABI."""
    __slots__ = ("guide_index", "contig_index", "window_start", "start_offset", "end_offset", "guide_start_offset",
                 "guide_end_offset", "score", "strand", "pam_index", "ops")

    def __init__(self, a):
        self.guide_index = a.guide_index
        self.contig_index = a.contig_index
        self.window_start = a.window_start
        self.start_offset = a.start_offset
        self.end_offset = a.end_offset
        self.guide_start_offset = a.guide_start_offset
        self.guide_end_offset = a.guide_end_offset
        self.score = a.score
        self.strand = chr(a.strand)
        self.pam_index = a.pam_index
        self.ops = bytes(a.ops[:a.n_ops]).decode()

    @property
    def cigar(self):
        out, i = [], 0
        while i < len(self.ops):
            j = i
            while j < len(self.ops) and self.ops[j] == self.ops[i]:
                j += 1
            out.append("%d%s" % (j - i, self.ops[i]))
            i = j
        return "".join(out)

    def to_c(self):
        a = AlnT()
        for f in ("guide_index", "contig_index", "window_start", "start_offset", "end_offset", "guide_start_offset",
                  "guide_end_offset", "score", "pam_index"):
            setattr(a, f, getattr(self, f))
        a.strand = ord(self.strand)
        a.n_ops = len(self.ops)
        for i, c in enumerate(self.ops.encode()):
            a.ops[i] = c
        return a


_KeyCall = collections.namedtuple("_KeyCall", ("pattern", "K", "M", "text", "n", "row", "index", "start", "end"))


class Context:
    """One GPU (device >= 0) or a host-only context (device = -1) holding a packed reference."""

    def __init__(self, device=0):
        h = ctypes.c_void_p()
        rc = lib.calitas_create(device, ctypes.byref(h))
        if rc != _lib.OK:
            msg = lib.calitas_last_error(None)
            raise CalitasError(rc, msg.decode() if msg else "?")
        self._h = h
        self.device = device
        self.contig_names = []
        self.contig_lengths = []
        self.regions = None                  # the Regions of the last set_regions (their class names label what the calls return)

    def close(self):
        if self._h:
            lib.calitas_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _load_contig_table(self):
        n = ctypes.c_int32()
        _lib.check(self._h, lib.calitas_reference_info(self._h, ctypes.byref(n), None, None))
        self.contig_names, self.contig_lengths = [], []
        self.regions = None                  # (a new reference drops the set)
        for i in range(n.value):
            nm, ln = ctypes.c_char_p(), ctypes.c_uint64()
            _lib.check(self._h, lib.calitas_contig_name(self._h, i, ctypes.byref(nm), ctypes.byref(ln)))
            self.contig_names.append(nm.value.decode())
            self.contig_lengths.append(ln.value)

    def set_reference(self, names, seqs, genome_build="unknown", lengths=None):
        """seqs: bytes-like objects or numpy uint8 arrays holding ASCII bases; borrowed only for the call.  seqs[i] None with
        lengths[i] given: contig i is absent (its name and length count, its bases are not held: a process of a multi-GPU job
        and the contigs its window range does not touch)."""
        n = len(names)
        c_names = (ctypes.c_char_p * n)(*[s.encode() for s in names])
        c_lens = (ctypes.c_uint64 * n)(*[(int(lengths[i]) if s is None else len(s)) for i, s in enumerate(seqs)])
        ptrs, keep = [], []
        for s in seqs:
            if s is None:
                ptrs.append(ctypes.c_void_p(None))
            elif hasattr(s, "ctypes"):  # numpy array
                keep.append(s)
                ptrs.append(ctypes.c_void_p(s.ctypes.data))
            else:
                b = bytes(s) if not isinstance(s, bytes) else s
                keep.append(b)
                ptrs.append(ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p))
        c_ptrs = (ctypes.c_void_p * n)(*ptrs)
        _lib.check(self._h, lib.calitas_set_reference(self._h, n, c_names, c_lens, c_ptrs, genome_build.encode()))
        self._load_contig_table()

    def set_reference_fasta(self, path):
        _lib.check(self._h, lib.calitas_set_reference_fasta(self._h, str(path).encode()))
        self._load_contig_table()

    def save_index(self, path):
        _lib.check(self._h, lib.calitas_save_index(self._h, str(path).encode()))

    def load_index(self, path):
        _lib.check(self._h, lib.calitas_load_index(self._h, str(path).encode()))
        self._load_contig_table()

    def genome_build(self):
        return lib.calitas_genome_build(self._h).decode()

    def reference_info(self):
        n, tb, pb = ctypes.c_int32(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._h, lib.calitas_reference_info(self._h, ctypes.byref(n), ctypes.byref(tb), ctypes.byref(pb)))
        return {"n_contigs": n.value, "total_bases": tb.value, "packed_bytes": pb.value}

    def fetch_bases(self, contig_index, start, length):
        buf = ctypes.create_string_buffer(length + 1)
        _lib.check(self._h, lib.calitas_fetch_bases(self._h, contig_index, start, length, buf))
        return buf.raw[:length].decode()

    def window_table(self, window_size, step, min_length, chrom_index=-1):
        out, n = ctypes.POINTER(ctypes.c_int32)(), ctypes.c_uint64()
        _lib.check(self._h, lib.calitas_window_table(self._h, window_size, step, min_length, chrom_index, ctypes.byref(out), ctypes.byref(n)))
        rows = [(out[3 * i], out[3 * i + 1], out[3 * i + 2]) for i in range(n.value)]
        lib.calitas_free(out)
        return rows

    def search_raw(self, guides, params):
        """calitas_search; returns (ctypes array pointer, count) -- caller must free with lib.calitas_free."""
        n = len(guides)
        self._keep = [g.to_c() for g in guides]
        arr = (GuideT * n)(*self._keep)
        out, cnt = ctypes.POINTER(AlnT)(), ctypes.c_uint64()
        _lib.check(self._h, lib.calitas_search(self._h, n, arr, ctypes.byref(params), ctypes.byref(out), ctypes.byref(cnt)))
        return out, cnt.value

    def tile_census(self):
        """calitas_reference_tiles: {"tiles", "dead", "masked", "tile_bases"} of the resident reference."""
        v = [ctypes.c_uint64() for _ in range(4)]
        _lib.check(self._h, lib.calitas_reference_tiles(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("tiles", "dead", "masked", "tile_bases"), [x.value for x in v]))

    def search_variants_raw(self, guide, guide_id, params, vcf_path, version=None, time_stamp=None, chrom=None):
        """calitas_search_variants without bringing the text into Python: (n_bytes, n_rows, n_variant_windows)."""
        g = guide.to_c()
        tsv, nbytes, rows, nwin = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._h, lib.calitas_search_variants(self._h, ctypes.byref(g), guide_id.encode(), ctypes.byref(params), str(vcf_path).encode(),
                                                        chrom.encode() if chrom is not None else None, None,
                                                        version.encode() if version else None, time_stamp.encode() if time_stamp else None,
                                                        ctypes.byref(tsv), ctypes.byref(nbytes), ctypes.byref(rows), ctypes.byref(nwin)))
        t_free = time.perf_counter()
        lib.calitas_free(tsv)
        self.last_free_ms = (time.perf_counter() - t_free) * 1e3    # (a hits.txt of tens of gigabytes: handing the block back is not free)
        return nbytes.value, rows.value, nwin.value

    def vcf_identifier(self, vcf_path):
        """calitas_vcf_identifier: "name:md5" of a VCF (ReferenceHit.scala:175-183), computed by the library."""
        out = ctypes.c_void_p()
        _lib.check(self._h, lib.calitas_vcf_identifier(self._h, str(vcf_path).encode(), ctypes.byref(out)))
        try:
            return ctypes.string_at(out).decode()
        finally:
            lib.calitas_free(out)

    def vcf_records(self, vcf_path, chrom=None):
        """calitas_vcf_records: the records of a VCF as the variant search reads them, a list of
        (chrom, pos, end, id, ref, [alts], [afs as the floats the search keeps])."""
        out, n = ctypes.c_void_p(), ctypes.c_uint64()
        _lib.check(self._h, lib.calitas_vcf_records(self._h, str(vcf_path).encode(), chrom.encode() if chrom is not None else None, ctypes.byref(out), ctypes.byref(n)))
        try:
            text = ctypes.string_at(out).decode()
        finally:
            lib.calitas_free(out)
        recs = []
        for line in text.split("\n")[:-1]:
            c, pos, end, vid, ref, alts, afs = line.split("\t")
            recs.append((c, int(pos), int(end), vid, ref, alts.split(","), [float(x) for x in afs.split(",")] if afs else []))
        assert len(recs) == n.value
        return recs

    def search_variants_into(self, guide, guide_id, params, vcf_path, address, capacity, version=None, time_stamp=None, chrom=None):
        """calitas_search_variants_into: the text goes to `capacity` bytes at `address` (memory of the caller, page-locked with pin_host: every
        contig's rows then cross the bus straight to their place).  Returns (n_bytes, n_rows, n_variant_windows)."""
        g = guide.to_c()
        nbytes, rows, nwin = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._h, lib.calitas_search_variants_into(self._h, ctypes.byref(g), guide_id.encode(), ctypes.byref(params), str(vcf_path).encode(),
                                                             chrom.encode() if chrom is not None else None, None,
                                                             version.encode() if version else None, time_stamp.encode() if time_stamp else None,
                                                             ctypes.c_void_p(address), capacity, ctypes.byref(nbytes), ctypes.byref(rows), ctypes.byref(nwin)))
        return nbytes.value, rows.value, nwin.value

    def scan_candidates(self, guides, params, columnwise=False):
        """calitas_scan_candidates: the candidate filter alone (columnwise: the same set from round 1's kernel, a test hook).  Returns a sorted list of (contig_index, contig_offset, pass, guide):
        one entry per end column whose seamless glocal bottom-row score reaches minGuideScore (pass 0 = target as is, the column
        is the alignment's last base; pass 1 = reverse-complemented target, the column is its first base in contig coordinates).
        Columns in the padding behind a contig are dropped."""
        import bisect
        n = len(guides)
        keep = [g.to_c() for g in guides]
        arr = (GuideT * n)(*keep)
        out, cnt = ctypes.POINTER(ctypes.c_uint32)(), ctypes.c_uint64()
        fn = lib.calitas_scan_candidates_columnwise if columnwise else lib.calitas_scan_candidates
        _lib.check(self._h, fn(self._h, n, arr, ctypes.byref(params), ctypes.byref(out), ctypes.byref(cnt)))
        try:
            words = out[:2 * cnt.value]
        finally:
            lib.calitas_free(out)
        nc = self.reference_info()["n_contigs"]
        bases, lens = [], []
        for i in range(nc):
            g, nm, ln = ctypes.c_uint64(), ctypes.c_char_p(), ctypes.c_uint64()
            _lib.check(self._h, lib.calitas_contig_packed_base(self._h, i, ctypes.byref(g)))
            _lib.check(self._h, lib.calitas_contig_name(self._h, i, ctypes.byref(nm), ctypes.byref(ln)))
            bases.append(g.value); lens.append(ln.value)
        res = []
        for k in range(cnt.value):
            gword, info = words[2 * k], words[2 * k + 1]
            c = bisect.bisect_right(bases, gword * 16) - 1
            for b in range(16):
                if (info >> b) & 1:
                    off = gword * 16 + b - bases[c]
                    if 0 <= off < lens[c]:
                        res.append((c, off, (info >> 16) & 1, (info >> 17) & 0x7F))
        res.sort()
        return res

    def search(self, guides, params):
        """Per-window accepted alignments of every guide, in the reference's order (list of Alignment)."""
        out, n = self.search_raw(guides, params)
        try:
            return [Alignment(out[i]) for i in range(n)]
        finally:
            lib.calitas_free(out)

    def search_hits(self, guide, guide_id, params, version=None, time_stamp=None, decode=True):
        """calitas_search_hits: one guide against the resident reference, finished hits.txt text back (tsv_text, n_rows);
        decode=False skips the copy into a Python str and returns (n_bytes, n_rows); decode="bytes" returns the raw bytes."""
        g = guide.to_c()
        tsv, nbytes, rows = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._h, lib.calitas_search_hits(self._h, ctypes.byref(g), guide_id.encode(), ctypes.byref(params),
                                                    version.encode() if version else None, time_stamp.encode() if time_stamp else None,
                                                    ctypes.byref(tsv), ctypes.byref(nbytes), ctypes.byref(rows)))
        if decode == "bytes":
            text = ctypes.string_at(tsv, nbytes.value)
        else:
            text = ctypes.string_at(tsv, nbytes.value).decode() if decode else nbytes.value
        lib.calitas_free(tsv)
        return text, rows.value

    def search_hits_into(self, guide, guide_id, params, address, capacity, version=None, time_stamp=None):
        """calitas_search_hits_into: the text goes to `capacity` bytes at `address` (memory of the caller, ideally pinned with
        pin_host).  Returns (n_bytes, n_rows)."""
        g = guide.to_c()
        nbytes, rows = ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._h, lib.calitas_search_hits_into(self._h, ctypes.byref(g), guide_id.encode(), ctypes.byref(params),
                                                         version.encode() if version else None, time_stamp.encode() if time_stamp else None,
                                                         ctypes.c_void_p(address), capacity, ctypes.byref(nbytes), ctypes.byref(rows)))
        return nbytes.value, rows.value

    @staticmethod
    def alloc_host(nbytes):
        """calitas_alloc_host: the address of a page-locked block of the runtime's own (free it with free_host) -- the destination the
        *_into calls like best."""
        p = lib.calitas_alloc_host(nbytes)
        if not p:
            raise MemoryError("calitas_alloc_host(%d)" % nbytes)
        return p

    @staticmethod
    def free_host(address):
        lib.calitas_free(ctypes.c_void_p(address))

    def pin_host(self, address, nbytes):
        _lib.check(self._h, lib.calitas_pin_host(self._h, ctypes.c_void_p(address), nbytes))

    def unpin_host(self, address):
        _lib.check(self._h, lib.calitas_unpin_host(self._h, ctypes.c_void_p(address)))

    def search_hits_stream(self, guide, guide_id, params, write, version=None, time_stamp=None):
        """calitas_search_hits_stream: `write(memoryview)` receives consecutive pieces of hits.txt (one piece when the search fits
        one call; header, then per-contig pieces when it does not fit the device).  A piece is the library's own buffer, valid only
        during the call -- file.write() takes it as it is, bytes(piece) keeps a copy.  Returns (n_bytes, n_rows)."""
        g = guide.to_c()
        nbytes, rows = ctypes.c_uint64(), ctypes.c_uint64()
        failure = []

        def sink(piece, n, _user):
            try:
                write(memoryview((ctypes.c_char * n).from_address(piece)).cast("B"))
                return 0
            except Exception as e:          # an exception must not cross the C frames
                failure.append(e)
                return 1
        cb = _lib.TextSink(sink)
        rc = lib.calitas_search_hits_stream(self._h, ctypes.byref(g), guide_id.encode(), ctypes.byref(params),
                                            version.encode() if version else None, time_stamp.encode() if time_stamp else None,
                                            cb, None, ctypes.byref(nbytes), ctypes.byref(rows))
        if failure:
            raise failure[0]
        _lib.check(self._h, rc)
        return nbytes.value, rows.value

    @contextlib.contextmanager
    def search_hits_view(self, guide, guide_id, params, version=None, time_stamp=None):
        """calitas_search_hits without a copy: yields (memoryview over the library's text buffer, n_rows); the buffer is
        released when the block ends."""
        g = guide.to_c()
        tsv, nbytes, rows = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._h, lib.calitas_search_hits(self._h, ctypes.byref(g), guide_id.encode(), ctypes.byref(params),
                                                    version.encode() if version else None, time_stamp.encode() if time_stamp else None,
                                                    ctypes.byref(tsv), ctypes.byref(nbytes), ctypes.byref(rows)))
        try:
            yield memoryview((ctypes.c_char * nbytes.value).from_address(tsv.value)).cast("B"), rows.value
        finally:
            lib.calitas_free(tsv)

    def search_hits_batch(self, guides, guide_ids, params, version=None, time_stamp=None, decode=True):
        """calitas_search_hits_batch: a list of (tsv_text or n_bytes, n_rows), one per guide, pipelined on the device."""
        n = len(guides)
        keep = [g.to_c() for g in guides]
        garr = (GuideT * n)(*keep)
        ids = (ctypes.c_char_p * n)(*[i.encode() for i in guide_ids])
        tsv = (ctypes.c_void_p * n)()
        nbytes, rows = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)()
        _lib.check(self._h, lib.calitas_search_hits_batch(self._h, n, garr, ids, ctypes.byref(params),
                                                          version.encode() if version else None, time_stamp.encode() if time_stamp else None,
                                                          tsv, nbytes, rows))
        out = []
        for i in range(n):
            if decode == "digest":      # a checksum of the text instead of the text (a full-size batch is many gigabytes)
                import zlib
                what = (zlib.crc32((ctypes.c_char * nbytes[i]).from_address(tsv[i])), nbytes[i])
            else:
                what = ctypes.string_at(tsv[i], nbytes[i]).decode() if decode else nbytes[i]
            out.append((what, rows[i]))
            lib.calitas_free(tsv[i])
        return out

    @staticmethod
    def _take_counts(ptr):
        """A calitas_counts_t block as a numpy uint64 array of shape (2, n_mm, n_gaps, n_pam); the block is freed."""
        import numpy as np
        try:
            c = ptr.contents
            shape = (2, c.n_mm, c.n_gaps, c.n_pam)
            n = 2 * c.n_mm * c.n_gaps * c.n_pam
            table = np.ctypeslib.as_array(c.counts, shape=(n,)).astype(np.uint64).reshape(shape)   # (astype copies)
            if int(table.sum()) != c.rows:
                raise CalitasError(_lib.EHIP, "the counts table does not add up to its rows")
            return table
        finally:
            lib.calitas_free(ptr)

    def search_counts(self, guide, params):
        """calitas_search_counts: the off-target table of one guide -- how many rows the hits.txt of search_hits (same guide, same
        params, window range included) has per (strand, guide_mm, guide_gaps, pam_mm) -- as a numpy uint64 array of shape
        (2, n_mm, n_gaps, n_pam), strand '+' first.  No text is built or copied.  The shape depends on guide and params only."""
        g = guide.to_c()
        out = ctypes.POINTER(CountsT)()
        _lib.check(self._h, lib.calitas_search_counts(self._h, ctypes.byref(g), ctypes.byref(params), ctypes.byref(out)))
        return self._take_counts(out)

    def search_counts_batch(self, guides, params):
        """calitas_search_counts_batch: a list of tables, one per guide (all of one length), pipelined on the device like
        search_hits_batch."""
        n = len(guides)
        keep = [g.to_c() for g in guides]
        garr = (GuideT * n)(*keep)
        out = (ctypes.POINTER(CountsT) * n)()
        _lib.check(self._h, lib.calitas_search_counts_batch(self._h, n, garr, ctypes.byref(params), out))
        return [self._take_counts(out[i]) for i in range(n)]

    def hits_counts(self, guide, params, alignments):
        """calitas_hits_counts: removeOverlaps on a guide's alignments (as search() returns them), then the table -- the host stage,
        usable on a host-only context."""
        g = guide.to_c()
        n = len(alignments)
        arr = (AlnT * max(1, n))(*[a.to_c() for a in alignments])
        out = ctypes.POINTER(CountsT)()
        _lib.check(self._h, lib.calitas_hits_counts(self._h, ctypes.byref(g), ctypes.byref(params), arr, n, ctypes.byref(out)))
        return self._take_counts(out)

    def _site_region(self, pattern, chrom, start, end):
        if not isinstance(pattern, Guide):
            pattern = Guide(pattern)
        if chrom is None:
            index = -1
        elif isinstance(chrom, str):
            if chrom not in self.contig_names:
                raise ValueError("Unknown chromosome: %s" % chrom)
            index = self.contig_names.index(chrom)
        else:
            index = int(chrom)
        return pattern, index, int(start), 0 if end is None else int(end)

    def _key_call(self, pattern, queries, key_length, chrom, start, end, max_mismatches=0):
        """What count_copies, count_near, score_near and list_near begin with, as a _KeyCall: the pattern as a Guide, K (key_length
        None: the whole protospacer), M, the queries as one byte per letter (text) and their number n, the width of a row of counts,
        the region's contig index, start and end."""
        pattern, index, start, end = self._site_region(pattern, chrom, start, end)
        queries = [q.decode() if isinstance(q, bytes) else str(q) for q in queries]
        K = pattern.protospacer_length if key_length is None else int(key_length)
        M = int(max_mismatches)
        for i, q in enumerate(queries):
            if len(q) != K:
                raise ValueError("queries[%d] has %d letters, the key has %d" % (i, len(q), K))
        # (latin-1 keeps one byte per letter whatever the letter: the library names a bad one by its query's index)
        text = "".join(queries).encode("latin-1", "replace")
        row = min(max(M, 0), 3) + 1                   # (an M outside 0 .. 3 is the library's to refuse)
        return _KeyCall(pattern, K, M, text, len(queries), row, index, start, end)

    @staticmethod
    def _take_records(out, n, ctype, dtype):
        """A block of n records the library allocated, as a numpy structured array of its own; the block is freed."""
        import numpy as np
        try:
            if n == 0:
                return np.zeros(0, dtype=dtype)
            block = (ctypes.c_char * (n * ctypes.sizeof(ctype))).from_address(ctypes.addressof(out.contents))
            return np.frombuffer(block, dtype=dtype).copy()
        finally:
            lib.calitas_free(out)

    def find_sites(self, pattern, chrom=None, start=0, end=None, host=False, filter=None):
        """calitas_find_sites: every place of the region where a guide of the IUPAC `pattern` (a Guide or its `-i` string, e.g.
        "NNNNNNNNNNNNNNNNNNNNnrg"; aux PAMs through Guide(..., aux)) can be cut out, as a numpy structured array with the fields of
        calitas_site_t (SITE_DTYPE; strand as the byte b'+' / b'-'), sorted by contig, protospacer start, '+' before '-'.  chrom: a
        name, an index or None (every contig); [start, end) in 0-based contig coordinates, end None: the contig's end.  host=True: the
        host twin (calitas_find_sites_host), which also works on a host-only context.  filter: a SiteFilter -- only the sites whose
        protospacer passes it (calitas_find_sites_filtered, on the device inside the same kernel); None: the unfiltered entry points."""
        pattern, index, start, end = self._site_region(pattern, chrom, start, end)
        g = pattern.to_c()
        out, n = ctypes.POINTER(SiteT)(), ctypes.c_uint64()
        if filter is None:
            fn = lib.calitas_find_sites_host if host else lib.calitas_find_sites
            rc = fn(self._h, ctypes.byref(g), index, start, end, ctypes.byref(out), ctypes.byref(n))
        else:
            f = filter.to_c()
            fn = lib.calitas_find_sites_filtered_host if host else lib.calitas_find_sites_filtered
            rc = fn(self._h, ctypes.byref(g), ctypes.byref(f), index, start, end, ctypes.byref(out), ctypes.byref(n))
        _lib.check(self._h, rc)
        return self._take_records(out, n.value, SiteT, SITE_DTYPE)

    def count_sites(self, pattern, chrom=None, start=0, end=None, filter=None):
        """calitas_count_sites: (total, per_contig_strand) -- the number of sites find_sites would list and a numpy uint64 array
        [n_contigs][2] ('+' first) of them, from the kernel's first pass alone: no record is written or copied.  filter: as in
        find_sites (calitas_count_sites_filtered)."""
        import numpy as np
        pattern, index, start, end = self._site_region(pattern, chrom, start, end)
        g = pattern.to_c()
        table = np.zeros((max(1, len(self.contig_names)), 2), dtype=np.uint64)
        n = ctypes.c_uint64()
        cells = table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        if filter is None:
            rc = lib.calitas_count_sites(self._h, ctypes.byref(g), index, start, end, cells, ctypes.byref(n))
        else:
            f = filter.to_c()
            rc = lib.calitas_count_sites_filtered(self._h, ctypes.byref(g), ctypes.byref(f), index, start, end, cells, ctypes.byref(n))
        _lib.check(self._h, rc)
        return n.value, table[:len(self.contig_names)]

    def count_copies(self, pattern, queries, key_length=None, chrom=None, start=0, end=None, host=False):
        """calitas_count_copies: per query the number of sites of `pattern` (as count_sites counts them, unfiltered) whose KEY equals it,
        a numpy uint64 array in the queries' order.  The key of a site is its protospacer as the guide reads it -- GuideSite.guide
        without the PAM -- cut to its PAM-proximal key_length bases: the last ones for a 3' PAM or none, the first for a 5' PAM;
        None: the whole protospacer.  queries: strings of that one length, A C G T in either case (U as T); a list or any iterable.
        A guide cut from the reference counts itself.  host=True: the host twin (calitas_count_copies_host), also on a host-only
        context."""
        import numpy as np
        c = self._key_call(pattern, queries, key_length, chrom, start, end)
        g = c.pattern.to_c()
        out = np.zeros(max(1, c.n), dtype=np.uint64)
        fn = lib.calitas_count_copies_host if host else lib.calitas_count_copies
        rc = fn(self._h, ctypes.byref(g), 0 if key_length is None else c.K, c.index, c.start, c.end, c.text, c.n,
                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
        _lib.check(self._h, rc)
        return out[:c.n]

    def count_near(self, pattern, queries, max_mismatches, key_length=None, chrom=None, start=0, end=None, host=False):
        """calitas_count_near: per query the number of sites of `pattern` (as count_sites counts them, unfiltered) whose key differs from
        it at exactly d positions, d = 0 .. M = max_mismatches (0 .. 3): a numpy uint64 array of shape (len(queries), M + 1) in the
        queries' order.  Key, key_length and queries as in count_copies, whose result is column 0; the key has at least M + 1 bases.  A
        Hamming count over the key next to a PAM that matches the pattern: no gaps, no PAM mismatches.  host=True: the host twin
        (calitas_count_near_host; sites x queries comparisons), also on a host-only context."""
        import numpy as np
        c = self._key_call(pattern, queries, key_length, chrom, start, end, max_mismatches)
        g = c.pattern.to_c()
        out = np.zeros((max(1, c.n), c.row), dtype=np.uint64)
        fn = lib.calitas_count_near_host if host else lib.calitas_count_near
        rc = fn(self._h, ctypes.byref(g), 0 if key_length is None else c.K, c.M, c.index, c.start, c.end, c.text, c.n,
                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
        _lib.check(self._h, rc)
        return out[:c.n]

    def score_near(self, pattern, queries, max_mismatches, model, chrom=None, start=0, end=None, host=False):
        """calitas_score_near: count_near over the whole protospacer, and per query the sum and the maximum of its near copies' scores
        under `model` (a ScoreModel of the protospacer's length; near_score is the contract on one pair) -- a NearScores.  Sites at
        d = 0 are counted, not scored.  host=True: the host twin (calitas_score_near_host), also on a host-only context."""
        import numpy as np
        c = self._key_call(pattern, queries, None, chrom, start, end, max_mismatches)
        g = c.pattern.to_c()
        m = model.to_c() if model is not None else None
        n = c.n
        near = np.zeros((max(1, n), c.row), dtype=np.uint64)
        words = np.zeros((max(1, n), 2), dtype=np.uint64)
        fn = lib.calitas_score_near_host if host else lib.calitas_score_near
        rc = fn(self._h, ctypes.byref(g), c.M, ctypes.byref(m) if m is not None else None, c.index, c.start, c.end, c.text, n,
                near.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
        _lib.check(self._h, rc)
        return NearScores(near[:n], words[:n, 0].copy(), words[:n, 1].copy())

    def list_near(self, pattern, queries, max_mismatches, model=None, limit=1000, chrom=None, start=0, end=None, host=False):
        """calitas_list_near: count_near over the whole protospacer, and per query the records of its sites at d = 0 .. M -- where they
        stand, what differs and the pair's score under `model` (a ScoreModel; None: no weights, every score 2^32) -- a NearList.  A
        query whose counts sum to more than `limit` (1 .. 4096) lists nothing.  near_hits_of is the contract on one query.  host=True:
        the host twin (calitas_list_near_host), also on a host-only context."""
        import numpy as np
        c = self._key_call(pattern, queries, None, chrom, start, end, max_mismatches)
        limit = int(limit)
        if not 0 <= limit < 1 << 32:
            raise ValueError("limit is 1 .. %d, not %d" % (_lib.NEAR_LIST_MAX, limit))
        g = c.pattern.to_c()
        m = model.to_c() if model is not None else None
        n = c.n
        near = np.zeros((max(1, n), c.row), dtype=np.uint64)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        out = ctypes.POINTER(_lib.NearHitT)()
        n_hits = ctypes.c_uint64()
        fn = lib.calitas_list_near_host if host else lib.calitas_list_near
        rc = fn(self._h, ctypes.byref(g), c.M, ctypes.byref(m) if m is not None else None, c.index, c.start, c.end, c.text, n, limit,
                near.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(out),
                ctypes.byref(n_hits))
        _lib.check(self._h, rc)
        hits = self._take_records(out, n_hits.value, _lib.NearHitT, NEAR_HIT_DTYPE)
        return NearList(near[:n], offsets, hits, limit, c.pattern.protospacer_length)

    def find_sites_scored(self, pattern, model, min_score=None, filter=None, chrom=None, start=0, end=None, host=False):
        """calitas_find_sites_scored: (sites, scores) -- the records of find_sites(pattern, filter=filter) and, in an int32 array beside
        them, each site's on-target activity under `model` (an ActivityModel; activity_of is the contract on one context), Q16.  A site
        whose window leaves its contig or holds a letter other than A C G T U has ACTIVITY_NONE.  min_score: a Q16 integer -- only the
        sites that score at least that much, which drops the unscored ones too; None keeps everything.  host=True: the host twin
        (calitas_find_sites_scored_host), also on a host-only context."""
        import numpy as np
        pattern, index, start, end = self._site_region(pattern, chrom, start, end)
        floor = _lib.ACTIVITY_NONE if min_score is None else int(min_score)
        if not -(1 << 31) <= floor < 1 << 31:
            raise ValueError("min_score is a 32-bit Q16 integer, not %d" % floor)
        g = pattern.to_c()
        f = filter.to_c() if filter is not None else None
        m = model.to_c() if model is not None else None
        out, words, n = ctypes.POINTER(SiteT)(), ctypes.POINTER(ctypes.c_int32)(), ctypes.c_uint64()
        fn = lib.calitas_find_sites_scored_host if host else lib.calitas_find_sites_scored
        rc = fn(self._h, ctypes.byref(g), ctypes.byref(f) if f is not None else None, ctypes.byref(m) if m is not None else None, floor, index, start, end,
                ctypes.byref(out), ctypes.byref(words), ctypes.byref(n))
        _lib.check(self._h, rc)
        try:
            scores = np.ctypeslib.as_array(words, shape=(n.value,)).astype(np.int32) if n.value else np.zeros(0, dtype=np.int32)   # (astype copies)
        finally:
            lib.calitas_free(words)
        return self._take_records(out, n.value, SiteT, SITE_DTYPE), scores

    def count_sites_scored(self, pattern, model, min_score=None, filter=None, chrom=None, start=0, end=None, host=False):
        """calitas_find_sites_scored without its blocks: the number of sites find_sites_scored would return."""
        pattern, index, start, end = self._site_region(pattern, chrom, start, end)
        g = pattern.to_c()
        f = filter.to_c() if filter is not None else None
        m = model.to_c()
        n = ctypes.c_uint64()
        fn = lib.calitas_find_sites_scored_host if host else lib.calitas_find_sites_scored
        rc = fn(self._h, ctypes.byref(g), ctypes.byref(f) if f is not None else None, ctypes.byref(m), _lib.ACTIVITY_NONE if min_score is None else int(min_score),
                index, start, end, None, None, ctypes.byref(n))
        _lib.check(self._h, rc)
        return n.value

    def find_sites_microhomology(self, pattern, model, cut_offset=None, min_out_of_frame=0, filter=None, chrom=None, start=0, end=None, host=False):
        """calitas_find_sites_microhomology: (sites, scores) -- the records of find_sites(pattern, filter=filter) and, in a structured array
        beside them (MH_SCORE_DTYPE: total_q16, out_of_frame_q16), each site's microhomology score around its cut under `model` (a
        MicrohomologyModel; microhomology_of is the contract on one window).  cut_offset: bases into the protospacer as the guide reads,
        0 .. L; None: L - 3, the Cas9 cut, which needs a 3' PAM.  A site whose window leaves its contig or holds a letter other than
        A C G T U has MH_NONE in both.  min_out_of_frame: a per-mille 0 .. 1000 -- 0 keeps everything, otherwise only the scored sites with
        total > 0 and out_of_frame * 1000 >= min_out_of_frame * total.  host=True: the host twin, also on a host-only context."""
        import numpy as np
        pattern, index, start, end = self._site_region(pattern, chrom, start, end)
        if cut_offset is None:
            if not pattern.pam_is_three_prime:
                raise ValueError("cut_offset is required unless the pattern has a 3' PAM (then it is L - 3)")
            cut_offset = pattern.protospacer_length - 3
        g = pattern.to_c()
        f = filter.to_c() if filter is not None else None
        m = model.to_c(cut_offset) if model is not None else None
        out, words, n = ctypes.POINTER(SiteT)(), ctypes.POINTER(_lib.MhScoreT)(), ctypes.c_uint64()
        fn = lib.calitas_find_sites_microhomology_host if host else lib.calitas_find_sites_microhomology
        rc = fn(self._h, ctypes.byref(g), ctypes.byref(f) if f is not None else None, ctypes.byref(m) if m is not None else None, int(min_out_of_frame),
                index, start, end, ctypes.byref(out), ctypes.byref(words), ctypes.byref(n))
        _lib.check(self._h, rc)
        scores = self._take_records(words, n.value, _lib.MhScoreT, MH_SCORE_DTYPE)
        return self._take_records(out, n.value, SiteT, SITE_DTYPE), scores

    def count_sites_microhomology(self, pattern, model, cut_offset=None, min_out_of_frame=0, filter=None, chrom=None, start=0, end=None, host=False):
        """calitas_find_sites_microhomology without its blocks: the number of sites find_sites_microhomology would return."""
        pattern, index, start, end = self._site_region(pattern, chrom, start, end)
        if cut_offset is None:
            if not pattern.pam_is_three_prime:
                raise ValueError("cut_offset is required unless the pattern has a 3' PAM (then it is L - 3)")
            cut_offset = pattern.protospacer_length - 3
        g = pattern.to_c()
        f = filter.to_c() if filter is not None else None
        m = model.to_c(cut_offset)
        n = ctypes.c_uint64()
        fn = lib.calitas_find_sites_microhomology_host if host else lib.calitas_find_sites_microhomology
        rc = fn(self._h, ctypes.byref(g), ctypes.byref(f) if f is not None else None, ctypes.byref(m), int(min_out_of_frame), index, start, end, None, None,
                ctypes.byref(n))
        _lib.check(self._h, rc)
        return n.value

    def _site_regions_opt(self, pattern, classes, extent):
        """The calitas_site_regions_t of classes (None: every class but "elsewhere"; names or indices of the context's Regions, or an
        integer mask) and extent ((from, to), None: the whole protospacer)."""
        if isinstance(classes, int) and not isinstance(classes, bool):
            mask = classes
        elif classes is None:
            mask = ((1 << len(self.regions.classes)) - 2) if self.regions is not None else 0xFE
        else:
            names = [c for c in classes.split(",") if c] if isinstance(classes, str) else list(classes)
            mask = 0
            for c in names:
                if isinstance(c, str):
                    if self.regions is None:
                        raise ValueError("class names need a Regions set on the context (set_regions)")
                    mask |= self.regions.mask_of([c])
                else:
                    mask |= 1 << int(c)
        if not 0 <= mask < 1 << 32:
            raise ValueError("the class mask of a regions listing is an integer of 32 bits")
        a, b = (0, 0) if extent is None else (int(extent[0]), int(extent[1]))
        if not (0 <= a < 256 and 0 <= b < 256):
            raise ValueError("extent (%d, %d): positions of the protospacer, 0 <= from < to <= its length" % (a, b))
        if extent is not None and (a, b) == (0, 0):
            raise ValueError("extent (0, 0) is empty: None means the whole protospacer")
        return _lib.SiteRegionsT(mask, a, b, 0)

    def find_sites_regions(self, pattern, classes=None, extent=None, filter=None, chrom=None, start=0, end=None, host=False):
        """calitas_find_sites_regions: (sites, classes) -- the records of find_sites(pattern, filter=filter) whose class under the
        context's regions (set_regions) is one of `classes`, and in a uint8 array beside them each record's class index.  classes:
        names or indices (an iterable or a comma-separated string; "elsewhere" is class 0), None: every class but "elsewhere".  extent:
        (from, to), the positions of the protospacer as the guide reads that are classed, 0-based and half-open -- (16, 18) on a 20-mer
        with a 3' PAM is the two bases beside the Cas9 cut; None: the whole protospacer.  site_class_of states the rule on one site.
        host=True: the host twin (calitas_find_sites_regions_host), also on a host-only context."""
        import numpy as np
        pattern, index, start, end = self._site_region(pattern, chrom, start, end)
        opt = self._site_regions_opt(pattern, classes, extent)
        g = pattern.to_c()
        f = filter.to_c() if filter is not None else None
        out, cls, n = ctypes.POINTER(SiteT)(), ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
        fn = lib.calitas_find_sites_regions_host if host else lib.calitas_find_sites_regions
        rc = fn(self._h, ctypes.byref(g), ctypes.byref(f) if f is not None else None, ctypes.byref(opt), index, start, end, ctypes.byref(out),
                ctypes.byref(cls), ctypes.byref(n))
        _lib.check(self._h, rc)
        try:
            of = np.ctypeslib.as_array(cls, shape=(n.value,)).astype(np.uint8) if n.value else np.zeros(0, dtype=np.uint8)   # (astype copies)
        finally:
            lib.calitas_free(cls)
        return self._take_records(out, n.value, SiteT, SITE_DTYPE), of

    def count_sites_regions(self, pattern, classes=None, extent=None, filter=None, chrom=None, start=0, end=None, host=False):
        """calitas_count_sites_regions: a numpy uint64 array [n_classes][2] ('+' first) of the sites find_sites_regions would return,
        per class and strand; the rows of classes outside `classes` are 0.  Nothing but the counters is copied back."""
        import numpy as np
        pattern, index, start, end = self._site_region(pattern, chrom, start, end)
        opt = self._site_regions_opt(pattern, classes, extent)
        g = pattern.to_c()
        f = filter.to_c() if filter is not None else None
        table = np.zeros((_lib.REGION_CLASSES_MAX, 2), dtype=np.uint64)
        n = ctypes.c_uint64()
        fn = lib.calitas_count_sites_regions_host if host else lib.calitas_count_sites_regions
        rc = fn(self._h, ctypes.byref(g), ctypes.byref(f) if f is not None else None, ctypes.byref(opt), index, start, end,
                table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(n))
        _lib.check(self._h, rc)
        table = table[:len(self.regions.classes)] if self.regions is not None else table
        assert int(table.sum()) == n.value
        return table

    def find_site_pairs(self, pattern, spec, filter=None, chrom=None, start=0, end=None, host=False):
        """calitas_find_site_pairs: (sites, pairs) -- the records of find_sites(pattern, filter=filter) and, as a numpy structured array
        with the fields of calitas_site_pair_t (SITE_PAIR_DTYPE), the pairs of them that `spec` (a SitePairs) admits: left and right
        index `sites`, distance is the right cut minus the left one, orientation (left is '-') + 2 (right is '-').  Ordered by the
        smaller and then the larger of the two indices.  site_pairs_of is the contract as a plain double loop.  host=True: the host
        twin (calitas_find_site_pairs_host), also on a host-only context."""
        pattern, index, start, end = self._site_region(pattern, chrom, start, end)
        opt = spec.to_c(pattern)
        g = pattern.to_c()
        f = filter.to_c() if filter is not None else None
        out, n = ctypes.POINTER(SiteT)(), ctypes.c_uint64()
        out_pairs, n_pairs = ctypes.POINTER(_lib.SitePairT)(), ctypes.c_uint64()
        fn = lib.calitas_find_site_pairs_host if host else lib.calitas_find_site_pairs
        rc = fn(self._h, ctypes.byref(g), ctypes.byref(f) if f is not None else None, ctypes.byref(opt), index, start, end, ctypes.byref(out),
                ctypes.byref(n), ctypes.byref(out_pairs), ctypes.byref(n_pairs))
        _lib.check(self._h, rc)
        try:
            pairs = self._take_records(out_pairs, n_pairs.value, _lib.SitePairT, SITE_PAIR_DTYPE)
        finally:
            sites = self._take_records(out, n.value, SiteT, SITE_DTYPE)
        return sites, pairs

    def count_site_pairs(self, pattern, spec, filter=None, chrom=None, start=0, end=None, host=False):
        """calitas_count_site_pairs: (n_sites, n_pairs, per_orientation) of what find_site_pairs would return, per_orientation a numpy
        uint64 array of the four orientations' pairs ("++", "-+", "+-", "--").  Nothing but the counters is copied back."""
        import numpy as np
        pattern, index, start, end = self._site_region(pattern, chrom, start, end)
        opt = spec.to_c(pattern)
        g = pattern.to_c()
        f = filter.to_c() if filter is not None else None
        by = np.zeros(4, dtype=np.uint64)
        n, n_pairs = ctypes.c_uint64(), ctypes.c_uint64()
        fn = lib.calitas_count_site_pairs_host if host else lib.calitas_count_site_pairs
        rc = fn(self._h, ctypes.byref(g), ctypes.byref(f) if f is not None else None, ctypes.byref(opt), index, start, end, ctypes.byref(n),
                ctypes.byref(n_pairs), by.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
        _lib.check(self._h, rc)
        return n.value, n_pairs.value, by

    def _snv_array(self, snvs):
        import numpy as np
        if not (hasattr(snvs, "dtype") and snvs.dtype == np.dtype(SNV_DTYPE)):
            snvs = snvs_of(snvs, self)
        return np.ascontiguousarray(snvs)

    def find_allele_sites(self, pattern, snvs, host=False):
        """calitas_find_allele_sites: the sites each single-nucleotide variant creates (kind 1), destroys (kind 2) or changes (kind 3),
        as an AlleleSites -- records with the fields of calitas_allele_site_t (ALLELE_SITE_DTYPE) ordered by snv_index, protospacer
        start, '+' before '-', and a status byte per SNV.  snvs: an array of SNV_DTYPE, or (chrom, pos1, ref, alt) tuples (snvs_of).
        allele_sites_of is the contract in plain Python.  host=True: the host twin, also on a host-only context."""
        import numpy as np
        if not isinstance(pattern, Guide):
            pattern = Guide(pattern)
        snvs = self._snv_array(snvs)
        g = pattern.to_c()
        status = np.zeros(max(1, len(snvs)), dtype=np.uint8)
        out, n = ctypes.POINTER(_lib.AlleleSiteT)(), ctypes.c_uint64()
        fn = lib.calitas_find_allele_sites_host if host else lib.calitas_find_allele_sites
        rc = fn(self._h, ctypes.byref(g), snvs.ctypes.data if len(snvs) else None, len(snvs), ctypes.byref(out), ctypes.byref(n), status.ctypes.data)
        _lib.check(self._h, rc)
        return AlleleSites(self._take_records(out, n.value, _lib.AlleleSiteT, ALLELE_SITE_DTYPE), status[:len(snvs)], pattern)

    def count_allele_sites(self, pattern, snvs, host=False):
        """calitas_count_allele_sites: (n, per_kind, status) of what find_allele_sites would return; per_kind a numpy uint64 array of
        four, [0] always 0.  No record is copied back."""
        import numpy as np
        if not isinstance(pattern, Guide):
            pattern = Guide(pattern)
        snvs = self._snv_array(snvs)
        g = pattern.to_c()
        status = np.zeros(max(1, len(snvs)), dtype=np.uint8)
        by = np.zeros(4, dtype=np.uint64)
        n = ctypes.c_uint64()
        fn = lib.calitas_count_allele_sites_host if host else lib.calitas_count_allele_sites
        rc = fn(self._h, ctypes.byref(g), snvs.ctypes.data if len(snvs) else None, len(snvs), by.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                ctypes.byref(n), status.ctypes.data)
        _lib.check(self._h, rc)
        return n.value, by, status[:len(snvs)]

    def find_edit_sites(self, pattern, edit, snvs, host=False):
        """calitas_find_edit_sites: the guides that put each single-nucleotide variant into the window of the base editor `edit` (a
        BaseEdit) on the strand it can change it on, as an EditSites -- records with the fields of calitas_edit_site_t
        (EDIT_SITE_DTYPE) ordered by snv_index, then protospacer start, and a status byte per SNV.  snvs: an array of SNV_DTYPE, or
        (chrom, pos1, ref, alt) tuples (snvs_of).  edit_sites_of is the contract in plain Python.  host=True: the host twin, also on
        a host-only context."""
        import numpy as np
        if not isinstance(pattern, Guide):
            pattern = Guide(pattern)
        snvs = self._snv_array(snvs)
        g, e = pattern.to_c(), edit.to_c()
        status = np.zeros(max(1, len(snvs)), dtype=np.uint8)
        out, n = ctypes.POINTER(_lib.EditSiteT)(), ctypes.c_uint64()
        fn = lib.calitas_find_edit_sites_host if host else lib.calitas_find_edit_sites
        rc = fn(self._h, ctypes.byref(g), ctypes.byref(e), snvs.ctypes.data if len(snvs) else None, len(snvs), ctypes.byref(out), ctypes.byref(n),
                status.ctypes.data)
        _lib.check(self._h, rc)
        return EditSites(self._take_records(out, n.value, _lib.EditSiteT, EDIT_SITE_DTYPE), status[:len(snvs)], pattern, edit, snvs)

    def count_edit_sites(self, pattern, edit, snvs, host=False):
        """calitas_count_edit_sites: (n, per_bystanders, status) of what find_edit_sites would return; per_bystanders a numpy uint64
        array of the records with 0, 1, 2 and 3 or more bystanders.  No record is copied back."""
        import numpy as np
        if not isinstance(pattern, Guide):
            pattern = Guide(pattern)
        snvs = self._snv_array(snvs)
        g, e = pattern.to_c(), edit.to_c()
        status = np.zeros(max(1, len(snvs)), dtype=np.uint8)
        by = np.zeros(4, dtype=np.uint64)
        n = ctypes.c_uint64()
        fn = lib.calitas_count_edit_sites_host if host else lib.calitas_count_edit_sites
        rc = fn(self._h, ctypes.byref(g), ctypes.byref(e), snvs.ctypes.data if len(snvs) else None, len(snvs),
                by.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(n), status.ctypes.data)
        _lib.check(self._h, rc)
        return n.value, by, status[:len(snvs)]

    def site_presence(self):
        """(test hook) calitas_site_presence: (bytes, first_word) -- the table the regions listing skips segments by, a uint8 array with
        one byte per 256 words (8192 bases) of the packed space from word first_word on; bit c: class c comes near the segment."""
        import numpy as np
        out, n, first = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._h, lib.calitas_site_presence(self._h, ctypes.byref(out), ctypes.byref(n), ctypes.byref(first)))
        try:
            return (np.ctypeslib.as_array(out, shape=(n.value,)).astype(np.uint8) if n.value else np.zeros(0, dtype=np.uint8)), first.value
        finally:
            lib.calitas_free(out)

    @staticmethod
    def _scores_of(c):
        """A calitas_scores_t as a Scores object (the table is copied)."""
        import numpy as np
        t = c.table
        shape = (2, t.n_mm, t.n_gaps, t.n_pam)
        n = 2 * t.n_mm * t.n_gaps * t.n_pam
        table = np.ctypeslib.as_array(t.counts, shape=(n,)).astype(np.uint64).reshape(shape)   # (astype copies)
        if int(table.sum()) != c.rows or t.rows != c.rows or c.perfect > c.rows:
            raise CalitasError(_lib.EHIP, "the scores block does not add up to its rows")
        return Scores(int(c.rows), int(c.perfect), int(c.sum_q32), int(c.max_q32), table)

    @staticmethod
    def _take_scores(ptr):
        """A calitas_scores_t block as a Scores object; the block is freed."""
        try:
            return Context._scores_of(ptr.contents)
        finally:
            lib.calitas_free(ptr)

    def _take_top(self, ptr):
        """A calitas_top_t block as a Top object; the block is freed."""
        try:
            t = ptr.contents
            scores = self._scores_of(t.scores)
            if t.n != min(t.k, scores.rows - scores.perfect):
                raise CalitasError(_lib.EHIP, "the top block does not hold min(k, imperfect rows) records")
            import numpy as np
            names = self.contig_names
            # (one copy and one tolist(): a ctypes field access per value cost 0.5 ms per 256 records, a quarter of an hg38-sized call)
            rec = np.frombuffer(ctypes.string_at(t.hits, 24 * t.n), dtype=TOP_DTYPE).tolist() if t.n else []
            hits = [TopHit(s, names[c], a, b, st.decode(), mm, gp, pm) for s, c, a, b, st, mm, gp, pm in rec]
            return Top(scores, int(t.k), hits)
        finally:
            lib.calitas_free(ptr)

    def search_top(self, guide, params, model, k):
        """calitas_search_top: search_scores plus the k (1 .. 256) highest-scoring imperfect hits -- a Top object.  Equal to top_of_rows
        of the hits.txt search_hits gives for the same guide and params, window range included; no text is built or copied."""
        g = guide.to_c()
        m = model.to_c()
        out = ctypes.POINTER(TopT)()
        _lib.check(self._h, lib.calitas_search_top(self._h, ctypes.byref(g), ctypes.byref(params), ctypes.byref(m), _top_k(k), ctypes.byref(out)))
        return self._take_top(out)

    def search_top_batch(self, guides, params, model, k):
        """calitas_search_top_batch: a list of Top, one per guide (all of one length: one model serves them), pipelined on the device
        like search_scores_batch."""
        n = len(guides)
        keep = [g.to_c() for g in guides]
        garr = (GuideT * n)(*keep)
        m = model.to_c()
        out = (ctypes.POINTER(TopT) * n)()
        _lib.check(self._h, lib.calitas_search_top_batch(self._h, n, garr, ctypes.byref(params), ctypes.byref(m), _top_k(k), out))
        return [self._take_top(out[i]) for i in range(n)]

    def hits_top(self, guide, params, model, k, alignments):
        """calitas_hits_top: hits_scores plus the list -- the host stage, usable on a host-only context."""
        g = guide.to_c()
        m = model.to_c()
        n = len(alignments)
        arr = (AlnT * max(1, n))(*[a.to_c() for a in alignments])
        out = ctypes.POINTER(TopT)()
        _lib.check(self._h, lib.calitas_hits_top(self._h, ctypes.byref(g), ctypes.byref(params), ctypes.byref(m), _top_k(k), arr, n, ctypes.byref(out)))
        return self._take_top(out)

    def set_regions(self, regions):
        """calitas_set_regions: a Regions object (None or an empty one clears the set).  The set is flattened and brought to the device
        here, once; set_reference* and load_index drop it.  Works on a host-only context."""
        self.regions = None
        if regions is None or not regions.intervals:
            _lib.check(self._h, lib.calitas_set_regions(self._h, 0, None, 0))
            return
        index = {nm: i for i, nm in enumerate(self.contig_names)}
        for chrom, _, _, _ in regions.intervals:
            if chrom not in index:
                raise ValueError("Unknown chromosome: %s" % chrom)
        n = len(regions.intervals)
        arr = (RegionT * n)(*[RegionT(index[chrom], a, b, c) for chrom, a, b, c in regions.intervals])
        _lib.check(self._h, lib.calitas_set_regions(self._h, n, arr, len(regions.classes)))
        self.regions = regions

    def region_class(self, chrom, start, end):
        """(test hook) The class the library's flattened set gives the extent [start, end) of a chromosome."""
        return lib.calitas_region_class(self._h, self.contig_names.index(chrom), start, end)

    def _take_regions(self, ptr):
        """A calitas_regions_t block as a RegionScores object; the block is freed."""
        try:
            r = ptr.contents
            t = r.top
            scores = self._scores_of(t.scores)
            import numpy as np
            names = self.contig_names
            rec = np.frombuffer(ctypes.string_at(t.hits, 24 * t.n), dtype=TOP_DTYPE).tolist() if t.n else []
            hits = [TopHit(s, names[c], a, b, st.decode(), mm, gp, pm) for s, c, a, b, st, mm, gp, pm in rec]
            hit_class = list(ctypes.string_at(r.hit_class, t.n)) if t.n else []
            by_class = [self._scores_of(r.by_class[c]) for c in range(r.n_classes)]
            classes = list(self.regions.classes) if getattr(self, "regions", None) is not None else ["class%d" % c for c in range(r.n_classes)]
            return RegionScores(Top(scores, int(t.k), hits), classes, by_class, hit_class)
        finally:
            lib.calitas_free(ptr)

    def search_regions(self, guide, params, model, k, list_mask=None):
        """calitas_search_regions: search_top split by the context's regions -- a RegionScores object.  k is 0 .. 256 (0: no list);
        list_mask: bit c set = hits of class c may be listed (None: every class).  Equal to regions_of_rows of the hits.txt
        search_hits gives for the same guide and params, window range included; no text is built or copied."""
        g = guide.to_c()
        m = model.to_c()
        out = ctypes.POINTER(RegionsT)()
        _lib.check(self._h, lib.calitas_search_regions(self._h, ctypes.byref(g), ctypes.byref(params), ctypes.byref(m), _top_k(k), _mask(list_mask),
                                                       ctypes.byref(out)))
        return self._take_regions(out)

    def search_regions_batch(self, guides, params, model, k, list_mask=None):
        """calitas_search_regions_batch: a list of RegionScores, one per guide (all of one length), pipelined like search_top_batch."""
        n = len(guides)
        keep = [g.to_c() for g in guides]
        garr = (GuideT * n)(*keep)
        m = model.to_c()
        out = (ctypes.POINTER(RegionsT) * n)()
        _lib.check(self._h, lib.calitas_search_regions_batch(self._h, n, garr, ctypes.byref(params), ctypes.byref(m), _top_k(k), _mask(list_mask), out))
        return [self._take_regions(out[i]) for i in range(n)]

    def hits_regions(self, guide, params, model, k, alignments, list_mask=None):
        """calitas_hits_regions: hits_top split by the context's regions -- the host stage, usable on a host-only context."""
        g = guide.to_c()
        m = model.to_c()
        n = len(alignments)
        arr = (AlnT * max(1, n))(*[a.to_c() for a in alignments])
        out = ctypes.POINTER(RegionsT)()
        _lib.check(self._h, lib.calitas_hits_regions(self._h, ctypes.byref(g), ctypes.byref(params), ctypes.byref(m), _top_k(k), _mask(list_mask), arr, n,
                                                     ctypes.byref(out)))
        return self._take_regions(out)

    def search_scores(self, guide, params, model):
        """calitas_search_scores: search_counts plus the specificity score of the guide's hits under `model` (a ScoreModel of the
        guide's protospacer length) -- a Scores object.  Equal to scores_of_rows of the hits.txt search_hits gives for the same guide
        and params, window range included; no text is built or copied."""
        g = guide.to_c()
        m = model.to_c()
        out = ctypes.POINTER(ScoresT)()
        _lib.check(self._h, lib.calitas_search_scores(self._h, ctypes.byref(g), ctypes.byref(params), ctypes.byref(m), ctypes.byref(out)))
        return self._take_scores(out)

    def search_scores_batch(self, guides, params, model):
        """calitas_search_scores_batch: a list of Scores, one per guide (all of one length: one model serves them), pipelined on the
        device like search_counts_batch."""
        n = len(guides)
        keep = [g.to_c() for g in guides]
        garr = (GuideT * n)(*keep)
        m = model.to_c()
        out = (ctypes.POINTER(ScoresT) * n)()
        _lib.check(self._h, lib.calitas_search_scores_batch(self._h, n, garr, ctypes.byref(params), ctypes.byref(m), out))
        return [self._take_scores(out[i]) for i in range(n)]

    def hits_scores(self, guide, params, model, alignments):
        """calitas_hits_scores: removeOverlaps on a guide's alignments (as search() returns them), then table and score -- the host
        stage, usable on a host-only context."""
        g = guide.to_c()
        m = model.to_c()
        n = len(alignments)
        arr = (AlnT * max(1, n))(*[a.to_c() for a in alignments])
        out = ctypes.POINTER(ScoresT)()
        _lib.check(self._h, lib.calitas_hits_scores(self._h, ctypes.byref(g), ctypes.byref(params), ctypes.byref(m), arr, n, ctypes.byref(out)))
        return self._take_scores(out)

    def timing(self):
        t = TimingT()
        _lib.check(self._h, lib.calitas_get_timing(self._h, ctypes.byref(t)))
        return {f: getattr(t, f) for f, _ in TimingT._fields_}

    def hits_tsv_raw(self, guide, guide_id, params, alns_ptr, n, version=None, time_stamp=None, decode=True):
        """calitas_hits_tsv on a C array of alignments. decode=False returns (None, n_rows) without copying the text
        into a Python str (the rows are still built)."""
        g = guide.to_c()
        tsv, rows = ctypes.c_void_p(), ctypes.c_uint64()
        _lib.check(self._h, lib.calitas_hits_tsv(self._h, ctypes.byref(g), guide_id.encode(), ctypes.byref(params), alns_ptr, n,
                                                 version.encode() if version else None, time_stamp.encode() if time_stamp else None,
                                                 ctypes.byref(tsv), ctypes.byref(rows)))
        text = ctypes.string_at(tsv).decode() if decode else None
        lib.calitas_free(tsv)
        return text, rows.value

    def hits_tsv(self, guide, guide_id, params, alignments, version=None, time_stamp=None):
        n = len(alignments)
        arr = (AlnT * max(1, n))(*[a.to_c() for a in alignments])
        return self.hits_tsv_raw(guide, guide_id, params, arr, n, version, time_stamp)

    def padded_strings(self, guide, aln):
        g, a = guide.to_c(), aln.to_c()
        bufs = [ctypes.create_string_buffer(_lib.MAX_OPS + 1) for _ in range(3)]
        _lib.check(self._h, lib.calitas_padded_strings(self._h, ctypes.byref(g), ctypes.byref(a), *bufs))
        return tuple(b.value.decode() for b in bufs)


def window_filter(alignments, max_total_diffs, max_overlap):
    """SequentialGuideAligner.scala:315-320 on one window's alignments; returns the survivors in output order."""
    n = len(alignments)
    arr = (AlnT * max(1, n))(*[a.to_c() for a in alignments])
    order = (ctypes.c_int32 * max(1, n))()
    kept = ctypes.c_int32()
    rc = lib.calitas_window_filter(arr, n, max_total_diffs, max_overlap, order, ctypes.byref(kept))
    if rc != _lib.OK:
        raise CalitasError(rc, "calitas_window_filter")
    return [alignments[order[i]] for i in range(kept.value)]


class SearchReference:
    """Mirror of the SearchReference tool (SearchReference.scala:451-649), reference-only branch.

    new SearchReference(guide=..., guideId=..., ref=..., output=...).execute() in the reference becomes
    SearchReference(guide=..., guide_id=..., ref=..., output=...).execute() here; `threads` is accepted and ignored
    (the GPU replaces the thread pool).  A Context may be passed to reuse a resident reference."""

    def __init__(self, guide, guide_id, ref=None, output=None, auxiliary_pams=(), threads=8, window_size=1000,
                 max_guide_diffs=Defaults.MaxGuideDiffs, max_pam_mismatches=Defaults.MaxPamMismatches,
                 max_gaps_between_guide_and_pam=Defaults.MaxGapsBetweenGuideAndPam, max_total_diffs=None,
                 max_overlap=Defaults.MaxOverlap, guide_mismatch_net_cost=Defaults.MismatchNetCost,
                 pam_mismatch_net_cost=Defaults.PamMismatchNetCost, genome_gap_net_cost=Defaults.GenomeGapNetCost,
                 guide_gap_net_cost=Defaults.GuideGapNetCost, chrom=None, variants=None,
                 max_variants=Defaults.MaxVariantsInCluster, context=None, device=0, eqx_by_score=0, two_stage=False):
        self.variants = variants
        self.two_stage = two_stage
        self.guide_str, self.guide_id, self.ref, self.output = guide, guide_id, ref, output
        self.query = Guide(guide, auxiliary_pams)  # SearchReference.scala:511: fail early on an invalid guide
        self.chrom = chrom
        self._kw = dict(window_size=window_size, max_guide_diffs=max_guide_diffs, max_pam_mismatches=max_pam_mismatches,
                        max_gaps_between_guide_and_pam=max_gaps_between_guide_and_pam, max_total_diffs=max_total_diffs,
                        max_overlap=max_overlap, guide_mismatch_net_cost=guide_mismatch_net_cost,
                        pam_mismatch_net_cost=pam_mismatch_net_cost, genome_gap_net_cost=genome_gap_net_cost,
                        guide_gap_net_cost=guide_gap_net_cost, max_variants=max_variants, eqx_by_score=eqx_by_score)
        self.context = context
        self.device = device
        self.timing = None
        self.wall_ms = None

    def run(self, version=None, time_stamp=None):
        """Returns (tsv_text, n_rows)."""
        ctx = self.context
        own = ctx is None
        if own:
            ctx = Context(self.device)
            ctx.set_reference_fasta(self.ref)
        try:
            chrom_index = -1
            if self.chrom is not None:
                if self.chrom not in ctx.contig_names:
                    raise ValueError("Unknown chromosome: %s" % self.chrom)
                chrom_index = ctx.contig_names.index(self.chrom)
            if self.variants is not None:   # SearchReference.scala:570-630
                from . import variants as V
                return V.search_variants(self, ctx, self.variants, chrom_index, version, time_stamp)
            params = make_params(chrom_index=chrom_index, **self._kw)
            t0 = time.perf_counter()
            if self.two_stage:   # calitas_search, then calitas_hits_tsv on the host copy of the alignments
                out, n = ctx.search_raw([self.query], params)
                try:
                    self.timing = ctx.timing()
                    text, rows = ctx.hits_tsv_raw(self.query, self.guide_id, params, out, n, version, time_stamp)
                finally:
                    lib.calitas_free(out)
            else:
                text, rows = ctx.search_hits(self.query, self.guide_id, params, version, time_stamp)
                self.timing = ctx.timing()
            self.wall_ms = (time.perf_counter() - t0) * 1e3
            return text, rows
        finally:
            if own:
                ctx.close()

    def counts(self):
        """The off-target table instead of hits.txt (Context.search_counts): a numpy uint64 array of shape (2, n_mm, n_gaps, n_pam)."""
        if self.variants is not None:
            raise ValueError("counts() covers the reference-genome branch only (no --variants)")
        ctx = self.context
        own = ctx is None
        if own:
            ctx = Context(self.device)
            ctx.set_reference_fasta(self.ref)
        try:
            chrom_index = -1
            if self.chrom is not None:
                if self.chrom not in ctx.contig_names:
                    raise ValueError("Unknown chromosome: %s" % self.chrom)
                chrom_index = ctx.contig_names.index(self.chrom)
            params = make_params(chrom_index=chrom_index, **self._kw)
            t0 = time.perf_counter()
            table = ctx.search_counts(self.query, params)
            self.timing = ctx.timing()
            self.wall_ms = (time.perf_counter() - t0) * 1e3
            return table
        finally:
            if own:
                ctx.close()

    def _score_pass(self, call):
        """What scores() and top() share: the context (this object's, or one of its own with the reference loaded), the params of the
        flags and the timing around call(ctx, params)."""
        if self.variants is not None:
            raise ValueError("scores() and top() cover the reference-genome branch only (no --variants)")
        ctx = self.context
        own = ctx is None
        if own:
            ctx = Context(self.device)
            ctx.set_reference_fasta(self.ref)
        try:
            chrom_index = -1
            if self.chrom is not None:
                if self.chrom not in ctx.contig_names:
                    raise ValueError("Unknown chromosome: %s" % self.chrom)
                chrom_index = ctx.contig_names.index(self.chrom)
            params = make_params(chrom_index=chrom_index, **self._kw)
            t0 = time.perf_counter()
            got = call(ctx, params)
            self.timing = ctx.timing()
            self.wall_ms = (time.perf_counter() - t0) * 1e3
            return got
        finally:
            if own:
                ctx.close()

    def scores(self, model):
        """The specificity score instead of hits.txt (Context.search_scores): a Scores object."""
        return self._score_pass(lambda ctx, params: ctx.search_scores(self.query, params, model))

    def top(self, model, k):
        """The scores and the k highest-scoring imperfect hits (Context.search_top): a Top object."""
        return self._score_pass(lambda ctx, params: ctx.search_top(self.query, params, model, k))

    def regions(self, model, regions, k=0, top_classes=None):
        """The scores, split by the classes of a Regions object or a BED file, and the k best imperfect hits of the classes named in
        top_classes (None: all) (Context.search_regions): a RegionScores object."""
        def call(ctx, params):
            reg = regions if isinstance(regions, Regions) else Regions.read_bed(regions, dict(zip(ctx.contig_names, ctx.contig_lengths)))
            ctx.set_regions(reg)
            return ctx.search_regions(self.query, params, model, k, None if top_classes is None else reg.mask_of(top_classes))
        return self._score_pass(call)

    def execute(self, counts=False, scores=None, top=None, regions=None, top_classes=None):
        """counts=True (`--counts`): the table as a TSV (counts_tsv) instead of hits.txt.  scores=ScoreModel (`--scores MODEL`): the
        scores TSV (scores_tsv); top=K with it (`--top K`): the top TSV (top_tsv) of the same pass behind an empty line; with counts as
        well, the counts TSV of the same pass's table follows behind an empty line.  regions=FILE.bed with scores (`--regions`): the
        classes' TSV (regions_tsv) behind the scores and an empty line, and the top TSV gains a last column `class`; top_classes
        (`--top-classes name,...`): the classes whose hits may be listed."""
        if top is not None and scores is None:
            raise ValueError("--top K requires --scores MODEL")
        if regions is not None and scores is None:
            raise ValueError("--regions FILE.bed requires --scores MODEL")
        if regions is not None and self.variants is not None:
            raise ValueError("--regions covers the reference-genome branch only (no --variants)")
        if top_classes is not None and (regions is None or top is None):
            raise ValueError("--top-classes requires --regions and --top")
        if regions is not None:
            got = self.regions(scores, regions, top or 0, top_classes)
            text = (scores_tsv(self.guide_id, got.top.scores) + "\n" + regions_tsv(self.guide_id, got)
                    + ("\n" + top_tsv(self.guide_id, got.top, [got.classes[c] for c in got.hit_class]) if top is not None else "")
                    + ("\n" + counts_tsv(self.guide_id, got.top.scores.table) if counts else ""))
        elif scores is not None:
            got = self.scores(scores) if top is None else self.top(scores, top)
            sc = got if top is None else got.scores
            text = (scores_tsv(self.guide_id, sc) + ("\n" + top_tsv(self.guide_id, got) if top is not None else "")
                    + ("\n" + counts_tsv(self.guide_id, sc.table) if counts else ""))
        else:
            text = counts_tsv(self.guide_id, self.counts()) if counts else self.run()[0]
        if self.output is None:
            import sys
            sys.stdout.write(text)
        else:
            with open(self.output, "w") as f:
                f.write(text)


# calitas_site_t as a numpy record
SITE_DTYPE = [("contig_index", "<i4"), ("protospacer_start", "<i4"), ("pam_start", "<i4"), ("strand", "S1"), ("pam_index", "i1"),
              ("pam_length", "u1"), ("protospacer_length", "u1")]

# calitas_near_hit_t
NEAR_HIT_DTYPE = [("score_q32", "<u8"), ("contig_index", "<i4"), ("protospacer_start", "<i4"), ("target_lo", "<u4"), ("target_hi", "<u4"),
                  ("diff_mask", "<u4"), ("strand", "S1"), ("pam_index", "i1"), ("mismatches", "u1"), ("reserved", "u1")]

_IUPAC_COMPLEMENT = str.maketrans("ACGTUMRWSYKVHDBN", "TGCAAKYWSRMBDHVN")


def iupac_revcomp(motif):
    """The reverse complement of an IUPAC string, upper case."""
    return motif.upper().translate(_IUPAC_COMPLEMENT)[::-1]


class SiteFilter:
    """calitas_site_filter_t: which sites of a pattern are guides worth ordering, decided on the protospacer as it reads on the site's
    strand.  gc_min / gc_max: bounds on the NUMBER of G and C (SiteFilter.percent turns percentages into them; a gc_max above the
    length means the length); max_run: the longest run allowed, an int for all four bases, or a dict by base / a 4-sequence in ACGT order
    (0: no limit); avoid: IUPAC motifs (at most 8, 1 .. 16 letters) none of which may occur -- in the orientation given: add
    iupac_revcomp(m) to avoid both."""

    def __init__(self, gc_min=0, gc_max=255, max_run=0, avoid=()):
        self.gc_min, self.gc_max = int(gc_min), int(gc_max)
        if isinstance(max_run, dict):
            unknown = set(k.upper() for k in max_run) - set("ACGT")
            if unknown:
                raise ValueError("max_run: not a base: %s" % ", ".join(sorted(unknown)))
            upper = {k.upper(): v for k, v in max_run.items()}
            self.max_run = tuple(int(upper.get(b, 0)) for b in "ACGT")
        elif isinstance(max_run, int):
            self.max_run = (max_run,) * 4
        else:
            self.max_run = tuple(int(x) for x in max_run)
            if len(self.max_run) != 4:
                raise ValueError("max_run: four limits, for A C G T")
        self.avoid = (avoid,) if isinstance(avoid, str) else tuple(avoid)
        for v in (self.gc_min, self.gc_max) + self.max_run:
            if not 0 <= v <= 255:
                raise ValueError("a site filter's numbers are 0 .. 255")

    @staticmethod
    def percent(L, lo, hi):
        """(gc_min, gc_max) for a protospacer of L bases whose G + C share lies in [lo, hi] percent (integers): ceil(lo L / 100),
        floor(hi L / 100)."""
        return -((-int(lo) * L) // 100), (int(hi) * L) // 100

    def to_c(self):
        f = SiteFilterT()                                  # (zeroed)
        f.gc_min, f.gc_max = self.gc_min, self.gc_max
        for i, r in enumerate(self.max_run):
            f.max_run[i] = r
        if len(self.avoid) > 8:
            raise ValueError("a site filter takes at most 8 motifs, not %d" % len(self.avoid))
        f.n_motifs = len(self.avoid)
        for i, m in enumerate(self.avoid):
            raw = m.encode()
            if len(raw) > 16 or b"\0" in raw:
                raise ValueError("a motif of a site filter has at most 16 letters: %s" % m)
            f.motifs[i].value = raw                        # (the library checks the letters)
        return f

    def __repr__(self):
        return "SiteFilter(gc_min=%d, gc_max=%d, max_run=%r, avoid=%r)" % (self.gc_min, self.gc_max, self.max_run, self.avoid)


COUNTS_COLUMNS = ("guide_id", "strand", "guide_mm", "guide_gaps", "pam_mm", "hits")


def counts_of_rows(rows, shape):
    """The table search_counts returns, built from hits.txt rows (read_hits output): cell [s][m][g][p] = rows with strand s ('+' = 0,
    '-' = 1), guide_mm m, guide_gaps g and pam_mm p.  A row outside `shape` = (2, n_mm, n_gaps, n_pam) is an error, never dropped."""
    import numpy as np
    table = np.zeros(shape, dtype=np.uint64)
    for r in rows:
        cell = ({"+": 0, "-": 1}[r["strand"]], int(r["guide_mm"]), int(r["guide_gaps"]), int(r["pam_mm"]))
        if any(not 0 <= c < n for c, n in zip(cell, shape)):
            raise ValueError("a hit at %r lies outside the table's extents %r" % (cell, tuple(shape)))
        table[cell] += 1
    return table


def counts_tsv(guide_id, table):
    """`SearchReference --counts`: header guide_id strand guide_mm guide_gaps pam_mm hits, then the non-zero cells in table order."""
    import numpy as np
    lines = ["\t".join(COUNTS_COLUMNS)]
    for s, m, g, p in np.argwhere(table):                   # (row-major: table order)
        lines.append("%s\t%s\t%d\t%d\t%d\t%d" % (guide_id, "+-"[s], m, g, p, int(table[s, m, g, p])))
    return "\n".join(lines) + "\n"


def read_counts_tsv(path_or_text, shape):
    """A --counts TSV back into the array of that shape."""
    import numpy as np
    text = path_or_text
    if "\n" not in path_or_text:
        with open(path_or_text) as f:
            text = f.read()
    lines = text.splitlines()
    if tuple(lines[0].split("\t")) != COUNTS_COLUMNS:
        raise ValueError("not a counts TSV: %r" % lines[0])
    table = np.zeros(shape, dtype=np.uint64)
    for ln in lines[1:]:
        _, s, m, g, p, n = ln.split("\t")
        table[{"+": 0, "-": 1}[s], int(m), int(g), int(p)] += np.uint64(int(n))
    return table


# ---- the specificity score (include/calitas_hip.h has the contract) ----

SCORES_COLUMNS = ("guide_id", "rows", "perfect", "offtarget_sum_q32", "max_q32", "specificity")
Q16_ONE = 65536
_LETTER = {"A": 0, "C": 1, "G": 2, "T": 3}
_MODEL_LETTERS = "ACGT"


def _q16(x):
    """A decimal of a model file in [0, 1] as Q16: floor(x * 65536 + 0.5) in double."""
    import math
    v = float(x)
    if not 0.0 <= v <= 1.0:
        raise ValueError("a factor of a score model lies in [0, 1], not %r" % (x,))
    return int(math.floor(v * 65536.0 + 0.5))


class ScoreModel:
    """The weights of a specificity score for protospacers of L bases, all Q16 (65536 = 1.0, none above it): mismatch[L][5][5] by guide
    position (0-based, the upper-case letters of the guide as written, left to right), guide letter and target letter (A 0, C 1, G 2,
    T 3, anything else 4), one gap factor, one pam_mismatch factor.  The library ships no published table: read() loads any table of
    this product form from a TSV with `#` comments and the lines

        length<TAB>L
        gap<TAB>x
        pam_mismatch<TAB>x
        mismatch<TAB>position (1-based, or *)<TAB>guide_base (A C G T, `other`, or *)<TAB>target_base (likewise)<TAB>x

    where x is a decimal in [0, 1], entries not given are 1.0 and later lines override earlier ones."""

    def __init__(self, L, mismatch, gap=Q16_ONE, pam_mismatch=Q16_ONE):
        import numpy as np
        self.L = int(L)
        self.mismatch = np.ascontiguousarray(mismatch, dtype=np.uint32)
        if self.mismatch.shape != (self.L, 5, 5):
            raise ValueError("mismatch must have shape (L, 5, 5) = (%d, 5, 5), not %r" % (self.L, self.mismatch.shape))
        self.gap, self.pam_mismatch = int(gap), int(pam_mismatch)

    @classmethod
    def uniform(cls, L, mismatch=Q16_ONE, gap=Q16_ONE, pam_mismatch=Q16_ONE):
        """Every mismatch the same factor, whatever the position and the letters."""
        import numpy as np
        return cls(L, np.full((int(L), 5, 5), int(mismatch), dtype=np.uint32), gap, pam_mismatch)

    def to_c(self):
        m = ScoreModelT()
        m.protospacer_length, m.gap, m.pam_mismatch = self.L, self.gap & 0xFFFFFFFF, self.pam_mismatch & 0xFFFFFFFF
        m.mismatch = self.mismatch.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        m._keep = self.mismatch
        return m

    @classmethod
    def read(cls, path):
        import numpy as np
        L, gap, pam, lines = None, Q16_ONE, Q16_ONE, []
        with open(path) as f:
            for ln in f:
                ln = ln.split("#", 1)[0].strip()
                if not ln:
                    continue
                fld = ln.split("\t")
                if fld[0] == "length" and len(fld) == 2:
                    L = int(fld[1])
                elif fld[0] == "gap" and len(fld) == 2:
                    gap = _q16(fld[1])
                elif fld[0] == "pam_mismatch" and len(fld) == 2:
                    pam = _q16(fld[1])
                elif fld[0] == "mismatch" and len(fld) == 5:
                    lines.append(fld[1:])
                else:
                    raise ValueError("%s: not a line of a score model: %r" % (path, ln))
        if L is None or not 1 <= L <= 32:
            raise ValueError("%s: a score model needs a `length` line with 1 <= L <= 32" % path)
        mm = np.full((L, 5, 5), Q16_ONE, dtype=np.uint32)

        def axis(word, n, names):
            if word == "*":
                return range(n)
            if names is None:
                k = int(word) - 1
            else:
                k = 4 if word.lower() == "other" else names.find(word.upper()) if len(word) == 1 else -1
            if not 0 <= k < n:
                raise ValueError("%s: %r is not a position / base of a score model" % (path, word))
            return [k]
        for pos, gb, tb, x in lines:
            v = _q16(x)
            for i in axis(pos, L, None):
                for g in axis(gb, 5, _MODEL_LETTERS):
                    for t in axis(tb, 5, _MODEL_LETTERS):
                        mm[i, g, t] = v
        return cls(L, mm, gap, pam)

    def write(self, path):
        """The model as a file read() gives back exactly: every factor as the shortest decimal that rounds to it."""
        def dec(q):
            for digits in range(1, 12):
                t = "%.*f" % (digits, q / 65536.0)
                if _q16(t) == q:
                    return t
            raise ValueError("factor %r is not a Q16 value in [0, 65536]" % (q,))
        names = list(_MODEL_LETTERS) + ["other"]
        with open(path, "w") as f:
            f.write("# calitas score model: Q16 factors as decimals (x -> floor(x * 65536 + 0.5)); entries not given are 1.0\n")
            f.write("length\t%d\ngap\t%s\npam_mismatch\t%s\n" % (self.L, dec(self.gap), dec(self.pam_mismatch)))
            for i in range(self.L):
                for g in range(5):
                    for t in range(5):
                        if int(self.mismatch[i, g, t]) != Q16_ONE:
                            f.write("mismatch\t%d\t%s\t%s\t%s\n" % (i + 1, names[g], names[t], dec(int(self.mismatch[i, g, t]))))


class Scores:
    """What a guide's hits add up to under a ScoreModel: rows (all hits), perfect (hits with total_mm_plus_gaps == 0: counted, not
    scored), sum_q32 and max_q32 (sum and maximum of the other hits' scores, 2^32 = 1.0) and the table of search_counts."""
    __slots__ = ("rows", "perfect", "sum_q32", "max_q32", "table")

    def __init__(self, rows, perfect, sum_q32, max_q32, table):
        self.rows, self.perfect, self.sum_q32, self.max_q32, self.table = rows, perfect, sum_q32, max_q32, table

    @property
    def offtarget_sum(self):
        return self.sum_q32 / 2.0 ** 32

    @property
    def specificity(self):
        return 2.0 ** 32 / (2.0 ** 32 + self.sum_q32)

    def __add__(self, o):
        """Window ranges, contigs, ranks of one job: everything adds, max_q32 takes the maximum."""
        return Scores(self.rows + o.rows, self.perfect + o.perfect, self.sum_q32 + o.sum_q32, max(self.max_q32, o.max_q32), self.table + o.table)

    def __eq__(self, o):
        import numpy as np
        return (isinstance(o, Scores) and (self.rows, self.perfect, self.sum_q32, self.max_q32) == (o.rows, o.perfect, o.sum_q32, o.max_q32)
                and self.table.shape == o.table.shape and bool(np.array_equal(self.table, o.table)))

    __hash__ = None

    def __repr__(self):
        return "Scores(rows=%d, perfect=%d, sum_q32=%d, max_q32=%d)" % (self.rows, self.perfect, self.sum_q32, self.max_q32)


def score_of_row(row, model):
    """The contract on one hits.txt row (a read_hits dict), in plain Python integers: None for a perfect row, else its score."""
    pg, pa, pt = row["padded_guide"], row["padded_alignment"], row["padded_target"]
    n_upper = sum(1 for c in pg if "A" <= c <= "Z")
    if n_upper != model.L:
        raise ValueError("a row with %d upper-case guide letters cannot be scored by a model of length %d" % (n_upper, model.L))
    if int(row["total_mm_plus_gaps"]) == 0:
        return None
    s, i = 1 << 32, 0
    for g, a, t in zip(pg, pa, pt):
        if not "A" <= g <= "Z":
            continue
        if a == ".":
            s = (s * int(model.mismatch[i, _LETTER.get(g, 4), _LETTER.get(t, 4)])) >> 16
        i += 1
    for _ in range(int(row["guide_gaps"])):
        s = (s * model.gap) >> 16
    for _ in range(int(row["pam_mm"])):
        s = (s * model.pam_mismatch) >> 16
    return s


def near_score(query, target, model):
    """The contract of calitas_score_near on one (query, site key) pair, in plain Python integers: two strings of model.L letters
    A C G T in either case, a U as a T; None at distance 0, else the factors of the differing positions multiplied into 2^32 in
    ascending guide position, truncated by 16 bits at every step."""
    q, t = query.upper().replace("U", "T"), target.upper().replace("U", "T")
    if len(q) != model.L or len(t) != model.L:
        raise ValueError("a pair of %d and %d letters cannot be scored by a model of length %d" % (len(q), len(t), model.L))
    if q == t:
        return None
    s = 1 << 32
    for i, (g, x) in enumerate(zip(q, t)):
        if g != x:
            s = (s * int(model.mismatch[i, _LETTER[g], _LETTER[x]])) >> 16
    return s


class NearScores:
    """What Context.score_near returns for n queries: near (uint64, shape (n, M + 1): count_near's table over the whole protospacer),
    sum_q32 and max_q32 (uint64, shape (n,): sum and maximum of the scores of the sites at d = 1 .. M, 2^32 = 1.0) and specificity
    = 2^32 / (2^32 + sum_q32) as float64."""
    __slots__ = ("near", "sum_q32", "max_q32")

    def __init__(self, near, sum_q32, max_q32):
        self.near, self.sum_q32, self.max_q32 = near, sum_q32, max_q32

    @property
    def specificity(self):
        import numpy as np
        return 2.0 ** 32 / (2.0 ** 32 + self.sum_q32.astype(np.float64))

    def merge(self, *others):
        """The same queries over disjoint contig sets: counts and sums add, the maxima take the maximum."""
        import numpy as np
        near, total, top = self.near.copy(), self.sum_q32.copy(), self.max_q32.copy()
        for o in others:
            if o.near.shape != near.shape:
                raise ValueError("near scores of different queries or max_mismatches do not merge")
            near, total, top = near + o.near, total + o.sum_q32, np.maximum(top, o.max_q32)
        return NearScores(near, total, top)

    def __add__(self, o):
        return self.merge(o)

    def __eq__(self, o):
        import numpy as np
        return (isinstance(o, NearScores) and self.near.shape == o.near.shape and bool(np.array_equal(self.near, o.near)) and
                bool(np.array_equal(self.sum_q32, o.sum_q32)) and bool(np.array_equal(self.max_q32, o.max_q32)))

    __hash__ = None

    def __repr__(self):
        return "NearScores(n=%d, M=%d)" % (self.near.shape[0], self.near.shape[1] - 1)


def near_hits_of(query, sites, max_mismatches, model=None):
    """The contract of calitas_list_near on one query, in plain Python: `sites` is an iterable of (contig_index, protospacer_start,
    strand '+' / '-', pam_index, protospacer as the guide reads it -- letters A C G T in either case, U as T).  Returns the query's
    stretch, whatever its length: a list of dicts with the fields of calitas_near_hit_t (strand as a str, and `target`, the site's
    letters) for the sites within max_mismatches substitutions of the query, ordered by contig_index, protospacer_start, '+' before
    '-'.  score_q32 is near_score's integer, 2^32 at distance 0 and wherever model is None."""
    q = query.upper().replace("U", "T")
    out = []
    for contig, start, strand, pam_index, target in sites:
        t = target.upper().replace("U", "T")
        if len(t) != len(q):
            raise ValueError("a site of %d letters cannot be held against a query of %d" % (len(t), len(q)))
        at = [i for i in range(len(q)) if q[i] != t[i]]
        if len(at) > max_mismatches:
            continue
        score = near_score(q, t, model) if model is not None and at else 1 << 32
        out.append({"score_q32": score, "contig_index": int(contig), "protospacer_start": int(start),
                    "target_lo": sum((_LETTER[c] & 1) << i for i, c in enumerate(t)), "target_hi": sum((_LETTER[c] >> 1) << i for i, c in enumerate(t)),
                    "diff_mask": sum(1 << i for i in at), "strand": strand, "pam_index": int(pam_index), "mismatches": len(at), "reserved": 0,
                    "target": t})
    out.sort(key=lambda h: (h["contig_index"], h["protospacer_start"], h["strand"] != "+"))
    return out


class NearList:
    """What Context.list_near returns for n queries: near (uint64, shape (n, M + 1): count_near's table over the whole protospacer),
    offsets (uint64, n + 1), hits (a numpy array of NEAR_HIT_DTYPE: query i's records are hits[offsets[i]:offsets[i + 1]], ordered by
    contig_index, protospacer_start, '+' before '-'), limit and L, the protospacer's length.  A query whose row of near sums to more
    than limit lists nothing."""
    __slots__ = ("near", "offsets", "hits", "limit", "L")

    def __init__(self, near, offsets, hits, limit, L):
        self.near, self.offsets, self.hits, self.limit, self.L = near, offsets, hits, int(limit), int(L)

    def of(self, i):
        """Query i's records."""
        return self.hits[int(self.offsets[i]):int(self.offsets[i + 1])]

    def listed(self, i):
        """Whether query i's copies are listed: its row of near sums to limit at most."""
        return int(self.near[i].sum()) <= self.limit

    def target(self, hit):
        """The protospacer of a record's site as the guide reads it, lower case where it differs from the query."""
        lo, hi, diff = int(hit["target_lo"]), int(hit["target_hi"]), int(hit["diff_mask"])
        letters = ["ACGT"[((lo >> i) & 1) | (((hi >> i) & 1) << 1)] for i in range(self.L)]
        return "".join(c.lower() if (diff >> i) & 1 else c for i, c in enumerate(letters))

    def merge(self, *others):
        """The same queries and limit over disjoint contig sets: the counts add, a query's stretches concatenate in contig order, and a
        query whose summed counts exceed the limit lists nothing."""
        import numpy as np
        parts = (self,) + others
        near = self.near.copy()
        for o in others:
            if o.near.shape != near.shape or o.limit != self.limit or o.L != self.L:
                raise ValueError("near lists of different queries, max_mismatches or limits do not merge")
            near = near + o.near
        n = near.shape[0]
        offsets = np.zeros(n + 1, dtype=np.uint64)
        stretches = []
        for i in range(n):
            length = 0
            if int(near[i].sum()) <= self.limit:
                both = np.concatenate([p.of(i) for p in parts])
                stretches.append(both[np.argsort(both["contig_index"], kind="stable")])
                length = len(both)
            offsets[i + 1] = offsets[i] + np.uint64(length)
        hits = np.concatenate(stretches) if stretches else np.zeros(0, dtype=NEAR_HIT_DTYPE)
        return NearList(near, offsets, hits, self.limit, self.L)

    def __eq__(self, o):
        import numpy as np
        return (isinstance(o, NearList) and self.limit == o.limit and self.L == o.L and self.near.shape == o.near.shape and bool(np.array_equal(self.near, o.near)) and
                bool(np.array_equal(self.offsets, o.offsets)) and self.hits.tobytes() == o.hits.tobytes())

    __hash__ = None

    def __repr__(self):
        return "NearList(n=%d, M=%d, hits=%d, limit=%d)" % (self.near.shape[0], self.near.shape[1] - 1, len(self.hits), self.limit)


def scores_of_rows(rows, model, shape=None):
    """What search_scores returns, from hits.txt rows (read_hits output): the reference implementation of the contract.  shape: the
    table's extents (as for counts_of_rows); without it the table is a 1-cell array holding the row count."""
    import numpy as np
    perfect, total, top = 0, 0, 0
    for r in rows:
        s = score_of_row(r, model)
        if s is None:
            perfect += 1
        else:
            total += s
            top = max(top, s)
    table = counts_of_rows(rows, shape) if shape is not None else np.array([len(rows)], dtype=np.uint64)
    return Scores(len(rows), perfect, total, top, table)


# calitas_top_hit_t as a numpy record
TOP_DTYPE = [("score_q32", "<u8"), ("contig_index", "<i4"), ("coordinate_start", "<i4"), ("coordinate_end", "<i4"), ("strand", "S1"),
             ("guide_mm", "u1"), ("guide_gaps", "u1"), ("pam_mm", "u1")]

TOP_COLUMNS = ("guide_id", "rank", "chromosome", "coordinate_start", "coordinate_end", "strand", "guide_mm", "guide_gaps", "pam_mm", "score_q32",
               "score")

# A record of a top list: calitas_top_hit_t with the chromosome's name in the place of contig_index.
TopHit = collections.namedtuple("TopHit", ("score_q32", "chromosome", "coordinate_start", "coordinate_end", "strand", "guide_mm",
                                           "guide_gaps", "pam_mm"))


def _top_k(k):
    if not isinstance(k, int) or isinstance(k, bool) or k < 0 or k >= 1 << 32:
        raise ValueError("k of a top call is an integer (1 .. %d)" % _lib.TOP_MAX)
    return k


class Top:
    """What a top call returns: `scores` (the Scores of the same pass), `k` as asked and `hits`, the min(k, rows - perfect)
    highest-scoring imperfect hits as TopHit records, best first; among equal scores the hit whose row comes earlier in hits.txt."""
    __slots__ = ("scores", "k", "hits")

    def __init__(self, scores, k, hits):
        self.scores, self.k, self.hits = scores, k, list(hits)

    def merge(self, *others):
        """Consecutive pieces of one job (window ranges, contigs, ranks) IN THEIR ORDER: the scores add, the lists merge stably by
        score (a piece's records stay in order and come before a later piece's equal scores), cut at k."""
        scores, hits = self.scores, list(self.hits)
        for o in others:
            if o.k != self.k:
                raise ValueError("top lists of different k do not merge")
            scores = scores + o.scores
            hits = hits + list(o.hits)
        hits.sort(key=lambda h: -h.score_q32)               # (stable: the tie rule)
        return Top(scores, self.k, hits[:self.k])

    def __eq__(self, o):
        return isinstance(o, Top) and self.k == o.k and self.hits == o.hits and self.scores == o.scores

    __hash__ = None

    def __repr__(self):
        return "Top(k=%d, n=%d, %r)" % (self.k, len(self.hits), self.scores)


def top_of_rows(rows, model, k, shape=None):
    """What search_top returns, from hits.txt rows (read_hits output) in the text's order: the reference implementation of the
    contract -- score_of_row per row, perfect rows dropped, a stable sort by descending score.  shape: as for scores_of_rows."""
    if not 1 <= k <= _lib.TOP_MAX:
        raise ValueError("k of a top call is 1 .. %d" % _lib.TOP_MAX)
    hits = []
    for r in rows:
        s = score_of_row(r, model)
        if s is None:
            continue
        hits.append(TopHit(s, r["chromosome"], int(r["coordinate_start"]), int(r["coordinate_end"]), r["strand"], int(r["guide_mm"]),
                           int(r["guide_gaps"]), int(r["pam_mm"])))
    hits.sort(key=lambda h: -h.score_q32)
    return Top(scores_of_rows(rows, model, shape), k, hits[:k])


def top_tsv(guide_id, top, class_names=None):
    """`SearchReference --scores MODEL --top K`: header guide_id rank chromosome coordinate_start coordinate_end strand guide_mm
    guide_gaps pam_mm score_q32 score, then one line per record; rank is 1-based, score = score_q32 / 2^32.  class_names (with
    `--regions`): one name per record, a last column `class`."""
    lines = ["\t".join(TOP_COLUMNS + (("class",) if class_names is not None else ()))]
    for i, h in enumerate(top.hits):
        lines.append("%s\t%d\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%.6f" % (guide_id, i + 1, h.chromosome, h.coordinate_start, h.coordinate_end, h.strand,
                                                                         h.guide_mm, h.guide_gaps, h.pam_mm, h.score_q32, h.score_q32 / 2.0 ** 32)
                     + ("\t" + class_names[i] if class_names is not None else ""))
    return "\n".join(lines) + "\n"


REGION_COLUMNS = ("guide_id", "class", "rows", "perfect", "offtarget_sum_q32", "max_q32", "specificity")


def _mask(list_mask):
    if list_mask is None:
        return 0xFFFFFFFF
    if not isinstance(list_mask, int) or isinstance(list_mask, bool) or list_mask < 0 or list_mask >= 1 << 32:
        raise ValueError("list_mask of a regions call is an integer of 32 bits")
    return list_mask


class Regions:
    """A set of annotated intervals: (chromosome, start, end, class_name) tuples, [start, end) 0-based and half-open like BED, in any
    order, overlapping or nested.  The class names take priority in order of first appearance -- classes[0] is "elsewhere" (no
    interval), classes[1] wins over classes[2] where both cover a hit -- and at most 7 are allowed.  intervals: the tuples with the
    class's index in the place of its name."""
    ELSEWHERE = "elsewhere"

    def __init__(self, intervals=(), classes=None):
        self.classes = [self.ELSEWHERE] + [c for c in (classes or [])]
        if len(set(self.classes)) != len(self.classes):
            raise ValueError("class names repeat, or one is the reserved name %r" % self.ELSEWHERE)
        self.intervals = []
        for chrom, start, end, name in intervals:
            if name == self.ELSEWHERE:
                raise ValueError("the class name %r is reserved for hits outside every interval" % self.ELSEWHERE)
            if name not in self.classes:
                self.classes.append(name)
            start, end = int(start), int(end)
            if not 0 <= start < end:
                raise ValueError("interval %s:%d-%d: start >= end (or negative)" % (chrom, start, end))
            self.intervals.append((chrom, start, end, self.classes.index(name)))
        if len(self.classes) > _lib.REGION_CLASSES_MAX:
            raise ValueError("%d class names: at most %d are allowed" % (len(self.classes) - 1, _lib.REGION_CLASSES_MAX - 1))
        if self.intervals and len(self.classes) < 2:
            raise ValueError("no class")

    def mask_of(self, names):
        """The list_mask of these class names (an iterable, or a comma-separated string); "elsewhere" is class 0."""
        if isinstance(names, str):
            names = [n for n in names.split(",") if n]
        mask = 0
        for n in names:
            if n not in self.classes:
                raise ValueError("unknown class %r (the set has %s)" % (n, ", ".join(self.classes)))
            mask |= 1 << self.classes.index(n)
        return mask

    @classmethod
    def read_bed(cls, path, contigs=None):
        """Four columns: chromosome, start, end, class name (further columns are ignored); lines starting with #, track or browser and
        empty lines are skipped.  contigs (name -> length, e.g. of a Context): intervals on a chromosome it lacks are skipped and
        counted on stderr, an interval past its contig's end is an error."""
        import sys
        rows, skipped = [], 0
        with open(path) as f:
            for no, line in enumerate(f, 1):
                line = line.rstrip("\r\n")
                if not line.strip() or line.startswith("#") or line.startswith("track") or line.startswith("browser"):
                    continue
                p = line.split("\t") if "\t" in line else line.split()
                if len(p) < 4:
                    raise ValueError("%s:%d: a regions file has four columns (chromosome, start, end, class)" % (path, no))
                try:
                    a, b = int(p[1]), int(p[2])
                except ValueError:
                    raise ValueError("%s:%d: start and end are integers" % (path, no))
                if contigs is not None and p[0] in contigs and b > contigs[p[0]]:
                    raise ValueError("%s:%d: the interval ends beyond %s (%d bases)" % (path, no, p[0], contigs[p[0]]))
                rows.append((p[0], a, b, p[3]))
        out = cls(rows)                         # (a class keeps its priority even when all its intervals are skipped)
        if contigs is not None:
            kept = [iv for iv in out.intervals if iv[0] in contigs]
            skipped = len(out.intervals) - len(kept)
            out.intervals = kept
        if skipped:
            sys.stderr.write("%d intervals on chromosomes the reference does not have were skipped\n" % skipped)
        return out


class RegionScores:
    """What a regions call returns: `top` (a Top: its scores are the totals, its hits the best k among the classes of the mask),
    `classes` (the names, class 0 = "elsewhere" first), `by_class` (a Scores per class; they add up to top.scores) and `hit_class`
    (the class index of every record of top.hits)."""
    __slots__ = ("top", "classes", "by_class", "hit_class")

    def __init__(self, top, classes, by_class, hit_class):
        self.top, self.classes, self.by_class, self.hit_class = top, list(classes), list(by_class), [int(c) for c in hit_class]

    def merge(self, *others):
        """Consecutive pieces of one job IN THEIR ORDER: by_class adds like Scores, the lists merge like Top's, and a record's class
        travels with it."""
        scores, by_class = self.top.scores, list(self.by_class)
        pairs = list(zip(self.top.hits, self.hit_class))
        for o in others:
            if o.top.k != self.top.k or o.classes != self.classes:
                raise ValueError("pieces of different k or classes do not merge")
            scores = scores + o.top.scores
            by_class = [a + b for a, b in zip(by_class, o.by_class)]
            pairs += list(zip(o.top.hits, o.hit_class))
        pairs.sort(key=lambda p: -p[0].score_q32)            # (stable: the tie rule)
        pairs = pairs[:self.top.k]
        return RegionScores(Top(scores, self.top.k, [p[0] for p in pairs]), self.classes, by_class, [p[1] for p in pairs])

    def __eq__(self, o):
        return (isinstance(o, RegionScores) and self.top == o.top and self.classes == o.classes and self.by_class == o.by_class
                and self.hit_class == o.hit_class)

    __hash__ = None

    def __repr__(self):
        return "RegionScores(%r, %s, hit_class=%r)" % (self.top, ", ".join("%s: %r" % (n, s) for n, s in zip(self.classes, self.by_class)), self.hit_class)


def class_of_row(row, regions, by_chromosome=None):
    """The contract on one hits.txt row: the smallest class index among the raw intervals of the row's chromosome with
    start < coordinate_end and end > coordinate_start; 0 when there is none or the extent is empty.  A plain scan of every interval
    (by_chromosome: the same intervals as lists per chromosome, so that many rows do not each pass over the other chromosomes')."""
    chrom, a, b = row["chromosome"], int(row["coordinate_start"]), int(row["coordinate_end"])
    best = 0
    if a < b:
        for c, s, e, k in (regions.intervals if by_chromosome is None else by_chromosome.get(chrom, ())):
            if c == chrom and s < b and e > a and (best == 0 or k < best):
                best = k
    return best


def site_class_of(site, regions, extent=None):
    """The contract of find_sites_regions on one site, as a plain scan of the raw intervals like class_of_row.  site: a GuideSite, or
    (chromosome, protospacer_start, strand, protospacer_length) with the strand as "+" / "-".  extent: (from, to), positions of the
    protospacer as the guide reads, 0 its 5' base, half-open; None: all of it.  They are the forward bases [p + from, p + to) on '+'
    and [p + L - to, p + L - from) on '-'; the class is the smallest class index among the intervals of the chromosome that overlap
    them, 0 when there is none."""
    if hasattr(site, "protospacer_start"):
        chrom, p, strand = site.chromosome, int(site.protospacer_start), site.strand
        L = sum(1 for ch in site.guide if ch.isupper())
    else:
        chrom, p, strand, L = site[0], int(site[1]), site[2], int(site[3])
    if isinstance(strand, bytes):
        strand = strand.decode()
    a, b = (0, L) if extent is None else (int(extent[0]), int(extent[1]))
    if not 0 <= a < b <= L:
        raise ValueError("extent (%d, %d): 0 <= from < to <= %d, the protospacer's length" % (a, b, L))
    lo, hi = (p + L - b, p + L - a) if strand == "-" else (p + a, p + b)
    best = 0
    for c, s, e, k in regions.intervals:
        if c == chrom and s < hi and e > lo and (best == 0 or k < best):
            best = k
    return best


# calitas_site_pair_t
SITE_PAIR_DTYPE = [("left", "<u4"), ("right", "<u4"), ("distance", "<i4"), ("orientation", "u1"), ("reserved", "u1", (3,))]
PAIR_CODES = ("++", "-+", "+-", "--")          # orientation o: (left is '-') + 2 (right is '-')
PAIR_MAX_DISTANCE = _lib.PAIR_MAX_DISTANCE


class SitePairs:
    """calitas_site_pairs_t: which two sites of a pattern make a pair.  min_distance .. max_distance: the bounds on the distance of
    their cuts, 0 .. PAIR_MAX_DISTANCE.  cut_offset: where a site is cut, a position 0 .. L in the protospacer as the guide reads
    it; None: L - 3, the Cas9 cut, which needs a 3' PAM.  orientations: "out" (the PAMs face outwards: "-+" with a 3' PAM, "+-" with a
    5' PAM -- the paired-nickase layout), "in" (the other of the two), "same" ("++" and "--"), "any", or a list (or comma-separated
    string) of the codes "++", "-+", "+-", "--": the left member's strand, then the right one's.  The names need a pattern with a PAM
    and are translated with its pam_is_five_prime; a PAM-less pattern takes codes only."""

    def __init__(self, min_distance, max_distance, cut_offset=None, orientations="out"):
        self.min_distance, self.max_distance = int(min_distance), int(max_distance)
        self.cut_offset = None if cut_offset is None else int(cut_offset)
        if isinstance(orientations, str):
            orientations = [o for o in orientations.split(",") if o]
        self.orientations = [str(o) for o in orientations]
        if not self.orientations:
            raise ValueError("orientations is empty: out, in, same, any, or codes among ++ -+ +- --")
        for o in self.orientations:
            if o not in ("out", "in", "same", "any") and o not in PAIR_CODES:
                raise ValueError("orientation %r: out, in, same, any, or a code among ++ -+ +- --" % o)

    def cut_of(self, pattern):
        """cut_offset, None resolved on the pattern (a Guide)."""
        if self.cut_offset is not None:
            return self.cut_offset
        if not pattern.pam_is_three_prime:
            raise ValueError("cut_offset is needed: the default, L - 3, is the Cas9 cut of a pattern with a 3' PAM")
        return pattern.protospacer_length - 3

    def mask_of(self, pattern):
        """The orientations as the mask of calitas_site_pairs_t, bit o = PAIR_CODES[o]."""
        mask = 0
        for o in self.orientations:
            if o in PAIR_CODES:
                mask |= 1 << PAIR_CODES.index(o)
            elif not pattern.pams:
                raise ValueError("orientation %r needs a PAM: a pattern without one takes the codes ++ -+ +- --" % o)
            elif o == "any":
                mask |= 15
            elif o == "same":
                mask |= 9
            else:
                mask |= 2 if (o == "out") == pattern.pam_is_three_prime else 4
        return mask

    def name_of(self, orientation, pattern):
        """What the pairs file calls an orientation code 0 .. 3: out / in / same, or the code itself for a PAM-less pattern."""
        if not pattern.pams:
            return PAIR_CODES[orientation]
        if orientation in (0, 3):
            return "same"
        return "out" if (orientation == 1) == pattern.pam_is_three_prime else "in"

    def to_c(self, pattern):
        cut = self.cut_of(pattern)
        if not 0 <= cut < 256:
            raise ValueError("cut_offset %d: a position of the protospacer, 0 .. its length" % cut)
        if not (-(1 << 31) <= self.min_distance < 1 << 31 and -(1 << 31) <= self.max_distance < 1 << 31):
            raise ValueError("the distances of a pair are 0 .. %d" % PAIR_MAX_DISTANCE)
        t = _lib.SitePairsT()
        t.min_distance, t.max_distance, t.cut_offset, t.orientations = self.min_distance, self.max_distance, cut, self.mask_of(pattern)
        return t

    def __repr__(self):
        return "SitePairs(%d, %d, cut_offset=%r, orientations=%r)" % (self.min_distance, self.max_distance, self.cut_offset, ",".join(self.orientations))


def site_cut_of(protospacer_start, strand, L, cut_offset):
    """Where a site is cut: protospacer_start + c on '+', protospacer_start + L - c on '-'."""
    if isinstance(strand, bytes):
        strand = strand.decode()
    return int(protospacer_start) + (L - cut_offset if strand == "-" else cut_offset)


def site_pairs_of(sites, spec, pattern):
    """The contract of find_site_pairs as a plain double loop.  sites: the listing in its order -- records of SITE_DTYPE, or
    (contig, protospacer_start, strand) tuples; spec: a SitePairs; pattern: the Guide (or its string) the sites are of.  Returns the
    pairs as (left, right, distance, orientation) tuples in (i, j) order: two different sites i < j of one contig whose cuts are
    min_distance .. max_distance apart and whose orientation is wanted; the left member has the smaller cut, at equal cuts the
    smaller index."""
    if not isinstance(pattern, Guide):
        pattern = Guide(pattern)
    L, c, mask = pattern.protospacer_length, spec.cut_of(pattern), spec.mask_of(pattern)
    flat = []
    for s in sites:
        contig, p, strand = (s["contig_index"], s["protospacer_start"], s["strand"]) if hasattr(s, "dtype") else (s[0], s[1], s[2])
        if isinstance(strand, bytes):
            strand = strand.decode()
        flat.append((int(contig) if not isinstance(contig, str) else contig, site_cut_of(p, strand, L, c), strand == "-"))
    pairs = []
    for i in range(len(flat)):
        for j in range(i + 1, len(flat)):
            if flat[i][0] != flat[j][0]:
                continue
            d = flat[j][1] - flat[i][1]
            left, right = (j, i) if d < 0 else (i, j)
            if not spec.min_distance <= abs(d) <= spec.max_distance:
                continue
            o = (1 if flat[left][2] else 0) + (2 if flat[right][2] else 0)
            if (mask >> o) & 1:
                pairs.append((left, right, abs(d), o))
    return pairs


# calitas_snv_t and calitas_allele_site_t
SNV_DTYPE = [("contig_index", "<i4"), ("position", "<i4"), ("ref", "S1"), ("alt", "S1"), ("reserved", "<u2")]
ALLELE_SITE_DTYPE = SITE_DTYPE + [("snv_index", "<u4"), ("kind", "u1"), ("other_pam_index", "i1"), ("guide_offset", "i1"), ("reserved", "u1"),
                                  ("guide_lo", "<u4"), ("guide_hi", "<u4")]
ALLELE_KINDS = ("", "alt", "ref", "both")       # kind k: (a site on alt) + 2 (a site on the reference)


def snvs_of(records, ctx):
    """(chrom, pos1, ref, alt) tuples -- chrom a name of ctx's contigs or an index, pos1 1-based as in a VCF, ref None or "" for "not
    checked" -- as an array of SNV_DTYPE."""
    import numpy as np
    out = np.zeros(len(records), dtype=SNV_DTYPE)
    index = {nm: i for i, nm in enumerate(ctx.contig_names)}
    for k, (chrom, pos1, ref, alt) in enumerate(records):
        if isinstance(chrom, str) and chrom not in index:
            raise ValueError("Unknown chromosome: %s" % chrom)
        out[k] = (index[chrom] if isinstance(chrom, str) else int(chrom), int(pos1) - 1, (ref or "").encode(), alt.encode(), 0)
    return out


class AlleleSites:
    """What Context.find_allele_sites returns.  sites: the records (ALLELE_SITE_DTYPE) in (snv_index, protospacer_start, strand) order;
    status: a byte per SNV -- 0 examined, 1 `ref` differs from the reference's base, 2 the reference's base is no A C G T U, 3 `alt`
    is the reference's base; pattern: the Guide."""

    def __init__(self, sites, status, pattern):
        self.sites, self.status, self.pattern = sites, status, pattern

    def __len__(self):
        return len(self.sites)

    def of(self, i):
        """The records of SNV i."""
        import numpy as np
        lo, hi = np.searchsorted(self.sites["snv_index"], [i, i + 1])
        return self.sites[lo:hi]

    def protospacer(self, rec):
        """The protospacer of the record's allele as the guide reads it, from guide_lo / guide_hi."""
        lo, hi = int(rec["guide_lo"]), int(rec["guide_hi"])
        return "".join("ACGT"[((lo >> i) & 1) | (((hi >> i) & 1) << 1)] for i in range(int(rec["protospacer_length"])))

    def guide(self, rec):
        """The `-i` string a search takes for the record: the protospacer of the allele named, the pattern's matched PAM in lower case
        behind it (in front of it for a 5' PAM)."""
        k = int(rec["pam_index"])
        pam = self.pattern.pams[k] if k >= 0 else ""
        proto = self.protospacer(rec)
        return (pam + proto) if self.pattern.pam_is_five_prime else (proto + pam)

    def merge(self, other):
        """This listing followed by `other`, the listing of the SNVs that came behind this one's in one list: other's snv_index moves
        up by this one's number of SNVs."""
        import numpy as np
        moved = other.sites.copy()
        moved["snv_index"] += len(self.status)
        return AlleleSites(np.concatenate([self.sites, moved]), np.concatenate([self.status, other.status]), self.pattern)


def allele_sites_of(contig_seqs, pattern, snvs):
    """The contract of find_allele_sites in plain Python: a letter of a string replaced, every start and PAM tried letter by letter.
    contig_seqs: the contigs' strings; snvs: (contig_index, position0, ref, alt) tuples or records of SNV_DTYPE.  Returns (records,
    status): records as tuples in ALLELE_SITE_DTYPE's field order, status a list."""
    if not isinstance(pattern, Guide):
        pattern = Guide(pattern)
    sets = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "M": "AC", "R": "AG", "W": "AT", "S": "CG", "Y": "CT", "K": "GT", "V": "ACG",
            "H": "ACT", "D": "AGT", "B": "CGT", "N": "ACGT"}
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    L, five, pams = pattern.protospacer_length, pattern.pam_is_five_prime, pattern.pams or [""]

    def site(seq, p, strand):
        """(pam index, footprint lo, hi, pam_start, protospacer as the guide reads) of the first PAM that matches, or None."""
        for k, pam in enumerate(pams):
            pl = len(pam)
            left = five != (strand == "-")
            lo = p - pl if left else p
            hi = lo + L + pl
            if lo < 0 or hi > len(seq):
                continue
            foot = seq[lo:hi].upper().replace("U", "T")
            if any(c not in "ACGT" for c in foot):
                continue
            read = foot if strand == "+" else "".join(comp[c] for c in reversed(foot))
            want = ((pam + pattern.guide) if five else (pattern.guide + pam)).upper()
            if all(r in sets[w] for r, w in zip(read, want)):
                proto = read[pl:] if five else read[:L]
                return k, lo, hi, (lo if left else p + L), proto
        return None

    records, status = [], []
    for i, v in enumerate(snvs):
        ci, pos, ref, alt = (int(v["contig_index"]), int(v["position"]), v["ref"].decode(), v["alt"].decode()) if hasattr(v, "dtype") else v
        seq = contig_seqs[ci]
        letter = lambda c: c.upper().replace("U", "T")
        here = letter(seq[pos])
        if here not in "ACGT":
            status.append(2)
            continue
        if ref and letter(ref) != here:
            status.append(1)
            continue
        if letter(alt) == here:
            status.append(3)
            continue
        status.append(0)
        with_alt = seq[:pos] + letter(alt) + seq[pos + 1:]
        for p in range(pos - 47, pos + 17):
            for strand in "+-":
                on_ref, on_alt = site(seq, p, strand), site(with_alt, p, strand)
                if not any(s is not None and s[1] <= pos < s[2] for s in (on_ref, on_alt)):
                    continue
                kind = (1 if on_alt else 0) + (2 if on_ref else 0)
                k, lo, hi, pam_start, proto = on_alt or on_ref
                bits = ["ACGT".index(c) for c in proto]
                records.append((ci, p, pam_start if pattern.pams else -1, strand.encode(), k if pattern.pams else -1, hi - lo - L, L, i, kind,
                                on_ref[0] if kind == 3 and pattern.pams else -1, (p + L - 1 - pos) if strand == "-" else (pos - p), 0,
                                sum((b & 1) << j for j, b in enumerate(bits)), sum((b >> 1) << j for j, b in enumerate(bits))))
    return records, status


# calitas_base_edit_t and calitas_edit_site_t
EDIT_SITE_DTYPE = SITE_DTYPE + [("snv_index", "<u4"), ("editable", "<u4"), ("guide_lo", "<u4"), ("guide_hi", "<u4")]
_IUPAC_SETS = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "M": "AC", "R": "AG", "W": "AT", "S": "CG", "Y": "CT", "K": "GT", "V": "ACG",
               "H": "ACT", "D": "AGT", "B": "CGT", "N": "ACGT"}


class BaseEdit:
    """A base editor (calitas_base_edit_t): it turns from_base into to_base ("C", "T": a CBE; "A", "G": an ABE; "C", "G": a CGBE) at
    the positions window = (FROM, TO) of the protospacer as the guide reads, 0-based and half-open, where the base 5' of the edited
    one lies in the IUPAC letter `context` ("N": any).  correct=False: install -- the cell carries REF and the edit makes ALT;
    correct=True: the cell carries ALT and the edit makes REF.  max_bystanders=N (0 .. 31): only guides with at most N other
    editable bases in the window; None: no bound."""

    def __init__(self, from_base, to_base, window, context="N", correct=False, max_bystanders=None):
        self.from_base, self.to_base, self.window, self.context = from_base, to_base, (int(window[0]), int(window[1])), context or "N"
        self.correct, self.max_bystanders = bool(correct), max_bystanders

    def to_c(self):
        for name, v in (("from_base", self.from_base), ("to_base", self.to_base), ("context", self.context)):
            if not (isinstance(v, str) and len(v) == 1 and ord(v) < 128):
                raise ValueError("BaseEdit: %s is one letter, not %r" % (name, v))
        if not all(0 <= w <= 255 for w in self.window):
            raise ValueError("BaseEdit: window is (FROM, TO) with 0 <= FROM < TO <= the protospacer's length, not %r" % (self.window,))
        by = _lib.EDIT_NO_BOUND if self.max_bystanders is None else int(self.max_bystanders)
        if not 0 <= by <= 255:
            raise ValueError("BaseEdit: max_bystanders is 0 .. 31 or None, not %r" % (self.max_bystanders,))
        return _lib.BaseEditT(self.from_base.encode(), self.to_base.encode(), self.window[0], self.window[1], self.context.encode(),
                              1 if self.correct else 0, by, 0)


class EditSites:
    """What Context.find_edit_sites returns.  sites: the records (EDIT_SITE_DTYPE) in (snv_index, protospacer_start) order; status: a
    byte per SNV -- 0 examined, 1 `ref` differs from the reference's base, 2 the reference's base is no A C G T U, 3 `alt` is the
    reference's base, 4 the change is not the editor's on either strand, 5 the target's 5' neighbour fails the context; pattern: the
    Guide; edit: the BaseEdit; snvs: the call's SNVs (SNV_DTYPE)."""

    def __init__(self, sites, status, pattern, edit, snvs):
        self.sites, self.status, self.pattern, self.edit, self.snvs = sites, status, pattern, edit, snvs

    def __len__(self):
        return len(self.sites)

    def of(self, i):
        """The records of SNV i."""
        import numpy as np
        lo, hi = np.searchsorted(self.sites["snv_index"], [i, i + 1])
        return self.sites[lo:hi]

    def offset(self, rec):
        """Where the record's SNV is in the protospacer as the guide reads."""
        pos, p = int(self.snvs[int(rec["snv_index"])]["position"]), int(rec["protospacer_start"])
        return (p + int(rec["protospacer_length"]) - 1 - pos) if rec["strand"] == b"-" else (pos - p)

    def bystanders(self, rec):
        """The other editable positions of the record's window, as the guide reads, ascending."""
        o, bits = self.offset(rec), int(rec["editable"])
        return [i for i in range(int(rec["protospacer_length"])) if (bits >> i) & 1 and i != o]

    def protospacer(self, rec):
        """The background allele's protospacer as the guide reads it, from guide_lo / guide_hi."""
        lo, hi = int(rec["guide_lo"]), int(rec["guide_hi"])
        return "".join("ACGT"[((lo >> i) & 1) | (((hi >> i) & 1) << 1)] for i in range(int(rec["protospacer_length"])))

    def guide(self, rec):
        """The `-i` string a search takes for the record: the background allele's protospacer, the pattern's matched PAM in lower
        case behind it (in front of it for a 5' PAM)."""
        k = int(rec["pam_index"])
        pam = self.pattern.pams[k] if k >= 0 else ""
        proto = self.protospacer(rec)
        return (pam + proto) if self.pattern.pam_is_five_prime else (proto + pam)


def edit_sites_of(contig_seqs, pattern, edit, snvs):
    """The contract of find_edit_sites in plain Python: string surgery -- the background contig as a string, the guide as a slice of
    it or of its reverse complement, every start and PAM tried letter by letter.  contig_seqs: the contigs' strings; snvs:
    (contig_index, position0, ref, alt) tuples or records of SNV_DTYPE.  Returns (records, status): records as tuples in
    EDIT_SITE_DTYPE's field order, status a list."""
    if not isinstance(pattern, Guide):
        pattern = Guide(pattern)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    letter = lambda c: c.upper().replace("U", "T")
    L, five, pams = pattern.protospacer_length, pattern.pam_is_five_prime, pattern.pams or [""]
    f, t = letter(edit.from_base), letter(edit.to_base)
    w0, w1 = edit.window
    allowed = _IUPAC_SETS[letter(edit.context)] if edit.context.upper() != "N" else None
    records, status = [], []
    for i, v in enumerate(snvs):
        ci, pos, ref, alt = (int(v["contig_index"]), int(v["position"]), v["ref"].decode(), v["alt"].decode()) if hasattr(v, "dtype") else v
        seq = contig_seqs[ci]
        here = letter(seq[pos])
        if here not in "ACGT":
            status.append(2)
            continue
        if ref and letter(ref) != here:
            status.append(1)
            continue
        if letter(alt) == here:
            status.append(3)
            continue
        b, p_ = (letter(alt), here) if edit.correct else (here, letter(alt))
        if (b, p_) == (f, t):
            strand = "+"
        elif (comp[b], comp[p_]) == (f, t):
            strand = "-"
        else:
            status.append(4)
            continue
        text = seq[:pos] + b + seq[pos + 1:]
        # what the guide's strand shows, 5' to 3': the text, or its reverse complement with every other letter kept as a placeholder
        shown = text.upper().replace("U", "T")
        if strand == "-":
            shown = "".join(comp.get(c, "?") for c in reversed(shown))
        at = pos if strand == "+" else len(seq) - 1 - pos          # the target on that strand
        if allowed is not None and (at == 0 or shown[at - 1] not in allowed):
            status.append(5)
            continue
        status.append(0)
        for q in (range(at - w1 + 1, at - w0 + 1) if strand == "+" else range(at - w0, at - w1, -1)):   # the protospacer's start on the guide's strand
            p = q if strand == "+" else len(seq) - q - L         # ... and its leftmost forward base, ascending either way
            if q < 0 or q + L > len(seq):
                continue
            proto = shown[q:q + L]
            for k, pam in enumerate(pams):
                lo, hi = (q - len(pam), q + L) if five else (q, q + L + len(pam))
                if lo < 0 or hi > len(seq) or any(c not in "ACGT" for c in shown[lo:hi]):
                    continue
                want = ((pam + pattern.guide) if five else (pattern.guide + pam)).upper()
                if all(r in _IUPAC_SETS[w_] for r, w_ in zip(shown[lo:hi], want)):
                    break
            else:
                continue
            editable = [j for j in range(w0, w1) if proto[j] == f and (allowed is None or (q + j > 0 and shown[q + j - 1] in allowed))]
            if at - q not in editable or (edit.max_bystanders is not None and len(editable) - 1 > edit.max_bystanders):
                continue
            pam_q = lo if five else q + L                       # the PAM's first base on the guide's strand
            pam_start = -1 if not pattern.pams else (pam_q if strand == "+" else len(seq) - pam_q - len(pam))
            bits = ["ACGT".index(c) for c in proto]
            records.append((ci, p, pam_start, strand.encode(), k if pattern.pams else -1, len(pam), L, i, sum(1 << j for j in editable),
                            sum((c & 1) << j for j, c in enumerate(bits)), sum((c >> 1) << j for j, c in enumerate(bits))))
    return records, status


def regions_of_rows(rows, model, regions, k, list_mask=None, shape=None):
    """What search_regions returns, from hits.txt rows (read_hits output) in the text's order: the contract in plain Python --
    class_of_row and score_of_row per row, the rows of a class summed by scores_of_rows, and a stable sort by descending score of
    the imperfect rows whose class is in list_mask.  It shares nothing with the library's flattened form."""
    if not 0 <= k <= _lib.TOP_MAX:
        raise ValueError("k of a regions call is 0 .. %d" % _lib.TOP_MAX)
    mask = _mask(list_mask)
    n = len(regions.classes)
    by_chromosome = {}
    for iv in regions.intervals:
        by_chromosome.setdefault(iv[0], []).append(iv)
    cls = [class_of_row(r, regions, by_chromosome) for r in rows]
    by_class = [scores_of_rows([r for r, c in zip(rows, cls) if c == i], model, shape) for i in range(n)]
    hits = []
    for r, c in zip(rows, cls):
        s = score_of_row(r, model)
        if s is None or not (mask >> c) & 1:
            continue
        hits.append((TopHit(s, r["chromosome"], int(r["coordinate_start"]), int(r["coordinate_end"]), r["strand"], int(r["guide_mm"]),
                            int(r["guide_gaps"]), int(r["pam_mm"])), c))
    hits.sort(key=lambda h: -h[0].score_q32)
    hits = hits[:k]
    return RegionScores(Top(scores_of_rows(rows, model, shape), k, [h[0] for h in hits]), regions.classes, by_class, [h[1] for h in hits])


def regions_tsv(guide_id, got):
    """`SearchReference --scores MODEL --regions FILE.bed`: header guide_id class rows perfect offtarget_sum_q32 max_q32 specificity,
    then one line per class in class order ("elsewhere" first)."""
    lines = ["\t".join(REGION_COLUMNS)]
    for name, s in zip(got.classes, got.by_class):
        lines.append("%s\t%s\t%d\t%d\t%d\t%d\t%.6f" % (guide_id, name, s.rows, s.perfect, s.sum_q32, s.max_q32, s.specificity))
    return "\n".join(lines) + "\n"


def scores_tsv(guide_id, scores):
    """`SearchReference --scores MODEL`: header guide_id rows perfect offtarget_sum_q32 max_q32 specificity, then one line."""
    return "\t".join(SCORES_COLUMNS) + "\n" + "%s\t%d\t%d\t%d\t%d\t%.6f\n" % (guide_id, scores.rows, scores.perfect, scores.sum_q32,
                                                                               scores.max_q32, scores.specificity)


def read_hits(path_or_text):
    """Metric.read[ReferenceHit]: list of dicts keyed by column name."""
    text = path_or_text
    if "\n" not in path_or_text:
        with open(path_or_text) as f:
            text = f.read()
    lines = text.splitlines()
    header = lines[0].split("\t")
    return [dict(zip(header, ln.split("\t"))) for ln in lines[1:]]


# ---- the on-target activity score (include/calitas_hip.h has the contract) ----

ACTIVITY_NONE = _lib.ACTIVITY_NONE
ACTIVITY_LINKS = ("identity", "logistic")
_ACTIVITY_DECIMAL = None


def _activity_q16(x):
    """A decimal of an activity model file in [-16, 16] as Q16: floor(x * 65536 + 0.5) in double.  Digits with at most one point and an
    optional sign, nothing else: what both tools read alike."""
    import math
    import re
    global _ACTIVITY_DECIMAL
    if _ACTIVITY_DECIMAL is None:
        _ACTIVITY_DECIMAL = re.compile(r"[+-]?([0-9]+\.?[0-9]*|\.[0-9]+)", re.ASCII)
    if not _ACTIVITY_DECIMAL.fullmatch(x) or not -16.0 <= float(x) <= 16.0:
        raise ValueError("a weight of an activity model is a decimal in [-16, 16], not %r" % (x,))
    return int(math.floor(float(x) * 65536.0 + 0.5))


def _activity_int(x):
    if not (x.isascii() and x.isdigit() and len(x) <= 4):
        raise ValueError("%r is not a number of an activity model" % (x,))
    return int(x)


class ActivityModel:
    """The weights of an on-target activity score (calitas_activity_model_t), all signed Q16 within +-16.0: for protospacers of L bases
    with `up` bases 5' and `down` bases 3' of them as the guide reads (0 .. 16 each; the context has W = up + L + down letters),
    single[W][4] by context position and base (A C G T), pair[W - 1][16] by position i and 4 * base(i) + base(i + 1), gc[L + 1] by the
    protospacer's G + C count, an intercept, and link: "identity" or "logistic" -- how a tool prints the score, nothing else.  The
    library ships no published table: read() loads any table of this additive form from a TSV with `#` comments and the lines

        length<TAB>L
        context<TAB>UP<TAB>DOWN
        link<TAB>identity|logistic
        intercept<TAB>x
        single<TAB>POS<TAB>BASE<TAB>x
        pair<TAB>POS<TAB>BASE<TAB>BASE<TAB>x
        gc<TAB>COUNT<TAB>x

    POS is 1-based in the context as the guide reads (UP + 1 is the protospacer's first base; a pair sits at its first letter's
    position, 1 .. W - 1), COUNT runs 0 .. L, `*` stands for every index; x is a decimal in [-16, 16]; entries not given are 0, later
    lines override earlier ones, a file without a `context` line has no flanks."""

    def __init__(self, L, up, down, single, pair, gc, intercept=0, link="identity"):
        import numpy as np
        self.L, self.up, self.down = int(L), int(up), int(down)
        W = self.W = self.up + self.L + self.down
        self.single = np.ascontiguousarray(single, dtype=np.int32)
        self.pair = np.ascontiguousarray(pair, dtype=np.int32)
        self.gc = np.ascontiguousarray(gc, dtype=np.int32)
        if W < 1 or self.single.shape != (W, 4) or self.pair.shape != (W - 1, 16) or self.gc.shape != (self.L + 1,):
            raise ValueError("an activity model of W = %d letters has single (W, 4), pair (W - 1, 16) and gc (L + 1,), not %r, %r, %r"
                             % (W, self.single.shape, self.pair.shape, self.gc.shape))
        self.intercept = int(intercept)
        if link not in ACTIVITY_LINKS:
            raise ValueError("link is identity or logistic, not %r" % (link,))
        self.link = link

    @classmethod
    def zeros(cls, L, up=0, down=0, link="identity"):
        import numpy as np
        W = int(up) + int(L) + int(down)
        return cls(L, up, down, np.zeros((W, 4), np.int32), np.zeros((max(W - 1, 0), 16), np.int32), np.zeros(int(L) + 1, np.int32), 0, link)

    def __eq__(self, other):
        import numpy as np
        return (isinstance(other, ActivityModel) and (self.L, self.up, self.down, self.intercept, self.link) ==
                (other.L, other.up, other.down, other.intercept, other.link) and np.array_equal(self.single, other.single) and
                np.array_equal(self.pair, other.pair) and np.array_equal(self.gc, other.gc))

    __hash__ = None

    def to_c(self):
        import numpy as np
        m = _lib.ActivityModelT()
        m.protospacer_length, m.up, m.down, m.link, m.intercept = self.L, self.up, self.down, ACTIVITY_LINKS.index(self.link), self.intercept
        pair = self.pair if self.pair.size else np.zeros(16, np.int32)         # (W = 1: no pair, and no NULL table either)
        ptr = ctypes.POINTER(ctypes.c_int32)
        m.single, m.pair, m.gc = self.single.ctypes.data_as(ptr), pair.ctypes.data_as(ptr), self.gc.ctypes.data_as(ptr)
        m._keep = (self.single, pair, self.gc)
        return m

    @classmethod
    def read(cls, path):
        L, up, down, link, intercept, lines = None, 0, 0, "identity", 0, []
        with open(path) as f:
            for ln in f:
                ln = ln.split("#", 1)[0].strip()
                if not ln:
                    continue
                fld = ln.split("\t")
                try:
                    if fld[0] == "length" and len(fld) == 2:
                        L = _activity_int(fld[1])
                    elif fld[0] == "context" and len(fld) == 3:
                        up, down = _activity_int(fld[1]), _activity_int(fld[2])
                    elif fld[0] == "link" and len(fld) == 2 and fld[1] in ACTIVITY_LINKS:
                        link = fld[1]
                    elif fld[0] == "intercept" and len(fld) == 2:
                        intercept = _activity_q16(fld[1])
                    elif (fld[0], len(fld)) in (("single", 4), ("pair", 5), ("gc", 3)):
                        lines.append(fld)
                    else:
                        raise ValueError("not a line of an activity model: %r" % ln)
                except ValueError as e:
                    raise ValueError("%s: %s" % (path, e)) from None
        if L is None or not 1 <= L <= 32:
            raise ValueError("%s: an activity model needs a `length` line with 1 <= L <= 32" % path)
        if up > _lib.ACTIVITY_MAX_FLANK or down > _lib.ACTIVITY_MAX_FLANK:
            raise ValueError("%s: the `context` of an activity model is 0 .. 16 bases on either side" % path)
        model = cls.zeros(L, up, down, link)
        model.intercept = intercept
        W = model.W

        def axis(word, n, names):
            if word == "*":
                return range(n)
            if names is None:
                k = _activity_int(word)
            else:
                k = names.find(word.upper()) if len(word) == 1 else -1
            if not 0 <= k < n:
                raise ValueError("%r is not a position, a count or a base of this activity model" % (word,))
            return [k]
        try:
            for fld in lines:
                v = _activity_q16(fld[-1])
                if fld[0] == "single":
                    for i in axis(fld[1], W + 1, None):
                        for b in axis(fld[2], 4, _MODEL_LETTERS):
                            if i >= 1:
                                model.single[i - 1, b] = v
                            elif fld[1] != "*":
                                raise ValueError("positions of an activity model count from 1")
                elif fld[0] == "pair":
                    for i in axis(fld[1], W, None):
                        for a in axis(fld[2], 4, _MODEL_LETTERS):
                            for b in axis(fld[3], 4, _MODEL_LETTERS):
                                if i >= 1:
                                    model.pair[i - 1, 4 * a + b] = v
                                elif fld[1] != "*":
                                    raise ValueError("positions of an activity model count from 1")
                else:
                    for k in axis(fld[1], L + 1, None):
                        model.gc[k] = v
        except ValueError as e:
            raise ValueError("%s: %s" % (path, e)) from None
        return model

    def write(self, path):
        """The model as a file read() gives back exactly: every weight as the shortest decimal that rounds to it."""
        def dec(q):
            for digits in range(1, 12):
                t = "%.*f" % (digits, q / 65536.0)
                if _activity_q16(t) == q:
                    return t
            raise ValueError("weight %r is not a Q16 value within +-16.0" % (q,))
        with open(path, "w") as f:
            f.write("# calitas activity model: signed Q16 weights as decimals (x -> floor(x * 65536 + 0.5)); entries not given are 0\n")
            f.write("length\t%d\ncontext\t%d\t%d\nlink\t%s\nintercept\t%s\n" % (self.L, self.up, self.down, self.link, dec(self.intercept)))
            for i in range(self.W):
                for b in range(4):
                    if int(self.single[i, b]):
                        f.write("single\t%d\t%s\t%s\n" % (i + 1, _MODEL_LETTERS[b], dec(int(self.single[i, b]))))
            for i in range(self.W - 1):
                for ab in range(16):
                    if int(self.pair[i, ab]):
                        f.write("pair\t%d\t%s\t%s\t%s\n" % (i + 1, _MODEL_LETTERS[ab >> 2], _MODEL_LETTERS[ab & 3], dec(int(self.pair[i, ab]))))
            for k in range(self.L + 1):
                if int(self.gc[k]):
                    f.write("gc\t%d\t%s\n" % (k, dec(int(self.gc[k]))))


def activity_of(context, model):
    """The contract of calitas_find_sites_scored on one context -- W letters as the guide reads, `up` before the protospacer and `down`
    behind it -- in plain Python integers; None when a letter is not one of A C G T U (either case)."""
    if len(context) != model.W:
        raise ValueError("the context has %d letters, the model's has %d" % (len(context), model.W))
    codes = [_LETTER.get(ch, -1) for ch in context.upper().replace("U", "T")]
    if min(codes) < 0:
        return None
    total = model.intercept
    for i, c in enumerate(codes):
        total += int(model.single[i, c])
    for i in range(model.W - 1):
        total += int(model.pair[i, 4 * codes[i] + codes[i + 1]])
    return total + int(model.gc[sum(1 for c in codes[model.up:model.up + model.L] if c in (1, 2))])


def activity_value(score_q16, model):
    """The number a tool prints for a score: score / 65536 under link identity, 1 / (1 + exp(-score / 65536)) under logistic, in
    double; None for ACTIVITY_NONE or None."""
    import math
    if score_q16 is None or int(score_q16) == ACTIVITY_NONE:
        return None
    x = int(score_q16) / 65536.0
    return x if model.link == "identity" else 1.0 / (1.0 + math.exp(-x))


# ---- the microhomology score (include/calitas_hip.h has the contract) ----

MH_NONE = _lib.MH_NONE
MH_SCORE_DTYPE = [("total_q16", "<u4"), ("out_of_frame_q16", "<u4")]
_MH_DECIMAL = None


def _mh_q16(x):
    """A decimal of a microhomology model file in [0, 1] as Q16: floor(x * 65536 + 0.5) in double.  Digits with at most one point,
    nothing else: what both tools read alike."""
    import math
    import re
    global _MH_DECIMAL
    if _MH_DECIMAL is None:
        _MH_DECIMAL = re.compile(r"([0-9]+\.?[0-9]*|\.[0-9]+)", re.ASCII)
    if not _MH_DECIMAL.fullmatch(x) or not 0.0 <= float(x) <= 1.0:
        raise ValueError("a weight of a microhomology model is a decimal in [0, 1], not %r" % (x,))
    return int(math.floor(float(x) * 65536.0 + 0.5))


def _mh_int(x):
    if not (x.isascii() and x.isdigit() and len(x) <= 4):
        raise ValueError("%r is not a number of a microhomology model" % (x,))
    return int(x)


class MicrohomologyModel:
    """The weights of a microhomology score (calitas_mh_model_t without its cut): a window of `left` bases 5' and `right` bases 3' of the
    cut as the guide reads (1 .. 32 each; W = left + right), min_length (2 .. 8), the shortest run that counts, and weight[W - 1],
    unsigned Q16 values of at most 65536 by deletion length d - 1.  The library ships no published table: exponential() gives the
    published shape exp(-d / tau), read() loads any table from a TSV with `#` comments and the lines

        window<TAB>LEFT<TAB>RIGHT
        min_length<TAB>N
        weight<TAB>DEL<TAB>x

    DEL is a deletion length 1 .. W - 1 or `*` for every one; x is a decimal in [0, 1], converted as floor(x * 65536 + 0.5); entries not
    given are 0, later lines override earlier ones, a file without a `min_length` line has 2."""

    def __init__(self, left, right, weight, min_length=2):
        import numpy as np
        self.left, self.right, self.min_length = int(left), int(right), int(min_length)
        self.W = self.left + self.right
        self.weight = np.ascontiguousarray(weight, dtype=np.uint32)
        if self.W < 2 or self.weight.shape != (self.W - 1,):
            raise ValueError("a microhomology model of W = %d letters has W - 1 weights, not %r" % (self.W, self.weight.shape))

    @classmethod
    def exponential(cls, tau, left, right, min_length=2):
        """weight[d - 1] = floor(exp(-d / tau) * 65536 + 0.5), d = 1 .. left + right - 1."""
        import math
        return cls(left, right, [int(math.floor(math.exp(-d / float(tau)) * 65536.0 + 0.5)) for d in range(1, int(left) + int(right))], min_length)

    def __eq__(self, other):
        import numpy as np
        return (isinstance(other, MicrohomologyModel) and (self.left, self.right, self.min_length) == (other.left, other.right, other.min_length)
                and np.array_equal(self.weight, other.weight))

    __hash__ = None

    def to_c(self, cut_offset):
        m = _lib.MhModelT()
        m.left, m.right, m.cut_offset, m.min_length = self.left, self.right, int(cut_offset), self.min_length
        m.weight = self.weight.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        m._keep = self.weight
        return m

    @classmethod
    def read(cls, path):
        import numpy as np
        window, min_length, lines = None, 2, []
        with open(path) as f:
            for ln in f:
                ln = ln.split("#", 1)[0].strip()
                if not ln:
                    continue
                fld = ln.split("\t")
                try:
                    if fld[0] == "window" and len(fld) == 3:
                        window = (_mh_int(fld[1]), _mh_int(fld[2]))
                    elif fld[0] == "min_length" and len(fld) == 2:
                        min_length = _mh_int(fld[1])
                    elif fld[0] == "weight" and len(fld) == 3:
                        lines.append(fld)
                    else:
                        raise ValueError("not a line of a microhomology model: %r" % ln)
                except ValueError as e:
                    raise ValueError("%s: %s" % (path, e)) from None
        if window is None or not (1 <= window[0] <= _lib.MH_MAX_SIDE and 1 <= window[1] <= _lib.MH_MAX_SIDE):
            raise ValueError("%s: a microhomology model needs a `window` line with 1 .. 32 bases on either side" % path)
        if not 2 <= min_length <= 8:
            raise ValueError("%s: the `min_length` of a microhomology model is 2 .. 8" % path)
        W = window[0] + window[1]
        weight = np.zeros(W - 1, np.uint32)
        try:
            for fld in lines:
                v = _mh_q16(fld[2])
                if fld[1] == "*":
                    weight[:] = v
                    continue
                d = _mh_int(fld[1])
                if not 1 <= d <= W - 1:
                    raise ValueError("%r is not a deletion length of this microhomology model" % (fld[1],))
                weight[d - 1] = v
        except ValueError as e:
            raise ValueError("%s: %s" % (path, e)) from None
        return cls(window[0], window[1], weight, min_length)

    def write(self, path):
        """The model as a file read() gives back exactly: every weight as the shortest decimal that rounds to it."""
        def dec(q):
            for digits in range(1, 12):
                t = "%.*f" % (digits, q / 65536.0)
                if _mh_q16(t) == q:
                    return t
            raise ValueError("weight %r is not a Q16 value within [0, 1]" % (q,))
        with open(path, "w") as f:
            f.write("# calitas microhomology model: unsigned Q16 weights by deletion length as decimals (x -> floor(x * 65536 + 0.5)); entries not given are 0\n")
            f.write("window\t%d\t%d\nmin_length\t%d\n" % (self.left, self.right, self.min_length))
            for d in range(1, self.W):
                if int(self.weight[d - 1]):
                    f.write("weight\t%d\t%s\n" % (d, dec(int(self.weight[d - 1]))))


def microhomology_of(window, left, model):
    """The contract of calitas_find_sites_microhomology on one window -- W letters as the guide reads, `left` of them before the cut -- in
    plain Python integers: (total_q16, out_of_frame_q16), or None when a letter is not one of A C G T U (either case).  A plain walk
    along every diagonal; nothing of the library is called."""
    left = int(left)
    W = len(window)
    if W != model.W or left != model.left:
        raise ValueError("the window has %d letters, %d before the cut; the model's has %d and %d" % (W, left, model.W, model.left))
    x = window.upper().replace("U", "T")
    if any(ch not in "ACGT" for ch in x):
        return None
    total = oof = 0
    for d in range(1, W):
        lo, hi = max(0, left - d), min(left, W - d)
        units = k = g = 0
        for i in range(lo, hi + 1):
            if i < hi and x[i] == x[i + d]:
                k += 1
                g += x[i] in "GC"
                continue
            if k >= model.min_length:
                units += k + g
            k = g = 0
        term = int(model.weight[d - 1]) * units
        total += term
        if d % 3:
            oof += term
    return total, oof
