// variants_rows.cpp -- the text of the variant branch: the 34-column row of a hit of a variant window (make_row: RH:210-254 with
// window-local flanks SR:598-613 and the variant columns RH:211-233), and the rows of a contig's entries as the device's row stage
// takes them (make_rows / rows_of, and the rows_for / fill callbacks of HitsExt that the helper and the filler thread call).
#include <algorithm>
#include <cmath>

#include "variants_internal.hpp"

namespace calitas __attribute__((visibility("hidden"))) {

static std::string format_metric_double(double d) {          // fgbio Metric.formatValue(Double), as variants.py states it
  char b[64];
  auto strip = [](std::string s) {
    while (!s.empty() && s.back() == '0') s.pop_back();
    if (!s.empty() && s.back() == '.') s.pop_back();
    return s;
  };
  if (d == 0) return "0";
  if (std::fabs(d) < 0.00001) {
    const int ex = (int)std::floor(std::log10(std::fabs(d)));
    std::snprintf(b, sizeof b, "%.5f", d / std::pow(10.0, ex));
    return strip(b) + "E" + std::to_string(ex);
  }
  std::snprintf(b, sizeof b, "%.6f", d);
  return strip(b);
}

std::string display_string(const Allele& a) {         // VariantAllele.displayString SR:108
  char b[64];
  std::snprintf(b, sizeof b, ":%d:", a.v->pos - 1);
  std::string s = (a.v->id.empty() ? std::string(".") : a.v->id) + b + a.v->ref + ">" + a.v->alts[a.alt];
  std::snprintf(b, sizeof b, ":%.3f", (double)a.af);
  return s + b;
}

static std::string revcomp(const std::string& s) { return revcomp_str(s); }

static int ga_count(const char* pg, const char* pa, int len, bool lower, bool both_sides, bool mms, bool gaps) {   // GA:139-163
  auto is_lower = [](char c) { return c >= 'a' && c <= 'z'; };
  auto is_letter = [](char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); };
  int n = 0;
  for (int i = 0; i < len; i++) {
    if (mms && pa[i] == '.' && is_lower(pg[i]) == lower) { n++; continue; }
    if (!(gaps && pa[i] == '~')) continue;
    const char gb = pg[i];
    bool me = gb != '-' && is_lower(gb) == lower;
    if (!me) {
      int pi = i; while (pi > 0 && pg[pi] == '-') pi--;
      int ni = i; while (ni < len - 1 && pg[ni] == '-') ni++;
      const char prev = pg[pi], next = pg[ni];
      if (both_sides) me = (prev == '-' || is_lower(prev) == lower) && (next == '-' || is_lower(next) == lower);
      else me = (is_letter(prev) && is_lower(prev) == lower) || (is_letter(next) && is_lower(next) == lower);
    }
    if (me) n++;
  }
  return n;
}

static std::string fetch_ref(const PackedRef& ref, int ci, long s1, long e1, bool minus) {   // fetchBases RH:261-266, 1-based closed
  const long clen = (long)ref.contigs[ci].len;
  const long as = std::max(1L, s1), ae = std::min(clen, e1);
  std::string b((size_t)std::max(0L, as - s1), 'N');
  for (long q = as; q <= ae; q++) b += ref.base_upper(ref.contigs[ci].gbase + (uint64_t)(q - 1));
  b.append((size_t)std::max(0L, e1 - ae), 'N');
  return minus ? revcomp(b) : b;
}

void make_row(const RowInputs& in, const ExtHit& h, const std::string& vid_text, std::string& row, bool compact, uint32_t* vid_at) {
  const PackedRef& ref = in.ref;
  const GuideHost& gh = in.gh;
  const std::string& gid = in.gid;
  const RowStrings& rs = in.rs;
  if (vid_at) *vid_at = 0;
  const Window& w = *h.w;
  const calitas_aln_t& a = *h.a;
  const int wl = w.len;
  const int gs = a.guide_start_offset, ge = a.guide_end_offset, as = a.start_offset, ae = a.end_offset;   // window-local
  int start = 0, end = 0, gstart = 0, gend = 0;
  (void)lift(w, a, start, end, gstart, gend);                                                 // (succeeded when the hit was keyed)
  auto flank = [&](int from, int to, bool have) { return have ? std::string(w.bases + from, (size_t)(to - from)) : std::string(); };
  const bool minus = a.strand == '-';
  const bool h_l10 = gs >= 10, h_r10 = wl - ge >= 10, h_l8 = as >= 8, h_r8 = wl - ae >= 8;
  std::string l10 = flank(gs - 10, gs, h_l10), r10 = flank(ge, ge + 10, h_r10), l8 = flank(as - 8, as, h_l8), r8 = flank(ae, ae + 8, h_r8);
  bool v_l10 = h_l10, v_r10 = h_r10, v_l8 = h_l8, v_r8 = h_r8;
  if (minus) {
    std::string t10 = l10, t8 = l8;
    l10 = h_r10 ? revcomp(r10) : std::string(); r10 = h_l10 ? revcomp(t10) : std::string();
    l8 = h_r8 ? revcomp(r8) : std::string();   r8 = h_l8 ? revcomp(t8) : std::string();
    v_l10 = h_r10; v_r10 = h_l10; v_l8 = h_r8; v_r8 = h_l8;
  }
  auto ten_left = [&] { return fetch_ref(ref, w.contig, gstart + 1 - 10, gstart, minus); };
  auto ten_right = [&] { return fetch_ref(ref, w.contig, gend + 1, gend + 10, minus); };
  auto eight_left = [&] { return fetch_ref(ref, w.contig, start + 1 - 8, start, minus); };
  auto eight_right = [&] { return fetch_ref(ref, w.contig, end + 1, end + 8, minus); };
  const std::string c5_10 = v_l10 ? l10 : (!minus ? ten_left() : ten_right());
  const std::string c3_10 = v_r10 ? r10 : (!minus ? ten_right() : ten_left());
  const std::string c5_8 = v_l8 ? l8 : (!minus ? eight_left() : eight_right());
  const std::string c3_8 = v_r8 ? r8 : (!minus ? eight_right() : eight_left());
  // padded strings from the window's own bases (SGA:511; '-' strand: revcomp of the window span)
  const std::string& q = rs.query[a.pam_index + 1];
  // (two million rows per call at full size: the pieces of a row are put together in buffers on the stack, not in strings of their own)
  char t[CALITAS_MAX_OPS + 8];
  {
    const int tl = std::min(ae - as, (int)CALITAS_MAX_OPS);
    if (!minus) std::memcpy(t, w.bases + as, (size_t)tl);
    else for (int i = 0; i < tl; i++) t[i] = complement_base(w.bases[ae - 1 - i]);
  }
  const int n_ops = a.n_ops;
  char pg[CALITAS_MAX_OPS + 1], pa[CALITAS_MAX_OPS + 1], pt[CALITAS_MAX_OPS + 1];
  size_t qi = 0, ti = 0;
  int mm = 0, gp = 0;
  for (int i = 0; i < n_ops; i++) {
    switch (a.ops[i]) {
      case 'I': pg[i] = q[qi++]; pa[i] = '~'; pt[i] = '-'; gp++; break;
      case 'D': pg[i] = '-'; pa[i] = '~'; pt[i] = t[ti++]; gp++; break;
      case '=': pg[i] = q[qi++]; pa[i] = '|'; pt[i] = t[ti++]; break;
      default:  pg[i] = q[qi++]; pa[i] = '.'; pt[i] = t[ti++]; mm++; break;
    }
  }
  int ps = -1, pe = -1;                                                                       // GA:111-115
  for (int i = 0; i < n_ops; i++) if (pg[i] >= 'A' && pg[i] <= 'Z') { if (ps < 0) ps = i; pe = i; }
  char unpadded_target[CALITAS_MAX_OPS + 1];
  size_t n_unpadded = 0;
  for (int i = ps; i >= 0 && i <= pe; i++) if (pt[i] != '-') unpadded_target[n_unpadded++] = pt[i];
  // variants under the hit (RH:211) and their columns (RH:211-233)
  const Allele* vs_few[8];
  std::vector<const Allele*> vs_many;
  size_t n_vs = 0;
  for_variants_under(w, start, end, [&](const Allele& al) {
    if (n_vs < 8) vs_few[n_vs] = &al;
    else { if (n_vs == 8) vs_many.assign(vs_few, vs_few + 8); vs_many.push_back(&al); }
    n_vs++;
  });
  const Allele* const* vs_p = n_vs <= 8 ? vs_few : vs_many.data();
  struct VsView { const Allele* const* p; size_t n; bool empty() const { return n == 0; } size_t size() const { return n; }
                  const Allele* operator[](size_t i) const { return p[i]; } const Allele* const* begin() const { return p; } const Allele* const* end() const { return p + n; } };
  const VsView vs{vs_p, n_vs};
  std::string ids, descs, af;
  if (!vs.empty()) {
    const Allele* mn = vs[0];
    for (const Allele* al : vs) if (al->af < mn->af) mn = al;                                 // minBy keeps the first minimum
    af = format_metric_double((double)mn->af);
    for (size_t i = 0; i < vs.size(); i++) { if (i) { ids += ';'; descs += ';'; } ids += vs[i]->v->id; descs += display_string(*vs[i]); }
  }
  const int gmm = ga_count(pg, pa, n_ops, false, false, true, false), ggp = ga_count(pg, pa, n_ops, false, false, false, true);
  char cigar[4 * CALITAS_MAX_OPS + 8];
  size_t n_cigar = 0;
  auto put_int = [](char* at, long v) -> size_t {            // decimal digits of v at `at`; returns how many
    char d[24]; int nd = 0; const bool neg = v < 0; unsigned long u = neg ? (unsigned long)(-v) : (unsigned long)v;
    do { d[nd++] = (char)('0' + u % 10); u /= 10; } while (u);
    size_t k = 0;
    if (neg) at[k++] = '-';
    while (nd) at[k++] = d[--nd];
    return k;
  };
  for (int i = 0; i < n_ops;) { int j = i; while (j < n_ops && a.ops[j] == a.ops[i]) j++; n_cigar += put_int(cigar + n_cigar, j - i); cigar[n_cigar++] = (char)a.ops[i]; i = j; }
  // the row is put together in place: room for the longest it can be, one pointer walking through it (sixty appends to a string,
  // each with its capacity check, were a microsecond per row -- two seconds of the workers' time per call at full size)
  const size_t row_at = row.size();                                                           // (appends to what is there)
  const std::string& build = vs.empty() ? ref.genome_build : in.build_with_variants;
  const std::string& pam_used = rs.pam_used[a.pam_index + 1];
  const size_t room = gid.size() + gh.protospacer.size() + build.size() + ref.names[w.contig].size() + n_unpadded + c5_10.size() + c3_10.size() +
                      pam_used.size() + ids.size() + descs.size() + vid_text.size() + af.size() + 3 * (size_t)n_ops + c5_8.size() + c3_8.size() + n_cigar +
                      rs.proto_len.size() + rs.tail.size() + 9 * 24 + 40;
  row.resize(row_at + room);
  char* wp = &row[row_at];
  auto add = [&](const std::string& s) { std::memcpy(wp, s.data(), s.size()); wp += s.size(); *wp++ = '\t'; };
  auto add_mem = [&](const char* m, size_t len) { std::memcpy(wp, m, len); wp += len; *wp++ = '\t'; };
  auto add_int = [&](long v) { wp += put_int(wp, v); *wp++ = '\t'; };
  if (!compact) { add(gid); add(gh.protospacer); }
  add(build); add(ref.names[w.contig]);
  add_int(gstart); add_int(gend); *wp++ = (char)a.strand; *wp++ = '\t'; add_mem(unpadded_target, n_unpadded);
  add(c5_10); add(c3_10); add(pam_used); add(ids); add(descs); if (vs.empty()) *wp++ = '\t'; else { if (vid_at) *vid_at = (uint32_t)(wp - &row[row_at]); add(vid_text); } add(af);
  add_int(a.score); add_int(gmm); add_int(ggp); add_int(gmm + ggp);
  add_int(ga_count(pg, pa, n_ops, true, true, true, false)); add_int(mm + gp);
  add_mem(pg, (size_t)n_ops); add_mem(pa, (size_t)n_ops); add_mem(pt, (size_t)n_ops);
  add(c5_8); add(c3_8); add_mem(cigar, n_cigar); add(rs.proto_len); add_int((long)n_unpadded);
  if (!compact) { std::memcpy(wp, rs.tail.data(), rs.tail.size()); wp += rs.tail.size(); }   // aligner .. time_stamp + '\n'
  else *wp++ = '\n';                                       // (the compact tail; the cell before it keeps its tab: the full tail starts with the next field)
  if (wp > &row[row_at] && wp[-1] == '\n') wp--;
  row.resize((size_t)(wp - row.data()));
}

// ---- the rows of a contig's entries ---------------------------------------------------------------------------------------------------
// Rows on demand (hits.hpp, HitsExt::rows_for): an entry's row is made when the device's walk has kept it -- one in ten at BASELINE config
// 5's size; the rows of all two million entries were 0.37-0.42 s of the lifter thread's 0.7 s per call, and 1.1 GB on their way to the
// device.  And the rows of the entries the device keeps never go to the device: the rows kernel leaves holes, the host fills them once
// the text is there (HitsExtRows::fill_on_host).  Compact rows (CALITAS_VARIANTS_COMPACT) send the kept rows up instead and the rows
// kernel copies them -- a hole's place is known in the text the device wrote.

// The rows of contig c's entries [lo, hi) -- of those with kept[i] != 0, or of all (kept null) -- as consecutive blocks of entries, each
// written into a buffer of its own (segs) by whichever worker takes it next (the entries with variants stand at the end of the order and
// their rows cost 2.5 times a plain one: equal shares per worker left seven workers with all of them, 25 ms against 10 per contig); the
// device takes the buffers piece by piece.  x.row_len[i] = the row's length with its newline, 0 for an entry that is not wanted.
void VariantSearch::make_rows(size_t c, size_t lo, size_t hi, const uint8_t* kept, std::vector<std::string>& segs) {
  ContigExt& x = cx[c];
  const size_t n = hi - lo;
  const size_t T = (size_t)ctx->pool->size();
  const size_t S = std::max<size_t>(1, std::min<size_t>(4 * T, (n + 255) / 256));
  segs.assign(S, std::string());
  if (n == 0) return;
  const std::string& vid_text = fill_on_host ? id.placeholder : id.vid;   // (filled in on the host: the MD5 may not be there yet)
  std::atomic<size_t> next_seg{0};
  ctx->pool->run([&](int) {
    for (;;) {
      const size_t sg = next_seg.fetch_add(1, std::memory_order_relaxed);
      if (sg >= S) return;
      const size_t b = lo + n * sg / S, e = lo + n * (sg + 1) / S;
      size_t wanted = e - b;
      if (kept) { wanted = 0; for (size_t i = b; i < e; i++) wanted += kept[i] != 0; }
      if (!wanted) continue;
      std::string& buf = segs[sg];
      buf.reserve(wanted * 700 + 2048);                        // (+ the room make_row asks for before it knows the last row's length)
      for (size_t i = b; i < e; i++) {
        if (kept && !kept[i]) continue;
        const size_t at = buf.size();
        make_row(row_in, *x.entry[i], vid_text, buf, source.compact_rows, fill_on_host ? &x.vid_off[i] : nullptr);   // (appends)
        buf += '\n';
        x.row_len[i] = (uint32_t)(buf.size() - at);
      }
      tm.rows_made.fetch_add(wanted, std::memory_order_relaxed);
      if (fill_on_host) {                                      // (the buffer is complete: where each of its rows stands)
        size_t acc = 0;
        for (size_t i = b; i < e; i++) if (x.row_len[i] && (!kept || kept[i])) { x.row_ptr[i] = buf.data() + acc; acc += x.row_len[i]; }
      }
    }
  });
}

// ... and what the device is given: the offsets of all entries' rows in the text that the buffers -- the plain entries', then the placed
// ones' -- make in this order.
int VariantSearch::rows_of(size_t c, HitsExtRows* out) {
  ContigExt& x = cx[c];
  const size_t n = x.entry.size();
  x.row_off.resize(n + 1);
  x.row_off[0] = 0;
  for (size_t i = 0; i < n; i++) x.row_off[i + 1] = x.row_off[i] + x.row_len[i];
  if (fill_on_host) { *out = HitsExtRows(); out->row_off = x.row_off.data(); out->fill_on_host = true; return CALITAS_OK; }
  x.seg_ptr.clear(); x.seg_off.assign(1, 0);
  for (std::vector<std::string>* group : {&x.segs, &x.segs_placed})
    for (const std::string& sg : *group) {
      if (sg.empty()) continue;
      x.seg_ptr.push_back(sg.data());
      x.seg_off.push_back(x.seg_off.back() + sg.size());
    }
  if (x.seg_off.back() != x.row_off[n])
    return calitas_fail(ctx, CALITAS_EINVAL, "the rows of a contig's entries are not where their offsets say (internal error)");
  if (x.seg_ptr.empty()) { x.seg_ptr.push_back(""); x.seg_off.push_back(0); }   // (no row at all: one empty piece)
  out->row_off = x.row_off.data(); out->rows = nullptr;
  out->n_seg = (uint32_t)x.seg_ptr.size(); out->seg = x.seg_ptr.data(); out->seg_off = x.seg_off.data();
  return CALITAS_OK;
}

// The rows of contig c's kept entries into the holes the rows kernel left in `text` (place[i]: where entry i's row belongs, ~0: not
// kept), with the identifier in the placeholder's place.  On the filler thread, or on the helper's copying thread (HitsExt::fill).
int VariantSearch::fill_rows(size_t c, const uint64_t* place, char* text) {
  const auto t_f = Clock::now();
  if (!id.need()) return calitas_fail(ctx, CALITAS_EIO, id.md5_err);
  const std::string& vid = id.vid;
  if (vid.size() != id.placeholder.size()) return calitas_fail(ctx, CALITAS_EINVAL, "the VCF's identifier is not as long as its placeholder (internal error)");
  ContigExt& y = cx[c];
  std::atomic<uint64_t> done{0};
  ctx->pool->for_blocks(y.entry.size(), [&](size_t b, size_t e, int) {
    uint64_t k = 0;
    for (size_t i = b; i < e; i++) {
      if (place[i] == ~0ull) continue;
      if (!y.row_ptr[i]) continue;                       // (counted below: a kept entry without a row is an error)
      char* dst = text + place[i];
      std::memcpy(dst, y.row_ptr[i], y.row_len[i]);
      if (y.vid_off[i]) std::memcpy(dst + y.vid_off[i], vid.data(), vid.size());
      k++;
    }
    done += k;
  });
  uint64_t want = 0;
  for (size_t i = 0; i < y.entry.size(); i++) want += place[i] != ~0ull;
  if (done.load() != want) return calitas_fail(ctx, CALITAS_EINVAL, "an entry the device kept has no row (internal error)");
  tm.rows_filled += want;
  tm.ns_fill += (long long)(ms_since(t_f) * 1e6);
  return CALITAS_OK;
}

// The rows of a finished contig (the finisher stage, behind the lifter: the lifter carried keys, groups and rows one after the other,
// 0.43-0.47 s per call at BASELINE config 5's size, and every other stage of the variant half waited for it).
// The placed entries -- kept by the walks of their own groups, so their rows are wanted whatever the device decides -- get their rows
// now; the plain ones when the device's walk has kept them (next to none: they repeat reference hits), on the helper thread inside the
// contig's row stage.  (The device merge's only: the host merge makes no rows here.)
// The two callbacks left in cx[c].ext hold a pointer to this call.  The helper and the filler call them, and both have been joined or
// drained when the call ends; cx may outlive the call as garbage, whose destruction only drops the callbacks.
int VariantSearch::finish_rows(size_t c) {
  ContigExt& x = cx[c];
  const size_t n = x.entry.size(), n_plain = x.n_plain;
  if (n == 0) return CALITAS_OK;
  const ScopedMs timed{tm.make};
  if (!fill_on_host && !id.need()) return calitas_fail(ctx, CALITAS_EIO, id.md5_err);
  make_rows(c, n_plain, n, nullptr, x.segs_placed);
  // Rows written into the text on the host (hits.hpp, HitsExtRows::fill_on_host): when the text goes to a buffer of the caller's (`stays`)
  // the copying thread of the reference passes only hands the job over -- the filler stage waits for the VCF's MD5 once and fills the holes.
  if (fill_on_host)
    x.ext.fill = [this, c](const uint64_t* place, char* text, bool stays) -> int {
      if (!stays) return fill_rows(c, place, text);
      auto held = std::make_shared<std::vector<uint64_t>>(place, place + cx[c].entry.size());   // (place[] is the device stage's: valid during this call only)
      return filler.enqueue([this, c, text, held](std::string&) -> int { return fill_rows(c, held->data(), text); }, 64, nullptr);
    };
  // (runs on the helper thread; cx[c] is this contig's alone from here on)
  x.ext.rows_for = [this, c, n_plain](const uint8_t* kept, HitsExtRows* out) -> int {
    const auto t_d = Clock::now();
    std::fill(cx[c].row_len.begin(), cx[c].row_len.begin() + (std::ptrdiff_t)n_plain, 0u);   // (a second row stage of the same contig starts afresh)
    make_rows(c, 0, n_plain, kept, cx[c].segs);
    const int r = rows_of(c, out);
    tm.ns_demand += (long long)(ms_since(t_d) * 1e6);
    return r;
  };
  return CALITAS_OK;
}

}  // namespace calitas
