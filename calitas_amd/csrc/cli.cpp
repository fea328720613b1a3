// cli.cpp -- `calitas SearchReference ...` and `calitas FindGuides ...` on the MI355X path: for the first, the flag surface of the reference tool
// (SearchReference.scala:452-470) over the C ABI of include/calitas_hip.h.  The Scala CLI stays the intended host in
// production; this binary is the same host logic for boxes without a JVM.
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/calitas_hip.h"

static void usage() {
  std::fprintf(stderr,
    "usage: calitas SearchReference -i GUIDEpam -I guide-id -r ref.fa [-o hits.txt] [-x aux-pam ...]\n"
    "         [-w window-size=1000] [-d max-guide-diffs=5] [-p max-pam-mismatches=1] [-g max-gaps-between-guide-and-pam=3]\n"
    "         [-D max-total-diffs] [-O max-overlap=10] [-m guide-mismatch-net-cost=-120] [-M pam-mismatch-net-cost=-260]\n"
    "         [-b genome-gap-net-cost=-122] [-B guide-gap-net-cost=-121] [-c chrom] [-t threads (ignored)]\n"
    "         [-v variants.vcf[.gz]] [-V max-variants=16]\n"
    "         [--counts (the table guide_id strand guide_mm guide_gaps pam_mm hits instead of hits.txt)]\n"
    "         [--top K (with --scores: the K highest-scoring imperfect hits behind the scores and an empty line)]\n"
    "         [--regions FILE.bed (with --scores: the scores per class of the four-column BED file behind the scores and an empty line;\n"
    "          the --top lines gain a last column class)] [--top-classes name,... (list only hits of these classes)]\n"
    "         [--scores model.tsv (guide_id rows perfect offtarget_sum_q32 max_q32 specificity instead of hits.txt; with --counts the\n"
    "          table follows behind an empty line)]\n"
    "         [--device N]\n"
    "       calitas FindGuides -i PATTERNpam -r ref.fa [-x aux-pam ...] [-c chrom] [-s start=0] [-e end] [-o guides.tsv]\n"
    "         [--gc-min PCT] [--gc-max PCT (G + C of the protospacer, percent)] [--max-run N | T=3,G=4 (longest run of a base)]\n"
    "         [--avoid MOTIF ... (IUPAC; with its reverse complement, 8 motifs in all)]\n"
    "         [--copies (the column copies: sites of the pattern in the whole reference with the row's protospacer, its own among them)]\n"
    "         [--seed-copies K (the column seed_copies: the same for the PAM-proximal K bases)]\n"
    "         [--max-copies N (drop rows with more; implies --copies)] [--max-seed-copies N (needs --seed-copies)]\n"
    "         [--near-copies M (0 .. 3: the columns copies_mm0 .. copies_mmM, the sites whose protospacer differs at exactly that many positions)]\n"
    "         [--max-near-copies N (drop rows whose copies_mm columns sum to more; needs --near-copies)]\n"
    "         [--near-scores model.tsv (with --near-copies: near_sum_q32 near_max_q32 near_specificity, the near copies' scores from the same pass)]\n"
    "         [--near-list out.tsv (with --near-copies: every kept guide's copies within M substitutions, one per line)] [--near-list-limit N (1 .. 4096, default 1000)]\n"
    "         [--activity model.tsv (the columns activity_q16 and activity: every site's on-target score under the activity model, NA where it has none)]\n"
    "         [--min-activity X (with --activity: drop rows whose LINEAR score is below the decimal X, and those without a score, before any\n"
    "          other flag looks at them; under `link logistic` a probability p is X = ln(p / (1 - p)))]\n"
    "         [--regions file.bed (chromosome start end class: only the sites in the named classes' intervals, and the column class)]\n"
    "         [--classes name,... (with --regions: the classes to keep; elsewhere: outside every interval)]\n"
    "         [--class-extent FROM:TO (with --regions: class these positions of the protospacer as the guide reads, 0-based half-open; default all)]\n"
    "         [--pairs out.tsv (the pairs of the kept guides, one per line) --pair-distance MIN:MAX (of the two cuts, 0 .. 65535)]\n"
    "         [--pair-cut N (with --pairs: the cut's position 0 .. L in the protospacer as the guide reads; default L - 3 with a 3' PAM)]\n"
    "         [--pair-orientation out|in|same|any|CODE,... (with --pairs: default out, the PAMs facing outwards; codes ++ -+ +- --)]\n"
    "         [--alleles FILE.vcf[.gz] --allele-sites out.tsv (the sites each SNV of the region creates, destroys or changes, one per line)]\n"
    "         [--allele-kinds alt,ref,both (with --alleles: the kinds of lines to write; default all three)]\n"
    "         [--alleles FILE.vcf[.gz] --edit-sites out.tsv --editor FROM:TO --edit-window FROM:TO (the guides that put each SNV of the region into the\n"
    "          base editor's window on the strand it can change it on, and their bystanders, one per line; C:T a CBE, A:G an ABE; the window 0-based\n"
    "          half-open in the protospacer as the guide reads)] [--edit-context LETTER (IUPAC: the base 5' of an edited base; default N)]\n"
    "         [--edit-mode install|correct (default install: the cell carries REF)] [--max-bystanders N (0 .. 31)]\n"
    "         [--microhomology model.tsv (the columns mh_total_q16, mh_oof_q16, mh_score and out_of_frame: the microhomology score around every site's\n"
    "          cut and the share of it that shifts the frame, NA where a site has none)] [--mh-cut N (default L - 3 with a 3' PAM, required otherwise)]\n"
    "         [--min-out-of-frame PCT (with --microhomology: drop rows whose out_of_frame is below the integer PCT, 0 .. 100, rows whose total is 0\n"
    "          and rows without a score, before any other flag looks at them)]\n"
    "         [--device N (-1: the host twin, no GPU)]\n");
}

static std::string long_to_short(const std::string& a) {
  static const char* map[][2] = {
    {"--guide", "-i"}, {"--guide-id", "-I"}, {"--auxiliary-pams", "-x"}, {"--ref", "-r"}, {"--variants", "-v"}, {"--max-variants", "-V"},
    {"--output", "-o"}, {"--threads", "-t"}, {"--window-size", "-w"}, {"--max-guide-diffs", "-d"}, {"--max-pam-mismatches", "-p"},
    {"--max-gaps-between-guide-and-pam", "-g"}, {"--max-total-diffs", "-D"}, {"--max-overlap", "-O"},
    {"--guide-mismatch-net-cost", "-m"}, {"--pam-mismatch-net-cost", "-M"}, {"--genome-gap-net-cost", "-b"},
    {"--guide-gap-net-cost", "-B"}, {"--chrom", "-c"}};
  for (auto& m : map) if (a == m[0]) return m[1];
  return a;
}

// Guide.apply(sequence, auxPams): split by case (SequentialGuideAligner.scala:81-107)
struct ParsedGuide {
  std::string proto;
  std::vector<std::string> pams;
  std::vector<const char*> pam_ptrs;
  int pam5 = 0;
  size_t cli_length = 0;
  calitas_guide_t c_guide() {
    pam_ptrs.clear();
    for (auto& s : pams) pam_ptrs.push_back(s.c_str());
    calitas_guide_t g;
    g.protospacer = proto.c_str(); g.n_pams = (int32_t)pams.size(); g.pams = pam_ptrs.empty() ? nullptr : pam_ptrs.data();
    g.pam_is_5prime = pam5; g.cli_length = (int32_t)cli_length;
    return g;
  }
};

static int parse_guide(const std::string& guide, const std::vector<std::string>& aux, ParsedGuide& out) {
  std::vector<std::string> parts;
  for (size_t i = 0; i < guide.size();) {
    bool lower = std::islower((unsigned char)guide[i]) != 0;
    size_t j = i;
    while (j < guide.size() && (std::islower((unsigned char)guide[j]) != 0) == lower) j++;
    parts.push_back(guide.substr(i, j - i));
    i = j;
  }
  if (parts.empty() || parts.size() > 2) { std::fprintf(stderr, "Invalid Guide sequence %s.\n", guide.c_str()); return 1; }
  if (parts.size() == 1 && !std::isupper((unsigned char)parts[0][0])) { std::fprintf(stderr, "Guide sequence cannot be all lower case.\n"); return 1; }
  if (!aux.empty() && parts.size() != 2) { std::fprintf(stderr, "Cannot provide auxiliary PAMs without providing a PAM in the guide sequence.\n"); return 1; }
  for (auto& x : aux) for (char c : x) if (std::isupper((unsigned char)c)) { std::fprintf(stderr, "All PAMs must be lower case.\n"); return 1; }
  if (parts.size() == 1) out.proto = parts[0];
  else if (std::isupper((unsigned char)parts[0][0])) { out.proto = parts[0]; out.pams.push_back(parts[1]); }
  else { out.proto = parts[1]; out.pams.push_back(parts[0]); out.pam5 = 1; }
  for (auto& x : aux) out.pams.push_back(x);
  out.cli_length = guide.size();
  return 0;
}

// A score model file (calitas_amd/aligner.py, ScoreModel.read: the same lines, the same integers -- strtod and Python's float() are both
// correctly rounded): `#` comments, length / gap / pam_mismatch / mismatch lines, `*` for every index, later lines override earlier ones.
struct ScoreModelFile {
  int L = 0;
  uint32_t gap = 65536, pam = 65536;
  std::vector<uint32_t> mm;
};
static bool read_score_model(const std::string& path, ScoreModelFile& out, std::string& err) {
  FILE* f = std::fopen(path.c_str(), "r");
  if (!f) { err = "cannot read " + path; return false; }
  std::vector<std::vector<std::string>> lines;
  char buf[1024];
  auto q16 = [&](const std::string& x, uint32_t* v) {
    char* end = nullptr;
    const double d = std::strtod(x.c_str(), &end);
    if (x.empty() || *end || !(d >= 0.0 && d <= 1.0)) { err = "a factor of a score model lies in [0, 1], not " + x; return false; }
    *v = (uint32_t)std::floor(d * 65536.0 + 0.5);
    return true;
  };
  bool ok = true;
  while (ok && std::fgets(buf, sizeof buf, f)) {
    std::string ln = buf;
    const size_t hash = ln.find('#');
    if (hash != std::string::npos) ln.erase(hash);
    while (!ln.empty() && std::isspace((unsigned char)ln.back())) ln.pop_back();
    size_t b = 0;
    while (b < ln.size() && std::isspace((unsigned char)ln[b])) b++;
    ln.erase(0, b);
    if (ln.empty()) continue;
    std::vector<std::string> fld;
    for (size_t i = 0;;) { const size_t t = ln.find('\t', i); fld.push_back(ln.substr(i, t == std::string::npos ? t : t - i)); if (t == std::string::npos) break; i = t + 1; }
    if (fld[0] == "length" && fld.size() == 2) out.L = std::atoi(fld[1].c_str());
    else if (fld[0] == "gap" && fld.size() == 2) ok = q16(fld[1], &out.gap);
    else if (fld[0] == "pam_mismatch" && fld.size() == 2) ok = q16(fld[1], &out.pam);
    else if (fld[0] == "mismatch" && fld.size() == 5) lines.push_back(fld);
    else { err = path + ": not a line of a score model: " + ln; ok = false; }
  }
  std::fclose(f);
  if (!ok) return false;
  if (out.L < 1 || out.L > 32) { err = path + ": a score model needs a `length` line with 1 <= L <= 32"; return false; }
  out.mm.assign((size_t)out.L * 25, 65536u);
  auto axis = [&](const std::string& w, int n, bool base, int* lo, int* hi) {
    if (w == "*") { *lo = 0; *hi = n; return true; }
    int k = -1;
    if (!base) k = std::atoi(w.c_str()) - 1;
    else if (w == "other" || w == "OTHER" || w == "Other") k = 4;
    else if (w.size() == 1) { const char* at = std::strchr("ACGT", std::toupper((unsigned char)w[0])); k = at && *at ? (int)(at - "ACGT") : -1; }
    if (k < 0 || k >= n) { err = path + ": " + w + " is not a position / base of a score model"; return false; }
    *lo = k; *hi = k + 1;
    return true;
  };
  for (auto& fld : lines) {
    uint32_t v = 0;
    int i0, i1, g0, g1, t0, t1;
    if (!q16(fld[4], &v) || !axis(fld[1], out.L, false, &i0, &i1) || !axis(fld[2], 5, true, &g0, &g1) || !axis(fld[3], 5, true, &t0, &t1)) return false;
    for (int i = i0; i < i1; i++) for (int g = g0; g < g1; g++) for (int t = t0; t < t1; t++) out.mm[(size_t)i * 25 + (size_t)g * 5 + (size_t)t] = v;
  }
  return true;
}

// An activity model file (calitas_amd/aligner.py, ActivityModel.read: the same lines accepted and refused, the same integers): `#`
// comments, length / context / link / intercept / single / pair / gc lines, `*` for every index, later lines override earlier ones.
struct ActivityModelFile {
  int L = 0, up = 0, down = 0, link = 0;
  int32_t intercept = 0;
  std::vector<int32_t> single, pair, gc;
};
// a decimal as both tools read it -- digits, at most one point, an optional sign -- within [-most, most], as Q16
static bool activity_decimal(const std::string& x, double most, int32_t* v) {
  size_t i = (!x.empty() && (x[0] == '+' || x[0] == '-')) ? 1 : 0, digits = 0, points = 0;
  for (size_t k = i; k < x.size(); k++) {
    if (x[k] >= '0' && x[k] <= '9') digits++;
    else if (x[k] == '.' && points == 0) points++;
    else return false;
  }
  if (digits == 0) return false;
  const double d = std::strtod(x.c_str(), nullptr);
  if (!(d >= -most && d <= most)) return false;
  *v = (int32_t)std::floor(d * 65536.0 + 0.5);
  return true;
}
// a number of at most four digits, nothing else
static bool activity_int(const std::string& x, int* v) {
  if (x.empty() || x.size() > 4 || x.find_first_not_of("0123456789") != std::string::npos) return false;
  *v = std::atoi(x.c_str());
  return true;
}
static bool read_activity_model(const std::string& path, ActivityModelFile& out, std::string& err) {
  FILE* f = std::fopen(path.c_str(), "r");
  if (!f) { err = "cannot read " + path; return false; }
  std::string text;
  char buf[65536];
  size_t got;
  while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
  std::fclose(f);
  std::vector<std::vector<std::string>> lines;
  bool have_length = false;
  for (size_t at = 0; at < text.size();) {
    size_t nl = text.find('\n', at);
    if (nl == std::string::npos) nl = text.size();
    std::string ln = text.substr(at, nl - at);
    at = nl + 1;
    const size_t hash = ln.find('#');
    if (hash != std::string::npos) ln.erase(hash);
    while (!ln.empty() && std::isspace((unsigned char)ln.back())) ln.pop_back();
    size_t b = 0;
    while (b < ln.size() && std::isspace((unsigned char)ln[b])) b++;
    ln.erase(0, b);
    if (ln.empty()) continue;
    std::vector<std::string> fld;
    for (size_t i = 0;;) { const size_t t = ln.find('\t', i); fld.push_back(ln.substr(i, t == std::string::npos ? t : t - i)); if (t == std::string::npos) break; i = t + 1; }
    bool ok = true;
    if (fld[0] == "length" && fld.size() == 2) { ok = activity_int(fld[1], &out.L); have_length = true; }
    else if (fld[0] == "context" && fld.size() == 3) ok = activity_int(fld[1], &out.up) && activity_int(fld[2], &out.down);
    else if (fld[0] == "link" && fld.size() == 2 && (fld[1] == "identity" || fld[1] == "logistic")) out.link = fld[1] == "logistic" ? 1 : 0;
    else if (fld[0] == "intercept" && fld.size() == 2) ok = activity_decimal(fld[1], 16.0, &out.intercept);
    else if ((fld[0] == "single" && fld.size() == 4) || (fld[0] == "pair" && fld.size() == 5) || (fld[0] == "gc" && fld.size() == 3)) lines.push_back(fld);
    else ok = false;
    if (!ok) { err = path + ": not a line of an activity model: " + ln; return false; }
  }
  if (!have_length || out.L < 1 || out.L > 32) { err = path + ": an activity model needs a `length` line with 1 <= L <= 32"; return false; }
  if (out.up > CALITAS_ACTIVITY_MAX_FLANK || out.down > CALITAS_ACTIVITY_MAX_FLANK) { err = path + ": the `context` of an activity model is 0 .. 16 bases on either side"; return false; }
  const int L = out.L, W = out.up + L + out.down;
  out.single.assign((size_t)W * 4, 0); out.pair.assign((size_t)std::max(W - 1, 1) * 16, 0); out.gc.assign((size_t)L + 1, 0);
  // [lo, hi) of an axis: n values from `first` on (1 for positions, 0 for counts and bases)
  auto axis = [&](const std::string& w, int first, int n, bool base, int* lo, int* hi) {
    if (w == "*") { *lo = first; *hi = first + n; return true; }
    int k = -1;
    if (!base) { if (!activity_int(w, &k)) k = -1; }
    else if (w.size() == 1) { const char* p = std::strchr("ACGT", std::toupper((unsigned char)w[0])); k = p && *p ? (int)(p - "ACGT") : -1; }
    if (k < first || k >= first + n) { err = path + ": " + w + " is not a position, a count or a base of this activity model"; return false; }
    *lo = k; *hi = k + 1;
    return true;
  };
  for (auto& fld : lines) {
    int32_t v = 0;
    int i0, i1, a0, a1, b0, b1;
    if (!activity_decimal(fld.back(), 16.0, &v)) { err = path + ": a weight of an activity model is a decimal in [-16, 16], not " + fld.back(); return false; }
    if (fld[0] == "single") {
      if (!axis(fld[1], 1, W, false, &i0, &i1) || !axis(fld[2], 0, 4, true, &a0, &a1)) return false;
      for (int i = i0; i < i1; i++) for (int a = a0; a < a1; a++) out.single[(size_t)(i - 1) * 4 + (size_t)a] = v;
    } else if (fld[0] == "pair") {
      if (!axis(fld[1], 1, W - 1, false, &i0, &i1) || !axis(fld[2], 0, 4, true, &a0, &a1) || !axis(fld[3], 0, 4, true, &b0, &b1)) return false;
      for (int i = i0; i < i1; i++) for (int a = a0; a < a1; a++) for (int b = b0; b < b1; b++) out.pair[(size_t)(i - 1) * 16 + (size_t)(4 * a + b)] = v;
    } else {
      if (!axis(fld[1], 0, L + 1, false, &i0, &i1)) return false;
      for (int i = i0; i < i1; i++) out.gc[(size_t)i] = v;
    }
  }
  return true;
}

// A microhomology model file (calitas_amd/aligner.py, MicrohomologyModel.read: the same lines accepted and refused, the same integers):
// `#` comments, window / min_length / weight lines, `*` for every deletion length, later lines override earlier ones.
struct MhModelFile {
  int left = 0, right = 0, min_length = 2;
  std::vector<uint32_t> weight;
};
// a decimal as both tools read it -- digits, at most one point, no sign -- within [0, 1], as Q16
static bool mh_decimal(const std::string& x, uint32_t* v) {
  size_t digits = 0, points = 0;
  for (size_t k = 0; k < x.size(); k++) {
    if (x[k] >= '0' && x[k] <= '9') digits++;
    else if (x[k] == '.' && points == 0) points++;
    else return false;
  }
  if (digits == 0) return false;
  const double d = std::strtod(x.c_str(), nullptr);
  if (!(d >= 0.0 && d <= 1.0)) return false;
  *v = (uint32_t)std::floor(d * 65536.0 + 0.5);
  return true;
}
static bool read_mh_model(const std::string& path, MhModelFile& out, std::string& err) {
  FILE* f = std::fopen(path.c_str(), "r");
  if (!f) { err = "cannot read " + path; return false; }
  std::string text;
  char buf[65536];
  size_t got;
  while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
  std::fclose(f);
  std::vector<std::vector<std::string>> lines;
  bool have_window = false;
  for (size_t at = 0; at < text.size();) {
    size_t nl = text.find('\n', at);
    if (nl == std::string::npos) nl = text.size();
    std::string ln = text.substr(at, nl - at);
    at = nl + 1;
    const size_t hash = ln.find('#');
    if (hash != std::string::npos) ln.erase(hash);
    while (!ln.empty() && std::isspace((unsigned char)ln.back())) ln.pop_back();
    size_t b = 0;
    while (b < ln.size() && std::isspace((unsigned char)ln[b])) b++;
    ln.erase(0, b);
    if (ln.empty()) continue;
    std::vector<std::string> fld;
    for (size_t i = 0;;) { const size_t t = ln.find('\t', i); fld.push_back(ln.substr(i, t == std::string::npos ? t : t - i)); if (t == std::string::npos) break; i = t + 1; }
    bool ok = true;
    if (fld[0] == "window" && fld.size() == 3) { ok = activity_int(fld[1], &out.left) && activity_int(fld[2], &out.right); have_window = true; }
    else if (fld[0] == "min_length" && fld.size() == 2) ok = activity_int(fld[1], &out.min_length);
    else if (fld[0] == "weight" && fld.size() == 3) lines.push_back(fld);
    else ok = false;
    if (!ok) { err = path + ": not a line of a microhomology model: " + ln; return false; }
  }
  if (!have_window || out.left < 1 || out.left > CALITAS_MH_MAX_SIDE || out.right < 1 || out.right > CALITAS_MH_MAX_SIDE) {
    err = path + ": a microhomology model needs a `window` line with 1 .. 32 bases on either side";
    return false;
  }
  if (out.min_length < 2 || out.min_length > 8) { err = path + ": the `min_length` of a microhomology model is 2 .. 8"; return false; }
  const int W = out.left + out.right;
  out.weight.assign((size_t)W - 1, 0);
  for (auto& fld : lines) {
    uint32_t v = 0;
    if (!mh_decimal(fld[2], &v)) { err = path + ": a weight of a microhomology model is a decimal in [0, 1], not " + fld[2]; return false; }
    if (fld[1] == "*") { out.weight.assign((size_t)W - 1, v); continue; }
    int d = 0;
    if (!activity_int(fld[1], &d) || d < 1 || d > W - 1) { err = path + ": " + fld[1] + " is not a deletion length of this microhomology model"; return false; }
    out.weight[(size_t)d - 1] = v;
  }
  return true;
}

// `calitas FindGuides`: the sites of an IUPAC pattern in a region as the guides a search takes -- the table of
// `python -m calitas_amd FindGuides`, byte for byte (calitas_amd/tools.py guides_tsv).  No reference counterpart.
// --regions FILE.bed: four columns (chromosome, start, end, class name; more are ignored); lines that start with #, track or browser
// and empty lines are skipped.  The class names take priority in order of first appearance (class 0 is "elsewhere", at most 7 names);
// an interval on a chromosome the reference lacks is skipped and counted on stderr, one past its contig's end is an error.
static bool set_regions_from_bed(calitas_ctx* ctx, const std::string& path, std::vector<std::string>& classes, std::string& err) {
  FILE* f = std::fopen(path.c_str(), "r");
  if (!f) { err = "cannot open " + path; return false; }
  std::string text;
  char buf[65536];
  size_t got;
  while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
  std::fclose(f);
  int32_t n_contigs = 0;
  calitas_reference_info(ctx, &n_contigs, nullptr, nullptr);
  std::vector<std::string> names((size_t)n_contigs);
  std::vector<uint64_t> lens((size_t)n_contigs);
  for (int32_t c = 0; c < n_contigs; c++) { const char* nm = ""; calitas_contig_name(ctx, c, &nm, &lens[(size_t)c]); names[(size_t)c] = nm; }
  classes.assign(1, "elsewhere");
  std::vector<calitas_region_t> iv;
  size_t skipped = 0, line_no = 0;
  for (size_t at = 0; at < text.size();) {
    size_t nl = text.find('\n', at);
    if (nl == std::string::npos) nl = text.size();
    std::string line = text.substr(at, nl - at);
    at = nl + 1; line_no++;
    while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
    if (line.find_first_not_of(" \t\r\f\v") == std::string::npos || line[0] == '#' || line.rfind("track", 0) == 0 || line.rfind("browser", 0) == 0) continue;
    const std::string where = path + ":" + std::to_string(line_no) + ": ";
    std::vector<std::string> col;
    if (line.find('\t') != std::string::npos) {
      for (size_t a = 0;;) { const size_t t = line.find('\t', a); col.push_back(line.substr(a, t == std::string::npos ? t : t - a)); if (t == std::string::npos) break; a = t + 1; }
    } else {
      for (size_t a = 0; (a = line.find_first_not_of(" \f\v", a)) != std::string::npos;) { const size_t t = line.find_first_of(" \f\v", a); col.push_back(line.substr(a, t == std::string::npos ? t : t - a)); if (t == std::string::npos) break; a = t; }
    }
    if (col.size() < 4) { err = where + "a regions file has four columns (chromosome, start, end, class)"; return false; }
    char *e1 = nullptr, *e2 = nullptr;
    const long long a = std::strtoll(col[1].c_str(), &e1, 10), b = std::strtoll(col[2].c_str(), &e2, 10);
    if (col[1].empty() || col[2].empty() || *e1 || *e2) { err = where + "start and end are integers"; return false; }
    if (col[3] == "elsewhere") { err = where + "the class name elsewhere is reserved for hits outside every interval"; return false; }
    size_t cls = std::find(classes.begin(), classes.end(), col[3]) - classes.begin();
    if (cls == classes.size()) classes.push_back(col[3]);
    if (classes.size() > CALITAS_REGION_CLASSES_MAX) { err = where + "more than 7 class names"; return false; }
    if (a < 0 || a >= b) { err = where + "start >= end (or negative)"; return false; }
    const size_t c = std::find(names.begin(), names.end(), col[0]) - names.begin();
    if (c == names.size()) { skipped++; continue; }
    if ((uint64_t)b > lens[c]) { err = where + "the interval ends beyond " + col[0]; return false; }
    iv.push_back(calitas_region_t{(int32_t)c, (int32_t)a, (int32_t)b, (uint32_t)cls});
  }
  if (skipped) std::fprintf(stderr, "%zu intervals on chromosomes the reference does not have were skipped\n", skipped);
  if (classes.size() < 2) { err = path + ": no interval"; return false; }
  if (calitas_set_regions(ctx, iv.size(), iv.data(), (uint32_t)classes.size()) != CALITAS_OK) { err = std::string("regions: ") + calitas_last_error(ctx); return false; }
  if (iv.empty()) { err = path + ": no interval lies on a chromosome of the reference"; return false; }
  return true;
}
// --top-classes name,...: the list_mask of those classes.
static bool class_mask(const std::vector<std::string>& classes, const std::string& names, uint32_t& mask, std::string& err) {
  mask = 0;
  for (size_t a = 0; a <= names.size();) {
    size_t t = names.find(',', a);
    if (t == std::string::npos) t = names.size();
    const std::string nm = names.substr(a, t - a);
    a = t + 1;
    if (nm.empty()) continue;
    const size_t c = std::find(classes.begin(), classes.end(), nm) - classes.begin();
    if (c == classes.size()) { err = "unknown class " + nm; return false; }
    mask |= 1u << c;
  }
  return true;
}

// --gc-min / --gc-max / --max-run / --avoid as a calitas_site_filter_t for a protospacer of L bases (calitas_amd/tools.py
// site_filter_of_flags: the same numbers, the same motifs in the same order).
static bool site_filter_of_flags(int L, int gc_lo, int gc_hi, bool limited, const std::string& max_run, const std::vector<std::string>& avoid, calitas_site_filter_t& f,
                                 std::string& err) {
  std::memset(&f, 0, sizeof f);
  if (gc_lo < 0 || gc_lo > 100 || gc_hi < 0 || gc_hi > 100) { err = "--gc-min and --gc-max are percentages, 0 .. 100"; return false; }
  f.gc_min = (uint8_t)((gc_lo * L + 99) / 100);
  f.gc_max = (uint8_t)(gc_hi * L / 100);
  for (size_t a = 0; limited && a <= max_run.size();) {
    size_t t = max_run.find(',', a);
    if (t == std::string::npos) t = max_run.size();
    std::string part = max_run.substr(a, t - a);
    a = t + 1;
    while (!part.empty() && part.front() == ' ') part.erase(0, 1);
    while (!part.empty() && part.back() == ' ') part.pop_back();
    const size_t eq = part.rfind('=');
    const std::string n = eq == std::string::npos ? part : part.substr(eq + 1);
    const char* at = eq == 1 ? std::strchr("ACGT", std::toupper((unsigned char)part[0])) : nullptr;
    const size_t nz = n.find_first_not_of('0');               // (leading zeros are digits, as int() has it)
    if (n.empty() || n.find_first_not_of("0123456789") != std::string::npos || (nz != std::string::npos && n.size() - nz > 3) || std::atoi(n.c_str()) > 255 ||
        (eq != std::string::npos && !(at && *at))) { err = "--max-run takes N or BASE=N,... (A C G T; 0 .. 255), not " + max_run; return false; }
    if (eq == std::string::npos) for (int b = 0; b < 4; b++) f.max_run[b] = (uint8_t)std::atoi(n.c_str());
    else f.max_run[at - "ACGT"] = (uint8_t)std::atoi(n.c_str());
  }
  std::vector<std::string> motifs;
  for (const std::string& m : avoid) {
    std::string up = m, rc;
    for (auto& c : up) c = (char)std::toupper((unsigned char)c);
    for (size_t i = up.size(); i-- > 0;) {
      const char* from = "ACGTUMRWSYKVHDBN";
      const char* to = "TGCAAKYWSRMBDHVN";
      const char* p = std::strchr(from, up[i]);
      rc += (p && *p) ? to[p - from] : up[i];
    }
    for (const std::string& x : {up, rc}) if (std::find(motifs.begin(), motifs.end(), x) == motifs.end()) motifs.push_back(x);
  }
  if (motifs.size() > 8) { err = "--avoid: more than 8 motifs once the reverse complements are added"; return false; }
  f.n_motifs = (uint8_t)motifs.size();
  for (size_t i = 0; i < motifs.size(); i++) {
    if (motifs[i].size() > 16) { err = "a motif of a site filter has at most 16 letters: " + motifs[i]; return false; }
    std::memcpy(f.motifs[i], motifs[i].data(), motifs[i].size());
  }
  return true;
}

static int find_guides_main(int argc, char** argv) {
  std::string pattern, ref, output, chrom, max_run;
  std::vector<std::string> aux, avoid;
  uint64_t start = 0, end = 0;
  int device = 0, gc_lo = 0, gc_hi = 100;
  bool filtered = false, limited = false, copies = false;
  long long seed_k = 0, max_copies = 0, max_seed_copies = 0;      // 0: the flag is not given
  bool have_seed = false, have_max = false, have_max_seed = false;
  long long near_m = 0, max_near = 0;
  bool have_near = false, have_max_near = false;
  std::string near_scores;     // --near-scores MODEL.tsv
  std::string near_list;       // --near-list FILE
  long long near_list_limit = 1000;
  bool have_list_limit = false;
  std::string activity, min_activity;     // --activity MODEL.tsv [--min-activity X]
  bool have_min_activity = false;
  std::string regions_path, class_names, class_extent;     // --regions FILE.bed [--classes name,...] [--class-extent FROM:TO]
  bool have_classes = false, have_extent = false;
  std::string pairs_path, pair_distance, pair_cut, pair_orientation;     // --pairs FILE --pair-distance MIN:MAX [--pair-cut N] [--pair-orientation ...]
  bool have_pair_distance = false, have_pair_cut = false, have_pair_orientation = false;
  std::string alleles_path, allele_sites_path, allele_kinds;             // --alleles FILE.vcf --allele-sites OUT.tsv [--allele-kinds alt,ref,both]
  bool have_allele_kinds = false;
  std::string edit_sites_path, editor, edit_window, edit_context, edit_mode, max_bystanders;   // --edit-sites OUT.tsv --editor FROM:TO --edit-window FROM:TO [...]
  bool have_editor = false, have_edit_window = false, have_edit_context = false, have_edit_mode = false, have_max_bystanders = false;
  std::string mh_path, mh_cut, min_oof;                                  // --microhomology MODEL.tsv [--mh-cut N] [--min-out-of-frame PCT]
  bool have_mh_cut = false, have_min_oof = false;
  for (int i = 2; i < argc; i++) {
    std::string a = argv[i], val;
    size_t eq = a.find('=');
    if (a.compare(0, 2, "--") == 0 && eq != std::string::npos) { val = a.substr(eq + 1); a = a.substr(0, eq); }
    a = long_to_short(a);
    auto next = [&]() -> std::string {
      if (!val.empty()) return val;
      if (i + 1 >= argc) { usage(); std::exit(2); }
      return argv[++i];
    };
    if (a == "-i") pattern = next();
    else if (a == "-r") ref = next();
    else if (a == "-o") output = next();
    else if (a == "-c") chrom = next();
    else if (a == "-s" || a == "--start") start = std::strtoull(next().c_str(), nullptr, 10);
    else if (a == "-e" || a == "--end") end = std::strtoull(next().c_str(), nullptr, 10);
    else if (a == "-x") { aux.push_back(next()); while (i + 1 < argc && argv[i + 1][0] != '-') aux.push_back(argv[++i]); }
    else if (a == "--device") device = std::atoi(next().c_str());
    else if (a == "--gc-min") { gc_lo = std::atoi(next().c_str()); filtered = true; }
    else if (a == "--gc-max") { gc_hi = std::atoi(next().c_str()); filtered = true; }
    else if (a == "--max-run") { max_run = next(); filtered = limited = true; }
    else if (a == "--avoid") { avoid.push_back(next()); filtered = true; }
    else if (a == "--copies") copies = true;
    else if (a == "--seed-copies") { seed_k = std::atoll(next().c_str()); have_seed = true; }
    else if (a == "--max-copies") { max_copies = std::atoll(next().c_str()); have_max = copies = true; }
    else if (a == "--max-seed-copies") { max_seed_copies = std::atoll(next().c_str()); have_max_seed = true; }
    else if (a == "--near-copies") { near_m = std::atoll(next().c_str()); have_near = true; }
    else if (a == "--max-near-copies") { max_near = std::atoll(next().c_str()); have_max_near = true; }
    else if (a == "--near-scores") near_scores = next();
    else if (a == "--near-list") near_list = next();
    else if (a == "--near-list-limit") { near_list_limit = std::atoll(next().c_str()); have_list_limit = true; }
    else if (a == "--activity") activity = next();
    else if (a == "--min-activity") { min_activity = next(); have_min_activity = true; }
    else if (a == "--regions") regions_path = next();
    else if (a == "--classes") { class_names = next(); have_classes = true; }
    else if (a == "--class-extent") { class_extent = next(); have_extent = true; }
    else if (a == "--pairs") pairs_path = next();
    else if (a == "--pair-distance") { pair_distance = next(); have_pair_distance = true; }
    else if (a == "--pair-cut") { pair_cut = next(); have_pair_cut = true; }
    else if (a == "--pair-orientation") { pair_orientation = next(); have_pair_orientation = true; }
    else if (a == "--alleles") alleles_path = next();
    else if (a == "--allele-sites") allele_sites_path = next();
    else if (a == "--allele-kinds") { allele_kinds = next(); have_allele_kinds = true; }
    else if (a == "--edit-sites") edit_sites_path = next();
    else if (a == "--editor") { editor = next(); have_editor = true; }
    else if (a == "--edit-window") { edit_window = next(); have_edit_window = true; }
    else if (a == "--edit-context") { edit_context = next(); have_edit_context = true; }
    else if (a == "--edit-mode") { edit_mode = next(); have_edit_mode = true; }
    else if (a == "--max-bystanders") { max_bystanders = next(); have_max_bystanders = true; }
    else if (a == "--microhomology") mh_path = next();
    else if (a == "--mh-cut") { mh_cut = next(); have_mh_cut = true; }
    else if (a == "--min-out-of-frame") { min_oof = next(); have_min_oof = true; }
    else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
  }
  if (pattern.empty() || ref.empty()) { usage(); return 2; }
  ParsedGuide pg;
  if (int rc = parse_guide(pattern, aux, pg)) return rc;
  calitas_guide_t g = pg.c_guide();
  calitas_site_filter_t filter;
  std::string filter_err;
  if (filtered && !site_filter_of_flags((int)pg.proto.size(), gc_lo, gc_hi, limited, max_run, avoid, filter, filter_err)) {
    std::fprintf(stderr, "calitas: %s\n", filter_err.c_str());
    return 2;
  }
  const calitas_site_filter_t* keep = filtered ? &filter : nullptr;
  if (have_seed && (seed_k < 1 || seed_k > (long long)pg.proto.size())) { std::fprintf(stderr, "calitas: --seed-copies K: K is 1 .. %zu, the protospacer's length\n", pg.proto.size()); return 2; }
  if (have_max && max_copies < 1) { std::fprintf(stderr, "calitas: --max-copies N: N is at least 1 (a guide counts itself)\n"); return 2; }
  if (have_max_seed && !have_seed) { std::fprintf(stderr, "calitas: --max-seed-copies requires --seed-copies K\n"); return 2; }
  if (have_max_seed && max_seed_copies < 1) { std::fprintf(stderr, "calitas: --max-seed-copies N: N is at least 1 (a guide counts itself)\n"); return 2; }
  if (have_near && (near_m < 0 || near_m > CALITAS_NEAR_MAX_MISMATCHES)) { std::fprintf(stderr, "calitas: --near-copies M: M is 0 .. %d\n", CALITAS_NEAR_MAX_MISMATCHES); return 2; }
  if (have_near && (long long)pg.proto.size() < near_m + 1) { std::fprintf(stderr, "calitas: --near-copies M: the protospacer has fewer than M + 1 bases\n"); return 2; }
  if (have_max_near && !have_near) { std::fprintf(stderr, "calitas: --max-near-copies requires --near-copies M\n"); return 2; }
  if (have_max_near && max_near < 1) { std::fprintf(stderr, "calitas: --max-near-copies N: N is at least 1 (a guide counts itself)\n"); return 2; }
  const bool have_near_scores = !near_scores.empty();
  if (have_near_scores && !have_near) { std::fprintf(stderr, "calitas: --near-scores requires --near-copies M\n"); return 2; }
  const bool have_near_list = !near_list.empty();
  if (have_near_list && !have_near) { std::fprintf(stderr, "calitas: --near-list requires --near-copies M\n"); return 2; }
  if (have_list_limit && !have_near_list) { std::fprintf(stderr, "calitas: --near-list-limit requires --near-list FILE\n"); return 2; }
  if (have_list_limit && (near_list_limit < 1 || near_list_limit > CALITAS_NEAR_LIST_MAX)) { std::fprintf(stderr, "calitas: --near-list-limit N: N is 1 .. %d\n", CALITAS_NEAR_LIST_MAX); return 2; }
  ScoreModelFile near_model;
  if (have_near_scores) {
    std::string err;
    if (!read_score_model(near_scores, near_model, err)) { std::fprintf(stderr, "calitas: %s\n", err.c_str()); return 2; }
    if (near_model.L != (int)pg.proto.size()) {
      std::fprintf(stderr, "calitas: --near-scores: the model is for protospacers of %d bases, the pattern's has %zu\n", near_model.L, pg.proto.size());
      return 2;
    }
  }
  const bool have_activity = !activity.empty();
  if (have_min_activity && !have_activity) { std::fprintf(stderr, "calitas: --min-activity requires --activity MODEL\n"); return 2; }
  ActivityModelFile act;
  int32_t min_score = CALITAS_ACTIVITY_NONE;
  if (have_activity) {
    std::string err;
    if (!read_activity_model(activity, act, err)) { std::fprintf(stderr, "calitas: %s\n", err.c_str()); return 2; }
    if (act.L != (int)pg.proto.size()) {
      std::fprintf(stderr, "calitas: --activity: the model is for protospacers of %d bases, the pattern's has %zu\n", act.L, pg.proto.size());
      return 2;
    }
    // (+-2064: 129 weights of 16.0, what a score can be)
    if (have_min_activity && !activity_decimal(min_activity, 2064.0, &min_score)) { std::fprintf(stderr, "calitas: --min-activity X: X is a decimal in [-2064, 2064], not %s\n", min_activity.c_str()); return 2; }
  }
  const bool have_regions = !regions_path.empty();
  if (!have_regions && (have_classes || have_extent)) { std::fprintf(stderr, "calitas: --classes and --class-extent require --regions FILE.bed\n"); return 2; }
  calitas_site_regions_t by_class{0, 0, 0, 0};
  if (have_extent) {
    const size_t colon = class_extent.find(':');
    const std::string from = class_extent.substr(0, colon), to = colon == std::string::npos ? std::string() : class_extent.substr(colon + 1);
    const auto digits = [](const std::string& t) { return !t.empty() && t.size() <= 6 && t.find_first_not_of("0123456789") == std::string::npos; };
    if (!digits(from) || !digits(to)) { std::fprintf(stderr, "calitas: --class-extent FROM:TO: two integers, 0-based and half-open in the protospacer, not %s\n", class_extent.c_str()); return 2; }
    const long a = std::atol(from.c_str()), b = std::atol(to.c_str());
    if (!(a < b && b <= (long)pg.proto.size())) { std::fprintf(stderr, "calitas: --class-extent FROM:TO: 0 <= FROM < TO <= %zu, the protospacer's length\n", pg.proto.size()); return 2; }
    by_class.ext_from = (uint8_t)a; by_class.ext_to = (uint8_t)b;
  }
  // --alleles: the kinds of lines to write (tools.py allele_sites_tool)
  const bool have_alleles = !alleles_path.empty(), have_allele_sites = !allele_sites_path.empty(), have_edit_sites = !edit_sites_path.empty();
  if (have_edit_sites && !(have_alleles && have_editor && have_edit_window)) { std::fprintf(stderr, "calitas: --edit-sites OUT.tsv requires --alleles FILE.vcf, --editor FROM:TO and --edit-window FROM:TO\n"); return 2; }
  if (!have_edit_sites && (have_editor || have_edit_window || have_edit_context || have_edit_mode || have_max_bystanders)) {
    std::fprintf(stderr, "calitas: --editor, --edit-window, --edit-context, --edit-mode and --max-bystanders require --edit-sites OUT.tsv\n");
    return 2;
  }
  if (!have_alleles && have_allele_sites) { std::fprintf(stderr, "calitas: --alleles FILE.vcf and --allele-sites OUT.tsv require each other\n"); return 2; }
  if (have_alleles && !have_allele_sites && !have_edit_sites) { std::fprintf(stderr, "calitas: --alleles FILE.vcf requires --allele-sites OUT.tsv or --edit-sites OUT.tsv\n"); return 2; }
  if (have_allele_kinds && !have_allele_sites) { std::fprintf(stderr, "calitas: --allele-kinds requires --alleles FILE.vcf and --allele-sites OUT.tsv\n"); return 2; }
  // --edit-sites: the editor from its flags (tools.py base_edit_of_flags)
  calitas_base_edit_t edit{};
  if (have_edit_sites) {
    const auto base = [](char c) { return c != 0 && std::strchr("ACGT", c) != nullptr; };
    if (!(editor.size() == 3 && editor[1] == ':' && base(editor[0]) && base(editor[2]) && editor[0] != editor[2])) {
      std::fprintf(stderr, "calitas: --editor FROM:TO: two different letters of A C G T (C:T a CBE, A:G an ABE), not %s\n", editor.c_str());
      return 2;
    }
    const size_t colon = edit_window.find(':');
    const std::string from = edit_window.substr(0, colon), to = colon == std::string::npos ? std::string() : edit_window.substr(colon + 1);
    const auto digits = [](const std::string& t) { return !t.empty() && t.size() <= 9 && t.find_first_not_of("0123456789") == std::string::npos; };
    if (!digits(from) || !digits(to)) { std::fprintf(stderr, "calitas: --edit-window FROM:TO: two integers, 0-based and half-open in the protospacer, not %s\n", edit_window.c_str()); return 2; }
    const long w0 = std::atol(from.c_str()), w1 = std::atol(to.c_str());
    if (!(w0 < w1 && w1 <= (long)pg.proto.size())) { std::fprintf(stderr, "calitas: --edit-window FROM:TO: 0 <= FROM < TO <= %zu, the protospacer's length\n", pg.proto.size()); return 2; }
    char context = 'N';
    if (have_edit_context) {
      context = edit_context.size() == 1 ? (char)std::toupper((unsigned char)edit_context[0]) : 0;
      if (context == 0 || !std::strchr("ACGTUMRWSYKVHDBN", context)) { std::fprintf(stderr, "calitas: --edit-context: one IUPAC letter, not %s\n", edit_context.c_str()); return 2; }
    }
    if (have_edit_mode && edit_mode != "install" && edit_mode != "correct") { std::fprintf(stderr, "calitas: --edit-mode: install or correct, not %s\n", edit_mode.c_str()); return 2; }
    if (have_max_bystanders && !(digits(max_bystanders) && std::atol(max_bystanders.c_str()) <= 31)) {
      std::fprintf(stderr, "calitas: --max-bystanders N: an integer 0 .. 31, not %s\n", max_bystanders.c_str());
      return 2;
    }
    edit.from_base = editor[0]; edit.to_base = editor[2];
    edit.window_from = (uint8_t)w0; edit.window_to = (uint8_t)w1;
    edit.context = context;
    edit.correct = edit_mode == "correct" ? 1 : 0;
    edit.max_bystanders = have_max_bystanders ? (uint8_t)std::atol(max_bystanders.c_str()) : 255;
  }
  unsigned kinds_wanted = have_allele_kinds ? 0u : 14u;                  // bit k: lines of kind k (1 alt, 2 ref, 3 both)
  if (have_allele_kinds) {
    bool ok = true;
    for (size_t at = 0; at <= allele_kinds.size();) {
      size_t comma = allele_kinds.find(',', at);
      if (comma == std::string::npos) comma = allele_kinds.size();
      const std::string k = allele_kinds.substr(at, comma - at);
      if (k == "alt") kinds_wanted |= 2u; else if (k == "ref") kinds_wanted |= 4u; else if (k == "both") kinds_wanted |= 8u; else if (!k.empty()) ok = false;
      at = comma + 1;
    }
    if (!ok || kinds_wanted == 0) { std::fprintf(stderr, "calitas: --allele-kinds: names among alt, ref, both, separated by commas, not %s\n", allele_kinds.c_str()); return 2; }
  }
  // --pairs: the rule of a pair from its flags (tools.py site_pairs_of_flags)
  const bool have_pairs = !pairs_path.empty();
  if (!have_pairs && (have_pair_distance || have_pair_cut || have_pair_orientation)) { std::fprintf(stderr, "calitas: --pair-distance, --pair-cut and --pair-orientation require --pairs FILE\n"); return 2; }
  if (have_pairs && !have_pair_distance) { std::fprintf(stderr, "calitas: --pairs requires --pair-distance MIN:MAX\n"); return 2; }
  calitas_site_pairs_t pair_rule{0, 0, 0, 0, {0, 0}};
  const bool pattern_has_pam = !pg.pams.empty(), three_prime = pattern_has_pam && !pg.pam5;
  if (have_pairs) {
    const auto digits = [](const std::string& t, size_t most) { return !t.empty() && t.size() <= most && t.find_first_not_of("0123456789") == std::string::npos; };
    const size_t colon = pair_distance.find(':');
    const std::string lo = pair_distance.substr(0, colon), hi = colon == std::string::npos ? std::string() : pair_distance.substr(colon + 1);
    if (!digits(lo, 9) || !digits(hi, 9) || !(std::atol(lo.c_str()) <= std::atol(hi.c_str()) && std::atol(hi.c_str()) <= CALITAS_PAIR_MAX_DISTANCE)) {
      std::fprintf(stderr, "calitas: --pair-distance MIN:MAX: two integers, 0 <= MIN <= MAX <= %d, not %s\n", CALITAS_PAIR_MAX_DISTANCE, pair_distance.c_str());
      return 2;
    }
    pair_rule.min_distance = (int32_t)std::atol(lo.c_str()); pair_rule.max_distance = (int32_t)std::atol(hi.c_str());
    if (!have_pair_cut && !three_prime) { std::fprintf(stderr, "calitas: --pair-cut N is required: the default, L - 3, is the Cas9 cut of a pattern with a 3' PAM\n"); return 2; }
    if (have_pair_cut && !(digits(pair_cut, 3) && std::atol(pair_cut.c_str()) <= (long)pg.proto.size())) {
      std::fprintf(stderr, "calitas: --pair-cut N: N is 0 .. %zu, the protospacer's length, not %s\n", pg.proto.size(), pair_cut.c_str());
      return 2;
    }
    const long cut = have_pair_cut ? std::atol(pair_cut.c_str()) : (long)pg.proto.size() - 3;
    if (cut < 0) { std::fprintf(stderr, "calitas: --pair-cut N is required: the protospacer has fewer than 3 bases\n"); return 2; }
    pair_rule.cut_offset = (uint8_t)cut;
    const std::string names = have_pair_orientation ? pair_orientation : std::string("out");
    unsigned mask = 0;
    bool any_name = false;
    for (size_t at = 0; at <= names.size();) {
      size_t comma = names.find(',', at);
      if (comma == std::string::npos) comma = names.size();
      const std::string o = names.substr(at, comma - at);
      at = comma + 1;
      if (o.empty()) continue;
      any_name = true;
      static const char* const codes[4] = {"++", "-+", "+-", "--"};
      int code = -1;
      for (int k = 0; k < 4; k++) if (o == codes[k]) code = k;
      if (code >= 0) { mask |= 1u << code; continue; }
      if (o != "out" && o != "in" && o != "same" && o != "any") { std::fprintf(stderr, "calitas: --pair-orientation: %s: out, in, same, any, or a code among ++ -+ +- --\n", o.c_str()); return 2; }
      if (!pattern_has_pam) { std::fprintf(stderr, "calitas: --pair-orientation: %s needs a PAM: a pattern without one takes the codes ++ -+ +- --\n", o.c_str()); return 2; }
      mask |= o == "any" ? 15u : o == "same" ? 9u : ((o == "out") == three_prime) ? 2u : 4u;
    }
    if (!any_name) { std::fprintf(stderr, "calitas: --pair-orientation is empty: out, in, same, any, or codes among ++ -+ +- --\n"); return 2; }
    pair_rule.orientations = (uint8_t)mask;
  }
  // --microhomology: the model, the cut and the per-mille from their flags (tools.py find_guides_tool)
  const bool have_mh = !mh_path.empty();
  if (!have_mh && (have_mh_cut || have_min_oof)) { std::fprintf(stderr, "calitas: --mh-cut and --min-out-of-frame require --microhomology MODEL\n"); return 2; }
  MhModelFile mh_file;
  calitas_mh_model_t mh_model{0, 0, 0, 0, nullptr};
  int32_t mh_permille = 0;
  if (have_mh) {
    std::string err;
    if (!read_mh_model(mh_path, mh_file, err)) { std::fprintf(stderr, "calitas: %s\n", err.c_str()); return 2; }
    const auto digits = [](const std::string& t, size_t most) { return !t.empty() && t.size() <= most && t.find_first_not_of("0123456789") == std::string::npos; };
    if (!have_mh_cut && !three_prime) { std::fprintf(stderr, "calitas: --mh-cut N is required: the default, L - 3, is the Cas9 cut of a pattern with a 3' PAM\n"); return 2; }
    if (have_mh_cut && !(digits(mh_cut, 3) && std::atol(mh_cut.c_str()) <= (long)pg.proto.size())) {
      std::fprintf(stderr, "calitas: --mh-cut N: N is 0 .. %zu, the protospacer's length, not %s\n", pg.proto.size(), mh_cut.c_str());
      return 2;
    }
    if (have_min_oof && !(digits(min_oof, 3) && std::atol(min_oof.c_str()) <= 100)) {
      std::fprintf(stderr, "calitas: --min-out-of-frame PCT: PCT is an integer 0 .. 100, not %s\n", min_oof.c_str());
      return 2;
    }
    mh_model.left = mh_file.left; mh_model.right = mh_file.right; mh_model.min_length = mh_file.min_length; mh_model.weight = mh_file.weight.data();
    mh_model.cut_offset = have_mh_cut ? (int32_t)std::atol(mh_cut.c_str()) : (int32_t)pg.proto.size() - 3;     // (below 0: the library refuses it)
    mh_permille = have_min_oof ? 10 * (int32_t)std::atol(min_oof.c_str()) : 0;
  }
  calitas_ctx* ctx = nullptr;
  if (calitas_create(device, &ctx) != CALITAS_OK) { std::fprintf(stderr, "calitas: %s\n", calitas_last_error(nullptr)); return 1; }
  auto die = [&](const char* what) { std::fprintf(stderr, "calitas: %s: %s\n", what, calitas_last_error(ctx)); calitas_destroy(ctx); std::exit(1); };
  if (calitas_set_reference_fasta(ctx, ref.c_str()) != CALITAS_OK) die("reading reference");
  int32_t chrom_index = -1;
  if (!chrom.empty()) {
    int32_t n = 0; calitas_reference_info(ctx, &n, nullptr, nullptr);
    for (int32_t i = 0; i < n; i++) { const char* nm; uint64_t len; calitas_contig_name(ctx, i, &nm, &len); if (chrom == nm) chrom_index = i; }
    if (chrom_index < 0) { std::fprintf(stderr, "Unknown chromosome: %s\n", chrom.c_str()); calitas_destroy(ctx); return 1; }
  }
  // --regions: the set goes to the context, the listing keeps the sites of the wanted classes (tools.py find_guides_tool)
  std::vector<std::string> classes;
  if (have_regions) {
    std::string err;
    if (!set_regions_from_bed(ctx, regions_path, classes, err)) { std::fprintf(stderr, "calitas: %s\n", err.c_str()); calitas_destroy(ctx); return 2; }
    if (have_classes) {
      if (!class_mask(classes, class_names, by_class.class_mask, err)) { std::fprintf(stderr, "calitas: %s\n", err.c_str()); calitas_destroy(ctx); return 2; }
    } else by_class.class_mask = ((1u << classes.size()) - 1u) & ~1u;        // every named class
  }
  calitas_site_t* sites = nullptr; uint64_t n_sites = 0;
  uint8_t* site_class = nullptr;       // with --regions: a class per site
  int32_t* activity_q16 = nullptr;     // with --activity: a score per site, from the listing's own call (tools.py find_guides)
  calitas_mh_score_t* mh_q16 = nullptr; // with --microhomology: the two sums per site, from a listing of its own
  const bool mh_alone = have_mh && !have_activity && !have_regions;
  int rc;
  if (have_activity) {
    calitas_activity_model_t m;
    m.protospacer_length = act.L; m.up = act.up; m.down = act.down; m.link = act.link; m.intercept = act.intercept;
    m.single = act.single.data(); m.pair = act.pair.data(); m.gc = act.gc.data();
    rc = device < 0 ? calitas_find_sites_scored_host(ctx, &g, keep, &m, min_score, chrom_index, start, end, &sites, &activity_q16, &n_sites)
                    : calitas_find_sites_scored(ctx, &g, keep, &m, min_score, chrom_index, start, end, &sites, &activity_q16, &n_sites);
  } else if (have_regions) {
    rc = device < 0 ? calitas_find_sites_regions_host(ctx, &g, keep, &by_class, chrom_index, start, end, &sites, &site_class, &n_sites)
                    : calitas_find_sites_regions(ctx, &g, keep, &by_class, chrom_index, start, end, &sites, &site_class, &n_sites);
  } else if (mh_alone) {
    rc = device < 0 ? calitas_find_sites_microhomology_host(ctx, &g, keep, &mh_model, mh_permille, chrom_index, start, end, &sites, &mh_q16, &n_sites)
                    : calitas_find_sites_microhomology(ctx, &g, keep, &mh_model, mh_permille, chrom_index, start, end, &sites, &mh_q16, &n_sites);
  } else {
    rc = device < 0 ? calitas_find_sites_filtered_host(ctx, &g, keep, chrom_index, start, end, &sites, &n_sites)
                    : calitas_find_sites_filtered(ctx, &g, keep, chrom_index, start, end, &sites, &n_sites);
  }
  if (rc != CALITAS_OK) die("finding sites");
  if (have_regions && have_activity) {
    // both listings over the same region, joined on (contig, protospacer start, strand) in one walk: both are in that order.  The
    // scored listing keeps the rows that are in both (a classed site below --min-activity has no partner and goes).
    calitas_site_t* classed = nullptr; uint64_t n_classed = 0;
    rc = device < 0 ? calitas_find_sites_regions_host(ctx, &g, keep, &by_class, chrom_index, start, end, &classed, &site_class, &n_classed)
                    : calitas_find_sites_regions(ctx, &g, keep, &by_class, chrom_index, start, end, &classed, &site_class, &n_classed);
    if (rc != CALITAS_OK) die("finding sites by regions");
    const auto less = [](const calitas_site_t& x, const calitas_site_t& y) {
      if (x.contig_index != y.contig_index) return x.contig_index < y.contig_index;
      if (x.protospacer_start != y.protospacer_start) return x.protospacer_start < y.protospacer_start;
      return x.strand == '+' && y.strand == '-';
    };
    uint64_t n = 0;
    for (uint64_t i = 0, j = 0; i < n_classed; i++) {
      while (j < n_sites && less(sites[j], classed[i])) j++;
      if (j < n_sites && !less(classed[i], sites[j])) { sites[n] = sites[j]; activity_q16[n] = activity_q16[j]; site_class[n] = site_class[i]; n++; }
    }
    n_sites = n;
    calitas_free(classed);
  }
  if (have_mh && !mh_alone) {
    // the same walk again: the microhomology listing over the same region, joined on (contig, protospacer start, strand); a site the
    // per-mille dropped has no partner and goes
    calitas_site_t* scored = nullptr; uint64_t n_scored = 0;
    rc = device < 0 ? calitas_find_sites_microhomology_host(ctx, &g, keep, &mh_model, mh_permille, chrom_index, start, end, &scored, &mh_q16, &n_scored)
                    : calitas_find_sites_microhomology(ctx, &g, keep, &mh_model, mh_permille, chrom_index, start, end, &scored, &mh_q16, &n_scored);
    if (rc != CALITAS_OK) die("scoring microhomology");
    const auto less = [](const calitas_site_t& x, const calitas_site_t& y) {
      if (x.contig_index != y.contig_index) return x.contig_index < y.contig_index;
      if (x.protospacer_start != y.protospacer_start) return x.protospacer_start < y.protospacer_start;
      return x.strand == '+' && y.strand == '-';
    };
    uint64_t n = 0;
    for (uint64_t i = 0, j = 0; i < n_sites; i++) {
      while (j < n_scored && less(scored[j], sites[i])) j++;
      if (j < n_scored && !less(sites[i], scored[j])) {              // (n <= i and n <= j: nothing is overwritten before it is read)
        sites[n] = sites[i]; mh_q16[n] = mh_q16[j];
        if (activity_q16) activity_q16[n] = activity_q16[i];
        if (site_class) site_class[n] = site_class[i];
        n++;
      }
    }
    n_sites = n;
    calitas_free(scored);
  }
  FILE* f = output.empty() ? stdout : std::fopen(output.c_str(), "w");
  if (!f) { std::fprintf(stderr, "cannot write %s\n", output.c_str()); calitas_free(sites); calitas_free(activity_q16); calitas_free(site_class); calitas_free(mh_q16); calitas_destroy(ctx); return 1; }
  std::fprintf(f, "guide_id\tchromosome\tstart\tend\tstrand\tpam_index\tguide\tpam_sequence%s%s%s%s%s", have_regions ? "\tclass" : "", have_activity ? "\tactivity_q16\tactivity" : "",
               have_mh ? "\tmh_total_q16\tmh_oof_q16\tmh_score\tout_of_frame" : "", copies ? "\tcopies" : "", have_seed ? "\tseed_copies" : "");
  for (long long d = 0; have_near && d <= near_m; d++) std::fprintf(f, "\tcopies_mm%lld", d);
  if (have_near_scores) std::fprintf(f, "\tnear_sum_q32\tnear_max_q32\tnear_specificity");
  std::fprintf(f, "\n");
  auto on_strand = [](std::string t, bool minus) {     // upper-case bases as fetched; '-': their reverse complement
    if (!minus) return t;
    std::string o(t.rbegin(), t.rend());
    for (auto& c : o) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : (c == 'T' || c == 'U') ? 'A' : c;
    return o;
  };
  const int64_t L = (int64_t)pg.proto.size();
  // the rows' protospacers, or their PAM-proximal K bases, counted over the whole reference (tools.py guide_copies)
  std::vector<std::string> protos((size_t)n_sites), pam_seqs((size_t)n_sites);
  for (uint64_t i = 0; i < n_sites; i++) {
    const calitas_site_t& s = sites[i];
    std::string proto((size_t)L, 'N'), pam((size_t)s.pam_length, 'N');
    if (calitas_fetch_bases(ctx, s.contig_index, (uint64_t)s.protospacer_start, (uint32_t)L, &proto[0]) != CALITAS_OK) die("fetching bases");
    if (s.pam_start >= 0 && calitas_fetch_bases(ctx, s.contig_index, (uint64_t)s.pam_start, s.pam_length, &pam[0]) != CALITAS_OK) die("fetching bases");
    proto = on_strand(proto, s.strand == '-'); pam_seqs[(size_t)i] = on_strand(pam, s.strand == '-');
    for (auto& c : proto) if (c == 'U') c = 'T';          // an ACGT guide
    protos[(size_t)i] = proto;
  }
  const bool five = pg.pam5 && !pg.pams.empty();
  auto count = [&](int64_t K, std::vector<uint64_t>& out) {
    std::string keys;
    for (const std::string& p : protos) keys += five ? p.substr(0, (size_t)K) : p.substr((size_t)(L - K));
    out.assign((size_t)n_sites + 1, 0);
    const uint64_t most = 1ull << 24;                     // what one call takes; the queries are independent: a call's worth at a time
    for (uint64_t at = 0; at < n_sites; at += most) {
      const uint64_t n = std::min(most, n_sites - at);
      const int rc2 = device < 0 ? calitas_count_copies_host(ctx, &g, (int32_t)K, -1, 0, 0, keys.data() + at * (uint64_t)K, n, out.data() + at)
                                 : calitas_count_copies(ctx, &g, (int32_t)K, -1, 0, 0, keys.data() + at * (uint64_t)K, n, out.data() + at);
      if (rc2 != CALITAS_OK) die("counting copies");
    }
  };
  std::vector<uint64_t> n_copies, n_seed;
  if (copies) count(L, n_copies);
  if (have_seed) count(seed_k, n_seed);
  // the whole protospacers within near_m substitutions (tools.py guide_near): rows of near_m + 1 counts; with --near-scores the one
  // scored pass gives them and the sums (tools.py guide_near_scores)
  const size_t near_row = (size_t)near_m + 1;
  std::vector<uint64_t> n_near;
  std::vector<calitas_near_score_t> near_sc;
  if (have_near_scores) {
    std::string keys;
    for (const std::string& p : protos) keys += p;
    n_near.assign(((size_t)n_sites + 1) * near_row, 0);
    near_sc.assign((size_t)n_sites + 1, calitas_near_score_t{0, 0});
    calitas_score_model_t m;
    m.protospacer_length = near_model.L; m.gap = near_model.gap; m.pam_mismatch = near_model.pam; m.mismatch = near_model.mm.data();
    const uint64_t most = 1ull << 24;
    for (uint64_t at = 0; at < n_sites; at += most) {
      const uint64_t n = std::min(most, n_sites - at);
      const int rc2 = device < 0 ? calitas_score_near_host(ctx, &g, (int32_t)near_m, &m, -1, 0, 0, keys.data() + at * (uint64_t)L, n, n_near.data() + at * near_row, near_sc.data() + at)
                                 : calitas_score_near(ctx, &g, (int32_t)near_m, &m, -1, 0, 0, keys.data() + at * (uint64_t)L, n, n_near.data() + at * near_row, near_sc.data() + at);
      if (rc2 != CALITAS_OK) die("scoring near copies");
    }
  } else if (have_near) {
    std::string keys;
    for (const std::string& p : protos) keys += p;
    n_near.assign(((size_t)n_sites + 1) * near_row, 0);
    const uint64_t most = 1ull << 24;
    for (uint64_t at = 0; at < n_sites; at += most) {
      const uint64_t n = std::min(most, n_sites - at);
      const int rc2 = device < 0 ? calitas_count_near_host(ctx, &g, (int32_t)L, (int32_t)near_m, -1, 0, 0, keys.data() + at * (uint64_t)L, n, n_near.data() + at * near_row)
                                 : calitas_count_near(ctx, &g, (int32_t)L, (int32_t)near_m, -1, 0, 0, keys.data() + at * (uint64_t)L, n, n_near.data() + at * near_row);
      if (rc2 != CALITAS_OK) die("counting near copies");
    }
  }
  uint64_t n_rows = 0;
  std::vector<uint64_t> kept;      // the rows written, for --near-list
  for (uint64_t i = 0; i < n_sites; i++) {
    if (have_max_near) {
      uint64_t sum = 0;
      for (size_t d = 0; d < near_row; d++) sum += n_near[(size_t)i * near_row + d];
      if (sum > (uint64_t)max_near) continue;
    }
    if (have_max && n_copies[(size_t)i] > (uint64_t)max_copies) continue;
    if (have_max_seed && n_seed[(size_t)i] > (uint64_t)max_seed_copies) continue;
    n_rows++;
    kept.push_back(i);
    const calitas_site_t& s = sites[i];
    const char* name; uint64_t len;
    calitas_contig_name(ctx, s.contig_index, &name, &len);
    const std::string &proto = protos[(size_t)i], &pam = pam_seqs[(size_t)i];
    const int64_t lo = s.pam_start < 0 ? s.protospacer_start : std::min<int64_t>(s.protospacer_start, s.pam_start);
    const int64_t hi = s.pam_start < 0 ? s.protospacer_start + L : std::max<int64_t>(s.protospacer_start + L, (int64_t)s.pam_start + s.pam_length);
    const std::string pat_pam = s.pam_index >= 0 ? pg.pams[(size_t)s.pam_index] : std::string();
    const std::string guide = pg.pam5 ? pat_pam + proto : proto + pat_pam;
    std::fprintf(f, "%s:%lld:%c\t%s\t%lld\t%lld\t%c\t%d\t%s\t%s", name, (long long)lo, (char)s.strand, name, (long long)lo, (long long)hi,
                 (char)s.strand, (int)s.pam_index, guide.c_str(), pam.c_str());
    if (have_regions) std::fprintf(f, "\t%s", classes[site_class[i]].c_str());
    if (have_activity && activity_q16[i] == CALITAS_ACTIVITY_NONE) std::fprintf(f, "\tNA\tNA");
    else if (have_activity) {
      const double x = (double)activity_q16[i] / 65536.0;
      std::fprintf(f, "\t%d\t%.6f", (int)activity_q16[i], act.link ? 1.0 / (1.0 + std::exp(-x)) : x);
    }
    if (have_mh && mh_q16[i].total_q16 == CALITAS_MH_NONE) std::fprintf(f, "\tNA\tNA\tNA\tNA");
    else if (have_mh) {
      const double total = (double)mh_q16[i].total_q16, oof = (double)mh_q16[i].out_of_frame_q16;
      std::fprintf(f, "\t%u\t%u\t%.3f", (unsigned)mh_q16[i].total_q16, (unsigned)mh_q16[i].out_of_frame_q16, 100.0 * total / 65536.0);
      if (mh_q16[i].total_q16) std::fprintf(f, "\t%.2f", 100.0 * oof / total);
      else std::fprintf(f, "\tNA");
    }
    if (copies) std::fprintf(f, "\t%llu", (unsigned long long)n_copies[(size_t)i]);
    if (have_seed) std::fprintf(f, "\t%llu", (unsigned long long)n_seed[(size_t)i]);
    for (size_t d = 0; have_near && d < near_row; d++) std::fprintf(f, "\t%llu", (unsigned long long)n_near[(size_t)i * near_row + d]);
    if (have_near_scores)
      std::fprintf(f, "\t%llu\t%llu\t%.6f", (unsigned long long)near_sc[(size_t)i].sum_q32, (unsigned long long)near_sc[(size_t)i].max_q32,
                   4294967296.0 / (4294967296.0 + (double)near_sc[(size_t)i].sum_q32));
    std::fprintf(f, "\n");
  }
  if (f != stdout) std::fclose(f);
  // the kept rows' copies within near_m substitutions, a line per record (tools.py guide_near_list, near_list_tsv)
  if (have_near_list) {
    FILE* lf = std::fopen(near_list.c_str(), "w");
    if (!lf) { std::fprintf(stderr, "cannot write %s\n", near_list.c_str()); calitas_free(sites); calitas_destroy(ctx); return 1; }
    std::fprintf(lf, "guide_id\tchromosome\tstart\tend\tstrand\tpam_index\tmismatches\ttarget\tscore_q32\tscore\n");
    if (kept.size() > (1ull << 24)) { std::fprintf(stderr, "calitas: more than 16777216 guides: list them in pieces\n"); calitas_free(sites); calitas_destroy(ctx); return 1; }
    std::string keys;
    for (uint64_t i : kept) keys += protos[(size_t)i];
    std::vector<uint64_t> l_near((kept.size() + 1) * near_row, 0), l_off(kept.size() + 1, 0);
    calitas_score_model_t m;
    m.protospacer_length = near_model.L; m.gap = near_model.gap; m.pam_mismatch = near_model.pam; m.mismatch = near_model.mm.data();
    calitas_near_hit_t* found = nullptr; uint64_t n_found = 0;
    const int rc2 = device < 0 ? calitas_list_near_host(ctx, &g, (int32_t)near_m, have_near_scores ? &m : nullptr, -1, 0, 0, keys.data(), kept.size(), (uint32_t)near_list_limit,
                                                        l_near.data(), l_off.data(), &found, &n_found)
                               : calitas_list_near(ctx, &g, (int32_t)near_m, have_near_scores ? &m : nullptr, -1, 0, 0, keys.data(), kept.size(), (uint32_t)near_list_limit,
                                                   l_near.data(), l_off.data(), &found, &n_found);
    if (rc2 != CALITAS_OK) die("listing near copies");
    for (size_t r = 0; r < kept.size(); r++) {
      const calitas_site_t& s = sites[kept[r]];
      const char* name; uint64_t len;
      calitas_contig_name(ctx, s.contig_index, &name, &len);
      const int64_t lo = s.pam_start < 0 ? s.protospacer_start : std::min<int64_t>(s.protospacer_start, s.pam_start);
      for (uint64_t at = l_off[r]; at < l_off[r + 1]; at++) {
        const calitas_near_hit_t& h = found[at];
        const char* where; uint64_t where_len;
        calitas_contig_name(ctx, h.contig_index, &where, &where_len);
        std::string target((size_t)L, 'N');
        for (int64_t b = 0; b < L; b++) {
          const char c = "ACGT"[((h.target_lo >> b) & 1u) | (((h.target_hi >> b) & 1u) << 1)];
          target[(size_t)b] = ((h.diff_mask >> b) & 1u) ? (char)std::tolower((unsigned char)c) : c;
        }
        std::fprintf(lf, "%s:%lld:%c\t%s\t%lld\t%lld\t%c\t%d\t%u\t%s\t%llu\t%.6f\n", name, (long long)lo, (char)s.strand, where, (long long)h.protospacer_start,
                     (long long)h.protospacer_start + (long long)L, (char)h.strand, (int)h.pam_index, (unsigned)h.mismatches, target.c_str(),
                     (unsigned long long)h.score_q32, (double)h.score_q32 / 4294967296.0);
      }
    }
    calitas_free(found);
    std::fclose(lf);
  }
  // the pairs of the kept rows (tools.py guide_pairs, pairs_tsv): the region's listing paired in one call, joined to the rows on
  // (contig, protospacer start, strand) in one walk -- both are in that order -- and a pair written when both members are rows
  if (have_pairs) {
    FILE* pf = std::fopen(pairs_path.c_str(), "w");
    if (!pf) { std::fprintf(stderr, "cannot write %s\n", pairs_path.c_str()); calitas_free(sites); calitas_free(activity_q16); calitas_free(site_class); calitas_destroy(ctx); return 1; }
    std::fprintf(pf, "pair_id\tleft_guide_id\tright_guide_id\tchromosome\tleft_cut\tright_cut\tdistance\tleft_strand\tright_strand\torientation\n");
    calitas_site_t* listed = nullptr; uint64_t n_listed = 0;
    calitas_site_pair_t* found = nullptr; uint64_t n_found = 0;
    const int rc2 = device < 0 ? calitas_find_site_pairs_host(ctx, &g, keep, &pair_rule, chrom_index, start, end, &listed, &n_listed, &found, &n_found)
                               : calitas_find_site_pairs(ctx, &g, keep, &pair_rule, chrom_index, start, end, &listed, &n_listed, &found, &n_found);
    if (rc2 != CALITAS_OK) die("pairing sites");
    const auto less = [](const calitas_site_t& x, const calitas_site_t& y) {
      if (x.contig_index != y.contig_index) return x.contig_index < y.contig_index;
      if (x.protospacer_start != y.protospacer_start) return x.protospacer_start < y.protospacer_start;
      return x.strand == '+' && y.strand == '-';
    };
    const uint64_t no_row = ~0ull;
    std::vector<uint64_t> row_of((size_t)n_listed, no_row);
    for (uint64_t i = 0, r = 0; i < n_listed; i++) {
      while (r < kept.size() && less(sites[kept[r]], listed[i])) r++;
      if (r < kept.size() && !less(listed[i], sites[kept[r]])) row_of[(size_t)i] = kept[r];
    }
    const auto id_of = [&](const calitas_site_t& s, const char* name) {
      const int64_t lo = s.pam_start < 0 ? s.protospacer_start : std::min<int64_t>(s.protospacer_start, s.pam_start);
      return std::string(name) + ":" + std::to_string((long long)lo) + ":" + (char)s.strand;
    };
    const auto cut_of = [&](const calitas_site_t& s) { return (long long)s.protospacer_start + (s.strand == '-' ? L - pair_rule.cut_offset : (int64_t)pair_rule.cut_offset); };
    uint64_t pair_id = 0;
    for (uint64_t k = 0; k < n_found; k++) {
      const uint64_t a = row_of[found[k].left], b = row_of[found[k].right];
      if (a == no_row || b == no_row) continue;
      const calitas_site_t &left = sites[a], &right = sites[b];
      const char* name; uint64_t len;
      calitas_contig_name(ctx, left.contig_index, &name, &len);
      const unsigned o = found[k].orientation;
      static const char* const codes[4] = {"++", "-+", "+-", "--"};
      const char* called = !pattern_has_pam ? codes[o & 3u] : (o == 0 || o == 3) ? "same" : ((o == 1) == three_prime) ? "out" : "in";
      std::fprintf(pf, "%llu\t%s\t%s\t%s\t%lld\t%lld\t%d\t%c\t%c\t%s\n", (unsigned long long)++pair_id, id_of(left, name).c_str(), id_of(right, name).c_str(), name,
                   cut_of(left), cut_of(right), (int)found[k].distance, (char)left.strand, (char)right.strand, called);
    }
    calitas_free(listed); calitas_free(found);
    std::fclose(pf);
  }
  // the sites the VCF's SNVs create, destroy or change (tools.py snvs_of_vcf, allele_sites_tool, allele_sites_tsv)
  if (have_alleles) {
    char* text = nullptr; uint64_t n_records = 0;
    if (calitas_vcf_records(ctx, alleles_path.c_str(), nullptr, &text, &n_records) != CALITAS_OK) die("reading the VCF");
    struct SnvRow { std::string chrom, id, ref, alt; long long pos1; };
    std::vector<SnvRow> snv_rows;
    std::vector<calitas_snv_t> snvs;
    unsigned long long other = 0, lacks = 0, beyond = 0;
    int32_t n_contigs = 0; calitas_reference_info(ctx, &n_contigs, nullptr, nullptr);
    for (const char* line = text; *line;) {
      const char* eol = std::strchr(line, '\n');
      if (!eol) eol = line + std::strlen(line);
      std::vector<std::string> fld;
      for (const char* at = line;;) {
        const char* tab = (const char*)std::memchr(at, '\t', (size_t)(eol - at));
        fld.emplace_back(at, tab ? tab : eol);
        if (!tab) break;
        at = tab + 1;
      }
      line = *eol ? eol + 1 : eol;
      if (fld.size() < 6) continue;
      int32_t ci = -1; uint64_t len = 0;
      for (int32_t i = 0; i < n_contigs && ci < 0; i++) { const char* nm; uint64_t l; calitas_contig_name(ctx, i, &nm, &l); if (fld[0] == nm) { ci = i; len = l; } }
      if (ci < 0) { lacks++; continue; }
      const long long pos1 = std::atoll(fld[1].c_str());
      if ((chrom_index >= 0 && ci != chrom_index) || pos1 - 1 < (long long)start || (end != 0 && pos1 - 1 >= (long long)end)) continue;
      const std::string& ref_allele = fld[4];
      for (size_t at = 0; at <= fld[5].size();) {
        size_t comma = fld[5].find(',', at);
        if (comma == std::string::npos) comma = fld[5].size();
        const std::string alt = fld[5].substr(at, comma - at);
        at = comma + 1;
        const auto base = [](const std::string& t) { return t.size() == 1 && std::strchr("ACGT", t[0]) != nullptr; };
        if (!base(ref_allele) || !base(alt)) other++;
        else if ((uint64_t)pos1 > len) beyond++;
        else {
          snv_rows.push_back(SnvRow{fld[0], fld[3], ref_allele, alt, pos1});
          snvs.push_back(calitas_snv_t{ci, (int32_t)(pos1 - 1), ref_allele[0], alt[0], 0});
        }
      }
    }
    calitas_free(text);
    if (have_allele_sites) {
      calitas_allele_site_t* found = nullptr; uint64_t n_found = 0;
      std::vector<uint8_t> status(snvs.size() + 1, 0);
      const int rc2 = device < 0 ? calitas_find_allele_sites_host(ctx, &g, snvs.data(), snvs.size(), &found, &n_found, status.data())
                                 : calitas_find_allele_sites(ctx, &g, snvs.data(), snvs.size(), &found, &n_found, status.data());
      if (rc2 != CALITAS_OK) die("finding allele sites");
      FILE* af = std::fopen(allele_sites_path.c_str(), "w");
      if (!af) { std::fprintf(stderr, "cannot write %s\n", allele_sites_path.c_str()); calitas_free(found); calitas_free(sites); calitas_free(activity_q16); calitas_free(site_class); calitas_destroy(ctx); return 1; }
      std::fprintf(af, "chromosome\tposition\tid\tref\talt\tallele\tstart\tend\tstrand\tpam_index\tsnv_offset\tguide\tpam_sequence\tother_pam_index\n");
      static const char* const kind_names[4] = {"", "alt", "ref", "both"};
      for (uint64_t k = 0; k < n_found; k++) {
        const calitas_allele_site_t& r = found[k];
        if (!((kinds_wanted >> r.kind) & 1u)) continue;
        const calitas_site_t& s = r.site;
        const SnvRow& v = snv_rows[r.snv_index];
        const int64_t lo = s.pam_start < 0 ? s.protospacer_start : std::min<int64_t>(s.protospacer_start, s.pam_start);
        const int64_t hi = s.pam_start < 0 ? s.protospacer_start + L : std::max<int64_t>(s.protospacer_start + L, (int64_t)s.pam_start + s.pam_length);
        std::string proto((size_t)L, 'N'), pam((size_t)s.pam_length, 'N');
        for (int64_t i = 0; i < L; i++) proto[(size_t)i] = "ACGT"[((r.guide_lo >> i) & 1u) | (((r.guide_hi >> i) & 1u) << 1)];
        if (s.pam_start >= 0 && s.pam_length) {
          if (calitas_fetch_bases(ctx, s.contig_index, (uint64_t)s.pam_start, s.pam_length, &pam[0]) != CALITAS_OK) die("fetching bases");
          if (r.kind != 2 && v.pos1 - 1 >= s.pam_start && v.pos1 - 1 < (long long)s.pam_start + s.pam_length) pam[(size_t)(v.pos1 - 1 - s.pam_start)] = v.alt[0];
          pam = on_strand(pam, s.strand == '-');
          for (auto& c : pam) if (c == 'U') c = 'T';
        }
        const std::string pattern_pam = s.pam_index >= 0 ? pg.pams[(size_t)s.pam_index] : std::string();
        const std::string guide = five ? pattern_pam + proto : proto + pattern_pam;
        std::fprintf(af, "%s\t%lld\t%s\t%s\t%s\t%s\t%lld\t%lld\t%c\t%d\t%d\t%s\t%s\t", v.chrom.c_str(), v.pos1, v.id.empty() ? "." : v.id.c_str(), v.ref.c_str(),
                     v.alt.c_str(), kind_names[r.kind & 3u], (long long)lo, (long long)hi, (char)s.strand, (int)s.pam_index, (int)r.guide_offset, guide.c_str(), pam.c_str());
        if (r.kind == 3) std::fprintf(af, "%d\n", (int)r.other_pam_index); else std::fprintf(af, ".\n");
      }
      std::fclose(af);
      unsigned long long by[4] = {0, 0, 0, 0};
      for (size_t i = 0; i < snvs.size(); i++) by[status[i] & 3u]++;
      std::fprintf(stderr, "alleles: %llu SNVs examined, %llu records; skipped: %llu other alleles, %llu records on chromosomes the reference lacks, %llu beyond a contig's end, "
                           "%llu with another REF than the reference, %llu on a base that is not A C G T, %llu with ALT equal to the reference\n",
                   by[0], (unsigned long long)n_found, other, lacks, beyond, by[1], by[2], by[3]);
      calitas_free(found);
    }
    // the guides that put the SNVs into the base editor's window (tools.py edit_sites_tool, edit_sites_tsv)
    if (have_edit_sites) {
      calitas_edit_site_t* found = nullptr; uint64_t n_found = 0;
      std::vector<uint8_t> status(snvs.size() + 1, 0);
      const int rc2 = device < 0 ? calitas_find_edit_sites_host(ctx, &g, &edit, snvs.data(), snvs.size(), &found, &n_found, status.data())
                                 : calitas_find_edit_sites(ctx, &g, &edit, snvs.data(), snvs.size(), &found, &n_found, status.data());
      if (rc2 != CALITAS_OK) die("finding edit sites");
      FILE* ef = std::fopen(edit_sites_path.c_str(), "w");
      if (!ef) { std::fprintf(stderr, "cannot write %s\n", edit_sites_path.c_str()); calitas_free(found); calitas_free(sites); calitas_free(activity_q16); calitas_free(site_class); calitas_destroy(ctx); return 1; }
      std::fprintf(ef, "chromosome\tposition\tid\tref\talt\tmode\tstart\tend\tstrand\tpam_index\tedit_offset\tguide\tpam_sequence\tbystanders\tbystander_offsets\tedited\n");
      const char product = (char)std::tolower((unsigned char)edit.to_base);
      for (uint64_t k = 0; k < n_found; k++) {
        const calitas_edit_site_t& r = found[k];
        const calitas_site_t& s = r.site;
        const SnvRow& v = snv_rows[r.snv_index];
        const int64_t lo = s.pam_start < 0 ? s.protospacer_start : std::min<int64_t>(s.protospacer_start, s.pam_start);
        const int64_t hi = s.pam_start < 0 ? s.protospacer_start + L : std::max<int64_t>(s.protospacer_start + L, (int64_t)s.pam_start + s.pam_length);
        const int offset = (int)(s.strand == '-' ? s.protospacer_start + L - 1 - (v.pos1 - 1) : (v.pos1 - 1) - s.protospacer_start);
        std::string proto((size_t)L, 'N'), pam((size_t)s.pam_length, 'N'), offsets;
        for (int64_t i = 0; i < L; i++) proto[(size_t)i] = "ACGT"[((r.guide_lo >> i) & 1u) | (((r.guide_hi >> i) & 1u) << 1)];
        std::string edited = proto;
        int bystanders = 0;
        for (int i = 0; i < (int)L; i++) {
          if (!((r.editable >> i) & 1u)) continue;
          edited[(size_t)i] = product;
          if (i == offset) continue;
          offsets += (bystanders++ ? "," : "") + std::to_string(i);
        }
        if (s.pam_start >= 0 && s.pam_length) {
          if (calitas_fetch_bases(ctx, s.contig_index, (uint64_t)s.pam_start, s.pam_length, &pam[0]) != CALITAS_OK) die("fetching bases");
          pam = on_strand(pam, s.strand == '-');
          for (auto& c : pam) if (c == 'U') c = 'T';
        }
        const std::string pattern_pam = s.pam_index >= 0 ? pg.pams[(size_t)s.pam_index] : std::string();
        const std::string guide = five ? pattern_pam + proto : proto + pattern_pam;
        std::fprintf(ef, "%s\t%lld\t%s\t%s\t%s\t%s\t%lld\t%lld\t%c\t%d\t%d\t%s\t%s\t%d\t%s\t%s\n", v.chrom.c_str(), v.pos1, v.id.empty() ? "." : v.id.c_str(),
                     v.ref.c_str(), v.alt.c_str(), edit.correct ? "correct" : "install", (long long)lo, (long long)hi, (char)s.strand, (int)s.pam_index, offset,
                     guide.c_str(), pam.c_str(), bystanders, offsets.empty() ? "." : offsets.c_str(), edited.c_str());
      }
      std::fclose(ef);
      unsigned long long by[6] = {0, 0, 0, 0, 0, 0};
      for (size_t i = 0; i < snvs.size(); i++) by[status[i] < 6 ? status[i] : 0]++;
      std::fprintf(stderr, "edits: %llu SNVs examined, %llu records; skipped: %llu other alleles, %llu records on chromosomes the reference lacks, %llu beyond a contig's end, "
                           "%llu with another REF than the reference, %llu on a base that is not A C G T, %llu with ALT equal to the reference, "
                           "%llu that are not the editor's change, %llu whose 5' neighbour fails the context\n",
                   by[0], (unsigned long long)n_found, other, lacks, beyond, by[1], by[2], by[3], by[4], by[5]);
      calitas_free(found);
    }
  }
  std::fprintf(stderr, "calitas: %llu guides\n", (unsigned long long)n_rows);
  calitas_free(sites); calitas_free(activity_q16); calitas_free(site_class); calitas_free(mh_q16); calitas_destroy(ctx);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::strcmp(argv[1], "FindGuides") == 0) return find_guides_main(argc, argv);
  if (argc < 2 || std::strcmp(argv[1], "SearchReference") != 0) { usage(); return 2; }
  std::string guide, guide_id, ref, output, chrom, variants, scores;
  std::vector<std::string> aux;
  calitas_params_t p{};
  p.window_size = 1000; p.max_guide_diffs = 5; p.max_pam_mismatches = 1; p.max_gaps_between_guide_and_pam = 3; p.max_total_diffs = -1;
  p.max_overlap = 10; p.guide_mismatch_net_cost = -120; p.pam_mismatch_net_cost = -260; p.genome_gap_net_cost = -122;
  p.guide_gap_net_cost = -121; p.chrom_index = -1; p.eqx_by_score = 0; p.max_variants = 16;
  int device = 0;
  bool counts = false;
  int top_k = -1;              // --top K: with --scores, the K highest-scoring imperfect hits behind the scores
  std::string regions_path, top_classes;   // --regions FILE.bed [--top-classes name,...]: with --scores, the same split by the file's classes
  bool have_top_classes = false;
  for (int i = 2; i < argc; i++) {
    std::string a = argv[i], val;
    size_t eq = a.find('=');
    if (a.compare(0, 2, "--") == 0 && eq != std::string::npos) { val = a.substr(eq + 1); a = a.substr(0, eq); }
    a = long_to_short(a);
    auto next = [&]() -> std::string {
      if (!val.empty()) return val;
      if (i + 1 >= argc) { usage(); std::exit(2); }
      return argv[++i];
    };
    if (a == "-i") guide = next();
    else if (a == "-I") guide_id = next();
    else if (a == "-r") ref = next();
    else if (a == "-o") output = next();
    else if (a == "-c") chrom = next();
    else if (a == "-x") { aux.push_back(next()); while (i + 1 < argc && argv[i + 1][0] != '-') aux.push_back(argv[++i]); }
    else if (a == "-w") p.window_size = std::atoi(next().c_str());
    else if (a == "-d") p.max_guide_diffs = std::atoi(next().c_str());
    else if (a == "-p") p.max_pam_mismatches = std::atoi(next().c_str());
    else if (a == "-g") p.max_gaps_between_guide_and_pam = std::atoi(next().c_str());
    else if (a == "-D") p.max_total_diffs = std::atoi(next().c_str());
    else if (a == "-O") p.max_overlap = std::atoi(next().c_str());
    else if (a == "-m") p.guide_mismatch_net_cost = std::atoi(next().c_str());
    else if (a == "-M") p.pam_mismatch_net_cost = std::atoi(next().c_str());
    else if (a == "-b") p.genome_gap_net_cost = std::atoi(next().c_str());
    else if (a == "-B") p.guide_gap_net_cost = std::atoi(next().c_str());
    else if (a == "-V") p.max_variants = std::atoi(next().c_str());
    else if (a == "-t") (void)next();
    else if (a == "--device") device = std::atoi(next().c_str());
    else if (a == "--counts") counts = true;
    else if (a == "--scores") scores = next();
    else if (a == "--top") top_k = std::atoi(next().c_str());
    else if (a == "--regions") regions_path = next();
    else if (a == "--top-classes") { top_classes = next(); have_top_classes = true; }
    else if (a == "-v") variants = next();
    else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); usage(); return 2; }
  }
  if (guide.empty() || guide_id.empty() || ref.empty()) { usage(); return 2; }
  if (counts && !variants.empty()) { std::fprintf(stderr, "--counts covers the reference-genome branch only (no --variants)\n"); return 2; }
  if (!scores.empty() && !variants.empty()) { std::fprintf(stderr, "--scores covers the reference-genome branch only (no --variants)\n"); return 2; }
  if (top_k != -1 && scores.empty()) { std::fprintf(stderr, "--top K requires --scores MODEL\n"); return 2; }
  if (top_k != -1 && (top_k < 1 || top_k > CALITAS_TOP_MAX)) { std::fprintf(stderr, "--top K: K is 1 .. %d\n", CALITAS_TOP_MAX); return 2; }
  if (!regions_path.empty() && scores.empty()) { std::fprintf(stderr, "--regions FILE.bed requires --scores MODEL\n"); return 2; }
  if (!regions_path.empty() && !variants.empty()) { std::fprintf(stderr, "--regions covers the reference-genome branch only (no --variants)\n"); return 2; }
  if (have_top_classes && (regions_path.empty() || top_k == -1)) { std::fprintf(stderr, "--top-classes requires --regions and --top\n"); return 2; }
  ScoreModelFile model;
  if (!scores.empty()) {
    std::string err;
    if (!read_score_model(scores, model, err)) { std::fprintf(stderr, "calitas: %s\n", err.c_str()); return 2; }
  }

  ParsedGuide pg;
  if (int rc = parse_guide(guide, aux, pg)) return rc;
  calitas_guide_t g = pg.c_guide();

  calitas_ctx* ctx = nullptr;
  if (calitas_create(device, &ctx) != CALITAS_OK) { std::fprintf(stderr, "calitas: %s\n", calitas_last_error(nullptr)); return 1; }
  auto die = [&](const char* what) { std::fprintf(stderr, "calitas: %s: %s\n", what, calitas_last_error(ctx)); calitas_destroy(ctx); std::exit(1); };
  if (calitas_set_reference_fasta(ctx, ref.c_str()) != CALITAS_OK) die("reading reference");
  if (!chrom.empty()) {
    int32_t n = 0; calitas_reference_info(ctx, &n, nullptr, nullptr);
    for (int32_t i = 0; i < n; i++) { const char* nm; uint64_t len; calitas_contig_name(ctx, i, &nm, &len); if (chrom == nm) p.chrom_index = i; }
    if (p.chrom_index < 0) { std::fprintf(stderr, "Unknown chromosome: %s\n", chrom.c_str()); calitas_destroy(ctx); return 1; }
  }
  char* tsv = nullptr; uint64_t rows = 0, bytes = 0;
  if (!variants.empty()) {   // SearchReference.scala:570-630
    uint64_t windows = 0;
    if (calitas_search_variants(ctx, &g, guide_id.c_str(), &p, variants.c_str(), chrom.empty() ? nullptr : chrom.c_str(), nullptr, nullptr, nullptr,
                                &tsv, &bytes, &rows, &windows) != CALITAS_OK) die("search with variants");
    std::fprintf(stderr, "calitas: %llu variant windows\n", (unsigned long long)windows);
  }
  FILE* f = output.empty() ? stdout : std::fopen(output.c_str(), "w");
  if (!f) { std::fprintf(stderr, "cannot write %s\n", output.c_str()); return 1; }
  auto write_counts = [&](const calitas_counts_t* t) {     // the non-zero cells in table order
    std::fprintf(f, "guide_id\tstrand\tguide_mm\tguide_gaps\tpam_mm\thits\n");
    uint64_t cell = 0;
    for (uint32_t s = 0; s < 2; s++)
      for (uint32_t m = 0; m < t->n_mm; m++)
        for (uint32_t gp = 0; gp < t->n_gaps; gp++)
          for (uint32_t pm = 0; pm < t->n_pam; pm++, cell++)
            if (t->counts[cell]) std::fprintf(f, "%s\t%c\t%u\t%u\t%u\t%llu\n", guide_id.c_str(), s ? '-' : '+', m, gp, pm, (unsigned long long)t->counts[cell]);
  };
  if (!scores.empty()) {      // the specificity score instead of hits.txt; with --counts the same pass's table behind an empty line
    const calitas_score_model_t cm{model.L, model.gap, model.pam, model.mm.data()};
    calitas_scores_t* sc = nullptr;
    calitas_top_t* tp = nullptr;                            // --top K: the same pass with the list; its scores are the scores
    calitas_regions_t* rg = nullptr;                        // --regions: the same pass split by the file's classes; its top is the top
    std::vector<std::string> classes;
    if (!regions_path.empty()) {
      std::string err;
      uint32_t mask = 0xFFFFFFFFu;
      if (!set_regions_from_bed(ctx, regions_path, classes, err) ||
          (have_top_classes && !class_mask(classes, top_classes, mask, err))) { std::fprintf(stderr, "%s\n", err.c_str()); return 2; }
      if (calitas_search_regions(ctx, &g, &p, &cm, top_k > 0 ? (uint32_t)top_k : 0u, mask, &rg) != CALITAS_OK) die("search");
      sc = &rg->top.scores;
      if (top_k > 0) tp = &rg->top;
    } else if (top_k > 0) {
      if (calitas_search_top(ctx, &g, &p, &cm, (uint32_t)top_k, &tp) != CALITAS_OK) die("search");
      sc = &tp->scores;
    } else if (calitas_search_scores(ctx, &g, &p, &cm, &sc) != CALITAS_OK) die("search");
    const double two32 = 4294967296.0;
    std::fprintf(f, "guide_id\trows\tperfect\tofftarget_sum_q32\tmax_q32\tspecificity\n%s\t%llu\t%llu\t%llu\t%llu\t%.6f\n", guide_id.c_str(),
                 (unsigned long long)sc->rows, (unsigned long long)sc->perfect, (unsigned long long)sc->sum_q32, (unsigned long long)sc->max_q32,
                 two32 / (two32 + (double)sc->sum_q32));
    if (rg) {
      std::fprintf(f, "\nguide_id\tclass\trows\tperfect\tofftarget_sum_q32\tmax_q32\tspecificity\n");
      for (uint32_t c = 0; c < rg->n_classes; c++) {
        const calitas_scores_t& s = rg->by_class[c];
        std::fprintf(f, "%s\t%s\t%llu\t%llu\t%llu\t%llu\t%.6f\n", guide_id.c_str(), classes[c].c_str(), (unsigned long long)s.rows,
                     (unsigned long long)s.perfect, (unsigned long long)s.sum_q32, (unsigned long long)s.max_q32, two32 / (two32 + (double)s.sum_q32));
      }
    }
    if (tp) {
      std::fprintf(f, "\nguide_id\trank\tchromosome\tcoordinate_start\tcoordinate_end\tstrand\tguide_mm\tguide_gaps\tpam_mm\tscore_q32\tscore%s\n", rg ? "\tclass" : "");
      for (uint32_t i = 0; i < tp->n; i++) {
        const calitas_top_hit_t& h = tp->hits[i];
        const char* nm = ""; uint64_t len = 0;
        calitas_contig_name(ctx, h.contig_index, &nm, &len);
        std::fprintf(f, "%s\t%u\t%s\t%d\t%d\t%c\t%u\t%u\t%u\t%llu\t%.6f", guide_id.c_str(), i + 1, nm, h.coordinate_start, h.coordinate_end, (char)h.strand,
                     (unsigned)h.guide_mm, (unsigned)h.guide_gaps, (unsigned)h.pam_mm, (unsigned long long)h.score_q32, (double)h.score_q32 / two32);
        if (rg) std::fprintf(f, "\t%s", classes[rg->hit_class[i]].c_str());
        std::fprintf(f, "\n");
      }
    }
    if (counts) { std::fprintf(f, "\n"); write_counts(&sc->table); }
    rows = sc->rows;
    calitas_free(rg ? (void*)rg : tp ? (void*)tp : (void*)sc);
  } else if (counts) {        // the off-target table instead of hits.txt
    calitas_counts_t* t = nullptr;
    if (calitas_search_counts(ctx, &g, &p, &t) != CALITAS_OK) die("search");
    write_counts(t);
    rows = t->rows;
    calitas_free(t);
  } else if (variants.empty()) {     // straight to the file: a hits.txt of tens of gigabytes (PAM-less, many diffs) is never held in memory
    auto to_file = [](const char* piece, uint64_t n, void* user) -> int { return std::fwrite(piece, 1, n, (FILE*)user) == n ? 0 : 1; };
    if (calitas_search_hits_stream(ctx, &g, guide_id.c_str(), &p, nullptr, nullptr, to_file, f, &bytes, &rows) != CALITAS_OK) die("search");
  } else std::fwrite(tsv, 1, bytes, f);
  if (f != stdout) std::fclose(f);
  calitas_timing_t tm; calitas_get_timing(ctx, &tm);
  std::fprintf(stderr, "calitas: %llu hits; scan %.3f ms, align %.3f ms, filter + rows %.3f ms, text copy %.3f ms (%u lane%s)\n",
               (unsigned long long)rows, tm.scan_kernel_ms, tm.align_kernel_ms, tm.hits_kernel_ms, tm.hits_copy_ms, tm.lanes, tm.lanes == 1 ? "" : "s");
  calitas_free(tsv); calitas_destroy(ctx);
  return 0;
}
