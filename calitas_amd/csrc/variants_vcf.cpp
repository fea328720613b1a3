// variants_vcf.cpp -- what the variant search knows about a VCF: its records (read_vcf: the file parsed on the worker pool and published
// wave by wave) and its identifier "name:md5" (ReferenceHit.scala:175-183), and the two C entry points that give both on their own.
// None of it has a counterpart in the reference, which reads its VCF through fgbio.
//
// VCF support is the subset the reference's path needs (fgbio vcf.api): CHROM POS ID REF ALT FILTER INFO(AF, END); plain or gzip.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>

#include "variants_internal.hpp"

namespace calitas __attribute__((visibility("hidden"))) {

namespace {

// strtod of p[0..n) for the numbers a VCF's AF holds.  Plain decimals of at most 15 significant digits and 22 decimal places are an
// integer below 2^53 divided by a power of ten that a double holds exactly: one correctly rounded division, the very double strtod
// returns (Clinger's fast path).  Everything else -- exponents, longer digit strings, inf / nan, blanks -- goes to strtod itself.
double parse_decimal(const char* p, size_t n) {
  static const double kPow10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  size_t i = 0;
  bool neg = false;
  if (i < n && (p[i] == '-' || p[i] == '+')) { neg = p[i] == '-'; i++; }
  uint64_t m = 0;
  int digits = 0, frac = 0;
  bool dot = false, any = false, simple = true;
  for (; i < n; i++) {
    const char c = p[i];
    if (c >= '0' && c <= '9') {
      any = true;
      if (m != 0 || c != '0') digits++;
      if (digits > 15) { simple = false; break; }
      m = m * 10 + (uint64_t)(c - '0');
      if (dot) frac++;
    } else if (c == '.' && !dot) dot = true;
    else { simple = false; break; }
  }
  if (simple && any && frac <= 22) {
    const double v = (double)m / kPow10[frac];
    return neg ? -v : v;
  }
  char num[64];
  const size_t cl = std::min(n, sizeof(num) - 1);
  std::memcpy(num, p, cl); num[cl] = 0;
  return std::strtod(num, nullptr);
}

// One VCF record (a line without its newline) -> v; false for headers, short lines and other chromosomes (read_vcf of variants.py).
bool parse_record(const char* b, const char* e, const char* chrom, size_t chrom_len, Var& v) {
  if (b >= e || *b == '#') return false;
  // fields 0-4 and 7 (CHROM POS ID REF ALT . . INFO), located in place
  const char* f0[9]; size_t fl[9]; int nf = 0;
  while (nf < 9) {
    const char* t = (const char*)std::memchr(b, '\t', (size_t)(e - b));
    f0[nf] = b; fl[nf] = (size_t)((t ? t : e) - b); nf++;
    if (!t) break;
    b = t + 1;
  }
  if (nf < 5 || (chrom && (fl[0] != chrom_len || std::memcmp(f0[0], chrom, fl[0]) != 0))) return false;
  // (everything in place: three million records per call at full size, and a temporary string per field -- the INFO column's entries
  // above all -- was most of the quarter second the file took)
  auto to_int = [](const char* p, size_t n) -> int {            // atoi of p[0..n): blanks, a sign, digits
    size_t i = 0;
    while (i < n && (p[i] == ' ' || (p[i] >= '\t' && p[i] <= '\r'))) i++;
    bool neg = false;
    if (i < n && (p[i] == '-' || p[i] == '+')) { neg = p[i] == '-'; i++; }
    long v = 0;
    while (i < n && p[i] >= '0' && p[i] <= '9') { v = v * 10 + (p[i] - '0'); i++; }
    return (int)(neg ? -v : v);
  };
  v.chrom.assign(f0[0], fl[0]);
  v.pos = to_int(f0[1], fl[1]);
  if (!(fl[2] == 1 && f0[2][0] == '.')) v.id.assign(f0[2], fl[2]);
  v.ref.assign(f0[3], fl[3]);
  {
    const char* a0 = f0[4];
    const char* const ae = f0[4] + fl[4];
    for (;;) {                                                  // split(ALT, ','): an empty ALT is one empty allele
      const char* c = (const char*)std::memchr(a0, ',', (size_t)(ae - a0));
      v.alts.emplace_back(a0, (size_t)((c ? c : ae) - a0));
      if (!c) break;
      a0 = c + 1;
    }
  }
  bool have_end = false;
  if (nf > 7) {
    const char* k0 = f0[7];
    const char* const ie = f0[7] + fl[7];
    for (;;) {                                                  // the INFO column's entries, ';' between them
      const char* sc = (const char*)std::memchr(k0, ';', (size_t)(ie - k0));
      const char* const ke = sc ? sc : ie;
      const size_t kl = (size_t)(ke - k0);
      if (kl >= 3 && std::memcmp(k0, "AF=", 3) == 0) {
        v.afs.clear();
        const char* x0 = k0 + 3;
        for (;;) {                                              // values between commas; "." and nothing are no value
          const char* c = (const char*)std::memchr(x0, ',', (size_t)(ke - x0));
          const char* const xe = c ? c : ke;
          const size_t xl = (size_t)(xe - x0);
          if (xl != 0 && !(xl == 1 && x0[0] == '.')) v.afs.push_back((float)parse_decimal(x0, xl));
          if (!c) break;
          x0 = c + 1;
        }
      } else if (kl >= 4 && std::memcmp(k0, "END=", 4) == 0) {
        v.end = to_int(k0 + 4, kl - 4); have_end = true;
      }
      if (!sc) break;
      k0 = sc + 1;
    }
  }
  if (!have_end) v.end = v.pos + (int)v.ref.size() - 1;
  return true;
}

}  // namespace

// The whole file in memory (gzip through zlib), then the lines parsed on the worker pool: every worker takes the lines that
// start in its byte range, and the per-worker lists are joined in file order.
std::string read_vcf(const char* path, const char* chrom, WorkerPool* pool, VarTable& out) {
  const auto t_read = Clock::now();
  std::string data;
  bool plain = false;
  // a plain file is mapped and parsed where the page cache has it (reading it into a block of the call's own was 37 ms of one thread
  // per 127 MB before the first record was looked at; zlib's transparent mode copies at ~1 GB/s)
  struct Mapping { void* p = MAP_FAILED; size_t n = 0; ~Mapping() { if (p != MAP_FAILED) (void)munmap(p, n); } } map;
  {
    const int fd = ::open(path, O_RDONLY);
    if (fd >= 0) {
      unsigned char magic[2] = {0, 0};
      struct stat st{};
      if (::fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 2 && ::pread(fd, magic, 2, 0) == 2 && !(magic[0] == 0x1f && magic[1] == 0x8b)) {
        map.p = ::mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (map.p != MAP_FAILED) { map.n = (size_t)st.st_size; plain = true; (void)::madvise(map.p, map.n, MADV_WILLNEED); }
      }
      ::close(fd);
    }
  }
  if (!plain) {
    gzFile f = gzopen(path, "rb");           // transparent for plain text
    if (!f) return std::string("cannot read ") + path;
    gzbuffer(f, 1 << 20);
    std::vector<char> buf(8u << 20);
    for (;;) {
      const int got = gzread(f, buf.data(), (unsigned)buf.size());
      if (got < 0) { gzclose(f); return std::string("cannot read ") + path; }
      if (got == 0) break;
      data.append(buf.data(), (size_t)got);
    }
    gzclose(f);
  }
  const double ms_read = ms_since(t_read);
  const auto t_parse = std::chrono::steady_clock::now();
  const char* const text = plain ? (const char*)map.p : data.data();
  const size_t n = plain ? map.n : data.size(), chrom_len = chrom ? std::strlen(chrom) : 0;
  const size_t T = (size_t)pool->size();
  // room for a pointer per line, so that the table never moves while the caller reads it
  {
    std::vector<size_t> lines(T, 0);
    pool->for_blocks(n, [&](size_t b, size_t e, int tid) {
      size_t c = 0;
      for (const char* p = text + b; p < text + e;) {
        const char* nl = (const char*)std::memchr(p, '\n', (size_t)(text + e - p));
        if (!nl) break;
        c++; p = nl + 1;
      }
      lines[(size_t)tid] += c;
    });
    size_t total_lines = 1;
    for (size_t c : lines) total_lines += c;
    out.at.assign(total_lines, nullptr);
  }
  // Waves of 16 MB (at least eight): every worker takes the lines that start in its share of the wave, the wave's records are listed
  // in file order and published, and the caller walks them while the next wave is parsed (the walk used to start when the last of
  // three million records was in: 0.06 s into the call at BASELINE config 5's size).
  const size_t wave = std::max<size_t>(1u << 20, std::min<size_t>(16u << 20, (n + 7) / 8));
  const size_t n_waves = n ? (n + wave - 1) / wave : 0;
  out.parts.assign(n_waves * T, std::vector<Var>());
  size_t total = 0;
  for (size_t w = 0; w < n_waves; w++) {
    const size_t w_lo = w * wave, w_hi = std::min(n, w_lo + wave);
    pool->for_blocks(w_hi - w_lo, [&](size_t b0, size_t e0, int tid) {
      const size_t b = w_lo + b0, e = w_lo + e0;
      const char* const base = text;
      const char* const end = base + n;
      const char* p = base + b;
      if (b > 0) { const char* nl = (const char*)std::memchr(base + b - 1, '\n', n - (b - 1)); p = nl ? nl + 1 : end; }   // first line start >= b
      std::vector<Var>& mine = out.parts[w * T + (size_t)tid];
      // (a record is parsed where it stays: a Var built aside and moved in, into a vector that doubled its way up, was a third of the
      // 0.11 s the records took -- room for a record per 24 bytes, which no line with an INFO column undercuts)
      mine.reserve((e - b) / 24 + 16);
      while (p < base + e) {
        const char* nl = (const char*)std::memchr(p, '\n', (size_t)(end - p));
        const char* le = nl ? nl : end;
        if (p < le && *p != '#') {
          mine.emplace_back();
          if (!parse_record(p, le, chrom, chrom_len, mine.back())) mine.pop_back();
        }
        p = le + 1;
      }
    });
    for (size_t t = 0; t < T; t++) {
      std::vector<Var>& mine = out.parts[w * T + t];
      if (total + mine.size() > out.at.size()) { out.publish(total, true); return "the VCF holds more records than lines (internal error)"; }
      for (size_t k = 0; k < mine.size(); k++) out.at[total + k] = &mine[k];
      total += mine.size();
    }
    out.publish(total, w + 1 == n_waves);
  }
  if (n_waves == 0) out.publish(0, true);
  if (TUNE_GET("CALITAS_TRACE") && total >= 100000)
    std::fprintf(stderr, "[calitas] read_vcf: %zu bytes read in %.1f ms, %zu records parsed in %.1f ms (%zu waves)\n", n, ms_read, total, ms_since(t_parse), n_waves);
  return "";
}

// MD5 (RFC 1321) of a file, hex: the second half of ReferenceHit's VCF identifier "name:md5" (RH:175-183).  One chain of dependent
// additions and rotations from the first byte to the last: 0.21 s per 127 MB as a loop over a step table, 0.14 s with the 64 steps
// written out (constants and rotations as immediates, the selection functions in their three-operation forms) -- and the first row that
// names a variant cannot be final before it is done, so at BASELINE config 5's size this is what the first contig's text waits for.
#define CALITAS_MD5_ROL(x, s) (((x) << (s)) | ((x) >> (32 - (s))))
#define CALITAS_MD5_F1(b, c, d) ((d) ^ ((b) & ((c) ^ (d))))
#define CALITAS_MD5_F2(b, c, d) ((c) ^ ((d) & ((b) ^ (c))))
#define CALITAS_MD5_F3(b, c, d) ((b) ^ (c) ^ (d))
#define CALITAS_MD5_F4(b, c, d) ((c) ^ ((b) | ~(d)))
#define CALITAS_MD5_STEP(f, a, b, c, d, g, k, s) a += f(b, c, d) + m[g] + (k); a = b + CALITAS_MD5_ROL(a, s);
static void md5_block(uint32_t* h, const unsigned char* p) {
  uint32_t m[16];
  std::memcpy(m, p, 64);                              // (little-endian words, as on every machine this library is built for)
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
#define S1(a, b, c, d, g, k, s) CALITAS_MD5_STEP(CALITAS_MD5_F1, a, b, c, d, g, k, s)
#define S2(a, b, c, d, g, k, s) CALITAS_MD5_STEP(CALITAS_MD5_F2, a, b, c, d, g, k, s)
#define S3(a, b, c, d, g, k, s) CALITAS_MD5_STEP(CALITAS_MD5_F3, a, b, c, d, g, k, s)
#define S4(a, b, c, d, g, k, s) CALITAS_MD5_STEP(CALITAS_MD5_F4, a, b, c, d, g, k, s)
  S1(a,b,c,d,0,0xd76aa478u,7) S1(d,a,b,c,1,0xe8c7b756u,12) S1(c,d,a,b,2,0x242070dbu,17) S1(b,c,d,a,3,0xc1bdceeeu,22)
  S1(a,b,c,d,4,0xf57c0fafu,7) S1(d,a,b,c,5,0x4787c62au,12) S1(c,d,a,b,6,0xa8304613u,17) S1(b,c,d,a,7,0xfd469501u,22)
  S1(a,b,c,d,8,0x698098d8u,7) S1(d,a,b,c,9,0x8b44f7afu,12) S1(c,d,a,b,10,0xffff5bb1u,17) S1(b,c,d,a,11,0x895cd7beu,22)
  S1(a,b,c,d,12,0x6b901122u,7) S1(d,a,b,c,13,0xfd987193u,12) S1(c,d,a,b,14,0xa679438eu,17) S1(b,c,d,a,15,0x49b40821u,22)
  S2(a,b,c,d,1,0xf61e2562u,5) S2(d,a,b,c,6,0xc040b340u,9) S2(c,d,a,b,11,0x265e5a51u,14) S2(b,c,d,a,0,0xe9b6c7aau,20)
  S2(a,b,c,d,5,0xd62f105du,5) S2(d,a,b,c,10,0x02441453u,9) S2(c,d,a,b,15,0xd8a1e681u,14) S2(b,c,d,a,4,0xe7d3fbc8u,20)
  S2(a,b,c,d,9,0x21e1cde6u,5) S2(d,a,b,c,14,0xc33707d6u,9) S2(c,d,a,b,3,0xf4d50d87u,14) S2(b,c,d,a,8,0x455a14edu,20)
  S2(a,b,c,d,13,0xa9e3e905u,5) S2(d,a,b,c,2,0xfcefa3f8u,9) S2(c,d,a,b,7,0x676f02d9u,14) S2(b,c,d,a,12,0x8d2a4c8au,20)
  S3(a,b,c,d,5,0xfffa3942u,4) S3(d,a,b,c,8,0x8771f681u,11) S3(c,d,a,b,11,0x6d9d6122u,16) S3(b,c,d,a,14,0xfde5380cu,23)
  S3(a,b,c,d,1,0xa4beea44u,4) S3(d,a,b,c,4,0x4bdecfa9u,11) S3(c,d,a,b,7,0xf6bb4b60u,16) S3(b,c,d,a,10,0xbebfbc70u,23)
  S3(a,b,c,d,13,0x289b7ec6u,4) S3(d,a,b,c,0,0xeaa127fau,11) S3(c,d,a,b,3,0xd4ef3085u,16) S3(b,c,d,a,6,0x04881d05u,23)
  S3(a,b,c,d,9,0xd9d4d039u,4) S3(d,a,b,c,12,0xe6db99e5u,11) S3(c,d,a,b,15,0x1fa27cf8u,16) S3(b,c,d,a,2,0xc4ac5665u,23)
  S4(a,b,c,d,0,0xf4292244u,6) S4(d,a,b,c,7,0x432aff97u,10) S4(c,d,a,b,14,0xab9423a7u,15) S4(b,c,d,a,5,0xfc93a039u,21)
  S4(a,b,c,d,12,0x655b59c3u,6) S4(d,a,b,c,3,0x8f0ccc92u,10) S4(c,d,a,b,10,0xffeff47du,15) S4(b,c,d,a,1,0x85845dd1u,21)
  S4(a,b,c,d,8,0x6fa87e4fu,6) S4(d,a,b,c,15,0xfe2ce6e0u,10) S4(c,d,a,b,6,0xa3014314u,15) S4(b,c,d,a,13,0x4e0811a1u,21)
  S4(a,b,c,d,4,0xf7537e82u,6) S4(d,a,b,c,11,0xbd3af235u,10) S4(c,d,a,b,2,0x2ad7d2bbu,15) S4(b,c,d,a,9,0xeb86d391u,21)
#undef S1
#undef S2
#undef S3
#undef S4
  h[0] += a; h[1] += b; h[2] += c; h[3] += d;
}
std::string md5_file(const char* path, std::string& hex) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return std::string("cannot read ") + path;
  uint32_t h[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
  std::vector<unsigned char> buf(1 << 20);
  uint64_t total = 0;
  size_t have = 0;                                   // bytes of an incomplete block at the start of buf
  for (;;) {
    const size_t got = std::fread(buf.data() + have, 1, buf.size() - have, f);
    total += got;
    const size_t n = have + got;
    size_t off = 0;
    for (; off + 64 <= n; off += 64) md5_block(h, buf.data() + off);
    have = n - off;
    std::memmove(buf.data(), buf.data() + off, have);
    if (got == 0) break;
  }
  std::fclose(f);
  unsigned char tail[128] = {0};
  std::memcpy(tail, buf.data(), have);
  tail[have] = 0x80;
  const size_t tl = have < 56 ? 64 : 128;
  const uint64_t bits = total * 8;
  for (int i = 0; i < 8; i++) tail[tl - 8 + i] = (unsigned char)(bits >> (8 * i));
  for (size_t off = 0; off < tl; off += 64) md5_block(h, tail + off);
  char out[33];
  for (int i = 0; i < 16; i++) std::snprintf(out + 2 * i, 3, "%02x", (h[i / 4] >> (8 * (i % 4))) & 0xFFu);
  hex = out;
  return "";
}

std::string vcf_identifier(const char* vcf_path, const std::string& md5_hex) {
  const char* slash = std::strrchr(vcf_path, '/');
  return std::string(slash ? slash + 1 : vcf_path) + ":" + md5_hex;
}

}  // namespace calitas

// ---- what the variant search knows about a VCF, on its own (callers that search many guides against one VCF; the CPU tests) ----------

extern "C" int calitas_vcf_identifier(calitas_ctx* ctx, const char* vcf_path, char** id) {
  if (!vcf_path || !id) return calitas_fail(ctx, CALITAS_EINVAL, "NULL argument");
  *id = nullptr;
  std::string hex;
  const std::string e = md5_file(vcf_path, hex);
  if (!e.empty()) return calitas_fail(ctx, CALITAS_EIO, e);
  const std::string v = vcf_identifier(vcf_path, hex);
  char* out = (char*)calitas_out_alloc(v.size() + 1);
  if (!out) return calitas_fail(ctx, CALITAS_EINVAL, "out of memory");
  std::memcpy(out, v.c_str(), v.size() + 1);
  *id = out;
  return CALITAS_OK;
}

extern "C" int calitas_vcf_records(calitas_ctx* ctx, const char* vcf_path, const char* chrom, char** text, uint64_t* n_records) {
  if (!ctx) return CALITAS_EINVAL;
  if (!vcf_path || !text) return calitas_fail(ctx, CALITAS_EINVAL, "NULL argument");
  *text = nullptr;
  if (n_records) *n_records = 0;
  VarTable vcf;
  const std::string e = read_vcf(vcf_path, chrom, ctx->pool, vcf);
  vcf.publish(vcf.size(), true);
  if (!e.empty()) return calitas_fail(ctx, CALITAS_EIO, e);
  std::string out;
  char num[64];
  for (size_t i = 0; vcf.have(i); i++) {                          // (through have(), as the search walks the table)
    const Var& v = vcf[i];
    out += v.chrom; out += '\t';
    out += std::to_string(v.pos); out += '\t';
    out += std::to_string(v.end); out += '\t';
    out += v.id; out += '\t';
    out += v.ref; out += '\t';
    for (size_t a = 0; a < v.alts.size(); a++) { if (a) out += ','; out += v.alts[a]; }
    out += '\t';
    for (size_t a = 0; a < v.afs.size(); a++) { if (a) out += ','; std::snprintf(num, sizeof(num), "%.9g", (double)v.afs[a]); out += num; }
    out += '\n';
  }
  char* block = (char*)calitas_out_alloc(out.size() + 1);
  if (!block) return calitas_fail(ctx, CALITAS_EINVAL, "out of memory");
  std::memcpy(block, out.c_str(), out.size() + 1);
  *text = block;
  if (n_records) *n_records = vcf.size();
  return CALITAS_OK;
}
