// edit_sites_asan.cpp -- the host twin of the edit sites (calitas_find_edit_sites_host, calitas_count_edit_sites_host: the plan, the
// base-by-base walk of one SNV, the block handed out) as a stand-alone program for a run under AddressSanitizer and UBSan: a
// host-only context, no device, nothing loaded into another process.
//   make -C calitas_amd/csrc SAN=address SANFLAGS="-fsanitize=address,undefined -fno-omit-frame-pointer -g -O1"
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-omit-frame-pointer tools/edit_sites_asan.cpp -Iinclude \
//         -Lcalitas_amd -lcalitas_hip_address -Wl,-rpath,$PWD/calitas_amd -o edit_sites_asan && ./edit_sites_asan GENOME.fa
// Over every contig of the FASTA: at every position the SNV each of four editors makes there in either mode, and every third position
// an SNV that is not the editor's, under six patterns.  The run is about memory; what it checks of the results is what needs no
// referee -- the count call against the listing, the order, the bound on a SNV's records, the target's bit, the statuses' meaning.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "calitas_hip.h"

static void die(calitas_ctx* ctx, const char* what) {
  std::fprintf(stderr, "%s: %s\n", what, calitas_last_error(ctx));
  std::exit(1);
}

static int code_of(char c) { c &= 0xDF; return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : (c == 'T' || c == 'U') ? 3 : -1; }

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: edit_sites_asan GENOME.fa\n"); return 2; }
  calitas_ctx* ctx = nullptr;
  if (calitas_create(-1, &ctx) != CALITAS_OK) die(nullptr, "calitas_create");
  if (calitas_set_reference_fasta(ctx, argv[1]) != CALITAS_OK) die(ctx, "calitas_set_reference_fasta");
  int32_t n_contigs = 0;
  calitas_reference_info(ctx, &n_contigs, nullptr, nullptr);

  struct Pattern { const char* proto; std::vector<const char*> pams; int five; };
  const std::string n20(20, 'N'), n32(32, 'N');
  const std::vector<Pattern> patterns = {{n20.c_str(), {"nrg"}, 0}, {n20.c_str(), {"tttv"}, 1}, {n20.c_str(), {"ngg", "ng", "nnaa"}, 0}, {n20.c_str(), {}, 0},
                                         {n32.c_str(), {"nnnnnnnnnnnnnngg"}, 0}, {"N", {"cnnnnnnnnnnnnnnn"}, 1}};
  unsigned long long calls = 0, records = 0, by_status[6] = {0, 0, 0, 0, 0, 0};
  for (const Pattern& pt : patterns) {
    const int L = (int)std::strlen(pt.proto);
    calitas_guide_t g{};
    g.protospacer = pt.proto; g.n_pams = (int32_t)pt.pams.size(); g.pams = pt.pams.empty() ? nullptr : pt.pams.data(); g.pam_is_5prime = pt.five;
    g.cli_length = L + (pt.pams.empty() ? 0 : (int32_t)std::strlen(pt.pams[0]));
    const calitas_base_edit_t editors[] = {{'C', 'T', (uint8_t)(L >= 8 ? 3 : 0), (uint8_t)(L >= 8 ? 8 : L), 'N', 0, 255, 0}, {'a', 'g', 0, (uint8_t)L, 'T', 0, 255, 0},
                                           {'C', 'G', (uint8_t)(L - 1), (uint8_t)L, 'h', 0, 1, 0}, {'G', 'U', 0, (uint8_t)L, 0, 0, 0, 0}};
    for (calitas_base_edit_t edit : editors) {
      for (int correct = 0; correct < 2; correct++) {
        edit.correct = (uint8_t)correct;
        std::vector<calitas_snv_t> snvs;
        for (int32_t ci = 0; ci < n_contigs; ci++) {
          const char* name; uint64_t len = 0;
          calitas_contig_name(ctx, ci, &name, &len);
          std::string seq(len, 'N');
          if (len && calitas_fetch_bases(ctx, ci, 0, (uint32_t)len, &seq[0]) != CALITAS_OK) die(ctx, "calitas_fetch_bases");
          for (uint64_t pos = 0; pos < len; pos++) {
            const int x = code_of(seq[pos]), from = code_of(edit.from_base), to = code_of(edit.to_base);
            const int seen = correct ? to : from, made = correct ? from : to;
            char alt = 0;
            if (x == seen) alt = "ACGT"[made]; else if (x == 3 - seen) alt = "ACGT"[3 - made];
            if (alt) snvs.push_back(calitas_snv_t{ci, (int32_t)pos, pos % 2 ? seq[pos] : (char)0, alt, 0});
            if (pos % 3 == 0) snvs.push_back(calitas_snv_t{ci, (int32_t)pos, pos % 5 ? (char)0 : 'A', "ACGT"[pos % 4], 0});   // whatever this is: every status
          }
        }
        calitas_edit_site_t* found = nullptr; uint64_t n = 0, n_counted = 0, by[4] = {0, 0, 0, 0};
        std::vector<uint8_t> status(snvs.size() + 1, 9), status2(snvs.size() + 1, 9);
        if (calitas_find_edit_sites_host(ctx, &g, &edit, snvs.data(), snvs.size(), &found, &n, status.data()) != CALITAS_OK) die(ctx, "calitas_find_edit_sites_host");
        if (calitas_count_edit_sites_host(ctx, &g, &edit, snvs.data(), snvs.size(), by, &n_counted, status2.data()) != CALITAS_OK) die(ctx, "calitas_count_edit_sites_host");
        bool ok = n == n_counted && by[0] + by[1] + by[2] + by[3] == n && status == status2;
        uint64_t seen_by[4] = {0, 0, 0, 0};
        for (uint64_t k = 0; k < n && ok; k++) {
          const calitas_edit_site_t& r = found[k];
          const calitas_snv_t& v = snvs[r.snv_index];
          const int o = r.site.strand == '-' ? r.site.protospacer_start + L - 1 - v.position : v.position - r.site.protospacer_start;
          const int others = __builtin_popcount(r.editable) - 1;
          ok = r.snv_index < snvs.size() && status[r.snv_index] == 0 && o >= edit.window_from && o < edit.window_to && ((r.editable >> o) & 1u) &&
               (edit.max_bystanders == 255 || others <= edit.max_bystanders) &&
               (k == 0 || found[k - 1].snv_index < r.snv_index || (found[k - 1].snv_index == r.snv_index && found[k - 1].site.protospacer_start < r.site.protospacer_start));
          seen_by[others < 3 ? others : 3]++;
        }
        ok = ok && std::memcmp(seen_by, by, sizeof(by)) == 0;
        for (size_t i = 0; i < snvs.size() && ok; i++) { ok = status[i] <= 5; if (ok) by_status[status[i]]++; }
        if (!ok) { std::fprintf(stderr, "the listing, the count call and the statuses do not agree (L %d, window %d:%d, correct %d)\n", L, edit.window_from, edit.window_to, correct); return 1; }
        // no SNV at all, and no status array
        calitas_edit_site_t* none = nullptr; uint64_t n_none = 9;
        if (calitas_find_edit_sites_host(ctx, &g, &edit, nullptr, 0, &none, &n_none, nullptr) != CALITAS_OK || n_none != 0 || !none) die(ctx, "no SNV");
        calitas_free(none); calitas_free(found);
        calls += 3; records += n;
      }
    }
    // what the plan refuses leaves nothing behind
    calitas_base_edit_t bad = editors[0];
    bad.window_to = (uint8_t)(L + 1);
    calitas_edit_site_t* found = nullptr; uint64_t n = 0;
    const calitas_snv_t one{0, 0, 0, 'A', 0};
    if (calitas_find_edit_sites_host(ctx, &g, &bad, &one, 1, &found, &n, nullptr) != CALITAS_EINVAL || found) { std::fprintf(stderr, "a window past L was taken\n"); return 1; }
  }
  std::printf("edit_sites_asan: %llu calls, %llu records, status 0 .. 5: %llu %llu %llu %llu %llu %llu: clean\n", calls, records, by_status[0], by_status[1],
              by_status[2], by_status[3], by_status[4], by_status[5]);
  calitas_destroy(ctx);
  return 0;
}
