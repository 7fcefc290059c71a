// Host-only check of the scratch layouts of the native entity and of the three options that read it (no GPU, no kernel runs):
//
//     hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//           -Wl,--unresolved-symbols=ignore-all -o check_tail_scratch tools/check_tail_scratch.hip
//     ./check_tail_scratch
//
// The four source files are included whole, so the layout functions are the ones the library compiles; what else they define
// is never called here (hence the unresolved symbols of the other source files).  The host code alone is built with the address
// and undefined-behaviour sanitizers.  For cap = 8, 33, 300, 2048: every part of entity_scratch, ss_scratch, exposure_scratch
// and domains_scratch starts 16-aligned behind the head, no two parts overlap, and the last one ends inside `total`; `total`
// and the head are what the *_need function reports.  Exit status 0 if all of it holds.
#include "../dmpfold2_amd/csrc/entity.hip"
#include "../dmpfold2_amd/csrc/ss.hip"
#include "../dmpfold2_amd/csrc/exposure.hip"
#include "../dmpfold2_amd/csrc/domains.hip"
#include <algorithm>
#include <cstdio>
#include <vector>

using namespace dmp;

struct Part { const char* name; int64_t at, bytes; };

// the parts in the order given: each 16-aligned, at or behind the end of the one before (the head first), the last inside total
static int check(const char* what, int cap, int64_t head, std::vector<Part> parts, int64_t total, ScratchNeed need) {
  int bad = 0;
  std::sort(parts.begin(), parts.end(), [](const Part& a, const Part& b) { return a.at < b.at; });
  int64_t end = head;
  for (const Part& p : parts) {
    if (p.at % 16 || p.at < end || p.bytes < 0) {
      std::printf("%s cap %d: part %s at %lld (%lld bytes) is misaligned or overlaps what ends at %lld\n", what, cap, p.name,
                  (long long)p.at, (long long)p.bytes, (long long)end);
      ++bad;
    }
    end = p.at + p.bytes;
  }
  if (end > total || need.bytes != total || need.head != head) {
    std::printf("%s cap %d: parts end at %lld, total %lld, need {%lld, %lld}, head %lld\n", what, cap, (long long)end, (long long)total,
                (long long)need.bytes, (long long)need.head, (long long)head);
    ++bad;
  }
  return bad;
}

int main() {
  int bad = 0;
  for (int cap : {8, 33, 300, 2048}) {
    const int64_t c = cap, words = ss_row_words(cap);
    const EntityScratch en = entity_scratch(cap);
    bad += check("entity_scratch", cap, ENTITY_HEAD_BYTES, {{"row", en.row, c}, {"bb", en.bb, 60 * c}}, en.total, entity_need(cap));
    const SsScratch ss = ss_scratch(cap);
    std::vector<Part> parts;
    for (int e = 0; e < 2; ++e) {
      parts.push_back({"h", ss.h[e], 24 * c});
      parts.push_back({"donor", ss.donor[e], c});
      parts.push_back({"R", ss.R[e], 4 * c * words});
      parts.push_back({"T", ss.T[e], 4 * c * words});
    }
    bad += check("ss_scratch", cap, SS_HEAD_BYTES, parts, ss.total, assign_ss_need(cap));
    if (4 * (SS_COUNTERS + 1) > SS_HEAD_BYTES || 4 * (EXP_COUNTERS + 1) > EXP_HEAD_BYTES) {
      std::printf("the counters and the ticket do not fit the head\n");
      ++bad;
    }
    bad += check("exposure_scratch", cap, EXP_HEAD_BYTES, {}, exposure_scratch(cap).total, exposure_need(cap));
    const DomScratch d = domains_scratch(cap);
    bad += check("domains_scratch", cap, DOM_HEAD_BYTES,
                 {{"node", d.node, 2 * 4 * c}, {"idx", d.idx, 2 * 4 * c}, {"slot", d.slot, 2 * DOM_MAX * (int64_t)sizeof(DomSlot)},
                  {"made", d.made, 2 * DOM_NODES * 8}, {"part", d.part, 2 * (int64_t)sizeof(DomCut) * c}, {"con", d.con, 2 * c * c},
                  {"sat", d.sat, 2 * 4 * (c + 16) * (c + 16)}},
                 d.total, domains_need(cap));
  }
  std::printf("%s\n", bad ? "FAILED" : "ok: entity, ss, exposure and domains scratches at cap 8, 33, 300, 2048");
  return bad ? 1 : 0;
}
