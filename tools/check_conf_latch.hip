// Host-only check of the d_conf layout of csrc/common.h (no GPU, no kernel):
//
//     hipcc --offload-arch=gfx950 -std=c++17 -o check_conf_latch tools/check_conf_latch.hip
//     ./check_conf_latch [tests/golden/conf_layout.json]
//
// 1. The floats a latched fault turns into NaN.  fault_latch_kernel (api.hip) asks conf_is_out(); until the layout stated each
//    block's out range it evaluated an interval expression over offsets.  That expression and the offsets it read are transcribed
//    here literally, and compared with the predicate for every float index below total + 3m + 8, over every combination of the
//    six layout options, L in {8, 9, 33}, pass rows R in {1, 3} and a structure of m in {0, 3} rows behind the align block.
// 2. conf_layout()'s offsets for the rows of tests/golden/conf_layout.json that have no search block: S0, M0 and A0 as recorded.
// Exit status 0 if nothing differs.
#include "../dmpfold2_amd/csrc/common.h"
#include <cstdio>
#include <cstring>
#include <set>
#include <tuple>

using namespace dmp;

// ---- the layout and the expression as they were, word for word ----
struct OldLayout { int64_t map_off, info_off, score_off, score_out, smap_off, align_off, align_out, total, pass_off, ss_off; };
static OldLayout old_layout(int L, int emit, int score, int align = 0, int smap = 0, int passes = 0, int ss = 0) {
  const int64_t info_off = L + (emit ? (int64_t)L * L : 0), score_off = info_off + (emit ? 3 : 0);
  const int64_t smap_off = score_off + (score ? score_layout(L).total : 0);
  const int64_t pass_off = smap_off + (smap ? mapscore_floats(L) : 0);
  const int64_t ss_off = pass_off + (passes ? pass_floats(passes) : 0);
  const int64_t align_off = ss_off + (ss ? ss_floats(L) : 0);
  return {L, info_off, score_off, score_off + score_layout(L).out, smap_off, align_off, align_off + 1,
          align_off + (align ? align_layout(L).in : 0), pass_off, ss_off};
}
static bool old_is_nan(const OldLayout& lay, int64_t i) {
  return i < lay.score_off || (i >= lay.score_out && i < lay.align_off) || (i >= lay.ss_off && i < lay.align_off) ||
         (i >= lay.align_out && i < lay.total);
}

static long check_predicate() {
  long differences = 0, indices = 0, cases = 0;
  const int Ls[] = {8, 9, 33}, Rs[] = {1, 3}, ms[] = {0, 3};
  for (int bits = 0; bits < 64; ++bits)
    for (int L : Ls)
      for (int R : Rs)
        for (int m : ms) {
          TailOpts o;
          o.emit = bits & 1; o.score = bits >> 1 & 1; o.smap = bits >> 2 & 1; o.passes = bits >> 3 & 1; o.ss = bits >> 4 & 1;
          o.align = bits >> 5 & 1;
          const int rows = o.passes ? R : 0;
          const OldLayout was = old_layout(L, o.emit, o.score, o.align, o.smap, rows, o.ss);
          const ConfLayout lay = conf_layout(L, o, rows);
          ++cases;
          if (was.total != lay.total) { ++differences; printf("total differs: bits %d L %d R %d\n", bits, L, R); }
          for (int64_t i = 0; i < was.total + 3 * m + 8; ++i, ++indices)
            if (old_is_nan(was, i) != conf_is_out(lay, i)) {
              if (++differences <= 20)
                printf("differs: emit %d score %d smap %d passes %d ss %d align %d L %d R %d m %d index %lld: was %d, is %d\n", o.emit,
                       o.score, o.smap, o.passes, o.ss, o.align, L, R, m, (long long)i, (int)old_is_nan(was, i), (int)conf_is_out(lay, i));
            }
        }
  printf("predicate: %ld cases (64 option sets x L 8, 9, 33 x R 1, 3 x m 0, 3), %ld float indices, %ld differences\n", cases, indices,
         differences);
  return differences;
}

// A row of the file is one line: [L,distmap,score,score_map,align_m,max_L,search,conf_floats,S0,M0,A0,...
static long check_golden(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { printf("cannot open %s\n", path); return 1; }
  static char line[1 << 16];
  long rows = 0, bad = 0;
  std::set<std::tuple<int, int, int, int>> seen;
  while (fgets(line, sizeof(line), f)) {
    if (line[0] != '[' || line[1] == '\n') continue;
    char* field[11];
    char* p = line + 1;
    bool ok = true;
    for (int k = 0; k < 11 && ok; ++k) {
      field[k] = p;
      if (*p == '[') ok = false;                     // a search block: skipped
      char* q = strchr(p, ',');
      if (!q) { ok = false; break; }
      *q = 0;
      p = q + 1;
    }
    if (!ok || strcmp(field[6], "null") != 0) continue;
    const int L = atoi(field[0]);
    TailOpts o;
    o.emit = !strcmp(field[1], "true"); o.score = !strcmp(field[2], "true"); o.smap = !strcmp(field[3], "true");
    const long long S0 = atoll(field[8]), M0 = atoll(field[9]), A0 = atoll(field[10]);
    const ConfLayout lay = conf_layout(L, o, 0);
    const bool same = lay.score.off == S0 && lay.smap.off == M0 && lay.align.off == A0;
    ++rows;
    bad += same ? 0 : 1;
    if (seen.insert({L, o.emit, o.score, o.smap}).second)
      printf("L %4d distmap %d score %d score_map %d: S0 %lld M0 %lld A0 %lld | conf_layout: score %lld smap %lld align %lld  %s\n", L, o.emit,
             o.score, o.smap, S0, M0, A0, (long long)lay.score.off, (long long)lay.smap.off, (long long)lay.align.off,
             same ? "equal" : "DIFFERENT");
  }
  fclose(f);
  printf("golden: %ld rows without a search block, %ld different\n", rows, bad);
  return bad + (rows == 0);
}

int main(int argc, char** argv) {
  const long a = check_predicate();
  const long b = check_golden(argc > 1 ? argv[1] : "tests/golden/conf_layout.json");
  return a || b ? 1 : 0;
}
