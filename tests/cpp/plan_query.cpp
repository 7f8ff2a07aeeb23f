// plan_query — asks the planner (yustack_amd/csrc/yucsum_plan.h) about shapes given
// to it, for tests/test_kernel_ledger.py. Built like plan_table: no GPU, no libyucsum.so.
//
//   plan_query < cases      "# knobs: NAME=VALUE ..." lines and case lines in the left-hand
//                           format of plan_table's rows (<U|R> mode align stride len n fill cu);
//                           prints the knob lines and the full rows
//   plan_query --reachable  the distinct keys the planner returns over plan_table's shape
//                           axes at 64 and 256 CUs, under every combination of YU_RAGGED,
//                           YU_NT, YU_RUNS and YU_FILL_WB (YU_VARIANT selects among the same
//                           functions and is left out):
//                             K <kernel> <form> <policy> <in place> <U|R>
//                           and, from the combination with no knob set,
//                             D <kernel> <mode> <in place> <U|R>
#include <iostream>
#include <set>
#include <sstream>

#include "plan_rows.h"

namespace {

std::set<std::string> g_keys, g_defaults;
bool g_default_knobs = false;

void collect(const yu::Shape &s, int, const yu::Plan &p) {
  char buf[160];
  snprintf(buf, sizeof buf, "K %s %s %u %d %c", p.name, kFormNames[(int)p.form], p.policy, (int)s.fill,
           s.ragged ? 'R' : 'U');
  g_keys.insert(buf);
  if (!g_default_knobs) return;
  snprintf(buf, sizeof buf, "D %s %s %d %c", p.name, kModeNames[s.mode], (int)s.fill, s.ragged ? 'R' : 'U');
  g_defaults.insert(buf);
}

int reachable() {
  g_quiet = true;
  g_sink = collect;
  for (const char *rag : {"", "loop", "seg4", "seg16", "seg8"})
    for (const char *nt : {"", "0", "1", "2"})
      for (const char *runs : {"0", "1", "2"})
        for (const char *wb : {"", "0"}) {
          std::vector<std::string> env;
          if (*rag) env.push_back(std::string("YU_RAGGED=") + rag);
          if (*nt) env.push_back(std::string("YU_NT=") + nt);
          env.push_back(std::string("YU_RUNS=") + runs);
          if (*wb) env.push_back(std::string("YU_FILL_WB=") + wb);
          set_knobs(env);
          g_default_knobs = !*rag && !*nt && runs[0] == '1' && !*wb;  // YU_RUNS=1 is the default
          for (int cus : {64, 256}) {
            g_cus = cus;
            shape_axes();
          }
        }
  for (const std::string &k : g_keys) printf("%s\n", k.c_str());
  for (const std::string &k : g_defaults) printf("%s\n", k.c_str());
  return 0;
}

int mode_of(const std::string &name) {
  for (int m = 0; m < YU_MODE_COUNT; ++m)
    if (name == kModeNames[m]) return m;
  return -1;
}

int query() {
  set_knobs({});
  std::string line;
  int lineno = 0;
  while (std::getline(std::cin, line)) {
    ++lineno;
    if (line.empty()) continue;
    std::istringstream in(line);
    if (line.compare(0, 8, "# knobs:") == 0) {
      std::string word;
      in >> word >> word;  // "#", "knobs:"
      std::vector<std::string> env;
      while (in >> word) env.push_back(word);
      set_knobs(env);
      continue;
    }
    if (line[0] == '#') continue;
    std::string layout, mode;
    unsigned long long align, stride, len, n;
    int fill, cus;
    if (!(in >> layout >> mode >> align >> stride >> len >> n >> fill >> cus) || (layout != "U" && layout != "R") ||
        mode_of(mode) < 0 || len > 0xFFFFFFFFull || cus < 1) {
      fprintf(stderr, "plan_query: line %d: %s\n", lineno, line.c_str());
      return 2;
    }
    row({layout == "R", align, stride, (uint32_t)len, n, mode_of(mode), fill != 0}, cus);
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && strcmp(argv[1], "--reachable") == 0) return reachable();
  return query();
}
