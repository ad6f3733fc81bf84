// Host-only driver of the share planner (nbody-demo-2023_amd/csrc/nbx_shares.hpp) for tests/test_shares_cpu.py; g++, no ROCm.
// One command per line of stdin, one answer per line of stdout; doubles are read by strtod (hex floats: exact) and printed as %a.
//   Q n ranks                                     equal_shares     -> "Q ranks block n_alloc begin count ..."
//   W n ranks nw w...                             weighted_shares (nw = 0: no weights) -> "W ranks n_alloc begin count ..." | "E rc text"
//   T ranks count... ms...                        tune_weights     -> "T w..." | "E rc text"
//   S cus n precision order ranks nw w...         a weighted group as nbx_group_create_weighted plans it: its shares, a fresh tuner,
//                                                 every rank a logical rank of a device with `cus` CUs, summation_order `order`
//                                                 -> "S ranks n_alloc begin count ..." | "E rc text"
//   C ms...                                       nbx_group_retune(force_ms) on it -> "K|M|B begin count ..." (kept, moved, taken
//                                                 back; the shares in force afterwards) | "E rc text"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "nbx_shares.hpp"

using namespace nbx;

static void print_shares(const char* tag, const Shares& s, bool with_alloc) {
  std::printf("%s", tag);
  if (with_alloc) std::printf(" %d %d", s.ranks, s.n_alloc);
  for (int r = 0; r < s.ranks; ++r) std::printf(" %d %d", s.begin[r], s.count[r]);
  std::printf("\n");
}

// the plan nbx_create gives rank r of the group: the options a group passes (own stream, plain launches, its slice of n_alloc records)
static Plan rank_plan(int cus, int n, int precision, int order, const Shares& s, int r) {
  nbx_opts o{};
  o.summation_order = order; o.use_graph = 2;
  o.i_begin = s.begin[r]; o.i_count = s.count[r]; o.n_alloc = s.n_alloc;
  Plan p;
  const char* msg = "";
  if (plan_launch({n, round_up(std::max(n, o.n_alloc), kTile), o.i_count, precision, cus, true}, o, &p, &msg) != NBX_OK) {
    std::fprintf(stderr, "plan_launch: %s\n", msg);
    std::exit(3);
  }
  return p;
}

int main() {
  int cus = 256, n = 0, precision = 32, order = 0;
  Shares own;
  Tuner tuner;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, tok;
    in >> cmd;
    std::vector<double> v;
    while (in >> tok) v.push_back(std::strtod(tok.c_str(), nullptr));
    const char* msg = "";
    int rc = NBX_OK;
    if (cmd == "Q") {
      const Shares s = equal_shares((int)v[0], (int)v[1]);
      std::printf("Q %d %d %d", s.ranks, s.block, s.n_alloc);
      print_shares("", s, false);
    } else if (cmd == "W" || cmd == "S") {
      const bool group = cmd == "S";
      const size_t at = group ? 4 : 1;  // of "ranks nw w..."
      if (group) { cus = (int)v[0]; precision = (int)v[2]; order = (int)v[3]; tuner = Tuner{}; }
      n = (int)v[group ? 1 : 0];
      const int ranks = (int)v[at], nw = (int)v[at + 1];
      rc = weighted_shares(n, ranks, nw ? v.data() + at + 2 : nullptr, &own, &msg);
      if (rc == NBX_OK) print_shares(cmd.c_str(), own, true);
    } else if (cmd == "T") {
      const int ranks = (int)v[0];
      std::vector<int> count(v.begin() + 1, v.begin() + 1 + ranks);
      std::vector<double> w((size_t)ranks);
      rc = tune_weights(ranks, count.data(), v.data() + 1 + ranks, w.data(), &msg);
      if (rc == NBX_OK) {
        std::printf("T");
        for (double x : w) std::printf(" %a", x);
        std::printf("\n");
      }
    } else if (cmd == "C") {
      std::vector<Plan> plan;  // of the contexts in force, as model_force_cost reads it
      for (int r = 0; r < own.ranks; ++r) plan.push_back(rank_plan(cus, n, precision, order, own, r));
      Shares next;
      const int verdict = tune_shares(&tuner, own, n, v.data(), [&](int r, int share) { return force_cost(plan[(size_t)r], precision, cus, share); }, &next, &msg);
      if (verdict < 0) rc = verdict;
      else {
        if (verdict != SHARES_KEEP) own = next;
        print_shares(verdict == SHARES_KEEP ? "K" : verdict == SHARES_MOVE ? "M" : "B", own, false);
      }
    } else {
      std::fprintf(stderr, "unknown command: %s\n", line.c_str());
      return 2;
    }
    if (rc != NBX_OK) std::printf("E %d %s\n", rc, msg);
  }
  return 0;
}
