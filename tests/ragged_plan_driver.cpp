// Host-only driver of the ragged-ensemble planner (nbody-demo-2023_amd/csrc/nbx_plan.hpp: plan_ragged) for tests/test_ragged_cpu.py; g++, no ROCm.
//   ragged_plan_driver plan CUS       stdin: "precision bodies_per_lane inner_loop members n_0 ... n_{members-1}" per line; stdout per row one
//                                     line of JSON: {"NB", "loop", "D", "W", "pairs", "instance", "pos_records", "vel_records", "ke_parts",
//                                     "spare", "member": [[pos_off, vel_off, ke_off, grid, n, n_alloc], ...], "work": [[member, wg, pos_off,
//                                     vel_off, ke_off, n, n_alloc], ...]} or {"error": rc, "text": "..."}
//   ragged_plan_driver uniform CUS    stdin: "n precision members bodies_per_lane inner_loop" per line; stdout: "P NB loop D W" of plan_ragged
//                                     with all members of n bodies, then "NB loop D grid_x grid_y" of plan_ensemble -- or "E <rc> <message>"
//                                     when BOTH refuse; a row only one of them refuses is "X"
//   ragged_plan_driver walk CUS       the walk of ensemble_plan_driver (members x sizes x every bodies_per_lane / inner_loop, both
//                                     precisions) with all members equal: exit 1 at the first row where plan_ragged and plan_ensemble differ
//                                     in NB, loop, D, W = members x grid_x or in whether they refuse, or whose kernel is not compiled
//   ragged_plan_driver instances      the declared instance set, one "precision NB loop" per line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nbx_plan.hpp"

using namespace nbx;

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  const int cus = argc > 2 ? std::atoi(argv[2]) : 256;
  if (!std::strcmp(mode, "instances")) {
    for (const Instance& k : kEnsembleInstances) std::printf("%d %d %d\n", k.precision, k.B, k.loop);
    return 0;
  }
  if (!std::strcmp(mode, "plan")) {
    int precision, bpl, il, members;
    while (std::scanf("%d %d %d %d", &precision, &bpl, &il, &members) == 4) {
      std::vector<int> n((size_t)(members > 0 ? members : 0));
      for (int& v : n)
        if (std::scanf("%d", &v) != 1) return 2;
      nbx_opts o{};
      o.bodies_per_lane = bpl; o.inner_loop = il;
      RaggedPlan p;
      const char* msg = "";
      const int rc = plan_ragged(n.data(), members, precision, cus, o, &p, &msg);
      if (rc != NBX_OK) { std::printf("{\"error\": %d, \"text\": \"%s\"}\n", rc, msg); continue; }
      std::printf("{\"NB\": %d, \"loop\": %d, \"D\": %d, \"W\": %d, \"pairs\": %.17g, \"instance\": %d, \"pos_records\": %lld, \"vel_records\": %lld, "
                  "\"ke_parts\": %lld, \"spare\": %d, \"member\": [", p.NB, p.loop, p.D, p.W, p.pairs_per_step, ensemble_instance_index(p.step),
                  p.pos_records, p.vel_records, p.ke_parts, kSgprOverread);
      for (size_t k = 0; k < p.member.size(); ++k) {
        const RaggedMember& m = p.member[k];
        std::printf("%s[%u, %u, %u, %d, %d, %d]", k ? ", " : "", m.pos_off, m.vel_off, m.ke_off, m.grid, m.n, m.n_alloc);
      }
      std::printf("], \"work\": [");
      for (size_t k = 0; k < p.work.size(); ++k) {
        const RaggedWork& w = p.work[k];
        std::printf("%s[%u, %u, %u, %u, %u, %d, %d]", k ? ", " : "", w.member, w.wg, w.pos_off, w.vel_off, w.ke_off, w.n, w.n_alloc);
      }
      std::printf("]}\n");
    }
    return 0;
  }
  if (!std::strcmp(mode, "uniform")) {
    int n, precision, members, bpl, il;
    while (std::scanf("%d %d %d %d %d", &n, &precision, &members, &bpl, &il) == 5) {
      nbx_opts o{};
      o.bodies_per_lane = bpl; o.inner_loop = il;
      const std::vector<int> sizes((size_t)(members > 0 ? members : 0), n);
      RaggedPlan r;
      EnsemblePlan e;
      const char *rmsg = "", *emsg = "";
      const int rrc = plan_ragged(sizes.data(), members, precision, cus, o, &r, &rmsg), erc = plan_ensemble(n, precision, members, cus, o, &e, &emsg);
      if (rrc != NBX_OK && erc != NBX_OK) { std::printf("E %d %s\n", rrc, rmsg); continue; }
      if (rrc != NBX_OK || erc != NBX_OK) { std::printf("X %d %d\n", rrc, erc); continue; }
      std::printf("P %d %d %d %d %d %d %d %d %d\n", r.NB, r.loop, r.D, r.W, e.NB, e.loop, e.D, e.grid_x, e.grid_y);
    }
    return 0;
  }
  if (!std::strcmp(mode, "walk")) {
    const int members[] = {1, 2, 3, 7, 64, 1000}, sizes[] = {1, 5, 255, 256, 257, 2000, 2048, 4096, 4099, 8192, 12288, 12289, 13000, 16383};
    const int bpl[] = {-1, 0, 1, 2, 3, 4, 8, 16, 32}, il[] = {-1, 0, 1, 2, 3, 4, 5};
    long plans = 0, errors = 0;
    for (int S : members) for (int n : sizes) for (int precision : {32, 64}) for (int b : bpl) for (int l : il) {
      nbx_opts o{};
      o.bodies_per_lane = b; o.inner_loop = l;
      const std::vector<int> all((size_t)S, n);
      RaggedPlan r;
      EnsemblePlan e;
      const char *rmsg = "", *emsg = "";
      const int rrc = plan_ragged(all.data(), S, precision, cus, o, &r, &rmsg), erc = plan_ensemble(n, precision, S, cus, o, &e, &emsg);
      if ((rrc == NBX_OK) != (erc == NBX_OK)) {
        std::printf("one planner refuses what the other takes: n %d precision %d members %d opts %d %d: ragged %d, ensemble %d\n", n, precision, S, b, l, rrc, erc);
        return 1;
      }
      if (rrc != NBX_OK) {
        if (!rmsg || std::strncmp(rmsg, "nbx_ragged_create: ", 19)) { std::printf("error without a text: n %d precision %d members %d opts %d %d\n", n, precision, S, b, l); return 1; }
        ++errors;
        continue;
      }
      ++plans;
      const bool same = r.NB == e.NB && r.loop == e.loop && r.D == e.D && (long long)r.W == (long long)S * e.grid_x && r.step == e.step &&
                        (int)r.work.size() == r.W && r.D == jlane_depth(precision, r.NB);
      if (!same || ensemble_instance_index(r.step) < 0) {
        std::printf("differs from plan_ensemble / no instance: n %d precision %d members %d opts %d %d -> NB %d loop %d D %d W %d against NB %d loop %d D %d grid %d x %d\n",
                    n, precision, S, b, l, r.NB, r.loop, r.D, r.W, e.NB, e.loop, e.D, e.grid_x, e.grid_y);
        return 1;
      }
    }
    std::printf("%ld plans %ld errors\n", plans, errors);
    return 0;
  }
  std::fprintf(stderr, "usage: ragged_plan_driver plan|uniform|walk|instances [cus]\n");
  return 2;
}
