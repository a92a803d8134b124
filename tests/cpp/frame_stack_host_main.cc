// frame_stack_host_main.cc -- the group planner of the image decoders (aerial_mapper_amd/csrc/
// amhip_frame_plan.h) as a stand-alone program.  tests/test_frame_stack_host.py builds it with
// -fsanitize=address,undefined and runs it as a child process.
//
//   frame_stack_host_main <case>...     a case: <budget>:<max_frames>:<cost>,<cost>,...
//     -> per case three lines:  groups <group_begin...>   bases <base...>   max <max_group_bytes>
// The costs are copied into a heap buffer of exactly their size and the bases are written into one:
// any access outside them is a sanitizer report and a non-zero exit.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "amhip_frame_plan.h"

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    char* at = argv[a];
    const size_t budget = std::strtoull(at, &at, 10);
    if (*at++ != ':') return 2;
    const size_t max_frames = std::strtoull(at, &at, 10);
    if (*at++ != ':') return 2;
    std::vector<size_t> parsed;
    while (*at) {
      parsed.push_back(std::strtoull(at, &at, 10));
      if (*at == ',') ++at;
    }
    const size_t F = parsed.size();
    std::unique_ptr<size_t[]> cost(new size_t[F]), base(new size_t[F]);
    for (size_t i = 0; i < F; ++i) cost[i] = parsed[i];
    std::vector<size_t> group_begin;
    size_t max_bytes = 0;
    amhip::plan_groups(cost.get(), F, budget, max_frames, &group_begin, base.get(), &max_bytes);
    std::printf("groups");
    for (size_t g : group_begin) std::printf(" %zu", g);
    std::printf("\nbases");
    for (size_t i = 0; i < F; ++i) std::printf(" %zu", base[i]);
    std::printf("\nmax %zu\n", max_bytes);
  }
  return 0;
}
