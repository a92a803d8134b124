// frame_stack_host_main.cc -- the group planner of the image decoders and encoders, the cut of a
// group's files into download slices and the files' offsets (aerial_mapper_amd/csrc/
// amhip_frame_plan.h) as a stand-alone program.  tests/test_frame_stack_host.py builds it with
// -fsanitize=address,undefined and runs it as a child process.
//
//   frame_stack_host_main <case>...     a case: <budget>:<max_frames>:<cost>,<cost>,...
//     -> per case three lines:  groups <group_begin...>   bases <base...>   max <max_group_bytes>
//   frame_stack_host_main slices <case>...     a case: <limit>:<size>,<size>,...
//     -> per case three lines:  ends <the file behind every slice...>   bytes <every slice's sum...>
//        offsets <F + 1 prefix sums>
// The costs and sizes are copied into heap buffers of exactly their size and the bases and offsets are
// written into such buffers: any access outside them is a sanitizer report and a non-zero exit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "amhip_frame_plan.h"

static std::vector<size_t> numbers(char* at) {
  std::vector<size_t> parsed;
  while (*at) {
    parsed.push_back(std::strtoull(at, &at, 10));
    if (*at == ',') ++at;
  }
  return parsed;
}

static int slices_main(int argc, char** argv) {
  for (int a = 2; a < argc; ++a) {
    char* at = argv[a];
    const size_t limit = std::strtoull(at, &at, 10);
    if (*at++ != ':') return 2;
    const std::vector<size_t> parsed = numbers(at);
    const size_t F = parsed.size();
    std::unique_ptr<unsigned long long[]> sizes(new unsigned long long[F]);
    std::unique_ptr<size_t[]> offsets(new size_t[F + 1]);
    for (size_t i = 0; i < F; ++i) sizes[i] = parsed[i];
    std::vector<size_t> ends, bytes;
    for (size_t f = 0; f < F;) {
      size_t sum = 0;
      f = amhip::slice_end(sizes.get(), f, F, limit, &sum);
      ends.push_back(f);
      bytes.push_back(sum);
    }
    amhip::prefix_offsets(sizes.get(), F, offsets.get());
    std::printf("ends");
    for (size_t e : ends) std::printf(" %zu", e);
    std::printf("\nbytes");
    for (size_t b : bytes) std::printf(" %zu", b);
    std::printf("\noffsets");
    for (size_t i = 0; i <= F; ++i) std::printf(" %zu", offsets[i]);
    std::printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "slices")) return slices_main(argc, argv);
  for (int a = 1; a < argc; ++a) {
    char* at = argv[a];
    const size_t budget = std::strtoull(at, &at, 10);
    if (*at++ != ':') return 2;
    const size_t max_frames = std::strtoull(at, &at, 10);
    if (*at++ != ':') return 2;
    const std::vector<size_t> parsed = numbers(at);
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
