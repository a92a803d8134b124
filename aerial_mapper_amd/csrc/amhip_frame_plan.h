// amhip_frame_plan.h -- how the image decoders and encoders (amhip_frame_stack.h) cut a call's frames
// into groups that share one scratch buffer, and a group's files into download slices.  No HIP in
// here: tests/cpp/frame_stack_host_main.cc compiles it alone under the sanitizers.
#ifndef AMHIP_FRAME_PLAN_H_
#define AMHIP_FRAME_PLAN_H_

#include <cstddef>
#include <vector>

namespace amhip {

// Groups of consecutive frames.  Frame i opens a group when i == 0, when the group's bytes so far
// plus cost_bytes[i] exceed `budget`, or when the group holds `max_frames` frames already; so a
// group has at least one frame, whatever that frame costs.  base_bytes[i]: the group's bytes in front
// of frame i.  group_begin: the first frame of every group, then F.  *max_group_bytes: the largest
// total of a group, what the scratch has to hold.
inline void plan_groups(const size_t* cost_bytes, size_t F, size_t budget, size_t max_frames,
                        std::vector<size_t>* group_begin, size_t* base_bytes, size_t* max_group_bytes) {
  group_begin->clear();
  *max_group_bytes = 0;
  size_t running = 0, count = 0;
  for (size_t i = 0; i < F; ++i) {
    if (i == 0 || running + cost_bytes[i] > budget || count == max_frames) {
      group_begin->push_back(i);
      running = 0;
      count = 0;
    }
    base_bytes[i] = running;
    running += cost_bytes[i];
    ++count;
    if (running > *max_group_bytes) *max_group_bytes = running;
  }
  group_begin->push_back(F);
}

// The cut of files [first, last) of consecutive `sizes` into download slices.  A slice starts at a
// file and takes the following files while the sum stays <= `limit`; so it holds at least one file,
// whatever that file's size.  -> the file behind the slice that starts at `first`; *bytes: its sum.
template <typename Size>
inline size_t slice_end(const Size* sizes, size_t first, size_t last, size_t limit, size_t* bytes) {
  size_t sum = (size_t)sizes[first], end = first + 1;
  while (end < last && sum + (size_t)sizes[end] <= limit) sum += (size_t)sizes[end++];
  *bytes = sum;
  return end;
}

// offsets[f]: the bytes in front of file f, offsets[F]: all of them (the exclusive prefix sums)
template <typename Size>
inline void prefix_offsets(const Size* sizes, size_t F, size_t* offsets) {
  offsets[0] = 0;
  for (size_t f = 0; f < F; ++f) offsets[f + 1] = offsets[f] + (size_t)sizes[f];
}

}  // namespace amhip

#endif  // AMHIP_FRAME_PLAN_H_
