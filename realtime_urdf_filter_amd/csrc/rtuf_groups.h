// rtuf_groups.h -- how a batch of n streams is split into launch groups, and how many counter blocks a batch slot needs for
// every batch a context accepts (1 <= n <= max_streams).
//
// Included by the host API (rtuf_api.cpp) and the CPU check tests/launch_groups_check.cpp (plain g++, no ROCm headers), which
// runs these functions for every lane count up to 8, launch group up to 1024 and max_streams up to 4096.  Host-only, plain C++.
#pragma once

namespace rtuf {

constexpr int kSplitMin = 32;        // batches of at least this many streams are split over the lanes; smaller ones take one
                                     // lane each, in turn (their cost is launches, not kernel time)

// The launch groups a batch of n streams asks for: as many as the lanes' bins need (`group` streams each at most), and, with
// several lanes, a multiple of the lanes for batches worth splitting, so that every lane gets the same amount of work.
inline int groups_asked(int n, int group, int lanes)
{
  const int g = group > 1 ? group : 1;
  int k = (n + g - 1) / g;
  if (k < 1) k = 1;
  if (lanes > 1 && n >= kSplitMin) k = ((k + lanes - 1) / lanes) * lanes;
  return k;
}

// The launch groups enqueue_batch makes: ceil(n / k) streams each, which can come to FEWER than k groups (100 streams in 16
// groups of 7 are 15).  The batch's status word starts at this number and every group takes one off.  Not monotone in n:
// 3 lanes, groups of 8 streams, 48 streams make 6 groups and 49 make 9.
inline int groups_for(int n, int group, int lanes)
{
  const int m = n > 1 ? n : 1, k = groups_asked(n, group, lanes);
  const int per_group = (m + k - 1) / k;
  return (m + per_group - 1) / per_group;
}

// Counter blocks (one per launch group) a batch slot needs for any batch of 1 .. max_streams streams.  groups_asked is
// monotone in n -- ceil(n / group) is, rounding up to a multiple of the lanes is, and the switch to that rounding at kSplitMin
// only raises it -- and groups_for(n) = ceil(n / ceil(n / k)) <= k.  So groups_asked(max_streams) bounds groups_for(n) for
// every n up to max_streams.  (groups_for(max_streams) does not: 3 lanes, groups of 8, max_streams 64 make 8 groups and a
// batch of 49 makes 9.)
inline int counter_blocks_for(int max_streams, int group, int lanes)
{
  return groups_asked(max_streams, group, lanes);
}

}  // namespace rtuf
