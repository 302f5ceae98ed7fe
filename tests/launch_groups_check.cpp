/* Exhaustive CPU check of the launch-group rule (realtime_urdf_filter_amd/csrc/rtuf_groups.h), the product's own functions:
 * for lanes 1..8 (RTUF_MAX_LANES is a build setting), launch group 1..1024 and max_streams 1..4096, every batch of
 * 1 <= n <= max_streams streams
 *   1. makes no more groups than the counter blocks a slot of that context holds: groups_for(n) <= counter_blocks_for(M)
 *   2. puts no more streams in a group than a lane's bins hold: ceil(n / groups) <= group
 *   3. makes no empty group: (groups - 1) * per_group < n <= groups * per_group
 * One pass over n per (lanes, group): the running maximum of groups_for over n <= M is compared with the bound for M.
 * With argument "old" it runs check 1 against the bound the library used before, groups_for(M), and must find the known
 * counter-examples (the check has teeth): prints them and "violations <count>", the number of (lanes, group, max_streams)
 * whose counter blocks that bound leaves short; "old L G M" limits the search to lanes <= L, group <= G, max_streams <= M.
 * g++ -O2 -I realtime_urdf_filter_amd/csrc;  prints "ok <cases>" or the first failure. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rtuf_groups.h"

using namespace rtuf;

int main(int argc, char** argv)
{
  const bool old = argc > 1 && strcmp(argv[1], "old") == 0;
  const int kLanes = argc > 4 ? atoi(argv[2]) : 8, kGroup = argc > 4 ? atoi(argv[3]) : 1024, kStreams = argc > 4 ? atoi(argv[4]) : 4096;
  unsigned long long cases = 0, violations = 0;
  for (int lanes = 1; lanes <= kLanes; lanes++)
    for (int group = 1; group <= kGroup; group++) {
      int most = 0, most_n = 0;                 // largest groups_for(n) over n <= M so far, and the first n that makes it
      for (int n = 1; n <= kStreams; n++) {
        const int groups = groups_for(n, group, lanes);
        const int per_group = (n + groups - 1) / groups;
        if (groups < 1 || per_group > group || !((groups - 1) * per_group < n && n <= groups * per_group)) {
          printf("lanes %d group %d n %d: %d groups of %d streams\n", lanes, group, n, groups, per_group);
          return 1;
        }
        if (groups > most) { most = groups; most_n = n; }
        const int M = n;
        const int bound = old ? groups_for(M, group, lanes) : counter_blocks_for(M, group, lanes);
        if (most > bound) {
          if (!old) {
            printf("lanes %d group %d max_streams %d: n %d makes %d groups, counter blocks %d\n", lanes, group, M, most_n, most, bound);
            return 1;
          }
          if (violations < 8 || (lanes == 3 && group == 8 && M == 64) || (lanes == 2 && group == 5 && M == 33))
            printf("lanes %d group %d max_streams %d: n %d makes %d groups, counter blocks %d\n", lanes, group, M, most_n, most, bound);
          violations++;
        }
        cases++;
      }
    }
  if (old) { printf("violations %llu\n", violations); return 0; }
  printf("ok %llu\n", cases);
  return 0;
}
