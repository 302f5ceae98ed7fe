"""The launch-group rule of realtime_urdf_filter_amd/csrc/rtuf_groups.h in Python, for the GPU tests' expectations (the CPU check
tests/launch_groups_check.cpp runs the library's own functions)."""

SPLIT_MIN = 32          # kSplitMin: batches of at least this many streams are split over the lanes


def groups_asked(n, group, lanes):
    """ceil(n / group), rounded up to a multiple of the lanes for batches of SPLIT_MIN streams or more."""
    k = max(-(-n // max(group, 1)), 1)
    if lanes > 1 and n >= SPLIT_MIN:
        k = -(-k // lanes) * lanes
    return k


def groups_for(n, group, lanes):
    """Launch groups a batch of n streams is split into: ceil(n / ceil(n / groups_asked))."""
    return -(-n // -(-n // groups_asked(n, group, lanes)))


def counter_blocks_for(max_streams, group, lanes):
    """Counter blocks per batch slot: an upper bound of groups_for(n) for every n <= max_streams."""
    return groups_asked(max_streams, group, lanes)
