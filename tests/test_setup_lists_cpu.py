"""CPU (-m "not gpu"): the set-up kernel keeps the fill of its three survivor lists as 10-bit fields of one LDS word, so that
a wave reserves in all three with one addition.  tests/setup_lists_check.cpp runs the helpers (list_counts and its fields:
rtuf_numerics.h, the bodies the kernel compiles) for every split of 768 entries over the three lists, for sums built wave by
wave, with a field at 768 and with the near hand-over's "+ 1"."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "realtime_urdf_filter_amd", "csrc")


def test_packed_list_counters(tmp_path):
    exe = str(tmp_path / "setup_lists_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", exe, os.path.join(HERE, "setup_lists_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 300_000


def test_the_kernel_uses_the_checked_helpers():
    """Every list fits its field, the wave's one addition and the hand-over go through the helpers."""
    dev = open(os.path.join(CSRC, "rtuf_kernels.hip")).read()
    assert "static_assert(kStreamsPerBlock * kBlock <= (int)kListFieldMask" in dev
    assert "atomicAdd(&s_counts, list_counts((uint32_t)__popcll(sm), (uint32_t)__popcll(tm), (uint32_t)__popcll(qm)))" in dev
    assert "s_list[list_count_rec(atomicAdd(&s_counts, 1u))] = (uint16_t)ent;" in dev
