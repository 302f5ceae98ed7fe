"""CPU (-m "not gpu"): the bit-pattern identities of the round-6 tile kernel.

gfx950 issues float add / mul / fma, integer add / sub, logic and right shifts at two cycles per wave64 instruction and
conversions, v_rndne, compares, selects, 24-bit multiplies and left shifts at four (profiles/valu_peak.json); the hot walks
replace instructions of the second kind by ones of the first wherever both give the same bits.  Whether
they do is arithmetic, not a GPU matter: tests/fast_class_check.cpp runs the kernels' own functions (rtuf_numerics.h) against
the forms they replace for every float z > 0.5, every 24-bit depth of the upper half and 120 M vertex pairs (~15 s)."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "realtime_urdf_filter_amd", "csrc")


def test_bit_pattern_identities_hold_for_every_input(tmp_path):
    exe = str(tmp_path / "fast_class_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", exe, os.path.join(HERE, "fast_class_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 1_100_000_000


def test_the_identities_are_used_only_where_they_hold():
    """z24_of_upper_half and z_of_upper_half_z24 hold for depths of the upper half only: the kernels may use them only in tiles
    without near geometry -- where the set-up's near flag (window z below 0.51 somewhere in the box) promises that."""
    dev = open(os.path.join(CSRC, "rtuf_kernels.hip")).read()
    # depth tests: not in the LOW instance (tiles with near geometry) nor in the exact-z pass
    assert dev.count("((!LOW && MODE == 0) ? z24_of_upper_half(z) : z24_of(z))") == 2
    # the cover-only tile: only without near geometry
    assert "near_tile ? z24_of(zf) : z24_of_upper_half(zf)" in dev
    # no exact-z pass outside tiles with near geometry, and the winner's z from its key by the upper-half form only there
    assert re.search(r"bool need = false;\s*if \(near_tile\) \{", dev)
    assert re.search(r"if \(!near_tile\) \{[^\n]*\n\s*z\[j\] = z_of_upper_half_z24\(khi\);", dev)
    # the near flag: window z below 0.51 anywhere in the box
    assert "return !(plane_min(a0, dzdx, dzdy, bx0, bx1, by0, by1) >= 0.51f) ? kNearBit : 0u;" in dev
