"""CPU (-m "not gpu"): the tile kernel's depth keys carry the low bits of a near fragment's float z so that the winner's
gl_FragCoord.z -- finer than the 24-bit depth below window z 0.5 -- is recovered without rasterising anything twice.
tests/near_key_check.cpp runs the functions involved (z24_of, near_z_from_key, exact_z_floor, key_shift_for: rtuf_numerics.h,
shared with the kernels and the host) and checks the round trip for EVERY float in the range the encoding claims, for every
key shift the library can choose (763 M cases, ~6 s)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "realtime_urdf_filter_amd", "csrc")


def test_every_near_float_is_recovered_from_its_key(tmp_path):
    exe = str(tmp_path / "near_key_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-I", CSRC, "-o", exe, os.path.join(HERE, "near_key_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 700_000_000


def test_the_kernel_decodes_only_the_range_the_check_covers():
    """near_z_from_key is exact for z24 in [exact_z_floor(shift), 2^23] with the shift the host chose by key_shift_for: below
    that floor a winner takes the exact-z pass, above 2^23 the upper-half form (tests/fast_class_check.cpp)."""
    dev = open(os.path.join(CSRC, "rtuf_kernels.hip")).read()
    api = open(os.path.join(CSRC, "rtuf_api.cpp")).read()
    assert "c->key_shift = key_shift_for((uint32_t)tri_seq);" in api
    assert "kf.zexact = near_tile ? exact_z_floor(a.key_shift) : 8388609u;" in dev
    assert dev.count("(uint32_t)(k >> 32) < kf.zexact") == 2          # the exact-z pass: the scan and the winners' filter
    assert "if (khi <= 8388608u) z[j] = near_z_from_key(khi, (uint32_t)k & kf.lowmask, kf.shift);" in dev
