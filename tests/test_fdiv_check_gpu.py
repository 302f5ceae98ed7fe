"""GPU (-m gpu): the compare threshold's division core (rtuf::div_core) gives the IEEE quotient for every operand pair the
library admits it for (rtuf::fast_div_admitted).  scripts/bin/fdiv_check (built by build()) runs both with the library's own
functions over every float z in [-1, 1 + 2^-11] for the library's default planes, four other plane pairs and a few random
constant pairs of the admitted domain."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDOM_PAIRS = 6


def test_div_core_equals_ieee_division_on_the_admitted_domain():
    exe = os.path.join(ROOT, "scripts", "bin", "fdiv_check")
    assert os.path.exists(exe), "%s is missing: run build()" % exe
    r = subprocess.run([exe, str(N_RANDOM_PAIRS)], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-2000:])
    m = re.search(r"^admitted domain: 0 differing of (\d+) quotients", r.stdout, re.M)
    assert m, r.stdout[-3000:]
    # the default planes (z_near 0.1, z_far 10) are admitted, and so are at least half of the random pairs
    assert int(m.group(1)) >= (1 + N_RANDOM_PAIRS // 2) * (0x3F801001 + 0x3F800001), r.stdout[-3000:]
    assert re.search(r"^num \S+ off \S+ \(library default z_near 0\.1 z_far 10\): 0 differing", r.stdout, re.M), r.stdout[-3000:]
