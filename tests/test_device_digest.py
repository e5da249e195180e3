"""tools/device_digest.py hashes a translation unit's gfx950 device assembly; a source clean-up shows that it left the kernels untouched by
comparing the digests of two checkouts.  That only means something if two compiles of one source give one digest (the fixed -cuid):
checked here on the smallest unit.  Cross-compiles; needs no GPU."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "device/probe_kernels.hip"


def _digest():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "device_digest.py"), UNIT], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    assert len(lines) == 1 and lines[0].split()[1:] == [UNIT], p.stdout
    return lines[0].split()[0]


def test_two_compiles_of_one_unit_give_one_digest():
    a, b = _digest(), _digest()
    assert a == b and re.fullmatch(r"[0-9a-f]{64}", a)
