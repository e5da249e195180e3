#!/usr/bin/env python3
"""sha256 of each translation unit's gfx950 device assembly, for showing that a source clean-up left the kernels untouched.

    python tools/device_digest.py [--root DIR] [UNIT ...]        prints "sha256  unit" per line

Every unit (default: all of build.py's SOURCES) is compiled with its flags from flag_manifest() plus
--offload-device-only -S -cuid=airwave; the fixed cuid makes two compiles of one source byte-identical.  --root points at another
checkout (a git worktree of the parent commit), so the two tables can be compared line by line.  The assembly is hashed only: never
read, searched or printed.  Cross-compiles, needs no GPU.  At most AW_BUILD_JOBS compiles side by side (default 8, never above 16).
"""
import argparse
import hashlib
import importlib.util
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor


def load_build(root):
    spec = importlib.util.spec_from_file_location("_aw_build_for_digest", os.path.join(root, "airwave_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)          # by path: importing the package would need the built library
    return m


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to digest (default: this one)")
    ap.add_argument("units", nargs="*", help="entries of build.py's SOURCES (default: all)")
    args = ap.parse_args(argv)
    b = load_build(os.path.abspath(args.root))
    units = args.units or b.SOURCES
    flags = b.flag_manifest()["flags_by_source"]
    unknown = [u for u in units if u not in flags]
    if unknown:
        ap.error("not in build.py's SOURCES: " + " ".join(unknown))

    def digest(unit):
        cmd = [b.hipcc()] + flags[unit] + (["-x", "hip"] if unit.endswith(".cpp") else []) + [
            "--offload-device-only", "-S", "-cuid=airwave", os.path.join(b.CSRC, unit), "-o", "-"]
        return hashlib.sha256(subprocess.run(cmd, check=True, stdout=subprocess.PIPE).stdout).hexdigest()

    jobs = max(1, min(16, int(os.environ.get("AW_BUILD_JOBS", "8"))))
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        for unit, h in zip(units, ex.map(digest, units)):
            print(f"{h}  {unit}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
