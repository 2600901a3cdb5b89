"""gfx950 device assembly listings of the three kernel-heavy translation units, with build.py's own flags.

    python tools/device_listing.py OUTDIR      # writes OUTDIR/{render,preprocess,radix_sort}.s

A source change that is meant to leave the kernels alone is checked by running this at both commits and comparing
the files (`diff -r`).  The `__hip_cuid_*` symbol lines, which differ between any two compiles, are left out.
"""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ("render.hip", "preprocess.hip", "radix_sort.hip")


def main(outdir):
    spec = importlib.util.spec_from_file_location("gsr_build", os.path.join(ROOT, "gs-livm_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    os.makedirs(outdir, exist_ok=True)
    for unit in UNITS:
        cmd = [b.HIPCC] + b.COMMON + b.UNITS[unit] + ["--cuda-device-only", "-S", os.path.join(b.CSRC, unit), "-o", "-"]
        text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout
        lines = [l for l in text.splitlines() if "__hip_cuid_" not in l]
        with open(os.path.join(outdir, unit.replace(".hip", ".s")), "w") as f:
            f.write("\n".join(lines) + "\n")
        print("%s: %d lines" % (unit, len(lines)))


if __name__ == "__main__":
    main(sys.argv[1])
