#!/usr/bin/env python3
"""The resources the compiler gives every kernel of a device file -- registers, spills, scratch, LDS, occupancy -- from
hipcc's -Rpass-analysis=kernel-resource-usage remarks: the one path `make asm`, the records under profiles/ and the resource
tests (tests/kernel_resources.py) share.  The flags are the Makefile's (`make print-hipflags`), stated nowhere else.

usage: kernel_usage.py remarks.txt        one line per kernel of a compile's stderr, names demangled (`make asm`)
       kernel_usage.py --record NAME      compiles csrc/NAME.hip and prints profiles/NAME_kernel_usage.txt"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudabrot_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FIGURES = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


def parse_remarks(text):
    """[{"name": mangled, remark: value}] of a compile's stderr, one per kernel, in the compiler's order."""
    kernels, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:") or body.startswith("Name:"):
            cur = {"name": body.split(":", 1)[1].strip()}
            kernels.append(cur)
        elif cur is not None and ":" in body:
            k, v = body.split(":", 1)
            cur[k.strip()] = v.strip()
    return kernels


def compile_kernels(name, defines=()):
    """(kernels, assembly) of cudabrot_amd/csrc/<name>.hip built for the device with the Makefile's flags and `defines`."""
    flags = subprocess.run(["make", "-s", "--no-print-directory", "-C", CSRC, "print-hipflags"], capture_output=True,
                           text=True, check=True).stdout.split()
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([HIPCC, *flags, *defines, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                              "-o", os.path.join(tmp, "kernels.s"), os.path.join(CSRC, name + ".hip")],
                             capture_output=True, text=True, cwd=CSRC)
        assert out.returncode == 0, out.stderr[-2000:]
        with open(os.path.join(tmp, "kernels.s")) as f:
            return parse_remarks(out.stderr), f.read()


def figures(k):
    """(VGPRs, AGPRs, SGPRs, scratch, LDS, waves per SIMD) of a kernel: what a record holds it to."""
    return tuple(int(k[f]) for f in FIGURES)


def row(k, name=None):
    """A kernel as one line: a record's row under its mangled name, `make asm`'s under `name`."""
    return (f"{name or k['name']:60s} VGPR {k.get('VGPRs','?'):>4} AGPR {k.get('AGPRs','?'):>3} "
            f"SGPR {k.get('TotalSGPRs', k.get('SGPRs','?')):>4} "
            f"spill s/v {k.get('SGPRs Spill','?')}/{k.get('VGPRs Spill','?')} scratch {k.get('ScratchSize [bytes/lane]','?')} "
            f"LDS {k.get('LDS Size [bytes/block]','?')} occ {k.get('Occupancy [waves/SIMD]','?')}")


def write_record(name, kernels, out):
    out.write(f"# {name}.hip: kernel resource usage, written by `python3 tools/kernel_usage.py --record {name}` "
              "(hipcc for gfx950, the Makefile's HIPFLAGS)\n")
    for k in kernels:
        out.write(row(k) + "\n")


def read_record(name):
    """{mangled name: figures} of profiles/<name>_kernel_usage.txt; a row with a spill does not parse."""
    rows = {}
    with open(os.path.join(ROOT, "profiles", name + "_kernel_usage.txt")) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            m = re.match(r"(\S+)\s+VGPR\s+(\d+) AGPR\s+(\d+) SGPR\s+(\d+) spill s/v 0/0 scratch (\d+) LDS (\d+) occ (\d+)$",
                         line.rstrip())
            assert m, line
            rows[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
    return rows


def demangled(name):
    try:
        name = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-cxxfilt", name], capture_output=True, text=True).stdout.strip() or name
    except OSError:
        pass
    return re.sub(r"\(cb::DrawArgs\)|cb::\(anonymous namespace\)::|void ", "", name)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        write_record(sys.argv[2], compile_kernels(sys.argv[2])[0], sys.stdout)
    elif len(sys.argv) == 2 and not sys.argv[1].startswith("-"):
        with open(sys.argv[1]) as f:
            for k in parse_remarks(f.read()):
                print(row(k, demangled(k["name"])))
    else:
        sys.exit(__doc__)
