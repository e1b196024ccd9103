#!/usr/bin/env python3
"""Is the gfx950 device code of the working tree the same as that of another commit?

For a refactor of kernel sources that must not change what runs on the GPU.  Needs no GPU: every unit is compiled as a plain
device ELF (the Makefile's own command line for that unit, plus --cuda-device-only --no-gpu-bundle-output), once from the base
commit (git archive into a temporary directory) and once from the working tree, and compared PER FUNCTION:

  * the set of function symbols and their sizes                                   (llvm-readelf -sW)
  * every kernel's .vgpr_count, .sgpr_count, .agpr_count, .group_segment_fixed_size,
    .private_segment_fixed_size and spill counts from the metadata note          (llvm-readelf --notes)
  * every function's instructions with their encodings, cut at the symbol's size  (llvm-objdump -d)

Whole-file hashes are not compared: a reordered instantiation changes the order in which functions are emitted and nothing else.

    python tools/device_code_diff.py                      # every unit of the Makefile against HEAD
    python tools/device_code_diff.py --base HEAD~1 fft_row_f32.hip fft_half.hip

Exit status 0: identical; 1: some function differs (each one is named).
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("pyfft_amd", "csrc")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
META = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".vgpr_spill_count", ".sgpr_spill_count")


def run(cmd, **kw):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, **kw).stdout


def makefile_units(csrc):
    text = open(os.path.join(csrc, "Makefile")).read()
    return re.search(r"^SRCS_HIP\s*:=\s*(.*)$", text, re.M).group(1).split()


def compile_command(csrc, unit, out):
    """The Makefile's command for build/<unit>.o, turned into a device-only compile that writes `out`."""
    stem = os.path.splitext(unit)[0]
    lines = run(["make", "-n", "-B", "-C", csrc, "build/%s.o" % stem]).splitlines()
    words = shlex.split(next(l for l in lines if " -c " in l and unit in l))
    cmd, skip = [], 0
    for w in words:
        if skip:
            skip -= 1
        elif w in ("-MF", "-o"):
            skip = 1
        elif w not in ("-MMD", "-MP"):
            cmd.append(w)
    return cmd + ["--cuda-device-only", "--no-gpu-bundle-output", "-o", out]


def functions(elf):
    """{symbol: (size, metadata dict or None, sha256 of the instruction text)} for every function of a device ELF."""
    sizes, ends = {}, {}
    for line in run([os.path.join(LLVM, "llvm-readelf"), "-sW", "--symbols", elf]).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND":
            sizes[f[7]] = int(f[2])
            ends[f[7]] = int(f[1], 16) + int(f[2])
    meta, cur = {}, None
    for line in run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf]).splitlines():
        # one list item of amdhsa.kernels per kernel: "  - .key: value" opens it, "    .key: value" continues it
        m = re.match(r"(  - |    )(\.[a-z_]+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is not None and m.group(2) in META:
            cur[m.group(2)] = m.group(3)
        elif cur is not None and m.group(2) == ".name":
            meta[m.group(3)] = cur
    text = {}
    if sizes:
        dis = run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr",
                   "--disassemble-symbols=" + ",".join(sorted(sizes)), elf])
        name = None
        for line in dis.splitlines():
            m = re.match(r"<(\S+)>:$", line)
            if m:
                name = m.group(1)
                text[name] = hashlib.sha256()
            elif name:
                # "<instruction> // <address>: <encoding> [<branch target>]".  objdump runs on to the next symbol: cut at this one's
                # size (what follows is padding).  The address is dropped, the encoding and a branch's <symbol+offset> stay.
                m = re.match(r"(\t.*//) *([0-9A-Fa-f]+):(.*)$", line)
                if m and int(m.group(2), 16) < ends[name]:
                    text[name].update((m.group(1) + m.group(3)).encode() + b"\n")
    return {s: (sizes[s], meta.get(s), text[s].hexdigest() if s in text else None) for s in sizes}


def compare_unit(unit, base_csrc, new_csrc, base_out, new_out):
    elfs = []
    for csrc, outdir, reuse in ((base_csrc, base_out, True), (new_csrc, new_out, False)):
        out = os.path.join(outdir, os.path.splitext(unit)[0] + ".elf")
        if not (reuse and os.path.exists(out)):
            subprocess.run(compile_command(csrc, unit, out + ".tmp"), check=True, cwd=csrc)
            os.replace(out + ".tmp", out)
        elfs.append(functions(out))
    a, b = elfs
    diffs = ["only in base: " + s for s in sorted(set(a) - set(b))] + ["only in new: " + s for s in sorted(set(b) - set(a))]
    for s in sorted(set(a) & set(b)):
        for what, x, y in zip(("size", "metadata", "instructions"), a[s], b[s]):
            if x != y:
                diffs.append("%s differs: %s (%s -> %s)" % (what, s, x, y))
    kernels = sum(1 for s in b if b[s][1] is not None)
    return unit, len(b), kernels, sum(v[0] for v in b.values()), diffs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("units", nargs="*", help="units of pyfft_amd/csrc (default: every unit of the Makefile)")
    ap.add_argument("--base", default="HEAD", help="commit to compare the working tree against")
    ap.add_argument("--cache", help="directory that keeps the base commit's device ELFs between runs (default: rebuilt every time)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    new_csrc = os.path.join(ROOT, CSRC)
    units = args.units or makefile_units(new_csrc)
    rev = run(["git", "-C", ROOT, "rev-parse", "--short", args.base]).strip()
    units = [u for u in units if os.path.exists(os.path.join(new_csrc, u))] or sys.exit("no such unit")
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        base, new_out = os.path.join(tmp, "base"), os.path.join(tmp, "new")
        base_out = os.path.join(os.path.abspath(args.cache), rev) if args.cache else os.path.join(tmp, "base_elf")
        for d in (base, new_out, base_out):
            os.makedirs(d, exist_ok=True)
        tar = subprocess.Popen(["git", "-C", ROOT, "archive", args.base, CSRC, "include"], stdout=subprocess.PIPE)
        subprocess.run(["tar", "-x", "-C", base], stdin=tar.stdout, check=True)
        if tar.wait():
            sys.exit("git archive failed")
        print("device code of the working tree against %s, per function (symbols and sizes, register / LDS / scratch metadata, "
              "instruction text)" % rev)
        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
            jobs = [pool.submit(compare_unit, u, os.path.join(base, CSRC), new_csrc, base_out, new_out) for u in units]
            for j in jobs:
                unit, nfun, nker, nbytes, diffs = j.result()
                print("%-24s %4d functions (%4d kernels) %9d bytes of code  %s"
                      % (unit, nfun, nker, nbytes, "identical" if not diffs else "%d DIFFERENCES" % len(diffs)), flush=True)
                for d in diffs:
                    print("    " + d)
                bad += bool(diffs)
    print("%d units compared, %d differ" % (len(units), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
