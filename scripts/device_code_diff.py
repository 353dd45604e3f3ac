#!/usr/bin/env python3
"""Compare the device code of two source trees, kernel by kernel.  No GPU needed.

For every object of the native library that holds kernels (the 7 tile objects, the 7 long-filter objects,
fft_f64, nd_f64, direct_f64, long_f64, long_step) the device side of both trees is compiled to assembly text with the flags of
csrc/Makefile (`hipcc ... --cuda-device-only -S`).  The kernels of the two sides are put in one-to-one
correspondence by demangled name -- conv1d_pers_kernel by (P, S, CIB, NB, NT) and the set of features its parameter
list switches on, in either spelling: the seven positional parameters or the pers:: feature mask -- and each pair is
compared in

  * the instruction text between the kernel's label and its .Lfunc_end, with the kernel's own mangled name and
    the function number in its local labels (.LBB<n>_, and BB<n>_ in comments) replaced by placeholders;
  * the metadata fields of FIELDS below.

Exit status 0 only if every object has the same kernels on both sides and every pair is identical.

    git worktree add /tmp/parent HEAD~1        # (or git archive)
    python scripts/device_code_diff.py /tmp/parent . [--jobs 8] [--only tile_32] [--keep DIR]
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

CSRC = os.path.join("fft_conv_pytorch_amd", "csrc")
# as csrc/Makefile: CXXFLAGS, TILES (P S NT), LONG_TILES (P S)
CXXFLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I../../include", "-I.", "-Wno-unused-result",
            "-fno-slp-vectorize"]
TILES = ["8_1_64", "8_2_64", "16_1_64", "16_2_128", "32_1_128", "32_2_256", "32_4_512"]
LONG_TILES = ["8_1", "8_2", "16_1", "16_2", "32_1", "32_2", "32_4"]
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
          ".max_flat_workgroup_size", ".kernarg_segment_size")
# conv1d_pers_kernel's build: the positional parameters behind <P, S, CIB, NB, NT, of the old list (None: not a feature),
# and the bits of the mask that replaced them (pers:: in conv1d_pers.hpp)
OLD_PERS = ("phases", None, "depthwise", "segments", "pairs", "stamps", "quads", "half_io")
NEW_PERS = ("phases", "pairs", "quads", "depthwise", "segments", "stamps", "half_io")


def objects():
    objs = []
    for t in TILES:
        p, s, nt = t.split("_")
        objs.append(("tile_" + t, "tile_inst.hip", ["-DFC_P=" + p, "-DFC_S=" + s, "-DFC_NT=" + nt]))
    for t in LONG_TILES:
        p, s = t.split("_")
        objs.append(("long_" + t, "long_inst.hip", ["-DFC_P=" + p, "-DFC_S=" + s]))
    for n in ("fft_f64", "nd_f64", "direct_f64", "long_f64", "long_step"):
        objs.append((n, n + ".hip", []))
    return objs


def tools():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    filt = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(filt):
        filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt:
        sys.exit("no llvm-cxxfilt / c++filt found")
    return hipcc, filt


def compile_device(hipcc, tree, src, defs, out, reuse):
    if reuse and os.path.exists(out):
        return out
    cmd = [hipcc] + CXXFLAGS + defs + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s failed in %s:\n%s" % (" ".join(cmd), tree, r.stderr[-2000:]))
    return out


def pers_key(name):
    """conv1d_pers_kernel<...>(...) -> geometry and feature set, whichever parameter list spells it."""
    m = re.search(r"conv1d_pers_kernel<([^>]*)>", name)
    if not m:
        return name
    args = [a.strip() for a in m.group(1).split(",")]
    geo, rest = args[:5], args[5:]
    if len(rest) == 1:
        mask = int(rest[0].rstrip("uU"))
        if mask >> len(NEW_PERS):
            raise ValueError("unknown feature bit in " + name)
        feats = [f for i, f in enumerate(NEW_PERS) if mask >> i & 1]
    elif len(rest) == len(OLD_PERS):
        if rest[1] != "2":
            raise ValueError("RING != 2 in " + name)
        feats = [f for f, v in zip(OLD_PERS, rest) if f and v in ("true", "1")]
    else:
        raise ValueError("unknown parameter list: " + name)
    return "conv1d_pers_kernel<%s> [%s]" % (", ".join(geo), " ".join(sorted(feats)) or "plain")


def parse(path, filt):
    """-> {key: (instruction lines, {field: value})}"""
    text = open(path).read()
    lines = text.split("\n")
    # metadata: the entries of amdhsa.kernels, kernel-level keys at an indent of 4 (the first behind "  - ")
    meta, cur, inside = {}, None, False
    for ln in lines:
        if ln.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if inside and ln and not ln.startswith(" "):
            inside = False
        if not inside:
            continue
        m = re.match(r"^(  - |    )(\.\w+):\s*(.*)$", ln)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        cur[m.group(2)] = m.group(3).strip()
        if m.group(2) == ".name":
            meta[m.group(3).strip().strip("'\"")] = cur
    names = sorted(meta)
    dem = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for sym, d in zip(names, dem):
        start = next(i for i, ln in enumerate(lines) if ln.startswith(sym + ":"))      # (a comment follows the label)
        end = next(i for i in range(start, len(lines)) if re.match(r"^\.Lfunc_end\d+:", lines[i]))
        body = [re.sub(r"BB\d+_", "BB_", ln.replace(sym, "@KERNEL@")) for ln in lines[start:end]]
        key = pers_key(re.sub(r"^void ", "", d))
        if key in out:
            raise ValueError("two kernels named " + key)
        out[key] = (body, {f: meta[sym].get(f) for f in FIELDS})
    return out


def compare(name, old, new, verbose):
    """-> (number of kernels on both sides, list of findings)"""
    bad = []
    for k in sorted(set(old) - set(new)):
        bad.append("only in the old tree: " + k)
    for k in sorted(set(new) - set(old)):
        bad.append("only in the new tree: " + k)
    for k in sorted(set(old) & set(new)):
        (bo, mo), (bn, mn) = old[k], new[k]
        if mo != mn:
            bad.append("metadata differs: %s\n      old %s\n      new %s" % (k, mo, mn))
        if bo != bn:
            d = list(difflib.unified_diff(bo, bn, "old", "new", lineterm="", n=2))
            bad.append("instructions differ: %s (%d diff lines)\n%s" % (k, len(d), "\n".join("      " + x for x in d[:verbose])))
    return (len(old), len(new)), bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--only", default="", help="objects whose name contains this")
    ap.add_argument("--keep", default=None, help="keep the assembly files in this directory")
    ap.add_argument("--reuse", action="store_true", help="do not recompile what --keep already holds (same trees only)")
    ap.add_argument("--diff-lines", type=int, default=40, help="lines of a differing kernel's diff to print")
    a = ap.parse_args()
    hipcc, filt = tools()
    objs = [o for o in objects() if a.only in o[0]]
    work = a.keep or tempfile.mkdtemp(prefix="device_code_diff_")
    os.makedirs(work, exist_ok=True)
    failed = False
    try:
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
            futs = {}
            for name, src, defs in sorted(objs, key=lambda o: not o[0].startswith("tile_32")):   # the slowest first
                for side, tree in (("old", a.old_tree), ("new", a.new_tree)):
                    out = os.path.join(os.path.abspath(work), "%s.%s.s" % (name, side))
                    futs[(name, side)] = pool.submit(compile_device, hipcc, os.path.abspath(tree), src, defs, out, a.reuse)
            total = 0
            for name, _, _ in objs:
                old = parse(futs[(name, "old")].result(), filt)
                new = parse(futs[(name, "new")].result(), filt)
                (no, nn), bad = compare(name, old, new, a.diff_lines)
                npers = sum(1 for k in new if k.startswith("conv1d_pers_kernel"))
                note = " (%d conv1d_pers_kernel builds)" % npers if npers else ""
                total += nn
                if bad or no != nn:
                    failed = True
                    print("%-16s %3d / %3d kernels%s  DIFFERENT" % (name, no, nn, note))
                    for b in bad:
                        print("    " + b)
                else:
                    print("%-16s %3d kernels%s  identical" % (name, nn, note))
                sys.stdout.flush()
        print("%d objects, %d kernels: %s" % (len(objs), total, "DIFFERENT" if failed else "all identical"))
    finally:
        if not a.keep:
            shutil.rmtree(work, ignore_errors=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
