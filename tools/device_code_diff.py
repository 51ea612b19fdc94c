#!/usr/bin/env python
"""Is the device code of two trees the same, symbol by symbol?  (The condition of DESIGN.md 3.12 for a change that only moves text.)

   python tools/device_code_diff.py <tree A> <tree B> [-j JOBS] [file.hip ...]

A tree is a checkout of this repository - every source of kvzip_amd/csrc/Makefile's SRCS (or the files named) is compiled with the
Makefile's compiler and flags plus `--cuda-device-only -S`, no GPU needed - or a directory of such `.s` files.  Per file the tool
prints the number of symbols (every function of the device assembly, __global__ or not) and the names of those that differ, and exits
1 if any does.  Two symbols are the same when their instruction streams agree line by line after comments are dropped and local labels
are renumbered in order of appearance, and, for a kernel, when the lines of its `.amdhsa_kernel` descriptor (registers, LDS, scratch)
agree.  The comparison is of text alone."""
import argparse, concurrent.futures, os, re, subprocess, sys, tempfile

CSRC = os.path.join("kvzip_amd", "csrc")


def make_vars(tree):
    """HIPCC, ARCH, CXXFLAGS and SRCS as csrc/Makefile sets them ($(ARCH) expanded; the environment overrides `?=` as make does)"""
    v = {}
    for line in open(os.path.join(tree, CSRC, "Makefile")):
        m = re.match(r"^(\w+)\s*(\?=|=)\s*(.*)$", line.rstrip("\n"))
        if m:
            v[m.group(1)] = os.environ.get(m.group(1), m.group(3)) if m.group(2) == "?=" else m.group(3)
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: v.get(m.group(1), ""), s)
    return expand(v["HIPCC"]), expand(v["CXXFLAGS"]).split(), v["SRCS"].split()


def assemble(tree, names, tmp, pool):
    """{file.hip: path of its device assembly}, and the compilations under way for them"""
    if not os.path.isfile(os.path.join(tree, CSRC, "Makefile")):   # a directory of .s files
        have = sorted(f[:-2] + ".hip" for f in os.listdir(tree) if f.endswith(".s"))
        return {n: os.path.join(tree, n[:-4] + ".s") for n in (names or have)}, []
    hipcc, flags, srcs = make_vars(tree)
    out = {n: os.path.join(tmp, n[:-4] + ".s") for n in (names or srcs)}
    run = lambda n: subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", n, "-o", out[n]], cwd=os.path.join(tree, CSRC), check=True)
    return out, [pool.submit(run, n) for n in out]


def symbols(path):
    """{symbol: normalised text}: the body of every function, and '<name> [descriptor]' for every kernel descriptor"""
    lines = [re.sub(r"\s*;.*$", "", l.rstrip("\n")).rstrip() for l in open(path)]   # (no string holds a ';' in device assembly)
    syms, i = {}, 0
    while i < len(lines):
        m = re.match(r"^\s*\.type\s+([^\s,]+),@function$", lines[i])
        if m:
            name, body, desc, labels = m.group(1), [], None, {}
            while lines[i] != name + ":":
                i += 1
            i += 1
            while not re.match(r"^\.Lfunc_end\d+:$", lines[i]):   # (a kernel's descriptor stands in front of the end of its function)
                l = lines[i].strip()
                if l.startswith(".amdhsa_kernel "):
                    desc = []
                elif l == ".end_amdhsa_kernel":
                    syms[name + " [descriptor]"], desc = "\n".join(desc), None
                elif desc is not None:
                    desc.append(l)
                elif l:
                    body.append(lines[i])
                i += 1
            for l in body:                                   # local labels in order of definition
                lm = re.match(r"^(\.L\w+):$", l)
                if lm:
                    labels[lm.group(1)] = ".L%d" % len(labels)
            syms[name] = "\n".join(re.sub(r"\.L\w+", lambda x: labels.get(x.group(0), x.group(0)), l) for l in body)
        i += 1
    return syms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("files", nargs="*", help="sources to compare (default: the Makefile's SRCS)")
    ap.add_argument("-j", "--jobs", type=int, default=min(16, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    differing = 0
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:   # (both trees at once: the longest file sets the time)
            (sa, ra), (sb, rb) = assemble(args.a, args.files, ta, pool), assemble(args.b, args.files, tb, pool)
            for r in ra + rb:
                r.result()
        for n in sorted(set(sa) | set(sb)):
            if n not in sa or n not in sb:
                print("%-24s only in %s" % (n, args.a if n in sa else args.b))
                differing += 1
                continue
            x, y = symbols(sa[n]), symbols(sb[n])
            bad = sorted(s for s in set(x) | set(y) if x.get(s) != y.get(s))
            funcs = sum(1 for s in x if not s.endswith(" [descriptor]"))
            print("%-24s %3d symbols (%d kernels)  %s" % (n, funcs, len(x) - funcs, "identical" if not bad else "%d DIFFER" % len(bad)))
            for s in bad:
                print("    %s%s" % (s, "" if s in x and s in y else "  (only in %s)" % (args.a if s in x else args.b)))
            differing += len(bad)
    print("all symbols identical" if not differing else "%d symbols differ" % differing)
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
