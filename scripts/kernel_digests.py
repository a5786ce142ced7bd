#!/usr/bin/env python3
"""One sha256 per compiled device function, for proving that a source change
leaves the generated code alone: run it at both commits and diff the lists.

usage: scripts/kernel_digests.py OUT.txt [jobs]

Covers the ahead-of-time library (make -C go-raytracer_amd/csrc asm), the same
with the phase target's flags, every case of scripts/spec_matrix.sh compiled as
scripts/spec_regs.sh compiles it, and every key of
tests/test_specialize.py::_spec_matrix translated to defines as spec_compile
does. A function is the text from its "Begin function" line to the next one's (its
code, its .amdhsa_kernel block and resource lines) plus its metadata entry;
lines naming __hip_cuid_ (a hash of the translation unit) are dropped first.
Lines: "<build>/<function> <sha256>".
"""
import concurrent.futures as cf
import hashlib
import os
import re
import subprocess
import sys
import tempfile

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(R, "go-raytracer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def split(path):
    """{function: text} of one .s file: the code section from a function's
    "Begin function" line to the next one's, and its metadata entry."""
    parts = {}
    name = "(head)"
    meta = False
    for l in open(path).read().split("\n"):
        if "__hip_cuid_" in l:
            continue
        m = re.search(r"; -- Begin function (\S+)", l)
        if m:
            name = m.group(1)
        elif ".amdgpu_metadata" in l:
            name, meta = "(metadata)", not meta
        elif meta and l.startswith("  - ."):  # a kernel's entry: named by its .name line, below
            name = "(entry)"
            parts[name] = []
        elif meta and not l.startswith("   "):
            name = "(metadata)"
        parts.setdefault(name, []).append(l)
        m = re.match(r"    \.name:\s+(\S+)", l)
        if meta and m and name == "(entry)":
            name = m.group(1)
            parts.setdefault(name, []).extend(parts.pop("(entry)"))
    return {n: "\n".join(t) for n, t in parts.items()}


def spec_cases():
    cases = []
    # scripts/spec_matrix.sh
    base = "-DRT_SPEC_KMASK=%d -DRT_SPEC_FEAT=0 -DRT_SPEC_NLIGHTS=%d -DRT_SPEC_POWBITS=6"
    for km in (1, 3, 7, 15, 31):
        for nl in (1, 2, 3, 4, 8):
            for q in ("false", "true"):
                cases.append((base % (km, nl) + " -DRT_CULL=0", "false false false " + q))
    for km in (3, 15):
        for nl in (2, 4):
            cases.append((base % (km, nl), "false true false true"))
            cases.append((base % (km, nl) + " -DRT_SHARE=2", "true true false true"))
    for nl in (1, 2, 3):
        cases.append((base % (39, nl) + " -DRT_SHARE=2", "true false true true"))
        cases.append((base % (39, nl) + " -DRT_SHARE=2 -DRT_PAIRS=1", "true false true false"))
    c3 = "-DRT_SPEC_KMASK=15 -DRT_SPEC_FEAT=0 -DRT_SPEC_NOBJ=4 -DRT_SPEC_KINDS=1,3,2,0 -DRT_SPEC_NLIGHTS=%d -DRT_SPEC_POWBITS=6"
    for nl in (1, 3, 4, 5, 8):
        for q in ("false", "true"):
            cases.append((c3 % nl, "true false false " + q))
    cases.append(("-DRT_SPEC_KMASK=15 -DRT_SPEC_FEAT=7 -DRT_SPEC_NOBJ=8 -DRT_SPEC_KINDS=0,0,0,0,1,2,3,0 -DRT_SPEC_NLIGHTS=8 "
                  "-DRT_SPEC_POWBITS=7", "true false false false"))
    cases.append(("-DRT_SPEC_KMASK=31 -DRT_SPEC_FEAT=7 -DRT_SPEC_NLIGHTS=3 -DRT_SPEC_POWBITS=7", "true true false true"))
    cases.append((c3 % 4 + " -DRT_SHARE=1", "true false false false"))
    cases.append((c3 % 4 + " -DRT_PAIRS=1", "true false false false"))
    # tests/test_specialize.py::_spec_matrix, as rt_kernel.hip spec_compile turns a key into options
    # (the function's text alone: the module imports the built package)
    test = open(os.path.join(R, "tests", "test_specialize.py")).read()
    ns = {}
    exec(re.search(r"^def _spec_matrix\(\):\n(?:(?: .*)?\n)+", test, re.M).group(0), ns)
    for key in ns["_spec_matrix"]():
        lds, bvh, csg, nobj, kinds, kmask, feat, nl, pb, nocull, sch, share, far = key.split(":")
        d = ["-DRT_SPEC_KMASK=" + kmask, "-DRT_SPEC_FEAT=" + feat]
        if int(nobj) > 0:
            d += ["-DRT_SPEC_NOBJ=" + nobj, "-DRT_SPEC_KINDS=" + kinds]
        if int(nl) > 0:
            d.append("-DRT_SPEC_NLIGHTS=" + nl)
        d.append("-DRT_SPEC_POWBITS=" + pb)
        if int(nocull):
            d.append("-DRT_CULL=0")
        if int(share):
            d.append("-DRT_SHARE=" + share)
        if int(sch) == 2:
            d.append("-DRT_PAIRS=1")
        if not int(far):
            d.append("-DRT_FAR_SHIFT=0")
        b = lambda v: "true" if int(v) else "false"
        cases.append((" ".join(d), " ".join((b(lds), b(bvh), b(csg), b(int(sch) == 1)))))
    return sorted(set(cases))


def digests(tag, path):
    return ["%s/%s %s" % (tag, n, hashlib.sha256(t.encode()).hexdigest()) for n, t in sorted(split(path).items())]


def library(tmp, tag, extra):
    """The Makefile's asm target (its flags), with extra defines in front."""
    s = os.path.join(tmp, tag + ".s")
    line = subprocess.run(["make", "-C", CSRC, "-n", "-B", "asm"], check=True, capture_output=True, text=True).stdout
    cmd = next(l for l in line.split("\n") if "--cuda-device-only" in l).replace("-o rt_kernel.s", "-o " + s)
    subprocess.run(cmd + " " + extra, shell=True, check=True, cwd=CSRC)
    return digests(tag, s)


def spec(tmp, n, case):
    defs, tmpl = case
    src, s = os.path.join(tmp, "spec%d.hip" % n), os.path.join(tmp, "spec%d.s" % n)
    open(src, "w").write('#include "rt_render.h"\ntemplate __global__ void rt_render_kernel<%s>(const char*, Params);\n'
                         % ", ".join(tmpl.split()))
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + R + "/include",
                    "-I" + CSRC, "--cuda-device-only", "-S", "-o", s, src] + defs.split(), check=True)
    return digests("spec[%s][%s]" % (tmpl, defs), s)


def main():
    out, jobs = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 6
    cases = spec_cases()
    subprocess.run(["make", "-C", CSRC, "rt_jit_src.inc"], check=True, capture_output=True)  # (the library embeds it)
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(jobs) as ex:
        futs = [ex.submit(library, tmp, "lib", ""), ex.submit(library, tmp, "lib-phase", "-DRT_PHASE_TIMING -DRT_EXACT_DIAG")]
        futs += [ex.submit(spec, tmp, n, c) for n, c in enumerate(cases)]
        lines = [l for f in futs for l in f.result()]
    open(out, "w").write("\n".join(lines) + "\n")
    print("%d functions in %d builds -> %s" % (len(lines), 2 + len(cases), out))


if __name__ == "__main__":
    main()
