#!/usr/bin/env python3
"""Which lines and branches of the kernel sources does the emulated (CPU) suite execute?

tests/emu compiles the product's own .hip and .h sources with g++, so a `--coverage -O1` build of the emulator library reports, per
line of multi_agent_rl_wrsn_amd/csrc, whether any test that is not marked gpu reaches it.  This tool

  1. builds that instrumented library into a temporary directory (nothing in the tree is copied, changed or rebuilt),
  2. points the emulator loader at it with WRSN_EMU_LIB (tests/emu/emu_env.py),
  3. runs `pytest -m "not gpu"` to its normal end, so that every worker process writes its counters on exit,
  4. reads the counters with gcov and writes, per source file under csrc/, the executed-line share, the taken-branch share and the
     unexecuted line ranges and the executed lines that still hold an untaken branch -- to stdout, or to the file given with -o.

    python tools/emu_coverage.py -o profiles/emu_coverage_after.txt

CPU only.  A line of a template or inline function counts as executed when any instantiation executed it, a branch as taken when any
instantiation took it; code that no translation unit instantiates has no counters and is not listed at all.  Lines between two
unexecuted lines that carry no code of their own (comments, continuation lines) are folded into the range.  DESIGN.md section 2 says
what the figure does not see."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi_agent_rl_wrsn_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")
# tests/emu/Makefile's flags, with -O1 --coverage in place of -O2 (lines and branches stay attributable)
CXXFLAGS = ["-O1", "-g", "--coverage", "-std=c++17", "-fPIC", "-ffp-contract=off", "-w"]
UNITS = ((os.path.join(EMU, "emu_runtime.cpp"), "emu_runtime"), (os.path.join(CSRC, "wrsn_api.hip"), "wrsn_api"))


def build(tmp, cxx):
    objs = []
    for src, stem in UNITS:
        obj = os.path.join(tmp, stem + ".o")
        subprocess.check_call([cxx] + CXXFLAGS + ["-I" + os.path.join(EMU, "include"), "-c", "-o", obj, "-x", "c++", src], cwd=tmp)
        objs.append(obj)
    lib = os.path.join(tmp, "libwrsn_emu.so")
    subprocess.check_call([cxx, "--coverage", "-shared", "-o", lib] + objs, cwd=tmp)
    return lib


def run_suite(lib, workers, extra):
    env = dict(os.environ, WRSN_EMU_LIB=lib, PYTHONDONTWRITEBYTECODE="1")
    cmd = [sys.executable, "-m", "pytest", "-m", "not gpu", "-q", "-p", "no:cacheprovider"] + (extra or [os.path.join(ROOT, "tests")])
    if workers > 1:
        cmd += ["-n", str(workers)]
    return subprocess.call(cmd, cwd=ROOT, env=env)


def collect(tmp, gcov):
    """{file under csrc: ({line: executed}, {(line, branch): taken})} over every instantiation."""
    lines, branches = {}, {}
    for _, stem in UNITS:
        gcda = os.path.join(tmp, stem + ".gcda")
        if not os.path.exists(gcda):
            continue
        out = subprocess.check_output([gcov, "-b", "-c", "--json-format", "--stdout", "-o", tmp, gcda], cwd=tmp)
        for doc in out.decode().splitlines():
            if not doc.strip():
                continue
            for f in json.loads(doc)["files"]:
                path = os.path.realpath(os.path.join(tmp, f["file"]))
                if os.path.dirname(path) != os.path.realpath(CSRC):
                    continue
                ln, br = lines.setdefault(os.path.basename(path), {}), branches.setdefault(os.path.basename(path), {})
                for rec in f["lines"]:
                    n = rec["line_number"]
                    ln[n] = ln.get(n, False) or rec["count"] > 0
                    for i, b in enumerate(rec.get("branches", ())):
                        if b.get("throw"):
                            continue
                        br[(n, i)] = br.get((n, i), False) or b["count"] > 0
    return lines, branches


def ranges(ln):
    """Lines of `ln` whose value is false, runs joined across lines that are not in `ln`."""
    out, start, last = [], None, None
    for n in sorted(ln):
        if not ln[n]:
            if start is None:
                start = n
            last = n
        elif start is not None:
            out.append((start, last)); start = None
    if start is not None:
        out.append((start, last))
    return out


def report(lines, branches, suite_status):
    def share(hit, tot):
        return "%d/%d (%.1f %%)" % (hit, tot, 100.0 * hit / tot) if tot else "0/0"
    rows = ["# Kernel-source coverage of the emulated suite: pytest -m \"not gpu\" on a --coverage -O1 build of tests/emu (tools/emu_coverage.py)",
            "# suite exit status: %d" % suite_status, ""]
    for name in sorted(lines):
        ln, br = lines[name], branches[name]
        rows.append("%s: lines executed %s, branches taken %s" % (name, share(sum(ln.values()), len(ln)), share(sum(br.values()), len(br))))
        rs = ranges(ln)
        text = ", ".join("%d" % a if a == b else "%d-%d" % (a, b) for a, b in rs) if rs else "none"
        rows.append("  unexecuted: " + text)
        full = {}                                              # executed line -> every branch on it was taken
        for (n, _), taken in br.items():
            if ln.get(n):
                full[n] = full.get(n, True) and taken
        rs = ranges(full)
        rows.append("  executed, with an untaken branch: " + (", ".join("%d" % a if a == b else "%d-%d" % (a, b) for a, b in rs) if rs else "none"))
    return "\n".join(rows) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-o", "--output", help="write the report here (default: stdout)")
    ap.add_argument("-n", "--workers", type=int, default=min(os.cpu_count() or 1, 16), help="pytest-xdist workers (1: no xdist)")
    ap.add_argument("--cxx", default=os.environ.get("CXX", "g++"))
    ap.add_argument("--gcov", default=os.environ.get("GCOV", "gcov"))
    ap.add_argument("pytest_args", nargs="*", help="test files or directories to run instead of the whole of tests/ (a partial figure)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="wrsn_emu_cov_") as tmp:
        lib = build(tmp, a.cxx)
        status = run_suite(lib, a.workers, a.pytest_args)
        text = report(*collect(tmp, a.gcov), status)
    if a.output:
        with open(a.output, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    return status


if __name__ == "__main__":
    sys.exit(main())
