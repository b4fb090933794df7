#!/usr/bin/env python3
"""Which compiled kernels does the GPU suite launch?

  kernel_coverage.py symbols LIB [--demangle]
      the kernel symbols (mangled, without .kd) of every gfx950 code object in LIB's .hip_fatbin, one per line

  kernel_coverage.py text LIB
      "<sha1 of the kernel's instruction text> <symbol>" per kernel: diff two builds to show which kernels a change touched

  kernel_coverage.py merge LIB DIR... [--manifest OUT --column parent|head] [--json OUT]
      DIR holds one sub-directory per traced run (named after the test file, "<file>" or "<file>.<part>" for a file traced
      in several parts), each with the *_kernel_stats.csv files rocprofv3 wrote for the process and its children:

          rocprofv3 --kernel-trace --stats -M --output-format csv -d DIR/<file> -- python -m pytest tests/<file>.py -q -m gpu

      (-M: mangled, untruncated names, so that a traced name equals a symbol).  Prints, for every symbol, the test files
      that launched it and how often; with --manifest, (re)writes that column of tests/kernel_coverage.txt.  With
      --part NAME instead, writes tests/kernel_coverage.d/NAME.txt from a traced run of the new test files alone: the rows
      of the kernels the manifest does not list yet and the code letters of the test files it does not name, and nothing
      else ("# sole-cover" lines added to a part by hand are read with the manifest's and kept when the part is rewritten) -- how a change that adds kernels records them while every existing row stays as the last full trace wrote
      it.  read_manifest() reads the manifest and every part; the next full re-trace (--manifest) takes the parts' rows
      and letters into the manifest and removes the part files.

The library's own kernels live in namespace ac (_ZN2ac..., or an anonymous namespace inside it); a traced name of that form
that matches no symbol is an error.  Kernels of torch, rocBLAS, RCCL ... are ignored.
"""

import argparse
import csv
import glob
import json
import os
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANIFEST = os.path.join(ROOT, "tests", "kernel_coverage.txt")
PARTS = os.path.join(ROOT, "tests", "kernel_coverage.d")      # additions to the manifest, one file per change (--part)


def code_objects(lib):
    """The device ELFs of every offload bundle in LIB's .hip_fatbin: [(target triple, bytes)]."""
    with tempfile.TemporaryDirectory() as tmp:
        raw = os.path.join(tmp, "fatbin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + raw, lib, os.path.join(tmp, "copy")],
                       check=True)
        data = open(raw, "rb").read()
    assert b"CCOB" != data[:4], "compressed offload bundles are not handled: build without --offload-compress"
    out, at = [], data.find(BUNDLE_MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", data, at + len(BUNDLE_MAGIC))
        p = at + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if size and triple.startswith("hip"):
                elf = data[at + off:at + off + size]
                assert elf[:4] == b"\x7fELF", (triple, at, off)
                out.append((triple, elf))
        at = data.find(BUNDLE_MAGIC, p)
    return out


def kernel_symbols(lib):
    """Mangled names of the kernels (the symbols ending in .kd, without that suffix), sorted; unique across code objects."""
    names = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, (_, elf) in enumerate(code_objects(lib)):
            f = os.path.join(tmp, "co%d.elf" % i)
            open(f, "wb").write(elf)
            r = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-s", "--wide", f], check=True, capture_output=True, text=True)
            mine = set()   # (-s lists .dynsym and .symtab: a kernel appears in both)
            for ln in r.stdout.splitlines():
                w = ln.split()
                if len(w) >= 8 and w[-1].endswith(".kd") and w[3] == "OBJECT":
                    mine.add(w[-1][:-3])
            names.extend(mine)
    dup = sorted(set(n for n in names if names.count(n) > 1)) if len(set(names)) != len(names) else []
    assert not dup, "kernel symbols defined in more than one code object: %s" % dup[:10]
    return sorted(names)


def demangle(names):
    """For display.  llvm-cxxfilt where the toolchain ships it; binutils' c++filt leaves the _Float16 / __bf16 instances
    (DF16_ / DF16b) mangled."""
    import shutil
    tool = next((t for t in (os.path.join(LLVM, "llvm-cxxfilt"), shutil.which("llvm-cxxfilt"), shutil.which("c++filt"))
                 if t and os.path.exists(t)), None)
    assert tool, "no llvm-cxxfilt / c++filt on this machine"
    r = subprocess.run([tool], input="\n".join(names) + "\n", check=True, capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert len(out) == len(names)
    return out


def kernel_text(lib):
    """{symbol: sha1 of its disassembled instruction text} -- two builds whose tables agree emit the same code per kernel."""
    import hashlib
    import re
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, (_, elf) in enumerate(code_objects(lib)):
            f = os.path.join(tmp, "co%d.elf" % i)
            open(f, "wb").write(elf)
            r = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", f],
                               check=True, capture_output=True, text=True)
            cur, buf = None, []
            for ln in r.stdout.splitlines() + ["<end>:"]:
                m = re.match(r"^[0-9a-f]* ?<(.+)>:$", ln.strip())
                if m and not re.match(r"L\d+$", m.group(1)):
                    if cur:
                        out[cur] = hashlib.sha1("\n".join(buf).encode()).hexdigest()
                    cur, buf = m.group(1), []
                elif cur:
                    buf.append(re.sub(r"\s*//.*", "", ln))
    kernels = set(kernel_symbols(lib))
    assert kernels <= set(out), sorted(kernels - set(out))[:5]
    return {k: v for k, v in out.items() if k in kernels}


def is_ours(name):
    return name.startswith("_ZN2ac") or name.startswith("ac::") or " ac::" in name


def read_stats(run_dir):
    """{kernel name (no .kd): calls} summed over every *kernel_stats.csv below run_dir (the process and its children)."""
    calls = {}
    files = glob.glob(os.path.join(run_dir, "**", "*kernel_stats.csv"), recursive=True)
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Name"]
                if name.endswith(".kd"):
                    name = name[:-3]
                calls[name] = calls.get(name, 0) + int(row["Calls"])
    return calls, len(files)


def merge(lib, dirs):
    """{symbol: {test file: calls}} over the traced runs below dirs; raises on a kernel of ours that is no symbol."""
    syms = kernel_symbols(lib)
    known = set(syms)
    by_demangled = None
    cover = {s: {} for s in syms}
    unknown = {}
    for top in dirs:
        for run in sorted(os.listdir(top)):
            run_dir = os.path.join(top, run)
            if not os.path.isdir(run_dir):
                continue
            test_file = run.split(".")[0]
            calls, nfiles = read_stats(run_dir)
            assert nfiles, "no *kernel_stats.csv under %s: the traced run left nothing" % run_dir
            for name, n in calls.items():
                if name not in known and not name.startswith("_Z") and is_ours(name):
                    # a trace taken without -M: demangle our side with the same tool and match on that
                    if by_demangled is None:
                        by_demangled = dict(zip(demangle(syms), syms))
                    name = by_demangled.get(name, name)
                if name in known:
                    cover[name][test_file] = cover[name].get(test_file, 0) + n
                elif is_ours(name):
                    unknown.setdefault(name, []).append(run)
    assert not unknown, "traced kernels of namespace ac that are no symbol of %s:\n  %s" % (
        lib, "\n  ".join("%s  (%s)" % (k, ",".join(v)) for k, v in sorted(unknown.items())))
    return cover


# ---- the manifest: tests/kernel_coverage.txt
def part_files():
    return sorted(glob.glob(os.path.join(PARTS, "*.txt")))


def read_manifest(path=MANIFEST, parts=True, skip=None):
    """(header lines, codes {code: test file}, rows {symbol: (parent codes, head codes)}) of the manifest and, for the
    manifest of the tree, of every part under tests/kernel_coverage.d (but ``skip``).  A part may only add: a code letter
    or a kernel named twice is an error.  Of a part's comment lines only its code letters and its "# sole-cover <kernel>
    <file>::<test>" lines (added by hand, for a new family only one test reaches) join the header."""
    header, codes, rows = [], {}, {}
    files = [path]
    if parts and os.path.abspath(path) == os.path.abspath(MANIFEST):
        files += [f for f in part_files() if skip is None or os.path.abspath(f) != os.path.abspath(skip)]
    for f in files:
        for ln in open(f).read().splitlines():
            if ln.startswith("#"):
                w = ln[1:].split()
                code = len(w) == 3 and w[0] == "code"
                if code:
                    assert w[1] not in codes, "%s: code %s is defined twice" % (f, w[1])
                    codes[w[1]] = w[2]
                if code or f == path or (len(w) == 3 and w[0] == "sole-cover"):
                    header.append(ln)
            elif ln.strip():
                w = ln.split()
                assert len(w) == 3, ln
                assert w[0] not in rows, "%s: kernel %s is listed twice" % (f, w[0])
                rows[w[0]] = (w[1], w[2])
    return header, codes, rows


def next_code(codes):
    return next(c for c in "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz" if c not in codes)


def write_part(cover, name):
    """tests/kernel_coverage.d/NAME.txt: the kernels of cover that the manifest (and the other parts) do not list, with the
    test files of cover that launched them; test files without a code letter get the next free one."""
    out = os.path.join(PARTS, name + ".txt")
    _, codes, rows = read_manifest(skip=out)
    by_file = {v: k for k, v in codes.items()}
    new = sorted(s for s in cover if s not in rows)
    header = ["# Addition to tests/kernel_coverage.txt, in its format (tools/kernel_coverage.py merge LIB DIR --part %s):" % name,
              "# the kernels that manifest does not list, from a traced run of the test files below.  The next full re-trace",
              "# (merge --manifest) moves these rows and code letters into the manifest and removes this file."]
    for f in sorted(set(f for s in new for f in cover[s])):
        if f not in by_file:
            code = next_code(codes)
            codes[code], by_file[f] = f, code
            header.append("# code %s %s" % (code, f))
    if os.path.exists(out):      # the sole covers named by hand survive a rewrite of the part
        header += [ln for ln in open(out).read().splitlines() if ln.startswith("# sole-cover ")]
    os.makedirs(PARTS, exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(header) + "\n")
        for s in new:
            fh.write("%s - %s\n" % (s, "".join(sorted(by_file[f] for f in cover[s])) or "-"))


def write_column(cover, column, path=MANIFEST):
    """(Re)writes one column of the manifest from a trace of the whole suite.  The parts are read with it, so their code
    letters and first columns carry over, and are removed once the manifest holds their rows: one source again."""
    header, codes, rows = read_manifest(path) if os.path.exists(path) else ([], {}, {})
    by_file = {v: k for k, v in codes.items()}
    files = sorted(set(f for c in cover.values() for f in c))
    for f in files:
        if f not in by_file:
            code = next_code(codes)
            codes[code], by_file[f] = f, code
            header.append("# code %s %s" % (code, f))
    out = {}
    for s, c in cover.items():
        mine = "".join(sorted(by_file[f] for f in c)) or "-"
        old = rows.get(s, ("-", "-"))
        out[s] = (mine, old[1]) if column == "parent" else (old[0], mine)
    with open(path, "w") as fh:
        fh.write("\n".join(header) + "\n")
        for s in sorted(out):
            fh.write("%s %s %s\n" % (s, out[s][0], out[s][1]))
    if os.path.abspath(path) == os.path.abspath(MANIFEST):
        for f in part_files():
            os.remove(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("symbols")
    a.add_argument("lib")
    a.add_argument("--demangle", action="store_true")
    c = sub.add_parser("text")
    c.add_argument("lib")
    b = sub.add_parser("merge")
    b.add_argument("lib")
    b.add_argument("dirs", nargs="+")
    b.add_argument("--manifest", help="write this column of the manifest (default tests/kernel_coverage.txt)", nargs="?", const=MANIFEST)
    b.add_argument("--column", choices=("parent", "head"), default="head")
    b.add_argument("--part", help="write tests/kernel_coverage.d/PART.txt (kernels the manifest does not list) instead")
    b.add_argument("--json", help="the full table {symbol: {test file: calls}}")
    b.add_argument("--demangle", action="store_true")
    args = ap.parse_args()
    if args.cmd == "symbols":
        syms = kernel_symbols(args.lib)
        for s in (demangle(syms) if args.demangle else syms):
            print(s)
        print("%d kernels in %d code objects" % (len(syms), len(code_objects(args.lib))), file=sys.stderr)
        return
    if args.cmd == "text":
        for k, v in sorted(kernel_text(args.lib).items()):
            print(v, k)
        return
    cover = merge(args.lib, args.dirs)
    shown = dict(zip(cover, demangle(list(cover)))) if args.demangle else {s: s for s in cover}
    for s in sorted(cover):
        print("%s\t%s" % (shown[s], " ".join("%s:%d" % kv for kv in sorted(cover[s].items())) or "-"))
    never = [s for s in cover if not cover[s]]
    print("%d of %d kernels launched, %d never" % (len(cover) - len(never), len(cover), len(never)), file=sys.stderr)
    if args.json:
        json.dump(cover, open(args.json, "w"), indent=0, sort_keys=True)
    if args.part:
        write_part(cover, args.part)
    elif args.manifest:
        write_column(cover, args.column, args.manifest)


if __name__ == "__main__":
    main()
