#!/usr/bin/env python3
"""One line per device kernel of the library: is its code the same as before?

    python tools/device_isa_report.py [--csrc DIR] [-j N] [-o FILE]
    python tools/device_isa_report.py --compare PARENT.txt BRANCH.txt

Compiles every file of the Makefile's SRCS with the Makefile's flags plus `--offload-device-only -S` (nothing is
linked or run), drops `.ident`, `.file` and comment lines, and prints for every kernel symbol
  * the SHA-256 (first 16 hex digits) of its normalised text,
  * .vgpr_count, .agpr_count, .sgpr_count, both spill counts, .private_segment_fixed_size, the static LDS size and
    whether the kernel also takes dynamic LDS (its size is a launch parameter, so only the fact is in the assembly),
  * its instruction count,
  * the SHA-256 of its mnemonic sequence (opcodes without operands) from the first to the last v_mfma*, and the
    number of instructions in that span ("-" for a kernel without matrix instructions).
A refactor that claims to leave device code alone runs it on both trees (--csrc points at the other checkout) and
compares: `identical` = same text hash; `equivalent` = same main-loop mnemonic hash, registers not higher, no
spills, no private segment, same LDS; anything else is `DIFFERENT`.  It hashes and counts; it looks for no
instruction other than the v_mfma prefix that delimits the loop.
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

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_CSRC = os.path.join(HERE, "..", "vae_tagger_amd", "csrc")
META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
             ".private_segment_fixed_size", ".group_segment_fixed_size")
COLUMNS = ("file", "kernel", "text", "vgpr", "agpr", "sgpr", "vspill", "sspill", "priv", "lds", "dynlds", "insts",
           "loop", "loop_insts")


def makefile_vars(csrc):
    """HIPCC, ARCH, CXXFLAGS and SRCS as the Makefile sets them (simple `NAME = value` / `NAME ?= value` lines)."""
    v = {}
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(r"^(\w+)\s*\??=\s*(.*)$", line.rstrip("\n"))
        if m:
            v[m.group(1)] = m.group(2)
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: v.get(m.group(1), ""), s)
    return os.environ.get("HIPCC", v["HIPCC"]), shlex.split(expand(v["CXXFLAGS"])), v["SRCS"].split()


def device_asm(csrc, hipcc, flags, src, extra):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "dev.s")
        subprocess.run([hipcc, *flags, *extra, "--offload-device-only", "-S", "-o", out, src], cwd=csrc, check=True)
        return open(out).read()


def strip_comment(line):
    i = line.find(";")
    return (line if i < 0 else line[:i]).rstrip()


def kernels_of(asm):
    """[(symbol, normalised body lines, metadata dict)] for every kernel of one device assembly file."""
    lines = asm.split("\n")
    records, cur = [], None
    for line in lines:                                 # the amdhsa.kernels list of the metadata note (YAML, one key per line)
        s = line.strip()
        if s.startswith("- .") or s.startswith("."):
            m = re.match(r"^(?:- )?(\.\w+):\s*(.*)$", s)
            if not m:
                continue
            k, val = m.group(1), m.group(2).strip().strip("'\"")
            if line.startswith("  - ."):               # a new kernel record begins
                cur = {}
                records.append(cur)
            if cur is not None:
                if k == ".value_kind":                 # the hidden argument the runtime fills when a kernel declares `extern __shared__`
                    cur["_dynlds"] = cur.get("_dynlds", False) or val == "hidden_dynamic_lds_size"
                else:
                    cur[k] = val
    by_symbol = {}
    for rec in records:
        if ".symbol" in rec:
            by_symbol[rec[".symbol"][:-3] if rec[".symbol"].endswith(".kd") else rec[".symbol"]] = rec
    out = []
    for name, rec in by_symbol.items():
        start = next((i for i, l in enumerate(lines) if l.startswith(name + ":")), None)
        if start is None:
            continue
        body = []
        for line in lines[start + 1:]:
            if line.startswith(".Lfunc_end"):
                break
            s = strip_comment(line).strip()
            if not s or s.startswith(".ident") or s.startswith(".file"):
                continue
            body.append(re.sub(r"\s+", " ", s))
        out.append((name, body, rec))
    return out


def is_instruction(s):
    return not (s.startswith(".") or s.endswith(":"))


def report_line(fname, name, body, rec, uses_dyn):
    insts = [s for s in body if is_instruction(s)]
    mn = [s.split(" ", 1)[0] for s in insts]
    idx = [i for i, m in enumerate(mn) if m.startswith("v_mfma")]
    if idx:
        span = mn[idx[0]:idx[-1] + 1]
        loop, loop_n = hashlib.sha256("\n".join(span).encode()).hexdigest()[:16], str(len(span))
    else:
        loop, loop_n = "-", "-"
    text = hashlib.sha256("\n".join(body).encode()).hexdigest()[:16]
    vals = [rec.get(k, "-") for k in META_KEYS]
    return "\t".join([fname, name, text, *vals, "yes" if uses_dyn else "no", str(len(insts)), loop, loop_n])


def one_file(args):
    csrc, hipcc, flags, src, extra = args
    asm = device_asm(csrc, hipcc, flags, src, extra)
    return sorted(report_line(src, name, body, rec, rec.get("_dynlds", False)) for name, body, rec in kernels_of(asm))


def build_report(csrc, jobs, extra):
    hipcc, flags, srcs = makefile_vars(csrc)
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        parts = list(ex.map(one_file, [(csrc, hipcc, flags, s, extra) for s in srcs]))
    return ["\t".join(COLUMNS)] + [l for p in parts for l in p]


def read_report(path):
    rows = {}
    for line in open(path):
        f = line.rstrip("\n").split("\t")
        if len(f) == len(COLUMNS) and f[0] != "file":
            rows[(f[0], f[1])] = dict(zip(COLUMNS, f))
    return rows


def classify(p, b):
    if p["text"] == b["text"]:
        return "identical"
    num = lambda r, k: int(r[k]) if r[k].isdigit() else 0
    ok = (p["loop"] == b["loop"] and num(b, "vgpr") <= num(p, "vgpr") and num(b, "agpr") <= num(p, "agpr")
          and all(num(b, k) == 0 for k in ("vspill", "sspill", "priv")) and p["lds"] == b["lds"] and p["dynlds"] == b["dynlds"])
    return "equivalent" if ok else "DIFFERENT"


def compare(parent, branch):
    P, B = read_report(parent), read_report(branch)
    lines, counts = [], {}
    for key in sorted(set(P) | set(B)):
        if key not in P or key not in B:
            cls, detail = ("ADDED" if key in B else "REMOVED"), ""
        else:
            p, b = P[key], B[key]
            cls = classify(p, b)
            detail = "" if cls == "identical" else "\t" + " ".join(
                f"{k}:{p[k]}->{b[k]}" for k in COLUMNS[2:] if p[k] != b[k]) + f" insts_diff:{int(b['insts']) - int(p['insts']):+d}"
        counts[cls] = counts.get(cls, 0) + 1
        if cls != "identical":
            lines.append(f"{cls}\t{key[0]}\t{key[1]}{detail}")
    lines.append("# " + ", ".join(f"{n} {c}" for c, n in sorted(counts.items())))
    return lines, all(c in ("identical", "equivalent") for c in counts)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=DEFAULT_CSRC, help="directory with the Makefile and the .hip files")
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("-o", default=None, help="write the report here instead of stdout")
    ap.add_argument("--define", action="append", default=[], help="extra compiler flag, e.g. --define=-DHALO_STAMP")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "BRANCH"))
    a = ap.parse_args()
    if a.compare:
        lines, ok = compare(*a.compare)
        print("\n".join(lines))
        return 0 if ok else 1
    lines = build_report(os.path.abspath(a.csrc), a.j, a.define)
    text = "\n".join(lines) + "\n"
    if a.o:
        open(a.o, "w").write(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
