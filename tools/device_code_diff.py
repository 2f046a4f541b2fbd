"""Is the device code of two source trees the same? Per device function of the named translation units: instruction lines, VGPRs,
AGPRs, SGPRs, scratch and static LDS bytes on both sides, and whether the code and the kernel descriptor are equal.
    python tools/device_code_diff.py <parent tree> <new tree> <unit>[=<parent's unit>] ... [--keep DIR]
e.g. python tools/device_code_diff.py ../parent . lorahip_wide lorahip_fma_wide lorahip_stream_wide=lorahip_wide
Each unit is compiled in <tree>/lora_sdr_amd/csrc with the library's flags (build.FLAGS) plus --cuda-device-only -S. A function is the
text from its `_Z...:` label to `.Lfunc_end<n>:`, comments (`;` to the end of the line) and empty lines dropped, every mangled name
inside a body replaced by one token and the function's ordinal taken out of its block labels (`.LBB<ordinal>_<block>`: it changes
when another function enters or leaves the unit); the `.amdhsa_kernel ... .end_amdhsa_kernel` block is taken out of the body and compared by
itself; the register, scratch and LDS figures are the compiler's `; Kernel info:` comments after the function. "instr" counts the
lines of a body that are neither directives nor labels. Functions are matched by mangled name (a function that only one side has is
listed as such: expected where a unit of the new tree holds part of a parent's). Two texts are compared, nothing else: the script
knows no instruction. --keep DIR leaves the assembly there (DIR/parent, DIR/new); with --reuse the assembly already there is compared
and nothing compiled (how the script itself is checked: alter a line of a copy). Exit status 1 if anything differs."""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lora_sdr_amd.build import FLAGS

MANGLED = re.compile(r"_Z[A-Za-z0-9_.$]+")
LOCAL = re.compile(r"\.LBB\d+_")                            # a block label carries the function's ordinal in its unit: not code
INFO = {"vgpr": r"; NumVgprs: (\d+)", "agpr": r"; NumAgprs: (\d+)", "sgpr": r"; TotalNumSgprs: (\d+)", "scratch": r"; ScratchSize: (\d+)", "lds": r"; LDSByteSize: (\d+)"}


def compile_unit(tree, unit, out):
    csrc = os.path.join(os.path.abspath(tree), "lora_sdr_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + ["--cuda-device-only", "-S", unit + ".hip", "-o", out]
    return subprocess.Popen(cmd, cwd=csrc)


def functions(path):
    """{mangled name: (body lines, descriptor lines, figures)} of one assembly file, in file order"""
    fns, name, body, desc, in_desc = {}, None, [], [], False
    lines = open(path).read().split("\n")
    for i, raw in enumerate(lines):
        line = raw.split(";")[0].rstrip()
        m = re.match(r"(_Z[A-Za-z0-9_.$]+):", line)
        if m or name is None:                               # (a `_Z` label without an end is a variable: dropped when the next one starts)
            if m:
                name, body, desc, in_desc = m.group(1), [], [], False
            continue
        if line.startswith(".Lfunc_end"):
            tail = "\n".join(lines[i:i + 80])
            tail = tail[:tail.find("\n_Z")] if "\n_Z" in tail else tail
            figs = {k: int(re.search(p, tail).group(1)) if re.search(p, tail) else 0 for k, p in INFO.items()}
            fns[name], name = (body, desc, figs), None
            continue
        if not line.strip():
            continue
        line = LOCAL.sub(".LBB_", MANGLED.sub("<sym>", line))
        if line.strip().startswith(".amdhsa_kernel"):
            in_desc = True
        (desc if in_desc else body).append(line)
        if line.strip().startswith(".end_amdhsa_kernel"):
            in_desc = False
    return fns


def row(tag, f):
    instr = sum(1 for l in f[0] if not l.strip().startswith(".") and not l.strip().endswith(":"))
    return "     %-6s %6d instr  %3d VGPR  %3d AGPR  %3d SGPR  %4d B scratch  %5d B LDS" % (tag, instr, f[2]["vgpr"], f[2]["agpr"], f[2]["sgpr"], f[2]["scratch"], f[2]["lds"])


def main(argv):
    reuse, keep, args = "--reuse" in argv, None, [a for a in argv if a != "--reuse"]
    if "--keep" in args:                                    # (by position: DIR may equal one of the trees)
        i = args.index("--keep")
        keep, args = args[i + 1], args[:i] + args[i + 2:]
    parent, new, units = args[0], args[1], [(u.split("=") + [u])[:2] for u in args[2:]]
    work = keep or tempfile.mkdtemp(prefix="device_code_diff_")
    jobs = []
    for side, tree, col in (("parent", parent, 1), ("new", new, 0)):
        os.makedirs(os.path.join(work, side), exist_ok=True)
        for u in sorted(set(p[col] for p in units)):
            if not reuse:
                jobs.append((side + "/" + u, compile_unit(tree, u, os.path.join(work, side, u + ".s"))))
    bad = [n for n, p in jobs if p.wait() != 0]
    if bad:
        raise SystemExit("hipcc failed: " + ", ".join(bad))
    n_code = n_desc = n_fn = n_single = 0
    seen = {}
    for nu, pu in units:
        fp, fn = functions(os.path.join(work, "parent", pu + ".s")), functions(os.path.join(work, "new", nu + ".s"))
        print("== %s.hip%s: %d device functions (parent), %d (new)" % (nu, "" if pu == nu else " (parent: %s.hip)" % pu, len(fp), len(fn)))
        for name in fn:
            print("   " + name)
            if name not in fp:
                n_single += 1
                print(row("new", fn[name]) + "   ONLY IN THE NEW TREE")
                continue
            code, desc = fp[name][0] == fn[name][0], fp[name][1] == fn[name][1]
            n_fn, n_code, n_desc = n_fn + 1, n_code + (not code), n_desc + (not desc)
            print(row("parent", fp[name]))
            print(row("new", fn[name]) + "   code %s, descriptor %s" % ("IDENTICAL" if code else "DIFFERENT", "IDENTICAL" if desc else "DIFFERENT"))
        seen.setdefault(pu, set()).update(fn)
    for pu in seen:                                         # (a parent's unit may be several of the new tree's)
        for name in functions(os.path.join(work, "parent", pu + ".s")):
            if name not in seen[pu]:
                n_single += 1
                print("== ONLY IN THE PARENT'S %s.hip: %s" % (pu, name))
    print("== %d functions compared: %d code differences, %d descriptor differences; %d functions on one side only" % (n_fn, n_code, n_desc, n_single))
    return 1 if (n_code or n_desc or n_single) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
