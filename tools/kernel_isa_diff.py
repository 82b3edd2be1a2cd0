"""Compare the gfx950 instruction streams of every kernel in two trees (no GPU needed).

    python tools/kernel_isa_diff.py OLD_TREE [NEW_TREE] [--jobs N] > profiles/NAME.txt

Each csrc/*.hip of both trees is compiled with its Makefile's HIPFLAGS plus
`--cuda-device-only -S`; the assembly is split per kernel, comments and directives are
dropped, local label numbers (.LBB<n>_) get one spelling, and the streams are compared by
demangled kernel name (parameter list dropped) after the renames in RENAMES. It reports the
kernels present in one tree only, the kernels that differ (with a unified diff of their
streams) and the counts. It only compares streams; exit status 1 when any common kernel differs.
"""
import concurrent.futures
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

CXXFILT = shutil.which("llvm-cxxfilt") or "c++filt"
# old name -> new name, for kernels whose dead template parameters were removed
RENAMES = [(r"gemm_pp_kernel<0, (\d+), false, false>", r"gemm_pp_kernel<\1>"),
           (r"lstm_fwd_persistent_kernel<(\d+), (true|false), 0>", r"lstm_fwd_persistent_kernel<\1, \2>"),
           (r"conv3x3_wgrad_rows_kernel<0>", r"conv3x3_wgrad_rows_kernel")]


def make_vars(tree):
    """HIPCC and the expanded HIPFLAGS of the tree's Makefile."""
    v = dict(re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", open(os.path.join(tree, "Makefile")).read(), re.M))
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: expand(v.get(m.group(1), "")), s)  # noqa: E731
    return expand(v["HIPCC"]), expand(v["HIPFLAGS"]).split(), expand(v["CSRC"])


def base_name(demangled):
    """`void ns::(anonymous namespace)::k<1, 2>(args)` -> `ns::k<1, 2>`."""
    s = demangled.replace("(anonymous namespace)::", "")
    depth = 0
    for i in range(len(s) - 1, -1, -1):                   # the parameter list: the last top-level (...)
        depth += (s[i] == ")") - (s[i] == "(")
        if depth == 0 and s[i] == "(":
            s = s[:i]
            break
    return s[5:] if s.startswith("void ") else s


def kernels(tree, out_dir, jobs):
    """{(file, name): [instruction lines]} of every kernel in tree/csrc/*.hip."""
    hipcc, flags, csrc = make_vars(tree)
    srcs = sorted(glob.glob(os.path.join(tree, csrc, "*.hip")))

    def compile_one(src):
        asm = os.path.join(out_dir, os.path.basename(src)[:-4] + ".s")
        subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", os.path.relpath(src, tree), "-o", asm],
                       cwd=tree, check=True, stderr=subprocess.DEVNULL)
        return asm

    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        asms = list(pool.map(compile_one, srcs))
    found = {}
    for asm in asms:
        text = open(asm).read()
        syms = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
        names = subprocess.run([CXXFILT], input="\n".join(syms), capture_output=True, text=True,
                               check=True).stdout.split("\n")
        for sym, name in zip(syms, names):
            body = text.split("\n" + sym + ":", 1)[1].split(".Lfunc_end", 1)[0]
            lines = []
            for ln in body.split("\n"):
                ln = ln.split(";", 1)[0].strip()
                if ln and (not ln.startswith(".") or ln.endswith(":")):     # directives go, labels stay
                    lines.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
            found[(os.path.basename(asm)[:-2], base_name(name))] = lines
    return found


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else 8
    if "--jobs" in sys.argv:
        args.remove(str(jobs))
    old_tree = os.path.abspath(args[0])
    new_tree = os.path.abspath(args[1] if len(args) > 1 else os.path.join(os.path.dirname(__file__), ".."))
    with tempfile.TemporaryDirectory() as d_old, tempfile.TemporaryDirectory() as d_new:
        old, new = kernels(old_tree, d_old, jobs), kernels(new_tree, d_new, jobs)
    renamed = {}
    for (f, name), lines in old.items():
        for pat, to in RENAMES:
            name = re.sub(pat, to, name)
        renamed[(f, name)] = lines
    both = sorted(set(renamed) & set(new))
    differ = [k for k in both if renamed[k] != new[k]]
    print(f"kernels: old {len(old)}, new {len(new)}, in both {len(both)}, identical {len(both) - len(differ)}, "
          f"different {len(differ)}")
    for title, keys in (("only in the old tree", sorted(set(renamed) - set(new))),
                        ("only in the new tree", sorted(set(new) - set(renamed)))):
        print(f"\n{title}: {len(keys)}")
        for f, name in keys:
            print(f"  {f}: {name}")
    print(f"\ndifferent: {len(differ)}")
    for k in differ:
        print(f"  {k[0]}: {k[1]} ({len(renamed[k])} -> {len(new[k])} instructions and labels)")
        for ln in list(difflib.unified_diff(renamed[k], new[k], "old", "new", n=0, lineterm=""))[2:]:
            print("      " + ln)
    print("\nidentical:")
    for f, name in both:
        if (f, name) not in differ:
            print(f"  {f}: {name} ({len(new[(f, name)])})")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
