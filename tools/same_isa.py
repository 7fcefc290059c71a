"""Do two kernels disassemble to the same instructions?  For a change that turns a kernel into one instantiation of a template
and promises that the old launch runs what it ran.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC [the file's flags of dmpfold2_amd/build.py] --cuda-device-only -S old/x.hip -o old.s
    hipcc ... -S new/x.hip -o new.s
    python tools/same_isa.py old.s new.s OLD_NAME NEW_NAME

OLD_NAME and NEW_NAME are substrings of the kernels' mangled names, each matching exactly one kernel of its file (for the
report on the alignment: `16msa_count_kernelEPKj` against `msa_count_kernelILb0E` of msa.hip, `22mapscore_select_kernelENS`
against `mapscore_select_kernelINS_12MsByDistance` of mapscore.hip).  Compared are the instructions in order, without comments
and directives and with the numbering of the basic-block labels taken out (it counts the functions of the file); the sizes
of the kernel arguments are printed beside them.  Exit status 0 when they are the same.
"""
import difflib
import re
import sys


def kernels(path):
    """{mangled name: [instruction, ...]} and {mangled name: kernarg bytes} of an assembly file."""
    code, args, cur, name = {}, {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            code[cur] = []
            continue
        m = re.match(r"\s*\.kernarg_segment_size:\s*(\d+)", line)
        if m:
            size = int(m.group(1))
        m = re.match(r"\s*\.name:\s*(_Z\w+)", line)
        if m:
            args[m.group(1)] = size
        if cur is not None:
            if line.startswith(".Lfunc_end") or line.strip().startswith(".section"):
                cur = None
                continue
            text = line.split(";")[0].strip()
            if text and not text.startswith("."):
                code[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", text))
    return code, args


def one(code, part, path):
    found = [k for k in code if part in k]
    if len(found) != 1:
        sys.exit(f"{path}: {len(found)} kernels match {part!r}: {found}")
    return found[0]


def main():
    if len(sys.argv) != 5:
        sys.exit(__doc__)
    old, new, old_part, new_part = sys.argv[1:]
    (a, a_args), (b, b_args) = kernels(old), kernels(new)
    ka, kb = one(a, old_part, old), one(b, new_part, new)
    same = a[ka] == b[kb]
    print(f"{ka}: {len(a[ka])} instructions, {a_args.get(ka)} bytes of arguments")
    print(f"{kb}: {len(b[kb])} instructions, {b_args.get(kb)} bytes of arguments")
    print("the same instructions" if same else "DIFFERENT")
    if not same:
        print("\n".join(list(difflib.unified_diff(a[ka], b[kb], lineterm="", n=1))[:60]))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
