#!/usr/bin/env python
"""A fold library for `dmpfold --search` / `dmpfold-batch --library` from a directory of PDB files.

    python tools/make_library.py DIR OUT.npz

Every *.pdb of DIR (first chain, C-alpha atoms; score.read_native_ca) becomes one entry named by its stem, in sorted
order; OUT.npz holds the arrays names, lengths and ca (score.Library.save).  An entry with fewer than 3 C-alpha atoms or
more than the build's maximum length is an error that names it.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dmpfold2_amd.score import Library          # noqa: E402  (no GPU needed)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2:
        print(__doc__, file=sys.stderr)
        return 2
    lib = Library.from_dir(argv[0])
    lib.check(2048)                             # DMP_MAX_L
    lib.save(argv[1])
    print(f"{argv[1]}: {len(lib)} entries, {lib.rows} rows, longest {lib.max_m}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
