"""Do two builds carry the same gfx950 machine code?  (CPU only.)

    python tools/kernel_diff.py A B

A and B are built libraries or single .o files; both carry the offload bundle that _lib.kernel_code_table reads ({mangled name:
(size, SHA-256)} of every kernel).  Prints how many kernels only A has, only B has and how many common ones differ, with their
names, and exits 1 if any common kernel differs or is ambiguous (a name that more than one code object of a build defines) --
which is how a refactor of a kernel is held to "nothing changed" (DESIGN.md 4.1): build the parent commit out of tree with the
same compiler and flags, then
    python tools/kernel_diff.py parent/libdeep3d_planesweep.so deep3d_aerial_amd/csrc/libdeep3d_planesweep.so"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def diff_tables(a, b):
    """(only_a, only_b, differing): sorted names of the kernels that only table a has, that only table b has, and that both have
    with entries that are not equal -- or that are ambiguous (None) on either side, where equality says nothing."""
    only_a = sorted(set(a) - set(b))
    only_b = sorted(set(b) - set(a))
    differing = sorted(n for n in set(a) & set(b) if a[n] is None or b[n] is None or a[n] != b[n])
    return only_a, only_b, differing


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    sys.path.insert(0, ROOT)
    from deep3d_aerial_amd import _lib

    a, b = _lib.kernel_code_table(argv[1]), _lib.kernel_code_table(argv[2])
    only_a, only_b, differing = diff_tables(a, b)
    print("kernels: %d / %d, only in A: %d, only in B: %d, differing: %d of %d common"
          % (len(a), len(b), len(only_a), len(only_b), len(differing), len(set(a) & set(b))))
    for title, names in (("only in A", only_a), ("only in B", only_b), ("differing", differing)):
        for n in names:
            print("%s: %s" % (title, n))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
