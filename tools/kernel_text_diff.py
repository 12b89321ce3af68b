#!/usr/bin/env python3
"""tools/kernel_text_diff.py <old.s> <new.s> -- do two builds hold the SAME KERNELS?  For the device assembly that `hipcc -save-temps=obj`
leaves (fpx_search-hip-amdgcn-amd-amdhsa-gfx950.s): each file is split into kernels at `_Z...:` ... `.Lfunc_end`, comments go, the
compiler's local labels (.LBB<n>_, .Ltmp<n>, ...) are renumbered in order of appearance, and the texts are compared.  Reports whether the
names are the same set, which bodies differ and whether the order differs; exits 1 on a differing name set or body (a kernel's code is
aligned on its own: the order is reported, not judged)."""
import re
import sys


def kernels(text):
    """{name: normalised body}, in the file's order."""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        seen = {}
        lines = [re.sub(r";.*", "", ln).strip() for ln in m.group(2).splitlines()]
        body = "\n".join(ln for ln in lines if ln)
        out[m.group(1)] = re.sub(r"\.L([A-Za-z_]*[A-Za-z])(\d+)", lambda l: ".L%s#%d" % (l.group(1), seen.setdefault(l.group(0), len(seen))), body)
    return out


def main(old_path, new_path):
    old, new = kernels(open(old_path).read()), kernels(open(new_path).read())
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(k for k in old if k in new and old[k] != new[k])
    print("kernels: %d old, %d new; names %s" % (len(old), len(new), "the same set" if not only_old and not only_new else "DIFFER"))
    for k in only_old: print("  only in old: " + k)
    for k in only_new: print("  only in new: " + k)
    print("bodies that differ: %d" % len(differ))
    for k in differ: print("  differs: " + k)
    print("order: %s" % ("the same" if list(old) == list(new) else "differs"))
    return 1 if only_old or only_new or differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3: sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
