#!/usr/bin/env python3
"""Are the live path's kernels the kernels they were?

    hipcc <COMMON> <LIVEFLAGS> --cuda-device-only -S pekf_live.hip -o new.s      (this tree)
    the same on the previous commit's pekf_live.hip                 -o old.s
    live_listing_diff.py old.s new.s

and the same for pekf_live_traj.hip (the TRAJ = true kernels) and pekf_frontend.hip (k_frontend, k_frontend_init;
the Makefile's flags for that file: COMMON alone).  Each kernel template instantiation over bools of namespace
pekf -- k_live<TE, R64, EV64, TRAJ>, k_frontend<TE, EV64>, k_frontend_init<EV64> -- of old.s is compared with
that of new.s: instructions and block labels, comments and assembler directives dropped, the kernel's own name
and its number in the .LBB labels normalised.  Prints a line per kernel (lines, identical or the unified diff)
and exits 1 on any difference, or on a kernel that only one of the listings has."""
import difflib
import re
import sys

NAME = re.compile(r"^(_ZN4pekf\d+(k_[a-z_]+)I((?:Lb\dE)+)E\w*):\s*(;.*)?$")


def kernels(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = NAME.match(line)
        if m:
            name, cur = m.group(1), []
            out["%s<%s>" % (m.group(2), ", ".join(re.findall(r"Lb(\d)E", m.group(3))))] = cur
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        text = line.split(";", 1)[0].rstrip()
        if not text.strip() or (text.lstrip().startswith(".") and not text.startswith(".LBB")):
            continue  # (the kernel descriptor's .amdhsa_* lines too: its kernarg size grows with the arguments)
        text = text.replace(name, "KERNEL")
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", text))
    return out


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    bad = 0
    for label in sorted(set(old) | set(new)):
        if label not in old or label not in new:
            print("%s: not in %s" % (label, new_path if label in old else old_path))
            bad += 1
            continue
        d = list(difflib.unified_diff(old[label], new[label], "old", "new", lineterm="", n=2))
        print("%s: %d lines before, %d after, %s" % (label, len(old[label]), len(new[label]),
                                                     "identical" if not d else "DIFFERENT"))
        if d:
            bad += 1
            print("\n".join(d[:200]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
