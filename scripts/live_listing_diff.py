#!/usr/bin/env python3
"""Are k_live's instantiations without trajectory output the kernels they were?

    hipcc <COMMON> <LIVEFLAGS> --cuda-device-only -S pekf_live.hip -o new.s      (this tree)
    the same on the previous commit's pekf_live.hip                 -o old.s
    live_listing_diff.py old.s new.s

Each k_live<TE, R64, EV64[, TRAJ = false]> body -- instructions and block labels, comments and assembler
directives dropped, the kernel's own name and its number in the .LBB labels normalised -- of old.s is compared
with that of new.s.  Prints a line per kernel (lines, identical or the unified diff) and exits 1 on any
difference.  Kernels with TRAJ = true are listed with their length only."""
import difflib
import re
import sys

NAME = re.compile(r"^(_ZN4pekf6k_liveILb(\d)ELb(\d)ELb(\d)E(?:Lb(\d)E)?E\w*):\s*(;.*)?$")


def kernels(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = NAME.match(line)
        if m:
            name, cur = m.group(1), []
            out[tuple(int(v or 0) for v in m.group(2, 3, 4, 5))] = cur
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
    for key in sorted(new):
        te, r64, ev64, traj = key
        label = "k_live<TE=%d, R64=%d, EV64=%d, TRAJ=%d>" % key
        if traj:
            print("%s: %d lines (new)" % (label, len(new[key])))
            continue
        if key not in old:
            print("%s: not in %s" % (label, old_path))
            bad += 1
            continue
        d = list(difflib.unified_diff(old[key], new[key], "old", "new", lineterm="", n=2))
        print("%s: %d lines before, %d after, %s" % (label, len(old[key]), len(new[key]),
                                                     "identical" if not d else "DIFFERENT"))
        if d:
            bad += 1
            print("\n".join(d[:200]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
