#!/usr/bin/env python3
"""Are the kernels the kernels they were?

    hipcc <COMMON> <the file's flags> --cuda-device-only -S FILE.hip -o new.s      (this tree)
    the same on the previous commit's FILE.hip                          -o old.s
    live_listing_diff.py old.s new.s

with the Makefile's flags for each file.  It began as the gate of the live path (hence the name): pekf_live.hip
and pekf_live_traj.hip (LIVEFLAGS) and pekf_frontend.hip (COMMON alone).  A change to the shared device math
(pekf_math.hpp, pekf_step.hpp) is checked over every file that includes it: those three, pekf_run.hip (RUNFLAGS),
pekf_run_multi.hip (RUNMULTIFLAGS), pekf_percall.hip (-ffp-contract=on), and pekf_side.hip, pekf_magcal.hip and
pekf_wire_dev.hip (COMMON alone).

Each __global__ kernel of namespace pekf in old.s (the listing's .amdhsa_kernel names: k_reset, k_live<TE, R64,
EV64, TRAJ>, k_run<Rec, ...>, k_op<OpWahba<1>>, whatever its template arguments) is compared with that of new.s:
instructions and block labels, comments and assembler directives dropped, the kernel's own name and its number in
the .LBB labels normalised.  A kernel is known by its name and template arguments, not by its parameter list; one
whose template gained trailing parameters that default to false (k_live<.., TRAJ> -> k_live<.., TRAJ, RESUME = 0>)
is compared under its old label.
Prints a line per kernel (lines, identical or the unified diff) and exits 1 on any difference, or on a kernel
that only one of the listings has."""
import difflib
import re
import sys

KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(_ZN4pekf\w+)")
LABEL = re.compile(r"^(_ZN4pekf\w+):\s*(;.*)?$")


def _args(s, i):
    """Itanium template arguments at s[i] == 'I' as text; returns (text, index after the closing 'E')."""
    out, i = [], i + 1
    while s[i] != "E":
        text, i = _type(s, i)
        out.append(text)
    return "<%s>" % ", ".join(out), i + 1


def _source_name(s, i):
    m = re.compile(r"\d+").match(s, i)
    end = m.end() + int(m.group())
    return s[m.end():end], end


def _type(s, i):
    if s[i] == "L":  # a literal: Lb1E, Li4E
        end = s.index("E", i)
        return s[i + 2:end], end + 1
    parts, nested = [], s[i] == "N"
    i += nested
    while True:
        if s[i] == "S":  # a substitution; here only S_ = pekf
            i = s.index("_", i) + 1
        elif s[i].isdigit():
            text, i = _source_name(s, i)
            parts.append(text)
        elif not parts and not nested:  # a builtin type
            return s[i], i + 1
        else:
            raise ValueError(s)
        if i < len(s) and s[i] == "I":
            text, i = _args(s, i)
            parts[-1] += text
        if not nested:
            break
        if s[i] == "E":
            i += 1
            break
    return "::".join(parts), i


def label_of(mangled):
    """k_run<Rec, 0, 1> from _ZN4pekf5k_runINS_3RecELb0ELb1EEEv...; the mangled name if it is beyond this parser"""
    try:
        name, i = _source_name(mangled, len("_ZN4pekf"))
        return name + (_args(mangled, i)[0] if mangled[i] == "I" else "")
    except (AttributeError, IndexError, ValueError):
        return mangled


def kernels(path):
    lines = open(path).read().splitlines()
    names = {m.group(1) for m in map(KERNEL.match, lines) if m}
    out, cur, name = {}, None, None
    for line in lines:
        m = LABEL.match(line)
        if m and m.group(1) in names:
            name, cur = m.group(1), []
            label = label_of(name)
            out[label if label not in out else name] = cur
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


def _grown(label, new):
    """The label in `new` of a kernel whose template gained trailing parameters that default to false
    (k_live<1, 1, 0, 0> -> k_live<1, 1, 0, 0, 0>: the same kernel, as k_live<TE, R64, EV64> was k_live<.., TRAJ = 0>)"""
    if not label.endswith(">"):
        return None
    for n in (1, 2, 3):
        grown = label[:-1] + ", 0" * n + ">"
        if grown in new:
            return grown
    return None


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    for label in [k for k in old if k not in new]:
        grown = _grown(label, new)
        if grown:
            new[label] = new.pop(grown)
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
    if not old and not new:
        print("no kernel of namespace pekf in either listing")
        bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
