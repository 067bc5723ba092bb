#!/usr/bin/env python3
"""Compares the gfx950 instruction text of two builds, function by function: tools/disasm_compare.py OLD.s NEW.s, with the files
tools/disasm.sh writes (RT_DISASM_TAG names them). Labels are renumbered per function and comments dropped; everything else has to
be the same for every device function OLD has. Prints the functions that differ or went missing and the ones NEW adds; exit
status 1 if any differs."""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+|k_\w+):\s*(;.*)?$", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name], name = body, None
            continue
        text = line.split(";")[0].rstrip()
        if text.strip():
            text = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", text)
            body.append(re.sub(r"\.L(tmp|__unnamed_)\d+", r".L\1", text))
    return out


def main(old, new):
    a, b = functions(old), functions(new)
    missing = [k for k in a if k not in b]
    differ = [k for k in a if k in b and a[k] != b[k]]
    print(f"{len(a)} device functions in {old}, {len(b)} in {new}: {len(missing)} missing, {len(differ)} differ")
    for k in missing:
        print("missing:", k)
    for k in differ:
        at = next((i for i, (p, q) in enumerate(zip(a[k], b[k])) if p != q), min(len(a[k]), len(b[k])))
        print(f"differs: {k} ({len(a[k])} -> {len(b[k])} lines, first at {at})")
    for k in b:
        if k not in a:
            print("new:", k)
    return 1 if missing or differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
