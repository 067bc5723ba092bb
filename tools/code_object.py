#!/usr/bin/env python3
"""Register budget of every kernel of a built library, read from the gfx950 code object inside it (tools/kernel_info.py reads the
same figures from a -S listing): VGPRs, SGPRs, scratch bytes, SGPR spills, VGPR spills.
usage: tools/code_object.py <librt_amd.so> [<parent librt_amd.so>] [substring]
       with two libraries: one line per kernel, parent -> this build (profiles/r05_registers.txt was written that way)."""
import os, re, struct, subprocess, sys, tempfile

LLVM_BIN = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".sgpr_spill_count", ".vgpr_spill_count")
ALSO_READ = (".group_segment_fixed_size", ".max_flat_workgroup_size")   # in kernels()' rows, not in the printed figures


def extract(lib, arch="gfx950"):
    """The code object of `arch` in the library's offload bundle, as bytes."""
    d = open(lib, "rb").read()
    i = d.find(MAGIC)
    if i < 0:
        raise RuntimeError(f"{lib}: no offload bundle")
    n, = struct.unpack_from("<Q", d, i + len(MAGIC))
    p = i + len(MAGIC) + 8
    for _ in range(n):
        off, size, idlen = struct.unpack_from("<QQQ", d, p)
        p += 24
        tid = d[p:p + idlen].decode()
        p += idlen
        if tid.endswith(arch) and size:
            return d[i + off:i + off + size]
    raise RuntimeError(f"{lib}: no {arch} code object in the bundle")


def _tool(name, args, blob):
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(blob)
        f.flush()
        return subprocess.run([os.path.join(LLVM_BIN, name)] + args + [f.name], capture_output=True, text=True, check=True).stdout


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def kernels(lib):
    """{demangled kernel name without its argument list: {field: value}} from the code object's metadata note."""
    text = _tool("llvm-readelf", ["--notes"], extract(lib))
    rows, cur = {}, {}
    for line in text.splitlines():
        m = re.match(r"\s+(?:- )?(\.\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if line.lstrip().startswith("- .agpr_count") and cur:   # the first key of the next kernel's map
            rows[cur[".name"]] = cur
            cur = {}
        if m.group(1) in FIELDS or m.group(1) in ALSO_READ:
            cur[m.group(1)] = int(m.group(2))
        elif m.group(1) == ".name" and line.startswith("    .name"):   # (arguments have a .name of their own, indented deeper)
            cur[".name"] = m.group(2)
    if cur:
        rows[cur[".name"]] = cur
    dm = demangle(list(rows))
    return {re.sub(r"\((DevScene|FusedKernArgs).*$", "", dm[k]): v for k, v in rows.items()}


def disassembly(lib):
    """{mangled symbol: [instruction mnemonics]} of the code object's text."""
    text = _tool("llvm-objdump", ["-d", "--no-show-raw-insn"], extract(lib))
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith(("\t", " ")) and line.strip():
            cur.append(line.split()[0])
    return out


def figures(k):
    return "(" + ", ".join(str(k.get(f, 0)) for f in FIELDS) + ")"


if __name__ == "__main__":
    libs = [a for a in sys.argv[1:] if a.endswith(".so")]
    sub = ([a for a in sys.argv[1:] if not a.endswith(".so")] + [""])[0]
    new = kernels(libs[0])
    old = kernels(libs[1]) if len(libs) > 1 else None
    print("# (VGPRs, SGPRs, scratch bytes, SGPR spills, VGPR spills)" + (", parent -> this build" if old else ""))
    for name in sorted(new):
        if sub in name:
            print(name + (figures(old[name]) + " -> " if old and name in old else "") + figures(new[name]))
