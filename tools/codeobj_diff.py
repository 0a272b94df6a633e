#!/usr/bin/env python3
"""Compare the gfx950 code objects of two builds of one translation unit, kernel by kernel (CPU only).
Usage: tools/codeobj_diff.py OLD.o NEW.o   (object files or libraries; exit status 0 when the device code matches)

For a change that must leave the device code alone (moving source text, a host-only edit).  Equal sha256 of
the two code objects settles it.  Otherwise -- hipcc names one symbol per unit, __hip_cuid_<hash>, after a
hash of the input path and the command line, so a new compiler option alone changes the file -- the tool shows
that both define the same kernels, that every kernel's machine code (the bytes of its symbol in .text) and
kernel descriptor match, and that every kernel's metadata record (registers, spills, scratch, LDS, kernarg
layout, workgroup size) matches.  A host-only edit that changes the order in which templates are instantiated
moves kernels inside .text: a descriptor's one position-dependent field, the distance to its kernel's code
(kernel_code_entry_byte_offset, bytes 16..23), is therefore compared as the address it resolves to -- in each
build it must be the kernel's own symbol -- and the other 56 bytes as they stand."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

from kernel_resources import LLVM, code_object


def readelf(co, *flags):
    return subprocess.run([LLVM + "/llvm-readelf", "-W", *flags, co], check=True, capture_output=True,
                          text=True).stdout


def load(obj, tmp, tag):
    co = os.path.join(tmp, tag)
    code_object(obj, co)
    blob = open(co, "rb").read()
    # section number -> (address, file offset), to find a symbol's bytes
    secs = {int(m.group(1)): (int(m.group(2), 16), int(m.group(3), 16)) for m in re.finditer(
        r"^\s*\[\s*(\d+)\]\s+\S+\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", readelf(co, "-S"), re.M)}
    syms, addrs = {}, {}
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)$",
                         readelf(co, "--symbols"), re.M):
        addr, size, ndx, name = int(m.group(1), 16), int(m.group(2)), int(m.group(4)), m.group(5)
        if ndx in secs and not name.startswith("__hip_cuid_"):
            base, off = secs[ndx]
            syms[name] = blob[off + addr - base: off + addr - base + size]
            addrs[name] = addr
    # a descriptor as (its bytes without the entry offset, whether that offset leads to the kernel's own code)
    for name in [n for n in syms if n.endswith(".kd") and len(syms[n]) == 64]:
        kd = syms[name]
        target = addrs[name] + int.from_bytes(kd[16:24], "little", signed=True)
        syms[name] = (kd[:16] + kd[24:], target == addrs.get(name[:-3]))
    # the metadata note: one record per kernel, a list item at indent 2 (see kernel_resources.py)
    meta, cur = {}, None
    for line in readelf(co, "--notes").splitlines():
        if line.startswith("  - "):
            cur = []
        elif not line.startswith("    "):
            cur = None
        if cur is not None:
            cur.append(line)
            m = re.match(r"^    \.name:\s+(\S+)", line)
            if m:
                meta[m.group(1)] = cur
    return hashlib.sha256(blob).hexdigest(), syms, meta


def main(old, new):
    with tempfile.TemporaryDirectory() as tmp:
        (ha, sa, ma), (hb, sb, mb) = load(old, tmp, "a"), load(new, tmp, "b")
    print("sha256 %s  %s\nsha256 %s  %s" % (ha, old, hb, new))
    print("kernels: %d and %d" % (len(ma), len(mb)))
    if ha == hb:
        print("IDENTICAL code objects")
        return 0
    bad = 0
    for what, a, b in (("symbol", sa, sb), ("metadata record", ma, mb)):
        for name in sorted(set(a) ^ set(b)):
            print("%s only in %s: %s" % (what, old if name in a else new, name))
            bad += 1
        diff = [n for n in sorted(set(a) & set(b)) if a[n] != b[n]]
        for name in diff:
            print("%s differs: %s" % (what, name))
        bad += len(diff)
        print("%d %ss compared, %d differ" % (len(set(a) & set(b)), what, len(diff)))
    for which, s in ((old, sa), (new, sb)):
        astray = [n for n, v in sorted(s.items()) if isinstance(v, tuple) and not v[1]]
        for name in astray:
            print("descriptor in %s does not lead to its kernel's code: %s" % (which, name))
        bad += len(astray)
    missing = [k for k in ma if k not in sa or k + ".kd" not in sa]
    for k in missing:
        print("kernel without code or descriptor symbol: %s" % k)
    bad += len(missing)
    print("SAME device code, kernel by kernel (the files differ outside it)" if not bad else "DIFFERENT device code")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
