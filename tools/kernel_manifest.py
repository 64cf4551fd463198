#!/usr/bin/env python3
"""Manifest of the gfx950 device code in a built liblandhydro_hip.so: per symbol a hash of its
instructions, per kernel its amdhsa metadata.  Two builds select among the same kernels exactly when
their manifests are equal, which is how a launch-side refactor is shown to leave the device code alone.

  tools/kernel_manifest.py LIB > a.txt           one line per symbol, then a count and a digest
  tools/kernel_manifest.py LIB_A LIB_B           the difference (exit status 1 if there is one)

An argument may also be a manifest written earlier.  The instruction text is llvm-objdump's with the
address column and the // comments removed, so code that only moved hashes the same.  A kernel entry that
lacks one of the metadata fields is an error, not a blank.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
META = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "max_flat_workgroup_size", "kernarg_segment_size")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True, errors="replace").stdout


def symbol_hashes(code_object):
    """{symbol: sha256 of its instruction lines} of one code object."""
    out, name, h = {}, None, None
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", code_object).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name, h = m.group(1), hashlib.sha256()
            out[name] = h
        elif name and line.startswith((" ", "\t")):
            text = re.sub(r"^\s*[0-9a-f]+:\s*", "", line.split("//")[0]).strip()
            # branch targets print as <symbol+0xOFFSET>: relative to the symbol, so they stay;
            # "..." is the zero fill up to the next symbol's alignment: placement, not code
            if text and text != "...":
                h.update(text.encode() + b"\n")
    return {k: v.hexdigest()[:16] for k, v in out.items()}


def kernel_metadata(code_object):
    """{kernel symbol: "key=value ..."} from the amdhsa.kernels note.  The note is YAML: a kernel is a
    list item of the kernels' own indentation ("  - "), its fields are the keys one level in; the
    argument entries nested under .args sit deeper and are not read."""
    notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", code_object).splitlines()
    out, entry = {}, None

    def close(entry):
        if entry is None:
            return
        missing = [k for k in ("name",) + META if k not in entry]
        if missing:
            sys.exit("%s: kernel entry %s lacks %s" % (code_object, entry.get("name", "?"), ", ".join(missing)))
        if entry["name"] in out:
            sys.exit("%s: two kernel entries named %s" % (code_object, entry["name"]))
        out[entry["name"]] = " ".join("%s=%s" % (k, entry[k]) for k in META)

    inside = False
    for line in notes:
        if not inside:
            inside = line.rstrip() == "amdhsa.kernels:"
            continue
        if line.startswith("  - "):          # the next kernel
            close(entry)
            entry, line = {}, "    " + line[4:]
        elif line and not line.startswith(" "):  # the next top-level key: the list is over
            break
        m = re.match(r"^    \.(\w+):\s*(\S*)\s*$", line)
        if m and entry is not None:
            entry[m.group(1)] = m.group(2)
    close(entry)
    if not out:
        sys.exit("%s: no amdhsa.kernels entries" % code_object)
    return out


def manifest_of_library(lib):
    lines = {}
    with tempfile.TemporaryDirectory() as tmp:
        # llvm-objdump --offloading writes the bundles beside its input: work on a copy
        copy = os.path.join(tmp, "lib.so")
        shutil.copy(lib, copy)
        run(os.path.join(LLVM, "llvm-objdump"), "--offloading", copy, cwd=tmp)
        objs = sorted(f for f in os.listdir(tmp) if f.endswith("gfx950"))
        if not objs:
            sys.exit("%s: no gfx950 code object" % lib)
        for f in objs:
            co = os.path.join(tmp, f)
            meta = kernel_metadata(co)
            for sym, h in symbol_hashes(co).items():
                # a template instantiated in several translation units: one entry per distinct body
                lines.setdefault(sym, set()).add("%s %s" % (h, meta.get(sym, "-")))
    return {sym: " | ".join(sorted(v)) for sym, v in lines.items()}


def read(path):
    with open(path, "rb") as f:
        if f.read(4) == b"\x7fELF":
            return manifest_of_library(path)
    lines = {}
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        sym, rest = line.rstrip("\n").split(" ", 1)
        lines[sym] = rest
    return lines


def digest(lines):
    h = hashlib.sha256()
    for sym in sorted(lines):
        h.update(("%s %s\n" % (sym, lines[sym])).encode())
    return h.hexdigest()


def summary(lines):
    kernels = sum(1 for v in lines.values() if not v.endswith(" -"))
    return "# %d symbols (%d kernels), sha256 %s" % (len(lines), kernels, digest(lines))


def main(argv):
    if len(argv) == 2:
        lines = read(argv[1])
        for sym in sorted(lines):
            print(sym, lines[sym])
        print(summary(lines))
        return 0
    if len(argv) != 3:
        sys.exit(__doc__)
    a, b = read(argv[1]), read(argv[2])
    for sym in sorted(set(a) - set(b)):
        print("only in %s: %s" % (argv[1], sym))
    for sym in sorted(set(b) - set(a)):
        print("only in %s: %s" % (argv[2], sym))
    changed = [s for s in sorted(set(a) & set(b)) if a[s] != b[s]]
    for sym in changed:
        print("differs: %s\n  %s\n  %s" % (sym, a[sym], b[sym]))
    print(argv[1], summary(a))
    print(argv[2], summary(b))
    same = a == b
    print("manifests are equal" if same else "manifests DIFFER")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
