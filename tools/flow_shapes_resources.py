"""Register, scratch and LDS use of every k_rows, k_rows4 and k_ell_quad instantiation, this build against another one
(CPU only: it reads the code-object metadata of the object files the Makefile built, nothing runs).

Run:  python tools/flow_shapes_resources.py --parent-build <csrc/build of a build of the parent commit> \
          [--out profiles/flow_shapes_resources.txt]

Per kernel: VGPRs (.vgpr_count), AGPRs (.agpr_count), scratch bytes (.private_segment_fixed_size) and static LDS bytes
(.group_segment_fixed_size) of the gfx950 code object.  A kernel is an extended-kind instantiation when the TGP_FLOWX bit (16:
"X", kinds ARCSINH .. INV_BOXCOX) or the TGP_FLOWX2 bit (128: "X2", every kind) of its MODE / NW / NB template argument is set.
The verdict lines at the end state the two conditions the new flow kinds were held to: every non-X instantiation identical to
the parent's, and no X instantiation with scratch where the parent had none.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LLVM = "/opt/rocm/lib/llvm/bin"
FLOWX, FLOWX2 = 16, 128
KEYS = (".vgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels_of(build):
    """{demangled-ish kernel name: (vgpr, agpr, scratch, lds)} over every object of a build directory."""
    out = {}
    for obj in sorted(os.listdir(build)):
        if not obj.endswith(".o"):
            continue
        with tempfile.TemporaryDirectory() as tmp:
            o = os.path.join(tmp, obj)
            with open(os.path.join(build, obj), "rb") as src, open(o, "wb") as dst:
                dst.write(src.read())
            subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", o], cwd=tmp,
                                  stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            for dev in (f for f in os.listdir(tmp) if "gfx950" in f):
                notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, dev)], text=True)
                for chunk in notes.split("  - .agpr_count:")[1:]:
                    chunk = ".agpr_count:" + chunk
                    name = re.search(r"\.name:\s+(\S+)", chunk)
                    if not name or not re.match(r"_ZN3tgp(6k_rowsI|7k_rows4I|10k_ell_quadI)", name.group(1)):
                        continue
                    out[name.group(1)] = tuple(int(re.search(re.escape(k) + r":\s+(\d+)", chunk).group(1)) for k in KEYS)
    return out


def is_x(name):
    """"X" / "X2" / "": the TGP_FLOWX / TGP_FLOWX2 bit of the template argument that carries it (k_rows: MODE, 3rd; k_rows4: NW,
    4th; k_ell_quad: NB, last)."""
    ints = [int(x) for x in re.findall(r"Li(\d+)E", name)]
    bits = ints[2] if name.startswith("_ZN3tgp6k_rowsI") else ints[-1]
    return "X2" if bits & FLOWX2 else ("X" if bits & FLOWX else "")


def short(name):
    """k_rows<5, 8, 17, 16> from the mangled name (template arguments: ints, bools, one likelihood class)."""
    base = re.match(r"_ZN3tgp\d+(k_\w+?)I", name).group(1)
    targs = name[name.index(base) + len(base) + 1:name.index("EEvN") if "EEvN" in name else len(name)]
    parts = []
    for m in re.finditer(r"NS_\d+(\w+?)E(?=L|$)|Li(\d+)E|Lb(\d)E", targs):
        parts.append(m.group(1) or m.group(2) or ("true" if m.group(3) == "1" else "false"))
    return "%s<%s>" % (base, ", ".join(parts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-build", required=True)
    ap.add_argument("--build", default=os.path.join(REPO, "tgp", "pytorch_amd", "csrc", "build"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "flow_shapes_resources.txt"))
    args = ap.parse_args()
    new, old = kernels_of(args.build), kernels_of(args.parent_build)
    lines = ["# k_rows / k_rows4 / k_ell_quad instantiations: VGPRs, AGPRs, scratch bytes, static LDS bytes (gfx950 code-object",
             "# metadata), this build against a build of the parent commit.  X = extended flow kind set (TGP_FLOWX bit set).",
             "# %-66s %-2s %-22s %-22s %s" % ("kernel", "X", "parent v/a/scr/lds", "this v/a/scr/lds", "same")]
    bad_plain, bad_scratch = [], []
    for name in sorted(set(new) | set(old), key=short):
        x, a, b = is_x(name), old.get(name), new.get(name)
        if not x and a != b:
            bad_plain.append(short(name))
        if x == "X" and (b is None or (a is not None and a[2] == 0 and b[2] > 0)):
            bad_scratch.append(short(name))
        fmt = lambda v: "-" if v is None else "%d/%d/%d/%d" % v      # noqa: E731
        lines.append("%-68s %-2s %-22s %-22s %s" % (short(name), x, fmt(a), fmt(b), "yes" if a == b else "NO"))
    nx, nx2 = sum(1 for n in new if is_x(n) == "X"), sum(1 for n in new if is_x(n) == "X2")
    lines.append("")
    lines.append("kernels: %d in this build (%d plain, %d X, %d X2), %d in the parent's" % (len(new), len(new) - nx - nx2, nx, nx2, len(old)))
    lines.append("plain (non-X) instantiations that differ from the parent: %d %s" % (len(bad_plain), bad_plain or ""))
    lines.append("X instantiations that gained scratch (parent 0 bytes): %d %s" % (len(bad_scratch), bad_scratch or ""))
    changed = [short(n) for n in new if is_x(n) == "X" and old.get(n) != new[n]]
    lines.append("X instantiations whose numbers changed at all: %d of %d %s" % (len(changed), nx, changed or ""))
    x2s = [n for n in new if is_x(n) == "X2" and new[n][2] > 0]
    lines.append("X2 instantiations (new) with scratch: %d of %d" % (len(x2s), nx2))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-5:]))
    return 1 if bad_plain or bad_scratch else 0


if __name__ == "__main__":
    sys.exit(main())
