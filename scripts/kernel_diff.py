#!/usr/bin/env python
"""Compare the device assembly of a library between two trees, kernel by kernel (CPU only).

    python scripts/kernel_diff.py [--policy] OLD NEW [-o table.txt]

OLD and NEW are each a checkout of this repository (its gpd.hip is cross-compiled to device
assembly with the flags of _build.build(); with --policy every unit of libgpd_policy.so, named as
_build.POLICY_UNITS names them and found under csrc/policy/ or, in a tree from before the move,
under csrc/, with the flags of _build.build_policy()) or a .s file made that way.  Per kernel symbol the
table says whether the two bodies are identical once comments are stripped and local labels are
renumbered, and lists VGPRs, SGPRs, scratch bytes, static LDS, code length and occupancy as the
assembler reports them.  Whole bodies are compared; nothing looks inside them.
"""
import argparse
import pathlib
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
from gym_pybullet_drones_routing_amd import _build  # noqa: E402

PKG = "gym_pybullet_drones_routing_amd"
FIELDS = (("vgpr", "NumVgprs"), ("agpr", "NumAgprs"), ("sgpr", "TotalNumSgprs"), ("scratch", "ScratchSize"),
          ("lds", "LDSByteSize"), ("code", "codeLenInByte"), ("occ", "Occupancy"))


def units(src, policy):
    """The translation units of the library in the tree `src`."""
    csrc = src / PKG / "csrc"
    if not policy:
        return [csrc / "gpd.hip"]
    found = []
    for u in _build.POLICY_UNITS:
        where = [d / u.name for d in (csrc / "policy", csrc) if (d / u.name).exists()]
        if not where:
            raise SystemExit(f"{src}: no {u.name} under {csrc / 'policy'} or {csrc}")
        found.append(where[0])
    return found


def device_asm(src, out, policy=False):
    """The device assembly of a tree, compiled to `out`.N.s (or the text of the .s file given)."""
    src = pathlib.Path(src)
    if not src.is_dir():
        return src.read_text()
    flags = _build.POLICY_FLAGS if policy else _build.DEVICE_FLAGS
    text = ""
    for n, unit in enumerate(units(src, policy)):
        asm = pathlib.Path(f"{out}.{n}.s")
        subprocess.run([_build.hipcc()] + flags + [f"-I{src / 'include'}", "--cuda-device-only", "-S", "-o", str(asm),
                                                   str(unit)], check=True)
        text += asm.read_text()
    return text


def kernels(asm):
    """{symbol: (normalised body lines, {field: value})} of every .amdhsa_kernel in the text."""
    lines = asm.splitlines()
    names = [m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
    start = {ln.split(":")[0]: i for i, ln in enumerate(lines) if re.match(r"[A-Za-z_][\w.$]*:", ln)}
    out = {}
    for name in names:
        i = start[name] + 1
        body, labels = [], {}
        while not re.match(r"\s*\.(section|amdhsa_kernel)\b", lines[i]):
            ln = lines[i].split(";")[0].strip()
            if ln:
                ln = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), ln)
                body.append(re.sub(r"\s+", " ", ln))
            i += 1
        info = {}
        while i < len(lines) and not (lines[i].startswith("\t.type") or lines[i].startswith("\t.protected")):
            for key, word in FIELDS:
                m = re.match(rf";\s*{word}:?\s*=?\s*(\d+)", lines[i])
                if m and key not in info:
                    info[key] = int(m.group(1))
            m = re.match(r"\s*\.amdhsa_(group|private)_segment_fixed_size\s+(\d+)\s*$", lines[i])
            if m:
                info["lds" if m.group(1) == "group" else "scratch"] = int(m.group(2))
            i += 1
        out[name] = (body, info)
    return out


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "c++filt"
    try:
        res = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, res.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name):
    name = re.sub(r"^(void )?(gpd|\(anonymous namespace\))::", "", name)
    return re.sub(r"\(.*$", "", name)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("-o", "--out", help="also write the table to this file")
    ap.add_argument("--policy", action="store_true", help="compare libgpd_policy.so's units instead of gpd.hip")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old, new = (kernels(device_asm(src, pathlib.Path(tmp) / str(i), args.policy))
                    for i, src in enumerate((args.old, args.new)))
    pretty = demangle(sorted(set(old) | set(new)))
    cols = [k for k, _ in FIELDS]
    rows = [f"{'kernel':<72} {'body':<9} " + " ".join(f"{c:>13}" for c in cols)]
    counts = {"same": 0, "differs": 0, "old only": 0, "new only": 0}
    for sym in sorted(pretty, key=lambda s: pretty[s]):
        o, n = old.get(sym), new.get(sym)
        verdict = "old only" if n is None else "new only" if o is None else "same" if o[0] == n[0] else "differs"
        counts[verdict] += 1
        cells = []
        for c in cols:
            a = "-" if o is None else o[1].get(c, "?")
            b = "-" if n is None else n[1].get(c, "?")
            cells.append(f"{a}" if a == b else f"{a}->{b}")
        rows.append(f"{short(pretty[sym]):<72} {verdict:<9} " + " ".join(f"{c:>13}" for c in cells))
    rows.append("")
    rows.append(", ".join(f"{v} {k}" for k, v in counts.items()))
    text = "\n".join(rows) + "\n"
    sys.stdout.write(text)
    if args.out:
        pathlib.Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
