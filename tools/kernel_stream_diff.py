"""Compare the gfx950 kernels of two builds instruction by instruction: for every kernel in the .s files of directory A that directory B
also has, the text between the kernel's label and its s_endpgm (comments and blank lines dropped) and five metadata values.

    python tools/kernel_stream_diff.py DIR_A DIR_B [file.s ...] > profiles/NAME.txt

Exit status 1 if any kernel differs or exists on one side only. tools/README.md shows how the .s files are made."""
import os
import re
import sys

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(path):
    """-> {name: (instruction lines, {meta key: value})}"""
    lines = open(path).read().splitlines()
    names = [m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.split(";")[0].strip() == name + ":")
        body = []
        for ln in lines[start + 1:]:
            # (local labels carry the kernel's ordinal in its file, .LBB12_3: dropped, so that kernels moving out of a file do not rename them)
            ln = re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", ln.split(";")[0].strip())
            if ln:
                body.append(ln)
            if ln == "s_endpgm":
                break
        out[name] = [body, {}]
    # the metadata note: one YAML map per kernel, `.name:` among its keys
    note = lines[next(i for i, ln in enumerate(lines) if ln.strip() == "amdhsa.kernels:"):]
    chunk = []
    for ln in note[1:] + ["  - end"]:
        if re.match(r"\s{2}- ", ln) or not ln.startswith(" "):
            kv = dict(m.groups() for c in chunk if (m := re.match(r"\s*-?\s*(\.\w+):\s*(\S+)\s*$", c)))
            if kv.get(".name") in out:
                out[kv[".name"]][1] = {k: kv.get(k) for k in META}
            chunk = []
        chunk.append(ln)
    return out


def main():
    a_dir, b_dir = sys.argv[1:3]
    files = sys.argv[3:] or sorted(f for f in os.listdir(a_dir) if f.endswith(".s"))
    bad = 0
    print(f"# A = {a_dir}   B = {b_dir}")
    print("# file kernel streams " + " ".join(k.lstrip(".") for k in META) + "   (A values; B's follow where they differ)")
    for f in files:
        a, b = kernels(os.path.join(a_dir, f)), kernels(os.path.join(b_dir, f))
        for name in sorted(set(a) | set(b)):
            if name not in a or name not in b:
                print(f"{f} {name} ONLY-IN-{'A' if name in a else 'B'}")
                bad += 1
                continue
            same = a[name][0] == b[name][0]
            meta_same = a[name][1] == b[name][1]
            bad += not (same and meta_same)
            line = f"{f} {name} {'identical' if same else 'DIFFERENT'} ({len(a[name][0])} lines) " + " ".join(str(a[name][1][k]) for k in META)
            if not meta_same:
                line += "   B: " + " ".join(str(b[name][1][k]) for k in META)
            print(line)
    print(f"# {bad} kernel(s) differ" if bad else "# every kernel identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
