#!/usr/bin/env python3
"""Per-kernel comparison of device assembly across a change that moves kernels
between translation units:

    make -C trex_amd/csrc tree.s                      # in a worktree of the old commit
    make -C trex_amd/csrc tree.s tree_gram.s ...      # in the new tree
    tools/asm_kernels.py [--rename=A=B ...] OLD.s [OLD.s ...] -- NEW.s [NEW.s ...]

Each side's `make NAME.s` listings are cut into one chunk per function, keyed
by the demangled name, and the kernels' metadata entries likewise; a chunk is
normalised (c++filt; `.section` / `.file` / `.ident` / comment lines dropped;
`__hip_cuid_<hash>` collapsed; each `--rename`'s demangled text A replaced by B,
for a type the change renamed; the function's ordinal taken out of `.LBB<n>_`
and `.Lfunc_end<n>` labels, which count functions per file) and the two sides
compared by name: instructions, labels, `.amdhsa_*` and metadata.  Prints the
names that differ or exist on one side only; exit status 1 if any."""
import re
import subprocess
import sys


RENAMES = []


def chunks(path):
    with open(path) as f:
        raw = subprocess.run(["c++filt"], stdin=f, capture_output=True, text=True, check=True).stdout
    for a, b in RENAMES:
        raw = raw.replace(a, b)
    raw = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", raw)
    text, _, meta = raw.partition("\t.amdgpu_metadata")
    text = text.split("\t.set amdgpu.max_num_vgpr")[0]  # the file's trailer
    funcs, key = {}, None
    for line in text.split("\n"):
        m = re.match(r"\s*\.globl\s+(.*?)\s*; -- Begin function", line)
        if m:
            key = m.group(1)
            assert key not in funcs, key
            funcs[key] = []
        if key is None or not line.strip() or re.match(r"\s*(\.section|\.file|\.ident|;)", line):
            continue
        line = re.sub(r"\s*;.*$", "", line)
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        funcs[key].append(re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line))
    md = {}
    for entry in re.split(r"\n(?=  - \.)", meta):
        m = re.search(r"\.name:\s+(.*)", entry)
        if m and ".kernarg_segment_size" in entry:
            md[m.group(1).strip().strip("'")] = entry.split("\namdhsa.target")[0].rstrip().split("\n")
    return funcs, md


def side(paths):
    funcs, md = {}, {}
    for p in paths:
        f, m = chunks(p)
        assert not set(f) & set(funcs), sorted(set(f) & set(funcs))
        funcs.update(f)
        md.update(m)
    return funcs, md


def main():
    args = sys.argv[1:]
    while args[0].startswith("--rename="):
        RENAMES.append(tuple(args.pop(0)[len("--rename="):].split("=", 1)))
    sep = args.index("--")
    (of, om), (nf, nm) = side(args[:sep]), side(args[sep + 1:])
    print(f"old: {len(of)} functions, {len(om)} kernels; new: {len(nf)} functions, {len(nm)} kernels")
    bad = 0
    for what, old, new in (("code", of, nf), ("metadata", om, nm)):
        for k in sorted(set(old) | set(new)):
            if k not in old or k not in new:
                print(f"{what} only in {'old' if k in old else 'new'}: {k}")
            elif old[k] != new[k]:
                n = sum(x != y for x, y in zip(old[k], new[k])) + abs(len(old[k]) - len(new[k]))
                print(f"{what} differs ({n} of {len(old[k])} lines): {k}")
            else:
                continue
            bad += 1
    print("differences:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
