"""Compare two hipcc -S (device-only) assembly files kernel by kernel: per mangled name, whether
the instruction streams are identical, and the kernel-descriptor fields (registers, spills, scratch,
LDS) of both.  Comments are dropped and basic-block labels renumbered per function, so a kernel
that merely moved in the file compares equal.

    python tools/isa_diff.py OLD.s NEW.s [--rename OLD_SUBSTRING=NEW_SUBSTRING ...] [SUBSTRING_OF_MANGLED_NAME ...]

--rename (repeatable) rewrites the OLD side's mangled names (the kernels' and the symbols their
instructions refer to) before pairing, for a change that drops or adds a template parameter:
--rename k_riccati_mfmaILi0E=k_riccati_mfmaI.

Exit status 1 if a kernel is missing on one side or differs.
"""
import difflib
import re
import sys

from isa_stats import kernel_bodies, stats

FIELDS = ["vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
          "private_segment_fixed_size", "group_segment_fixed_size"]


def insts(body):
    out = []
    for line in body.splitlines():
        t = line.split(";")[0].strip()
        if not t or t.startswith("."):
            if not re.match(r"\.LBB\d+_\d+:", t):
                continue
        out.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t))
    return out


def descriptors(text):
    """{mangled name: {field: value}} from the amdhsa.kernels metadata"""
    d = {}
    meta = text[text.find("amdhsa.kernels:"):]
    for chunk in re.split(r"^  - (?=\.)", meta, flags=re.M)[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", chunk, re.M)
        if name:
            d[name.group(1)] = {f: int(m.group(1)) for f in FIELDS
                                if (m := re.search(rf"^\s+\.{f}:\s+(\d+)", chunk, re.M))}
    return d


def main():
    args, renames = sys.argv[1:], []
    while "--rename" in args:
        i = args.index("--rename")
        renames.append(args[i + 1].split("=", 1))
        del args[i:i + 2]
    old, new, pats = open(args[0]).read(), open(args[1]).read(), args[2:]

    for a, b in renames:
        old = old.replace(a, b)
    ko, kn = dict(kernel_bodies(old)), dict(kernel_bodies(new))
    do, dn = descriptors(old), descriptors(new)
    bad = 0
    for name in sorted(set(ko) | set(kn)):
        if not all(p in name for p in pats) or not (name in do or name in dn):  # (kernels only: no data symbols)
            continue
        if name not in ko or name not in kn:
            print(f"{name[:100]}: only in {'OLD' if name in ko else 'NEW'}")
            bad = 1
            continue
        a, b = insts(ko[name]), insts(kn[name])
        n = sum(1 for op in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes() if op[0] != "equal"
                for _ in range(max(op[2] - op[1], op[4] - op[3]))) if a != b else 0
        same_d = do.get(name) == dn.get(name)
        verdict = "identical" if a == b else f"DIFFERS ({n} of {len(a)} lines; insts {stats(ko[name])['insts']} -> {stats(kn[name])['insts']})"
        if a != b and [t.split()[0] for t in a] == [t.split()[0] for t in b]:
            verdict += " (same opcode sequence: operands only)"
        elif a != b and sorted(t.split()[0] for t in a) == sorted(t.split()[0] for t in b):
            verdict += " (same opcode counts: reordered)"
        print(f"{name[:100]}: {verdict}; descriptor {'identical' if same_d else 'DIFFERS'}")
        if a != b or not same_d:
            bad = 1
            for f in FIELDS:  # (the fields that changed; one a side lacks shows as None)
                if do.get(name, {}).get(f) != dn.get(name, {}).get(f):
                    print(f"    {f}: {do.get(name, {}).get(f)} -> {dn.get(name, {}).get(f)}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
