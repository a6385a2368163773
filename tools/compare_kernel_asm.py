#!/usr/bin/env python3
"""Compare the kernels of two device-assembly files, old -> new (CPU only).

For a refactor that must not change device code: compile the translation unit
before and after with the flags ``ops/build.py`` gives it plus
``--cuda-device-only -S`` and hand both ``.s`` files to this script.  Every
kernel of NEW is matched *by name* to the kernel of OLD it replaces and two
things are compared after normalisation: the function body (its label up to
``.Lfunc_end``) and the ``.amdhsa_kernel`` descriptor (VGPRs, SGPRs, LDS,
scratch ...).  Normalisation strips comments, whitespace, the function index of
``.L`` labels and the kernel's own symbol name.

A kernel whose template parameters changed needs a rule that rebuilds the old
argument list from the new one ``a`` (a tuple of ints and bools), e.g.

    --rule 'flash_attn_kernel=a + (True, False)'

Kernels without a rule are matched to the same name and arguments.  Exit status
0 when every kernel of NEW is identical to its OLD counterpart.

    python tools/compare_kernel_asm.py old.s new.s [--rule NAME=EXPR ...]
"""
import argparse
import re
import sys

LIT = re.compile(r"L([a-z])(n?)(\d+)E")


def parse_symbol(sym):
    """``_ZN3dnn8kernelILi64ELb1EEEv...`` -> ("kernel", (64, True)); non-template kernels -> (name, ())."""
    m = re.match(r"_ZN?", sym)
    pos, name = m.end(), None
    while (m := re.compile(r"(\d+)").match(sym, pos)):  # nested names: the last one is the function
        n = int(m.group(1))
        name, pos = sym[m.end():m.end() + n], m.end() + n
    args = []
    if sym[pos:pos + 1] == "I":
        pos += 1
        while (m := LIT.match(sym, pos)):
            v = int(m.group(3)) * (-1 if m.group(2) else 1)
            args.append(bool(v) if m.group(1) == "b" else v)
            pos = m.end()
        if sym[pos:pos + 1] != "E":
            raise ValueError(f"template arguments other than integer literals: {sym}")
    return name, tuple(args)


def show(name, args):
    return name + ("<" + ",".join(str(a).lower() if isinstance(a, bool) else str(a) for a in args) + ">" if args else "")


def kernels(path):
    """{(name, args): (body lines, descriptor lines)} of every ``.amdhsa_kernel`` of the file."""
    lines = open(path).read().splitlines()
    out = {}
    for i, line in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if not m:
            continue
        sym = m.group(1)
        start = next(j for j in range(i, -1, -1) if lines[j].startswith(sym + ":"))
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        dend = next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])

        def norm(chunk):
            res = []
            for s in chunk:
                s = s.split(";")[0].replace(sym, "@K").replace(sym[2:], "@K")
                s = re.sub(r"\.L([A-Za-z_]+)\d+(_\d+)?", r".L\1\2", s)
                s = "".join(s.split())
                if s:
                    res.append(s)
            return res
        key = parse_symbol(sym)
        if key in out:
            raise ValueError(f"{path}: two kernels parse to {show(*key)}")
        out[key] = (norm(lines[start + 1:i] + lines[dend + 1:end]), norm(lines[i + 1:dend]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rule", action="append", default=[], metavar="NAME=EXPR",
                    help="old template arguments of kernel NAME as a Python expression of the new ones, a")
    a = ap.parse_args()
    rules = dict(r.split("=", 1) for r in a.rule)
    old, new = kernels(a.old), kernels(a.new)
    print(f"old: {len(old)} kernels, new: {len(new)} kernels")
    print("| old | new | body lines | body | descriptor |")
    print("|---|---|---|---|---|")
    bad = 0
    for (name, args), (body, desc) in sorted(new.items(), key=lambda kv: (kv[0][0], [int(x) for x in kv[0][1]])):
        oargs = tuple(eval(rules[name], {"__builtins__": {}, "a": args})) if name in rules else args
        if (name, oargs) not in old:
            print(f"| {show(name, oargs)}: not in old | {show(name, args)} | {len(body)} | - | - |")
            bad += 1
            continue
        obody, odesc = old[(name, oargs)]
        same_b, same_d = obody == body, odesc == desc
        bad += not (same_b and same_d)
        print(f"| {show(name, oargs)} | {show(name, args)} | {len(body)} | "
              f"{'identical' if same_b else 'DIFFERS'} | {'identical' if same_d else 'DIFFERS'} |")
    print(f"{len(new) - bad} of {len(new)} identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
