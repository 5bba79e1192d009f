#!/usr/bin/env python3
r"""Do two device-assembly files (hipcc --cuda-device-only -S) hold the same kernels?  Pairs them by mangled name and prints every
pair whose instruction lines or resource metadata (the .amdhsa_ directives and the "; Kernel info:" block: registers, ScratchSize,
LDS, kernel-argument size, ...) differ, and every kernel without a partner; exit status 1 if there is any.  The check behind
"this change leaves the kernels' instruction streams untouched".
    python scripts/isa_diff.py old.s new.s [map.txt]
map.txt renames kernels of old.s, one `<regex> <replacement>` (re.sub on the mangled name) per line.  A kernel's own name inside its
labels / symbol references, the function number of local labels (.LBB<n>_) and the file-wide counter of a long branch's
.Lpost_getpc<n> label (it moves when a kernel in front of it leaves the file) are neutralised before comparing.
A changed parameter type renames EVERY instantiation, not only a renamed kernel.  Example: gemm_fp8.hip, when gemm_fp8_mfma_tr /
gemm_fp8_tail_tr became the TR instantiations of gemm_fp8_mfma / gemm_fp8_tail (argument std::conditional_t<TR, GemmArgs8T, GemmArgs8>):
    16gemm_fp8_mfma_trI(\w+?E)EEvNS0_10GemmArgs8TE$ 13gemm_fp8_mfmaI\1Lb1ELb1ELb1EEEvNSt11conditionalIXT6_ENS0_10GemmArgs8TENS0_9GemmArgs8EE4typeE
    16gemm_fp8_tail_trI(\w+?E)EEvNS0_10GemmArgs8TE$ 13gemm_fp8_tailI\1Lb1ELb1EEEvNSt11conditionalIXT1_ENS0_10GemmArgs8TENS0_9GemmArgs8EE4typeE
    (13gemm_fp8_mfmaI\w+?E)EEvNS0_9GemmArgs8E$ \1Lb0EEEvNSt11conditionalIXT6_ENS0_10GemmArgs8TENS0_9GemmArgs8EE4typeE
    (13gemm_fp8_tailI\w+?E)EEvNS0_9GemmArgs8E$ \1Lb0EEEvNSt11conditionalIXT1_ENS0_10GemmArgs8TENS0_9GemmArgs8EE4typeE"""
import re
import sys

from isa_order import kernels


def load(path):
    """{mangled name: (instruction lines, metadata lines)}"""
    text = open(path).read()
    code = kernels(text, end=".Lfunc_end")
    out = {}
    for f in re.split(r"\n(?=_Z\w+:)", text)[1:]:
        name = f.split(":")[0]
        meta = [re.sub(r"\s+", " ", l).strip() for l in f.splitlines()]
        meta = [l for l in meta if l.startswith(".amdhsa_") or re.match(r"; [\w:]+ ?: ", l)]
        neutral = lambda l: re.sub(r"\.L(BB|JTI|tmp)\d+_|\.L(post_getpc)\d+", r".L\1\2_", l.replace(name, "<self>"))
        out[name] = ([neutral(l) for l in code[name]], [neutral(l) for l in meta])
    return out


def main():
    old, new = load(sys.argv[1]), load(sys.argv[2])
    if len(sys.argv) > 3:
        for line in open(sys.argv[3]):
            if line.strip():
                pat, repl = line.split()
                old = {re.sub(pat, repl, n): v for n, v in old.items()}
    bad = 0
    for n in sorted(set(old) | set(new)):
        if n not in old or n not in new:
            print("unpaired (%s only): %s" % ("old" if n in old else "new", n)); bad += 1
            continue
        for what, a, b in zip(("instructions", "metadata"), old[n], new[n]):
            if a != b:
                first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                print("%s differ: %s\n   %d | %d lines, first at %d:  %s  |  %s" % (what, n, len(a), len(b), first, a[first:first + 1], b[first:first + 1]))
                bad += 1
                break
    print("isa_diff: %d kernels in old, %d in new, %d paired, %d differing or unpaired" % (len(old), len(new), len(set(old) & set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
