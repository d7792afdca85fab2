#!/usr/bin/env python3
"""Hand-written `asm volatile` global loads (csrc/vit.hip: rt_gload) are invisible to the compiler: it believes the destination
registers hold their data as soon as the statement is passed, and under register pressure it may copy them (to an AGPR) or reuse
them - as an ADDRESS register, say - before the hand-placed s_waitcnt has retired the load.  This compiles one .hip file for
gfx950 (device only, no GPU needed) and reports, per kernel, every instruction that touches the destination of such a load while
it is still in flight.  Exit status 1 if any.
    tools/check_asm_loads.py semantic-slam-master_amd/csrc/vit.hip"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def regs_of(text):
    out = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]", text):
        out |= set(range(int(m.group(1)), int(m.group(2)) + 1))
    for m in re.finditer(r"\bv(\d+)\b", text):
        out.add(int(m.group(1)))
    return out


def check(lines):
    pending, in_asm, bad = [], False, []          # pending: (destination registers, line) of asm loads, oldest first
    for n, l in enumerate(lines, 1):
        s = l.strip()
        if s.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if s.startswith(";;#ASMEND"):
            in_asm = False
            continue
        if not s or s[0] in ";.":
            continue
        m = re.match(r"s_waitcnt.*vmcnt\((\d+)\)", s)
        if m:                                     # memory operations retire in issue order: at most N stay outstanding
            del pending[:max(0, len(pending) - int(m.group(1)))]
            continue
        if in_asm and s.startswith("global_load"):
            touched = regs_of(s)
            bad += [(n, s, ln) for p, ln in pending if p & touched]
            pending.append((regs_of(s.split(",")[0]), n))
            continue
        r = regs_of(s)
        hit = [ln for p, ln in pending if p & r]
        if hit:
            bad.append((n, s, hit[0]))
    return bad


def main():
    src = sys.argv[1]
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "dev.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                               "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S", "-I" + os.path.dirname(os.path.abspath(src)),
                               src, "-o", asm], stderr=subprocess.DEVNULL)
        text = open(asm).read()
    total = 0
    for name in re.findall(r"^(\w+):\s*; @", text, flags=re.M):
        a = text.index("\n" + name + ":")
        b = text.find("s_endpgm", a)
        if b < 0:
            continue
        bad = check(text[a:b].split("\n"))
        print(f"{name[:90]:90s} {len(bad)}")
        for n, s, ln in bad[:5]:
            print(f"    +{n}: {s}   <- destination of the load at +{ln} still in flight")
        total += len(bad)
    return 1 if total else 0


if __name__ == "__main__":
    sys.exit(main())
