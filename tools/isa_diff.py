"""Per-kernel diff of the gfx950 machine code of two source trees: python tools/isa_diff.py OLD_TREE NEW_TREE [FILE.hip ...]

Compiles every evcont_amd/csrc/*.hip of both trees (or only the named files) device-only to assembly with the flags of
evcont_amd/build.py and compares, kernel symbol by kernel symbol, the instructions and the .amdhsa_* descriptor fields
(registers, LDS, scratch), ignoring label numbering, symbol order and which file a kernel lives in.  Three verdicts:
  identical                          the same instructions and the same descriptor;
  identical up to register names     the same sequence of mnemonics, immediates and modifiers and the same descriptor, only
                                     the numbers of s<N> / v<N> / a<N> operands differ (listed by name);
  DIFFERS                            anything else, with the register / LDS / scratch figures of both.
A refactor that only moves code prints nothing but the first two."""
import glob, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

FIGURES = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(tree, tmp):
    sys.path.insert(0, tree)
    from evcont_amd import build as b
    del sys.path[0]
    for m in [m for m in sys.modules if m.startswith("evcont_amd")]:
        del sys.modules[m]
    srcs = sorted(glob.glob(os.path.join(tree, "evcont_amd", "csrc", "*.hip")))
    if sys.argv[3:]:
        srcs = [s for s in srcs if os.path.basename(s) in sys.argv[3:]]

    def asm(src):
        out = os.path.join(tmp, os.path.basename(src) + ".s")
        subprocess.run([b._hipcc(), f"--offload-arch={b.ARCH}", "--offload-device-only", "-S", "-O3", "-std=c++17",
                        "-w"] + b.EXTRA + [src, "-o", out], check=True)
        return open(out).read()

    found = {}
    with ThreadPoolExecutor(8) as ex:
        for text in ex.map(asm, srcs):
            text = re.sub(r"[ \t]*;.*", "", text)                 # comments
            text = re.sub(r"\.L(BB|func_end|tmp)\d+", r".L\1", text)   # label numbering
            text = re.sub(r"(?m)^\s*$\n", "", text)
            for name in re.findall(r"(?m)^\s*\.amdhsa_kernel (\S+)", text):
                body = text.split(f"\n{name}:\n", 1)[1].split("\n.Lfunc_end:", 1)[0]
                body = re.sub(r"(?m)^\s*\.(section|text)\b.*\n?", "", body)   # (a specialisation is no COMDAT: same code)
                desc = text.split(f".amdhsa_kernel {name}\n", 1)[1].split(".end_amdhsa_kernel", 1)[0]
                found[name] = (body, desc)
    return found


def unnumbered(body):
    """the instructions with the register numbers taken out: v12 -> v#, s[4:5] -> s[#2] (the width stays)"""
    body = re.sub(r"\b([sva])\[(\d+):(\d+)\]", lambda m: f"{m[1]}[#{int(m[3]) - int(m[2]) + 1}]", body)
    return re.sub(r"\b([sva])\d+\b", r"\1#", body)


def figures(desc):
    got = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", desc))
    return " ".join(f"{k}={got[k]}" for k in FIGURES if k in got)


with tempfile.TemporaryDirectory() as t0, tempfile.TemporaryDirectory() as t1:
    old, new = kernels(os.path.abspath(sys.argv[1]), t0), kernels(os.path.abspath(sys.argv[2]), t1)
demangle = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip().split("(")[0]
same = renamed = 0
for name in sorted(set(old) | set(new)):
    if name not in old or name not in new:
        print(f"ONLY IN {'OLD' if name in old else 'NEW'}: {demangle(name)}")
    elif old[name] == new[name]:
        same += 1
    elif old[name][1] == new[name][1] and unnumbered(old[name][0]) == unnumbered(new[name][0]):
        renamed += 1
        print(f"identical up to register names: {demangle(name)}")
    else:
        what = [w for w, i in (("instructions", 0), ("descriptor", 1)) if old[name][i] != new[name][i]]
        print(f"DIFFERS ({', '.join(what)}): {demangle(name)}\n   old: {figures(old[name][1])}\n   new: {figures(new[name][1])}")
print(f"identical: {same}, identical up to register names: {renamed}, of {len(set(old) | set(new))} kernels")
