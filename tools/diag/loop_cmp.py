"""Diagnostic (build-time): does a change outside the rollout loops leave them alone?  Extracts the
staged fast rollout loops of one kernel from two hipcc -S listings of the same translation unit
and compares their opcode sequences pairwise, in the kernel's order (operands, i.e. register
names, are ignored).  A rollout loop is an innermost backward-branch span with more than FMIN fp64
instructions and no global-memory access: the staged fast step reads LDS only (the staging loop
and the general re-run load from global memory; the staging's sincos has half as many fp64
instructions).  The headline kernel has two: the position-split quad's (the one
tools/diag/isa_counts.py counts) and the unsplit one.  Exit status 0: same sequences; 1: not.
usage: python tools/diag/loop_cmp.py OLD.s NEW.s [kernel symbol regex]"""
import re
import sys

HEADLINE = r"^_ZN6llampc11plan_kernelILi0ELb1ELi4ELi0ELb0ELi0E\S+:"
FMIN = 300


def kernel_body(path, pattern):
    asm = open(path).read().split("\n")
    s = next(i for i, l in enumerate(asm) if re.match(pattern, l))
    e = next(i for i in range(s, len(asm)) if re.match(r"^\s+\.amdhsa_kernarg_size", asm[i]))
    return asm[s:e]


def rollout_loops(body):
    labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    spans = []
    for i, l in enumerate(body):
        m = re.match(r"^\s+\S+\s+(\.LBB\d+_\d+)\s*$", l)       # a branch: its one operand is a label
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            spans.append((labels[m.group(1)], i))
    loops = []
    for s, e in spans:
        if any((s2, e2) != (s, e) and s <= s2 and e2 <= e for s2, e2 in spans):
            continue                                           # not innermost
        ops = [x.group(1) for y in body[s:e + 1] if (x := re.match(r"^\s+([a-z]\w+)", y))]
        f = sum(o.endswith("_f64") or "_f64_" in o for o in ops)
        if f > FMIN and not any(o.startswith(("global_", "flat_", "buffer_", "scratch_")) for o in ops):
            loops.append(ops)
    return loops


def main():
    old, new = sys.argv[1], sys.argv[2]
    pattern = sys.argv[3] if len(sys.argv) > 3 else HEADLINE
    a, b = rollout_loops(kernel_body(old, pattern)), rollout_loops(kernel_body(new, pattern))
    alu = lambda ops: sum(o.startswith(("v_", "s_")) for o in ops)
    print(f"{old}: {len(a)} rollout loops; {new}: {len(b)}")
    same = len(a) == len(b) and len(a) > 0
    for x, y in zip(a, b):
        if x == y:
            print(f"  {len(x)} instructions ({alu(x)} VALU+SALU): same opcode sequence")
            continue
        same = False
        k = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
        print(f"  {len(x)} ({alu(x)}) / {len(y)} ({alu(y)}) instructions: different from {k}: {x[k:k + 4]} / {y[k:k + 4]}")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
