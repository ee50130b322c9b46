"""Diagnostic (build-time): VALU+SALU instructions per H-step of the fast look-ahead rollout
loop for each lane split (LPM 1/2/4) of plan_kernel<RK4, staged, LPM, xref shared> and of the
controller tick's ctl_kernel<LPM> (candidates in LDS, input terms staged: the shortest loop), and of
the NLP kernel's Euler rollout (nlp_kernel<staged>, LPM 4) without and with the corridor term, and of
the corridor look-ahead's rollouts (plan_kernel_corr, RK4 and NLP-Euler) beside their plain counterparts, from
hipcc -S listings of the translation units that hold them.  bench.py's ISSUE_INSTR_PER_STEP holds the plan numbers.
usage: python tools/diag/isa_counts.py [extra hipcc flags, e.g. -DLLAMPC_LEAN_TERMS=7]"""
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
tmp = tempfile.mkdtemp()


def listing(tu):
    out = f"{tmp}/{tu}.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm",
                    "-disable-machine-licm", *sys.argv[1:], f"-I{REPO}/include", f"-I{REPO}/lla-mpc_amd/csrc", "--cuda-device-only",
                    "-S", f"{REPO}/lla-mpc_amd/csrc/{tu}.hip", "-o", out], cwd=tmp, check=True, stderr=subprocess.DEVNULL)
    return open(out).read().split("\n")


def loop_of(asm, pattern, fmin=150, rcp=1, nmin=200, skip=0):
    s = next(i for i, l in enumerate(asm) if re.match(pattern, l))
    # the kernel's end, not its first s_endpgm: a block that ends the program may be laid out
    # ahead of the loop
    e = next(i for i in range(s, len(asm)) if re.match(r"^\.Lfunc_end\d+:", asm[i]))
    body = asm[s:e]
    labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    best, found = None, []
    for i, l in enumerate(body):
        m = re.match(r"^\s+s_(?:cbranch_\w+|branch)\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            seg = body[labels[m.group(1)]:i + 1]
            n = sum(1 for x in seg if re.match(r"^\s+(v_|s_)", x))
            f = sum(1 for x in seg if re.match(r"^\s+v_\w+_f64", x))
            # the rollout step: the innermost loop with the division and most fp64 work
            if sum("v_rcp_f64" in x for x in seg) >= rcp and nmin < n < 2000 and f > fmin:
                found.append((n, seg))
                if best is None or n < best[0]:
                    best = (n, seg)
    # skip: the skip-th shortest such loop instead (the quad kernels hold two fast rollouts: the
    # position quadrature's and, longer, the unsplit one)
    found.sort(key=lambda t: t[0])
    return best if not skip else (found[skip] if skip < len(found) else None)


def report(name, best):
    if best is None:
        print(f"{name}: no rollout loop found")
        return
    n, seg = best
    ops = collections.Counter(re.match(r"^\s+(\S+)", x).group(1) for x in seg if re.match(r"^\s+(v_|s_|ds_|global_|flat_|buffer_|scratch_)", x))
    fp64 = sum(v for k, v in ops.items() if k.endswith("_f64"))
    spill = sum(v for k, v in ops.items() if k.startswith(("v_readlane", "v_writelane", "scratch_")))
    mem = sum(v for k, v in ops.items() if k.startswith(("ds_", "global_", "flat_", "buffer_")))
    print(f"{name}: {n} VALU+SALU per step (fp64 {fp64}, lane moves/spill {spill}, memory {mem})")


asm4 = listing("plan_rk4_l4")
report("plan LPM 4 (staged)", loop_of(asm4, r"^_ZN6llampc11plan_kernelILi0ELb1ELi4ELi0ELb0ELi0E\S+:"))
report("plan LPM 4 (staged), the unsplit rollout", loop_of(asm4, r"^_ZN6llampc11plan_kernelILi0ELb1ELi4ELi0ELb0ELi0E\S+:", skip=1))
asm2 = listing("plan_rk4_l2")
report("plan LPM 2 (staged)", loop_of(asm2, r"^_ZN6llampc11plan_kernelILi0ELb1ELi2ELi0ELb0ELi0E\S+:"))
asm1 = listing("plan_rk4_l1")
report("plan LPM 1 (staged)", loop_of(asm1, r"^_ZN6llampc11plan_kernelILi0ELb1ELi1ELi0ELb0ELi0E\S+:"))
report("plan LPM 1 (work queue, 8 waves)", loop_of(asm1, r"^_ZN6llampc11plan_kernelILi0ELb1ELi1ELi0ELb0ELi2E\S+:"))
# the corridor look-ahead (plan_kernel_corr): the unsplit fast rollout with the corridor term
asmk = listing("plan_corr_rk4")
for lpm in (4, 2, 1):
    report(f"plan corridor LPM {lpm} (staged)", loop_of(asmk, rf"^_ZN6llampc16plan_kernel_corrILi0ELb1ELi{lpm}EEE\S+:"))
asme, asmke = listing("plan_euler"), listing("plan_corr_euler")
for lpm in (4, 2, 1):
    report(f"plan Euler LPM {lpm} (staged)", loop_of(asme, rf"^_ZN6llampc11plan_kernelILi1ELb1ELi{lpm}ELi0ELb0ELi0E\S+:", 60, 2, 100))
    report(f"plan Euler corridor LPM {lpm} (staged)", loop_of(asmke, rf"^_ZN6llampc16plan_kernel_corrILi1ELb1ELi{lpm}EEE\S+:", 60, 2, 100))
asmc = listing("ctl")
for lpm in (4, 2, 1):
    # a whole RK4 step: 4 stages x 2 chains' divisions (the look-back's and the walker's loops
    # divide too)
    report(f"ctl LPM {lpm} (staged inputs)", loop_of(asmc, rf"^_ZN6llampc10ctl_kernelILi{lpm}ELb0EEEvNS_9CtlLaunchE:", 300, 8))
asmn = listing("nlp")
# one Euler step (two divisions: the slip angles'), the staged fast run; the corridor instantiation
# is the one with the NlpCorridor argument
report("nlp Euler LPM 4 (staged, H <= 28)", loop_of(asmn, r"^_ZN6llampc10nlp_kernelILb1ELi512EJEEE\S+:", 60, 2, 100))
report("nlp Euler LPM 4 (staged) + corridor", loop_of(asmn, r"^_ZN6llampc10nlp_kernelILb1ELi512EJNS_11NlpCorridorEEEE\S+:", 60, 2, 100))
report("nlp Euler LPM 4 (unstaged, H > 28)", loop_of(asmn, r"^_ZN6llampc10nlp_kernelILb0ELi256EJEEE\S+:", 60, 2, 100))
report("nlp Euler LPM 4 (unstaged) + corridor", loop_of(asmn, r"^_ZN6llampc10nlp_kernelILb0ELi256EJNS_11NlpCorridorEEEE\S+:", 60, 2, 100))
