"""Hazard fillers (s_nop) of the fused flat step kernel by cause, from the asm target's output: for
every s_nop the mnemonic before and after it, nothing more.  Classes:

  trans     the instruction before is a transcendental (v_rcp / v_rsq / v_sqrt / v_exp / v_log /
            v_sin / v_cos): its result is used right after
  dpp       the instruction after reads a just-written VGPR across lanes (v_*_dpp, v_permlane*)
  vcc       a VCC (or SGPR-pair) write by a VALU compare / carry followed by a v_cndmask, v_addc or
            v_div_fmas that reads it
  lane      v_readlane / v_writelane / v_readfirstlane next to a VALU write of the lane or value
  exec      a VALU instruction after an EXEC write by s_* (saveexec, s_mov exec)
  vmem      a global / scratch / flat access whose address or data VGPR was just written (64-bit)
  other     none of the above

  make -C pupperv3-mjx_amd/csrc asm && python tools/nop_classes.py [/tmp/pp3_env.s] [-v]
"""
import re
import sys
from collections import Counter

TRANS = ("v_rcp", "v_rsq", "v_sqrt", "v_exp", "v_log", "v_sin", "v_cos")


def classify(prev, nxt):
    pm, nm = prev.split()[0], nxt.split()[0]
    if pm.startswith(TRANS):
        return "trans"
    if "_dpp" in nm or nm.startswith("v_permlane") or "row_" in nxt or "quad_perm" in nxt:
        return "dpp"
    if nm.startswith(("v_readlane", "v_writelane", "v_readfirstlane")) or pm.startswith(("v_readlane", "v_writelane")):
        return "lane"
    if nm.startswith(("v_cndmask", "v_addc", "v_subb", "v_div_fmas")) or (pm.startswith(("v_cmp", "v_add_co", "v_sub_co"))
                                                                       and nm.startswith("v_")):
        return "vcc"
    if pm.startswith("s_") and "exec" in prev and nm.startswith("v_"):
        return "exec"
    if nm.startswith(("global_", "scratch_", "flat_", "buffer_")):
        return "vmem"
    return "other"


def main(path, verbose):
    s = open(path).read()
    a = re.search(r"^_ZN3pp315env_step_kernelILi8ELb1E(?:Li1E)?(?:Lb0E){0,2}EEv\S*:", s, re.M).start()
    body = [L.strip() for L in s[a:s.index(".Lfunc_end", a)].split("\n")]
    ins = [L for L in body if L and not L.startswith((".", ";")) and not L.endswith(":") and not L.startswith("//")]
    by, pairs = Counter(), Counter()
    for i, L in enumerate(ins):
        if not L.startswith("s_nop") or i == 0 or i + 1 >= len(ins):
            continue
        c = classify(ins[i - 1], ins[i + 1])
        by[(c, L)] += 1
        pairs[(c, ins[i - 1].split()[0], ins[i + 1].split()[0])] += 1
    total = sum(by.values())
    print(f"{total} s_nop among {len(ins)} instructions of the fused flat kernel")
    for c in ("trans", "dpp", "vcc", "lane", "exec", "vmem", "other"):
        row = {k[1]: v for k, v in by.items() if k[0] == c}
        print(f"  {c:6s} {sum(row.values()):4d}   " + "  ".join(f"{k}: {v}" for k, v in sorted(row.items())))
    if verbose:
        for (c, p, n), v in pairs.most_common(40):
            print(f"    {v:4d}  {c:6s} {p} -> {n}")


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if x != "-v"]
    main(args[0] if args else "/tmp/pp3_env.s", "-v" in sys.argv)
