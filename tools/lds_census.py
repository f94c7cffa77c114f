"""Static census of the LDS reads of one kernel body, per PHASE segment of the prof build's assembly.

  python tools/lds_census.py [asm] [symbol-substring] [--pairs]
      (defaults: /tmp/pp3_prof.s from `make asm-prof`; env_step_kernelILi8ELb1ELi1ELb0E, the fused
       flat kernel; an assembly without PP3PHASE markers, `make asm`, is one segment)

Per segment (a segment is named after the `; PP3PHASE k` marker that CLOSES it; the code after
the last marker is the segment "tail"):
  the LDS reads by form;
  adj: the ds_read2_b32 that fetch two ADJACENT dwords (offset1 = offset0 + 1): 8 contiguous bytes
       per lane, a ds_read_b64 had the address been provably 8-byte aligned (even0: offset0 even);
       likewise adj64 for ds_read2_b64 (16 contiguous bytes, a ds_read_b128);
  rounds: LDS reads retired per `s_waitcnt lgkmcnt` (reads issued since the last such wait minus
       the count the wait leaves outstanding) as size:occurrences; 1:n are single-read rounds.
       (Scalar loads share the counter; they are not counted as reads.)
The "substep" total sums the segments on the substep path (5 per env step): every segment but
ENV_PHASES below, i.e. but those closed by markers 9-12 (env prologue / epilogue) and "tail" (the
code behind the last marker: the step's stores and the loop back).  Only the gfx9 mnemonics
(ds_read*) are counted.
--pairs lists every adjacent-pair ds_read2_b32 with its line in the listing and, where the assembly
carries line tables (add -gline-tables-only to the asm-prof command: the code is the same), the
source line of one of the two fused loads (innermost inlined location first).
"""
import re
import sys
from collections import Counter

ENV_PHASES = ("9", "10", "11", "12", "tail")
FORMS = ("ds_read_b32", "ds_read2_b32", "ds_read_b64", "ds_read2_b64", "ds_read_b96", "ds_read_b128",
         "ds_read2st64_b32", "ds_read2st64_b64")


def segments(body):
    seg = {"ops": Counter(), "adj": 0, "even0": 0, "adj64": 0, "rounds": Counter(), "pairs": []}
    pending = 0
    loc = ""
    for no, line in body:
        t = line.strip()
        if t.startswith(".loc") and ";" in t:
            loc = " ".join(re.findall(r"(\w+\.(?:hip|h):\d+)", t.split(";", 1)[1])[:3])
        m = re.search(r"PP3PHASE (\d+)", t)
        if m:
            yield m.group(1), seg
            seg = {"ops": Counter(), "adj": 0, "even0": 0, "adj64": 0, "rounds": Counter(), "pairs": []}
            continue
        if not t or t.startswith((".", ";")) or t.endswith(":"):
            continue
        op = t.split()[0]
        if op.startswith("ds_read"):
            seg["ops"][op] += 1
            pending += 1
            if op in ("ds_read2_b32", "ds_read2_b64"):
                o0 = re.search(r"offset0:(\d+)", t)
                o1 = re.search(r"offset1:(\d+)", t)
                o0, o1 = int(o0.group(1)) if o0 else 0, int(o1.group(1)) if o1 else 0
                if o1 == o0 + 1:
                    if op == "ds_read2_b32":
                        seg["adj"] += 1
                        seg["even0"] += o0 % 2 == 0
                        seg["pairs"].append((no, t + ("   <- " + loc if loc else "")))
                    else:
                        seg["adj64"] += 1
        elif op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", t)
            if m:
                left = int(m.group(1))
                if pending > left:
                    seg["rounds"][pending - left] += 1
                    pending = left
    yield "tail", seg


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else "/tmp/pp3_prof.s"
    pat = args[1] if len(args) > 1 else "env_step_kernelILi8ELb1ELi1ELb0E"
    lines = open(path).read().split("\n")
    start = next(i for i, L in enumerate(lines) if re.match(r"^_Z\w+:", L) and pat in L)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = list(enumerate(lines[start:end], start + 1))
    n_inst = sum(1 for _, L in body if L.strip() and not L.strip().startswith((".", ";")) and not L.strip().endswith(":"))
    print(f"{lines[start][:-1]}: {n_inst} instructions")
    total = {"ops": Counter(), "adj": 0, "even0": 0, "adj64": 0, "rounds": Counter()}
    sub = {"ops": Counter(), "adj": 0, "even0": 0, "adj64": 0, "rounds": Counter()}
    pairs = []

    def show(name, s):
        forms = " ".join(f"{f[3:]}={s['ops'][f]}" for f in FORMS if s["ops"][f])
        other = sum(v for k, v in s["ops"].items() if k not in FORMS)
        rounds = " ".join(f"{k}:{v}" for k, v in sorted(s["rounds"].items()))
        print(f"{name:>8} | {forms}{' other=%d' % other if other else ''} | adj={s['adj']} (even0={s['even0']}) "
              f"adj64={s['adj64']} | rounds {rounds}")

    for name, s in segments(body):
        show(name, s)
        for acc in (total,) + (() if name in ENV_PHASES else (sub,)):
            acc["ops"] += s["ops"]
            acc["rounds"] += s["rounds"]
            for k in ("adj", "even0", "adj64"):
                acc[k] += s[k]
        pairs += [(name,) + p for p in s["pairs"]]
    show("substep", sub)
    show("total", total)
    if "--pairs" in sys.argv:
        for name, no, t in pairs:
            print(f"  phase {name} line {no}: {t}")


if __name__ == "__main__":
    main()
