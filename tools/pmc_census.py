"""Dynamic instruction census of the fused step kernel from counters-only rocprofv3 passes.

  python tools/pmc_census.py <dir> --steps-per-launch 200 [--out profiles/<name>.json] [--against <other.json>]

<dir> holds one sub-directory per `rocprofv3 --pmc ...` pass of the same bench command (any names);
every counter of the LAST dispatch of env_step_kernel<8, true, 1, false, false, ...> (the timed fused launch,
whichever size caps it was compiled for)
is divided by that pass's SQ_WAVES and by the launch's step count: figures per wave and env step
(a wave runs two envs).  Counters collected in more than one pass are averaged.  --against prints
the difference to an earlier census.
"""
import csv
import glob
import json
import os
import sys
from collections import defaultdict

KERNEL = "env_step_kernel<8, true, 1, false, false"  # (a prefix: the size caps follow from round 9 on)


def _arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def census(d, spl):
    vals = defaultdict(list)
    passes = 0
    for sub in sorted(glob.glob(os.path.join(d, "*"))):
        per = defaultdict(lambda: defaultdict(float))
        for f in glob.glob(os.path.join(sub, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                if KERNEL in r["Kernel_Name"]:
                    per[int(r["Dispatch_Id"])][r["Counter_Name"]] += float(r["Counter_Value"])
        if not per:
            continue
        passes += 1
        last = per[max(per)]
        waves = last.get("SQ_WAVES")
        if not waves:
            raise SystemExit(f"{sub}: pass without SQ_WAVES")
        vals["waves"].append(waves)
        for k, v in last.items():
            if k != "SQ_WAVES":
                vals[k].append(v / waves / spl)
    if not passes:
        raise SystemExit(f"no counter_collection.csv with {KERNEL} under {d}")
    return {k: sum(v) / len(v) for k, v in sorted(vals.items())}


def main():
    spl = int(_arg("--steps-per-launch", 200))
    c = census(sys.argv[1], spl)
    out = {"kernel": KERNEL, "steps_per_launch": spl, "waves": c.pop("waves"), "per_wave_step": c}
    if "SQ_WAVE_CYCLES" in c:
        out["share_of_wave_cycles"] = {k: c[k] / c["SQ_WAVE_CYCLES"] for k in
                                       ("SQ_ACTIVE_INST_ANY", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_WAIT_INST_LDS")
                                       if k in c}
    other = _arg("--against")
    if other:
        o = json.load(open(other))["per_wave_step"]
        out["minus_" + os.path.basename(other)] = {k: c[k] - o[k] for k in c if k in o}
    print(json.dumps(out, indent=1))
    if _arg("--out"):
        json.dump(out, open(_arg("--out"), "w"), indent=1)


if __name__ == "__main__":
    main()
